"""The model-based S0 / ADC super-resolution of csrc/tvadc.hip restated in float64 NumPy, on the operators of
tests/tvsr_common.py: the unknowns are the two parameter maps s (the b = 0 signal) and d (the ADC) of the mono-exponential model
x_c = s exp(-b_c d), under the block operator A and a Huber-TV prior on the two maps.  A group of data is [..., C, h, w], the maps are
[..., H, W].  The tests compare the kernel with these functions; nothing here imports the package."""
import functools

import numpy as np

from tests import tvj_common as J
from tests import tvsr_common as T


def normalise(b, s_max, adc_max, adc0, k):
    """What the host side of the entry point forms, in float64: (beta [C], b_max, u_max, u0, tau) with u = d b_max the normalised
    ADC and tau = sigma = 1 / sqrt(8 + c_A L2), c_A = (sum |k|)(max |k|), L2 = sum_c (1 + beta_c^2 s_max^2) in ascending c."""
    b = np.asarray(b, np.float64)
    b_max = float(b.max())
    beta = b / b_max
    l2 = 0.0
    for bc in beta:
        l2 += 1.0 + bc * bc * (s_max * s_max)
    c_a = float(np.abs(k).sum() * np.abs(k).max())
    return beta, b_max, adc_max * b_max, adc0 * b_max, 1.0 / np.sqrt(8.0 + c_a * l2)


def _mu(map_weights, dtype):
    mu = np.asarray(map_weights, dtype)
    assert mu.shape == (2,) and (mu >= 0).all() and (mu <= 1).all()
    return mu


def model(s, u, beta):
    """[..., H, W] maps -> the model's images [..., C, H, W]: s exp(-(beta_c u))."""
    return s[..., None, :, :] * np.exp(-(beta[:, None, None] * u[..., None, :, :]))


def energy_adc(s, u, beta, y, k, lam, alpha, w=None, map_weights=(1.0, 1.0), coupling="joint"):
    """1/2 sum_c sum w (A (s exp(-beta_c u)) - y_c)^2 + lam R(s, u) per group; R: H_alpha of the coupled norm sqrt(mu_s^2 |grad s|^2 +
    mu_u^2 |grad u|^2) ('none': one term per map)."""
    r = T.apply_A(model(s, u, np.asarray(beta, s.dtype)), k) - y
    data = 0.5 * ((1.0 if w is None else w) * r * r).sum(axis=(-3, -2, -1))
    if lam == 0:
        return data
    mu = _mu(map_weights, s.dtype)
    sq = []
    for m, field in zip(mu, (s, u)):
        g0, g1 = T.grad(field)
        g0, g1 = m * g0, m * g1
        sq.append(g0 * g0 + g1 * g1)
    if coupling == "joint":
        return data + lam * T.huber(np.sqrt(sq[0] + sq[1]), alpha).sum(axis=(-2, -1))
    return data + lam * (T.huber(np.sqrt(sq[0]), alpha) + T.huber(np.sqrt(sq[1]), alpha)).sum(axis=(-2, -1))


def start(y, b, factors, s_max, adc_max, adc0, x0=None, dtype=np.float64):
    """The start (s, u) in the box: the given maps x0 = (s0, adc), or the block replication of the first channel of smallest b and
    u = adc0 b_max everywhere, each through fmin(fmax(., 0), top)."""
    b = np.asarray(b, np.float64)
    b_max = float(b.max())
    u_max = adc_max * b_max
    if x0 is not None:
        s, u = np.array(x0[0], dtype), np.array(x0[1], dtype) * dtype(b_max)
    else:
        s = T.replicate(np.asarray(y, dtype)[..., int(np.argmin(b)), :, :], factors)
        u = np.full(s.shape, adc0 * b_max, dtype)
    return np.fmin(np.fmax(s, 0.0), dtype(s_max)), np.fmin(np.fmax(u, 0.0), dtype(u_max))


def solve_adc(y, b, factors, kernel="mean", lam=5e-3, alpha=0.01, n_iter=100, map_weights=(1.0, 0.1), coupling="joint", s_max=1.5,
              adc_max=4e-3, adc0=1e-3, w=None, x0=None, return_info=False, dtype=np.float64):
    """The exact nonlinear primal-dual iteration of csrc/tvadc.hip (Valkonen 2014) in its expression order, from the start of
    ``start``, p = 0, z = 0.  -> (s, adc) and, with ``return_info``, the objective at the result and max(|s' - s|, |u' - u|) of the
    last iteration.  ``dtype``: np.longdouble runs the same iteration in extended precision (the normalisation stays the host's)."""
    assert coupling in ("joint", "none")
    y = np.asarray(y, dtype)
    k = T.block_kernel(kernel, factors)
    beta64, b_max, u_max, _, tau64 = normalise(b, s_max, adc_max, adc0, k)
    k = k.astype(dtype)
    beta = beta64.astype(dtype)[:, None, None]
    tau = sigma = dtype(tau64)
    lam, alpha, s_top, u_top = dtype(lam), dtype(alpha), dtype(s_max), dtype(u_max)
    mu = _mu(map_weights, dtype)
    w = np.ones_like(y) if w is None else np.broadcast_to(np.asarray(w, dtype), y.shape)
    missing = w == 0
    wd = np.where(missing, 1.0, w)
    yd = np.where(missing, 0.0, y)                                         # w = 0: the datum is never read
    s, u = start(y, b, factors, s_max, adc_max, adc0, x0, dtype)
    sbar, ubar = s.copy(), u.copy()
    ps0, ps1, pu0, pu1 = (np.zeros_like(s) for _ in range(4))
    z = np.zeros_like(y)
    change = np.zeros(s.shape[:-2], dtype)
    for _ in range(n_iter):
        if lam > 0:
            den = 1.0 + sigma * alpha / lam
            gs0, gs1 = T.grad(sbar)
            gu0, gu1 = T.grad(ubar)
            ps0, ps1 = (ps0 + sigma * (mu[0] * gs0)) / den, (ps1 + sigma * (mu[0] * gs1)) / den
            pu0, pu1 = (pu0 + sigma * (mu[1] * gu0)) / den, (pu1 + sigma * (mu[1] * gu1)) / den
            sq_s, sq_u = ps0 * ps0 + ps1 * ps1, pu0 * pu0 + pu1 * pu1
            if coupling == "joint":
                n_s = n_u = np.sqrt(sq_s + sq_u) / lam
            else:
                n_s, n_u = np.sqrt(sq_s) / lam, np.sqrt(sq_u) / lam
            n_s, n_u = np.where(n_s > 1.0, n_s, 1.0), np.where(n_u > 1.0, n_u, 1.0)
            ps0, ps1, pu0, pu1 = ps0 / n_s, ps1 / n_s, pu0 / n_u, pu1 / n_u
        r = T.apply_A(sbar[..., None, :, :] * np.exp(-(beta * ubar[..., None, :, :])), k) - yd
        z = np.where(missing, 0.0, (z + sigma * r) / (1.0 + sigma / wd))
        # ---- barrier 1
        e = np.exp(-(beta * u[..., None, :, :]))
        kz = T.apply_AT(z, k)
        g_s, g_u = np.zeros_like(s), np.zeros_like(u)
        for c in range(y.shape[-3]):                                       # ascending c
            g_s = g_s + e[..., c, :, :] * kz[..., c, :, :]
            g_u = g_u + (-(beta[c] * s) * e[..., c, :, :]) * kz[..., c, :, :]
        g_s = g_s - mu[0] * T.div(ps0, ps1)
        g_u = g_u - mu[1] * T.div(pu0, pu1)
        sn = np.fmin(np.fmax(s - tau * g_s, 0.0), s_top)
        un = np.fmin(np.fmax(u - tau * g_u, 0.0), u_top)
        change = np.maximum(np.abs(sn - s).max(axis=(-2, -1)), np.abs(un - u).max(axis=(-2, -1)))
        sbar, ubar = 2.0 * sn - s, 2.0 * un - u
        s, u = sn, un
        # ---- barrier 2
    adc = u / dtype(b_max)
    if return_info:
        return s, adc, energy_adc(s, u, beta64, yd, k, lam, alpha, w, map_weights, coupling), change
    return s, adc


# ---- the small case: HR 6 x 10, factors (3, 2), the mean kernel, beta = (0, 0.4, 1), one w = 0 and a few w != 1 -----------------------
CASE_FACTORS = (3, 2)
CASE_B = np.array([0.0, 400.0, 1000.0])
CASE_LAM, CASE_ALPHA, CASE_MU = 0.02, 0.01, (1.0, 0.1)
CASE_SMAX, CASE_ADCMAX, CASE_ADC0, CASE_NOISE = 1.5, 6e-3, 1e-3, 0.02


def case_data():
    """-> (s [1, 6, 10] in [0.2, 1], u [1, 6, 10] in [0.5, 3], y [1, 3, 2, 5] with noise 0.02, w [1, 3, 2, 5] with exactly one zero)."""
    rng = np.random.default_rng(0)
    s = 0.2 + 0.8 * rng.random((1, 6, 10))
    u = 0.5 + 2.5 * rng.random((1, 6, 10))
    y = T.apply_A(model(s, u, CASE_B / CASE_B.max()), T.block_kernel("mean", CASE_FACTORS)) + CASE_NOISE * rng.standard_normal((1, 3, 2, 5))
    return s, u, y, J.case_data()[2]


def case_solve(n_iter, coupling="joint", dtype=np.float64, **kw):
    _, _, y, w = case_data()
    return solve_adc(y, CASE_B, CASE_FACTORS, "mean", CASE_LAM, CASE_ALPHA, n_iter, CASE_MU, coupling, CASE_SMAX, CASE_ADCMAX, CASE_ADC0,
                     w=w, return_info=True, dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def case_minimum(coupling="joint"):
    """-> (E*, the four minima): bounded L-BFGS-B on the small case from the solver's start and from three random starts in the box."""
    _, _, y, w = case_data()
    k = T.block_kernel("mean", CASE_FACTORS)
    first = start(y, CASE_B, CASE_FACTORS, CASE_SMAX, CASE_ADCMAX, CASE_ADC0)
    rng = np.random.default_rng(1)
    u_max = CASE_ADCMAX * CASE_B.max()
    starts = [first] + [(CASE_SMAX * rng.random(first[0].shape), u_max * rng.random(first[0].shape)) for _ in range(3)]
    minima = [lbfgs_minimum_adc(y, CASE_B, k, CASE_LAM, CASE_ALPHA, w, CASE_MU, CASE_SMAX, CASE_ADCMAX, s0, coupling) for s0 in starts]
    return min(minima), minima


def objective_and_gradient(s, u, beta, y, k, lam, alpha, w, map_weights, coupling="joint"):
    """The restated objective of ONE group and its analytic gradient with respect to (s, u): the data term through the Jacobian of the
    model, the prior through H'(t) / t; y holds 0 where w = 0."""
    beta = np.asarray(beta, np.float64)[:, None, None]
    mu = _mu(map_weights, np.float64)
    e = np.exp(-(beta * u[..., None, :, :]))
    res = T.apply_A(s[..., None, :, :] * e, k) - y
    back = T.apply_AT(w * res, k)
    g_s = (e * back).sum(axis=-3)
    g_u = (-(beta * s[..., None, :, :]) * e * back).sum(axis=-3)
    value = 0.5 * (w * res * res).sum()
    if lam > 0:
        gs0, gs1 = (mu[0] * g for g in T.grad(s))
        gu0, gu1 = (mu[1] * g for g in T.grad(u))
        if coupling == "joint":
            t_s = t_u = np.sqrt(gs0 * gs0 + gs1 * gs1 + gu0 * gu0 + gu1 * gu1)
            value = value + lam * T.huber(t_s, alpha).sum()
        else:
            t_s, t_u = np.sqrt(gs0 * gs0 + gs1 * gs1), np.sqrt(gu0 * gu0 + gu1 * gu1)
            value = value + lam * (T.huber(t_s, alpha).sum() + T.huber(t_u, alpha).sum())
        scale = lambda t: np.where(t <= alpha, 1.0 / alpha, 1.0 / np.maximum(t, 1e-300))       # H'(t) / t
        g_s = g_s - lam * mu[0] * T.div(scale(t_s) * gs0, scale(t_s) * gs1)
        g_u = g_u - lam * mu[1] * T.div(scale(t_u) * gu0, scale(t_u) * gu1)
    return float(value), g_s, g_u


def lbfgs_minimum_adc(y, b, k, lam, alpha, w, map_weights, s_max, adc_max, start_su, coupling="joint"):
    """The minimum of the restated objective over the box by bounded L-BFGS-B with the analytic gradient (scipy), five restarts as in
    tvj_common.lbfgs_minimum_joint, from ``start_su`` = (s, u): independent of the iteration."""
    from scipy.optimize import minimize

    beta, _, u_max, _, _ = normalise(b, s_max, adc_max, 0.0, k)
    yd = np.where(w == 0, 0.0, y)
    shape = start_su[0].shape
    half = start_su[0].size

    def fun(v):
        value, g_s, g_u = objective_and_gradient(v[:half].reshape(shape), v[half:].reshape(shape), beta, yd, k, lam, alpha, w, map_weights,
                                                 coupling)
        return value, np.concatenate([g_s.ravel(), g_u.ravel()])

    v = np.concatenate([start_su[0].ravel(), start_su[1].ravel()]).astype(np.float64)
    bounds = [(0.0, s_max)] * half + [(0.0, u_max)] * half
    for _ in range(5):                                                                # restarts: the memory is rebuilt at the iterate
        res = minimize(fun, v, jac=True, method="L-BFGS-B", bounds=bounds,
                       options={"maxiter": 20000, "maxfun": 200000, "ftol": 0, "gtol": 1e-14, "maxcor": 50})
        v = res.x
    return float(res.fun)


# ---- the study case of tests/tvj_common.py with the maps as the truth -----------------------------------------------------------------
STUDY_B = J.STUDY_B
STUDY_FACTORS = (2, 2)


def study_truth():
    """-> (hr [3, 4, 50, 50], s [3, 50, 50], adc [3, 50, 50]) of tvj_common.study_case."""
    roi = T.pat07_roi()[list(J.STUDY_SLICES)]
    hr, adc = J.synthetic_decay(roi)
    return hr, roi, adc


def study_mask(hr):
    return hr[:, 0] > 0.25 * hr[:, 0].max()


def map_scores(s, adc, hr, adc_true):
    """-> (PSNR of the b = 0 image, PSNR of the last b-value of the model's images, RMSE of the solver's ADC map inside the study
    mask)."""
    images = model(s, adc, STUDY_B)
    err = (adc - adc_true)[study_mask(hr)]
    return T.psnr(hr[:, 0], images[:, 0]), T.psnr(hr[:, -1], images[:, -1]), float(np.sqrt(np.mean(err * err)))


def image_scores(x, hr, adc_true):
    """The same three of reconstructed images x [3, 4, 50, 50], the ADC by the clipped log-linear fit against the TRUE map."""
    err = (J.adc_loglinear(x, STUDY_B) - adc_true)[study_mask(hr)]
    return T.psnr(hr[:, 0], x[:, 0]), T.psnr(hr[:, -1], x[:, -1]), float(np.sqrt(np.mean(err * err)))
