"""The channel-coupled (vectorial) TV / Huber super-resolution of csrc/tvj.hip restated in float64 NumPy, on the
operators of tests/tvsr_common.py.  A group is [..., C, H, W]: the third axis from the end is the channel axis, leading axes are a
batch of groups.  The tests compare the kernel with these functions; nothing here imports the package."""
import numpy as np

from tests import tvsr_common as T

TAU = SIGMA = T.TAU


def _mu(channel_weights, C, dtype=np.float64):
    mu = np.ones(C, dtype) if channel_weights is None else np.asarray(channel_weights, dtype)
    assert mu.shape == (C,) and (mu >= 0).all() and (mu <= 1).all()
    return mu[:, None, None]


def energy_joint(x, y, k, lam, alpha, w=None, channel_weights=None, coupling="joint"):
    """1/2 sum_c sum w (A x_c - y_c)^2 + lam sum H_alpha(sqrt(sum_c mu_c^2 |grad x_c|^2)) per group ('none': the norm per channel)."""
    r = T.apply_A(x, k) - y
    data = 0.5 * ((1.0 if w is None else w) * r * r).sum(axis=(-3, -2, -1))
    if lam == 0:
        return data
    mu = _mu(channel_weights, x.shape[-3], x.dtype)
    g0, g1 = T.grad(x)
    g0, g1 = mu * g0, mu * g1
    sq = g0 * g0 + g1 * g1
    if coupling == "joint":
        return data + lam * T.huber(np.sqrt(sq.sum(axis=-3)), alpha).sum(axis=(-2, -1))
    return data + lam * T.huber(np.sqrt(sq), alpha).sum(axis=(-3, -2, -1))


def solve_joint(y, factors, kernel="mean", lam=1e-3, alpha=0.0, n_iter=100, channel_weights=None, coupling="joint", w=None, x0=None,
                return_info=False, dtype=np.float64):
    """Chambolle-Pock, tau = sigma = 1/sqrt(8), from x = xbar = x0 (default: block replication of y), p = 0; the expressions of
    tvsr_common.solve with the products by mu_c placed as csrc/tvj.hip places them.  ``dtype``: np.longdouble runs the same
    iteration in extended precision."""
    assert coupling in ("joint", "none")
    y = np.asarray(y, dtype)
    C = y.shape[-3]
    k = T.block_kernel(kernel, factors).astype(dtype)
    k2 = (k * k).sum()
    mu = _mu(channel_weights, C, dtype)
    tau = sigma = dtype(1.0) / np.sqrt(dtype(8.0))
    lam, alpha = dtype(lam), dtype(alpha)
    w = np.ones_like(y) if w is None else np.broadcast_to(np.asarray(w, dtype), y.shape)
    c = tau * w / (1.0 + tau * w * k2)
    yd = np.where(w == 0, 0.0, y)                                          # w = 0: the datum is never read
    x = T.replicate(y, factors) if x0 is None else np.array(x0, dtype)
    xbar = x.copy()
    p0, p1 = np.zeros_like(x), np.zeros_like(x)
    change = np.zeros(x.shape[:-3], dtype)
    for _ in range(n_iter):
        if lam > 0:
            g0, g1 = T.grad(xbar)
            den = 1.0 + sigma * alpha / lam
            p0 = (p0 + sigma * (mu * g0)) / den
            p1 = (p1 + sigma * (mu * g1)) / den
            sq = p0 * p0 + p1 * p1
            if coupling == "joint":
                total = sq[..., 0, :, :].copy()
                for ch in range(1, C):                                      # ascending c
                    total = total + sq[..., ch, :, :]
                n = (np.sqrt(total) / lam)[..., None, :, :]
            else:
                n = np.sqrt(sq) / lam
            s = np.where(n > 1.0, n, 1.0)
            p0, p1 = p0 / s, p1 / s
        v = x + tau * (mu * T.div(p0, p1))
        xn = v - T.apply_AT(c * (T.apply_A(v, k) - yd), k)
        change = np.abs(xn - x).max(axis=(-3, -2, -1))
        xbar = 2.0 * xn - x
        x = xn
    if return_info:
        return x, energy_joint(x, yd, k, lam, alpha, w, channel_weights, coupling), change
    return x


# the weighted 3-channel case: 6 x 10, factors (3, 2), the mean kernel, mu = (1, 0.5, 0.25), one w = 0
CASE_FACTORS = T.CASE_FACTORS
CASE_MU = (1.0, 0.5, 0.25)
CASE_LAM, CASE_ALPHA = T.CASE_LAM, T.CASE_ALPHA


def case_data():
    """-> (hr [1, 3, 6, 10], y [1, 3, 2, 5], w [1, 3, 2, 5] with exactly one zero)."""
    rng = np.random.default_rng(0)
    base = rng.random((1, 1, 6, 10))
    hr = base * np.array([1.0, 0.6, 0.3])[None, :, None, None] + 0.05 * rng.random((1, 3, 6, 10))
    w = np.stack([T.CASE_W[0], np.ones((2, 5)), np.array([[2, 1, 1, .5, 1], [1, 1, 3, 1, 1]], np.float64)])[None]
    return hr, T.apply_A(hr, T.block_kernel("mean", CASE_FACTORS)), w


def lbfgs_minimum_joint(y, k, lam, alpha, w, channel_weights, shape):
    """The minimum of the COUPLED Huber energy by L-BFGS-B with its analytic gradient (scipy), independent of the iteration."""
    from scipy.optimize import minimize

    mu = _mu(channel_weights, shape[-3])

    def fun(z):
        x = z.reshape(shape)
        res = T.apply_A(x, k) - y
        r = res * w
        g0, g1 = T.grad(x)
        g0, g1 = mu * g0, mu * g1
        t = np.sqrt((g0 * g0 + g1 * g1).sum(axis=-3, keepdims=True))
        scale = np.where(t <= alpha, 1.0 / alpha, 1.0 / np.maximum(t, 1e-300))       # H'(t) / t
        e = 0.5 * (r * res).sum() + lam * T.huber(t, alpha).sum()
        return e, (T.apply_AT(r, k) - lam * mu * T.div(scale * g0, scale * g1)).ravel()

    z = T.replicate(np.where(w == 0, 0.0, y), k.shape).ravel()
    for _ in range(5):                                                                # restarts: the memory is rebuilt at the iterate
        res = minimize(fun, z, jac=True, method="L-BFGS-B", options={"maxiter": 20000, "maxfun": 200000, "ftol": 0, "gtol": 1e-14,
                                                                     "maxcor": 50})
        z = res.x
    return float(res.fun)


# the study case: pat07 slices 10 / 14 / 18, ROI 40:90, a synthetic mono-exponential decay over four b-values, 2 x 2 block means
STUDY_B = np.array([0.0, 150.0, 1000.0, 1500.0])
STUDY_SLICES = (10, 14, 18)
STUDY_NOISE, STUDY_LAM, STUDY_HUBER, STUDY_ITERS = 0.02, 0.024, 0.03, 300


def synthetic_decay(roi, b=STUDY_B):
    """[Z, R, R] in [0, 1] -> (hr [Z, B, R, R], adc [Z, R, R]): ADC high where the smoothed image is dark."""
    from scipy.ndimage import gaussian_filter
    adc = 0.6e-3 + 1.8e-3 * (1 - np.clip(gaussian_filter(roi, (0, 1, 1)) / roi.max(), 0, 1))
    return roi[:, None] * np.exp(-b[None, :, None, None] * adc[:, None]), adc


def study_case(seed):
    """-> (hr [3, 4, 50, 50], y [3, 4, 25, 25], b [4]); the noise is the first draw of default_rng(seed)."""
    roi = T.pat07_roi()[list(STUDY_SLICES)]
    hr, _ = synthetic_decay(roi)
    y = T.apply_A(hr, T.block_kernel("mean", (2, 2))) + STUDY_NOISE * np.random.default_rng(seed).standard_normal((3, 4, 25, 25))
    return hr, y, STUDY_B


def adc_loglinear(x, b=STUDY_B):
    """ADC [..., H, W] of x [..., B, H, W] by log-linear least squares on clip(x, 1e-3): minus the slope of log x over b."""
    logs = np.log(np.clip(x, 1e-3, None))
    bc = b - b.mean()
    return -(bc[:, None, None] * logs).sum(axis=-3) / (bc * bc).sum()


def study_scores(x, hr, b=STUDY_B):
    """-> (PSNR of the last b-value, PSNR over all channels, ADC RMSE inside b0 > 0.25 max(b0))."""
    mask = hr[:, 0] > 0.25 * hr[:, 0].max()
    err = (adc_loglinear(x, b) - adc_loglinear(hr, b))[mask]
    return T.psnr(hr[:, -1], x[:, -1]), T.psnr(hr, x), float(np.sqrt(np.mean(err * err)))
