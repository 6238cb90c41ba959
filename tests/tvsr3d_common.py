"""The 3-D TV / Huber super-resolution of csrc/tvsr3d.hip restated in float64 NumPy: the separable block operator A
with its slice profile, its adjoint, the weighted forward-difference gradient, the divergence, the objective and the Chambolle-Pock
iteration.  Volumes are the trailing three axes (slice, row, column), leading axes are a batch.  The order of operations is the
kernels': wherever the 2-D restatement (tests/tvsr_common.py) combines its two axes, this one combines row, column, then slice, so
with one slice or g0 = 0 it computes the bits of the 2-D restatement.  Nothing here imports the package."""
import numpy as np

from tests import tvsr_common as T2

pat07_roi, psnr, huber = T2.pat07_roi, T2.psnr, T2.huber


def slice_profile(f, kind="mean", fwhm=None):
    """k0 [f]: 'mean', 'decimate', or a Gaussian of `fwhm` thick slices sampled at the f sub-slice centres, normalised to sum 1."""
    if kind == "mean":
        return np.full(f, 1.0 / f)
    if kind == "decimate":
        k = np.zeros(f)
        k[0] = 1.0
        return k
    if kind == "gaussian":
        sigma = fwhm / (2.0 * np.sqrt(2.0 * np.log(2.0)))
        k = np.exp(-0.5 * (((2.0 * np.arange(f) + 1.0 - f) / (2.0 * f)) / sigma) ** 2)
        return k / k.sum()
    raise ValueError(kind)


def block_factors(kernel, factors):
    """'mean', 'decimate' or a triple of 1-D arrays -> the float64 factors (k0 [f0], k1 [f1], k2 [f2])."""
    if isinstance(kernel, str):
        return tuple(slice_profile(f, kernel) for f in factors)
    ks = tuple(np.asarray(k, np.float64) for k in kernel)
    assert tuple(k.shape for k in ks) == tuple((f,) for f in factors)
    return ks


def block_table(ks):
    """k[a][b][c] = (k1[b] * k2[c]) * k0[a]."""
    k0, k1, k2 = ks
    return (k1[None, :, None] * k2[None, None, :]) * k0[:, None, None]


def table_sq(k):
    """sum k^2 over the table in memory order."""
    s = 0.0
    for v in k.ravel():
        s += v * v
    return s


def apply_A(x, k):
    """(A x)[l, i, j] = sum_{a, b, c} k[a, b, c] x[f0 l + a, f1 i + b, f2 j + c]: the sub-slices a in ascending order, each one's
    in-plane sum by the 2-D restatement's apply_A with the table k[a] -- so one sub-slice (f0 = 1) IS the 2-D restatement, bit for
    bit.  (The kernels add every term in ascending (a, b, c); NumPy's einsum does not promise that order in-plane, which moves the
    last bits only.)"""
    f0 = k.shape[0]
    acc = 0.0
    for a in range(f0):
        acc = acc + T2.apply_A(x[..., a::f0, :, :], k[a])
    return acc


def apply_AT(r, k):
    """A^T r spreads k[a, b, c] r[l, i, j] over block (l, i, j)."""
    f = k.shape
    d, h, w = r.shape[-3:]
    out = r[..., :, None, :, None, :, None] * k[:, None, :, None, :]
    return out.reshape(*r.shape[:-3], d * f[0], h * f[1], w * f[2])


def diffs(x):
    """Forward differences with a zero last plane / row / column -> (d0, d1, d2) along slice, row, column, unweighted."""
    d0, d1, d2 = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    d0[..., :-1, :, :] = x[..., 1:, :, :] - x[..., :-1, :, :]
    d1[..., :, :-1, :] = x[..., :, 1:, :] - x[..., :, :-1, :]
    d2[..., :, :, :-1] = x[..., :, :, 1:] - x[..., :, :, :-1]
    return d0, d1, d2


def grad(x, g=(1.0, 1.0, 1.0)):
    d0, d1, d2 = diffs(x)
    return g[0] * d0, g[1] * d1, g[2] * d2


def div(p0, p1, p2, g=(1.0, 1.0, 1.0)):
    """-grad^T: + g1 p1[e] - g1 p1[e - W] + g2 p2[e] - g2 p2[e - 1], then + g0 p0[e] - g0 p0[e - HW]; the last plane of p0, row of
    p1 and column of p2 do not count (grad is zero there)."""
    d = np.zeros_like(p0)
    d[..., :, :-1, :] += g[1] * p1[..., :, :-1, :]
    d[..., :, 1:, :] -= g[1] * p1[..., :, :-1, :]
    d[..., :, :, :-1] += g[2] * p2[..., :, :, :-1]
    d[..., :, :, 1:] -= g[2] * p2[..., :, :, :-1]
    d[..., :-1, :, :] += g[0] * p0[..., :-1, :, :]
    d[..., 1:, :, :] -= g[0] * p0[..., :-1, :, :]
    return d


def step(shape, g, lam):
    """(tau = sigma, the lambda in force): 1 / sqrt(4 sum g_a^2) in the order (1, 2, 0) over the axes longer than 1; a zero sum
    switches the prior off."""
    D, H, W = shape[-3:]
    s = 0.0
    if H > 1:
        s += g[1] * g[1]
    if W > 1:
        s += g[2] * g[2]
    if D > 1:
        s += g[0] * g[0]
    if s == 0.0:
        return 1.0 / np.sqrt(8.0), 0.0
    return 1.0 / np.sqrt(4.0 * s), lam


def energy(x, y, k, lam, alpha, w=None, g=(1.0, 1.0, 1.0)):
    """1/2 sum w (A x - y)^2 + lam sum H_alpha(sqrt((g1 d1 x)^2 + (g2 d2 x)^2 + (g0 d0 x)^2)), per volume."""
    r = apply_A(x, k) - y
    data = 0.5 * ((1.0 if w is None else w) * r * r).sum(axis=(-3, -2, -1))
    _, lam = step(x.shape, g, lam)
    if lam == 0:
        return data
    t0, t1, t2 = grad(x, g)
    return data + lam * huber(np.sqrt((t1 * t1 + t2 * t2) + t0 * t0), alpha).sum(axis=(-3, -2, -1))


def replicate(y, factors):
    return apply_AT(y, np.ones(factors))


def solve(y, factors, kernel="mean", lam=1e-3, alpha=0.0, n_iter=100, g=(1.0, 1.0, 1.0), w=None, x0=None, return_info=False):
    """Chambolle-Pock as tests/tvsr_common.solve states it, from x = xbar = x0 (default: block replication of y), p = 0."""
    y = np.asarray(y, np.float64)
    k = block_table(block_factors(kernel, factors))
    k2 = table_sq(k)
    w = np.ones_like(y) if w is None else np.broadcast_to(np.asarray(w, np.float64), y.shape)
    x = replicate(y, factors) if x0 is None else np.array(x0, np.float64)
    tau, lam_on = step(x.shape, g, lam)
    sigma = tau
    c = tau * w / (1.0 + tau * w * k2)
    xbar = x.copy()
    p0, p1, p2 = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    change = np.zeros(x.shape[:-3])
    for _ in range(n_iter):
        if lam_on > 0:
            d0, d1, d2 = diffs(xbar)
            den = 1.0 + sigma * alpha / lam_on
            p1 = (p1 + sigma * (g[1] * d1)) / den
            p2 = (p2 + sigma * (g[2] * d2)) / den
            p0 = (p0 + sigma * (g[0] * d0)) / den
            s = np.maximum(1.0, np.sqrt((p1 * p1 + p2 * p2) + p0 * p0) / lam_on)
            p0, p1, p2 = p0 / s, p1 / s, p2 / s
        v = x + tau * div(p0, p1, p2, g)
        xn = v - apply_AT(c * (apply_A(v, k) - y), k)
        change = np.abs(xn - x).max(axis=(-3, -2, -1))
        xbar = 2.0 * xn - x
        x = xn
    if return_info:
        return x, energy(x, y, k, lam, alpha, w, g), change
    return x


# the issue's weighted Huber case: 4 x 6 x 6, factors (2, 3, 2), kernels ([.25, .75], mean, [.2, .8]), weights in [0.5, 1.5) with one zero
CASE_FACTORS = (2, 3, 2)
CASE_KERNEL = (np.array([0.25, 0.75]), np.full(3, 1.0 / 3.0), np.array([0.2, 0.8]))
CASE_LAM, CASE_ALPHA = 0.05, 0.02
CASE_GRAD_WEIGHTS = ((1.0, 1.0, 1.0), (0.4, 1.0, 1.0))


def case_data():
    """-> (hr [1, 4, 6, 6], y [1, 2, 2, 3], w [1, 2, 2, 3])."""
    rng = np.random.default_rng(0)
    hr = rng.random((1, 4, 6, 6))
    w = 0.5 + rng.random((1, 2, 2, 3))
    w[0, 1, 0, 2] = 0.0
    return hr, apply_A(hr, block_table(CASE_KERNEL)), w


def lbfgs_minimum(y, k, lam, alpha, w, shape, g=(1.0, 1.0, 1.0)):
    """The minimum of the Huber energy by L-BFGS-B with the analytic gradient (scipy), independent of the iteration."""
    from scipy.optimize import minimize

    def fun(z):
        x = z.reshape(shape)
        r = (apply_A(x, k) - y) * w
        t0, t1, t2 = grad(x, g)
        t = np.sqrt(t0 * t0 + t1 * t1 + t2 * t2)
        scale = np.where(t <= alpha, 1.0 / alpha, 1.0 / np.maximum(t, 1e-300))       # H'(t) / t
        e = 0.5 * (r * (apply_A(x, k) - y)).sum() + lam * huber(t, alpha).sum()
        return e, (apply_AT(r, k) - lam * div(scale * t0, scale * t1, scale * t2, g)).ravel()

    z = replicate(y, k.shape).ravel()
    for _ in range(5):                                                                # restarts: the memory is rebuilt at the iterate
        res = minimize(fun, z, jac=True, method="L-BFGS-B", options={"maxiter": 20000, "maxfun": 200000, "ftol": 0, "gtol": 1e-14,
                                                                     "maxcor": 50})
        z = res.x
    return float(res.fun)
