"""The model-based TV / Huber super-resolution of csrc/tvsr.hip restated in float64 NumPy: the block operator A, its
adjoint, the forward-difference gradient, the divergence, the objective and the Chambolle-Pock iteration.  Images are the trailing
two axes, leading axes are a batch.  The tests compare the kernels with these functions; nothing here imports the package."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = SIGMA = 1.0 / np.sqrt(8.0)


def block_kernel(kernel, factors):
    """'mean', 'decimate' or an array [f0][f1] -> the float64 block kernel k [f0][f1]."""
    f0, f1 = factors
    if isinstance(kernel, str):
        if kernel == "mean":
            return np.full((f0, f1), 1.0 / (f0 * f1))
        if kernel == "decimate":
            k = np.zeros((f0, f1))
            k[0, 0] = 1.0
            return k
        raise ValueError(kernel)
    k = np.asarray(kernel, np.float64)
    assert k.shape == (f0, f1)
    return k


def apply_A(x, k):
    """(A x)[i, j] = sum_{a, b} k[a, b] x[f0 i + a, f1 j + b]."""
    f0, f1 = k.shape
    H, W = x.shape[-2:]
    blocks = x.reshape(*x.shape[:-2], H // f0, f0, W // f1, f1)
    return np.einsum("...iajb,ab->...ij", blocks, k)


def apply_AT(r, k):
    """A^T r spreads k[a, b] r[i, j] over block (i, j)."""
    f0, f1 = k.shape
    h, w = r.shape[-2:]
    return (r[..., :, None, :, None] * k[:, None, :]).reshape(*r.shape[:-2], h * f0, w * f1)


def grad(x):
    """Forward differences, zero last row / column -> (g0, g1)."""
    g0, g1 = np.zeros_like(x), np.zeros_like(x)
    g0[..., :-1, :] = x[..., 1:, :] - x[..., :-1, :]
    g1[..., :, :-1] = x[..., :, 1:] - x[..., :, :-1]
    return g0, g1


def div(p0, p1):
    """-grad^T: (p0[i] - p0[i-1]) + (p1[j] - p1[j-1]), the missing terms zero; the last row of p0 / column of p1 does not count
    (grad is zero there)."""
    d = np.zeros_like(p0)
    d[..., :-1, :] += p0[..., :-1, :]
    d[..., 1:, :] -= p0[..., :-1, :]
    d[..., :, :-1] += p1[..., :, :-1]
    d[..., :, 1:] -= p1[..., :, :-1]
    return d


def huber(t, alpha):
    if alpha == 0:
        return t
    return np.where(t <= alpha, t * t / (2.0 * alpha), t - alpha / 2.0)


def energy(x, y, k, lam, alpha, w=None):
    """1/2 sum w (A x - y)^2 + lam sum H_alpha(|grad x|), per image."""
    r = apply_A(x, k) - y
    data = 0.5 * ((1.0 if w is None else w) * r * r).sum(axis=(-2, -1))
    if lam == 0:
        return data
    g0, g1 = grad(x)
    return data + lam * huber(np.sqrt(g0 * g0 + g1 * g1), alpha).sum(axis=(-2, -1))


def replicate(y, factors):
    return apply_AT(y, np.ones(factors))


def solve(y, factors, kernel="mean", lam=1e-3, alpha=0.0, n_iter=100, w=None, x0=None, return_info=False):
    """Chambolle-Pock, tau = sigma = 1/sqrt(8), from x = xbar = x0 (default: block replication of y), p = 0."""
    y = np.asarray(y, np.float64)
    k = block_kernel(kernel, factors)
    k2 = (k * k).sum()
    w = np.ones_like(y) if w is None else np.broadcast_to(np.asarray(w, np.float64), y.shape)
    c = TAU * w / (1.0 + TAU * w * k2)
    x = replicate(y, factors) if x0 is None else np.array(x0, np.float64)
    xbar = x.copy()
    p0, p1 = np.zeros_like(x), np.zeros_like(x)
    change = np.zeros(x.shape[:-2])
    for _ in range(n_iter):
        if lam > 0:
            g0, g1 = grad(xbar)
            den = 1.0 + SIGMA * alpha / lam
            p0 = (p0 + SIGMA * g0) / den
            p1 = (p1 + SIGMA * g1) / den
            s = np.maximum(1.0, np.sqrt(p0 * p0 + p1 * p1) / lam)
            p0, p1 = p0 / s, p1 / s
        v = x + TAU * div(p0, p1)
        xn = v - apply_AT(c * (apply_A(v, k) - y), k)
        change = np.abs(xn - x).max(axis=(-2, -1))
        xbar = 2.0 * xn - x
        x = xn
    if return_info:
        return x, energy(x, y, k, lam, alpha, w), change
    return x


# the issue's weighted Huber case: 6 x 10, factors (3, 2), the mean kernel
CASE_FACTORS = (3, 2)
CASE_W = np.array([[1, .5, 2, 1, 0], [1, 1, 1, 3, 1]], np.float64)[None]
CASE_LAM, CASE_ALPHA = 0.05, 0.02


def case_data():
    hr = np.random.default_rng(0).random((1, 6, 10))
    return hr, apply_A(hr, block_kernel("mean", CASE_FACTORS))


def lbfgs_minimum(y, k, lam, alpha, w, shape):
    """The minimum of the Huber energy by L-BFGS-B with the analytic gradient (scipy), independent of the iteration."""
    from scipy.optimize import minimize

    def fun(z):
        x = z.reshape(shape)
        r = (apply_A(x, k) - y) * w
        g0, g1 = grad(x)
        t = np.sqrt(g0 * g0 + g1 * g1)
        scale = np.where(t <= alpha, 1.0 / alpha, 1.0 / np.maximum(t, 1e-300))       # H'(t) / t
        e = 0.5 * (r * (apply_A(x, k) - y)).sum() + lam * huber(t, alpha).sum()
        return e, (apply_AT(r, k) - lam * div(scale * g0, scale * g1)).ravel()

    z = replicate(y, k.shape).ravel()
    for _ in range(5):                                                                # restarts: the memory is rebuilt at the iterate
        res = minimize(fun, z, jac=True, method="L-BFGS-B", options={"maxiter": 20000, "maxfun": 200000, "ftol": 0, "gtol": 1e-14,
                                                                     "maxcor": 50})
        z = res.x
    return float(res.fun)


def pat07_roi(r0=40, r1=90):
    """tests/golden/pat07_volume.npz, ROI r0:r1, as [Z, R, R] float64 in [0, 1]."""
    vol = np.load(os.path.join(ROOT, "tests", "golden", "pat07_volume.npz"))["vol"][r0:r1, r0:r1].astype(np.float64)
    return np.ascontiguousarray((vol / vol.max()).transpose(2, 0, 1))


def psnr(a, b, data_range=1.0):
    return 10.0 * np.log10(data_range ** 2 / np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
