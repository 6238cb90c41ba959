"""The TV / Huber super-resolution under a dense separable operator of csrc/tvop.hip restated in float64 NumPy: the
operator A x = R0 x R1^T and its adjoint, the step bound, the default start, the objective, the Chambolle-Pock iteration with both
terms dual, the operator makers and an independent L-BFGS-B minimum.  One image at a time or a batch on leading axes: x [..., H, W],
y [..., h, w], R0 [h, H], R1 [w, W].  The tests compare the kernels with these functions; nothing here imports the package."""
import numpy as np

from tests import fourier_common as F
from tests import tvsr_common as T

psnr, pat07_roi = T.psnr, T.pat07_roi
X_BOUND, CHANGE_BOUND, ENERGY_REL = 1e-10, 2e-10, 1e-12      # the solver against this file (the issue's derivation)

# (H, W) -> (h, w): ragged 16- and 64-tiles, a K loop of more than one stage, h > H, a single row / column
SHAPES = [((12, 20), (5, 7)), ((1, 70), (1, 33)), ((70, 1), (33, 1)), ((33, 17), (33, 17)), ((130, 70), (37, 33)), ((37, 33), (130, 70))]


def apply(x, R0, R1):
    """A x = (R0 x) R1^T."""
    return np.matmul(np.matmul(R0, x), R1.T)


def adjoint(r, R0, R1):
    """A^T r = R0^T (r R1)."""
    return np.matmul(R0.T, np.matmul(r, R1))


def norm_bound(R):
    """(max_i sum_j |R[i][j]|) (max_j sum_i |R[i][j]|) = |R|_inf |R|_1 >= |R|_2^2, every sum in ascending index."""
    a = np.abs(np.asarray(R, np.float64))
    rows, cols = np.zeros(a.shape[0]), np.zeros(a.shape[1])
    for j in range(a.shape[1]):
        rows = rows + a[:, j]
    for i in range(a.shape[0]):
        cols = cols + a[i, :]
    return rows.max() * cols.max()


def step(R0, R1):
    """tau = sigma = 1 / sqrt(8 + c0 c1)."""
    return 1.0 / np.sqrt(8.0 + norm_bound(R0) * norm_bound(R1))


def usable(y, w=None):
    """u = [w > 0] (all of it without weights), of the shape of y."""
    if w is None:
        return np.ones(np.shape(y), bool)
    with np.errstate(invalid="ignore"):
        return np.asarray(w, np.float64) > 0


def default_start(y, R0, R1, w=None):
    """(|R0|^T (u y) |R1|) / (|R0|^T u |R1|), 0 where the denominator is not > 0; a datum outside u is not read."""
    u = usable(y, w)
    a0, a1 = np.abs(R0), np.abs(R1)
    num = adjoint(np.where(u, y, 0.0), a0, a1)
    den = adjoint(u.astype(np.float64), a0, a1)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def energy(x, y, R0, R1, lam, alpha, w=None):
    """1/2 sum w (A x - y)^2 + lam sum H_alpha(|grad x|), per image; data of weight 0 are not read."""
    u = usable(y, w)
    ww = np.where(u, 1.0 if w is None else w, 0.0)
    res = np.where(u, apply(x, R0, R1) - np.where(u, y, 0.0), 0.0)
    data = 0.5 * (ww * res * res).sum(axis=(-2, -1))
    if lam == 0:
        return data
    g0, g1 = T.grad(x)
    return data + lam * T.huber(np.sqrt(g0 * g0 + g1 * g1), alpha).sum(axis=(-2, -1))


def solve(y, R0, R1, lam, alpha, n_iter, w=None, x0=None, return_info=False, dtype=np.float64):
    """Chambolle-Pock with both terms dual, from x = xbar = x0 (default: the back-projection), p = 0, q = 0.  ``dtype``: the iteration
    in another float type (longdouble: the restatement's own error)."""
    R0, R1 = np.asarray(R0, dtype), np.asarray(R1, dtype)
    u = usable(y, w)
    yy = np.where(u, np.asarray(y, dtype), 0).astype(dtype)
    safe = np.where(u, 1.0 if w is None else np.asarray(w, dtype), 1).astype(dtype)
    tau = sigma = dtype(step(R0.astype(np.float64), R1.astype(np.float64)))
    x = (default_start(y, R0, R1, w) if x0 is None else np.array(x0)).astype(dtype)
    xbar = x.copy()
    p0, p1, q = np.zeros_like(x), np.zeros_like(x), np.zeros_like(yy)
    change = np.zeros(x.shape[:-2])
    lam_t, alpha_t = dtype(lam), dtype(alpha)
    for _ in range(n_iter):
        if lam > 0:
            g0, g1 = T.grad(xbar)
            den = 1 + sigma * alpha_t / lam_t
            p0, p1 = (p0 + sigma * g0) / den, (p1 + sigma * g1) / den
            s = np.maximum(1, np.sqrt(p0 * p0 + p1 * p1) / lam_t)
            p0, p1 = p0 / s, p1 / s
        q = np.where(u, (q + sigma * (apply(xbar, R0, R1) - yy)) / (1 + sigma / safe), 0)
        xn = x - tau * (adjoint(q, R0, R1) - T.div(p0, p1))
        change = np.abs(xn - x).max(axis=(-2, -1))
        xbar = 2 * xn - x
        x = xn
    if return_info:
        return x, energy(x.astype(np.float64), y, R0.astype(np.float64), R1.astype(np.float64), lam, alpha, w), change
    return x


# ---- the operator makers ----------------------------------------------------------------------------------------------------------------
def psf_operator(n, m, fwhm, kind="gaussian"):
    """[m][n]: row i is a point-spread function of full width at half maximum ``fwhm`` LR pixels centred on HR sample
    (i + 1/2) n / m - 1/2, normalised to sum 1 over the samples inside the line.  'gaussian': sampled at the HR samples; 'box': the
    overlap of the box with every sample's unit cell."""
    c = (np.arange(m) + 0.5) * n / m - 0.5
    j = np.arange(n, dtype=np.float64)
    width = fwhm * n / m
    if kind == "gaussian":
        sigma = width / (2.0 * np.sqrt(2.0 * np.log(2.0)))
        R = np.exp(-0.5 * ((j[None, :] - c[:, None]) / sigma) ** 2)
    else:
        lo, hi = c[:, None] - width / 2.0, c[:, None] + width / 2.0
        R = np.clip(np.minimum(hi, j[None, :] + 0.5) - np.maximum(lo, j[None, :] - 0.5), 0.0, None)
    return R / R.sum(axis=1, keepdims=True)


def block_operator(n, f, kernel="mean"):
    """[n / f][n]: R[i][f i + a] = k[a], the dense form of a 1-D block kernel ('mean', 'decimate' or f values)."""
    if isinstance(kernel, str):
        k = np.full(f, 1.0 / f) if kernel == "mean" else np.eye(f)[0]
    else:
        k = np.asarray(kernel, np.float64)
    R = np.zeros((n // f, n))
    for i in range(n // f):
        R[i, f * i:f * i + f] = k
    return R


def fourier_pair(shape, lr_shape, align, boundary):
    return tuple(F.restated_operator(n, m, align, boundary, 0.0) for n, m in zip(shape, lr_shape))


def gaussian_pair(shape, lr_shape, fwhm=(1.2, 1.0)):
    return tuple(psf_operator(n, m, fw) for n, m, fw in zip(shape, lr_shape, fwhm))


def random_pair(shape, lr_shape, seed=0):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal((m, n)) / np.sqrt(n) for n, m in zip(shape, lr_shape))


# the issue's weighted Huber case: (12, 20) -> (5, 7), Gaussian operators of FWHM 1.2 / 1.0, weights in [0.5, 1.5) with one zero
CASE_SHAPE, CASE_LR = (12, 20), (5, 7)
CASE_LAM, CASE_ALPHA = 0.05, 0.02


def case_data(seed=0):
    """(hr [12][20], y [5][7], weight [5][7], (R0, R1))."""
    rng = np.random.default_rng(seed)
    ops = gaussian_pair(CASE_SHAPE, CASE_LR)
    hr = rng.random(CASE_SHAPE)
    w = 0.5 + rng.random(CASE_LR)
    w[2, 3] = 0.0
    return hr, apply(hr, *ops), w, ops


def lbfgs_minimum(y, R0, R1, lam, alpha, w, shape):
    """The minimum of the Huber energy by L-BFGS-B with the analytic gradient (scipy), independent of the iteration."""
    from scipy.optimize import minimize
    u = usable(y, w)
    ww = np.where(u, 1.0 if w is None else w, 0.0)
    yy = np.where(u, y, 0.0)

    def fun(z):
        x = z.reshape(shape)
        res = apply(x, R0, R1) - yy
        g0, g1 = T.grad(x)
        t = np.sqrt(g0 * g0 + g1 * g1)
        scale = np.where(t <= alpha, 1.0 / alpha, 1.0 / np.maximum(t, 1e-300))       # H'(t) / t
        e = 0.5 * (ww * res * res).sum() + lam * T.huber(t, alpha).sum()
        return e, (adjoint(ww * res, R0, R1) - lam * T.div(scale * g0, scale * g1)).ravel()

    z = default_start(y, R0, R1, w).ravel()
    for _ in range(5):                                                                # restarts: the memory is rebuilt at the iterate
        res = minimize(fun, z, jac=True, method="L-BFGS-B", options={"maxiter": 20000, "maxfun": 200000, "ftol": 0, "gtol": 1e-14,
                                                                     "maxcor": 50})
        z = res.x
    return float(res.fun)
