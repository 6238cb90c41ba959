"""The multi-frame TV / Huber super-resolution of csrc/tvmf.hip restated in float64 NumPy: the per-frame operator
A_k = B S_k through its effective kernel, the validity of a datum, the adjoint, the objective, the Chambolle-Pock iteration with both
terms dual, the shift estimate (Fourier up-sampling + masked cross-correlation, through the oracles of fourier_common and
register_common) and the simulation of the study.  One image at a time: x [H][W], frames [K][h][w], shifts [K][2] in HR pixels.  The
tests compare the kernels with these functions; nothing here imports the package."""
import numpy as np

from tests import fourier_common as F
from tests import register_common as R
from tests import tvsr_common as T

MAX_SHIFT = 2.0 ** 20
block_kernel, replicate, psnr, pat07_roi = T.block_kernel, T.replicate, T.psnr, T.pat07_roi


def geometry(s):
    """(usable, n [2] int, t [2]): n = floor(s), t = s - n; a shift that is not finite or beyond 2^20 is unusable (n = t = 0)."""
    s = np.asarray(s, np.float64)
    ok = bool(np.all(np.abs(s) <= MAX_SHIFT))                 # False for NaN and the infinities
    c = s if ok else np.zeros(2)
    n = np.floor(c)
    return ok, n.astype(np.int64), c - n


def eff_kernel(k, t):
    """ke [f0 + (t0 > 0)][f1 + (t1 > 0)] = sum over the taps of (wa wb) k displaced by (da, db); a tap with t == 0 is not visited."""
    f0, f1 = k.shape
    ke = np.zeros((f0 + (t[0] > 0), f1 + (t[1] > 0)))
    for da in range(1 + (t[0] > 0)):
        for db in range(1 + (t[1] > 0)):
            wa, wb = (t[0] if da else 1.0 - t[0]), (t[1] if db else 1.0 - t[1])
            ke[da:da + f0, db:db + f1] += (wa * wb) * k
    return ke


def _frame(k, s, H, W):
    """(n, ke, valid LR rows [h] bool, valid LR columns [w] bool) of one frame."""
    f0, f1 = k.shape
    ok, n, t = geometry(s)
    ke = eff_kernel(k, t)
    ii, jj = n[0] + f0 * np.arange(H // f0), n[1] + f1 * np.arange(W // f1)
    vi = ok & (ii >= 0) & (ii + ke.shape[0] <= H)
    vj = ok & (jj >= 0) & (jj + ke.shape[1] <= W)
    return n, ke, vi, vj


def valid_mask(k, s, H, W):
    _, _, vi, vj = _frame(k, s, H, W)
    return np.outer(vi, vj)


def apply_frame(x, k, s):
    """A_k x [h][w], 0 at invalid data: (A x)[i][j] = sum_{a, b} ke[a][b] x[n0 + f0 i + a][n1 + f1 j + b]."""
    H, W = x.shape
    f0, f1 = k.shape
    n, ke, vi, vj = _frame(k, s, H, W)
    out = np.zeros((H // f0, W // f1))
    ii, jj = n[0] + f0 * np.flatnonzero(vi), n[1] + f1 * np.flatnonzero(vj)
    acc = np.zeros((len(ii), len(jj)))
    for a in range(ke.shape[0]):
        for b in range(ke.shape[1]):
            acc += ke[a, b] * x[np.ix_(ii + a, jj + b)]
    out[np.ix_(vi, vj)] = acc
    return out


def adjoint_frame(r, k, s, H, W):
    """A_k^T r [H][W]: ke[a][b] r[i][j] of every valid datum lands on pixel (n0 + f0 i + a, n1 + f1 j + b)."""
    f0, f1 = k.shape
    n, ke, vi, vj = _frame(k, s, H, W)
    out = np.zeros((H, W))
    ii, jj = n[0] + f0 * np.flatnonzero(vi), n[1] + f1 * np.flatnonzero(vj)
    rv = r[np.ix_(vi, vj)]
    for a in range(ke.shape[0]):
        for b in range(ke.shape[1]):
            out[np.ix_(ii + a, jj + b)] += ke[a, b] * rv
    return out


def apply_frames(x, k, shifts):
    return np.stack([apply_frame(x, k, s) for s in shifts])


def adjoint_frames(r, k, shifts, H, W):
    return sum(adjoint_frame(rk, k, s, H, W) for rk, s in zip(r, shifts))


def weights(k, shifts, H, W, w=None):
    """The weights the solver works with [K][h][w]: ``w`` (default 1) where a datum is valid and w > 0, else 0."""
    valid = np.stack([valid_mask(k, s, H, W) for s in shifts])
    w = np.ones(valid.shape) if w is None else np.asarray(w, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(valid & (w > 0), w, 0.0)


def step(k, shifts, H, W):
    """tau = sigma = 1 / sqrt(8 + K' c): c = (sum |k|) (max |k|), K' the frames with a valid datum."""
    live = sum(bool(valid_mask(k, s, H, W).any()) for s in shifts)
    return 1.0 / np.sqrt(8.0 + live * (np.abs(k).sum() * np.abs(k).max()))


def energy(x, frames, k, shifts, lam, alpha, w=None):
    """1/2 sum_k sum w (A_k x - y_k)^2 + lam sum H_alpha(|grad x|); data of weight 0 are not read."""
    ww = weights(k, shifts, *x.shape, w)
    res = np.where(ww > 0, apply_frames(x, k, shifts) - np.where(ww > 0, frames, 0.0), 0.0)
    data = 0.5 * (ww * res * res).sum()
    if lam == 0:
        return data
    g0, g1 = T.grad(x)
    return data + lam * T.huber(np.sqrt(g0 * g0 + g1 * g1), alpha).sum()


def solve(frames, factors, shifts, kernel="mean", lam=0.01, alpha=0.03, n_iter=300, w=None, x0=None, return_info=False):
    """Chambolle-Pock with both terms dual, from x = xbar = x0 (default: the block replication of frame 0), p = 0, q = 0."""
    frames = np.asarray(frames, np.float64)
    k = block_kernel(kernel, factors)
    H, W = frames.shape[-2] * factors[0], frames.shape[-1] * factors[1]
    shifts = np.asarray(shifts, np.float64)
    ww = weights(k, shifts, H, W, w)
    y = np.where(ww > 0, frames, 0.0)
    safe = np.where(ww > 0, ww, 1.0)
    tau = sigma = step(k, shifts, H, W)
    x = replicate(frames[0], factors) if x0 is None else np.array(x0, np.float64)
    xbar = x.copy()
    p0, p1, q = np.zeros_like(x), np.zeros_like(x), np.zeros_like(y)
    change = 0.0
    for _ in range(n_iter):
        if lam > 0:
            g0, g1 = T.grad(xbar)
            den = 1.0 + sigma * alpha / lam
            p0, p1 = (p0 + sigma * g0) / den, (p1 + sigma * g1) / den
            s = np.maximum(1.0, np.sqrt(p0 * p0 + p1 * p1) / lam)
            p0, p1 = p0 / s, p1 / s
        q = np.where(ww > 0, (q + sigma * (apply_frames(xbar, k, shifts) - y)) / (1.0 + sigma / safe), 0.0)
        xn = x - tau * (adjoint_frames(q, k, shifts, H, W) - T.div(p0, p1))
        change = np.abs(xn - x).max()
        xbar = 2.0 * xn - x
        x = xn
    if return_info:
        valid = np.stack([valid_mask(k, s, H, W) for s in shifts])
        return x, energy(x, frames, k, shifts, lam, alpha, w), change, valid.mean()
    return x


# the issue's three-frame case: 6 x 10, factors (3, 2), the mean kernel, frame weights 1 / 0.5 / 2
CASE_FACTORS = (3, 2)
CASE_SHIFTS = np.array([[0.0, 0.0], [1.25, -0.5], [-0.75, 1.0]])
CASE_FRAME_WEIGHTS = (1.0, 0.5, 2.0)
CASE_LAM, CASE_ALPHA = 0.05, 0.02


def case_data():
    """(hr [6][10], frames [3][2][5], weight [3][2][5])."""
    hr = np.random.default_rng(0).random((6, 10))
    k = block_kernel("mean", CASE_FACTORS)
    frames = apply_frames(hr, k, CASE_SHIFTS)
    return hr, frames, np.stack([np.full(frames.shape[1:], v) for v in CASE_FRAME_WEIGHTS])


def lbfgs_minimum(frames, k, shifts, lam, alpha, w, shape):
    """The minimum of the Huber energy by L-BFGS-B with the analytic gradient (scipy), independent of the iteration."""
    from scipy.optimize import minimize
    ww = weights(k, shifts, *shape, w)
    y = np.where(ww > 0, frames, 0.0)

    def fun(z):
        x = z.reshape(shape)
        res = apply_frames(x, k, shifts) - y
        g0, g1 = T.grad(x)
        t = np.sqrt(g0 * g0 + g1 * g1)
        scale = np.where(t <= alpha, 1.0 / alpha, 1.0 / np.maximum(t, 1e-300))       # H'(t) / t
        e = 0.5 * (ww * res * res).sum() + lam * T.huber(t, alpha).sum()
        return e, (adjoint_frames(ww * res, k, shifts, *shape) - lam * T.div(scale * g0, scale * g1)).ravel()

    z = replicate(frames[0], k.shape).ravel()
    for _ in range(5):                                                                # restarts: the memory is rebuilt at the iterate
        res = minimize(fun, z, jac=True, method="L-BFGS-B", options={"maxiter": 20000, "maxfun": 200000, "ftol": 0, "gtol": 1e-14,
                                                                     "maxcor": 50})
        z = res.x
    return float(res.fun)


# ---- the simulation of the study and the shift estimate -------------------------------------------------------------------------------
def simulate(hr, factors, shifts, kernel="mean"):
    """The noiseless frames [K][h][w] of ``hr`` with ZEROS beyond its border, so that every datum is defined: the frames of the
    image padded by whole blocks, cut back to the h x w data of the image itself."""
    k = block_kernel(kernel, factors)
    shifts = np.asarray(shifts, np.float64)
    pad = [f * int(np.ceil((np.abs(shifts[:, a]).max() + 1.0) / f)) for a, f in enumerate(factors)]
    big = np.pad(hr, ((pad[0], pad[0]), (pad[1], pad[1])))
    out = apply_frames(big, k, shifts)
    b0, b1 = pad[0] // factors[0], pad[1] // factors[1]
    return out[:, b0:b0 + hr.shape[0] // factors[0], b1:b1 + hr.shape[1] // factors[1]]


def estimate_shifts(frames, factors, upsample=4, max_shift=None, reference=0):
    """[K][2] in HR pixels: every frame up-sampled by the Fourier oracle (align 'center', mirror boundary), correlated with the
    up-sampled reference by the FFT oracle of the masked cross-correlation with an all-clear mask; the step is f / upsample."""
    h, w = frames.shape[-2:]
    ups = [F.oracle_resize(fr, (upsample * h, upsample * w), "center", "mirror", 0.0) for fr in frames]
    m = np.ones_like(ups[0])
    win = None if max_shift is None else int(np.ceil(max_shift * upsample))
    steps = np.array([R.shift_of(R.fft_xcorr(ups[reference], x, m, R.OVERLAP, win))[0] for x in ups])
    return steps * (np.asarray(factors, np.float64) / upsample)


STUDY_ROI, STUDY_SLICES, STUDY_FACTORS, STUDY_FRAMES = (30, 102), (10, 14, 18), (2, 2), 8
STUDY_MAX_SHIFT, STUDY_NOISE, STUDY_MARGIN, STUDY_SEED = 1.5, 0.02, 4, 1


def study_frames(hr, seed, n_frames=STUDY_FRAMES, max_shift=STUDY_MAX_SHIFT, noise=STUDY_NOISE, factors=STUDY_FACTORS, kernel="mean"):
    """(shifts [K][2], frames [K][h][w]) as scripts/multi_frame.py draws them: shifts uniform in +- max_shift with frame 0 at rest,
    then the noise, one generator seeded per slice."""
    rng = np.random.default_rng(seed)
    shifts = rng.uniform(-max_shift, max_shift, (n_frames, 2))
    shifts[0] = 0.0
    frames = simulate(hr, factors, shifts, kernel)
    return shifts, frames + noise * rng.standard_normal(frames.shape)


def margin_psnr(ref, x, margin=STUDY_MARGIN):
    c = slice(margin, -margin) if margin else slice(None)
    return psnr(ref[c, c], x[c, c])
