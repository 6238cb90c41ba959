"""The float64 restatement of MP-PCA denoising (include/inrhip.h: inr_mppca_denoise), the phantom the tests share and
the cases the issue fixes.  Nothing here runs on a device.

The definition, per voxel inside the mask: the window starts at clamp(i - w / 2, 0, n - w) along each axis (shifted inward at the
edges, never mirrored), X is the M x N matrix of its voxels in (dz, dy, dx) order and c the voxel's own column; G = X X^T (M <= N) or
X^T X (N < M) is r x r, r = min(M, N), q = max(M, N); lam_p = max(s_p, 0) / q of the ascending eigenvalues s; the loop

    clam += lam_p;  gam = (p + 1) / (q - (r - p - 1))  (exp2)  or  (p + 1) / q  (exp1)
    a = clam / (p + 1);  b = (lam_p - lam_0) / (4 sqrt(gam));  b < a: sigma2 = a, cut = p + 1

gives sigma = sqrt(sigma2), rank = r - cut and the projection of the voxel's column onto the eigenvectors cut .. r - 1.  An eigenvalue
s_p <= q eps s_{r-1} is numerically zero -- what summing q products leaves of an exact zero: its lam_p is 0 and it is cut whatever the loop
decides (cut = max(cut, number of them)).  With noise no eigenvalue comes near that floor (the smallest is about sigma^2 (sqrt(q) -
sqrt(r))^2, seven to nine orders above it on the test cases), so there the rule changes no bit."""
import functools

import numpy as np

SIGMA = 0.05
EPS = 2.220446049250313e-16
# (M, volume, window): the cases of tests/test_mppca_cpu.py and tests/test_gpu_mppca.py, drawn in this order from default_rng(0)
CASES = ((16, (1, 24, 24), (1, 5, 5)),
         (16, (6, 12, 12), (3, 5, 5)),
         (8, (5, 9, 11), (3, 3, 3)),
         (30, (4, 7, 9), (3, 3, 3)),          # N = 27 < M = 30
         (64, (1, 12, 12), (1, 9, 9)))        # rank 64
CASE_IDS = tuple(f"M{m}-{'x'.join(map(str, v))}-w{'x'.join(map(str, w))}" for m, v, w in CASES)
ESTIMATORS = {"exp1": 1, "exp2": 2}


def window_start(i, w, n):
    return min(max(i - w // 2, 0), n - w)


def scaled(s, q):
    """(lam [r], zeros) of the ascending eigenvalues ``s``: lam_p = s_p / q, or 0 where s_p <= q eps s_{r-1} (numerically zero, which
    includes every s_p <= 0); ``zeros`` counts those."""
    s = np.asarray(s, np.float64)
    zero = s <= q * EPS * max(s[-1], 0.0)
    return np.where(zero, 0.0, s / q), int(zero.sum())


def cutoff(lam, q, estimator=2, zeros=0):
    """(sigma2, cut, margin) of the ascending scaled eigenvalues ``lam`` [r] (``scaled``): the loop of the definition, then cut =
    max(cut, zeros); ``margin`` is min over p >= 1 of |b - a| / lam[r - 1] (inf where lam[r - 1] == 0 or r == 1)."""
    r = len(lam)
    clam, cut, sigma2, margin = 0.0, 0, 0.0, np.inf
    for p in range(r):
        clam += lam[p]
        gam = (p + 1) / (q - (r - p - 1)) if estimator == 2 else (p + 1) / q
        a = clam / (p + 1)
        b = (lam[p] - lam[0]) / (4.0 * np.sqrt(gam))
        if b < a:
            sigma2, cut = a, p + 1
        if p >= 1 and lam[r - 1] > 0:
            margin = min(margin, abs(b - a) / lam[r - 1])
    return sigma2, max(cut, zeros), margin


def mppca(x, window, mask=None, estimator=2):
    """x [M, D, H, W] float64 -> (out [M, D, H, W], sigma [D, H, W], rank [D, H, W] int32, margin [D, H, W])."""
    x = np.asarray(x, np.float64)
    M, D, H, W = x.shape
    w0, w1, w2 = window
    N = w0 * w1 * w2
    r, q = min(M, N), max(M, N)
    out = x.copy()
    sigma = np.zeros((D, H, W))
    rank = np.full((D, H, W), -1, np.int32)
    margin = np.full((D, H, W), np.inf)
    for z in range(D):
        z0 = window_start(z, w0, D)
        for y in range(H):
            y0 = window_start(y, w1, H)
            for xx in range(W):
                if mask is not None and not mask[z, y, xx]:
                    continue
                x0 = window_start(xx, w2, W)
                X = x[:, z0:z0 + w0, y0:y0 + w1, x0:x0 + w2].reshape(M, N)
                c = ((z - z0) * w1 + (y - y0)) * w2 + (xx - x0)
                G = X @ X.T if M <= N else X.T @ X
                s, V = np.linalg.eigh(G)
                lam, zeros = scaled(s, q)
                sigma2, cut, margin[z, y, xx] = cutoff(lam, q, estimator, zeros)
                Vs = V[:, cut:]
                xhat = Vs @ (Vs.T @ X[:, c]) if M <= N else X @ (Vs @ Vs[c, :])
                out[:, z, y, xx] = xhat
                sigma[z, y, xx] = np.sqrt(sigma2)
                rank[z, y, xx] = r - cut
    return out, sigma, rank, margin


def mppca_reversed(x, window, mask=None, estimator=2):
    """The same result computed with the measurement rows in reversed order: what two float64 evaluations of one definition differ by."""
    out, sigma, rank, margin = mppca(np.ascontiguousarray(np.asarray(x, np.float64)[::-1]), window, mask, estimator)
    return np.ascontiguousarray(out[::-1]), sigma, rank, margin


def components(shape):
    """Three smooth positive spatial maps [3, D, H, W] on the unit cube."""
    D, H, W = shape
    zz, yy, xx = np.meshgrid(np.linspace(0.0, 1.0, D) if D > 1 else np.zeros(1), np.linspace(0.0, 1.0, H), np.linspace(0.0, 1.0, W),
                             indexing="ij")
    return np.stack([0.6 + 0.4 * np.sin(2 * np.pi * (xx + 0.3 * zz)),
                     0.6 + 0.4 * np.cos(2 * np.pi * (yy - 0.2 * zz)),
                     0.2 + xx * yy + 0.3 * zz])


def curves(M, rates=(0.5, 2.0, 6.0)):
    """Exponential decay curves [3, M] over t in [0, 1]."""
    t = np.linspace(0.0, 1.0, M)
    return np.stack([np.exp(-k * t) for k in rates])


def phantom(M, shape, sigma=SIGMA, rng=None, n_components=3):
    """(clean, noisy) [M, D, H, W]: ``n_components`` spatial maps times exponential decay curves, plus Gaussian noise."""
    clean = np.einsum("km,kzyx->mzyx", curves(M)[:n_components], components(shape)[:n_components])
    noisy = clean if sigma == 0 else clean + sigma * rng.standard_normal(clean.shape)
    return clean, noisy


@functools.lru_cache(maxsize=None)
def cases():
    """The five cases, drawn in order from default_rng(0): a tuple of dicts (M, shape, window, clean, noisy), computed once."""
    rng = np.random.default_rng(0)
    made = []
    for M, shape, window in CASES:
        clean, noisy = phantom(M, shape, SIGMA, rng)
        noisy.setflags(write=False)
        made.append(dict(M=M, shape=shape, window=window, clean=clean, noisy=noisy))
    return tuple(made)


@functools.lru_cache(maxsize=None)
def reference(index, estimator=2):
    """(out, sigma, rank, margin) of case ``index``, computed once and shared (read-only)."""
    c = cases()[index]
    res = mppca(c["noisy"], c["window"], None, estimator)
    for a in res:
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def reference_spread(index, estimator=2):
    """d_ref of case ``index``: the largest deviation, over ``out`` and ``sigma``, between the restatement and the restatement with the
    measurement rows reversed -- (d_out, d_sigma), absolute."""
    c = cases()[index]
    a = reference(index, estimator)
    b = mppca_reversed(c["noisy"], c["window"], None, estimator)
    return float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max())


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))
