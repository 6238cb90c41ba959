"""Non-local means on volumes and non-local upsampling restated in float64 numpy from the definition in include/inrhip.h,
and the cases the CPU and GPU tests share.  ``nlm`` evaluates the definition offset by offset over whole volumes; with
``reverse=True`` the offsets and the patch terms are summed in the opposite order, and the deviation between the two evaluations
(``d_ref``) is what rounding alone does to a result: the kernel must lie within ``BOUND_FACTOR * d_ref``.  ``nlm_voxel`` is the
definition as a triple loop around one voxel.  References are computed once per process and returned read-only."""
import functools
import itertools

import numpy as np

EPS = np.finfo(np.float64).eps
BOUND_FACTOR = 32               # the project's factor between a reference's own rounding and what a kernel may deviate
WMAX_FLOOR = 1e-100             # below it center = 'max' sits at the discontinuity wmax = 0 of the definition
RICIAN_FLOOR = 1e-3             # m - 2 sigma2 at least this: the square root amplifies rounding at 0
SIGMA = 0.03


def phantom(shape, floor=0.0):
    """A piecewise-smooth volume in [floor, 1] whose structures stay several voxels wide on the small grids of the cases: an
    elliptic cylinder and a half-space over a ramp."""
    D, H, W = shape
    z, y, x = np.meshgrid((np.arange(D) + 0.5) / D - 0.5, (np.arange(H) + 0.5) / H - 0.5, (np.arange(W) + 0.5) / W - 0.5, indexing="ij")
    v = 0.2 + 0.2 * (x + 0.5)
    v = v + 0.4 * ((x / 0.3) ** 2 + ((y + 0.1) / 0.25) ** 2 < 1.0)
    v = v - 0.15 * (y + 0.3 * z > 0.27)
    return floor + (1.0 - floor) * np.clip(v, 0.0, 1.0)


# name -> (shape, search, patch)
CASES = {
    "1-small-odd": ((5, 11, 13), (2, 3, 3), (1, 1, 1)),
    "2-image": ((1, 24, 24), (0, 3, 3), (0, 1, 1)),
    "3-tiles": ((9, 19, 21), (3, 3, 3), (1, 1, 1)),
    "4-largest-radii": ((7, 9, 12), (5, 5, 5), (2, 2, 2)),
    "5-anisotropic": ((3, 40, 7), (1, 5, 2), (1, 2, 0)),
    "6-rician-mean-guide": ((4, 14, 15), (1, 2, 2), (1, 1, 1)),
}
CASE_IDS = tuple(CASES)
SCALAR_CASES = CASE_IDS[:5]
H2 = 2.0 * SIGMA ** 2


@functools.lru_cache(maxsize=None)
def case(name, member=0):
    """The inputs of a case as a dict of read-only arrays: x [C, D, H, W], guide [D, H, W], h2 (a float or a map), sigma2 (None or a map),
    truth [C, D, H, W].  ``member``: another draw of the noise (the batch of case 3)."""
    shape, search, patch = CASES[name]
    rng = np.random.default_rng(1000 * (CASE_IDS.index(name) + 1) + member)
    if name != "6-rician-mean-guide":
        truth = phantom(shape)[None]
        x = truth + SIGMA * rng.standard_normal(truth.shape)
        out = dict(x=x, guide=x[0].copy(), h2=H2, sigma2=None, sigma=None, truth=truth)
    else:
        s0 = phantom(shape, floor=0.3)
        adc = 0.2 + 0.5 * phantom(shape[::-1]).transpose(2, 1, 0)[:shape[0], :shape[1], :shape[2]]
        truth = np.stack([s0 * np.exp(-b * adc) for b in (0.0, 0.5, 1.0)])
        sigma = np.broadcast_to(np.linspace(0.02, 0.03, shape[2]), shape).copy()
        x = np.sqrt((truth + sigma * rng.standard_normal(truth.shape)) ** 2 + (sigma * rng.standard_normal(truth.shape)) ** 2)
        out = dict(x=x, guide=x.mean(axis=0), h2=2.0 * sigma ** 2 / 3.0, sigma2=sigma ** 2, sigma=sigma, truth=truth)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    out.update(search=search, patch=patch)
    return out


def _inside_pair(n, t):
    """The slice of u along an axis of n samples for which u and u + t are both inside."""
    return slice(max(0, -t), min(n, n - t))


def _box(F, r, order):
    """sum_d F[u + d] over the patch offsets d, zero outside: the terms in ascending (d0, d1, d2), or the reverse."""
    P = np.pad(F, [(ra, ra) for ra in r])
    D, H, W = F.shape
    offs = list(itertools.product(range(2 * r[0] + 1), range(2 * r[1] + 1), range(2 * r[2] + 1)))
    S = np.zeros_like(F)
    for d0, d1, d2 in (offs if order > 0 else offs[::-1]):
        S = S + P[d0:d0 + D, d1:d1 + H, d2:d2 + W]
    return S


def offsets(search, reverse=False):
    ts = [t for t in itertools.product(*(range(-s, s + 1) for s in search)) if t != (0, 0, 0)]
    return ts[::-1] if reverse else ts


def nlm(x, guide, search, patch, h2, sigma2=None, mask=None, center="max", reverse=False, return_info=False):
    """The definition on x [C, D, H, W] under guide [D, H, W]; h2 a float or [D, H, W]; sigma2 None or [D, H, W]; mask None or [D, H, W].
    -> out [C, D, H, W] (and, ``return_info``, a dict with wmax [D, H, W] and m [C, D, H, W], the mean before the Rician step)."""
    x = np.asarray(x, dtype=np.float64)
    G = np.asarray(guide, dtype=np.float64)
    C, D, H, W = x.shape
    h2v = np.broadcast_to(np.asarray(h2, dtype=np.float64), (D, H, W))
    filt = h2v > 0.0
    if mask is not None:
        filt = filt & (np.asarray(mask) != 0)
    h2s = np.where(filt, h2v, 1.0)
    V = x * x if sigma2 is not None else x
    acc, sw, wmax = np.zeros_like(x), np.zeros((D, H, W)), np.zeros((D, H, W))
    order = -1 if reverse else 1
    with np.errstate(invalid="ignore", over="ignore"):
        for t in offsets(search, reverse):
            sl = tuple(_inside_pair(n, ta) for n, ta in zip((D, H, W), t))
            sq = tuple(slice(s.start + ta, s.stop + ta) for s, ta in zip(sl, t))
            if any(s.stop <= s.start for s in sl):
                continue
            F, I = np.zeros((D, H, W)), np.zeros((D, H, W))
            F[sl] = (G[sl] - G[sq]) ** 2
            I[sl] = 1.0
            S, n = _box(F, patch, order), _box(I, patch, order)
            w = np.exp(-(S[sl] / n[sl]) / h2s[sl])
            acc[(slice(None),) + sl] += w * V[(slice(None),) + sq]
            sw[sl] += w
            wmax[sl] = np.fmax(wmax[sl], w)
        wc = np.ones((D, H, W)) if center == "one" else np.where(wmax > 0.0, wmax, 1.0)
        m = (acc + wc * V) / (sw + wc)
        out = m if sigma2 is None else np.sqrt(np.maximum(m - 2.0 * np.asarray(sigma2), 0.0))
    out = np.where(filt, out, x)
    return (out, dict(wmax=np.where(filt, wmax, 1.0), m=m, filtered=filt)) if return_info else out


def nlm_voxel(x, guide, search, patch, h2, p, sigma2=None, center="max"):
    """The definition at the one voxel p, term by term."""
    C, D, H, W = x.shape
    N = (D, H, W)
    inside = lambda v: all(0 <= v[a] < N[a] for a in range(3))
    V = x * x if sigma2 is not None else x
    acc, sw, wmax = np.zeros(C), 0.0, 0.0
    for t in offsets(search):
        q = tuple(p[a] + t[a] for a in range(3))
        if not inside(q):
            continue
        total, n = 0.0, 0
        for d in itertools.product(*(range(-r, r + 1) for r in patch)):
            pd, qd = tuple(p[a] + d[a] for a in range(3)), tuple(q[a] + d[a] for a in range(3))
            if inside(pd) and inside(qd):
                total += (guide[pd] - guide[qd]) ** 2
                n += 1
        w = np.exp(-(total / n) / h2)
        acc += w * V[(slice(None),) + q]
        sw += w
        wmax = max(wmax, w)
    wc = 1.0 if center == "one" else (wmax if wmax > 0.0 else 1.0)
    m = (acc + wc * V[(slice(None),) + tuple(p)]) / (sw + wc)
    return m if sigma2 is None else np.sqrt(np.maximum(m - 2.0 * sigma2[tuple(p)], 0.0))


@functools.lru_cache(maxsize=None)
def reference(name, center="max", member=0):
    """(out, d_ref, info) of a case: the forward evaluation, its largest deviation from the reversed one, and the forward info."""
    c = case(name, member)
    args = (c["x"], c["guide"], c["search"], c["patch"], c["h2"], c["sigma2"], None, center)
    out, info = nlm(*args, reverse=False, return_info=True)
    back = nlm(*args, reverse=True)
    out.setflags(write=False)
    return out, float(np.abs(out - back).max()), info


# ---- the upsampling ---------------------------------------------------------------------------------------------------------------------
def kernel_table(k0, k1, k2):
    """k[a][b][c] = (k1[b] k2[c]) k0[a], as the block operator forms it."""
    k0, k1, k2 = (np.asarray(k, dtype=np.float64) for k in (k0, k1, k2))
    return (k1[None, :, None] * k2[None, None, :]) * k0[:, None, None]


def named_kernel(kind, factors):
    if kind == "mean":
        return tuple(np.full(f, 1.0 / f) for f in factors)
    return tuple(np.eye(f)[0] for f in factors)        # 'decimate'


def block_apply(x, factors, ks, reverse=False):
    """A x: the block sums in ascending (a, b, c), or the reverse."""
    f0, f1, f2 = factors
    D, H, W = x.shape
    blocks = x.reshape(D // f0, f0, H // f1, f1, W // f2, f2)
    terms = list(itertools.product(range(f0), range(f1), range(f2)))
    acc = np.zeros((D // f0, H // f1, W // f2))
    for a, b, c in (terms[::-1] if reverse else terms):
        acc = acc + ks[a, b, c] * blocks[:, a, :, b, :, c]
    return acc


def replicate(r, factors):
    return np.repeat(np.repeat(np.repeat(r, factors[0], axis=0), factors[1], axis=1), factors[2], axis=2)


def upsample(lr, factors, kernel, levels, n_iter, search, patch, relax=1.0, x0=None, guide=None, reverse=False):
    """The solve on one volume lr [d, h, w]; kernel: (k0, k1, k2).  -> (x, change [passes])."""
    ks = kernel_table(*kernel)
    x = replicate(lr, factors) if x0 is None else np.array(x0, dtype=np.float64)
    change = []
    for h in levels:
        for _ in range(n_iter):
            xp = nlm(x[None], x if guide is None else guide, search, patch, h * h, center="one", reverse=reverse)[0]
            new = xp - relax * replicate(block_apply(xp, factors, ks, reverse) - lr, factors)
            change.append(float(np.abs(new - x).mean()))
            x = new
    return x, np.array(change)


def change_in_kernel_order(new, old, factors):
    """mean |new - old| added as inr_nlm_upsample adds it: per block in ascending (a, b, c); the blocks t, t + 256, ... of thread t in
    ascending order; then the 256 sums in order; divided by the number of voxels.  Bit for bit what the entry point stores."""
    f0, f1, f2 = factors
    D, H, W = new.shape
    diff = np.abs(new - old).reshape(D // f0, f0, H // f1, f1, W // f2, f2)
    part = np.zeros((D // f0, H // f1, W // f2))
    for a, b, c in itertools.product(range(f0), range(f1), range(f2)):
        part = part + diff[:, a, :, b, :, c]
    flat = part.reshape(-1)
    rows = -(-flat.size // 256)
    padded = np.zeros(rows * 256)
    padded[:flat.size] = flat
    per_thread = np.zeros(256)
    for row in padded.reshape(rows, 256):
        per_thread = per_thread + row
    total = 0.0
    for v in per_thread:
        total = total + v
    return total / float(D * H * W)


UPSAMPLE = dict(lr_shape=(4, 6, 7), factors=(2, 2, 2), levels=(0.125, 0.03125), n_iter=2, search=(2, 2, 2), patch=(1, 1, 1))


@functools.lru_cache(maxsize=None)
def upsample_case():
    """(lr, truth) of the upsampling tests: the block mean of a phantom, read-only."""
    u = UPSAMPLE
    hr = tuple(s * f for s, f in zip(u["lr_shape"], u["factors"]))
    truth = phantom(hr)
    lr = block_apply(truth, u["factors"], kernel_table(*named_kernel("mean", u["factors"])))
    lr.setflags(write=False)
    truth.setflags(write=False)
    return lr, truth


@functools.lru_cache(maxsize=None)
def upsample_reference():
    """((x, change), d_ref of x, d_ref of change) of the whole solve, by the same reordering."""
    u = UPSAMPLE
    lr, _ = upsample_case()
    k = named_kernel("mean", u["factors"])
    x, ch = upsample(lr, u["factors"], k, u["levels"], u["n_iter"], u["search"], u["patch"])
    xb, chb = upsample(lr, u["factors"], k, u["levels"], u["n_iter"], u["search"], u["patch"], reverse=True)
    x.setflags(write=False)
    return (x, ch), float(np.abs(x - xb).max()), float(np.abs(ch - chb).max())


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))
