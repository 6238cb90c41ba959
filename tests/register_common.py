"""Shared by tests/test_register_cpu.py and tests/test_gpu_register.py: the masked normalised cross-correlation (Padfield 2012) by
its definition, the scipy shift it feeds, and the host logic of the PROBA-V preparation restated in NumPy.

``direct_xcorr`` is the oracle: float64, no FFT.  For every displacement d the pixel p of ``ref`` is paired with the pixel p - d of
``x``; the pairs with m(p) and m(p - d) both set give n, num = S_ab - S_a S_b / n, da = max(S_aa - S_a^2 / n, 0), db likewise, den =
sqrt(da db); over the map tol = 1e3 2^-52 max den, C = clip(num / den, -1, 1) where den > tol else 0, and C = 0 where
n < overlap_ratio max n.  ``fft_xcorr`` forms the same six correlations with FFTs, as skimage does (scikit-image is not installed:
parity is pinned to the definition); their difference is the formula's own arithmetic noise.  ``shift_of`` is the mean position of
the maxima of C: the translation to apply to ``x``.

``CASES`` are the four correlation cases: smoothed noise on an offset, a planted integer translation (both images cut from one
larger field, so nothing wraps), 2 % added noise, two masked blocks.  ``case_stats`` gives the conditions under which a device map
can be compared entry by entry: a unique maximum, its distance to the runner-up, the cancellation factor kappa of the centred sums
and the distance of every den from tol.
"""
import numpy as np
import scipy.ndimage as ndi

OVERLAP = 3 / 10
# (shape, planted shift): a 16-wide tile of displacements (2H - 1 by 2W - 1 of them) and of pixels is missed, crossed twice, met
CASES = [((24, 20), (2, -3)), ((17, 23), (-4, 1)), ((33, 31), (5, 6)), ((16, 16), (0, 0))]
CASE_IDS = [f"{s[0]}x{s[1]}" for s, _ in CASES]
SHIFT_BOUND = 2e-7                    # of max|in|, rescale_common.BOUND: fp64 arithmetic rounded once to fp32


def f32(a):
    """fp32-representable values (what the device entry points take), as float64."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def field(shape, seed, margin=8):
    """Smoothed unit-variance noise on an offset of 4, `margin` pixels larger than `shape` on every side."""
    rng = np.random.default_rng(seed)
    big = ndi.gaussian_filter(rng.standard_normal((shape[0] + 2 * margin, shape[1] + 2 * margin)), 1.5, mode="wrap")
    return 4.0 + big / big.std(), rng


def cut(big, shape, s, margin=8):
    """x with x(q) = ref(q + s) for the ref cut at the margin: shift(x, s) lies on ref."""
    return big[margin + s[0]:margin + s[0] + shape[0], margin + s[1]:margin + s[1] + shape[1]]


def blocks_mask(shape, rng):
    m = np.ones(shape)
    for _ in range(2):
        r, c = rng.integers(0, shape[0] - 4), rng.integers(0, shape[1] - 4)
        m[r:r + 4, c:c + 3] = 0
    return m


def make_case(shape, planted, seed=0, noise=0.02):
    """(ref, x, m): float64 arrays of fp32-representable values."""
    big, rng = field(shape, seed)
    ref = cut(big, shape, (0, 0)) + noise * rng.standard_normal(shape)
    x = cut(big, shape, planted) + noise * rng.standard_normal(shape)
    return f32(ref), f32(x), blocks_mask(shape, rng)


def window(shape, max_shift=None):
    my, mx = shape[0] - 1, shape[1] - 1
    if max_shift is not None:
        my, mx = min(my, int(max_shift)), min(mx, int(max_shift))
    return my, mx


def _windows(a, my, mx):
    """v[dy + my, dx + mx, p] = a(p - d), zero outside the image."""
    H, W = a.shape
    padded = np.pad(a, ((my, my), (mx, mx)))
    v = np.lib.stride_tricks.sliding_window_view(padded, (H, W))          # v[i, j] = padded[i:i + H, j:j + W] = a(p - (my - i, mx - j))
    return v[::-1, ::-1]


def _sums_direct(ref, x, m, my, mx):
    mb = (np.asarray(m) != 0).astype(np.float64)
    a, b = ref * mb, x * mb
    wm, wb, wbb = _windows(mb, my, mx), _windows(b, my, mx), _windows(b * b, my, mx)
    e = lambda left, right: np.einsum("ij,yxij->yx", left, right)
    return e(mb, wm), e(a, wm), e(mb, wb), e(a * a, wm), e(mb, wbb), e(a, wb)


def _sums_fft(ref, x, m, my, mx):
    H, W = ref.shape
    mb = (np.asarray(m) != 0).astype(np.float64)
    a, b = ref * mb, x * mb
    full = (2 * H - 1, 2 * W - 1)
    F = lambda z: np.fft.rfft2(z, full)

    def corr(left, right):                                                 # sum_p left(p) right(p - d), d = -(H - 1) .. H - 1
        c = np.fft.irfft2(F(left) * np.conj(F(right)), full)
        c = np.roll(c, (H - 1, W - 1), axis=(0, 1))
        return c[H - 1 - my:H + my, W - 1 - mx:W + mx]
    n = np.round(corr(mb, mb))
    return n, corr(a, mb), corr(mb, b), corr(a * a, mb), corr(mb, b * b), corr(a, b)


def _finish(sums, overlap_ratio, parts):
    n, sa, sb, saa, sbb, sab = sums
    safe = np.where(n > 0, n, 1.0)
    some = n > 0
    num = np.where(some, sab - sa * sb / safe, 0.0)
    da = np.where(some, np.maximum(saa - sa * sa / safe, 0.0), 0.0)
    db = np.where(some, np.maximum(sbb - sb * sb / safe, 0.0), 0.0)
    den = np.sqrt(da * db)
    tol = 1e3 * 2.0 ** -52 * den.max()
    C = np.where(den > tol, np.clip(num / np.where(den > tol, den, 1.0), -1.0, 1.0), 0.0)
    kept = n >= overlap_ratio * n.max()
    C = np.where(kept, C, 0.0)
    if parts:
        return C, dict(n=n, saa=saa, sbb=sbb, da=da, db=db, den=den, tol=tol, kept=kept)
    return C


def direct_xcorr(ref, x, m, overlap_ratio=OVERLAP, max_shift=None, parts=False):
    my, mx = window(ref.shape, max_shift)
    return _finish(_sums_direct(np.asarray(ref, np.float64), np.asarray(x, np.float64), m, my, mx), overlap_ratio, parts)


def fft_xcorr(ref, x, m, overlap_ratio=OVERLAP, max_shift=None):
    my, mx = window(ref.shape, max_shift)
    return _finish(_sums_fft(np.asarray(ref, np.float64), np.asarray(x, np.float64), m, my, mx), overlap_ratio, False)


def shift_of(C):
    """(mean position of the maxima, the maximum, their number); the map's centre is the displacement (0, 0)."""
    at = np.argwhere(C == C.max())
    centre = (np.asarray(C.shape) - 1) / 2
    return at.mean(axis=0) - centre, float(C.max()), len(at)


def case_stats(ref, x, m, overlap_ratio=OVERLAP, max_shift=None):
    C, p = direct_xcorr(ref, x, m, overlap_ratio, max_shift, parts=True)
    s, peak, count = shift_of(C)
    second = np.sort(C.ravel())[-2]
    k = p["kept"] & (p["n"] > 0)
    kappa = max((p["saa"][k] / p["da"][k]).max(), (p["sbb"][k] / p["db"][k]).max())
    near_tol = bool(np.any((p["den"] > p["tol"] / 2) & (p["den"] < 2 * p["tol"])))
    return dict(C=C, shift=s, peak=peak, second=float(second), count=count, kappa=float(kappa), near_tol=near_tol,
                fft_diff=float(np.abs(fft_xcorr(ref, x, m, overlap_ratio, max_shift) - C).max()))


def map_bound(stats, n_pixels):
    """max(100 y, 4 N 2^-53 kappa): y the FFT-against-direct difference (the formula's own noise; 100 for a third summation order),
    the second term the first-order forward error of one ratio of three centred sums over N pixels."""
    return max(100.0 * stats["fft_diff"], 4.0 * n_pixels * 2.0 ** -53 * stats["kappa"])


def scipy_register_imgset(imgset, mask, overlap_ratio=OVERLAP, max_shift=None):
    """The body of register_imgset through the oracle and scipy: (registered images, shifted masks, shifts [T, 2], reference index)."""
    imgset, mask = np.asarray(imgset, np.float64), np.asarray(mask, np.float64)
    best = int(np.argmax(np.mean(mask, axis=(0, 1))))
    ref = imgset[..., best]
    out, out_m, shifts = np.empty(imgset.shape), np.empty(mask.shape), []
    for i in range(imgset.shape[-1]):
        s, _, _ = shift_of(direct_xcorr(ref, imgset[..., i], mask[..., i], overlap_ratio, max_shift))
        out[..., i] = ndi.shift(imgset[..., i], s, mode="reflect")
        out_m[..., i] = ndi.shift(mask[..., i], s, mode="constant", cval=0)
        shifts.append(s)
    return out, out_m, np.asarray(shifts), best


# ---- the host logic of select_T_images, gen_sub and augment_* (index lists from clearances and seeds), restated -------------------
def select_indexes(clearance, T, thr, remove_bad):
    """Per set: the indexes (into the set's T_i images) that are kept, in order, or None for a removed set."""
    clearance = np.asarray(clearance)
    clear = np.flatnonzero(clearance > thr)
    if not len(clear):
        if remove_bad:
            return None
        clear = np.array([int(np.argmax(clearance))])
    order = list(np.argsort(clearance[clear])[::-1])
    extra = []
    for _ in range(T - len(clear)):                                        # drawn from the sorted list as it stands before the draws
        extra.append(np.random.choice(order))
    order = order + extra
    return [int(clear[j]) for j in order[:T]]


def select_restated(X, masks, T=9, thr=0.85, remove_bad=True):
    chosen, removed = [], []
    for i in range(len(X)):
        idx = select_indexes(np.mean(masks[i], axis=(0, 1)), T, thr, remove_bad)
        if idx is None:
            removed.append(i)
        else:
            chosen.append(np.asarray(X[i])[..., idx])
    return np.array(chosen), removed


def gen_sub_restated(array, d, s):
    n = (array.shape[1] - d) // s + 1
    return np.array([X[i * s:i * s + d, j * s:j * s + d] for X in array for i in range(n) for j in range(n)], dtype=np.float64)


def augment_restated(X, y, y_masks, n_augment):
    Xa, ya, ma = [], [], []
    for i in range(len(X)):
        Xa.append(X[i])
        for _ in range(n_augment - 1):
            Xa.append(X[i][..., np.random.permutation(X[i].shape[-1])])
        ya += [y[i]] * n_augment
        ma += [y_masks[i]] * n_augment
    return np.array(Xa, np.float64), np.array(ya, np.float64), np.array(ma, np.float64)


# ---- the inputs of the device tests ---------------------------------------------------------------------------------------------------
def make_sets(shape, planted, seed=0):
    """Two sets of three images of one case's shape for ONE correlation call: set 0 is (ref, x, ref with fresh noise) of
    ``make_case`` with the reference first, set 1 comes from another field with its reference last.  Returns planes, masks
    [2, 3, H, W], the reference indexes and the planted translations [2, 3, 2]."""
    ref, x, m = make_case(shape, planted, seed)
    rng = np.random.default_rng(seed + 50)
    again = f32(ref + 0.02 * rng.standard_normal(shape))
    big, rng_b = field(shape, seed + 1)
    s1, s2 = (-planted[0], -planted[1]), (1, -2)
    noisy = lambda s: f32(cut(big, shape, s) + 0.02 * rng_b.standard_normal(shape))
    planes = np.array([[ref, x, again], [noisy(s1), noisy(s2), noisy((0, 0))]])
    masks = np.array([[m, m, blocks_mask(shape, rng)], [blocks_mask(shape, rng_b) for _ in range(3)]])
    return planes, masks, np.array([0, 2], dtype=np.int32), np.array([[(0, 0), planted, (0, 0)], [s1, s2, (0, 0)]], dtype=np.float64)


def make_imgset(shape=(24, 20), shifts=((1, -2), (0, 3), (-3, 0), (0, 0), (2, 2)), seed=4):
    """A set [H, W, T] whose image 3 (of five) is the clearest: image t is the reference field cut at ``shifts[t]`` plus noise, its mask has
    t-dependent blocks cleared (unequal clearances, image 3 with the fewest)."""
    big, rng = field(shape, seed)
    imgs = np.stack([f32(cut(big, shape, s) + 0.02 * rng.standard_normal(shape)) for s in shifts], axis=-1)
    masks = np.ones(shape + (len(shifts),))
    for t, rows in enumerate((4, 3, 5, 1, 2)[:len(shifts)]):
        r, c = rng.integers(0, shape[0] - 6), rng.integers(0, shape[1] - 6)
        masks[r:r + rows, c:c + 4, t] = 0
    return imgs, masks, np.asarray(shifts, dtype=np.float64)


RAMS_PLANTED = {2: (1, -2), 5: (-3, 1), 7: (2, 2)}


def rams_case(n=20, T=10, Z=2, seed=8):
    """The synthetic patient of tests/test_gpu_cssim.py::test_rams_master_ssim_flag with three acquisitions of every slice rolled so
    that ``shift(acquisition, RAMS_PLANTED[t])`` lies on acquisition 0.  Returns (dwi [n, n, Z, T], b0 [n, n, Z]) float32."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n), indexing="ij")
    base = 60.0 + 50.0 * np.sin(5 * gx) * np.cos(4 * gy)
    dwi = np.stack([np.stack([base * (1 + 0.1 * z) * (1 + 0.04 * rng.standard_normal(base.shape)) for _ in range(T)], axis=-1)
                    for z in range(Z)], axis=2).clip(1, 250).astype(np.float32)
    for t, s in RAMS_PLANTED.items():
        dwi[..., t] = np.roll(dwi[..., t], (-s[0], -s[1]), axis=(0, 1))
    b0 = np.stack([2.5 * base * (1 + 0.1 * z) for z in range(Z)], axis=2).astype(np.float32)
    return dwi, b0
