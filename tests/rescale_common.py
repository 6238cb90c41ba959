"""Shared by tests/test_rescale_cpu.py and tests/test_gpu_rescale.py: what skimage 0.20 ``resize`` computes for a 2-D image, twice.

``scipy_resize`` is the composition of scipy calls skimage makes (scikit-image itself is not installed: parity is pinned to these
calls, as for the linear up-scale):  ``gaussian_filter(img, max(0, (f - 1)/2), mode=M)`` when anti-aliasing, then
``zoom(., out/in, order, mode=M, grid_mode=True)``, then the clip to the input's range; M = 'mirror' for 'reflect', 'nearest' for
'edge'.

``restated_resize`` restates the same steps in plain float64 numpy, line by line as csrc/rescale.hip runs them: it is the
definition the kernels are written from, checked against scipy here so that a device mismatch can be told from a wrong
restatement.
"""
import numpy as np
import scipy.ndimage as ndi

NDI_MODE = {"reflect": "mirror", "edge": "nearest"}
PAD = 12                              # scipy pre-pads by 12 edge samples per side before the spline prefilter of mode 'nearest'
POLE = np.sqrt(3.0) - 2.0

# (shape, scale, order, mode, anti_aliasing) -- the cases of the issue, CPU and GPU alike
DOWN_LINEAR = [((25, 19), 0.5), ((64, 64), 0.5), ((7, 5), 0.5), ((3, 4), 0.25)]
CASES = [(s, f, 1, m, True) for m in ("reflect", "edge") for s, f in DOWN_LINEAR] + \
        [(s, 3, 3, "edge", False) for s in ((5, 4), (11, 7), (16, 16))] + \
        [((11, 7), 3, 3, "reflect", False), ((25, 19), 0.5, 3, "reflect", True)]
CASE_IDS = [f"{s[0]}x{s[1]}-x{f}-o{o}-{m}-{'aa' if aa else 'noaa'}" for s, f, o, m, aa in CASES]
BOUND = 2e-7                          # of max|in|: fp64 arithmetic rounded once to fp32 errs by <= 6e-8 of the value


def out_shape(shape, scale):
    return tuple(int(v) for v in np.round(np.asarray(shape, dtype=np.float64) * scale))      # half to even, as skimage


def case_image(shape, seed=0):
    """fp32-representable values (what the device entry points take), as float64."""
    return np.random.default_rng(seed).random(shape).astype(np.float32).astype(np.float64)


def scipy_resize(img, out_hw, order=1, mode="reflect", anti_aliasing=None, clip=True, clip_range=None):
    img = np.asarray(img, dtype=np.float64)
    f = np.asarray(img.shape, dtype=np.float64) / np.asarray(out_hw, dtype=np.float64)
    if anti_aliasing is None:
        anti_aliasing = bool(np.any(f > 1))
    m = NDI_MODE[mode]
    filtered = ndi.gaussian_filter(img, np.maximum(0, (f - 1) / 2), mode=m) if anti_aliasing else img
    out = ndi.zoom(filtered, 1 / f, order=order, mode=m, grid_mode=True)
    assert out.shape == tuple(out_hw)
    if clip:
        lo, hi = clip_range if clip_range is not None else (img.min(), img.max())
        out = np.clip(out, lo, hi)
    return out


def _index(i, n, mode):
    if mode == "edge":
        return np.clip(i, 0, n - 1)
    if n <= 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.mod(i, period)
    return np.where(i < n, i, period - i)


def _gauss_axis0(a, sigma, mode):
    if sigma <= 0:
        return a
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    w /= w.sum()
    n = a.shape[0]
    out = np.zeros_like(a)
    for k, wk in zip(x, w):
        out += wk * a[_index(np.arange(n) + k, n, mode)]
    return out


def _prefilter_axis0(c):
    """The cubic B-spline prefilter along axis 0 with scipy's mirror start (ni_splines.c)."""
    n = c.shape[0]
    if n <= 1:
        return c
    z = POLE
    c = c * ((1 - z) * (1 - 1 / z))
    zn = z ** (n - 1)
    c0 = c[0] + zn * c[n - 1]
    zi = z
    for i in range(1, n - 1):
        c0 = c0 + zi * (c[i] + zn * c[n - 1 - i])
        zi *= z
    c[0] = c0 / (1 - zn * zn)
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def _bspline3(t):
    return np.stack([(1 - t) ** 3 / 6, (4 - 6 * t ** 2 + 3 * t ** 3) / 6, (1 + 3 * t + 3 * t ** 2 - 3 * t ** 3) / 6, t ** 3 / 6])


def _sample_axis0(c, n_in, n_out, order, mode, pad):
    x = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5 + pad
    i0 = np.floor(x).astype(np.int64)
    t = (x - i0).reshape((-1,) + (1,) * (c.ndim - 1))
    n = c.shape[0]
    if order == 1:
        return (1 - t) * c[_index(i0, n, mode)] + t * c[_index(i0 + 1, n, mode)]
    w = _bspline3(t)
    return sum(w[k] * c[_index(i0 - 1 + k, n, mode)] for k in range(4))


def restated_resize(img, out_hw, order=1, mode="reflect", anti_aliasing=None, clip=True, clip_range=None):
    img = np.asarray(img, dtype=np.float64)
    (h, w), (oh, ow) = img.shape, out_hw
    f = (h / oh, w / ow)
    if anti_aliasing is None:
        anti_aliasing = f[0] > 1 or f[1] > 1
    a = img
    if anti_aliasing:
        a = _gauss_axis0(a, max(0.0, (f[0] - 1) / 2), mode)
        a = _gauss_axis0(a.T, max(0.0, (f[1] - 1) / 2), mode).T
    pad = 0
    if order == 3:
        pad = PAD if mode == "edge" else 0
        a = np.pad(a, pad, mode="edge") if pad else a.copy()
        a = _prefilter_axis0(a)
        a = _prefilter_axis0(np.ascontiguousarray(a.T)).T
    out = _sample_axis0(a, h, oh, order, mode, pad)
    out = _sample_axis0(np.ascontiguousarray(out.T), w, ow, order, mode, pad).T
    if clip:
        lo, hi = clip_range if clip_range is not None else (img.min(), img.max())
        out = np.clip(out, lo, hi)
    return out
