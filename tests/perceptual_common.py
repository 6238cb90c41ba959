"""The reader study's scores restated in float64 NumPy / SciPy from their DEFINITIONS, independently of the kernels:
MATLAB's documented defaults for ``ssim``, ``immse``, ``imfilter`` and ``fspecial('unsharp')``, and Wang et al. 2003 for MS-SSIM.
Nothing here was ever compared with MATLAB output.  The Gaussian window runs through ``scipy.ndimage.correlate1d(mode='nearest')``
(edge replicated), the 3 x 3 filter through ``scipy.ndimage.correlate(mode='constant')`` (zero padding).  One image per call."""
import math
import os

import numpy as np
from scipy import ndimage

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reader_study_crops.npz")


def gauss_window(sigma):
    r = int(math.ceil(3.0 * sigma))
    k = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-k ** 2 / (2.0 * sigma ** 2))
    return g / g.sum()


def smooth(img, g):
    """rows, then columns; out-of-range indices clamped to the edge"""
    return ndimage.correlate1d(ndimage.correlate1d(img, g, axis=0, mode="nearest"), g, axis=1, mode="nearest")


def ssim_parts(x, y, sigma=1.5, data_range=1.0):
    """(the maps l and cs) of two 2-D images, float64"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    g = gauss_window(sigma)
    mx, my = smooth(x, g), smooth(y, g)
    vx = np.maximum(smooth(x * x, g) - mx * mx, 0.0)
    vy = np.maximum(smooth(y * y, g) - my * my, 0.0)
    vxy = smooth(x * y, g) - mx * my
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    return (2 * mx * my + c1) / (mx * mx + my * my + c1), (2 * vxy + c2) / (vx + vy + c2)


def ssim_gauss(x, y, sigma=1.5, data_range=1.0):
    """(score, mean of cs, map)"""
    l, cs = ssim_parts(x, y, sigma, data_range)
    return float((l * cs).mean()), float(cs.mean()), l * cs


def down2(img):
    """2 x 2 block means with the indices clamped: ceil(H/2) x ceil(W/2)"""
    h, w = img.shape
    i0, j0 = np.arange(0, h, 2), np.arange(0, w, 2)
    i1, j1 = np.minimum(i0 + 1, h - 1), np.minimum(j0 + 1, w - 1)
    return 0.25 * (img[np.ix_(i0, j0)] + img[np.ix_(i0, j1)] + img[np.ix_(i1, j0)] + img[np.ix_(i1, j1)])


def ms_ssim(x, y, weights=MS_SSIM_WEIGHTS, sigma=1.5, data_range=1.0):
    """(score, the per-scale values); a negative value under a fractional weight gives NaN, as numpy's power does"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    vals = []
    for s in range(len(weights)):
        if s:
            x, y = down2(x), down2(y)
        l, cs = ssim_parts(x, y, sigma, data_range)
        vals.append((l * cs).mean() if s == len(weights) - 1 else cs.mean())
    vals = np.array(vals, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return float(np.prod(np.power(vals, np.asarray(weights, dtype=np.float64)))), vals


def unsharp_kernel(alpha=0.2):
    a = float(alpha)
    return np.array([[-a, a - 1, -a], [a - 1, a + 5, a - 1], [-a, a - 1, -a]], dtype=np.float64) / (a + 1)


def filter3x3(img, k):
    """3 x 3 correlation, zero padding, float64 (the device rounds this once to fp32)"""
    return ndimage.correlate(np.asarray(img, dtype=np.float32).astype(np.float64), np.asarray(k, dtype=np.float64), mode="constant",
                             cval=0.0)


def hpf(img, alpha=0.2):
    """as the device returns it: rounded to fp32"""
    return filter3x3(img, unsharp_kernel(alpha)).astype(np.float32)


def mse(x, y):
    d = np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64)
    return float((d * d).mean())


def hf_gain(h_sr, h_inter):
    a, b = np.asarray(h_sr, dtype=np.float64), np.asarray(h_inter, dtype=np.float64)
    return float((np.maximum(a - b, 0.0) ** 2).sum() / (b ** 2).sum())


def reader_study_scores(inter, sr, base, data_range, hpf_data_range):
    """the keys of perceptual.reader_study_scores for ONE slice"""
    out = {}
    hi, hs, hb = hpf(inter), hpf(sr), hpf(base)
    for filt, a_i, a_s, ref, rng in (("raw", inter, sr, base, data_range), ("hpf", hi, hs, hb, hpf_data_range)):
        for panel, a in (("interpolated", a_i), ("SR", a_s)):
            out[f"ssim_{filt}_{panel}"] = ssim_gauss(a, ref, data_range=rng)[0]
            out[f"mse_{filt}_{panel}"] = mse(a, ref)
            out[f"ms_ssim_{filt}_{panel}"] = ms_ssim(a, ref, data_range=rng)[0]
    out["hf_gain"] = hf_gain(hs, hi)
    return out


def smooth_noisy(shape, seed, noise=0.05):
    """smooth positive images (values in 0.2 .. 0.8) plus `noise` of uniform noise, and second copies with independent noise; fp32"""
    rng = np.random.default_rng(seed)
    h, w = shape[-2], shape[-1]
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    xs, ys = [], []
    for _ in range(int(np.prod(shape[:-2], dtype=np.int64))):
        p = rng.random(3) * 6.0
        base = 0.5 + 0.2 * np.sin(5 * xx + p[0]) * np.cos(7 * yy + p[1]) + 0.1 * np.sin(3 * (xx + yy) + p[2])
        xs.append(base + noise * rng.random((h, w)))
        ys.append(base + noise * rng.random((h, w)))
    return np.stack(xs).reshape(shape).astype(np.float32), np.stack(ys).reshape(shape).astype(np.float32)
