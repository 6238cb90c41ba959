"""Shared by tests/test_metrics_edges_cpu.py and tests/test_gpu_metrics_edges.py: plain float64 restatements of what the kernels
of csrc/metrics.hip compute, and the edge inputs both files use (so that the CPU file can check the conditions the GPU tests lean
on -- the planted clips clip, the fractional mask separates the two bias formulas, the two spline solvers agree -- on the very
inputs the device sees).
"""
import numpy as np

# ---- PSNR ----------------------------------------------------------------------------------------------------------------------
PSNR_SIZES = (1, 255, 257, 16384, 16385, 3 * 16384 + 5)       # one trip of the 64 x 256 grid holds 16,384 pixels
PSNR_BOUND = 1e-9                                             # dB, absolute (tests/test_gpu_metrics.py)


def psnr64(x, y, data_range):
    """10 log10(R^2 / mean((x - y)^2)) in float64 on the values given; +inf for identical inputs, as NumPy gives."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(divide="ignore"):
        return float(10.0 * np.log10(float(data_range) ** 2 / np.mean((x - y) ** 2)))


def psnr_pair(n, data_range, seed, noise=0.01):
    """Two fp32 vectors of n values in [0, data_range], the second one the first plus Gaussian noise of `noise` * data_range."""
    rng = np.random.default_rng(seed)
    x = (rng.random(n) * data_range).astype(np.float32)
    y = (x + noise * data_range * rng.standard_normal(n)).astype(np.float32)
    return x, y


# ---- SSIM ----------------------------------------------------------------------------------------------------------------------
SSIM_BOUND = 1e-10                                            # absolute (tests/test_gpu_metrics.py)
# (shape, win): 144 x 125 = 18,000 cropped pixels exceed one trip of the grid; one cropped pixel; one cropped row, twice
SSIM_SHAPES = [((150, 131), 3), ((150, 131), 7), ((150, 131), 11), ((7, 7), 7), ((7, 40), 7), ((3, 200), 3)]
SSIM_RANGES = [(1.0, 1.0), (4000.0, 4000.0), (60000.0, 65535.0)]       # (largest intensity, data_range)


def ssim_pair(shape, top, seed):
    """fp32 images in [0, top]: smooth structure plus noise, and a noisier copy."""
    rng = np.random.default_rng(seed)
    h, w = shape[-2:]
    gy, gx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    base = 0.5 + 0.3 * np.sin(7 * gx + 3 * gy) * np.cos(5 * gy)
    x = np.clip(base + 0.1 * rng.standard_normal(shape), 0, 1) * top
    y = np.clip(x / top + 0.05 * rng.standard_normal(shape), 0, 1) * top
    return x.astype(np.float32), y.astype(np.float32)


def ssim_window_sums(x, y, data_range, win=7, mask_threshold=None):
    """skimage-0.20 structural_similarity defaults in the direct form: the five sums over every win x win window, the sample
    covariance (N / (N - 1)), K1 = 0.01, K2 = 0.03, the mean over the windows that fit.  With `mask_threshold` both images are
    multiplied by (x > threshold) first."""
    from numpy.lib.stride_tricks import sliding_window_view
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if mask_threshold is not None:
        m = (x > mask_threshold).astype(np.float64)
        x, y = x * m, y * m
    n = float(win * win)

    def s(a):
        return sliding_window_view(a, (win, win)).sum(axis=(-1, -2))

    ux, uy = s(x) / n, s(y) / n
    cov = n / (n - 1.0)
    vx, vy, vxy = cov * (s(x * x) / n - ux * ux), cov * (s(y * y) / n - uy * uy), cov * (s(x * y) / n - ux * uy)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    return float((((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))).mean())


# ---- ADC -----------------------------------------------------------------------------------------------------------------------
ADC_NB = (2, 3, 32)
ADC_PIXELS = (1, 255, 256, 257)
ADC_ULP = 1             # fp32 ULPs: the two libraries' fp64 log may differ by 1 fp64 ULP, which can move the fp32 rounding one step
CLIP_BVALS = (0.0, 900.0)
CLIP_DATA = np.array([[1000.0, 1e-3], [1e-3, 1000.0]], np.float32)      # -slope = +-15.35: clipped to 3 and to -10


def adc_case(n_b, npix, seed):
    """(bvals [n_b], data [npix, n_b]) fp32: a mono-exponential decay with D in [0.5, 2.5] um^2/ms and 3 % noise, so that the
    slope is of order one (the fp32 ULP of the result is then far above the fp64 rounding of the sums)."""
    rng = np.random.default_rng(seed)
    b = np.linspace(0.0, 1500.0, n_b).astype(np.float32)
    d = rng.uniform(0.5, 2.5, (npix, 1))
    s0 = rng.uniform(200.0, 1200.0, (npix, 1))
    data = s0 * np.exp(-b.astype(np.float64) / 1000.0 * d) * (1 + 0.03 * rng.standard_normal((npix, n_b)))
    return b, data.astype(np.float32)


def ulp32_distance(a, b):
    """Element-wise distance in fp32 ULPs; 0 where both are NaN, 2^31 where only one is."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)

    def ordered(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(2 ** 31) - i, i)

    d = np.abs(ordered(a) - ordered(b))
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na & nb, 0, np.where(na ^ nb, 2 ** 31, d))


# ---- shift-tolerant losses -----------------------------------------------------------------------------------------------------
# (images, size, border): one shift; a one-pixel crop; 33 x 33 = 1,089 shifts; a 17 x 17 = 289-pixel crop (a ragged second trip of
# the 256-thread loop); a second, ragged block of the 64-thread finish kernels
SHIFT_CASES = [(3, 5, 0), (3, 3, 1), (2, 40, 16), (2, 23, 3), (65, 12, 3)]
SHIFT_LOSS_RTOL = 1e-9
SHIFT_GRAD_REL = 1e-6                                          # of max|gradient|


def shift_case(nimg, size, border, seed):
    """(y_true, y_pred, mask) fp32 [nimg, size, size]; the mask takes the values 0, 0.5 and 1 (0.5 and 1 alone where the crop is
    a single pixel: a crop whose mask sums to 0 has no loss)."""
    rng = np.random.default_rng(seed)
    shape = (nimg, size, size)
    y_true = (rng.random(shape) * 30000 + 5000).astype(np.float32)
    y_pred = (np.roll(y_true, (-1, 1), axis=(1, 2)) * 1.02 - 90 + rng.standard_normal(shape) * 40).astype(np.float32)
    levels = (0.5, 1.0) if size - 2 * border == 1 else (0.0, 0.5, 1.0)
    mask = rng.choice(np.asarray(levels, np.float32), size=shape, p=(0.5, 0.5) if len(levels) == 2 else (0.2, 0.3, 0.5))
    if len(levels) == 2:
        mask[0] = 0.5             # no shift with m = 1, whose loss would be an exact 0 under either bias formula
    return y_true, y_pred, mask.astype(np.float32)


def shift_losses_bias_outside_mask(y_true, y_pred, y_mask, size, border):
    """The WRONG formula m (pred + b) in place of the reference's m (m pred + b) (oracle/rams_port.shift_losses): equal for a
    mask of zeros and ones, different for a fractional one.  Here so that the CPU test can show the inputs tell them apart."""
    yt, yp, mk = (np.asarray(a, np.float64) for a in (y_true, y_pred, y_mask))
    c = size - 2 * border
    pred = yp[:, border:size - border, border:size - border]
    l1s = []
    for i in range(2 * border + 1):
        for j in range(2 * border + 1):
            lab, m = yt[:, i:i + c, j:j + c], mk[:, i:i + c, j:j + c]
            tot = m.sum(axis=(1, 2))
            b = ((lab * m - pred * m).sum(axis=(1, 2)) / tot)[:, None, None]
            l1s.append(np.abs(lab * m - (pred + b) * m).sum(axis=(1, 2)) / tot)
    return np.min(np.stack(l1s), axis=0)


def shift_l1_and_grad(y_true, y_pred, y_mask, size, border, upstream=None):
    """float64 (loss [B], d sum(upstream * loss) / d y_pred [B, size, size]) by autograd on oracle/rams_port.shift_l1_torch."""
    import torch

    from oracle import rams_port as R
    yt, mk = torch.from_numpy(np.asarray(y_true, np.float64)), torch.from_numpy(np.asarray(y_mask, np.float64))
    yp = torch.from_numpy(np.asarray(y_pred, np.float64)).requires_grad_(True)
    loss = R.shift_l1_torch(yt, yp, mk, size, border)
    up = torch.ones(loss.shape[0], dtype=torch.float64) if upstream is None else torch.from_numpy(np.asarray(upstream, np.float64))
    (loss * up).sum().backward()
    return loss.detach().numpy(), yp.grad.numpy()


# ---- linear up-scale -----------------------------------------------------------------------------------------------------------
def zoom_linear(img, out_hw):
    """scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True) in float64: what skimage 0.20 resize computes when up-scaling."""
    import scipy.ndimage as ndi
    img = np.asarray(img, np.float64)
    out = ndi.zoom(img, (out_hw[0] / img.shape[0], out_hw[1] / img.shape[1]), order=1, mode="mirror", grid_mode=True)
    assert out.shape == tuple(out_hw), out.shape
    return out


# ---- through-plane spline ------------------------------------------------------------------------------------------------------
SPLINE_BOUND = 1e-12                                          # tests/test_gpu_through_plane.py (n_in <= 128)
SPLINE_E0_LIMIT = 4 * 2.5e-13                                 # the restatement against scipy at n_in = 8192


def spline_lines(n_lines, n_in, seed):
    return np.random.default_rng(seed).random((n_lines, n_in))


def scipy_cubic(lines, n_out):
    from scipy.interpolate import interp1d
    lines = np.asarray(lines, np.float64)
    return interp1d(np.linspace(0, 1, lines.shape[-1]), lines, kind="cubic", axis=-1)(np.linspace(0, 1, n_out))


def thomas_cubic(lines, n_out):
    """The recurrence of resize_z_cubic_kernel in float64 NumPy, all lines at once: with c_i = h^2 s''(x_i), rows 1 and n - 2 of
    the not-a-knot system read 6 c_i = 6 D_i, the rows between c_{i-1} + 4 c_i + c_{i+1} = 6 D_i (D_i the second difference);
    Thomas elimination with the shared factor cp, back substitution, the two end values by extrapolation, then the evaluation
    at linspace(0, 1, n_out)."""
    y = np.asarray(lines, np.float64)
    n = y.shape[-1]
    last = n - 2
    cp = np.zeros(n)
    for i in range(2, last):
        cp[i] = 1.0 / (4.0 - cp[i - 1])
    d = np.zeros_like(y)
    d[:, 1:-1] = y[:, :-2] - 2.0 * y[:, 1:-1] + y[:, 2:]
    c = np.zeros_like(y)
    c[:, 1] = d[:, 1]
    for i in range(2, last):
        c[:, i] = (6.0 * d[:, i] - c[:, i - 1]) * cp[i]
    c[:, last] = d[:, last]
    for i in range(last - 1, 0, -1):
        c[:, i] -= cp[i] * c[:, i + 1]
    c[:, 0] = 2.0 * c[:, 1] - c[:, 2]
    c[:, last + 1] = 2.0 * c[:, last] - c[:, last - 1]
    step = 1.0 / (n_out - 1) if n_out > 1 else 0.0
    u = np.arange(n_out) * step
    if n_out > 1:
        u[-1] = 1.0
    u = u * float(n - 1)
    j = np.clip(np.floor(u).astype(np.int64), 0, n - 2)
    a = u - j
    b = 1.0 - a
    return b * y[:, j] + a * y[:, j + 1] + ((b * b * b - b) * c[:, j] + (a * a * a - a) * c[:, j + 1]) / 6.0


# ---- per-slice AutoERD on non-finite pixels --------------------------------------------------------------------------------------
BAD_PIXELS = (5, 9, 40, 66)                                   # 66: a lane of the second, ragged 64-pixel block
OVERFLOW_PIXEL = 30                                           # finite values whose largest distance overflows


def plant_non_finite(clean):
    """[70, 12] -> a copy with NaN, +inf and -inf planted as tests/test_gpu_erd_volume.py plants them."""
    x = np.array(clean, np.float64, copy=True)
    x[5, 3] = np.nan
    x[9, 0] = np.inf
    x[40, 11] = -np.inf
    x[66, 7] = np.nan
    return x


def plant_overflow(clean):
    x = np.array(clean, np.float64, copy=True)
    x[OVERFLOW_PIXEL, :] = 1e308
    x[OVERFLOW_PIXEL, 1::3] = -1e308
    x[OVERFLOW_PIXEL, 2] = 3.0
    return x
