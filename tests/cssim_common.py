"""Float64 restatement of the shift-tolerant SSIM (cSSIM) of multi-image-super-resolution/utils/loss.py:131-177, with
``tf.image.ssim`` written out from its public definition (11 x 11 Gaussian window of sigma 1.5 as a 'VALID' correlation,
K1 = 0.01, K2 = 0.03, no sample-covariance correction).  One implementation, written with operators and slices only, serves NumPy
arrays (values) and torch float64 tensors (autograd).  TensorFlow is not available, so this restatement -- not the reference's own
output -- is what the kernels are pinned to; test_cssim_cpu.py pins the restatement itself to cases with known answers."""
import numpy as np

BORDER = 3
MAX_VAL = 65535.0
C1 = (0.01 * MAX_VAL) ** 2
C2 = (0.03 * MAX_VAL) ** 2


def gauss_window():
    k = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-k * k / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def gauss_filter(a):
    """'VALID' correlation of the last two axes with the 11 x 11 window (the outer product of ``gauss_window()``)."""
    g = [float(v) for v in gauss_window()]
    n = a.shape[-1] - 10
    rows = sum(g[k] * a[..., :, k:k + n] for k in range(11))
    m = a.shape[-2] - 10
    return sum(g[k] * rows[..., k:k + m, :] for k in range(11))


def ssim_tf(x, y):
    """tf.image.ssim(x, y, max_val=65535) for [..., H, W] float64 -> [...]"""
    mx, my = gauss_filter(x), gauss_filter(y)
    lum = (2.0 * mx * my + C1) / (mx * mx + my * my + C1)
    cs = (2.0 * gauss_filter(x * y) - 2.0 * mx * my + C2) / (gauss_filter(x * x + y * y) - mx * mx - my * my + C2)
    return (lum * cs).mean((-2, -1))


def _shift_values(y_true, y_pred, mask, size, clear_only):
    """The 49 per-shift cSSIM vectors ([B] each), shift (i, j) at position 7 i + j."""
    c = size - 2 * BORDER
    pred = y_pred[:, BORDER:size - BORDER, BORDER:size - BORDER]
    out = []
    for i in range(2 * BORDER + 1):
        for j in range(2 * BORDER + 1):
            lab, m = y_true[:, i:i + c, j:j + c], mask[:, i:i + c, j:j + c]
            tot = m.sum((1, 2))
            b = ((lab * m - pred * m).sum((1, 2)) / tot)[:, None, None]
            x = (pred * m + b) * m
            y = lab * m
            s = ssim_tf(x, y)
            if clear_only:
                s = (s - 1.0) * tot / (c * c) + 1.0
            out.append(s)
    return out


def cssim_table(y_true, y_pred, mask, size, clear_only=False):
    """NumPy float64: the per-shift table [B, 7, 7]."""
    f = lambda a: np.asarray(a, np.float64)
    vals = _shift_values(f(y_true), f(y_pred), f(mask), size, clear_only)
    return np.stack(vals, axis=1).reshape(-1, 2 * BORDER + 1, 2 * BORDER + 1)


def cssim_per_image(y_true, y_pred, mask, size, clear_only=False):
    return cssim_table(y_true, y_pred, mask, size, clear_only).reshape(len(y_true), -1).max(axis=1)


def cssim_loss_torch(y_true, y_pred, mask, size, clear_only=False):
    """torch float64, differentiable in ``y_pred``: loss[b] = 1 - max over the shifts."""
    import torch
    vals = _shift_values(y_true.double(), y_pred.double(), mask.double(), size, clear_only)
    return 1.0 - torch.stack(vals, dim=1).max(dim=1).values


def planted_case(seed, B, size, roll=(1, -2), gain=0.97, offset=150.0, noise=30.0, masked=0.15, soft_mask=False):
    """Inputs in the manner of test_shift_tolerant_losses_match_oracle: uint16-range labels, the prediction = the label rolled by
    a planted shift, scaled, offset and noised; about ``masked`` of the pixels masked out (``soft_mask``: the clear ones carry
    weights in [0.25, 1] instead of 1)."""
    rng = np.random.default_rng(seed)
    y_true = (rng.random((B, size, size)) * 40000 + 2000).astype(np.float32)
    y_pred = (np.roll(y_true, roll, axis=(1, 2)) * gain + offset + rng.standard_normal((B, size, size)) * noise).astype(np.float32)
    clear = rng.random((B, size, size)) > masked
    weight = 0.25 + 0.75 * rng.random((B, size, size)) if soft_mask else 1.0
    return y_true, y_pred, (clear * weight).astype(np.float32)
