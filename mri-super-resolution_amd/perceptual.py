"""The reader study's image scores on the device, through libinrhip.so (csrc/perceptual.hip).

The reference scores the panels of prepare_qual_images.py in MATLAB
(implicit-neural-representations/perceptual_similarity_tests/perceptual_similarity.m, HPF.m): ``ssim``, ``immse`` and ``multissim`` of
``interpolated`` and of ``SR`` against ``base``, on the images and on their 3 x 3 high-passed versions, and a high-frequency gain.
This module computes the same scores by the definitions of DESIGN.md 4g -- MATLAB's documented defaults for ``ssim``, ``immse``,
``imfilter`` and ``fspecial('unsharp')``, and Wang et al. 2003 for MS-SSIM.  No MATLAB output was ever compared against: parity with
MATLAB is UNPINNED; the kernels are pinned against the float64 NumPy / SciPy restatement of those definitions
(tests/perceptual_common.py).  FSIM and SR-SIM (perceptual_similarity.m:53-54) are third-party files under a research-only licence
and are not part of this project.

``ssim_gauss`` is NOT ``metrics.ssim``: Gaussian window (radius ``ceil(3 sigma)``, edge replicated), the full image, the biased
variance -- against skimage's uniform window, cropped border and sample covariance.

Inputs are device fp32 tensors (trailing two axes an image, leading axes a batch) and results float64 device tensors, with no host
sync inside; an ndarray in gives an ndarray out, as ``baselines.resize`` does.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import ops
from ._lib import check, lib

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang et al. 2003; multissim's default

__all__ = ["ssim_gauss", "ms_ssim", "hpf", "filter3x3", "unsharp_kernel", "mse", "hf_gain", "reader_study_scores"]


def _images(image, name):
    """(flat [n, H, W] device fp32 tensor, leading shape, was it an ndarray)"""
    as_numpy = isinstance(image, np.ndarray)
    x = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(ops.require_gpu()) if as_numpy else image
    if not as_numpy and isinstance(x, torch.Tensor) and x.is_cuda:
        x = x.contiguous()
    ops._chk(x, name)
    if x.data_ptr() % 16:                    # a view into a batch: the entry points take 16-byte aligned pointers
        x = x.clone()
    if x.dim() < 2:
        raise ValueError(f"{name} must be at least 2-D")
    h, w = int(x.shape[-2]), int(x.shape[-1])
    if h < 1 or w < 1 or x.numel() == 0:
        raise ValueError(f"{name}: empty image ({tuple(x.shape)})")
    return x.reshape(-1, h, w), tuple(x.shape[:-2]), as_numpy


def _pair(x, y, xname="x", yname="y"):
    fx, lead, as_numpy = _images(x, xname)
    fy, _, _ = _images(y, yname)
    if fx.shape != fy.shape:
        raise ValueError(f"{xname} {tuple(fx.shape)} / {yname} {tuple(fy.shape)} shape mismatch")
    return fx, fy, lead, as_numpy


def _out(t, lead, as_numpy, tail=()):
    t = t.reshape(tuple(lead) + tuple(tail))
    return t.cpu().numpy() if as_numpy else t


def _workspace(n, h, w, scales, device):
    need = lib().inr_perceptual_workspace_doubles(n, h, w, scales)
    if need == 0:
        raise ValueError(lib().inr_last_error().decode("utf-8", "replace"))
    return torch.empty(int(need), dtype=torch.float64, device=device)


def ssim_gauss(x, y, sigma: float = 1.5, data_range: float = 1.0, return_cs: bool = False, return_map: bool = False):
    """Gaussian-window SSIM per image (MATLAB ``ssim(A, ref)`` by its documented defaults, perceptual_similarity.m:50): the mean
    of ``l * cs`` over the full image.  ``return_cs`` adds the mean of ``cs``, ``return_map`` the fp32 map ``[..., H, W]``; the
    result is then a tuple in that order."""
    fx, fy, lead, as_numpy = _pair(x, y)
    n, h, w = fx.shape
    score = torch.empty(n, dtype=torch.float64, device=fx.device)
    cs = torch.empty(n, dtype=torch.float64, device=fx.device) if return_cs else None
    smap = torch.empty((n, h, w), dtype=torch.float32, device=fx.device) if return_map else None
    ws = _workspace(n, h, w, 1, fx.device)
    check(lib().inr_ssim2d_gauss(score.data_ptr(), ops._ptr(cs), ops._ptr(smap), fx.data_ptr(), fy.data_ptr(), n, h, w, float(sigma),
                                 float(data_range), ws.data_ptr(), ws.numel(), ops._stream()), "inr_ssim2d_gauss")
    res = [_out(score, lead, as_numpy)]
    if return_cs:
        res.append(_out(cs, lead, as_numpy))
    if return_map:
        res.append(_out(smap, lead, as_numpy, (h, w)))
    return res[0] if len(res) == 1 else tuple(res)


def ms_ssim(x, y, weights=MS_SSIM_WEIGHTS, sigma: float = 1.5, data_range: float = 1.0, return_per_scale: bool = False):
    """Multi-scale SSIM per image (Wang et al. 2003; MATLAB ``multissim``, perceptual_similarity.m:52): ``prod v_s ** w_s`` with
    ``v_s`` the mean of ``cs`` at every scale but the last and the mean of ``l * cs`` at the last; 2 x 2 block means between scales.
    A non-positive ``v_s`` under a fractional weight gives NaN.  ``return_per_scale`` adds the ``v_s`` as ``[..., len(weights)]``."""
    fx, fy, lead, as_numpy = _pair(x, y)
    n, h, w = fx.shape
    wts = [float(v) for v in weights]
    if not 1 <= len(wts) <= 8:
        raise ValueError(f"ms_ssim: 1 to 8 scales (got {len(wts)})")
    out = torch.empty(n, dtype=torch.float64, device=fx.device)
    per = torch.empty((n, len(wts)), dtype=torch.float64, device=fx.device) if return_per_scale else None
    ws = _workspace(n, h, w, len(wts), fx.device)
    check(lib().inr_msssim2d(out.data_ptr(), ops._ptr(per), fx.data_ptr(), fy.data_ptr(), n, h, w, (C.c_double * len(wts))(*wts),
                             len(wts), float(sigma), float(data_range), ws.data_ptr(), ws.numel(), ops._stream()), "inr_msssim2d")
    if return_per_scale:
        return _out(out, lead, as_numpy), _out(per, lead, as_numpy, (len(wts),))
    return _out(out, lead, as_numpy)


def unsharp_kernel(alpha: float = 0.2) -> np.ndarray:
    """MATLAB's ``fspecial('unsharp', alpha)`` (HPF.m:5 takes the default 0.2), coefficients formed in double."""
    a = float(alpha)
    return np.array([[-a, a - 1, -a], [a - 1, a + 5, a - 1], [-a, a - 1, -a]], dtype=np.float64) / (a + 1)


def filter3x3(image, k):
    """``imfilter(single(image), k)`` for a 3 x 3 ``k``: correlation, zero padding, same size; fp64 sums rounded once to fp32."""
    k = np.ascontiguousarray(k, dtype=np.float64)
    if k.shape != (3, 3):
        raise ValueError(f"filter3x3: the kernel must be 3 x 3 (got {k.shape})")
    fx, lead, as_numpy = _images(image, "image")
    n, h, w = fx.shape
    out = torch.empty_like(fx)
    check(lib().inr_filter3x3(out.data_ptr(), fx.data_ptr(), n, h, w, (C.c_double * 9)(*k.reshape(-1).tolist()), ops._stream()),
          "inr_filter3x3")
    return _out(out, lead, as_numpy, (h, w))


def hpf(image, alpha: float = 0.2):
    """``HPF(image)`` of the reference (HPF.m): ``imfilter(single(image), fspecial('unsharp'))``."""
    return filter3x3(image, unsharp_kernel(alpha))


def _pair_score(entry, name, x, y):
    fx, fy, lead, as_numpy = _pair(x, y)
    n, h, w = fx.shape
    out = torch.empty(n, dtype=torch.float64, device=fx.device)
    ws = _workspace(n, 1, 1, 1, fx.device)
    check(entry(out.data_ptr(), fx.data_ptr(), fy.data_ptr(), n, h * w, ws.data_ptr(), ws.numel(), ops._stream()), name)
    return _out(out, lead, as_numpy)


def mse(x, y):
    """``immse(x, y)`` per image: the mean of ``(x - y) ** 2``."""
    return _pair_score(lib().inr_image_mse, "inr_image_mse", x, y)


def hf_gain(h_sr, h_inter):
    """The high-frequency gain of perceptual_similarity.m:41-47 per image, on HIGH-PASSED images:
    ``sum(max(h_sr - h_inter, 0) ** 2) / sum(h_inter ** 2)``."""
    return _pair_score(lib().inr_hf_gain, "inr_hf_gain", h_sr, h_inter)


def reader_study_scores(inter, sr, base, data_range: float, hpf_data_range: float):
    """Everything perceptual_similarity.m:41-52 computes per slice (but FSIM / SR-SIM), for a batch of slices: a dict with the
    twelve scores ``f"{index}_{filter}_{panel}"`` -- index in ``ssim, mse, ms_ssim``; filter ``raw`` (the images as they are,
    ``data_range``) or ``hpf`` (after ``hpf``, ``hpf_data_range``); panel ``interpolated`` or ``SR``, each against ``base`` -- and
    ``hf_gain``.  ``inter``, ``sr`` and ``base`` share a shape ``[..., H, W]``; every value has the leading shape.  Both panels go
    through each kernel as one batch."""
    fi, fb, lead, as_numpy = _pair(inter, base, "inter", "base")
    fs, _, _, _ = _pair(sr, base, "sr", "base")
    n = fi.shape[0]
    test = torch.cat([fi, fs])                       # [2n, H, W]: interpolated, then SR
    ref = torch.cat([fb, fb])
    high = hpf(torch.cat([test, fb]))
    h_test, h_ref = high[:2 * n].contiguous(), torch.cat([high[2 * n:], high[2 * n:]])
    out = {}
    for filt, a, b, rng in (("raw", test, ref, data_range), ("hpf", h_test, h_ref, hpf_data_range)):
        for index, val in (("ssim", ssim_gauss(a, b, data_range=rng)), ("mse", mse(a, b)), ("ms_ssim", ms_ssim(a, b, data_range=rng))):
            out[f"{index}_{filt}_interpolated"], out[f"{index}_{filt}_SR"] = val[:n], val[n:]
    out["hf_gain"] = hf_gain(h_test[n:], h_test[:n])
    return {k: _out(v.contiguous(), lead, as_numpy) for k, v in out.items()}
