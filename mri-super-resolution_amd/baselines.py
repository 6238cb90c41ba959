"""The interpolation baselines the reference reports its results against, on the device.

``rescale`` is ``skimage.transform.rescale(image, scale, anti_aliasing=True)`` as called at superresDWI.py:172-191 and
master.py:175 for up-scaling 2-D images: default order 1, mode 'reflect' -- which skimage 0.20 evaluates as
``scipy.ndimage.zoom(image, scale, order=1, mode='mirror', grid_mode=True)``; the anti-aliasing Gaussian has sigma
``max(0, (1/scale - 1)/2) = 0`` when ``scale >= 1``.  scikit-image itself is not installed in the build image: parity with
skimage is therefore UNPINNED; the kernel is pinned against the scipy call skimage makes (tests).  ``rescale`` serves
``scale >= 1`` only and refuses the rest, as it always has.

``resize`` and ``rescale2d`` are skimage 0.20's ``resize`` / ``rescale`` for 2-D images in full (``inr_rescale2d``): the
anti-aliasing Gaussian of a down-scale (``scipy.ndimage.gaussian_filter(img, max(0, (f - 1)/2))``, ``f = in/out`` from the rounded
shapes), orders 1 and 3 (``scipy.ndimage.zoom(., 1/f, order, grid_mode=True)``, the cubic with scipy's B-spline prefilter), modes
'reflect' (scipy 'mirror') and 'edge' (scipy 'nearest'), and the clip to the input's range.  They serve
``rescale(x, .5, anti_aliasing=True)`` of prepare_qual_images.py:152,198,207,267 and ``bicubic`` of
multi-image-super-resolution/utils/preprocessing.py:271-294.  Pinned to that scipy composition, like ``rescale``; skimage itself
is not.

``resize_z`` is ``resize_array(arr, new_size, kind='cubic')`` (SRDWI.py:132-141), the through-plane baseline of
superresDWI.py:231: scipy's ``interp1d(kind='cubic')`` -- a not-a-knot cubic spline -- along the last axis, in fp64
(``inr_resize_z_cubic``).

``fourier_resize``, ``fourier_rescale``, ``fourier_resample`` and ``fourier_operator`` are not the reference's: they re-sample in
k-space (zero-fill up, truncation down), the interpolation an MR scanner applies and the definition of
``scipy.signal.resample``, with a mirrored boundary so that a cropped region does not wrap around (``inr_fourier_resample2d``,
DESIGN.md 4j).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, lib


def rescale(image, scale, anti_aliasing: bool = True):
    """Up-scales the trailing two axes of ``image`` (ndarray or device tensor; leading axes are a batch) by ``scale``.
    Returns the type it was given (ndarray in -> float64 ndarray out, like skimage; tensor in -> fp32 device tensor)."""
    if scale < 1:
        raise ValueError("rescale: only up-scaling (scale >= 1) is implemented -- the drivers never down-scale")
    as_numpy = isinstance(image, np.ndarray)
    x = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(ops.require_gpu()) if as_numpy else image
    ops._chk(x, "image")
    if x.dim() < 2:
        raise ValueError("rescale needs at least 2-D input")
    h, w = x.shape[-2], x.shape[-1]
    oh, ow = int(round(h * scale)), int(round(w * scale))        # skimage: np.round(scale * input_shape)
    flat = x.reshape(-1, h, w).contiguous()
    out = torch.empty((flat.shape[0], oh, ow), dtype=torch.float32, device=x.device)
    check(lib().inr_rescale2d_linear(out.data_ptr(), flat.data_ptr(), flat.shape[0], h, w, oh, ow, ops._stream()),
          "inr_rescale2d_linear")
    out = out.reshape(*x.shape[:-2], oh, ow)
    return out.cpu().numpy().astype(np.float64) if as_numpy else out


_MODES = {"reflect": 0, "edge": 1}       # INR_RESCALE_REFLECT, INR_RESCALE_EDGE (include/inrhip.h)


def _resize(who, image, out_hw, order, mode, anti_aliasing, clip, group_axes=None):
    """The trailing two axes of ``image`` re-sampled to ``out_hw``; the images are clipped in groups of the product of the last
    ``group_axes`` leading axes (None: all of them, one group)."""
    if order not in (1, 3):
        raise ValueError(f"{who}: order must be 1 or 3 (got {order!r})")
    if mode not in _MODES:
        raise ValueError(f"{who}: mode must be 'reflect' or 'edge' (got {mode!r})")
    as_numpy = isinstance(image, np.ndarray)
    x = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(ops.require_gpu()) if as_numpy else image
    if not as_numpy and isinstance(x, torch.Tensor) and x.is_cuda:
        x = x.contiguous()
    ops._chk(x, "image")
    if x.dim() < 2:
        raise ValueError(f"{who} needs at least 2-D input")
    h, w = int(x.shape[-2]), int(x.shape[-1])
    oh, ow = (int(v) for v in out_hw)
    if min(h, w, oh, ow) < 1:
        raise ValueError(f"{who}: empty image or output shape ({h} x {w} -> {oh} x {ow})")
    if anti_aliasing is None:
        anti_aliasing = oh < h or ow < w                        # skimage: on exactly when an axis shrinks
    flat = x.reshape(-1, h, w)
    n = flat.shape[0]
    out = torch.empty((n, oh, ow), dtype=torch.float32, device=x.device)
    if n > 0:
        lead = x.shape[:-2]
        group = int(np.prod(lead if group_axes is None else lead[len(lead) - group_axes:], dtype=np.int64)) if clip else 0
        need = lib().inr_rescale2d_workspace_doubles(n, h, w, order, _MODES[mode])
        ws = torch.empty(max(int(need), 2), dtype=torch.float64, device=x.device)
        check(lib().inr_rescale2d(out.data_ptr(), flat.data_ptr(), n, h, w, oh, ow, order, _MODES[mode], int(bool(anti_aliasing)),
                                  group, ws.data_ptr(), ws.numel(), ops._stream()), "inr_rescale2d")
    out = out.reshape(*x.shape[:-2], oh, ow)
    return out.cpu().numpy().astype(np.float64) if as_numpy else out


def resize(image, output_shape, order: int = 1, mode: str = 'reflect', anti_aliasing=None, clip: bool = True):
    """``skimage.transform.resize`` (0.20) on the trailing two axes of ``image`` (ndarray in -> float64 ndarray out; device tensor
    in -> fp32 device tensor): orders 1 and 3, modes 'reflect' and 'edge'; ``anti_aliasing=None`` switches the Gaussian on exactly
    when an axis shrinks.  Leading axes are a batch that is clipped as ONE group (the minimum and maximum of all its images).
    There is no CPU fallback."""
    if len(output_shape) != 2:
        raise ValueError("resize: output_shape is (rows, columns) of the trailing two axes")
    return _resize("resize", image, output_shape, order, mode, anti_aliasing, clip)


def rescale2d(image, scale, order: int = 1, mode: str = 'reflect', anti_aliasing: bool = False, clip: bool = True):
    """``skimage.transform.rescale`` (0.20) for 2-D images -- what ``from skimage.transform import rescale`` of
    prepare_qual_images.py resolves to.  The output shape is ``np.round(scale * shape)`` (half to even); the rest is ``resize``."""
    out_hw = np.round(scale * np.asarray(image.shape[-2:], dtype=np.float64)).astype(np.int64)
    return _resize("rescale2d", image, out_hw, order, mode, anti_aliasing, clip)


_FOURIER_ALIGN = {"sample": _lib.INR_FOURIER_SAMPLE, "center": _lib.INR_FOURIER_CENTER}
_FOURIER_BOUNDARY = {"periodic": _lib.INR_FOURIER_PERIODIC, "mirror": _lib.INR_FOURIER_MIRROR}


def _fourier_modes(who, align, boundary, apodize):
    if align not in _FOURIER_ALIGN:
        raise ValueError(f"{who}: align must be 'sample' or 'center' (got {align!r})")
    if boundary not in _FOURIER_BOUNDARY:
        raise ValueError(f"{who}: boundary must be 'periodic' or 'mirror' (got {boundary!r})")
    apodize = float(apodize)
    if not 0.0 <= apodize <= 1.0:
        raise ValueError(f"{who}: apodize must be in [0, 1] (got {apodize!r})")
    return _FOURIER_ALIGN[align], _FOURIER_BOUNDARY[boundary], apodize


def _fourier_axis(who, n, m, align, boundary, passes=True):
    """Refuses what ``inr_fourier_resample2d`` would refuse for one axis (``passes``: a 1 -> 1 axis is passed through)."""
    if n < 1 or m < 1:
        raise ValueError(f"{who}: empty line or output ({n} -> {m})")
    if max(n, m) > _lib.INR_FOURIER_MAX_LINE:
        raise ValueError(f"{who}: lines of at most {_lib.INR_FOURIER_MAX_LINE} samples (got {n} -> {m})")
    if boundary == "mirror" and align == "sample" and not (passes and n == m == 1) and (n < 2 or ((2 * n - 2) * m) % n):
        raise ValueError(f"{who}: boundary='mirror' with align='sample' needs n >= 2 and (2n - 2) * m divisible by n (got {n} -> {m}); "
                         "align='center' and boundary='periodic' take any pair")


def _fourier_input(who, image):
    """Refuses by name what is neither an ndarray nor a float32 / float64 device tensor; True for an ndarray."""
    if isinstance(image, np.ndarray):
        return True
    if not isinstance(image, torch.Tensor):
        raise TypeError(f"{who} takes an ndarray or a device tensor (got {type(image).__name__})")
    if not image.is_cuda:
        raise ops.InrDeviceError(f"{who}: the tensor is on {image.device}; pass an ndarray or a device tensor (there is no CPU fallback)")
    if image.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{who}: device tensors must be float32 or float64 (got {image.dtype})")
    return False


def _fourier_resize(who, image, out_hw, align, boundary, apodize):
    modes = _fourier_modes(who, align, boundary, apodize)
    as_numpy = _fourier_input(who, image)
    if image.ndim < 2:
        raise ValueError(f"{who} needs at least 2-D input")
    h, w = int(image.shape[-2]), int(image.shape[-1])
    oh, ow = (int(v) for v in out_hw)
    _fourier_axis(who, h, oh, align, boundary)
    _fourier_axis(who, w, ow, align, boundary)
    x = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float64)).to(ops.require_gpu()) if as_numpy else image
    flat = x.reshape(-1, h, w).contiguous()
    n = flat.shape[0]
    out = torch.empty((n, oh, ow), dtype=x.dtype, device=x.device)
    if n > 0:
        ws = torch.empty(max(int(lib().inr_fourier_resample_workspace_doubles(n, h, w, oh, ow)), 2), dtype=torch.float64, device=x.device)
        entry = "inr_fourier_resample2d" if x.dtype == torch.float64 else "inr_fourier_resample2d_f32"
        check(getattr(lib(), entry)(out.data_ptr(), flat.data_ptr(), n, h, w, oh, ow, *modes, ws.data_ptr(), ws.numel(), ops._stream()),
              entry)
    out = out.reshape(*x.shape[:-2], oh, ow)
    return out.cpu().numpy() if as_numpy else out


def fourier_resize(image, output_shape, align: str = 'sample', boundary: str = 'mirror', apodize: float = 0.0):
    """Re-samples the trailing two axes of ``image`` to ``output_shape`` in k-space -- zero-filling when an axis grows, truncating
    when it shrinks: the interpolation an MR scanner applies (``inr_fourier_resample2d``).  Leading axes are a batch.
    ``align='sample'`` keeps sample 0 on sample 0 (the grid of a decimation ``x[::2]``; ``scipy.signal.resample``), ``'center'``
    aligns pixel centres (the grid of ``rescale``).  ``boundary='mirror'`` re-samples the mirrored line, so a cropped region does
    not wrap around; with ``align='sample'`` it needs ``(2n - 2) * m`` divisible by ``n`` per axis (integer factors, and 1/2 of an
    even length).  ``apodize`` in [0, 1] is a Tukey window over the kept band (0: none, 1: Hann).
    ndarray in -> float64 ndarray out, fp64 throughout; device fp32 / fp64 tensor in -> the same out (fp64 inside, rounded once).
    There is no CPU fallback."""
    if len(output_shape) != 2:
        raise ValueError("fourier_resize: output_shape is (rows, columns) of the trailing two axes")
    return _fourier_resize("fourier_resize", image, output_shape, align, boundary, apodize)


def fourier_rescale(image, scale, align: str = 'sample', boundary: str = 'mirror', apodize: float = 0.0):
    """``fourier_resize`` to the output shape ``np.round(scale * shape)`` of the trailing two axes (half to even, as ``rescale2d``)."""
    _fourier_modes("fourier_rescale", align, boundary, apodize)
    _fourier_input("fourier_rescale", image)
    if image.ndim < 2:
        raise ValueError("fourier_rescale needs at least 2-D input")
    out_hw = np.round(scale * np.asarray(image.shape[-2:], dtype=np.float64)).astype(np.int64)
    return _fourier_resize("fourier_rescale", image, out_hw, align, boundary, apodize)


def fourier_resample(x, num, axis: int = -1, align: str = 'sample', boundary: str = 'mirror', apodize: float = 0.0):
    """The 1-D form, in ``scipy.signal.resample``'s argument order: ``axis`` of ``x`` re-sampled to ``num`` points; with
    ``boundary='periodic'`` and the other defaults it is that function.  Types as ``fourier_resize``."""
    _fourier_modes("fourier_resample", align, boundary, apodize)
    as_numpy = _fourier_input("fourier_resample", x)
    if x.ndim < 1:
        raise ValueError("fourier_resample needs at least 1-D input")
    move = (lambda a, s, d: np.moveaxis(a, s, d)) if as_numpy else (lambda a, s, d: a.movedim(s, d))
    lines = move(x, axis, -1)
    out = _fourier_resize("fourier_resample", lines[..., None, :], (1, int(num)), align, boundary, apodize)
    return move(out[..., 0, :], -1, axis)


def fourier_operator(n, m, align: str = 'sample', boundary: str = 'mirror', apodize: float = 0.0):
    """The operator ``A`` [m][n] of one axis (``y = A x``) as a float64 ndarray, formed on the device (``inr_fourier_operator``)."""
    modes = _fourier_modes("fourier_operator", align, boundary, apodize)
    n, m = int(n), int(m)
    _fourier_axis("fourier_operator", n, m, align, boundary, passes=False)
    op = torch.empty((m, n), dtype=torch.float64, device=ops.require_gpu())
    check(lib().inr_fourier_operator(op.data_ptr(), n, m, *modes, ops._stream()), "inr_fourier_operator")
    return op.cpu().numpy()


def resize_z(arr, new_size: int = 128, kind: str = 'cubic'):
    """Re-samples the last axis of ``arr`` (ndarray or device tensor; leading axes are lines) to ``new_size`` points with the
    not-a-knot cubic spline of ``scipy.interpolate.interp1d(linspace(0, 1, n), arr, kind='cubic')``.  Returns the type it was
    given (ndarray in -> float64 ndarray out, like ``resize_array``; tensor in -> float64 device tensor)."""
    if kind != 'cubic':
        raise ValueError(f"resize_z: only kind='cubic' is implemented (got {kind!r})")
    as_numpy = isinstance(arr, np.ndarray)
    dev = ops.require_gpu()
    x = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64)).to(dev) if as_numpy else arr
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ops.InrDeviceError("resize_z takes an ndarray or a device tensor (there is no CPU fallback)")
    if x.dim() < 1 or int(new_size) < 1:
        raise ValueError("resize_z needs at least 1-D input and new_size >= 1")
    n_in, new_size = int(x.shape[-1]), int(new_size)
    flat = x.reshape(-1, n_in).to(torch.float64).contiguous()
    out = torch.empty((flat.shape[0], new_size), dtype=torch.float64, device=x.device)
    if flat.shape[0] > 0:
        ws = ops._ws(lib().inr_resize_z_cubic_workspace_bytes(flat.shape[0], n_in), x.device)
        check(lib().inr_resize_z_cubic(out.data_ptr(), flat.data_ptr(), flat.shape[0], n_in, new_size, ws.data_ptr(), ws.numel(),
                                       ops._stream()), "inr_resize_z_cubic")
    out = out.reshape(*x.shape[:-1], new_size)
    return out.cpu().numpy() if as_numpy else out
