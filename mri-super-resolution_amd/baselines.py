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

``tv_superres``, ``block_apply`` and ``block_adjoint`` are not the reference's either: the classical model-based reconstruction --
the block operator ``A`` of the acquisition (block mean or decimation), no network, a TV / Huber prior, Chambolle-Pock on the
device (``inr_tvsr_solve2d``) -- the comparator that says how much of a forward-model fit's gain is the model's.

``tv_superres3d``, ``block_apply3d``, ``block_adjoint3d`` and ``slice_profile`` are the same reconstruction on volumes: a separable
block operator whose first factor is the slice profile, a 3-D prior with per-axis gradient weights, one volume over many workgroups
(``inr_tvsr3d_solve``) -- what the through-plane study (``scripts/through_plane``) scores beside the spline.

``tv_superres_multi``, ``frame_apply``, ``frame_adjoint`` and ``estimate_shifts`` are the multi-frame form: K acquisitions of one
image, each displaced by a fraction of a pixel, one operator ``A_k = B S_k`` per frame with a bilinear translation ``S_k``, data and
prior both dual (``inr_tvmf_solve2d``) -- the classical comparator of the multi-image methods, which the
register-and-average baseline is not (it aligns to whole pixels and discards what the fractions hold).

``tv_superres_stacks``, ``stack_geometry``, ``profile_taps``, ``stack_apply`` and ``stack_adjoint`` are the multi-stack form on
volumes: 1 .. 8 stacks of thick slices of one volume -- different orientations, whole-voxel offsets, slice profiles wider
(overlapping) or narrower (gapped) than the slice spacing --, one operator ``A_s`` per stack with a validity rule for footprints that
leave the volume, data and prior both dual (``inr_tvms_solve``) -- what ``scripts/multi_stack`` scores.

``tv_superres_operator``, ``operator_apply``, ``operator_adjoint``, ``psf_operator`` and ``block_operator`` are the same prior under
ANY separable linear acquisition model ``A x = R0 x R1^T`` with dense operators: k-space truncation (``fourier_operator``), a
point-spread function wider than the pixel, a ratio that is no whole number -- the models the block solvers cannot write.  Two fp64
GEMMs per operator application inside the iteration (``inr_tvop_solve2d``).

``tv_superres_joint`` and ``channel_weights`` are the block solver with ONE prior over the channels of a group -- the b-values of a
DWI slice --: one gradient norm per pixel over all channels (vectorial TV / Huber), so that the low-SNR channels take their edges
from the others.  One workgroup per group (``inr_tvj_solve2d``); what ``superresDWI --tv_joint`` and
``scripts/joint_bvalues`` score.

``tv_superres_adc`` and ``adc_signal`` put the mono-exponential model inside the block solver: the unknowns of a group of b-values are
the two parameter maps, the b = 0 signal and the ADC, in a box, under a Huber-TV prior on the maps; the exact nonlinear primal-dual
method with the data term dualised, one workgroup per group (``inr_tvadc_solve2d``); what ``superresDWI --tv_adc`` and
``scripts/joint_bvalues --with_adc_model`` score.
"""
from __future__ import annotations

import math

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


TV_DEFAULT_LAMBDA, TV_DEFAULT_HUBER, TV_DEFAULT_ITERS = 3e-3, 0.3, 300       # the sweep of DESIGN.md 4l


def _named_kernel(kind, *f):
    """The block kernel 'mean' or 'decimate' of the factors ``f`` (one: 1-D, two: [f0][f1]) as a float64 ndarray; None for another name."""
    if kind == "mean":
        return np.full(f, 1.0 / math.prod(f))
    if kind == "decimate":
        k = np.zeros(f)
        k.flat[0] = 1.0
        return k
    return None


def _block_kernel(who, kernel, factors):
    """'mean', 'decimate' or an array [f0][f1] -> (f0, f1, nested float lists), refusing by name."""
    f0, f1 = ops.tv_factors(who, factors)
    if isinstance(kernel, str):
        name, kernel = kernel, _named_kernel(kernel, f0, f1)
        if kernel is None:
            raise ValueError(f"{who}: kernel must be 'mean', 'decimate' or an array [f0][f1] (got {name!r})")
    return f0, f1, ops.tv_block_kernel(who, kernel, (f0, f1))


def _block_input(who, image, name="input"):
    """Refuses by name what is no image batch; -> (True for an ndarray, rows, columns, leading shape).  Touches no device."""
    as_numpy = _fourier_input(who, image)
    if image.ndim < 2:
        raise ValueError(f"{who} needs at least 2-D {name}")
    return as_numpy, int(image.shape[-2]), int(image.shape[-1]), tuple(image.shape[:-2])


def _device_batch(value, as_numpy, rank):
    """-> the device tensor [n, <the trailing ``rank`` axes>] (an ndarray as float64)."""
    x = torch.from_numpy(np.ascontiguousarray(value, dtype=np.float64)).to(ops.require_gpu()) if as_numpy else value
    return x.reshape(-1, *x.shape[-rank:]).contiguous()


def _block_batch(image, as_numpy):
    """-> the device tensor [n, rows, columns] (an ndarray as float64)."""
    return _device_batch(image, as_numpy, 2)


def block_apply(x, factors, kernel="mean"):
    """``A x``: every ``f0 x f1`` block of the trailing two axes of ``x`` summed with the weights ``kernel`` -- 'mean' (the block mean),
    'decimate' (its first sample: LR sample j on HR sample f j) or an array [f0][f1] that sums to 1 (``inr_block_apply2d``, fp64).
    Leading axes are a batch; ndarray in -> float64 ndarray out, device fp32 / fp64 tensor in -> the same out."""
    f0, f1, k = _block_kernel("block_apply", kernel, factors)
    as_numpy, H, W, lead = _block_input("block_apply", x)
    ops.tv_hr_sides("block_apply", (H, W), (f0, f1))
    flat = _block_batch(x, as_numpy)
    out = ops.block_apply(flat.double(), (f0, f1), k).to(flat.dtype).reshape(*lead, H // f0, W // f1)
    return out.cpu().numpy() if as_numpy else out


def block_adjoint(r, factors, kernel="mean"):
    """``A^T r``: ``kernel[a][b] r[i][j]`` spread over block (i, j) (``inr_block_adjoint2d``); types as ``block_apply``."""
    f0, f1, k = _block_kernel("block_adjoint", kernel, factors)
    as_numpy, h, w, lead = _block_input("block_adjoint", r)
    ops.tv_hr_sides("block_adjoint", (h * f0, w * f1), (f0, f1))
    flat = _block_batch(r, as_numpy)
    out = ops.block_adjoint(flat.double(), (f0, f1), k).to(flat.dtype).reshape(*lead, h * f0, w * f1)
    return out.cpu().numpy() if as_numpy else out


def _weight_and_start(who, lr, as_numpy, lead, weight, lr_shape, x0, hr_shape, like="lr"):
    """``weight`` (``lead + lr_shape``) and ``x0`` (``lead + hr_shape``) of a solver, refused by name where they are not given like
    ``lr`` (``like``: what the messages call it); -> {"weight", "x0"}: None, or the device tensor [n, *lr_shape] / [n, *hr_shape]."""
    extra = {}
    for name, value, shape in (("weight", weight, lr_shape), ("x0", x0, hr_shape)):
        if value is None:
            extra[name] = None
            continue
        if isinstance(value, np.ndarray) != as_numpy:
            raise TypeError(f"{who}: {name} must be given like {like} ({'an ndarray' if as_numpy else 'a device tensor'})")
        _fourier_input(who, value)
        if tuple(value.shape) != lead + shape or (not as_numpy and value.dtype != lr.dtype):
            raise ValueError(f"{who}: {name} must have shape {lead + shape} and the type of {like} (got {tuple(value.shape)}, "
                             f"{value.dtype})")
        if name == "weight" and as_numpy and not (np.isfinite(value).all() and (value >= 0).all()):
            raise ValueError(f"{who}: weight must be finite and >= 0")
        extra[name] = (value, len(shape))
    return {name: None if item is None else _device_batch(item[0], as_numpy, item[1]) for name, item in extra.items()}   # the device last


def _tv_output(as_numpy, lead, out, trailing, info, return_info):
    """The tail of a solver: ``out`` [n, *trailing] and the per-image ``info`` tensors [n] in the leading shape, ndarrays if ndarrays
    came in."""
    out = out.reshape(*lead, *trailing)
    info = {name: v.reshape(lead) for name, v in info.items()}
    if as_numpy:
        out, info = out.cpu().numpy(), {name: v.cpu().numpy() for name, v in info.items()}
    return (out, info) if return_info else out


def tv_superres(lr, factors, kernel="mean", lam: float = TV_DEFAULT_LAMBDA, huber: float = TV_DEFAULT_HUBER,
                n_iter: int = TV_DEFAULT_ITERS, weight=None, x0=None, return_info: bool = False):
    """Model-based super-resolution of the trailing two axes of ``lr`` by ``factors`` = (f0, f1), 1 .. 8 each ((1, 1) denoises):
    ``n_iter`` Chambolle-Pock iterations on ``1/2 sum w (A x - lr)^2 + lam sum H_huber(|grad x|)`` with the block operator ``A`` of
    ``block_apply`` -- ``kernel`` 'mean', 'decimate' or an array [f0][f1] --, forward-difference gradient, ``huber`` = 0 the isotropic
    TV and > 0 the Huber function (quadratic up to ``huber``); ``lam`` = 0 keeps the data term only.  ``weight`` (shape of ``lr``,
    >= 0; 0 marks a missing datum) defaults to 1, ``x0`` (HR shape) to the block replication of ``lr``.  One launch for the whole
    batch, one workgroup per image (``inr_tvsr_solve2d``).  ndarray in -> float64 ndarray out; device fp32 / fp64
    tensor in -> the same out (fp64 inside, rounded once); ``weight`` / ``x0`` are given like ``lr``.  There is no CPU fallback.
    ``return_info``: also a dict with ``energy`` (the objective at the result) and ``change`` (max |x' - x| of the last iteration),
    both of the leading shape."""
    who = "tv_superres"
    f0, f1, k = _block_kernel(who, kernel, factors)
    lam, huber, n_iter = ops.tv_scalars(who, lam, huber, n_iter)
    as_numpy, h, w, lead = _block_input(who, lr)
    ops.tv_hr_sides(who, (h * f0, w * f1), (f0, f1))
    extra = _weight_and_start(who, lr, as_numpy, lead, weight, (h, w), x0, (h * f0, w * f1))
    y = _block_batch(lr, as_numpy)
    out, energy, change = ops.tvsr_solve(y, (f0, f1), k, lam, huber, n_iter, extra["weight"], extra["x0"])
    return _tv_output(as_numpy, lead, out, (h * f0, w * f1), {"energy": energy, "change": change}, return_info)


TVJ_DEFAULT_LAMBDA, TVJ_DEFAULT_HUBER, TVJ_DEFAULT_ITERS = 0.048, 0.01, 300    # the sweep of DESIGN.md 4q (ADC RMSE, noise 0.02)


def channel_weights(lr, rule: str = "equal"):
    """The channel weights ``mu`` [C] (float64 ndarray) of ``tv_superres_joint`` for ``lr`` [..., C, h, w].  'equal': all 1.
    'sqrt_signal': ``mu_c = sqrt(min_c' m_c' / m_c)`` with ``m_c`` the mean of channel c over every other axis -- the strongest channel
    gets the smallest weight, the weakest gets 1, so that no channel's edges drown the others' in the joint norm, and every weight
    is within (0, 1] as the solver's step bound requires.  The means are ONE host read of C values, taken here, outside the solve
    (which reads nothing back); a channel whose mean is not positive raises."""
    who = "channel_weights"
    as_numpy = _fourier_input(who, lr)
    if lr.ndim < 3:
        raise ValueError(f"{who} needs at least 3-D input [..., C, h, w]")
    C = int(lr.shape[-3])
    if rule == "equal":
        return np.ones(C, np.float64)
    if rule != "sqrt_signal":
        raise ValueError(f"{who}: rule must be 'equal' or 'sqrt_signal' (got {rule!r})")
    axes = tuple(a for a in range(lr.ndim) if a != lr.ndim - 3)
    m = np.asarray(lr, np.float64).mean(axis=axes) if as_numpy else lr.double().mean(dim=axes).cpu().numpy()
    if not (np.isfinite(m).all() and (m > 0).all()):
        raise ValueError(f"{who}: 'sqrt_signal' needs a positive mean in every channel (got {m.tolist()})")
    return np.sqrt(m.min() / m)


def tv_superres_joint(lr, factors, kernel="mean", lam: float = TVJ_DEFAULT_LAMBDA, huber: float = TVJ_DEFAULT_HUBER,
                      n_iter: int = TVJ_DEFAULT_ITERS, channel_weights=None, coupling: str = "joint", weight=None, x0=None,
                      return_info: bool = False):
    """``tv_superres`` with ONE prior over the channels of a group: ``lr`` [..., C, h, w], the third axis from the end the channel axis
    (the b-values of a slice), 1 <= C <= 16, leading axes a batch of groups.  ``n_iter`` Chambolle-Pock iterations on
    ``1/2 sum_c sum w (A x_c - lr_c)^2 + lam sum_j H_huber(sqrt(sum_c mu_c^2 |grad x_c|_j^2))``: one gradient norm per pixel over all
    channels, so that edges are shared and noise is not.  ``coupling='none'`` takes the norm per channel
    (``sum_c lam H_huber(mu_c |grad x_c|)``; with ``mu = 1`` that is ``tv_superres`` of every channel, bit for bit).
    ``channel_weights``: C values in [0, 1] (``channel_weights(lr, rule)``; None: all 1) -- larger weights are a rescaled ``lam`` and
    ``huber``.  At equal ``lam`` the coupled prior is weaker per channel than the per-channel one: it has defaults of its own.
    ``weight`` / ``x0`` / types / ``return_info`` as ``tv_superres`` (``energy`` and ``change`` per group, of the leading shape).  One
    launch for the whole batch, one workgroup per group (``inr_tvj_solve2d``).  There is no CPU fallback."""
    who = "tv_superres_joint"
    f0, f1, k = _block_kernel(who, kernel, factors)
    lam, huber, n_iter = ops.tv_scalars(who, lam, huber, n_iter)
    ops.tv_coupling(who, coupling)
    as_numpy = _fourier_input(who, lr)
    if lr.ndim < 3:
        raise ValueError(f"{who} needs at least 3-D input [..., C, h, w]")
    C, h, w, lead = int(lr.shape[-3]), int(lr.shape[-2]), int(lr.shape[-1]), tuple(lr.shape[:-3])
    ops.tvj_channels(who, C)
    ops.tv_hr_sides(who, (h * f0, w * f1), (f0, f1))
    mu = ops.tvj_channel_weights(who, channel_weights, C)
    extra = _weight_and_start(who, lr, as_numpy, lead, weight, (C, h, w), x0, (C, h * f0, w * f1))
    y = _device_batch(lr, as_numpy, 3)
    out, energy, change = ops.tvj_solve(y, (f0, f1), k, mu, lam, huber, coupling, n_iter, extra["weight"], extra["x0"])
    return _tv_output(as_numpy, lead, out, (C, h * f0, w * f1), {"energy": energy, "change": change}, return_info)


# the sweep of DESIGN.md 4t (ADC RMSE of the solver's map subject to the b = 0 PSNR of the per-channel solver, noise 0.02)
ADC_DEFAULT_LAMBDA, ADC_DEFAULT_HUBER, ADC_DEFAULT_ITERS = 0.00125, 0.03, 3000
ADC_DEFAULT_MAP_WEIGHTS, ADC_DEFAULT_COUPLING = (1.0, 0.05), "joint"
ADC_DEFAULT_S_MAX, ADC_DEFAULT_ADC_MAX, ADC_DEFAULT_ADC0 = 1.5, 4e-3, 1e-3


def tv_superres_adc(lr, b, factors, kernel="mean", lam: float = ADC_DEFAULT_LAMBDA, huber: float = ADC_DEFAULT_HUBER,
                    n_iter: int = ADC_DEFAULT_ITERS, map_weights=ADC_DEFAULT_MAP_WEIGHTS, coupling: str = ADC_DEFAULT_COUPLING,
                    s_max: float = ADC_DEFAULT_S_MAX, adc_max: float = ADC_DEFAULT_ADC_MAX, adc0: float = ADC_DEFAULT_ADC0, weight=None,
                    x0=None, return_info: bool = False):
    """Model-based super-resolution of the two PARAMETER MAPS of a multi-b-value group: ``lr`` [..., C, h, w], the third axis from the
    end the b-values ``b`` [C] of a slice (2 <= C <= 16, finite, >= 0, not all equal), leading axes a batch of groups.  ``n_iter``
    iterations of the exact nonlinear primal-dual method on
    ``1/2 sum_c sum w (A (s0 exp(-b_c adc)) - lr_c)^2 + lam R(s0, adc)`` over ``0 <= s0 <= s_max``, ``0 <= adc <= adc_max``, with the
    block operator ``A`` of ``tv_superres`` and the Huber-TV prior of ``tv_superres_joint`` on the two maps -- the ADC normalised by the
    largest b-value --: ``coupling='joint'`` one gradient norm per pixel over both maps, ``'none'`` one per map; ``map_weights`` =
    (mu_s, mu_d) in [0, 1].  Two unknowns per pixel instead of C: noise in the high-b channels can only enter through the ADC, both
    maps are non-negative, and the ADC needs no clipped logarithm.  The objective is not convex and the method converges locally: from
    the default start -- the block replication of the lowest b-value and ``adc0`` everywhere -- it needs about three times the
    iterations of ``tv_superres_joint``.  -> ``(s0 [..., H, W], adc [..., H, W])``, and with ``return_info`` a dict with ``energy`` (the
    objective at the result) and ``change`` (max |s' - s|, |u' - u| of the last iteration, u the normalised ADC) of the leading shape.
    ``x0``: a pair ``(s0, adc)`` of HR maps, clamped into the box; ``weight`` (shape of ``lr``, >= 0; 0 a missing datum).  ndarray in ->
    float64 ndarrays out; device fp32 / fp64 tensor in -> the same out (fp64 inside, rounded once).  One launch for the whole batch,
    one workgroup per group (``inr_tvadc_solve2d``).  There is no CPU fallback."""
    who = "tv_superres_adc"
    f0, f1, k = _block_kernel(who, kernel, factors)
    lam, huber, n_iter = ops.tv_scalars(who, lam, huber, n_iter)
    as_numpy = _fourier_input(who, lr)
    if lr.ndim < 3:
        raise ValueError(f"{who} needs at least 3-D input [..., C, h, w]")
    C, h, w, lead = int(lr.shape[-3]), int(lr.shape[-2]), int(lr.shape[-1]), tuple(lr.shape[:-3])
    vals, mu, s_max, adc_max, adc0 = ops.tvadc_model(who, b, C, map_weights, coupling, s_max, adc_max, adc0)
    H, W = h * f0, w * f1
    ops.tv_hr_sides(who, (H, W), (f0, f1))
    if x0 is not None:
        if not isinstance(x0, (tuple, list)) or len(x0) != 2:
            raise ValueError(f"{who}: x0 is a pair (s0, adc) of maps of shape {lead + (H, W)}")
        for m in x0:
            if isinstance(m, np.ndarray) != as_numpy:
                raise TypeError(f"{who}: x0 must be given like lr ({'ndarrays' if as_numpy else 'device tensors'})")
            _fourier_input(who, m)
            if tuple(m.shape) != lead + (H, W) or (not as_numpy and m.dtype != lr.dtype):
                raise ValueError(f"{who}: x0 is a pair (s0, adc) of maps of shape {lead + (H, W)} and the type of lr (got "
                                 f"{tuple(m.shape)}, {m.dtype})")
        x0 = np.stack(x0, axis=-3) if as_numpy else torch.stack(tuple(x0), dim=-3)
    extra = _weight_and_start(who, lr, as_numpy, lead, weight, (C, h, w), x0, (2, H, W))
    y = _device_batch(lr, as_numpy, 3)
    s0, adc, energy, change = ops.tvadc_solve(y, vals, (f0, f1), k, mu, lam, huber, coupling, n_iter, s_max, adc_max, adc0,
                                              extra["weight"], extra["x0"])
    info = {name: v.reshape(lead) for name, v in (("energy", energy), ("change", change))}
    s0, adc = s0.reshape(*lead, H, W), adc.reshape(*lead, H, W)
    if as_numpy:
        s0, adc, info = s0.cpu().numpy(), adc.cpu().numpy(), {name: v.cpu().numpy() for name, v in info.items()}
    return (s0, adc, info) if return_info else (s0, adc)


def adc_signal(s0, adc, b):
    """The images of the mono-exponential model, ``s0 exp(-b_c adc)`` [..., C, H, W], of two maps [..., H, W] of one shape and type and
    1 .. 16 finite b-values (``inr_adc_signal``; fp64 inside, rounded once).  ndarrays in -> float64 ndarray out, device fp32 / fp64
    tensors in -> the same out."""
    who = "adc_signal"
    as_numpy, H, W, lead = _block_input(who, s0)
    if isinstance(adc, np.ndarray) != as_numpy:
        raise TypeError(f"{who}: adc must be given like s0 ({'an ndarray' if as_numpy else 'a device tensor'})")
    _fourier_input(who, adc)
    if tuple(adc.shape) != tuple(s0.shape) or (not as_numpy and adc.dtype != s0.dtype):
        raise ValueError(f"{who}: adc must have the shape and type of s0 ({tuple(s0.shape)}; got {tuple(adc.shape)}, {adc.dtype})")
    vals = ops.adc_bvalues(who, b)
    out = ops.adc_signal(_block_batch(s0, as_numpy), _block_batch(adc, as_numpy), vals).reshape(*lead, len(vals), H, W)
    return out.cpu().numpy() if as_numpy else out


TGV_DEFAULT_LAMBDA, TGV_DEFAULT_RATIO, TGV_DEFAULT_HUBER, TGV_DEFAULT_ITERS = 0.005, 0.5, 0.0, 300   # the sweep of DESIGN.md 4r


def tgv_superres(lr, factors, kernel="mean", lam: float = TGV_DEFAULT_LAMBDA, ratio: float = TGV_DEFAULT_RATIO,
                 huber: float = TGV_DEFAULT_HUBER, n_iter: int = TGV_DEFAULT_ITERS, weight=None, x0=None, return_info: bool = False):
    """``tv_superres`` under the second-order total generalized variation, which does not terrace smooth intensity: ``n_iter``
    Chambolle-Pock iterations on ``1/2 sum w (A x - lr)^2 + lam sum H_huber(|grad x - v|) + ratio lam sum |E v|_F`` over the image ``x``
    and an auxiliary vector field ``v`` that absorbs the smooth part of the gradient (``E v`` its symmetrised derivative): a ramp costs
    nothing, an edge still costs its jump.  ``ratio`` > 0 weighs the second-order term against the first (large: towards
    ``tv_superres``); ``lam`` = 0 keeps the data term only.  Input types, leading-axis batching, ``kernel``, ``weight``, ``x0`` and dtype
    rules as ``tv_superres``.  One launch for the whole batch, one workgroup per image (``inr_tgv_solve2d``).  There is no
    CPU fallback.  ``return_info``: also a dict with ``energy`` (the objective at the returned ``(x, v)``), ``change`` (max |x' - x| of
    the last iteration), both of the leading shape, and ``v`` [..., 2, H, W]."""
    who = "tgv_superres"
    f0, f1, k = _block_kernel(who, kernel, factors)
    ratio = float(ratio)
    lam, huber, n_iter = ops.tv_scalars(who, lam, huber, n_iter)
    ops.tgv_ratio(who, ratio)
    as_numpy, h, w, lead = _block_input(who, lr)
    ops.tv_hr_sides(who, (h * f0, w * f1), (f0, f1))
    extra = _weight_and_start(who, lr, as_numpy, lead, weight, (h, w), x0, (h * f0, w * f1))
    y = _block_batch(lr, as_numpy)
    out, v, energy, change = ops.tgv_solve(y, (f0, f1), k, lam, ratio, huber, n_iter, extra["weight"], extra["x0"], want_v=return_info)
    if not return_info:
        return _tv_output(as_numpy, lead, out, (h * f0, w * f1), {}, False)
    out, info = _tv_output(as_numpy, lead, out, (h * f0, w * f1), {"energy": energy, "change": change}, True)
    v = v.reshape(*lead, 2, h * f0, w * f1)
    info["v"] = v.cpu().numpy() if as_numpy else v
    return out, info


TVMF_DEFAULT_LAMBDA,TVMF_DEFAULT_HUBER, TVMF_DEFAULT_ITERS = 0.01, 0.03, 300  # the sweep of DESIGN.md 4n (8 frames, noise 0.02)


def _shift_input(who, shifts, lead, K=None):
    """Refuses by name what is no shift array for images of leading shape ``lead``: [..., K, 2] or [K, 2] for all images, an array-like
    or a float32 / float64 device tensor.  -> K.  Touches no device."""
    if isinstance(shifts, torch.Tensor):
        if not shifts.is_cuda:
            raise ops.InrDeviceError(f"{who}: shifts is on {shifts.device}; pass an array or a device tensor (there is no CPU fallback)")
        if shifts.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{who}: device shifts must be float32 or float64 (got {shifts.dtype})")
        shape = tuple(shifts.shape)
    else:
        try:
            shape = np.asarray(shifts, dtype=np.float64).shape
        except (TypeError, ValueError):
            raise TypeError(f"{who}: shifts must be an array [..., K, 2] or a device tensor (got {type(shifts).__name__})") from None
    if len(shape) < 2 or shape[-1] != 2 or (len(shape) > 2 and shape[:-2] != tuple(lead)) or (K is not None and shape[-2] != K):
        want = f"{tuple(lead) + ('K' if K is None else K, 2)} or {('K' if K is None else K, 2)}"
        raise ValueError(f"{who}: shifts must have shape {want}, (rows, columns) in HR pixels per frame (got {shape})")
    ops.tvmf_frame_count(who, shape[-2])
    return shape[-2]


def _shift_batch(shifts, n, device):
    """-> the device tensor [n, K, 2] float64; no host read for a device tensor."""
    s = shifts.to(torch.float64) if isinstance(shifts, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(shifts, dtype=np.float64)).to(device)
    K = s.shape[-2]
    return (s.expand(n, K, 2) if s.dim() == 2 else s.reshape(n, K, 2)).contiguous()


def frame_apply(x, factors, shifts, kernel="mean", return_valid: bool = False):
    """The K frames ``A_k x = B S_k x`` of the trailing two axes of ``x``: ``S_k`` translates by ``shifts[..., k, :]`` = (rows, columns)
    in HR pixels with bilinear weights -- ``(S x)[i] = x[i + s]`` --, ``B`` is ``block_apply`` (``inr_frame_apply2d``, fp64,
    DESIGN.md 4n).  ``x`` [..., H, W] -> [..., K, H/f0, W/f1]; ``shifts`` [..., K, 2], or [K, 2] for all images, an array or a device
    tensor.  A datum whose footprint leaves the image is invalid and comes back 0; ``return_valid`` adds the bool mask.  Types as
    ``block_apply``."""
    who = "frame_apply"
    f0, f1, k = _block_kernel(who, kernel, factors)
    as_numpy, H, W, lead = _block_input(who, x)
    ops.tv_hr_sides(who, (H, W), (f0, f1))
    K = _shift_input(who, shifts, lead)
    flat = _block_batch(x, as_numpy)
    res = ops.frame_apply(flat.double(), _shift_batch(shifts, flat.shape[0], flat.device), (f0, f1), k, return_valid)
    out, valid = res if return_valid else (res, None)
    out = out.to(flat.dtype).reshape(*lead, K, H // f0, W // f1)
    if return_valid:
        valid = valid.reshape(out.shape)
        return (out.cpu().numpy(), valid.cpu().numpy()) if as_numpy else (out, valid)
    return out.cpu().numpy() if as_numpy else out


def frame_adjoint(r, factors, shifts, kernel="mean"):
    """``sum_k A_k^T r_k``, the adjoint of ``frame_apply``: ``r`` [..., K, h, w] -> [..., f0 h, f1 w], a gather with no atomics in which
    invalid data take no part (``inr_frame_adjoint2d``); types as ``block_apply``."""
    who = "frame_adjoint"
    f0, f1, k = _block_kernel(who, kernel, factors)
    as_numpy, h, w, lead = _block_input(who, r)
    if len(lead) < 1:
        raise ValueError(f"{who} needs at least 3-D input [..., K, h, w]")
    lead, K = lead[:-1], lead[-1]
    ops.tvmf_frame_count(who, K)
    ops.tv_hr_sides(who, (h * f0, w * f1), (f0, f1))
    _shift_input(who, shifts, lead, K)
    flat = _block_batch(r, as_numpy).reshape(-1, K, h, w)
    out = ops.frame_adjoint(flat.double(), _shift_batch(shifts, flat.shape[0], flat.device), (f0, f1), k)
    out = out.to(flat.dtype).reshape(*lead, h * f0, w * f1)
    return out.cpu().numpy() if as_numpy else out


def tv_superres_multi(frames, factors, shifts, kernel="mean", lam: float = TVMF_DEFAULT_LAMBDA, huber: float = TVMF_DEFAULT_HUBER,
                      n_iter: int = TVMF_DEFAULT_ITERS, weight=None, x0=None, return_info: bool = False):
    """Multi-frame model-based super-resolution: ``frames`` [..., K, h, w] are K acquisitions of one image, frame k displaced by
    ``shifts[..., k, :]`` = (rows, columns) HR pixels (``frame_apply``'s convention; [K, 2] serves all images; see
    ``estimate_shifts``).  ``n_iter`` Chambolle-Pock iterations, data and prior both dual, on
    ``1/2 sum_k sum w_k (A_k x - frames_k)^2 + lam sum H_huber(|grad x|)`` with the prior of ``tv_superres``.  The objective is NOT
    divided by K: the data term grows with the number of frames, so ``lam`` is chosen for a frame count (the default for 8 frames at
    noise 0.02 of a [0, 1] image; scale it with K).  A datum whose footprint leaves the image has weight 0 and is never read (it
    may be NaN); a frame with a non-finite shift or one beyond 2^20 is ignored.  ``weight`` (shape of ``frames``, >= 0) defaults to 1,
    ``x0`` [..., f0 h, f1 w] to the block replication of frame 0.  ``inr_tvmf_solve2d``.  ndarray in -> float64
    ndarray out; device fp32 / fp64 tensor in -> the same out (fp64 inside, rounded once); ``weight`` / ``x0`` are given like
    ``frames``.  There is no CPU fallback.  ``return_info``: also a dict with ``energy`` (the objective at the result), ``change``
    (max |x' - x| of the last iteration) and ``valid_fraction`` (the valid share of the data), each of the leading shape."""
    who = "tv_superres_multi"
    f0, f1, k = _block_kernel(who, kernel, factors)
    lam, huber, n_iter = ops.tv_scalars(who, lam, huber, n_iter, ops.TVSR3D_MAX_ITER, "in 0 ..")
    as_numpy, h, w, lead = _block_input(who, frames, "frames")
    if len(lead) < 1:
        raise ValueError(f"{who} needs at least 3-D frames [..., K, h, w]")
    lead, K = lead[:-1], lead[-1]
    ops.tvmf_frame_count(who, K)
    ops.tv_hr_sides(who, (h * f0, w * f1), (f0, f1))
    _shift_input(who, shifts, lead, K)
    extra = _weight_and_start(who, frames, as_numpy, lead, weight, (K, h, w), x0, (h * f0, w * f1), like="frames")
    y = _device_batch(frames, as_numpy, 3)
    out, energy, change, valid = ops.tvmf_solve(y, _shift_batch(shifts, y.shape[0], y.device), (f0, f1), k, lam, huber, n_iter,
                                                extra["weight"], extra["x0"])
    return _tv_output(as_numpy, lead, out, (h * f0, w * f1), {"energy": energy, "change": change, "valid_fraction": valid}, return_info)


def estimate_shifts(frames, factors, upsample: int = 4, max_shift=None, reference: int = 0):
    """The shifts of ``frames`` [..., K, h, w] against frame ``reference``, for ``tv_superres_multi``: every frame is re-sampled to
    (``upsample`` h, ``upsample`` w) by ``fourier_resize(align='center', boundary='mirror')`` and correlated with the re-sampled
    reference by the masked normalised cross-correlation of ``registration`` with all-clear masks (two existing kernel families, no
    new one).  The sign is ``masked_register_translation(ref, x, m)``'s -- ``x[i] ~ ref[i + s]`` --, which is ``frame_apply``'s.
    ``max_shift`` (None: any overlap) limits the search, in LR pixels.  Returns [..., K, 2] float64 IN HR PIXELS, a multiple of the step
    ``f / upsample`` per axis (means of equal maxima aside); the reference's row is 0.  ndarray in -> ndarray out; device tensor in ->
    device tensor out with no host read on the way."""
    from . import registration
    who = "estimate_shifts"
    f0, f1 = ops.tv_factors(who, factors)
    if isinstance(upsample, bool) or int(upsample) != upsample or not 1 <= upsample <= 16:
        raise ValueError(f"{who}: upsample must be an integer in 1 .. 16 (got {upsample!r})")
    u = int(upsample)
    as_numpy, h, w, lead = _block_input(who, frames, "frames")
    if len(lead) < 1:
        raise ValueError(f"{who} needs at least 3-D frames [..., K, h, w]")
    lead, K = lead[:-1], lead[-1]
    ops.tvmf_frame_count(who, K)
    if isinstance(reference, bool) or int(reference) != reference or not 0 <= reference < K:
        raise ValueError(f"{who}: reference must be a frame index in 0 .. {K - 1} (got {reference!r})")
    if max_shift is not None and not 0.0 <= float(max_shift) < np.inf:
        raise ValueError(f"{who}: max_shift must be None or a finite number of LR pixels >= 0 (got {max_shift!r})")
    window = registration._window(who, (u * h, u * w), None if max_shift is None else int(np.ceil(float(max_shift) * u)))
    _fourier_axis(who, h, u * h, "center", "mirror")
    _fourier_axis(who, w, u * w, "center", "mirror")
    up =fourier_resize(_block_batch(frames, as_numpy).double(), (u * h, u * w), align="center", boundary="mirror")
    planes = up.reshape(-1, K, u * h, u * w).float().contiguous()
    ref = torch.full((planes.shape[0],), int(reference), dtype=torch.int32, device=planes.device)
    steps, _, _, _ = registration._xcorr(planes, torch.ones_like(planes), ref, window, 3 / 10)
    out = (steps * torch.tensor([f0 / u, f1 / u], dtype=torch.float64, device=planes.device)).reshape(*lead, K, 2)
    return out.cpu().numpy() if as_numpy else out


TV3D_DEFAULT_LAMBDA, TV3D_DEFAULT_HUBER, TV3D_DEFAULT_ITERS = 3e-3, 0.1, 300   # the sweep of DESIGN.md 4m
TV3D_DEFAULT_GRAD_WEIGHTS = (1.0, 1.0, 1.0)


def _gaussian_taps(who, count, spacing, fwhm):
    """``count`` samples of a Gaussian of full width at half maximum ``fwhm`` at the positions ``(t + 1/2 - count/2) / spacing``, centred
    on the footprint and normalised to sum 1."""
    sigma = float(fwhm) / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    pos = (2.0 * np.arange(count) + 1.0 - count) / (2.0 * spacing)       # antisymmetric to the bit
    k = np.exp(-0.5 * (pos / sigma) ** 2)
    if not k.sum() > 0.0:
        raise ValueError(f"{who}: fwhm {fwhm!r} is too narrow: every sample of the Gaussian underflows")
    return k / k.sum()


def slice_profile(f, kind: str = "mean", fwhm=None):
    """The slice profile k0 [f] of a thick slice made of ``f`` thin ones, as a float64 ndarray that sums to 1: 'mean' (a box over the
    thick slice), 'decimate' (its first thin slice) or 'gaussian' -- a Gaussian of full width at half maximum ``fwhm``, in THICK
    slices, centred on the thick slice and sampled at the centres of its ``f`` thin slices (positions ``(a + 1/2) / f - 1/2``), the
    samples normalised to sum 1.  ``fwhm`` belongs to 'gaussian' alone."""
    who = "slice_profile"
    if int(f) != f or not 1 <= int(f) <= ops.TVSR_MAX_FACTOR:
        raise ValueError(f"{who}: f is an integer 1 .. {ops.TVSR_MAX_FACTOR} (got {f!r})")
    f = int(f)
    if kind != "gaussian" and fwhm is not None:
        raise ValueError(f"{who}: fwhm belongs to kind='gaussian' (got kind={kind!r})")
    if kind == "gaussian":
        if fwhm is None or not 0.0 < float(fwhm) < np.inf:
            raise ValueError(f"{who}: kind='gaussian' needs a finite fwhm > 0, in thick slices (got {fwhm!r})")
        return _gaussian_taps(who, f, f, fwhm)                   # at (a + 1/2) / f - 1/2
    k = _named_kernel(kind, f)
    if k is None:
        raise ValueError(f"{who}: kind must be 'mean', 'decimate' or 'gaussian' (got {kind!r})")
    return k


def _kernel_factors(who, kernel, f, taps=False):
    """'mean', 'decimate' or a triple of 1-D arrays (k0, k1, k2) -> three float lists: of ``f`` entries per axis, or (``taps``) the
    arrays of any 1 .. 16 entries."""
    if isinstance(kernel, str):
        if kernel not in ("mean", "decimate"):
            raise ValueError(f"{who}: kernel must be 'mean', 'decimate' or a triple of 1-D arrays (k0, k1, k2) (got {kernel!r})")
        kernel = [_named_kernel(kernel, v) for v in f]
    return ops.tv_kernel_factors(who, kernel, None if taps else f)


def _block_kernel3d(who, kernel, factors):
    """'mean', 'decimate' or a triple of 1-D arrays (k0 [f0], k1 [f1], k2 [f2]) -> ((f0, f1, f2), three float lists), refusing by name."""
    f = ops.tv_factors(who, factors, 3)
    return f, _kernel_factors(who, kernel, f)


def _volume_input(who, volume, name="input"):
    """Refuses by name what is no batch of volumes; -> (True for an ndarray, (slices, rows, columns), leading shape)."""
    as_numpy = _fourier_input(who, volume)
    if volume.ndim < 3:
        raise ValueError(f"{who} needs at least 3-D {name}")
    return as_numpy, tuple(int(v) for v in volume.shape[-3:]), tuple(volume.shape[:-3])


def _volume_batch(volume, as_numpy):
    """-> the device tensor [n, slices, rows, columns] (an ndarray as float64)."""
    return _device_batch(volume, as_numpy, 3)


def block_apply3d(x, factors, kernel="mean"):
    """``A x`` on volumes: every ``f0 x f1 x f2`` block of the trailing three axes (slice, row, column) of ``x`` summed with the
    separable weights ``k[a][b][c] = (k1[b] k2[c]) k0[a]`` -- ``kernel`` 'mean', 'decimate' or a triple of 1-D arrays (k0, k1, k2),
    each summing to 1; k0 is the slice profile (``slice_profile``) -- (``inr_tvsr3d_block_apply``, fp64).  Leading axes are
    a batch; ndarray in -> float64 ndarray out, device fp32 / fp64 tensor in -> the same out."""
    f, k = _block_kernel3d("block_apply3d", kernel, factors)
    as_numpy, hr, lead = _volume_input("block_apply3d", x)
    ops.tv_hr_sides("block_apply3d", hr, f)
    flat = _volume_batch(x, as_numpy)
    out = ops.block_apply3d(flat.double(), f, k).to(flat.dtype).reshape(*lead, *(s // v for s, v in zip(hr, f)))
    return out.cpu().numpy() if as_numpy else out


def block_adjoint3d(r, factors, kernel="mean"):
    """``A^T r`` on volumes: ``k[a][b][c] r[l][i][j]`` spread over block (l, i, j) (``inr_tvsr3d_block_adjoint``); types as
    ``block_apply3d``."""
    f, k = _block_kernel3d("block_adjoint3d", kernel, factors)
    as_numpy, lr, lead = _volume_input("block_adjoint3d", r)
    hr = tuple(s * v for s, v in zip(lr, f))
    ops.tv_hr_sides("block_adjoint3d", hr, f)
    flat = _volume_batch(r, as_numpy)
    out = ops.block_adjoint3d(flat.double(), f, k).to(flat.dtype).reshape(*lead, *hr)
    return out.cpu().numpy() if as_numpy else out


def tv_superres3d(lr, factors, kernel="mean", lam: float = TV3D_DEFAULT_LAMBDA, huber: float = TV3D_DEFAULT_HUBER,
                  n_iter: int = TV3D_DEFAULT_ITERS, grad_weights=TV3D_DEFAULT_GRAD_WEIGHTS, weight=None, x0=None,
                  return_info: bool = False):
    """Model-based super-resolution of the trailing three axes (slice, row, column) of ``lr`` by ``factors`` = (f0, f1, f2), 1 .. 8
    each: ``n_iter`` Chambolle-Pock iterations on ``1/2 sum w (A x - lr)^2 + lam sum H_huber(|grad x|)`` with the block operator
    ``A`` of ``block_apply3d`` -- ``kernel`` 'mean', 'decimate' or a triple of 1-D arrays (k0, k1, k2), k0 the slice profile -- and
    the forward-difference gradient scaled per axis by ``grad_weights`` = (g0, g1, g2) >= 0 (slice, row, column; the voxel spacing:
    g0 = in-plane spacing / slice spacing; g0 = 0 uncouples the slices, which then are ``tv_superres`` of each, bit for bit).
    ``huber``, ``lam``, ``weight`` (shape of ``lr``) and ``x0`` (HR shape) as for ``tv_superres``.  Leading axes are a batch; a
    volume is spread over many workgroups, two plain launches per iteration (``inr_tvsr3d_solve``).  ndarray in ->
    float64 ndarray out; device fp32 / fp64 tensor in -> the same out (fp64 inside, rounded once).  There is no CPU fallback.
    ``return_info``: also a dict with ``energy`` and ``change``, both of the leading shape."""
    who = "tv_superres3d"
    f, k = _block_kernel3d(who, kernel, factors)
    lam, huber, n_iter = ops.tv_scalars(who, lam, huber, n_iter, ops.TVSR3D_MAX_ITER)
    g = ops.tv_grad_weights(who, grad_weights)
    as_numpy, lo, lead = _volume_input(who, lr)
    hr = tuple(s * v for s, v in zip(lo, f))
    ops.tv_hr_sides(who, hr, f)
    extra = _weight_and_start(who, lr, as_numpy, lead, weight, lo, x0, hr)
    y = _volume_batch(lr, as_numpy)
    out, energy, change = ops.tvsr_solve3d(y, f, k, lam, huber, n_iter, g, extra["weight"], extra["x0"])
    return _tv_output(as_numpy, lead, out, hr, {"energy": energy, "change": change}, return_info)


NLM_DEFAULT_LEVELS = (0.125, 0.0625, 0.03125, 0.015625, 0.0078125)   # Manjon et al. 2010: h = 32 .. 2 on an 8-bit scale, data in [0, 1]
NLM_DEFAULT_ITERS, NLM_DEFAULT_SEARCH, NLM_DEFAULT_PATCH = 2, 2, 1


def nlm_upsample(lr, factors, kernel="mean", levels=NLM_DEFAULT_LEVELS, n_iter: int = NLM_DEFAULT_ITERS, search=NLM_DEFAULT_SEARCH,
                 patch=NLM_DEFAULT_PATCH, relax: float = 1.0, guide=None, x0=None, return_info: bool = False):
    """Non-local upsampling (Manjon et al., Medical Image Analysis 2010) of the trailing three axes (slice, row, column) of ``lr`` by
    ``factors`` = (f0, f1, f2), 1 .. 8 each: from ``x0`` (None: the block replication of ``lr``), for every strength ``h`` of
    ``levels`` and each of ``n_iter`` passes, a non-local-means filter (search radius ``search``, patch radius ``patch``, an int or a
    triple; strength ``h^2``, centre weight 1) guided by the current estimate -- or by the fixed ``guide`` (HR shape), e.g. another
    contrast --, followed by the mean correction ``x <- x' - relax N(A x' - lr)`` under the block operator ``A`` of ``block_apply3d``
    (``kernel`` 'mean', 'decimate' or a triple of 1-D arrays), ``N`` the replication over a block: with ``relax`` = 1 every pass ends
    with ``A x = lr``.  The levels suit data in [0, 1].  Leading axes are a batch (``inr_nlm_upsample``).  ndarray in ->
    float64 ndarray out; device fp32 / fp64 tensor in -> the same out (fp64 inside, rounded once).  There is no CPU fallback.
    ``return_info``: also a dict with ``change`` [passes, ...leading shape], the mean absolute change of every pass."""
    who = "nlm_upsample"
    f, k = _block_kernel3d(who, kernel, factors)
    s, r = ops.nlm_radii(who, search, patch)
    lv, n_iter, relax = ops.nlm_schedule(who, levels, n_iter, relax)
    as_numpy, lo, lead = _volume_input(who, lr)
    hr = tuple(v * g for v, g in zip(lo, f))
    ops.nlm_volume(who, hr)
    for name, value in (("x0", x0), ("guide", guide)):
        if value is None:
            continue
        if isinstance(value, np.ndarray) != as_numpy:
            raise TypeError(f"{who}: {name} must be given like lr ({'an ndarray' if as_numpy else 'a device tensor'})")
        _fourier_input(who, value)
        if tuple(value.shape) != lead + hr or (not as_numpy and value.dtype != lr.dtype):
            raise ValueError(f"{who}: {name} must have shape {lead + hr} and the type of lr (got {tuple(value.shape)}, {value.dtype})")
    y = _volume_batch(lr, as_numpy)                                      # the device last
    start, gd = (None if v is None else _volume_batch(v, as_numpy) for v in (x0, guide))
    out, change = ops.nlm_upsample(y, f, k, lv, n_iter, s, r, relax, gd, start, want_change=return_info)
    out = out.reshape(*lead, *hr)
    if as_numpy:
        out = out.cpu().numpy()
    if not return_info:
        return out
    change = change.reshape((len(lv) * n_iter,) + lead)
    return out, {"change": change.cpu().numpy() if as_numpy else change}


TVMS_DEFAULT_LAMBDA, TVMS_DEFAULT_HUBER, TVMS_DEFAULT_ITERS = 0.01, 0.01, 300  # the sweep of DESIGN.md 4o (3 stacks, noise 0.02)


class StackGeometry(tuple):
    """The immutable record ``(factors, kernels, offsets)`` of one stack (``stack_geometry``)."""
    __slots__ = ()
    factors = property(lambda self: self[0])
    kernels = property(lambda self: self[1])
    offsets = property(lambda self: self[2])

    def __repr__(self):
        return f"StackGeometry(factors={self[0]!r}, kernels={self[1]!r}, offsets={self[2]!r})"


def stack_geometry(factors, kernel="mean", offsets=(0, 0, 0)):
    """One stack of thick slices for ``stack_apply`` / ``tv_superres_stacks``: per trailing axis (slice, row, column) a spacing
    ``factors`` = (f0, f1, f2), 1 .. 8, between neighbouring LR samples, a profile and an offset in HR voxels (|o| <= 2^20, it may be
    negative): LR sample i of an axis is the profile-weighted sum of the HR samples o + f i .. o + f i + L - 1.  ``kernel``: 'mean' /
    'decimate' (length f per axis, as in ``tv_superres3d``) or a triple of 1-D arrays of ANY length 1 .. 16, each summing to 1
    (``profile_taps``): longer than f the slices overlap, shorter they leave gaps.  Returns an immutable record (factors, kernels,
    offsets)."""
    who = "stack_geometry"
    f = ops.tv_factors(who, factors, 3, whole=True)
    ks = _kernel_factors(who, kernel, f, taps=True)
    o = ops.tvms_offsets(who, offsets)
    return StackGeometry((f, tuple(tuple(k) for k in ks), o))


def profile_taps(length, spacing, kind: str = "gaussian", fwhm=None):
    """``length`` taps (1 .. 16) of a slice profile on HR sub-slice centres, centred on the footprint and normalised to sum 1, as a
    float64 ndarray: 'mean' (a box over the footprint) or 'gaussian' of full width at half maximum ``fwhm`` in units of ``spacing`` HR
    voxels (the slice spacing), sampled at the positions ``(t + 1/2 - length/2) / spacing``.  ``length == spacing`` is
    ``slice_profile``; a longer profile overlaps its neighbours.  ``fwhm`` belongs to 'gaussian' alone."""
    who = "profile_taps"
    if isinstance(length, bool) or int(length) != length or not 1 <= int(length) <= ops.TVMS_MAX_TAPS:
        raise ValueError(f"{who}: length is an integer 1 .. {ops.TVMS_MAX_TAPS} (got {length!r})")
    if isinstance(spacing, bool) or int(spacing) != spacing or not 1 <= int(spacing) <= ops.TVSR_MAX_FACTOR:
        raise ValueError(f"{who}: spacing is an integer 1 .. {ops.TVSR_MAX_FACTOR} (got {spacing!r})")
    L, f = int(length), int(spacing)
    if kind != "gaussian" and fwhm is not None:
        raise ValueError(f"{who}: fwhm belongs to kind='gaussian' (got kind={kind!r})")
    if kind == "mean":
        return _named_kernel(kind, L)
    if kind == "gaussian":
        if fwhm is None or not 0.0 < float(fwhm) < np.inf:
            raise ValueError(f"{who}: kind='gaussian' needs a finite fwhm > 0, in units of the spacing (got {fwhm!r})")
        return _gaussian_taps(who, L, f, fwhm)
    raise ValueError(f"{who}: kind must be 'gaussian' or 'mean' (got {kind!r})")


def _geometries(who, geometries):
    """One record or a sequence of them -> a list of ``StackGeometry``, 1 .. 8 of them."""
    geos = [geometries] if isinstance(geometries, StackGeometry) else list(geometries)
    ops.tvms_stack_count(who, len(geos))
    for g in geos:
        if not isinstance(g, StackGeometry):
            raise TypeError(f"{who}: every geometry is a record of stack_geometry() (got {type(g).__name__})")
    return geos


def default_lr_shape(geometry, hr_shape):
    """Per axis ``max(1, floor((N - L - o) / f) + 1)``: the LR indices from 0 to the last whose footprint lies inside the volume."""
    return tuple(max(1, (int(N) - len(k) - o) // f + 1) for N, f, k, o in zip(hr_shape, *geometry))


def stack_apply(x, geometry, lr_shape=None, return_valid: bool = False):
    """``A_s x``, one stack of thick slices of the trailing three axes (slice, row, column) of ``x``:
    ``(A x)[l][i][j] = sum k[a][b][c] x[o0 + f0 l + a][o1 + f1 i + b][o2 + f2 j + c]`` with ``geometry`` of ``stack_geometry`` and
    ``k[a][b][c] = (k1[b] k2[c]) k0[a]`` (``inr_tvms_apply``, fp64); a block stack is ``block_apply3d`` bit for bit.
    ``lr_shape`` (n0, n1, n2) defaults per axis to ``max(1, floor((N - L - o) / f) + 1)``, the indices whose footprints lie inside.
    A datum whose footprint leaves the volume is invalid and comes back 0; ``return_valid`` adds the bool mask.  Leading axes are a
    batch; ndarray in -> float64 ndarray out, device fp32 / fp64 tensor in -> the same out."""
    who = "stack_apply"
    if not isinstance(geometry, StackGeometry):
        raise TypeError(f"{who}: geometry is a record of stack_geometry() (got {type(geometry).__name__})")
    as_numpy, hr, lead = _volume_input(who, x)
    ops.tv_hr_shape3d(who, hr)
    n = default_lr_shape(geometry, hr) if lr_shape is None else lr_shape
    n = ops.tvms_lr_shape(who, n)
    flat = _volume_batch(x, as_numpy)
    res = ops.stack_apply(flat.double(), [(geometry.factors, geometry.kernels, geometry.offsets, n)], return_valid)
    out, valid = res if return_valid else (res, None)
    out = out.to(flat.dtype).reshape(*lead, *n)
    if return_valid:
        valid = valid.reshape(out.shape)
        return (out.cpu().numpy(), valid.cpu().numpy()) if as_numpy else (out, valid)
    return out.cpu().numpy() if as_numpy else out


def stack_adjoint(r, geometry, hr_shape):
    """``A_s^T r``, the adjoint of ``stack_apply``: ``r`` [..., n0, n1, n2] -> [..., D, H, W], a gather with no atomics in which invalid
    data take no part (``inr_tvms_adjoint``); for a block stack ``block_adjoint3d`` bit for bit.  Types as ``stack_apply``."""
    who = "stack_adjoint"
    if not isinstance(geometry, StackGeometry):
        raise TypeError(f"{who}: geometry is a record of stack_geometry() (got {type(geometry).__name__})")
    as_numpy, n, lead = _volume_input(who, r)
    ops.tvms_lr_shape(who, n)
    hr = ops.tv_hr_shape3d(who, hr_shape)
    flat = _volume_batch(r, as_numpy)
    out = ops.stack_adjoint(flat.double().reshape(flat.shape[0], -1), [(geometry.factors, geometry.kernels, geometry.offsets, n)], hr)
    out = out.to(flat.dtype).reshape(*lead, *hr)
    return out.cpu().numpy() if as_numpy else out


def tv_superres_stacks(stacks, geometries, hr_shape, lam: float = TVMS_DEFAULT_LAMBDA, huber: float = TVMS_DEFAULT_HUBER,
                       n_iter: int = TVMS_DEFAULT_ITERS, grad_weights=TV3D_DEFAULT_GRAD_WEIGHTS, weight=None, x0=None,
                       return_info: bool = False):
    """Multi-stack model-based reconstruction of one volume ``hr_shape`` = (D, H, W) from 1 .. 8 ``stacks`` of thick slices -- a list
    of arrays [..., n0, n1, n2] with the same leading axes and type, stack s acquired with ``geometries[s]`` of ``stack_geometry``:
    stacks of different orientation (the thick axis on different axes), stacks that differ only in their offset (slice-shifted), and
    profiles wider (overlap) or narrower (gaps) than the slice spacing.  ``n_iter`` Chambolle-Pock iterations, data and prior both
    dual, on ``1/2 sum_s sum w_s (A_s x - stacks_s)^2 + lam sum H_huber(|grad x|)`` with the prior, ``grad_weights`` and ``huber`` of
    ``tv_superres3d``.  The objective is NOT divided by the number of stacks: the data term grows with it, so ``lam`` BELONGS TO A
    STACK COUNT AND A NOISE LEVEL (the default: three orthogonal stacks at noise 0.02 of a [0, 1] volume; a noiseless design wants a
    smaller one).  A datum whose footprint leaves the volume has weight 0 and is never read (it may be NaN).  ``weight``: a list of
    the shapes of ``stacks`` (>= 0; 0 marks a missing datum) or None; ``x0`` [..., D, H, W] defaults to the normalised
    back-projection ``(sum A_s^T y_s) / (sum A_s^T 1)``.  ``inr_tvms_solve``.  ndarrays in -> float64 ndarray out;
    device fp32 / fp64 tensors in -> the same out (fp64 inside, rounded once).  There is no CPU fallback.  ``return_info``: also a
    dict with ``energy`` (the objective at the result), ``change`` (max |x' - x| of the last iteration) and ``valid_fraction`` (the
    valid share of the data), each of the leading shape."""
    who = "tv_superres_stacks"
    geos = _geometries(who, geometries)
    if isinstance(stacks, (np.ndarray, torch.Tensor)) or not hasattr(stacks, "__len__"):
        raise TypeError(f"{who}: stacks is a list of arrays, one per geometry (got {type(stacks).__name__})")
    stacks = list(stacks)
    if len(stacks) != len(geos):
        raise ValueError(f"{who}: {len(stacks)} stacks for {len(geos)} geometries")
    hr = ops.tv_hr_shape3d(who, hr_shape)
    lam, huber, n_iter = ops.tv_scalars(who, lam, huber, n_iter, ops.TVSR3D_MAX_ITER)
    g = ops.tv_grad_weights(who, grad_weights)
    as_numpy, _, lead = _volume_input(who, stacks[0], "stacks")
    table = []
    for s, (y, geo) in enumerate(zip(stacks, geos)):
        if _volume_input(who, y, "stacks")[0] != as_numpy:
            raise TypeError(f"{who}: the stacks must all be ndarrays or all device tensors")
        if tuple(y.shape[:-3]) != lead or y.dtype != stacks[0].dtype:
            raise ValueError(f"{who}: stack {s} must have the leading axes {lead} and the type of stack 0 (got {tuple(y.shape)}, {y.dtype})")
        table.append((geo.factors, geo.kernels, geo.offsets, ops.tvms_lr_shape(who, y.shape[-3:])))
    if weight is not None:
        if isinstance(weight, (np.ndarray, torch.Tensor)) or not hasattr(weight, "__len__") or len(weight) != len(stacks):
            raise TypeError(f"{who}: weight is a list of arrays, one per stack, or None")
        for s, (wv, y) in enumerate(zip(weight, stacks)):
            if isinstance(wv, np.ndarray) != as_numpy:
                raise TypeError(f"{who}: weight must be given like stacks ({'ndarrays' if as_numpy else 'device tensors'})")
            _fourier_input(who, wv)
            if tuple(wv.shape) != tuple(y.shape) or (not as_numpy and wv.dtype != y.dtype):
                raise ValueError(f"{who}: weight {s} must have shape {tuple(y.shape)} and the type of its stack "
                                 f"(got {tuple(wv.shape)}, {wv.dtype})")
            if as_numpy:
                with np.errstate(invalid="ignore"):
                    if (wv < 0).any() or np.isinf(wv).any():
                        raise ValueError(f"{who}: weight must be >= 0 and not infinite")
    if x0 is not None:
        if isinstance(x0, np.ndarray) != as_numpy:
            raise TypeError(f"{who}: x0 must be given like stacks ({'an ndarray' if as_numpy else 'a device tensor'})")
        _fourier_input(who, x0)
        if tuple(x0.shape) != lead + hr or (not as_numpy and x0.dtype != stacks[0].dtype):
            raise ValueError(f"{who}: x0 must have shape {lead + hr} and the type of stacks (got {tuple(x0.shape)}, {x0.dtype})")

    def rows(arrays):
        flat = [_volume_batch(a, as_numpy) for a in arrays]
        return torch.cat([a.reshape(a.shape[0], -1) for a in flat], dim=1).contiguous()

    y = rows(stacks)
    wt = None if weight is None else rows(weight)
    start = None if x0 is None else _volume_batch(x0, as_numpy)
    out, energy, change, valid = ops.tvms_solve(y, table, hr, lam, huber, n_iter, g, wt, start)
    return _tv_output(as_numpy, lead, out, hr, {"energy": energy, "change": change, "valid_fraction": valid}, return_info)


# the sweep of DESIGN.md 4p (k-space truncation and a Gaussian PSF, x2, noise 0.02 of a [0, 1] image)
TVOP_DEFAULT_LAMBDA, TVOP_DEFAULT_HUBER, TVOP_DEFAULT_ITERS = 3e-3, 0.03, 500


def psf_operator(n, m, fwhm, kind: str = "gaussian"):
    """The operator [m][n] of one axis for a point-spread function wider (or narrower) than the pixel, a float64 ndarray formed on the
    host: row ``i`` is centred on HR sample ``(i + 1/2) n / m - 1/2`` -- pixel centres, any ratio ``n / m`` -- and has the full width at
    half maximum ``fwhm`` in LR pixels.  'gaussian': the Gaussian sampled at the HR samples; 'box': the overlap of a box of that width
    with every sample's unit cell (``fwhm = 1`` on a whole ratio is the block mean).  Every row is normalised to sum 1 over the samples
    inside the line.  For ``tv_superres_operator``, ``operator_apply`` and ``operator_adjoint``."""
    who = "psf_operator"
    for name, v in (("n", n), ("m", m)):
        if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= ops.TVSR_MAX_SIDE:
            raise ValueError(f"{who}: {name} is an integer 1 .. {ops.TVSR_MAX_SIDE} (got {v!r})")
    if kind not in ("gaussian", "box"):
        raise ValueError(f"{who}: kind must be 'gaussian' or 'box' (got {kind!r})")
    try:
        ok = 0.0 < float(fwhm) < np.inf
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{who}: fwhm must be finite and > 0, in LR pixels (got {fwhm!r})")
    n, m = int(n), int(m)
    centre = (np.arange(m) + 0.5) * n / m - 0.5
    j = np.arange(n, dtype=np.float64)
    width = float(fwhm) * n / m                                     # in HR samples
    if kind == "gaussian":
        sigma = width / (2.0 * np.sqrt(2.0 * np.log(2.0)))
        op = np.exp(-0.5 * ((j[None, :] - centre[:, None]) / sigma) ** 2)
    else:
        lo, hi = centre[:, None] - width / 2.0, centre[:, None] + width / 2.0
        op = np.clip(np.minimum(hi, j[None, :] + 0.5) - np.maximum(lo, j[None, :] - 0.5), 0.0, None)
    total = op.sum(axis=1, keepdims=True)
    if not (total > 0.0).all():
        raise ValueError(f"{who}: fwhm {fwhm!r} is too narrow: a row of the operator holds no sample")
    return op / total


def block_operator(n, f, kernel="mean"):
    """The dense form [n / f][n] of a 1-D block kernel, a float64 ndarray: ``op[i][f i + a] = kernel[a]`` -- 'mean' (1 / f), 'decimate'
    (the block's first sample) or ``f`` finite values that sum to 1.  ``(block_operator(H, f0, k0), block_operator(W, f1, k1))`` is the
    operator of ``block_apply`` with the kernel ``outer(k0, k1)``."""
    who = "block_operator"
    if isinstance(f, bool) or int(f) != f or not 1 <= int(f) <= ops.TVSR_MAX_FACTOR:
        raise ValueError(f"{who}: f is an integer 1 .. {ops.TVSR_MAX_FACTOR} (got {f!r})")
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= ops.TVSR_MAX_SIDE or int(n) % int(f):
        raise ValueError(f"{who}: n is an integer 1 .. {ops.TVSR_MAX_SIDE} and a whole number of blocks of {f} (got {n!r})")
    n, f = int(n), int(f)
    if isinstance(kernel, str):
        k = _named_kernel(kernel, f)
        if k is None:
            raise ValueError(f"{who}: kernel must be 'mean', 'decimate' or {f} values (got {kernel!r})")
    else:
        k = np.asarray(kernel, dtype=np.float64)
        if k.shape != (f,):
            raise ValueError(f"{who}: the kernel array must have {f} entries (got shape {k.shape})")
        if not np.isfinite(k).all() or abs(k.sum() - 1.0) > 1e-9:
            raise ValueError(f"{who}: the kernel array must be finite and sum to 1 (got sum {k.sum()!r})")
    op = np.zeros((n // f, n))
    for i in range(n // f):
        op[i, f * i:f * i + f] = k
    return op


def _operator_pair(who, operators):
    """``operators`` = (R0 [h, H], R1 [w, W]), float64 ndarrays (finite) or device float64 tensors -> (getter of the device pair, H, W,
    h, w), refusing by name.  Touches no device until the getter is called."""
    r0, r1 = ops.tvop_operator_pair(who, operators)
    sides = []
    for name, r in (("operators[0]", r0), ("operators[1]", r1)):
        if isinstance(r, np.ndarray):
            if r.dtype != np.float64:
                raise TypeError(f"{who}: {name} must be float64 (got {r.dtype})")
            if r.ndim == 2 and not np.isfinite(r).all():
                raise ValueError(f"{who}: {name} must be finite")
        elif isinstance(r, torch.Tensor):
            if r.dtype != torch.float64:
                raise TypeError(f"{who}: {name} must be float64 (got {r.dtype})")
            if not r.is_cuda:
                raise ops.InrDeviceError(f"{who}: {name} is on {r.device}; pass an ndarray or a device tensor (there is no CPU fallback)")
        else:
            raise TypeError(f"{who}: {name} must be a float64 ndarray or a device float64 tensor (got {type(r).__name__})")
        sides.append(ops.tvop_operator_shape(who, name, r.shape))
    (h, H), (w, W) = sides

    def device_pair():
        dev = ops.require_gpu()
        return tuple((torch.from_numpy(np.ascontiguousarray(r)).to(dev) if isinstance(r, np.ndarray) else r.contiguous()) for r in (r0, r1))

    return device_pair, H, W, h, w


def _operator_through(who, image, operators, forward):
    pair, H, W, h, w = _operator_pair(who, operators)
    as_numpy, rows, cols, lead = _block_input(who, image)
    src, dst = ((H, W), (h, w)) if forward else ((h, w), (H, W))
    if (rows, cols) != src:
        raise ValueError(f"{who}: the operators take images of {src[0]} x {src[1]} (got {rows} x {cols})")
    flat = _block_batch(image, as_numpy)
    out = (ops.tvop_apply if forward else ops.tvop_adjoint)(flat.double(), pair()).to(flat.dtype).reshape(*lead, *dst)
    return out.cpu().numpy() if as_numpy else out


def operator_apply(x, operators):
    """``A x = R0 x R1^T`` on the trailing two axes of ``x`` [..., H, W] -> [..., h, w]; ``operators`` = (R0 [h, H], R1 [w, W]) as
    float64 ndarrays or device float64 tensors (``fourier_operator``, ``psf_operator``, ``block_operator`` or any other).  Two fp64
    GEMM launches (``inr_tvop_apply``).  ndarray in -> float64 ndarray out, device fp32 / fp64 tensor in -> the same out (fp64
    inside, rounded once)."""
    return _operator_through("operator_apply", x, operators, True)


def operator_adjoint(r, operators):
    """``A^T r = R0^T r R1`` on the trailing two axes of ``r`` [..., h, w] -> [..., H, W] (``inr_tvop_adjoint``); types as
    ``operator_apply``."""
    return _operator_through("operator_adjoint", r, operators, False)


def tv_superres_operator(lr, operators, lam: float = TVOP_DEFAULT_LAMBDA, huber: float = TVOP_DEFAULT_HUBER,
                         n_iter: int = TVOP_DEFAULT_ITERS, weight=None, x0=None, return_info: bool = False):
    """Model-based super-resolution under ANY separable linear acquisition model: ``lr`` [..., h, w] was made as ``A x = R0 x R1^T``
    with ``operators`` = (R0 [h, H], R1 [w, W]), float64 ndarrays (finite) or device float64 tensors shared by the whole batch --
    k-space truncation (``fourier_operator``), a point-spread function wider than the pixel (``psf_operator``), a ratio that is no
    whole number, a block kernel (``block_operator``).  ``n_iter`` Chambolle-Pock iterations, data and prior both dual, on
    ``1/2 sum w (A x - lr)^2 + lam sum H_huber(|grad x|)`` with the prior of ``tv_superres``; the step comes from a bound on the
    operators' norms formed on the device.  The defaults are those of data in [0, 1] at noise 0.02; scale ``lam`` and
    ``huber`` with the data's range.  ``weight`` (shape of ``lr``, >= 0; 0 marks a missing datum, which is never read) defaults to 1,
    ``x0`` [..., H, W] to the normalised back-projection through the absolute operators.  ``inr_tvop_solve2d``.
    ndarray in -> float64 ndarray out; device fp32 / fp64 tensor in -> the same out (fp64 inside, rounded once); ``weight`` / ``x0``
    are given like ``lr``.  There is no CPU fallback.  ``return_info``: also a dict with ``energy`` (the objective at the result) and
    ``change`` (max |x' - x| of the last iteration), both of the leading shape."""
    who = "tv_superres_operator"
    pair, H, W, h, w = _operator_pair(who, operators)
    lam, huber, n_iter = ops.tv_scalars(who, lam, huber, n_iter, ops.TVSR3D_MAX_ITER, "in 0 ..")
    as_numpy, rows, cols, lead = _block_input(who, lr, "lr")
    if (rows, cols) != (h, w):
        raise ValueError(f"{who}: the operators make LR images of {h} x {w} (got lr of {rows} x {cols})")
    extra = _weight_and_start(who, lr, as_numpy, lead, weight, (h, w), x0, (H, W))
    y = _block_batch(lr, as_numpy)
    out, energy, change = ops.tvop_solve(y, pair(), lam, huber, n_iter, extra["weight"], extra["x0"])
    return _tv_output(as_numpy, lead, out, (H, W), {"energy": energy, "change": change}, return_info)


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
