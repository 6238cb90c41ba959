"""The interpolation baselines the reference reports its results against, on the device.

``rescale`` is ``skimage.transform.rescale(image, scale, anti_aliasing=True)`` as called at superresDWI.py:172-191 and
master.py:175 for up-scaling 2-D images: default order 1, mode 'reflect' -- which skimage 0.20 evaluates as
``scipy.ndimage.zoom(image, scale, order=1, mode='mirror', grid_mode=True)``; the anti-aliasing Gaussian has sigma
``max(0, (1/scale - 1)/2) = 0`` when ``scale >= 1``.  scikit-image itself is not installed in the build image: parity with
skimage is therefore UNPINNED; the kernel is pinned against the scipy call skimage makes (tests).  Down-scaling (a real
anti-aliasing filter) is not needed by the drivers and is rejected.

``resize_z`` is ``resize_array(arr, new_size, kind='cubic')`` (SRDWI.py:132-141), the through-plane baseline of
superresDWI.py:231: scipy's ``interp1d(kind='cubic')`` -- a not-a-knot cubic spline -- along the last axis, in fp64
(``inr_resize_z_cubic``).
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
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
