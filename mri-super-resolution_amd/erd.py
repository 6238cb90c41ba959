"""AutoERD acceptance weights of the 2-D slice driver (master.py:77-93) on the device.

The reference loops over the ROI in Python and fits one ``sklearn.cluster.AgglomerativeClustering(n_clusters=2,
linkage='complete')`` per pixel (3,600 fits per case) to mark outlying acquisitions in ``case.accept``; ``inr_auto_erd`` does
all pixels in one launch with the same partition, ties included (csrc/metrics.hip).

``erd_volume`` and its companions are david.py:44-91 -- the same clustering on every pixel of whole slices and volumes, the
plain and the ERD-accepted mean per gradient direction and their ADC maps -- in one launch of csrc/erd_volume.hip.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from . import ops
from ._lib import check, lib


def auto_erd(img, rule: int, erd_map=None) -> np.ndarray:
    """``img`` [H, W, n_acquisitions] (all acquisitions of one slice, any real dtype) -> accept [H, W, n] of 0 / 1 (int64, the
    dtype of ``case.accept``).  ``rule`` 1 = majority voting (--erd 1), 2 = intensity-cognisant (--erd 2; ``erd_map`` [H, W]:
    pixels where it is not positive keep everything, master.py:89).  A pixel holding a non-finite value, or finite values whose
    largest difference overflows, is not clustered and keeps every acquisition, as in ``erd_volume``."""
    dev = ops.require_gpu()
    a = np.ascontiguousarray(np.asarray(img), dtype=np.float64)
    if a.ndim != 3:
        raise ValueError("img must be [H, W, n_acquisitions]")
    H, W, n = a.shape
    vals = torch.from_numpy(a.reshape(H * W, n)).to(dev)
    emap = None
    if erd_map is not None:
        e = np.ascontiguousarray(np.asarray(erd_map), dtype=np.float32)
        if e.shape != (H, W):
            raise ValueError(f"erd_map must be [{H}, {W}]")
        emap = torch.from_numpy(e.reshape(-1)).to(dev)
    out = torch.empty((H * W, n), dtype=torch.float32, device=dev)
    check(lib().inr_auto_erd(out.data_ptr(), vals.data_ptr(), 0 if emap is None else emap.data_ptr(), H * W, n, int(rule),
                             torch.cuda.current_stream().cuda_stream), "inr_auto_erd")
    return out.cpu().numpy().reshape(H, W, n).astype(np.int64)


def apply_auto_erd(case, rule: int, roi_begin: int, roi_end: int) -> None:
    """master.py:77-93 on a ``contrast.case``: clears ``case.accept`` inside the ROI of the cancer slice for the rejected
    acquisitions (rule 2 needs ``case.erd``)."""
    s = case.cancer_slice
    img = case.dwi[roi_begin:roi_end, roi_begin:roi_end, s, :]
    emap = None
    if rule == 2:
        if case.erd is None:
            raise ValueError("--erd 2 needs the patient's ERD map (pat<NN>_ERD.mat: ADC_alldata_mm_ERD)")
        emap = case.erd[roi_begin:roi_end, roi_begin:roi_end, s]
    keep = auto_erd(img, rule, emap)
    block = case.accept[roi_begin:roi_end, roi_begin:roi_end, s, :]
    block[keep == 0] = 0


# ---- whole slices and volumes (david.py:44-91): csrc/erd_volume.hip ----------------------------------------------------------------
_TORCH_WRAPS = tuple(np.dtype(t) for t in (np.float32, np.float64, np.int8, np.int16, np.int32, np.int64, np.uint8))
ErdVolume = collections.namedtuple("ErdVolume", "accept direction_mean accepted_mean direction_adc accepted_adc adc")


def _device_f64(a, name, shape=None):
    """ndarray of any real dtype or device tensor -> device float64 tensor (the conversion runs on the device; float64 holds
    every float32, float64 and 16- / 32-bit integer value exactly)."""
    if isinstance(a, np.ndarray):
        if a.dtype.kind not in "fiub":
            raise TypeError(f"{name} must be real-valued (got {a.dtype})")
        if a.dtype.newbyteorder("=") not in _TORCH_WRAPS or not a.dtype.isnative:      # widened on the host, exactly
            a = a.astype(np.int32 if a.dtype.kind in "ub" and a.dtype.itemsize <= 2 else np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(ops.require_gpu())
    elif isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise ops.InrDeviceError(f"{name} is on {a.device}: the ERD kernels only run on a HIP device (there is no CPU fallback)")
        if a.is_complex():
            raise TypeError(f"{name} must be real-valued (got {a.dtype})")
        t = a
    else:
        raise TypeError(f"{name} must be a numpy.ndarray or a device tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {list(shape)} (got {list(t.shape)})")
    return t.to(torch.float64)


def _planes(t, n):
    """[..., n] pixel-major -> [n][P] acquisition-major planes, on the device."""
    return t.reshape(-1, n).t().contiguous()


def erd_volume(dwi, b0, acquisitions, b, rule: int = 1, erd_map=None, accept=None, per_acquisition_adc: bool = False) -> ErdVolume:
    """david.py:44-91 for every pixel of ``dwi`` [..., n] in one launch: AutoERD (``rule`` 1 = majority voting, 2 = intensity-
    cognisant with ``erd_map`` [...], only its positive entries reject; 0 = no clustering: ``accept`` [..., n], or all ones, is
    used as it is), then per group of ``acquisitions`` (sizes of consecutive groups, at most 8, summing to n) the plain and the
    accepted mean and the ADC ``-log(v / (b0 + 1e-7) + 1e-7) / b * 1000`` of both, all float64.

    Returns ``ErdVolume(accept [..., n], direction_mean, accepted_mean, direction_adc, accepted_adc [G, ...], adc)``; ``adc`` is
    the ADC of every single acquisition [..., n] with ``per_acquisition_adc``, else None.  ``accepted_mean`` is NaN where a whole
    group is rejected.  A pixel holding a non-finite value is not clustered and keeps every acquisition.  ndarrays in give
    ndarrays out (``accept`` int64 under rules 1 and 2, like ``auto_erd``); device tensors in give float64 device tensors out
    with no host sync."""
    as_numpy = isinstance(dwi, np.ndarray)
    x = _device_f64(dwi, "dwi")
    if x.dim() < 1:
        raise ValueError("dwi must be [..., n_acquisitions]")
    lead, n = tuple(x.shape[:-1]), int(x.shape[-1])
    groups = [int(g) for g in np.asarray(acquisitions).reshape(-1)]
    rule = int(rule)
    if accept is not None and rule != 0:
        raise ValueError("accept= supplies the weights of rule 0; rules 1 and 2 compute them")
    dev = x.device
    P = int(np.prod(lead, dtype=np.int64))
    vals = _planes(x, n) if n > 0 else x.reshape(0, P)
    b0_t = _device_f64(b0, "b0", lead).reshape(-1).contiguous()
    emap = None if erd_map is None else _device_f64(erd_map, "erd_map", lead).reshape(-1).contiguous()
    acc_in = None if accept is None else _planes(_device_f64(accept, "accept", lead + (n,)), n)
    G = len(groups)
    acc = torch.empty((n, P), dtype=torch.float64, device=dev)
    maps = torch.empty((4, G, P), dtype=torch.float64, device=dev)
    adc = torch.empty((n, P), dtype=torch.float64, device=dev) if per_acquisition_adc else None
    check(lib().inr_auto_erd_volume(acc.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(), maps[3].data_ptr(),
                               ops._ptr(adc), vals.data_ptr(), b0_t.data_ptr(), ops._ptr(emap), ops._ptr(acc_in), P, n,
                               (C.c_int * max(G, 1))(*groups), G, float(b), rule, ops._stream()), "inr_auto_erd_volume")
    acc = acc.t().reshape(lead + (n,))
    adc = None if adc is None else adc.t().reshape(lead + (n,))
    maps = maps.reshape((4, G) + lead)
    if not as_numpy:
        return ErdVolume(acc.contiguous(), maps[0], maps[1], maps[2], maps[3], None if adc is None else adc.contiguous())
    acc = np.ascontiguousarray(acc.cpu().numpy())
    m = maps.cpu().numpy()
    return ErdVolume(acc.astype(np.int64) if rule else acc, m[0], m[1], m[2], m[3],
                     None if adc is None else np.ascontiguousarray(adc.cpu().numpy()))


def auto_erd_volume(dwi, rule: int, erd_map=None):
    """The acceptance array [..., n] of ``erd_volume`` alone (rule 1 or 2), for any number of leading axes."""
    as_numpy = isinstance(dwi, np.ndarray)
    x = _device_f64(dwi, "dwi")
    if x.dim() < 1:
        raise ValueError("dwi must be [..., n_acquisitions]")
    lead, n = tuple(x.shape[:-1]), int(x.shape[-1])
    if int(rule) not in (1, 2):
        raise ValueError("rule must be 1 (majority voting) or 2 (intensity-cognisant)")
    P = int(np.prod(lead, dtype=np.int64))
    vals = _planes(x, n) if n > 0 else x.reshape(0, P)
    emap = None if erd_map is None else _device_f64(erd_map, "erd_map", lead).reshape(-1).contiguous()
    acc = torch.empty((n, P), dtype=torch.float64, device=x.device)
    check(lib().inr_auto_erd_volume(acc.data_ptr(), 0, 0, 0, 0, 0, vals.data_ptr(), 0, ops._ptr(emap), 0, P, n, (C.c_int * 1)(n), 1, 1.0,
                               int(rule), ops._stream()), "inr_auto_erd_volume")
    acc = acc.t().reshape(lead + (n,))
    return acc.cpu().numpy().astype(np.int64) if as_numpy else acc.contiguous()


def case_slices(case, slices):
    """``"cancer"`` -> [case.cancer_slice], ``"all"`` -> every slice, else the iterable's slice indices."""
    if isinstance(slices, str):
        if slices == "cancer":
            return [int(case.cancer_slice)]
        if slices == "all":
            return list(range(case.dwi.shape[2]))
        raise ValueError(f"slices must be 'cancer', 'all' or an iterable of slice indices (got {slices!r})")
    return [int(s) for s in slices]


def apply_auto_erd_volume(case, rule: int, slices="cancer") -> None:
    """david.py:47-55 on a ``contrast.case``, for whole slices and any number of them in one launch: clears ``case.accept`` for
    the rejected acquisitions of every pixel of ``slices`` (rule 2 needs ``case.erd``; its -inf entries keep everything)."""
    idx = case_slices(case, slices)
    emap = None
    if rule == 2:
        if case.erd is None:
            raise ValueError("--erd 2 needs the patient's ERD map (pat<NN>_ERD.mat: ADC_alldata_mm_ERD)")
        emap = np.asarray(case.erd)[:, :, idx]
    keep = auto_erd_volume(np.asarray(case.dwi)[:, :, idx, :], rule, emap)
    block = case.accept[:, :, idx, :]
    block[keep == 0] = 0
    case.accept[:, :, idx, :] = block
