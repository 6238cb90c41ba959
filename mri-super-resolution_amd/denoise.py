"""Denoising of the multi-measurement acquisition stack before any fit: Marchenko-Pastur PCA (Veraart et al., NeuroImage 2016; the
cutoff estimators of Cordero-Grande et al. 2019) on the HIP kernel of csrc/mppca.hip (``inr_mppca_denoise``).

The reference's later driver (inrDWI.py:44) fits ``hybrid_raw_clean``, the multi-b / multi-TE stack after a denoising step made outside
its tree; ``mppca`` is that step, ``stack_hybrid`` / ``unstack_hybrid`` turn the ``[b][TE]`` cell of a ``master.mat`` into the
measurement-major stack it takes and back, and ``scripts/denoise.py`` writes the clean cell.  Every voxel of the 16 to ~40
measurements spans only a few signal components: the spectrum of the M x N matrix of a voxel's window tells the noise level and how many
components are noise, and the voxel is projected onto the others.  The noise map ``sigma`` comes with it.

``degibbs`` / ``degibbs_lines`` are the step that follows it in every pipeline (``mrdegibbs`` after ``dwidenoise``): Gibbs-ringing
removal by local sub-voxel shifts (Kellner et al., MRM 2016) on the HIP kernels of csrc/degibbs.hip (``inr_degibbs2d``,
``inr_degibbs_lines``).  An MR image is a truncated Fourier series, so every edge rings with a period of one acquired
pixel; MP-PCA cannot remove that, it is signal.  The data must lie on the acquired grid -- scanner-interpolated or partial-Fourier data
ring at another period and are not served -- and the 3-D variant is out of scope.

``nlm`` is the non-local-means filter in its MRI form (Rician bias correction, a noise level per voxel) on the HIP kernel of csrc/nlm.hip
(``inr_nlm3d``): the consumer of the noise map that ``mppca`` returns.  There is no CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from . import ops

DEFAULT_WINDOW = (5, 5, 5)
ESTIMATORS = tuple(ops.MPPCA_ESTIMATORS)
DEGIBBS_DEFAULT_SHIFTS, DEGIBBS_DEFAULT_WINDOW = ops.DEGIBBS_DEFAULT_SHIFTS, ops.DEGIBBS_DEFAULT_WINDOW


def mppca(data, window=DEFAULT_WINDOW, mask=None, estimator="exp2", return_info=False, measurement_axis=0):
    """MP-PCA denoising of ``data`` [M, D, H, W] (``measurement_axis=0``) or [X, Y, Z, M] (``measurement_axis=-1``, the layout of the
    drivers); a 3-D input [M, H, W] (or [X, Y, M]) is one slice, and takes a window (1, a, b) or its two in-plane sides (a, b).
    ``data``: an ndarray (any real dtype; float64 inside and out) or a device tensor (float32 or float64, returned as given).
    ``window``: three odd sides over the volume axes in the order they have in ``data``, each at most its axis -- larger sides are
    refused by name, not shrunk.  ``mask``: the volume's shape, non-zero inside; outside it the data pass through.  ``estimator``:
    'exp2' (the default) or 'exp1'.  Returns the denoised data like ``data``; with ``return_info`` also a dict with ``sigma`` (the
    noise map, the volume's shape) and ``rank`` (the number of signal components, int32; -1 outside the mask, -2 where the
    eigensolver did not converge -- data that is not finite)."""
    who = "mppca"
    if measurement_axis not in (0, -1):
        raise ValueError(f"{who}: measurement_axis must be 0 or -1 (got {measurement_axis!r})")
    as_numpy = isinstance(data, np.ndarray)
    if not as_numpy:
        if not isinstance(data, torch.Tensor):
            raise TypeError(f"{who} takes an ndarray or a device tensor (got {type(data).__name__})")
        if not data.is_cuda:
            raise ops.InrDeviceError(f"{who}: the tensor is on {data.device}; pass an ndarray or a device tensor (there is no CPU fallback)")
        if data.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{who}: device tensors must be float32 or float64 (got {data.dtype})")
    if data.ndim not in (3, 4):
        raise ValueError(f"{who}: data must be [M, D, H, W] or one slice [M, H, W] (got shape {tuple(data.shape)})")
    if estimator not in ops.MPPCA_ESTIMATORS:
        raise ValueError(f"{who}: estimator must be 'exp1' or 'exp2' (got {estimator!r})")
    one_slice = data.ndim == 3
    window = tuple(window)
    if one_slice and len(window) == 2:
        window = (1,) + window
    last = measurement_axis == -1
    volume = tuple(data.shape[:-1] if last else data.shape[1:])
    M = int(data.shape[-1] if last else data.shape[0])
    if one_slice:
        volume = (1,) + volume
    window = ops.mppca_window(who, window, volume, M)               # host-only refusals come before the device is asked for
    if mask is not None and tuple(mask.shape) != (volume[1:] if one_slice else volume):
        raise ValueError(f"{who}: mask has shape {tuple(mask.shape)}, expected {volume[1:] if one_slice else volume}")
    device = ops.require_gpu() if as_numpy else data.device
    x = torch.from_numpy(np.array(data, dtype=np.float64, order="C")).to(device) if as_numpy else data
    if last:
        x = x.movedim(-1, 0)
    x = x.reshape((M,) + volume).contiguous()
    m = None
    if mask is not None:
        m = torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0)) if isinstance(mask, np.ndarray) else (mask != 0)
        m = m.to(device).reshape(volume).contiguous().view(torch.uint8)
    out, sigma, rank = ops.mppca_denoise(x, window, m, estimator, want_sigma=return_info, want_rank=return_info)
    shape_v = volume[1:] if one_slice else volume
    out = out.reshape((M,) + shape_v)
    if last:
        out = out.movedim(0, -1).contiguous()
    if as_numpy:
        out = out.cpu().numpy()
    if not return_info:
        return out
    sigma, rank = sigma.reshape(shape_v), rank.reshape(shape_v)
    if as_numpy:
        sigma, rank = sigma.cpu().numpy(), rank.cpu().numpy()
    return out, {"sigma": sigma, "rank": rank}


def _degibbs_input(who, data):
    """True for an ndarray; refuses everything that is neither an ndarray nor a device float32 / float64 tensor."""
    if isinstance(data, np.ndarray):
        if data.dtype.kind not in "fiu" or data.dtype == np.float16:
            raise TypeError(f"{who}: an ndarray must be real and at least float32 (got {data.dtype})")
        return True
    if not isinstance(data, torch.Tensor):
        raise TypeError(f"{who} takes an ndarray or a device tensor (got {type(data).__name__})")
    if data.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{who}: device tensors must be float32 or float64 (got {data.dtype})")
    if not data.is_cuda:
        raise ops.InrDeviceError(f"{who}: the tensor is on {data.device}; pass an ndarray or a device tensor (there is no CPU fallback)")
    return False


def _axis(who, axis, ndim):
    if isinstance(axis, bool) or int(axis) != axis or not -ndim <= axis < ndim:
        raise ValueError(f"{who}: axis {axis!r} is out of range for {ndim} axes")
    return int(axis) % ndim


def degibbs(data, axes=(-2, -1), nshifts=DEGIBBS_DEFAULT_SHIFTS, window=DEGIBBS_DEFAULT_WINDOW, return_info=False):
    """Gibbs-ringing removal of the images spanned by the two ``axes`` of ``data``; every other axis is batch (``axes=(0, 1)`` serves
    the drivers' [X, Y, Z, M] layout; axes that are not the last two are moved and made contiguous here).  ``data``: an ndarray (any
    real dtype; float64 inside and out) or a device tensor (float32 or float64, returned as given).  ``nshifts``: sub-pixel shifts per
    side, 1 .. 64; ``window``: (w_min, w_max) of the oscillation measure, 1 <= w_min <= w_max <= 8; each image side needs
    2 w_max + 3 .. 1024 samples.  Returns the unrung data like ``data``; with ``return_info`` also a dict with ``shift`` [2, ...], the
    chosen shifts in pixels (float64) of the pass along ``axes[0]`` and of the pass along ``axes[1]``."""
    who = "degibbs"
    as_numpy = _degibbs_input(who, data)
    if data.ndim < 2 or len(tuple(axes)) != 2:
        raise ValueError(f"{who}: data needs at least 2 axes and axes names two of them (got shape {tuple(data.shape)}, axes {axes!r})")
    a0, a1 = (_axis(who, a, data.ndim) for a in axes)
    if a0 == a1:
        raise ValueError(f"{who}: axes must be two different axes (got {axes!r})")
    nshifts, w_min, w_max = ops.degibbs_params(who, (data.shape[a0], data.shape[a1]), nshifts, window)   # host-only refusals first
    device = ops.require_gpu() if as_numpy else data.device
    x = torch.from_numpy(np.array(data, dtype=np.float64, order="C")).to(device) if as_numpy else data
    moved = x.movedim((a0, a1), (-2, -1))
    batch = tuple(moved.shape[:-2])
    H, W = moved.shape[-2:]
    out, choice = ops.degibbs2d(moved.reshape((-1, H, W)).contiguous(), nshifts, (w_min, w_max), want_choice=return_info)
    out = out.reshape(batch + (H, W)).movedim((-2, -1), (a0, a1)).contiguous()
    if as_numpy:
        out = out.cpu().numpy()
    if not return_info:
        return out
    shift = ops.degibbs_shift(choice, nshifts).reshape((2,) + batch + (H, W)).movedim((-2, -1), (a0 + 1, a1 + 1)).contiguous()
    return out, {"shift": shift.cpu().numpy() if as_numpy else shift}


def degibbs_lines(x, axis=-1, nshifts=DEGIBBS_DEFAULT_SHIFTS, window=DEGIBBS_DEFAULT_WINDOW, return_info=False):
    """The 1-D operation of ``degibbs`` on the lines of ``x`` along ``axis`` (periodic lines on the acquired grid); input, output and
    ``return_info`` (``shift``, the shape of ``x``) as for ``degibbs``."""
    who = "degibbs_lines"
    as_numpy = _degibbs_input(who, x)
    if x.ndim < 1:
        raise ValueError(f"{who}: x needs at least 1 axis")
    ax = _axis(who, axis, x.ndim)
    nshifts, w_min, w_max = ops.degibbs_params(who, (x.shape[ax],), nshifts, window)
    device = ops.require_gpu() if as_numpy else x.device
    t = torch.from_numpy(np.array(x, dtype=np.float64, order="C")).to(device) if as_numpy else x
    moved = t.movedim(ax, -1)
    out, choice = ops.degibbs_lines(moved.reshape((-1, moved.shape[-1])).contiguous(), nshifts, (w_min, w_max), want_choice=return_info)
    out = out.reshape(moved.shape).movedim(-1, ax).contiguous()
    if as_numpy:
        out = out.cpu().numpy()
    if not return_info:
        return out
    shift = ops.degibbs_shift(choice, nshifts).reshape(moved.shape).movedim(-1, ax).contiguous()
    return out, {"shift": shift.cpu().numpy() if as_numpy else shift}


def _nlm_like(who, name, value, shape):
    """``value`` (an ndarray or a tensor) as a tensor, refused by name unless it has ``shape``."""
    if isinstance(value, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(value, dtype=np.float64))
    elif isinstance(value, torch.Tensor):
        t = value
    else:
        raise TypeError(f"{who}: {name} must be an ndarray or a tensor (got {type(value).__name__})")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def nlm(data, sigma, beta=1.0, search=3, patch=1, guide=None, rician=False, mask=None, center="max"):
    """Non-local-means denoising (Buades et al. 2005; for MRI Wiest-Daessle et al. 2008, Manjon et al. 2008) on the HIP kernel of
    csrc/nlm.hip (``inr_nlm3d``).  The trailing three axes of ``data`` are the volume (a 2-D input is one image, D = 1),
    leading axes a batch.  ``data``: an ndarray (any real dtype; float64 inside and out) or a device tensor (float32 or float64,
    returned as given).  ``sigma``: the noise level, a number or an array of the volume's shape -- ``mppca(..., return_info=True)``
    returns one; the strength is ``h2 = 2 beta sigma^2`` per voxel, and a voxel whose strength is not > 0 passes through.  ``search``
    / ``patch``: the radii of the search box (0 .. 5) and of the patch (0 .. 2), an int or a triple over the volume's axes.  ``guide``:
    None (each volume guides itself), 'mean' (the mean over the leading axes guides all of them: one group of at most 16 channels that
    share their weights -- the measurements of one acquisition) or an array of the volume's shape.  ``rician``: average the squares
    and remove the bias ``2 sigma^2`` (magnitude data).  ``mask``: the volume's shape, non-zero inside; outside it the data pass
    through.  ``center``: 'max' (the centre voxel weighs as much as its best neighbour) or 'one'.  There is no CPU fallback."""
    who = "nlm"
    as_numpy = _degibbs_input(who, data)
    if data.ndim < 2:
        raise ValueError(f"{who}: data needs at least 2 axes (got shape {tuple(data.shape)})")
    image = data.ndim == 2
    given = tuple(int(v) for v in (data.shape if image else data.shape[-3:]))      # the volume as the caller sees it
    volume = (1,) + given if image else given
    lead = () if image else tuple(int(v) for v in data.shape[:-3])
    s, r = ops.nlm_radii(who, search, patch)                                         # host-only refusals come before the device
    if image:
        if (isinstance(search, (tuple, list)) and s[0]) or (isinstance(patch, (tuple, list)) and r[0]):
            raise ValueError(f"{who}: an image has no first axis to search (got search {search!r}, patch {patch!r})")
        s, r = (0,) + s[1:], (0,) + r[1:]
    ops.nlm_center(who, center)
    ops.nlm_volume(who, volume)
    beta = float(beta)
    if not (np.isfinite(beta) and beta > 0.0):
        raise ValueError(f"{who}: beta must be finite and > 0 (got {beta!r})")
    if sigma is None:
        raise ValueError(f"{who}: sigma is required: a number or an array of the volume's shape {given}")
    sigma_map = None
    if isinstance(sigma, (np.ndarray, torch.Tensor)) and sigma.ndim > 0:
        sigma_map = _nlm_like(who, "sigma", sigma, given)
    else:
        try:
            sigma = float(sigma)
        except (TypeError, ValueError):
            raise TypeError(f"{who}: sigma must be a number, an ndarray or a tensor (got {type(sigma).__name__})") from None
        if not (np.isfinite(sigma) and sigma > 0.0):
            raise ValueError(f"{who}: a scalar sigma must be finite and > 0 (got {sigma!r})")
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    shared = guide is not None
    if isinstance(guide, str):
        if guide != "mean":
            raise ValueError(f"{who}: guide must be None, 'mean' or an array of the volume's shape (got {guide!r})")
        if n > ops._lib.INR_NLM_MAX_CHANNELS:
            raise ValueError(f"{who}: guide='mean' filters the leading axes as one group of at most {ops._lib.INR_NLM_MAX_CHANNELS} channels "
                             f"(got {n}): split them")
    elif guide is not None:
        guide = _nlm_like(who, "guide", guide, given)
    if mask is not None:
        mask = _nlm_like(who, "mask", mask, given)
    device = ops.require_gpu() if as_numpy else data.device
    x = torch.from_numpy(np.array(data, dtype=np.float64, order="C")).to(device) if as_numpy else data
    x = x.reshape((n,) + volume).contiguous()
    dtype = x.dtype

    def per_group(t, groups):
        return None if t is None else t.to(device=device, dtype=dtype).reshape((1,) + volume).expand((groups,) + volume).contiguous()

    if sigma_map is not None:
        sg = sigma_map.to(device=device, dtype=torch.float64)
        h2_one, s2_one = (2.0 * beta) * sg * sg, sg * sg
    else:
        h2_one = None
        s2_one = torch.full(volume, sigma * sigma, dtype=torch.float64, device=device) if rician else None
    if not rician:
        s2_one = None
    m_one = None if mask is None else (mask.to(device) != 0).reshape((1,) + volume)
    if isinstance(guide, str):
        g_one = x.mean(dim=0)
    else:
        g_one = guide

    def run(xs, groups, chans, gd):
        h2 = per_group(h2_one, groups) if h2_one is not None else 2.0 * beta * sigma * sigma
        mk = None if m_one is None else m_one.expand((groups,) + volume).contiguous().view(torch.uint8)
        return ops.nlm3d(xs.reshape((groups, chans) + volume), h2, s, r, gd, per_group(s2_one, groups), mk, center)

    if not shared:
        out = run(x, n, 1, None)
    else:
        gd = per_group(g_one, 1)
        step = ops._lib.INR_NLM_MAX_CHANNELS
        out = torch.cat([run(x[i:i + step], 1, min(step, n - i), gd).reshape((-1,) + volume) for i in range(0, n, step)]) if n else x.clone()
    out = out.reshape(lead + given)
    return out.cpu().numpy() if as_numpy else out


def nlm_stack(stack, sigma, beta=1.0, search=3, patch=1, rician=False):
    """``nlm`` of a measurement-major ndarray stack [M, X, Y, Z] under the noise map ``sigma`` (that of ``mppca``), in groups of at most
    16 measurements in the stack's order, each group guided by its mean -- what ``scripts/denoise --method nlm`` and ``superresDWI
    --denoise nlm`` run."""
    step = ops._lib.INR_NLM_MAX_CHANNELS
    return np.concatenate([nlm(stack[i:i + step], sigma, beta, search, patch, guide="mean", rician=rician)
                           for i in range(0, stack.shape[0], step)], axis=0)


def _cell_rows(cell):
    """The ``[b][TE]`` cell (an object ndarray or nested sequences) as a list of lists of ndarrays."""
    if isinstance(cell, np.ndarray) and cell.dtype == object:
        if cell.ndim != 2:
            raise ValueError(f"the cell must be [b][TE] (got an object array of shape {cell.shape})")
        return [[np.asarray(cell[b, te]) for te in range(cell.shape[1])] for b in range(cell.shape[0])]
    return [[np.asarray(v) for v in row] for row in cell]


def stack_hybrid(cell):
    """The ``[b][TE]`` cell of a ``master.mat`` (b = 0: [X, Y, Z] or [X, Y, Z, 1]; b > 0: [X, Y, Z, K]) as ONE stack [M, X, Y, Z], every
    acquisition its own measurement, in the order (b, TE, acquisition).  The values are copied, never converted: the dtype is the
    cell's (mixed dtypes are refused), so ``unstack_hybrid(stack_hybrid(cell), cell)`` is the cell bit for bit."""
    rows = _cell_rows(cell)
    volumes, shape, dtype = [], None, None
    for b, row in enumerate(rows):
        for te, a in enumerate(row):
            if a.ndim not in (3, 4):
                raise ValueError(f"cell [{b}][{te}] must be [X, Y, Z] or [X, Y, Z, K] (got shape {a.shape})")
            shape = a.shape[:3] if shape is None else shape
            dtype = a.dtype if dtype is None else dtype
            if a.shape[:3] != shape or a.dtype != dtype:
                raise ValueError(f"cell [{b}][{te}] is {a.dtype} {a.shape[:3]}, the cells before it {dtype} {shape}")
            volumes.extend([a] if a.ndim == 3 else [a[..., k] for k in range(a.shape[3])])
    if not volumes:
        raise ValueError("the cell is empty")
    return np.stack(volumes, axis=0)


def unstack_hybrid(stack, like):
    """``stack`` [M, X, Y, Z] back in the layout of the cell ``like`` (the one ``stack_hybrid`` read): an object ndarray where ``like`` is
    one, else nested lists."""
    rows = _cell_rows(like)
    stack = np.asarray(stack)
    need = sum(1 if a.ndim == 3 else a.shape[3] for row in rows for a in row)
    if stack.ndim != 4 or stack.shape[0] != need:
        raise ValueError(f"the stack must be [M, X, Y, Z] with the M = {need} measurements of the cell (got shape {stack.shape})")
    out, at = [], 0
    for row in rows:
        new_row = []
        for a in row:
            k = 1 if a.ndim == 3 else a.shape[3]
            part = stack[at] if a.ndim == 3 else np.stack([stack[at + j] for j in range(k)], axis=-1)
            new_row.append(np.ascontiguousarray(part))
            at += k
        out.append(new_row)
    if isinstance(like, np.ndarray) and like.dtype == object:
        arr = np.empty(like.shape, dtype=object)
        for b, row in enumerate(out):
            for te, a in enumerate(row):
                arr[b, te] = a
        return arr
    return out
