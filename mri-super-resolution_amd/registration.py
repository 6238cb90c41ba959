"""The data preparation of the multi-image tree (multi-image-super-resolution/utils/preprocessing.py) on the device: masked
registration, the best ``T`` images of a set, patches and temporal augmentation.

``register_imgset`` (preprocessing.py:138-161) takes the image of a set with the clearest quality mask as the reference and, for every
image ``x`` with mask ``m``: ``s = masked_register_translation(ref, x, m)``, ``x <- shift(x, s, mode='reflect')``,
``m <- shift(m, s, mode='constant', cval=0)``.  The vendored copy is damaged in two places: it never imports
``masked_register_translation`` (the import at :15 is commented out, so the function raises ``NameError`` as shipped), and :161
returns ``imgset`` -- its input -- beside ``mask_reg``.  What is built here is what the body computes, and the registered images are
returned, as the function's own docstring says.

``masked_register_translation`` is scikit-image's name and argument order (Padfield 2012).  scikit-image is not installed in the build
image, so parity is pinned to the DEFINITION (``inr_masked_xcorr`` in include/inrhip.h; restated in float64 without FFTs by
tests/register_common.py) and, for ``shift``, to ``scipy.ndimage.shift`` 1.15; skimage itself is unpinned, and so is the choice among
equal maxima beyond their mean.  ``max_shift`` limits the search to ``|dy|, |dx| <= max_shift`` (the reference searches every overlap);
the correlation's ``max den`` and ``max n`` are then taken over that window.

The usual convention: ndarray in -> float64 ndarray out, device tensor in -> device tensor out with no host read on the way (the
correlation hands its shifts to the shift kernel on the device).  There is no CPU fallback (``ops.InrDeviceError``), and every
argument error is raised before any device work.  ``select_T_images`` draws ``np.random.choice`` and ``augment_*`` draw
``np.random.permutation`` in the reference's order: the same NumPy seed gives the same sets.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import check, lib

_SHIFT_MODES = {"reflect": 0, "constant": 1}      # INR_SHIFT_REFLECT, INR_SHIFT_CONSTANT (include/inrhip.h)
_XCORR_MAX_IMAGES = 65535
_XCORR_MAX_SIDE = 4096                            # INR_XCORR_MAX_SIDE
_XCORR_WS_DOUBLES = 1 << 27                       # sets beyond 1 GiB of correlation sums go through a further call


# ---- argument checks (host only) -----------------------------------------------------------------------------------------------------
def _is_tensor(a):
    return isinstance(a, torch.Tensor)


def _shape(a):
    return tuple(a.shape) if _is_tensor(a) else np.shape(a)


def _window(who, hw, max_shift):
    if max(hw) > _XCORR_MAX_SIDE:
        raise ValueError(f"{who}: images of at most {_XCORR_MAX_SIDE} x {_XCORR_MAX_SIDE} (got {hw[0]} x {hw[1]})")
    if max_shift is None:
        return hw[0] - 1, hw[1] - 1
    if isinstance(max_shift, bool) or int(max_shift) != max_shift or max_shift < 0:
        raise ValueError(f"{who}: max_shift must be None or a non-negative integer (got {max_shift!r})")
    return min(int(max_shift), hw[0] - 1), min(int(max_shift), hw[1] - 1)


def _check_overlap(who, overlap_ratio):
    if not 0.0 <= float(overlap_ratio) <= 1.0:
        raise ValueError(f"{who}: overlap_ratio must lie in [0, 1] (got {overlap_ratio!r})")


def _check_pair(who, image, mask, image_name="image", mask_name="mask", ndim=None):
    si, sm = _shape(image), _shape(mask)
    if ndim is not None and len(si) != ndim:
        raise ValueError(f"{who}: {image_name} must have {ndim} axes (got shape {si})")
    if si != sm:
        raise ValueError(f"{who}: {image_name} {si} and {mask_name} {sm} differ in shape")
    if min(si, default=0) < 1:
        raise ValueError(f"{who}: empty {image_name} {si}")


def _dev(a, name, dtype=torch.float32):
    """ndarray -> device tensor of ``dtype``; a tensor must already live on the device."""
    if _is_tensor(a):
        if not a.is_cuda:
            raise ops.InrDeviceError(f"{name} is on {a.device}: registration only runs on a HIP device (there is no CPU fallback)")
        return a.to(dtype).contiguous()
    dev = ops.require_gpu()
    return torch.from_numpy(np.ascontiguousarray(a, dtype={torch.float32: np.float32, torch.float64: np.float64}[dtype])).to(dev)


def _back(t, as_numpy):
    return t.cpu().numpy().astype(np.float64) if as_numpy else t


# ---- device calls ----------------------------------------------------------------------------------------------------------------------
def _image_means(planes):
    """planes [S, T, H, W] fp32 -> (means [S, T] float64, argmax [S] int32), both on the device."""
    S, T, H, W = planes.shape
    means = torch.empty((S, T), dtype=torch.float64, device=planes.device)
    best = torch.empty((S,), dtype=torch.int32, device=planes.device)
    check(lib().inr_image_means(means.data_ptr(), best.data_ptr(), planes.data_ptr(), S, T, H, W, ops._stream()), "inr_image_means")
    return means, best


def _xcorr(planes, masks, ref_index, window, overlap_ratio, want_map=False):
    """planes, masks [S, T, H, W] fp32, ref_index [S] int32 -> shifts [S, T, 2] float64, peak [S, T] float64, n_max [S, T] int32 and
    (``want_map``) the maps [S, T, 2 my + 1, 2 mx + 1] float64; sets go through as few calls as the workspace cap allows."""
    S, T, H, W = planes.shape
    my, mx = window
    dev = planes.device
    shifts = torch.empty((S, T, 2), dtype=torch.float64, device=dev)
    peak = torch.empty((S, T), dtype=torch.float64, device=dev)
    n_max = torch.empty((S, T), dtype=torch.int32, device=dev)
    cmap = torch.empty((S, T, 2 * my + 1, 2 * mx + 1), dtype=torch.float64, device=dev) if want_map else None
    if T > _XCORR_MAX_IMAGES:
        raise ValueError(f"registration: at most {_XCORR_MAX_IMAGES} images per set (got {T})")
    per_set = int(lib().inr_masked_xcorr_workspace_doubles(1, T, H, W, my, mx))
    if per_set <= 0:
        raise ValueError("registration: " + lib().inr_last_error().decode("utf-8", "replace"))
    step = max(1, min(_XCORR_MAX_IMAGES // T, _XCORR_WS_DOUBLES // per_set))
    ws = torch.empty(max(per_set * min(step, S), 2), dtype=torch.float64, device=dev)
    for s0 in range(0, S, step):
        n = min(step, S - s0)
        check(lib().inr_masked_xcorr(shifts[s0:].data_ptr(), peak[s0:].data_ptr(), n_max[s0:].data_ptr(),
                                     cmap[s0:].data_ptr() if want_map else 0, planes[s0:].data_ptr(), masks[s0:].data_ptr(),
                                     ref_index[s0:].data_ptr(), n, T, H, W, my, mx, float(overlap_ratio), ws.data_ptr(), ws.numel(),
                                     ops._stream()), "inr_masked_xcorr")
    return shifts, peak, n_max, cmap


def _shift_planes(planes, shifts, mode, cval):
    """planes [n, H, W] fp32, shifts [n, 2] float64, both on the device -> [n, H, W] fp32."""
    n, H, W = planes.shape
    out = torch.empty_like(planes)
    if n > 0:
        need = int(lib().inr_shift2d_workspace_doubles(n, H, W, _SHIFT_MODES[mode]))
        ws = torch.empty(max(need, 2), dtype=torch.float64, device=planes.device)
        check(lib().inr_shift2d(out.data_ptr(), planes.data_ptr(), shifts.data_ptr(), n, H, W, _SHIFT_MODES[mode], float(cval),
                                ws.data_ptr(), ws.numel(), ops._stream()), "inr_shift2d")
    return out


# ---- the correlation ---------------------------------------------------------------------------------------------------------------------
def _pair_call(who, src_image, target_image, src_mask, target_mask, overlap_ratio, max_shift, want_map):
    if target_mask is not None:
        raise ValueError(f"{who}: target_mask is not supported -- the reference never passes one (preprocessing.py:155), and "
                         "src_mask then serves both images, as in scikit-image")
    _check_pair(who, src_image, target_image, "src_image", "target_image", ndim=2)
    _check_pair(who, src_image, src_mask, "src_image", "src_mask")
    _check_overlap(who, overlap_ratio)
    window = _window(who, _shape(src_image), max_shift)
    as_numpy = not _is_tensor(src_image)
    src, tgt, m = _dev(src_image, "src_image"), _dev(target_image, "target_image"), _dev(src_mask, "src_mask")
    planes = torch.stack([src, tgt])[None]                                   # one set: the reference first
    masks = torch.stack([m, m])[None]
    ref = torch.zeros((1,), dtype=torch.int32, device=planes.device)
    shifts, _, _, cmap = _xcorr(planes, masks, ref, window, overlap_ratio, want_map)
    return shifts[0, 1], (cmap[0, 1] if want_map else None), as_numpy


def masked_register_translation(src_image, target_image, src_mask, target_mask=None, overlap_ratio=3 / 10, max_shift=None):
    """The translation ``s`` (rows, columns) that lays ``target_image`` on ``src_image`` -- ``shift(target_image, s)`` -- by masked
    normalised cross-correlation with ``src_mask`` on both images: the mean position of the maxima of ``masked_xcorr``.  [2] float64
    (ndarray in -> ndarray, device tensor in -> device tensor).  ``target_mask`` other than None raises."""
    s, _, as_numpy = _pair_call("masked_register_translation", src_image, target_image, src_mask, target_mask, overlap_ratio, max_shift,
                                False)
    return s.cpu().numpy() if as_numpy else s


def masked_xcorr(src_image, target_image, src_mask, target_mask=None, overlap_ratio=3 / 10, max_shift=None):
    """The correlation map ``C`` itself, float64 [2 my + 1, 2 mx + 1] with the displacement (0, 0) at its centre; ``my, mx`` are
    ``H - 1, W - 1`` or ``max_shift``, whichever is smaller."""
    _, cmap, as_numpy = _pair_call("masked_xcorr", src_image, target_image, src_mask, target_mask, overlap_ratio, max_shift, True)
    return cmap.cpu().numpy() if as_numpy else cmap


# ---- the shift --------------------------------------------------------------------------------------------------------------------------
def shift(image, shift, mode='reflect', cval=0.0, order=3):
    """``scipy.ndimage.shift(image, shift, order=3, mode=mode, cval=cval)`` on the trailing two axes of ``image``; leading axes are a
    batch.  ``shift`` is one (rows, columns) pair for all images or one pair per image ([..., 2], an ndarray or a device float64
    tensor).  Order 3 and the modes 'reflect' and 'constant' only."""
    if order != 3:
        raise ValueError(f"shift: only order 3 is implemented (got {order!r})")
    if mode not in _SHIFT_MODES:
        raise ValueError(f"shift: mode must be 'reflect' or 'constant' (got {mode!r})")
    if not np.isfinite(cval):
        raise ValueError(f"shift: cval must be finite (got {cval!r})")
    shape = _shape(image)
    if len(shape) < 2 or min(shape) < 1:
        raise ValueError(f"shift needs a non-empty input of at least 2 axes (got shape {shape})")
    n = int(np.prod(shape[:-2], dtype=np.int64))
    s_shape = _shape(shift)
    if s_shape != (2,) and (s_shape[-1:] != (2,) or int(np.prod(s_shape[:-1], dtype=np.int64)) != n):
        raise ValueError(f"shift: shift must be (rows, columns) or one pair per image (got shape {s_shape} for image {shape})")
    as_numpy = not _is_tensor(image)
    x = _dev(image, "image")
    s = _dev(shift, "shift", torch.float64).reshape(-1, 2)
    if s.shape[0] != n:
        s = s.expand(n, 2).contiguous()
    out = _shift_planes(x.reshape(n, shape[-2], shape[-1]), s, mode, cval).reshape(shape)
    return _back(out, as_numpy)


# ---- register_imgset / register_dataset ----------------------------------------------------------------------------------------------------
def _register_sets(X, M, window, overlap_ratio):
    """X, M [S, H, W, T] on the device (any float dtype) -> registered images, shifted masks [S, H, W, T] fp32, shifts [S, T, 2]."""
    planes = X.to(torch.float32).permute(0, 3, 1, 2).contiguous()
    masks = M.to(torch.float32).permute(0, 3, 1, 2).contiguous()
    S, T, H, W = planes.shape
    _, best = _image_means(masks)
    shifts, _, _, _ = _xcorr(planes, masks, best, window, overlap_ratio)
    flat = shifts.reshape(S * T, 2)
    reg = _shift_planes(planes.reshape(S * T, H, W), flat, "reflect", 0.0).reshape(S, T, H, W)
    reg_m = _shift_planes(masks.reshape(S * T, H, W), flat, "constant", 0.0).reshape(S, T, H, W)
    return reg.permute(0, 2, 3, 1).contiguous(), reg_m.permute(0, 2, 3, 1).contiguous(), shifts


def register_imgset(imgset, mask, max_shift=None, return_shifts=False, overlap_ratio=3 / 10):
    """preprocessing.py:138-161 for one set ``imgset`` [H, W, T] with quality masks ``mask`` [H, W, T]: every image is laid on the one
    with the largest ``mean(mask)`` (the first, among equals).  Returns ``(imgset_reg, mask_reg)`` -- the REGISTERED images, where
    the vendored copy returns its input -- and with ``return_shifts`` also the applied translations [T, 2] (float64)."""
    _check_pair("register_imgset", imgset, mask, "imgset", "mask", ndim=3)
    _check_overlap("register_imgset", overlap_ratio)
    window = _window("register_imgset", _shape(imgset)[:2], max_shift)
    as_numpy = not _is_tensor(imgset)
    reg, reg_m, shifts = _register_sets(_dev(imgset, "imgset")[None], _dev(mask, "mask")[None], window, overlap_ratio)
    out = (_back(reg[0], as_numpy), _back(reg_m[0], as_numpy))
    return out + ((shifts[0].cpu().numpy() if as_numpy else shifts[0]),) if return_shifts else out


def register_dataset(X, masks, max_shift=None, return_shifts=False, overlap_ratio=3 / 10):
    """preprocessing.py:115-134: ``register_imgset`` for every set of ``X`` (a list or array of [H, W, T_i]) -- the sets of one shape
    go through one call.  Returns the lists ``(X_reg, masks_reg)`` and with ``return_shifts`` the list of [T_i, 2] translations."""
    if len(X) != len(masks):
        raise ValueError(f"register_dataset: {len(X)} sets but {len(masks)} mask sets")
    groups = {}
    for i in range(len(X)):
        _check_pair(f"register_dataset: set {i}", X[i], masks[i], "imgset", "mask", ndim=3)
        _window("register_dataset", _shape(X[i])[:2], max_shift)
        groups.setdefault(_shape(X[i]), []).append(i)
    _check_overlap("register_dataset", overlap_ratio)
    X_reg, masks_reg, all_shifts = [None] * len(X), [None] * len(X), [None] * len(X)
    for shape, members in groups.items():
        as_numpy = [not _is_tensor(X[i]) for i in members]
        Xg = torch.stack([_dev(X[i], "X") for i in members])
        Mg = torch.stack([_dev(masks[i], "masks") for i in members])
        reg, reg_m, shifts = _register_sets(Xg, Mg, _window("register_dataset", shape[:2], max_shift), overlap_ratio)
        for k, i in enumerate(members):
            X_reg[i], masks_reg[i] = _back(reg[k], as_numpy[k]), _back(reg_m[k], as_numpy[k])
            all_shifts[i] = shifts[k].cpu().numpy() if as_numpy[k] else shifts[k]
    return (X_reg, masks_reg, all_shifts) if return_shifts else (X_reg, masks_reg)


# ---- select_T_images ---------------------------------------------------------------------------------------------------------------------
def select_indexes(clearance, T=9, thr=0.85, remove_bad=True):
    """The host half of preprocessing.py:186-214 for one set: from the clearances of its images the indexes of the ``T`` that are
    kept, in order -- those above ``thr`` by falling clearance, repeated by ``np.random.choice`` draws where fewer than ``T`` are
    clear -- or None where none is clear and ``remove_bad`` holds (without it the single best image is repeated)."""
    clearance = np.asarray(clearance, dtype=np.float64)
    clear = np.flatnonzero(clearance > thr)
    if not len(clear):
        if remove_bad:
            return None
        clear = np.array([int(np.argmax(clearance))])
    order = list(np.argsort(clearance[clear])[::-1])
    order += [np.random.choice(order) for _ in range(T - len(clear))]
    return [int(clear[j]) for j in order[:T]]


def clearances(masks):
    """``mean(mask, axis=(0, 1))`` of every set of ``masks`` (a list or array of [H, W, T_i]) on the device: a list of float64
    ndarrays [T_i].  The sets of one shape go through one call."""
    groups = {}
    for i in range(len(masks)):
        if len(_shape(masks[i])) != 3 or min(_shape(masks[i])) < 1:
            raise ValueError(f"clearances: set {i} must be a non-empty [H, W, T] (got shape {_shape(masks[i])})")
        groups.setdefault(_shape(masks[i]), []).append(i)
    out = [None] * len(masks)
    for members in groups.values():
        planes = torch.stack([_dev(masks[i], "masks") for i in members]).permute(0, 3, 1, 2).contiguous()
        means = _image_means(planes)[0].cpu().numpy()
        for k, i in enumerate(members):
            out[i] = means[k]
    return out


def select_T_images(X, masks, T=9, thr=0.85, remove_bad=True):
    """preprocessing.py:165-216: the ``T`` clearest images of every set, ``(X_selected [B', H, W, T], remove_indexes)`` as the
    reference returns them.  The clearances are computed on the device, the selection is ``select_indexes``; the images are indexed,
    not converted (an ndarray keeps its dtype; device tensors give a stacked device tensor)."""
    if isinstance(T, bool) or int(T) != T or T < 1:
        raise ValueError(f"select_T_images: T must be a positive integer (got {T!r})")
    if not 0.0 <= float(thr) <= 1.0:
        raise ValueError(f"select_T_images: thr is a share of clear pixels in [0, 1] (got {thr!r})")
    if len(X) != len(masks):
        raise ValueError(f"select_T_images: {len(X)} sets but {len(masks)} mask sets")
    for i in range(len(X)):
        _check_pair(f"select_T_images: set {i}", X[i], masks[i], "imgset", "mask", ndim=3)
    clear = clearances(masks)
    selected, removed = [], []
    for i in range(len(X)):
        idx = select_indexes(clear[i], int(T), thr, remove_bad)
        if idx is None:
            print("Removing number", i)
            removed.append(i)
            continue
        selected.append(X[i][..., torch.as_tensor(idx, device=X[i].device)] if _is_tensor(X[i]) else np.asarray(X[i])[..., idx])
    if selected and _is_tensor(selected[0]):
        return torch.stack(selected), removed
    return np.array(selected), removed


# ---- patches -----------------------------------------------------------------------------------------------------------------------------
def patch_count(d_o, d, s):
    """``n = (d_o - d) / s + 1`` of preprocessing.py:255-258, with its ValueError where that is no integer."""
    d, s = int(d), int(s)
    if d < 1 or s < 1 or d > d_o:
        raise ValueError(f"d, s and n should be integer values (d={d}, s={s} on a side of {d_o}).")
    n = (d_o - d) / s + 1
    if int(n) != n:
        raise ValueError("d, s and n should be integer values.")
    return int(n)


def _patches(t, d, s, n):
    """t [l, H, W, ch] on the device -> [l n^2, d, d, ch], patch n i + j of an item at rows i s, columns j s."""
    if t.shape[2] < (n - 1) * s + d:
        raise ValueError(f"gen_sub: {n} patches of {d} at stride {s} do not fit {t.shape[2]} columns")
    w = t.unfold(1, d, s)[:, :n].unfold(2, d, s)[:, :, :n]                  # [l, n, n, ch, d, d]
    return w.permute(0, 1, 2, 4, 5, 3).reshape(t.shape[0] * n * n, d, d, t.shape[3]).contiguous()


def _index_in(a, name):
    """What the indexing functions run on: an ndarray travels as float64 (exactly), a device tensor as it is."""
    return _dev(a, name, torch.float64) if not _is_tensor(a) else _dev(a, name, a.dtype)


def sub_images(X, d, s, n):
    """preprocessing.py:218-230: the ``n^2`` patches [d, d, ch] of one item ``X`` [H, W, ch], rows first."""
    if len(_shape(X)) != 3:
        raise ValueError("Wrong array shape.")
    d, s, n = int(d), int(s), int(n)
    if min(d, s, n) < 1 or (n - 1) * s + d > _shape(X)[0]:
        raise ValueError(f"sub_images: {n} patches of {d} at stride {s} do not fit {_shape(X)[0]} rows")
    out = _patches(_index_in(X, "X")[None], d, s, n)
    return out if _is_tensor(X) else out.cpu().numpy()


def gen_sub(array, d, s, verbose=True):
    """preprocessing.py:232-269: all patches of ``array`` [B, H, W, ch] -> [B n^2, d, d, ch] in the reference's order (item, row,
    column), with its ``ValueError``s.  Indexing on the device, no arithmetic."""
    if len(_shape(array)) != 4:
        raise ValueError("Wrong array shape.")
    d, s = int(d), int(s)
    n = patch_count(_shape(array)[1], d, s)
    out = _patches(_index_in(array, "array"), d, s, n)
    if verbose:
        print(tuple(out.shape))
    return out if _is_tensor(array) else out.cpu().numpy()


# ---- temporal augmentation -----------------------------------------------------------------------------------------------------------------
def augment_permutations(T, n_augment):
    """[n_augment, T] channel indexes of preprocessing.py:104-111: the identity, then ``n_augment - 1`` ``np.random.permutation(T)``."""
    return np.stack([np.arange(T)] + [np.random.permutation(T) for _ in range(n_augment - 1)])


def _check_augment(who, n_augment):
    if isinstance(n_augment, bool) or int(n_augment) != n_augment or n_augment < 1:
        raise ValueError(f"{who}: n_augment must be a positive integer (got {n_augment!r})")
    return int(n_augment)


def _repeat(a, n):
    """np.array([a] * n) for an ndarray, the same for a device tensor."""
    return a[None].expand(n, *a.shape).contiguous() if _is_tensor(a) else np.array([np.asarray(a)] * n)


def augment_imgset(X_imgset, y_imgset, y_mask_imgset, n_augment):
    """preprocessing.py:89-111: ``X_imgset`` [H, W, T] with its channels permuted ``n_augment - 1`` times behind the original
    ([n_augment, H, W, T]), and the label and its mask repeated."""
    n_augment = _check_augment("augment_imgset", n_augment)
    if len(_shape(X_imgset)) != 3:
        raise ValueError(f"augment_imgset: X_imgset must be [H, W, T] (got shape {_shape(X_imgset)})")
    x = _index_in(X_imgset, "X_imgset")
    perms = torch.from_numpy(augment_permutations(x.shape[-1], n_augment)).to(x.device)
    out = x[..., perms].permute(2, 0, 1, 3).contiguous()                      # [H, W, n, T] -> [n, H, W, T]
    return (out if _is_tensor(X_imgset) else out.cpu().numpy()), _repeat(y_imgset, n_augment), _repeat(y_mask_imgset, n_augment)


def augment_dataset(X, y, y_masks, n_augment=7):
    """preprocessing.py:62-85: ``augment_imgset`` for every item of ``X`` [B, H, W, T], item by item ([B n_augment, ...] each; an
    ndarray gives float64, as the reference's ``np.empty`` does)."""
    n_augment = _check_augment("augment_dataset", n_augment)
    if len(_shape(X)) != 4 or len(y) != len(X) or len(y_masks) != len(X):
        raise ValueError(f"augment_dataset: X must be [B, H, W, T] with one label and one mask per item (got X {_shape(X)}, "
                         f"{len(y)} labels, {len(y_masks)} masks)")
    x = _index_in(X, "X")
    B, T = x.shape[0], x.shape[-1]
    perms = torch.from_numpy(np.stack([augment_permutations(T, n_augment) for _ in range(B)])).to(x.device)     # [B, n, T]
    idx = perms[:, :, None, None, :].expand(B, n_augment, x.shape[1], x.shape[2], T)
    out = torch.gather(x[:, None].expand(B, n_augment, *x.shape[1:]), 4, idx).reshape(B * n_augment, *x.shape[1:])

    def rep(a):
        if _is_tensor(a):
            return a[:, None].expand(a.shape[0], n_augment, *a.shape[1:]).reshape(a.shape[0] * n_augment, *a.shape[1:]).contiguous()
        return np.repeat(np.asarray(a, dtype=np.float64), n_augment, axis=0)
    return (out if _is_tensor(X) else out.cpu().numpy()), rep(y), rep(y_masks)
