"""Host plumbing every fitter shares: the flat parameter buffer a module's parameters are views of, the two kinds of
workspace buffer, and the Adam state beside the flat buffer.  Only torch is used here -- no library call, no device
requirement -- so everything in this module also runs on CPU tensors.
"""
from __future__ import annotations

import torch


def _bytes(need, device):
    return torch.empty(need, dtype=torch.uint8, device=device)


def _view(vector, off, like):
    """The slice of the float ``vector`` at ``off`` in the shape of ``like``.  A complex tensor is its interleaved (re, im)
    float pairs -- torch's own layout -- seen through ``view_as_complex`` (``off`` must then be even)."""
    if like.is_complex():
        return torch.view_as_complex(vector[off:off + 2 * like.numel()].view(*like.shape, 2))
    return vector[off:off + like.numel()].view_as(like)


class FlatParams:
    """One flat fp32 buffer of ``total`` floats holding tensor k at ``offsets[k]``, in the order in which the caller hands
    its parameters over.  ``adopt`` re-points the parameters at views of the buffer, so the module, an external optimizer
    and the kernels all see the same live weights."""

    def __init__(self, total, offsets):
        self.total, self.offsets = int(total), [int(o) for o in offsets]
        self.flat = None
        self._views = []

    def _carve(self, vector, like):
        if len(like) != len(self.offsets):
            raise ValueError(f"{len(like)} tensors for a layout of {len(self.offsets)}")
        return [_view(vector, off, t) for off, t in zip(self.offsets, like)]

    def adopt(self, params, zero=True):
        """Build the buffer on ``params[0].device``, copy every parameter in and re-point its ``.data`` at its view.
        ``zero`` clears the buffer first: a layout that pads its tensors needs the padding to be zero (and to stay zero under
        Adam, whose ``grads`` / ``m`` / ``v`` are ``zeros_like`` this buffer)."""
        flat = (torch.zeros if zero else torch.empty)(self.total, dtype=torch.float32, device=params[0].device)
        views = self._carve(flat, params)
        for p, view in zip(params, views):
            view.copy_(p.detach())
            p.data = view
        self.flat, self._views = flat, views
        return flat

    def owns(self, params):
        """Are these parameters still the views of ``flat``?  (One pass of ``data_ptr()`` comparisons: a module that was moved
        or reloaded has new storage.)"""
        return self.flat is not None and len(params) == len(self._views) and self.flat.device == params[0].device and \
            all(p.data_ptr() == v.data_ptr() for p, v in zip(params, self._views))

    def ensure(self, params, zero=True):
        """Adopt again if the parameters are no longer views of ``flat``; says whether it did."""
        if self.owns(params):
            return False
        self.adopt(params, zero)
        return True

    def split(self, vector):
        """Per-tensor views of any vector of ``total`` floats, in the adopted shapes."""
        return self._carve(vector, self._views)

    def pack(self, params):
        """A fresh packed copy of ``params`` (padding zero); nothing is re-pointed."""
        flat = torch.zeros(self.total, dtype=torch.float32, device=params[0].device)
        for p, view in zip(params, self._carve(flat, params)):
            view.copy_(p.detach())
        return flat


class WorkspacePool:
    """The stash workspace of a pending forward: ``take`` hands the free buffer out (or a new one), the backward gives it
    back.  A forward whose backward never runs simply keeps its buffer, and the next ``take`` allocates."""

    def __init__(self):
        self._free = None            # a workspace no pending forward owns

    def take(self, need, device):
        """(workspace of at least ``need`` bytes on ``device``, whether it had to be allocated)."""
        ws, self._free = self._free, None
        if ws is not None and ws.numel() >= need and ws.device == device:
            return ws, False
        return _bytes(need, device), True

    def give_back(self, ws):
        if self._free is None or ws.numel() >= self._free.numel():
            self._free = ws


class Workspace:
    """A grow-only workspace one owner keeps between its calls."""

    def __init__(self):
        self.buf = None

    def grow(self, need, device):
        if self.buf is None or self.buf.numel() < need:
            self.buf = None          # the old buffer is freed BEFORE the new one is requested: the two never coexist
            self.buf = _bytes(need, device)
        return self.buf

    def release(self):
        self.buf = None


class AdamState:
    """``grads`` / ``m`` / ``v`` like the flat parameter buffer, and the number of steps taken."""

    def __init__(self, flat):
        self._numel, self._device = flat.numel(), flat.device      # (not `flat` itself: a re-adoption replaces that)
        self.reset()

    def reset(self):
        """A fresh optimizer: zeroed moments and gradient, step 0."""
        self.grads, self.m, self.v = (torch.zeros(self._numel, dtype=torch.float32, device=self._device) for _ in range(3))
        self.step_count = 0


def _adam_attr(name):
    return property(lambda self: getattr(self.adam, name), lambda self, value: setattr(self.adam, name, value))


class AdamOwner:
    """Mixin of the fitters: ``self.adam`` (an ``AdamState``) read and written under the attribute names their callers use."""
    grads, m, v, step_count = (_adam_attr(name) for name in ("grads", "m", "v", "step_count"))
