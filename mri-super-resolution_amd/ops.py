"""torch-tensor wrappers over the C ABI (include/inrhip.h).

PyTorch is used here only for device memory (allocation of outputs/workspaces) and for the
current HIP stream.  Every wrapper validates device, dtype, contiguity and shapes on the host
BEFORE a kernel is enqueued, and raises instead of falling back: tensors must live on a HIP
device and libinrhip.so must be loadable.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import SirenDesc, check, lib, shape_array


class InrDeviceError(RuntimeError):
    """Raised when an op is asked to run without a HIP device (there is no CPU path)."""


def require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise InrDeviceError("mri-super-resolution_amd needs a HIP GPU (MI355X / gfx950); "
                             "no CPU fallback exists for the INR kernels.")
    lib()
    return torch.device("cuda", torch.cuda.current_device())


def _chk(t: torch.Tensor, name: str, shape=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise InrDeviceError(f"{name} is on {t.device}: the INR kernels only run on a HIP device "
                             "(move it with .cuda(); there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _nbytes(t) -> int:
    return t.numel() * t.element_size()


def _workspace(workspace, need, device, name="workspace", flags=None):
    """The caller's workspace, or a new one where none came.  One that is too small is an error -- except with ``flags``
    (an int: the REUSE_* entry points), where it is replaced like a missing one, which a REUSE flag forbids: the flag speaks
    of what the previous call left in its workspace."""
    if workspace is not None and _nbytes(workspace) >= need:
        return workspace
    if workspace is not None and flags is None:
        raise ValueError(f"{name} too small")
    if flags:
        raise ValueError("REUSE_* flags need the workspace of the previous call")
    return _ws(need, device)


def _rows(x, in_features, name="x") -> int:
    """``x`` is a device tensor [n, in_features]; returns n."""
    _chk(x, name)
    if x.dim() != 2 or x.shape[1] != in_features:
        raise ValueError(f"{name} {tuple(x.shape)} must be [n,{in_features}]")
    return x.shape[0]


def _chk_losses(losses, n_steps, name="losses"):
    if losses is not None:
        _chk(losses, name)
        if losses.numel() < n_steps:
            raise ValueError(f"{name} buffer shorter than n_steps")


def _layer_dims(x, W, b, xname="x"):
    """(n, fin, fout) of ``x`` [n, fin], ``W`` [fout, fin] and the optional bias [fout]."""
    _chk(x, xname)
    _chk(W, "weight")
    if x.dim() != 2 or W.dim() != 2 or x.shape[1] != W.shape[1]:
        raise ValueError(f"{xname} {tuple(x.shape)} / weight {tuple(W.shape)} mismatch")
    if b is not None:
        _chk(b, "bias", (W.shape[0],))
    return x.shape[0], x.shape[1], W.shape[0]


def _grid_rows(shape, row_begin: int = 0, n_rows=None):
    """(shape as ints, its row count, the length of the row window from ``row_begin`` -- by default to the end)."""
    shape = tuple(int(s) for s in shape)
    total = 1
    for s in shape:
        total *= s
    n_rows = total - row_begin if n_rows is None else int(n_rows)
    if row_begin < 0 or n_rows < 0 or row_begin + n_rows > total:
        raise ValueError("row range outside the grid")
    return shape, total, n_rows


def param_layout(count_fn, offsets_fn, desc, n_entries: int):
    """Ask the library for a flat parameter layout: ``count_fn(desc)`` gives the total in floats (negative: refused),
    ``offsets_fn(desc, offsets, n_entries)`` fills the ``n_entries`` float offsets and returns a status.  Returns
    ``(total, [offsets])``; a refusal raises ``InrHipError``."""
    total = count_fn(C.byref(desc))
    if total < 0:
        check(int(total), getattr(count_fn, "__name__", "param count"))
    offs = (C.c_int64 * n_entries)()
    check(offsets_fn(C.byref(desc), offs, n_entries), getattr(offsets_fn, "__name__", "param offsets"))
    return int(total), [int(o) for o in offs]


def make_desc(in_features, hidden_features, hidden_layers, out_features, first_omega=30.0, hidden_omega=30.0):
    return SirenDesc(int(in_features), int(hidden_features), int(hidden_layers), int(out_features),
                     float(first_omega), float(hidden_omega))


def device_caps(device: int = 0) -> dict:
    caps = _lib.DeviceCaps()
    check(lib().inr_device_caps(int(device), C.byref(caps)), "inr_device_caps")
    return {f: (getattr(caps, f).decode() if f == "arch" else getattr(caps, f)) for f, _ in caps._fields_}


# ---- a-1 / a-3 ------------------------------------------------------------------------------------
def mgrid(shape, row_begin: int = 0, n_rows: int | None = None) -> torch.Tensor:
    dev = require_gpu()
    shape, _, n_rows = _grid_rows(shape, row_begin, n_rows)
    out = torch.empty((n_rows, len(shape)), dtype=torch.float32, device=dev)
    if n_rows == 0:
        return out
    check(lib().inr_mgrid(out.data_ptr(), shape_array(shape), len(shape), row_begin, n_rows, _stream()), "inr_mgrid")
    return out


def fourier_map(x: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    _chk(x, "x")
    _chk(B, "B")
    if x.dim() != 2 or B.dim() != 2 or x.shape[1] != B.shape[1]:
        raise ValueError(f"x {tuple(x.shape)} and B {tuple(B.shape)} must be [n,d] and [m,d]")
    n, d = x.shape
    m = B.shape[0]
    out = torch.empty((n, 2 * m), dtype=torch.float32, device=x.device)
    if n == 0:
        return out
    check(lib().inr_fourier_map(out.data_ptr(), x.data_ptr(), B.data_ptr(), n, d, m, _stream()), "inr_fourier_map")
    return out


def grid_fourier_map(shape, B: torch.Tensor, row_begin: int = 0, n_rows: int | None = None) -> torch.Tensor:
    _chk(B, "B")
    shape = tuple(int(s) for s in shape)
    if B.dim() != 2 or B.shape[1] != len(shape):
        raise ValueError(f"B {tuple(B.shape)} must be [m,{len(shape)}]")
    _, _, n_rows = _grid_rows(shape, row_begin, n_rows)
    m = B.shape[0]
    out = torch.empty((n_rows, 2 * m), dtype=torch.float32, device=B.device)
    if n_rows == 0:
        return out
    check(lib().inr_grid_fourier_map(out.data_ptr(), shape_array(shape), len(shape), row_begin, n_rows,
                                     B.data_ptr(), m, _stream()), "inr_grid_fourier_map")
    return out


# ---- per-layer pieces (autograd path) -------------------------------------------------------------------
def sine_layer_forward(x, W, b, omega: float, stash: bool):
    n, fin, fout = _layer_dims(x, W, b)
    act = torch.empty((n, fout), dtype=torch.float32, device=x.device)
    dact = torch.empty_like(act) if stash else None
    if n == 0:      # nothing to launch (an empty tensor has no address to pass)
        return act, dact
    check(lib().inr_sine_layer_forward(act.data_ptr(), _ptr(dact), x.data_ptr(), W.data_ptr(), _ptr(b), n, fin, fout,
                                       float(omega), _stream()), "inr_sine_layer_forward")
    return act, dact


def tanh_layer_forward(x, W, b, scale: float, stash: bool):
    """act = scale*tanh(x W^T + b) and (if ``stash``) its derivative factor scale*(1-tanh^2)."""
    n, fin, fout = _layer_dims(x, W, b)
    act = torch.empty((n, fout), dtype=torch.float32, device=x.device)
    dact = torch.empty_like(act) if stash else None
    if n == 0:      # nothing to launch (an empty tensor has no address to pass)
        return act, dact
    check(lib().inr_tanh_layer_forward(act.data_ptr(), _ptr(dact), x.data_ptr(), W.data_ptr(), _ptr(b), n, fin, fout,
                                       float(scale), _stream()), "inr_tanh_layer_forward")
    return act, dact


def linear_tanh_head_forward(a, W, b, scale: float, stash: bool):
    """y = scale*tanh(a W^T + b) for a few output columns, and (if ``stash``) scale*(1-tanh^2)."""
    n, hidden, out_f = _layer_dims(a, W, b, "a")
    y = torch.empty((n, out_f), dtype=torch.float32, device=a.device)
    dy = torch.empty_like(y) if stash else None
    check(lib().inr_linear_tanh_head_forward(y.data_ptr(), _ptr(dy), a.data_ptr(), W.data_ptr(), _ptr(b), n, hidden,
                                             out_f, float(scale), _stream()), "inr_linear_tanh_head_forward")
    return y, dy


def mul(a, b):
    _chk(a, "a")
    _chk(b, "b", a.shape)
    out = torch.empty_like(a)
    check(lib().inr_mul(out.data_ptr(), a.data_ptr(), b.data_ptr(), a.numel(), _stream()), "inr_mul")
    return out


def acquisition_products(raw_b0, raw_b1, raw_b2, raw_b3):
    """All combinations of one acquisition per b-value at every voxel (SRDWI.py:143-152 over superresDWI.py:57-76):
    raw_b0 [...], raw_bk [..., nk] device fp32 -> [..., 4, n1*n2*n3] in itertools.product order."""
    for name, t in (("raw_b0", raw_b0), ("raw_b1", raw_b1), ("raw_b2", raw_b2), ("raw_b3", raw_b3)):
        _chk(t, name)
    lead = tuple(raw_b0.shape)
    if any(tuple(t.shape[:-1]) != lead for t in (raw_b1, raw_b2, raw_b3)):
        raise ValueError("acquisition_products: leading (voxel) shapes differ")
    n1, n2, n3 = raw_b1.shape[-1], raw_b2.shape[-1], raw_b3.shape[-1]
    out = torch.empty(lead + (4, n1 * n2 * n3), dtype=torch.float32, device=raw_b0.device)
    check(lib().inr_acquisition_products(out.data_ptr(), raw_b0.data_ptr(), raw_b1.data_ptr(), raw_b2.data_ptr(),
                                         raw_b3.data_ptr(), raw_b0.numel(), n1, n2, n3, _stream()), "inr_acquisition_products")
    return out


def linear_head_forward(a, W, b, clamp_min=None):
    n, hidden, out_f = _layer_dims(a, W, b, "a")
    y = torch.empty((n, out_f), dtype=torch.float32, device=a.device)
    check(lib().inr_linear_head_forward(y.data_ptr(), a.data_ptr(), W.data_ptr(), _ptr(b), n, hidden, out_f,
                                        0 if clamp_min is None else 1, float(clamp_min or 0.0), _stream()),
          "inr_linear_head_forward")
    return y


def mse_loss_grad(y, t, w=None):
    """Returns (loss[1] device tensor, gy like y)."""
    _chk(y, "y")
    _chk(t, "target", y.shape)
    if w is not None:
        _chk(w, "weight", y.shape)
    count = y.numel()
    gy = torch.empty_like(y)
    loss = torch.empty((1,), dtype=torch.float32, device=y.device)
    nbytes = lib().inr_mse_workspace_bytes(count)
    ws = _ws(nbytes, y.device)
    check(lib().inr_mse_loss_grad(gy.data_ptr(), loss.data_ptr(), y.data_ptr(), t.data_ptr(), _ptr(w), count,
                                  ws.data_ptr(), ws.numel(), _stream()), "inr_mse_loss_grad")
    return loss, gy


def linear_head_backward(gy, a_last, dact_last, W, need_dz=True, need_param=True, need_bias_last=False):
    """dz_last = (gy W) * dact_last (plain product when dact_last is None); gW, gb of the head; with
    ``need_bias_last`` also colsum(dz_last), the bias gradient of the last sine layer."""
    _chk(gy, "gy")
    _chk(a_last, "a_last")
    _chk(W, "weight")
    n, hidden = a_last.shape
    out_f = W.shape[0]
    if tuple(gy.shape) != (n, out_f) or tuple(W.shape) != (out_f, hidden):
        raise ValueError("head backward shape mismatch")
    if dact_last is not None:
        _chk(dact_last, "dact_last", (n, hidden))
    dz = torch.empty((n, hidden), dtype=torch.float32, device=gy.device) if need_dz else None
    gW = torch.empty_like(W) if need_param else None
    gb = torch.empty((out_f,), dtype=torch.float32, device=gy.device) if need_param else None
    gb_last = torch.empty((hidden,), dtype=torch.float32, device=gy.device) if (need_bias_last and need_dz) else None
    nbytes = lib().inr_head_backward_workspace_bytes(n, hidden, out_f)
    ws = _ws(nbytes, gy.device)
    check(lib().inr_linear_head_backward(_ptr(dz), _ptr(gW), _ptr(gb), _ptr(gb_last), gy.data_ptr(), a_last.data_ptr(),
                                         _ptr(dact_last), W.data_ptr(), n, hidden, out_f, ws.data_ptr(), ws.numel(),
                                         _stream()), "inr_linear_head_backward")
    return dz, gW, gb, gb_last


def sine_layer_backward_input(dz, W, dact_prev, out=None, need_bias=False):
    """(dz @ W) * dact_prev  ->  [n, in]; `out` may alias dact_prev (in place).  With ``need_bias`` also returns
    colsum of the result (bias gradient of the layer below) from the fused epilogue."""
    _chk(dz, "dz")
    _chk(W, "weight")
    n, fout = dz.shape
    if W.shape[0] != fout:
        raise ValueError("dz / weight mismatch")
    fin = W.shape[1]
    if dact_prev is not None:
        _chk(dact_prev, "dact_prev", (n, fin))
    if out is None:
        out = torch.empty((n, fin), dtype=torch.float32, device=dz.device)
    else:
        _chk(out, "out", (n, fin))
    gb = ws = None
    ws_ptr, ws_bytes = 0, 0
    if need_bias:
        gb = torch.empty((fin,), dtype=torch.float32, device=dz.device)
        ws = _ws(lib().inr_sine_layer_backward_input_workspace_bytes(n, fin), dz.device)
        ws_ptr, ws_bytes = ws.data_ptr(), ws.numel()
    if n == 0:      # nothing to launch: an empty result, and the sum over no rows
        return (out, gb.zero_()) if need_bias else out
    check(lib().inr_sine_layer_backward_input(out.data_ptr(), _ptr(gb), dz.data_ptr(), W.data_ptr(), _ptr(dact_prev), n,
                                              fin, fout, ws_ptr, ws_bytes, _stream()),
          "inr_sine_layer_backward_input")
    return (out, gb) if need_bias else out


def linear_param_grad(dz, x, need_bias=True):
    _chk(dz, "dz")
    _chk(x, "x")
    n, fout = dz.shape
    if x.shape[0] != n:
        raise ValueError("dz / x row mismatch")
    fin = x.shape[1]
    gW = torch.empty((fout, fin), dtype=torch.float32, device=dz.device)
    gb = torch.empty((fout,), dtype=torch.float32, device=dz.device) if need_bias else None
    nbytes = lib().inr_linear_param_grad_workspace_bytes(n, fin, fout)
    ws = _ws(nbytes, dz.device)
    check(lib().inr_linear_param_grad(gW.data_ptr(), _ptr(gb), dz.data_ptr(), x.data_ptr(), n, fin, fout,
                                      ws.data_ptr(), ws.numel(), _stream()), "inr_linear_param_grad")
    return gW, gb


def adam_step(p, g, m, v, step: int, lr: float, beta1=0.9, beta2=0.999, eps=1e-8):
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _chk(t, name)
        if t.numel() != p.numel():
            raise ValueError("adam tensors must have equal numel")
    check(lib().inr_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), int(step),
                              float(lr), float(beta1), float(beta2), float(eps), _stream()), "inr_adam_step")


# ---- fused SIREN -----------------------------------------------------------------------------------------
def siren_param_layout(desc: SirenDesc):
    """(total_floats, [(w_off, b_off)] per layer in network order, head last)."""
    total, offs = param_layout(lib().inr_siren_param_count, lambda d, o, n: lib().inr_siren_param_offsets(d, o), desc,
                               2 * (desc.hidden_layers + 2))
    return total, list(zip(offs[0::2], offs[1::2]))


def _chk_flat(desc: SirenDesc, **tensors):
    """Every named tensor is a device fp32 vector of the layout's total."""
    total, _ = siren_param_layout(desc)
    for name, t in tensors.items():
        _chk(t, name)
        if t.numel() != total:
            raise ValueError(f"{name} has {t.numel()} floats, layout needs {total}")


def siren_forward(desc: SirenDesc, params, x, clamp_min=None):
    _chk_flat(desc, params=params)
    n = _rows(x, desc.in_features)
    y = torch.empty((n, desc.out_features), dtype=torch.float32, device=x.device)
    nbytes = lib().inr_siren_forward_workspace_bytes(C.byref(desc), n)
    ws = _ws(nbytes, x.device)
    check(lib().inr_siren_forward(C.byref(desc), params.data_ptr(), x.data_ptr(), n, y.data_ptr(),
                                  0 if clamp_min is None else 1, float(clamp_min or 0.0), ws.data_ptr(), ws.numel(),
                                  _stream()), "inr_siren_forward")
    return y


def siren_reconstruct(desc: SirenDesc, params, shape, B=None, clamp_min=0.0, chunk_rows: int = 1 << 20):
    _chk_flat(desc, params=params)
    shape, total_rows, _ = _grid_rows(shape)
    m = 0
    if B is not None:
        _chk(B, "B")
        if B.dim() != 2 or B.shape[1] != len(shape) or 2 * B.shape[0] != desc.in_features:
            raise ValueError(f"B {tuple(B.shape)} must be [{desc.in_features // 2},{len(shape)}]")
        m = B.shape[0]
    elif len(shape) != desc.in_features:
        raise ValueError("without B the grid dimension must equal in_features")
    chunk_rows = max(1, min(int(chunk_rows), total_rows))
    y = torch.empty((total_rows, desc.out_features), dtype=torch.float32, device=params.device)
    nbytes = lib().inr_siren_reconstruct_workspace_bytes(C.byref(desc), chunk_rows)
    ws = _ws(nbytes, params.device)
    check(lib().inr_siren_reconstruct(C.byref(desc), params.data_ptr(), shape_array(shape), len(shape), _ptr(B), m,
                                      y.data_ptr(), 0 if clamp_min is None else 1, float(clamp_min or 0.0),
                                      chunk_rows, ws.data_ptr(), ws.numel(), _stream()), "inr_siren_reconstruct")
    return y


def _derivative_maps(planner, rows_fn, grid_fn, ws_dtype, desc, params, x, shape, B, d_tangent, want_grad, want_lap,
                     chunk_rows):
    """What ``siren_jet`` and ``wire_derivatives`` share once ``params`` has been checked: ``x`` or ``shape``, ``B``, the outputs,
    a workspace of ``planner``'s count of ``ws_dtype`` elements, and the rows (``rows_fn``) or grid (``grid_fn``) entry point."""
    if x is not None:
        _chk(x, "x")
        if x.dim() != 2:
            raise ValueError(f"x {tuple(x.shape)} must be [n, d]")
        n, d = int(x.shape[0]), int(x.shape[1])
    else:
        shape, n, _ = _grid_rows(shape)
        d = len(shape)
    m = 0
    if B is not None:
        _chk(B, "B")
        if B.dim() != 2 or B.shape[1] != d:
            raise ValueError(f"B {tuple(B.shape)} must be [m, {d}]")
        m = int(B.shape[0])
    dt = d if d_tangent is None else int(d_tangent)
    chunk_rows = max(1, min(int(chunk_rows), max(n, 1)))
    dev = params.device
    y = torch.empty(n, dtype=torch.float32, device=dev)
    grad = torch.empty((n, dt), dtype=torch.float32, device=dev) if want_grad else None
    lap = torch.empty(n, dtype=torch.float32, device=dev) if want_lap else None
    count = int(getattr(lib(), planner)(C.byref(desc), d, m, chunk_rows, 1 if want_lap else 0))
    ws = torch.empty(max(count, 16), dtype=ws_dtype, device=dev)      # (0 for a shape the kernels refuse: the call below says which)
    if x is not None:
        check(getattr(lib(), rows_fn)(C.byref(desc), params.data_ptr(), x.data_ptr(), n, d, dt, _ptr(B), m, y.data_ptr(), _ptr(grad),
                                      _ptr(lap), chunk_rows, ws.data_ptr(), ws.numel(), _stream()), rows_fn)
    else:
        check(getattr(lib(), grid_fn)(C.byref(desc), params.data_ptr(), shape_array(shape), d, dt, _ptr(B), m, y.data_ptr(),
                                      _ptr(grad), _ptr(lap), chunk_rows, ws.data_ptr(), ws.numel(), _stream()), grid_fn)
    return y, grad, lap


def siren_jet(desc: SirenDesc, params, x=None, shape=None, B=None, d_tangent=None, want_grad=True, want_lap=True,
              chunk_rows: int = 1 << 15):
    """Value, coordinate gradient and Laplacian of a SIREN in forward mode (``inr_siren_jet`` on the rows ``x`` [n, d], or
    ``inr_siren_jet_grid`` on ``get_mgrid(shape)``; exactly one of the two).  Returns ``(y [n], grad [n, d_tangent] or None,
    lap [n] or None)``; derivatives are taken along the ``d_tangent`` leading axes (default: all ``d``)."""
    if (x is None) == (shape is None):
        raise ValueError("siren_jet takes exactly one of x and shape")
    _chk_flat(desc, params=params)
    return _derivative_maps("inr_siren_jet_workspace_bytes", "inr_siren_jet", "inr_siren_jet_grid", torch.uint8, desc,
                            params, x, shape, B, d_tangent, want_grad, want_lap, chunk_rows)


def wire_derivatives(desc: _lib.WireDesc, params, x=None, shape=None, B=None, d_tangent=None, want_grad=True, want_lap=True,
                     chunk_rows: int = 1 << 15):
    """Value, coordinate gradient and Laplacian of a WIRE network in forward mode (``inr_wire_derivatives`` on the rows ``x``
    [n, d], or ``inr_wire_derivatives_grid`` on ``get_mgrid(shape)``; exactly one of the two).  ``params`` is the flat buffer of
    ``inr_wire_param_offsets``.  Returns ``(y [n], grad [n, d_tangent] or None, lap [n] or None)``; derivatives are taken along
    the ``d_tangent`` leading axes (default: all ``d``)."""
    if (x is None) == (shape is None):
        raise ValueError("wire_derivatives takes exactly one of x and shape")
    _chk(params, "params")
    total = lib().inr_wire_param_count(C.byref(desc))
    if total < 0:
        check(int(total), "inr_wire_param_count")
    if params.numel() != total:
        raise ValueError(f"params has {params.numel()} floats, layout needs {total}")
    return _derivative_maps("inr_wire_derivatives_workspace_floats", "inr_wire_derivatives",
                            "inr_wire_derivatives_grid", torch.float32, desc, params, x, shape, B, d_tangent, want_grad, want_lap,
                            chunk_rows)


def siren_fit_workspace_bytes(desc: SirenDesc, n: int) -> int:
    return int(lib().inr_siren_fit_workspace_bytes(C.byref(desc), int(n)))


def siren_fit(desc: SirenDesc, params, grads, m, v, x, target, weight, first_step: int, n_steps: int, lr: float,
              beta1=0.9, beta2=0.999, eps=1e-8, losses=None, workspace=None):
    _chk_flat(desc, params=params, grads=grads, m=m, v=v)
    n = _rows(x, desc.in_features)
    _chk(target, "target")
    if target.numel() != n * desc.out_features:
        raise ValueError("target must have n*out_features elements")
    if weight is not None:
        _chk(weight, "weight")
        if weight.numel() != n * desc.out_features:
            raise ValueError("weight must have n*out_features elements")
    _chk_losses(losses, n_steps)
    workspace = _workspace(workspace, siren_fit_workspace_bytes(desc, n), x.device)
    check(lib().inr_siren_fit(C.byref(desc), params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(),
                              x.data_ptr(), target.data_ptr(), _ptr(weight), n, int(first_step), int(n_steps),
                              float(lr), float(beta1), float(beta2), float(eps), _ptr(losses), workspace.data_ptr(),
                              _nbytes(workspace), _stream()), "inr_siren_fit")
    return workspace


def siren_fit_cycle(desc: SirenDesc, params, grads, m, v, x, targets, weights, first_acq: int, first_step: int,
                    n_steps: int, lr: float, beta1=0.9, beta2=0.999, eps=1e-8, losses=None, workspace=None):
    """``inr_siren_fit_cycle``: ``targets`` (and ``weights``) are [n_acq, n * out_features]; step ``it`` fits acquisition
    ``(first_acq + it) % n_acq`` (master.py:137-148)."""
    _chk_flat(desc, params=params, grads=grads, m=m, v=v)
    n = _rows(x, desc.in_features)
    _chk(targets, "targets")
    if targets.dim() != 2 or targets.shape[1] != n * desc.out_features:
        raise ValueError("targets must be [n_acq, n*out_features]")
    n_acq = targets.shape[0]
    if weights is not None:
        _chk(weights, "weights")
        if tuple(weights.shape) != tuple(targets.shape):
            raise ValueError("weights must have the shape of targets")
    if not 0 <= int(first_acq) < n_acq:
        raise ValueError("first_acq out of range")
    _chk_losses(losses, n_steps)
    workspace = _workspace(workspace, siren_fit_workspace_bytes(desc, n), x.device)
    check(lib().inr_siren_fit_cycle(C.byref(desc), params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(),
                                    x.data_ptr(), targets.data_ptr(), _ptr(weights), int(n_acq), int(first_acq), n,
                                    int(first_step), int(n_steps), float(lr), float(beta1), float(beta2), float(eps),
                                    _ptr(losses), workspace.data_ptr(), _nbytes(workspace),
                                    _stream()), "inr_siren_fit_cycle")
    return workspace


def siren_fit_cycle_batch(desc: SirenDesc, params, grads, m, v, x, targets, weights, first_acqs, first_step: int,
                          n_steps: int, lr: float, beta1=0.9, beta2=0.999, eps=1e-8, losses=None, workspaces=None):
    """``inr_siren_fit_cycle_batch``: K independent fits of one shape on one ``x``.  ``params`` / ``grads`` / ``m`` / ``v`` /
    ``targets`` / ``workspaces`` are lists of K tensors (fit k: ``targets[k]`` is [n_acq_k, n * out_features]);
    ``weights`` / ``losses`` are None or lists whose entries may be None.  Bit for bit the K ``siren_fit_cycle`` calls in
    order; small networks share persistent launches.  Returns the list of workspaces."""
    K = len(params)
    if K < 1:
        raise ValueError("need at least one fit")
    for name, lst in (("grads", grads), ("m", m), ("v", v), ("targets", targets), ("first_acqs", first_acqs)):
        if len(lst) != K:
            raise ValueError(f"{name} has {len(lst)} entries, params {K}")
    for name, lst in (("weights", weights), ("losses", losses), ("workspaces", workspaces)):
        if lst is not None and len(lst) != K:
            raise ValueError(f"{name} has {len(lst)} entries, params {K}")
    for k in range(K):
        _chk_flat(desc, **{f"params[{k}]": params[k], f"grads[{k}]": grads[k], f"m[{k}]": m[k], f"v[{k}]": v[k]})
    if len({t.data_ptr() for t in params}) != K:
        raise ValueError("two fits share one params buffer")
    n = _rows(x, desc.in_features)
    n_acq = []
    for k in range(K):
        _chk(targets[k], f"targets[{k}]")
        if targets[k].dim() != 2 or targets[k].shape[1] != n * desc.out_features:
            raise ValueError(f"targets[{k}] must be [n_acq, n*out_features]")
        n_acq.append(int(targets[k].shape[0]))
        if weights is not None and weights[k] is not None:
            _chk(weights[k], f"weights[{k}]")
            if tuple(weights[k].shape) != tuple(targets[k].shape):
                raise ValueError(f"weights[{k}] must have the shape of targets[{k}]")
        if not 0 <= int(first_acqs[k]) < n_acq[k]:
            raise ValueError(f"first_acqs[{k}] out of range")
        if losses is not None:
            _chk_losses(losses[k], n_steps, f"losses[{k}]")
    need = siren_fit_workspace_bytes(desc, n)
    workspaces = [_workspace(w, need, x.device, f"workspaces[{k}]")
                  for k, w in enumerate(workspaces if workspaces is not None else [None] * K)]
    if len({w.data_ptr() for w in workspaces}) != K:
        raise ValueError("two fits share one workspace")
    ws_bytes = min(_nbytes(w) for w in workspaces)

    def ptrs(lst):
        return (C.c_void_p * K)(*[None if t is None else t.data_ptr() for t in lst])

    check(lib().inr_siren_fit_cycle_batch(
        C.byref(desc), K, ptrs(params), ptrs(grads), ptrs(m), ptrs(v), x.data_ptr(), ptrs(targets),
        None if weights is None else ptrs(weights), (C.c_int * K)(*n_acq), (C.c_int * K)(*[int(a) for a in first_acqs]), n,
        int(first_step), int(n_steps), float(lr), float(beta1), float(beta2), float(eps),
        None if losses is None else ptrs(losses), ptrs(workspaces), ws_bytes, _stream()), "inr_siren_fit_cycle_batch")
    return workspaces


REUSE_INPUT_IMAGE, REUSE_TARGET_STATS = 1, 2        # INR_REUSE_* of include/inrhip.h


def siren_loss_grad(desc: SirenDesc, params, grads, x, target, weight, count_total: int, loss, workspace=None, flags: int = 0):
    """Forward + loss + backward of one row shard (no optimizer); see ``inr_siren_loss_grad`` / ``_ex`` (``flags``: the
    caller vouches that x / the targets are those of the previous call on this workspace)."""
    _chk_flat(desc, params=params, grads=grads)
    n = _rows(x, desc.in_features)
    _chk(target, "target")
    _chk(loss, "loss")
    if target.numel() != n * desc.out_features:
        raise ValueError("target must have n*out_features elements")
    if weight is not None:
        _chk(weight, "weight")
    workspace = _workspace(workspace, siren_fit_workspace_bytes(desc, n), x.device, flags=int(flags))
    check(lib().inr_siren_loss_grad_ex(C.byref(desc), params.data_ptr(), grads.data_ptr(), x.data_ptr(), target.data_ptr(),
                                       _ptr(weight), n, int(count_total), loss.data_ptr(), workspace.data_ptr(),
                                       _nbytes(workspace), int(flags), _stream()),
          "inr_siren_loss_grad_ex")
    return workspace


def siren_hp_eligible(desc: SirenDesc) -> bool:
    """May the whole-network entry points run this shape on the pre-split kernels (``inr_siren_forward_train`` needs it)?"""
    return bool(lib().inr_siren_hp_eligible(C.byref(desc)))


def siren_forward_train(desc: SirenDesc, params, x, workspace=None, flags: int = 0):
    """``inr_siren_forward_train``: y = network(x), every layer's stash left in ``workspace`` for ``siren_backward_train``.
    Returns (y [n, 1], workspace)."""
    _chk_flat(desc, params=params)
    n = _rows(x, desc.in_features)
    workspace = _workspace(workspace, siren_fit_workspace_bytes(desc, n), x.device, flags=int(flags))
    y = torch.empty(n, desc.out_features, dtype=torch.float32, device=x.device)
    check(lib().inr_siren_forward_train(C.byref(desc), params.data_ptr(), x.data_ptr(), y.data_ptr(), n, workspace.data_ptr(),
                                        _nbytes(workspace), int(flags), _stream()),
          "inr_siren_forward_train")
    return y, workspace


def siren_backward_train(desc: SirenDesc, params, grads, gy, workspace):
    """``inr_siren_backward_train``: the flat gradient (network order) of sum(gy * y) from the pending forward's stash."""
    _chk(params, "params")
    _chk(grads, "grads")
    _chk(gy, "gy")
    n = gy.numel() // desc.out_features
    check(lib().inr_siren_backward_train(C.byref(desc), params.data_ptr(), grads.data_ptr(), gy.data_ptr(), n,
                                         workspace.data_ptr(), _nbytes(workspace), _stream()),
          "inr_siren_backward_train")
    return grads


# ---- the voxel-footprint forward model (include/inrhip.h (g)) ------------------------------------------------------------------
FOOTPRINT_MAX_SAMPLES = 64      # INR_FOOTPRINT_MAX_SAMPLES


def _chk_footprint_weights(fw) -> int:
    _chk(fw, "footprint weights")
    if fw.dim() != 1 or not 1 <= fw.numel() <= FOOTPRINT_MAX_SAMPLES:
        raise ValueError(f"footprint weights {tuple(fw.shape)} must be [K], 1 <= K <= {FOOTPRINT_MAX_SAMPLES}")
    return fw.numel()


def _chk_footprint_data(n, target, weight):
    _chk(target, "target")
    if target.numel() != n:
        raise ValueError(f"target has {target.numel()} elements, expected one per datum ({n})")
    if weight is not None:
        _chk(weight, "weight")
        if weight.numel() != n:
            raise ValueError(f"weight has {weight.numel()} elements, expected one per datum ({n})")


def footprint_expand(x: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """``inr_footprint_expand``: ``x`` [n, d] and ``offsets`` [K, d] -> [n*K, d], row ``i*K + k`` = ``x[i] + offsets[k]``."""
    _chk(x, "x")
    _chk(offsets, "offsets")
    if x.dim() != 2 or offsets.dim() != 2 or x.shape[1] != offsets.shape[1] or not 1 <= x.shape[1] <= 4:
        raise ValueError(f"x {tuple(x.shape)} and offsets {tuple(offsets.shape)} must be [n,d] and [K,d], 1 <= d <= 4")
    n, d = x.shape
    K = offsets.shape[0]
    if not 1 <= K <= FOOTPRINT_MAX_SAMPLES:
        raise ValueError(f"a footprint has 1 .. {FOOTPRINT_MAX_SAMPLES} sub-samples (got {K})")
    out = torch.empty((n * K, d), dtype=torch.float32, device=x.device)
    if n == 0:
        return out
    check(lib().inr_footprint_expand(out.data_ptr(), x.data_ptr(), offsets.data_ptr(), n, d, K, _stream()), "inr_footprint_expand")
    return out


def footprint_reduce(y: torch.Tensor, fw: torch.Tensor) -> torch.Tensor:
    """``inr_footprint_reduce``: ``y`` (n*K elements, sub-sample minor) and the weights ``fw`` [K] -> ``pred`` [n]."""
    _chk(y, "y")
    K = _chk_footprint_weights(fw)
    if y.numel() % K:
        raise ValueError(f"y has {y.numel()} elements, no multiple of K = {K}")
    n = y.numel() // K
    pred = torch.empty(n, dtype=torch.float32, device=y.device)
    if n == 0:
        return pred
    check(lib().inr_footprint_reduce(pred.data_ptr(), y.data_ptr(), fw.data_ptr(), n, K, _stream()), "inr_footprint_reduce")
    return pred


def footprint_loss_grad(y, target, weight, fw, count_total: int = 0, want_pred: bool = False):
    """``inr_footprint_loss_grad``: returns (gy [n*K], loss [1], pred [n] or None) of the footprint-averaged, weighted MSE."""
    _chk(y, "y")
    K = _chk_footprint_weights(fw)
    if y.numel() == 0 or y.numel() % K:
        raise ValueError(f"y has {y.numel()} elements, no positive multiple of K = {K}")
    n = y.numel() // K
    _chk_footprint_data(n, target, weight)
    gy = torch.empty(n * K, dtype=torch.float32, device=y.device)
    loss = torch.empty(1, dtype=torch.float32, device=y.device)
    pred = torch.empty(n, dtype=torch.float32, device=y.device) if want_pred else None
    floats = int(lib().inr_footprint_loss_workspace_floats(n))
    ws = _ws(4 * floats, y.device)
    check(lib().inr_footprint_loss_grad(gy.data_ptr(), loss.data_ptr(), _ptr(pred), y.data_ptr(), target.data_ptr(), _ptr(weight),
                                        fw.data_ptr(), n, K, int(count_total), ws.data_ptr(), _nbytes(ws) // 4, _stream()),
          "inr_footprint_loss_grad")
    return gy, loss, pred


def siren_fit_footprint_workspace_floats(desc: SirenDesc, n: int, K: int) -> int:
    """``inr_siren_fit_footprint_workspace_floats``; 0 for what ``inr_siren_fit_footprint`` does not serve."""
    return int(lib().inr_siren_fit_footprint_workspace_floats(C.byref(desc), int(n), int(K)))


def siren_fit_footprint(desc: SirenDesc, params, grads, m, v, x_sub, target, weight, fw, first_step: int, n_steps: int, lr: float,
                        beta1=0.9, beta2=0.999, eps=1e-8, losses=None, workspace=None):
    """``inr_siren_fit_footprint``: ``x_sub`` [n*K, in_features] (sub-sample minor), ``target`` / ``weight`` one per datum,
    ``fw`` [K].  Returns the workspace."""
    _chk_flat(desc, params=params, grads=grads, m=m, v=v)
    rows = _rows(x_sub, desc.in_features, "x_sub")
    K = _chk_footprint_weights(fw)
    if rows == 0 or rows % K:
        raise ValueError(f"x_sub has {rows} rows, no positive multiple of K = {K}")
    n = rows // K
    _chk_footprint_data(n, target, weight)
    _chk_losses(losses, n_steps)
    if not siren_hp_eligible(desc):
        raise ValueError("inr_siren_fit_footprint does not serve this network (ask inr_siren_hp_eligible: every sine layer a "
                         "multiple of 32 wide, hidden 128 / 256 / 512 / 1024, one output)")
    workspace = _workspace(workspace, 4 * siren_fit_footprint_workspace_floats(desc, n, K), x_sub.device)
    check(lib().inr_siren_fit_footprint(C.byref(desc), params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(),
                                        x_sub.data_ptr(), target.data_ptr(), _ptr(weight), fw.data_ptr(), n, K, int(first_step),
                                        int(n_steps), float(lr), float(beta1), float(beta2), float(eps), _ptr(losses),
                                        workspace.data_ptr(), _nbytes(workspace) // 4, _stream()), "inr_siren_fit_footprint")
    return workspace


# ---- model-based TV / Huber super-resolution (include/inrhip.h) --------------------------------------------------------
#
# Every rule about a HOST argument of this family is one validator below, named after its unit and taking ``who``, the caller's name: the
# public wrappers (baselines.py, the drivers) call it before the device is asked for, the entry-point wrappers here call it again in
# front of the kernel.  A validator reads no device tensor and returns plain Python values; the C arrays are the entry points' own step.
TVSR_MAX_FACTOR, TVSR_MAX_SIDE = _lib.INR_TVSR_MAX_FACTOR, _lib.INR_TVSR_MAX_SIDE
TVJ_MAX_CHANNELS, TVMF_MAX_FRAMES, TVSR3D_MAX_ITER = _lib.INR_TVJ_MAX_CHANNELS, _lib.INR_TVMF_MAX_FRAMES, _lib.INR_TVSR3D_MAX_ITER
TVMS_MAX_STACKS, TVMS_MAX_TAPS = _lib.INR_TVMS_MAX_STACKS, _lib.INR_TVMS_MAX_TAPS
TVMS_MAX_OFFSET, TVMS_MAX_EXTENT = 1 << 20, 2048
_TVJ_COUPLING = {"none": 0, "joint": 1}


def _chk_batch(t, name, rank, what, dtypes, shape=None, dtype_first=False) -> torch.Tensor:
    """A contiguous device batch of ``rank`` axes -- ``what`` names them -- of one of ``dtypes`` and, where given, of ``shape``.
    ``dtype_first``: the dtype, a host-only refusal, comes before the device."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    wrong_dtype = TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)} (got {t.dtype})") if t.dtype not in dtypes else None
    if dtype_first and wrong_dtype:
        raise wrong_dtype
    if not t.is_cuda:
        raise InrDeviceError(f"{name} is on {t.device}: the kernels only run on a HIP device (there is no CPU fallback)")
    if wrong_dtype:
        raise wrong_dtype
    if t.dim() != rank or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {what} batch (got {tuple(t.shape)})")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _chk_images(t, name, dtypes=(torch.float64,), shape=None) -> torch.Tensor:
    return _chk_batch(t, name, 3, "[n, rows, columns]", dtypes, shape)


def tv_factors(who, factors, rank=2, whole=False):
    """The ``rank`` block factors as ints, 1 .. TVSR_MAX_FACTOR each, refused by name; ``whole``: a fractional factor is refused, not
    truncated."""
    try:
        f = tuple(int(v) for v in factors)
        if len(f) != rank or (whole and any(int(v) != v for v in factors)):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"{who}: factors are {'(f0, f1)' if rank == 2 else '(f0, f1, f2)'}, one per trailing axis (got {factors!r})") from None
    if not all(1 <= v <= TVSR_MAX_FACTOR for v in f):
        raise ValueError(f"{who}: factors are 1 .. {TVSR_MAX_FACTOR} per axis (got {' x '.join(str(v) for v in f)})")
    return f


def tv_block_kernel(who, kernel, factors):
    """The HOST block kernel [f0][f1] as nested floats: finite, summing to 1 within 1e-9."""
    f0, f1 = factors
    k = np.asarray(kernel, dtype=np.float64)
    if k.shape != (f0, f1):
        raise ValueError(f"{who}: the kernel array must be [{f0}][{f1}] (got {k.shape})")
    if not np.isfinite(k).all() or abs(k.sum() - 1.0) > 1e-9:
        raise ValueError(f"{who}: the kernel array must be finite and sum to 1 (got sum {k.sum()!r})")
    return k.tolist()


def tv_kernel_factors(who, kernel, factors=None):
    """The HOST triple of 1-D kernel factors (k0, k1, k2) as float lists, each finite and summing to 1 within 1e-9: of ``factors``
    entries per axis, or (None: the taps of a stack) of any 1 .. TVMS_MAX_TAPS."""
    try:
        ks = [np.asarray(k, dtype=np.float64) for k in kernel]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: kernel must be 'mean', 'decimate' or a triple of 1-D arrays (k0, k1, k2)") from None
    if factors is None:
        if len(ks) != 3 or any(k.ndim != 1 or not 1 <= k.size <= TVMS_MAX_TAPS for k in ks):
            raise ValueError(f"{who}: the kernel is a triple of 1-D arrays of 1 .. {TVMS_MAX_TAPS} taps (got {[k.shape for k in ks]})")
    elif len(ks) != 3 or any(k.shape != (v,) for k, v in zip(ks, factors)):
        f = factors
        raise ValueError(f"{who}: the kernel factors must be 1-D arrays of {f[0]}, {f[1]} and {f[2]} entries (got {[k.shape for k in ks]})")
    for axis, k in enumerate(ks):
        if not np.isfinite(k).all() or abs(k.sum() - 1.0) > 1e-9:
            raise ValueError(f"{who}: kernel factor k{axis} must be finite and sum to 1 (got sum {k.sum()!r})")
    return [k.tolist() for k in ks]


def tv_hr_sides(who, hr, factors=None):
    """The HR sides (two: an image, three: a volume), 1 .. TVSR_MAX_SIDE each and, where given, whole blocks of ``factors``."""
    what, got = "image" if len(hr) == 2 else "volume", " x ".join(str(s) for s in hr)
    if any(s < 1 or s > TVSR_MAX_SIDE for s in hr):
        raise ValueError(f"{who}: HR {what}s of 1 .. {TVSR_MAX_SIDE} samples per axis (got {got})")
    if factors is not None and any(s % f for s, f in zip(hr, factors)):
        raise ValueError(f"{who}: the HR {what} {got} is no whole number of {' x '.join(str(f) for f in factors)} blocks")


def tv_hr_shape3d(who, hr_shape):
    """``hr_shape`` = (D, H, W) of a volume as ints, every side 1 .. TVSR_MAX_SIDE."""
    try:
        hr = tuple(int(v) for v in hr_shape)
        if len(hr) != 3:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"{who}: hr_shape is (D, H, W) (got {hr_shape!r})") from None
    tv_hr_sides(who, hr)
    return hr


def tv_scalars(who, lam, huber, n_iter, max_iter=None, span="0 .."):
    """(lam, huber, n_iter) of a solver, refused by name; ``span``: how the caller words the range of ``n_iter`` up to ``max_iter``."""
    lam, huber = float(lam), float(huber)
    if not 0.0 <= lam < np.inf:
        raise ValueError(f"{who}: lam must be finite and >= 0 (got {lam!r})")
    if not 0.0 <= huber < np.inf:
        raise ValueError(f"{who}: huber must be finite and >= 0 (got {huber!r})")
    if int(n_iter) != n_iter or n_iter < 0 or (max_iter is not None and n_iter > max_iter):
        bound = ">= 0" if max_iter is None else f"{span} {max_iter}"
        raise ValueError(f"{who}: n_iter must be an integer {bound} (got {n_iter!r})")
    return lam, huber, int(n_iter)


def tv_grad_weights(who, grad_weights):
    """(g0, g1, g2) of a 3-D prior as floats, refused by name."""
    try:
        g = tuple(float(v) for v in grad_weights)
    except (TypeError, ValueError):
        g = ()
    if len(g) != 3 or not all(0.0 <= v < np.inf for v in g):
        raise ValueError(f"{who}: grad_weights are (g0, g1, g2), finite and >= 0 (got {grad_weights!r})")
    return g


def tv_coupling(who, coupling):
    """'joint' or 'none', the prior's norm over the channels (or maps) of a group."""
    if coupling not in tuple(_TVJ_COUPLING):
        raise ValueError(f"{who}: coupling must be 'joint' or 'none' (got {coupling!r})")
    return coupling


def tvj_channels(who, channels):
    if not 1 <= channels <= TVJ_MAX_CHANNELS:
        raise ValueError(f"{who}: channels are 1 .. {TVJ_MAX_CHANNELS} per group (got {channels})")


def tvj_channel_weights(who, channel_weights, channels):
    """The HOST channel weights as ``channels`` floats within [0, 1], or None (all 1)."""
    if channel_weights is None:
        return None
    mu = np.asarray(channel_weights, np.float64).reshape(-1)
    if mu.shape != (channels,) or not (np.isfinite(mu).all() and (mu >= 0).all() and (mu <= 1).all()):
        raise ValueError(f"{who}: channel_weights are {channels} finite values within [0, 1] (got {mu.tolist()}); larger weights are a "
                         f"rescaled lam and huber")
    return mu.tolist()


def tvadc_model(who, b, channels, map_weights, coupling, s_max, adc_max, adc0):
    """The S0 / ADC model's host values, refused by name: -> (b, (mu_s, mu_d), s_max, adc_max, adc0) as floats."""
    try:
        vals = np.asarray(b, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: b must be a sequence of b-values (got {b!r})") from None
    if not 2 <= channels <= TVJ_MAX_CHANNELS:
        raise ValueError(f"{who}: b-values are 2 .. {TVJ_MAX_CHANNELS} per group (got {channels})")
    if vals.shape != (channels,):
        raise ValueError(f"{who}: b has {vals.size} b-values, expected one per channel ({channels})")
    if not (np.isfinite(vals).all() and (vals >= 0).all()):
        raise ValueError(f"{who}: b-values must be finite and >= 0 (got {vals.tolist()})")
    if vals.max() == vals.min():
        raise ValueError(f"{who}: the b-values are all equal ({vals[0]!r}): they determine no ADC")
    tv_coupling(who, coupling)
    try:
        mu = np.asarray(map_weights, np.float64).reshape(-1)
    except (TypeError, ValueError):
        mu = np.zeros(0)
    if mu.shape != (2,) or not (np.isfinite(mu).all() and (mu >= 0).all() and (mu <= 1).all()):
        raise ValueError(f"{who}: map_weights are (mu_s, mu_d), two finite values within [0, 1] (got {map_weights!r}); larger weights are "
                         f"a rescaled lam and huber")
    s_max, adc_max, adc0 = float(s_max), float(adc_max), float(adc0)
    if not 0.0 < s_max < np.inf:
        raise ValueError(f"{who}: s_max must be finite and > 0 (got {s_max!r})")
    if not 0.0 < adc_max < np.inf or not adc_max * vals.max() < np.inf:
        raise ValueError(f"{who}: adc_max must be finite and > 0 (got {adc_max!r})")
    if not 0.0 <= adc0 <= adc_max:
        raise ValueError(f"{who}: adc0 must be within [0, adc_max] (got {adc0!r}, adc_max {adc_max!r})")
    return vals.tolist(), mu.tolist(), s_max, adc_max, adc0


def adc_bvalues(who, b):
    """The HOST b-values of ``adc_signal`` as floats: 1 .. TVJ_MAX_CHANNELS of them, finite."""
    vals = np.asarray(b, np.float64).reshape(-1)
    if not 1 <= vals.size <= TVJ_MAX_CHANNELS or not np.isfinite(vals).all():
        raise ValueError(f"{who}: b is 1 .. {TVJ_MAX_CHANNELS} finite b-values (got {vals.tolist()})")
    return vals.tolist()


def tgv_ratio(who, ratio):
    ratio = float(ratio)
    if not 0.0 < ratio < np.inf:
        raise ValueError(f"{who}: ratio must be finite and > 0 (got {ratio!r})")
    return ratio


def tvmf_frame_count(who, K):
    if not 1 <= K <= TVMF_MAX_FRAMES:
        raise ValueError(f"{who}: frames per image are 1 .. {TVMF_MAX_FRAMES} (got {K})")


def tvms_stack_count(who, count):
    if not 1 <= count <= TVMS_MAX_STACKS:
        raise ValueError(f"{who}: stacks per volume are 1 .. {TVMS_MAX_STACKS} (got {count})")


def tvms_offsets(who, offsets):
    """The offsets of a stack, three whole numbers of HR voxels within +-TVMS_MAX_OFFSET, as ints."""
    try:
        o = tuple(int(v) for v in offsets)
        if len(o) != 3 or any(int(v) != v for v in offsets):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"{who}: offsets are three whole numbers of HR voxels (got {offsets!r})") from None
    if not all(abs(v) <= TVMS_MAX_OFFSET for v in o):
        raise ValueError(f"{who}: offsets are within +-{TVMS_MAX_OFFSET} HR voxels (got {o})")
    return o


def tvms_lr_shape(who, shape):
    """The LR shape (n0, n1, n2) of a stack as ints, 1 .. TVMS_MAX_EXTENT each."""
    try:
        n = tuple(int(v) for v in shape)
        if len(n) != 3:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"{who}: an LR shape is (n0, n1, n2) (got {shape!r})") from None
    if not all(1 <= v <= TVMS_MAX_EXTENT for v in n):
        raise ValueError(f"{who}: LR extents are 1 .. {TVMS_MAX_EXTENT} per axis (got {n})")
    return n


def tvop_operator_pair(who, operators):
    try:
        r0, r1 = operators
    except (TypeError, ValueError):
        raise ValueError(f"{who}: operators are a pair (R0 [h, H], R1 [w, W])") from None
    return r0, r1


def tvop_operator_shape(who, name, shape):
    """The shape [rows, columns] of one operator of the pair as ints, every side 1 .. TVSR_MAX_SIDE."""
    if len(shape) != 2 or not all(1 <= int(s) <= TVSR_MAX_SIDE for s in shape):
        raise ValueError(f"{who}: {name} must be 2-D with sides of 1 .. {TVSR_MAX_SIDE} (got shape {tuple(shape)})")
    return int(shape[0]), int(shape[1])


def _f64_workspace(workspace, need, device) -> torch.Tensor:
    """The caller's workspace, or a fresh one of ``need`` doubles."""
    if workspace is None:
        return torch.empty(need, dtype=torch.float64, device=device)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.float64 or not workspace.is_cuda or workspace.numel() < need:
        raise ValueError(f"workspace must be a device float64 tensor of at least {need} elements")
    return workspace


def _tv_solve(entry, y, chk_y, chk_x0, hr, weight, x0, workspace, need, rest, results=2, after_out=(), after_y=()):
    """The tail the solves share, behind their checks of ``y`` and of the host values: ``weight`` like ``y`` (``chk_y``) and ``x0`` like
    the result [n, *hr] (``chk_x0``), both of the dtype of ``y``; the result and ``results`` per-image float64 values; ``entry`` or its
    ``_f32`` twin by the dtype; nothing launched for n = 0; the float64 workspace of ``need()`` doubles, the caller's or a fresh one;
    the call ``entry(out, *after_out, *results, y, *after_y, weight, x0, *rest, workspace, its doubles, stream)``.
    -> (out, *results)."""
    n = y.shape[0]
    if weight is not None:
        chk_y(weight, "weight", (y.dtype,), y.shape)
    if x0 is not None:
        chk_x0(x0, "x0", (y.dtype,), (n, *hr))
    out = torch.empty((n, *hr), dtype=y.dtype, device=y.device)
    values = [torch.zeros(n, dtype=torch.float64, device=y.device) for _ in range(results)]
    if n:
        entry = entry if y.dtype == torch.float64 else entry + "_f32"
        workspace = _f64_workspace(workspace, need(), y.device)
        check(getattr(lib(), entry)(out.data_ptr(), *after_out, *(v.data_ptr() for v in values), y.data_ptr(), *after_y, _ptr(weight),
                                    _ptr(x0), *rest, workspace.data_ptr(), workspace.numel(), _stream()), entry)
    return (out, *values)


def _solve_scalars(who, lam, alpha, n_iter, max_iter=None):
    """``tv_scalars`` of what ``float`` and ``int`` make of an entry point's scalars: a fractional ``n_iter`` is truncated here, as ever."""
    return tv_scalars(who, float(lam), float(alpha), int(n_iter), max_iter)


def _doubles(values):
    """The C array of host floats an entry point takes."""
    values = list(values)
    return (C.c_double * len(values))(*values)


def _block_kernel(who, kernel, factors):
    """(f0, f1, the C array [f0][f1]) of a 2-D block operator."""
    f0, f1 = tv_factors(who, factors)
    return f0, f1, _doubles(v for row in tv_block_kernel(who, kernel, (f0, f1)) for v in row)


def block_apply(x: torch.Tensor, factors, kernel) -> torch.Tensor:
    """``inr_block_apply2d``: ``x`` [n, H, W] float64 -> ``A x`` [n, H/f0, W/f1]; ``kernel`` [f0][f1] host values that sum to 1."""
    _chk_images(x, "x")
    f0, f1, k = _block_kernel("block_apply", kernel, factors)
    n, H, W = x.shape
    tv_hr_sides("block_apply", (H, W), (f0, f1))
    out = torch.empty((n, H // f0, W // f1), dtype=torch.float64, device=x.device)
    check(lib().inr_block_apply2d(out.data_ptr(), x.data_ptr(), n, H, W, f0, f1, k, _stream()), "inr_block_apply2d")
    return out


def block_adjoint(r: torch.Tensor, factors, kernel) -> torch.Tensor:
    """``inr_block_adjoint2d``: ``r`` [n, h, w] float64 -> ``A^T r`` [n, f0 h, f1 w]."""
    _chk_images(r, "r")
    f0, f1, k = _block_kernel("block_adjoint", kernel, factors)
    n, h, w = r.shape
    tv_hr_sides("block_adjoint", (h * f0, w * f1), (f0, f1))
    out = torch.empty((n, h * f0, w * f1), dtype=torch.float64, device=r.device)
    check(lib().inr_block_adjoint2d(out.data_ptr(), r.data_ptr(), n, h * f0, w * f1, f0, f1, k, _stream()), "inr_block_adjoint2d")
    return out


def tvsr_workspace_doubles(n: int, H: int, W: int) -> int:
    """``inr_tvsr_workspace_doubles``; 0 for sizes ``inr_tvsr_solve2d`` refuses."""
    return int(lib().inr_tvsr_workspace_doubles(int(n), int(H), int(W)))


def tvsr_solve(y: torch.Tensor, factors, kernel, lam: float, alpha: float, n_iter: int, weight=None, x0=None, workspace=None):
    """``inr_tvsr_solve2d`` / ``_f32`` by the dtype of ``y`` [n, h, w]: returns (x [n, f0 h, f1 w] of that dtype, energy [n] float64,
    change [n] float64).  ``weight`` [n, h, w] and ``x0`` [n, f0 h, f1 w] share the dtype; ``workspace``: a float64 tensor."""
    who = "tvsr_solve"
    _chk_images(y, "y", (torch.float32, torch.float64))
    f0, f1, k = _block_kernel(who, kernel, factors)
    n, h, w = y.shape
    H, W = h * f0, w * f1
    tv_hr_sides(who, (H, W), (f0, f1))
    lam, alpha, n_iter = _solve_scalars(who, lam, alpha, n_iter)
    return _tv_solve("inr_tvsr_solve2d", y, _chk_images, _chk_images, (H, W), weight, x0, workspace,
                     lambda: tvsr_workspace_doubles(n, H, W), (n, H, W, f0, f1, k, lam, alpha, n_iter))


# ---- the same with one prior over the channels of a group (include/inrhip.h) -------------------------------------------
def _chk_groups(t, name, dtypes, shape=None) -> torch.Tensor:
    return _chk_batch(t, name, 4, "[n, channels, rows, columns]", dtypes, shape)


def tvj_workspace_doubles(n: int, channels: int, H: int, W: int) -> int:
    """``inr_tvj_workspace_doubles``; 0 for sizes ``inr_tvj_solve2d`` refuses."""
    return int(lib().inr_tvj_workspace_doubles(int(n), int(channels), int(H), int(W)))


def tvj_solve(y: torch.Tensor, factors, kernel, channel_weights, lam: float, alpha: float, coupling, n_iter: int, weight=None, x0=None,
              workspace=None):
    """``inr_tvj_solve2d`` / ``_f32`` by the dtype of ``y`` [n, C, h, w]: returns (x [n, C, f0 h, f1 w] of that dtype, energy [n]
    float64, change [n] float64).  ``channel_weights``: C host values in [0, 1] or None (all 1); ``coupling``: 'joint' or 'none';
    ``weight`` [n, C, h, w] and ``x0`` [n, C, f0 h, f1 w] share the dtype; ``workspace``: a float64 tensor."""
    who = "tvj_solve"
    _chk_groups(y, "y", (torch.float32, torch.float64))
    f0, f1, k = _block_kernel(who, kernel, factors)
    n, ch, h, w = y.shape
    H, W = h * f0, w * f1
    tvj_channels(who, ch)
    tv_hr_sides(who, (H, W), (f0, f1))
    tv_coupling(who, coupling)
    mu = tvj_channel_weights(who, channel_weights, ch)
    lam, alpha, n_iter = _solve_scalars(who, lam, alpha, n_iter)
    return _tv_solve("inr_tvj_solve2d", y, _chk_groups, _chk_groups, (ch, H, W), weight, x0, workspace,
                     lambda: tvj_workspace_doubles(n, ch, H, W),
                     (n, ch, H, W, f0, f1, k, None if mu is None else _doubles(mu), lam, alpha, _TVJ_COUPLING[coupling], n_iter))


# ---- the S0 / ADC maps of a group as the unknowns (include/inrhip.h) ------------------------------------------------------
def tvadc_workspace_doubles(n: int, channels: int, H: int, W: int, factors) -> int:
    """``inr_tvadc_workspace_doubles``; 0 for sizes ``inr_tvadc_solve2d`` refuses."""
    return int(lib().inr_tvadc_workspace_doubles(int(n), int(channels), int(H), int(W), int(factors[0]), int(factors[1])))


def tvadc_solve(y: torch.Tensor, b, factors, kernel, map_weights, lam: float, alpha: float, coupling, n_iter: int, s_max: float,
                adc_max: float, adc0: float, weight=None, x0=None, workspace=None):
    """``inr_tvadc_solve2d`` / ``_f32`` by the dtype of ``y`` [n, C, h, w]: returns (s0 [n, f0 h, f1 w] and adc [n, f0 h, f1 w] of that
    dtype -- two views of one [n, 2, H, W] tensor --, energy [n] float64, change [n] float64).  ``b``: C host b-values; ``map_weights``:
    (mu_s, mu_d) host values in [0, 1]; ``coupling``: 'joint' or 'none'; ``weight`` [n, C, h, w] and ``x0`` [n, 2, f0 h, f1 w] (the
    maps s0, adc) share the dtype; ``workspace``: a float64 tensor."""
    who = "tvadc_solve"
    _chk_groups(y, "y", (torch.float32, torch.float64))
    f0, f1, k = _block_kernel(who, kernel, factors)
    n, ch, h, w = y.shape
    H, W = h * f0, w * f1
    vals, mu, s_max, adc_max, adc0 = tvadc_model(who, b, ch, map_weights, coupling, s_max, adc_max, adc0)
    tv_hr_sides(who, (H, W), (f0, f1))
    lam, alpha, n_iter = _solve_scalars(who, lam, alpha, n_iter)
    out, energy, change = _tv_solve("inr_tvadc_solve2d", y, _chk_groups, _chk_groups, (2, H, W), weight, x0, workspace,
                                    lambda: tvadc_workspace_doubles(n, ch, H, W, (f0, f1)),
                                    (n, ch, H, W, f0, f1, k, _doubles(vals), _doubles(mu), lam, alpha, _TVJ_COUPLING[coupling], n_iter,
                                     s_max, adc_max, adc0))
    return out[:, 0], out[:, 1], energy, change


def adc_signal(s0: torch.Tensor, adc: torch.Tensor, b) -> torch.Tensor:
    """``inr_adc_signal`` / ``_f32`` by the dtype of ``s0`` [n, H, W]: the model's images ``s0 exp(-b_c adc)`` [n, C, H, W] of two maps
    of one shape and dtype; ``b``: C host b-values, 1 .. 16."""
    _chk_images(s0, "s0", (torch.float32, torch.float64))
    _chk_images(adc, "adc", (s0.dtype,), s0.shape)
    vals = adc_bvalues("adc_signal", b)
    n, H, W = s0.shape
    out = torch.empty((n, len(vals), H, W), dtype=s0.dtype, device=s0.device)
    if out.numel() == 0:
        return out
    entry = "inr_adc_signal" if s0.dtype == torch.float64 else "inr_adc_signal_f32"
    check(getattr(lib(), entry)(out.data_ptr(), s0.data_ptr(), adc.data_ptr(), _doubles(vals), n, len(vals), H * W, _stream()), entry)
    return out


# ---- MP-PCA denoising of a multi-measurement stack (include/inrhip.h) -----------------------------------------------------
MPPCA_ESTIMATORS = {"exp1": 1, "exp2": 2}


def mppca_window(who, window, shape, M):
    """The window (w0, w1, w2) of a stack of ``M`` measurements over a volume ``shape`` as ints; refuses, by name, what
    ``inr_mppca_denoise`` would refuse."""
    try:
        win = tuple(int(w) for w in window)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: window must be three odd sides (got {window!r})") from None
    if len(win) != 3 or any(w < 1 or w % 2 == 0 for w in win) or any(int(w) != w for w in window):
        raise ValueError(f"{who}: window must be three odd sides >= 1 (got {tuple(window)!r})")
    for name, w, n in zip(("first", "second", "third"), win, shape):
        if n > 0 and w > n:
            raise ValueError(f"{who}: the {name} window side ({w}) is larger than its axis ({n}): choose a smaller window "
                             f"(volume {tuple(shape)}, window {win})")
    N = win[0] * win[1] * win[2]
    if M < 2 or N < 2:
        raise ValueError(f"{who}: at least 2 measurements and a window of at least 2 voxels are needed (got M = {M}, N = {N})")
    if min(M, N) > _lib.INR_MPPCA_MAX_RANK:
        raise ValueError(f"{who}: min(M, N) = min({M}, {N}) exceeds the rank limit {_lib.INR_MPPCA_MAX_RANK}: shrink the window or "
                         f"split the measurements")
    if max(M, N) > _lib.INR_MPPCA_MAX_LONG:
        raise ValueError(f"{who}: max(M, N) = max({M}, {N}) exceeds {_lib.INR_MPPCA_MAX_LONG}")
    return win


def mppca_denoise(x: torch.Tensor, window=(5, 5, 5), mask=None, estimator="exp2", want_sigma=True, want_rank=True):
    """``inr_mppca_denoise`` / ``_f32`` by the dtype of ``x`` [M, D, H, W] on the current stream: returns (out [M, D, H, W] of that dtype,
    sigma [D, H, W] of that dtype or None, rank [D, H, W] int32 or None).  ``mask``: a device uint8 or bool tensor [D, H, W] or None;
    ``estimator``: 'exp1' or 'exp2'."""
    who = "mppca_denoise"
    _chk_batch(x, "x", 4, "[M, D, H, W]", (torch.float32, torch.float64))
    if estimator not in MPPCA_ESTIMATORS:
        raise ValueError(f"{who}: estimator must be 'exp1' or 'exp2' (got {estimator!r})")
    M, D, H, W = x.shape
    win = mppca_window(who, window, (D, H, W), M)
    if mask is not None:
        _chk_batch(mask, "mask", 3, "[D, H, W]", (torch.uint8, torch.bool), (D, H, W))
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    out = torch.empty_like(x)
    sigma = torch.empty((D, H, W), dtype=x.dtype, device=x.device) if want_sigma else None
    rank = torch.empty((D, H, W), dtype=torch.int32, device=x.device) if want_rank else None
    if D * H * W == 0:
        return out, sigma, rank
    entry = "inr_mppca_denoise" if x.dtype == torch.float64 else "inr_mppca_denoise_f32"
    check(getattr(lib(), entry)(out.data_ptr(), _ptr(sigma), _ptr(rank), x.data_ptr(), _ptr(mask), M, D, H, W, *win,
                                MPPCA_ESTIMATORS[estimator], _stream()), entry)
    return out, sigma, rank


# ---- Gibbs-ringing removal by local sub-voxel shifts (include/inrhip.h) ---------------------------------------------------
DEGIBBS_DEFAULT_SHIFTS, DEGIBBS_DEFAULT_WINDOW = 20, (1, 3)


def degibbs_params(who, sides, nshifts, window):
    """(nshifts, w_min, w_max) as ints for lines of the lengths ``sides``; refuses, by name, what ``inr_degibbs_lines`` /
    ``inr_degibbs2d`` would refuse."""
    try:
        win = tuple(int(w) for w in window)
        ok = len(win) == 2 and all(int(w) == w for w in window)
    except (TypeError, ValueError):
        win, ok = (), False
    if not ok or not 1 <= win[0] <= win[1] <= _lib.INR_DEGIBBS_MAX_WINDOW:
        raise ValueError(f"{who}: window must be (w_min, w_max) with 1 <= w_min <= w_max <= {_lib.INR_DEGIBBS_MAX_WINDOW} (got {window!r})")
    if isinstance(nshifts, bool) or int(nshifts) != nshifts or not 1 <= int(nshifts) <= _lib.INR_DEGIBBS_MAX_SHIFTS:
        raise ValueError(f"{who}: nshifts must be 1 .. {_lib.INR_DEGIBBS_MAX_SHIFTS} (got {nshifts!r})")
    for n in sides:
        if not 2 * win[1] + 3 <= n <= _lib.INR_DEGIBBS_MAX_LINE:
            raise ValueError(f"{who}: lines of 2 w_max + 3 = {2 * win[1] + 3} .. {_lib.INR_DEGIBBS_MAX_LINE} samples (got {n})")
    return int(nshifts), win[0], win[1]


def degibbs_lines_workspace_doubles(n_lines: int, n: int, nshifts: int = DEGIBBS_DEFAULT_SHIFTS) -> int:
    """``inr_degibbs_lines_workspace_doubles``; 0 for sizes every call refuses."""
    return int(lib().inr_degibbs_lines_workspace_doubles(n_lines, n, nshifts))


def degibbs2d_workspace_doubles(n: int, H: int, W: int, nshifts: int = DEGIBBS_DEFAULT_SHIFTS) -> int:
    """``inr_degibbs2d_workspace_doubles``; 0 for sizes every call refuses."""
    return int(lib().inr_degibbs2d_workspace_doubles(n, H, W, nshifts))


def degibbs_lines(x: torch.Tensor, nshifts=DEGIBBS_DEFAULT_SHIFTS, window=DEGIBBS_DEFAULT_WINDOW, want_choice=False, workspace=None):
    """``inr_degibbs_lines`` / ``_f32`` by the dtype of ``x`` [n_lines, n] on the current stream: returns (out like ``x``, choice
    [n_lines, n] int32 -- the index of the chosen shift in list order -- or None)."""
    _chk_batch(x, "x", 2, "[n_lines, n]", (torch.float32, torch.float64), dtype_first=True)
    n_lines, n = x.shape
    nshifts, w_min, w_max = degibbs_params("degibbs_lines", (n,), nshifts, window)
    out = torch.empty_like(x)
    choice = torch.empty((n_lines, n), dtype=torch.int32, device=x.device) if want_choice else None
    if n_lines == 0:
        return out, choice
    ws = _f64_workspace(workspace, degibbs_lines_workspace_doubles(n_lines, n, nshifts), x.device)
    entry = "inr_degibbs_lines" if x.dtype == torch.float64 else "inr_degibbs_lines_f32"
    check(getattr(lib(), entry)(out.data_ptr(), _ptr(choice), x.data_ptr(), n_lines, n, nshifts, w_min, w_max, ws.data_ptr(), ws.numel(),
                                _stream()), entry)
    return out, choice


def degibbs2d(x: torch.Tensor, nshifts=DEGIBBS_DEFAULT_SHIFTS, window=DEGIBBS_DEFAULT_WINDOW, want_choice=False, workspace=None):
    """``inr_degibbs2d`` / ``_f32`` by the dtype of ``x`` [n, H, W] on the current stream: returns (out like ``x``, choice [2, n, H, W]
    int32, the axis-0 pass first, or None)."""
    _chk_images(x, "x", (torch.float32, torch.float64))
    n, H, W = x.shape
    nshifts, w_min, w_max = degibbs_params("degibbs2d", (H, W), nshifts, window)
    out = torch.empty_like(x)
    choice = torch.empty((2, n, H, W), dtype=torch.int32, device=x.device) if want_choice else None
    if n == 0:
        return out, choice
    ws = _f64_workspace(workspace, degibbs2d_workspace_doubles(n, H, W, nshifts), x.device)
    entry = "inr_degibbs2d" if x.dtype == torch.float64 else "inr_degibbs2d_f32"
    check(getattr(lib(), entry)(out.data_ptr(), _ptr(choice), x.data_ptr(), n, H, W, nshifts, w_min, w_max, ws.data_ptr(), ws.numel(),
                                _stream()), entry)
    return out, choice


def degibbs_shift(choice: torch.Tensor, nshifts: int) -> torch.Tensor:
    """The chosen shifts in pixels (float64) from the indices ``choice`` of ``degibbs_lines`` / ``degibbs2d``."""
    c = choice.to(torch.float64)
    return torch.where(c <= nshifts, c, nshifts - c) / (2.0 * nshifts)


# ---- non-local means on volumes and non-local upsampling (include/inrhip.h) ----------------------------------------------
NLM_CENTERS = {"max": _lib.INR_NLM_CENTER_MAX, "one": _lib.INR_NLM_CENTER_ONE}


def _nlm_triple(who, name, value, most):
    try:
        raw = (value,) * 3 if isinstance(value, (int, np.integer)) and not isinstance(value, bool) else tuple(value)
        t = tuple(int(v) for v in raw)
        ok = len(t) == 3 and all(int(v) == v and not isinstance(v, bool) for v in raw)
    except (TypeError, ValueError):
        t, ok = (), False
    if not ok or not all(0 <= v <= most for v in t):
        raise ValueError(f"{who}: {name} must be an int or a triple of ints 0 .. {most} (got {value!r})")
    return t


def nlm_radii(who, search, patch):
    """The search radii (s0, s1, s2), 0 .. 5 each, and the patch radii (r0, r1, r2), 0 .. 2 each, from an int or a triple; refuses, by
    name, what ``inr_nlm3d`` would refuse."""
    return _nlm_triple(who, "search", search, _lib.INR_NLM_MAX_SEARCH), _nlm_triple(who, "patch", patch, _lib.INR_NLM_MAX_PATCH)


def nlm_center(who, center):
    if center not in NLM_CENTERS:
        raise ValueError(f"{who}: center must be 'max' or 'one' (got {center!r})")
    return NLM_CENTERS[center]


def nlm_strength(who, h2):
    """A scalar strength ``h2`` as a float: finite and > 0."""
    try:
        v = float(h2)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: h2 must be a number or a device map (got {h2!r})") from None
    if not (np.isfinite(v) and v > 0.0):
        raise ValueError(f"{who}: a scalar h2 must be finite and > 0 (got {h2!r})")
    return v


def nlm_channels(who, channels):
    if not 1 <= channels <= _lib.INR_NLM_MAX_CHANNELS:
        raise ValueError(f"{who}: channels must be 1 .. {_lib.INR_NLM_MAX_CHANNELS} (got {channels})")
    return channels


def nlm_volume(who, shape):
    """A volume (D, H, W): every side at least 1, fewer than 2^31 voxels."""
    if len(shape) != 3 or any(s < 1 for s in shape) or shape[0] * shape[1] * shape[2] >= 1 << 31:
        raise ValueError(f"{who}: volumes of at least 1 sample per axis and fewer than 2^31 voxels (got {' x '.join(str(s) for s in shape)})")


def nlm_schedule(who, levels, n_iter, relax):
    """(the levels as floats, n_iter, relax): every level finite and > 0, ``len(levels) * n_iter`` in 0 .. 10,000, relax in (0, 1]."""
    try:
        lv = [float(v) for v in levels]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: levels must be a sequence of numbers (got {levels!r})") from None
    if not all(np.isfinite(v) and v > 0.0 and v * v > 0.0 for v in lv):
        raise ValueError(f"{who}: every level must be finite and > 0 (got {levels!r})")
    if isinstance(n_iter, bool) or int(n_iter) != n_iter or int(n_iter) < 0 or len(lv) * int(n_iter) > _lib.INR_NLM_MAX_PASSES:
        raise ValueError(f"{who}: n_iter must be an integer >= 0 with len(levels) * n_iter <= {_lib.INR_NLM_MAX_PASSES} "
                         f"(got {len(lv)} levels, n_iter = {n_iter!r})")
    relax = float(relax)
    if not 0.0 < relax <= 1.0:
        raise ValueError(f"{who}: relax must lie in (0, 1] (got {relax!r})")
    return lv, int(n_iter), relax


def nlm3d(x: torch.Tensor, h2, search=3, patch=1, guide=None, sigma2=None, mask=None, center="max"):
    """``inr_nlm3d`` / ``_f32`` by the dtype of ``x`` [G, C, D, H, W] on the current stream: returns out like ``x``.  ``h2``: a number
    (finite, > 0) or a device map [G, D, H, W] of that dtype; ``guide`` [G, D, H, W] of that dtype or None (C must be 1: ``x`` guides
    itself); ``sigma2`` [G, D, H, W] of that dtype or None (None: no Rician correction); ``mask`` [G, D, H, W] uint8 / bool or None;
    ``search`` / ``patch``: an int or a triple; ``center``: 'max' or 'one'."""
    who = "nlm3d"
    s, r = nlm_radii(who, search, patch)
    c = nlm_center(who, center)
    h2_map = h2 if isinstance(h2, torch.Tensor) else None
    h2 = 0.0 if h2_map is not None else nlm_strength(who, h2)
    _chk_batch(x, "x", 5, "[G, C, D, H, W]", (torch.float32, torch.float64), dtype_first=True)
    G, Cn, D, H, W = x.shape
    nlm_channels(who, Cn)
    nlm_volume(who, (D, H, W))
    if guide is None and Cn != 1:
        raise ValueError(f"{who}: without a guide x must have one channel (got {Cn}): the guide is x itself")
    for name, t in (("guide", guide), ("h2", h2_map), ("sigma2", sigma2)):
        if t is not None:
            _chk_batch(t, name, 4, "[G, D, H, W]", (x.dtype,), (G, D, H, W))
    if mask is not None:
        _chk_batch(mask, "mask", 4, "[G, D, H, W]", (torch.uint8, torch.bool), (G, D, H, W))
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    out = torch.empty_like(x)
    if G == 0:
        return out
    entry = "inr_nlm3d" if x.dtype == torch.float64 else "inr_nlm3d_f32"
    check(getattr(lib(), entry)(out.data_ptr(), x.data_ptr(), _ptr(guide), h2, _ptr(h2_map), _ptr(sigma2), _ptr(mask), G, Cn, D, H, W, *s, *r,
                                c, _stream()), entry)
    return out


def nlm_upsample_workspace_doubles(n: int, D: int, H: int, W: int, factors) -> int:
    """``inr_nlm_upsample_workspace_doubles``; 0 for sizes ``inr_nlm_upsample`` refuses."""
    f0, f1, f2 = (int(v) for v in factors)
    return int(lib().inr_nlm_upsample_workspace_doubles(int(n), int(D), int(H), int(W), f0, f1, f2))


def nlm_upsample(y: torch.Tensor, factors, kernel, levels, n_iter: int = 2, search=2, patch=1, relax: float = 1.0, guide=None, x0=None,
                 workspace=None, want_change=True):
    """``inr_nlm_upsample`` / ``_f32`` by the dtype of ``y`` [n, d, h, w]: returns (x [n, f0 d, f1 h, f2 w] of that dtype, change
    [len(levels) * n_iter, n] float64 or None).  ``kernel``: (k0, k1, k2) host values; ``levels``: the strengths h_l, one NLM pass uses
    h2 = h_l^2; ``guide`` and ``x0`` [n, f0 d, f1 h, f2 w] share the dtype; ``workspace``: a float64 tensor."""
    who = "nlm_upsample"
    f, k = _block_kernel3d(who, kernel, factors)
    s, r = nlm_radii(who, search, patch)
    lv, n_iter, relax = nlm_schedule(who, levels, n_iter, relax)
    _chk_volumes(y, "y", (torch.float32, torch.float64))
    n, d, h, w = y.shape
    D, H, W = d * f[0], h * f[1], w * f[2]
    nlm_volume(who, (D, H, W))
    for name, t in (("guide", guide), ("x0", x0)):
        if t is not None:
            _chk_volumes(t, name, (y.dtype,), (n, D, H, W))
    out = torch.empty((n, D, H, W), dtype=y.dtype, device=y.device)
    change = torch.zeros((len(lv) * n_iter, n), dtype=torch.float64, device=y.device) if want_change else None
    if n:
        entry = "inr_nlm_upsample" if y.dtype == torch.float64 else "inr_nlm_upsample_f32"
        ws = _f64_workspace(workspace, nlm_upsample_workspace_doubles(n, D, H, W, f), y.device)
        check(getattr(lib(), entry)(out.data_ptr(), _ptr(change), y.data_ptr(), _ptr(x0), _ptr(guide), n, D, H, W, *f, *k, _doubles(lv),
                                    len(lv), n_iter, relax, *s, *r, ws.data_ptr(), ws.numel(), _stream()), entry)
    return out, change


# ---- second-order TGV under the block operator (include/inrhip.h) --------------------------------------------------------
def tgv_workspace_doubles(n: int, H: int, W: int) -> int:
    """``inr_tgv_workspace_doubles``; 0 for sizes ``inr_tgv_solve2d`` refuses."""
    return int(lib().inr_tgv_workspace_doubles(int(n), int(H), int(W)))


def tgv_solve(y: torch.Tensor, factors, kernel, lam: float, ratio: float, alpha: float, n_iter: int, weight=None, x0=None,
              workspace=None, want_v=True):
    """``inr_tgv_solve2d`` / ``_f32`` by the dtype of ``y`` [n, h, w]: returns (x [n, f0 h, f1 w] of that dtype, v [n, 2, f0 h, f1 w] of
    that dtype or None where ``want_v`` is false, energy [n] float64, change [n] float64).  ``lam`` weighs the first-order term,
    ``ratio * lam`` the second-order one; ``weight`` [n, h, w] and ``x0`` [n, f0 h, f1 w] share the dtype; ``workspace``: a float64
    tensor."""
    who = "tgv_solve"
    _chk_images(y, "y", (torch.float32, torch.float64))
    f0, f1, k = _block_kernel(who, kernel, factors)
    n, h, w = y.shape
    H, W = h * f0, w * f1
    tv_hr_sides(who, (H, W), (f0, f1))
    ratio = float(ratio)
    lam, alpha, n_iter = _solve_scalars(who, lam, alpha, n_iter)
    tgv_ratio(who, ratio)
    v = torch.empty((n, 2, H, W), dtype=y.dtype, device=y.device) if want_v else None
    out, energy, change = _tv_solve("inr_tgv_solve2d", y, _chk_images, _chk_images, (H, W), weight, x0, workspace,
                                    lambda: tgv_workspace_doubles(n, H, W), (n, H, W, f0, f1, k, lam, ratio, alpha, n_iter),
                                    after_out=(_ptr(v),))
    return out, v, energy, change


# ---- the same on volumes: slice profile, 3-D prior, many workgroups per volume (include/inrhip.h) ----------------------
def _chk_volumes(t, name, dtypes=(torch.float64,), shape=None) -> torch.Tensor:
    return _chk_batch(t, name, 4, "[n, slices, rows, columns]", dtypes, shape)


def _block_kernel3d(who, kernel, factors):
    """((f0, f1, f2), the C arrays k0 [f0], k1 [f1], k2 [f2]) of a 3-D block operator."""
    f = tv_factors(who, factors, 3)
    return f, [_doubles(k) for k in tv_kernel_factors(who, kernel, f)]


def block_apply3d(x: torch.Tensor, factors, kernel) -> torch.Tensor:
    """``inr_tvsr3d_block_apply``: ``x`` [n, D, H, W] float64 -> ``A x`` [n, D/f0, H/f1, W/f2]; ``kernel``: (k0, k1, k2) host values."""
    _chk_volumes(x, "x")
    f, k = _block_kernel3d("block_apply3d", kernel, factors)
    n, D, H, W = x.shape
    tv_hr_sides("block_apply3d", (D, H, W), f)
    out = torch.empty((n, D // f[0], H // f[1], W // f[2]), dtype=torch.float64, device=x.device)
    check(lib().inr_tvsr3d_block_apply(out.data_ptr(), x.data_ptr(), n, D, H, W, *f, *k, _stream()), "inr_tvsr3d_block_apply")
    return out


def block_adjoint3d(r: torch.Tensor, factors, kernel) -> torch.Tensor:
    """``inr_tvsr3d_block_adjoint``: ``r`` [n, d, h, w] float64 -> ``A^T r`` [n, f0 d, f1 h, f2 w]."""
    _chk_volumes(r, "r")
    f, k = _block_kernel3d("block_adjoint3d", kernel, factors)
    n, d, h, w = r.shape
    D, H, W = d * f[0], h * f[1], w * f[2]
    tv_hr_sides("block_adjoint3d", (D, H, W), f)
    out = torch.empty((n, D, H, W), dtype=torch.float64, device=r.device)
    check(lib().inr_tvsr3d_block_adjoint(out.data_ptr(), r.data_ptr(), n, D, H, W, *f, *k, _stream()), "inr_tvsr3d_block_adjoint")
    return out


def tvsr3d_workspace_doubles(n: int, D: int, H: int, W: int, factors) -> int:
    """``inr_tvsr3d_workspace_doubles``; 0 for sizes ``inr_tvsr3d_solve`` refuses."""
    f0, f1, f2 = (int(v) for v in factors)
    return int(lib().inr_tvsr3d_workspace_doubles(int(n), int(D), int(H), int(W), f0, f1, f2))


def tvsr_solve3d(y: torch.Tensor, factors, kernel, lam: float, alpha: float, n_iter: int, grad_weights=(1.0, 1.0, 1.0), weight=None,
                 x0=None, workspace=None):
    """``inr_tvsr3d_solve`` / ``_f32`` by the dtype of ``y`` [n, d, h, w]: returns (x [n, f0 d, f1 h, f2 w] of that dtype, energy [n]
    float64, change [n] float64).  ``kernel``: (k0, k1, k2); ``grad_weights``: (g0, g1, g2) >= 0 for slice, row, column; ``weight``
    [n, d, h, w] and ``x0`` [n, f0 d, f1 h, f2 w] share the dtype; ``workspace``: a float64 tensor."""
    who = "tvsr_solve3d"
    _chk_volumes(y, "y", (torch.float32, torch.float64))
    f, k = _block_kernel3d(who, kernel, factors)
    n, d, h, w = y.shape
    D, H, W = d * f[0], h * f[1], w * f[2]
    tv_hr_sides(who, (D, H, W), f)
    lam, alpha, n_iter = _solve_scalars(who, lam, alpha, n_iter, TVSR3D_MAX_ITER)
    g = tv_grad_weights(who, grad_weights)
    return _tv_solve("inr_tvsr3d_solve", y, _chk_volumes, _chk_volumes, (D, H, W), weight, x0, workspace,
                     lambda: tvsr3d_workspace_doubles(n, D, H, W, f), (n, D, H, W, *f, *k, _doubles(g), lam, alpha, n_iter))


# ---- multi-frame TV / Huber super-resolution with sub-pixel shifts (include/inrhip.h) ----------------------------------
def _chk_frames(t, name, dtypes=(torch.float64,), shape=None) -> torch.Tensor:
    return _chk_batch(t, name, 4, "[n, frames, rows, columns]", dtypes, shape, dtype_first=True)


def _chk_shifts(shifts, n, K) -> torch.Tensor:
    """The DEVICE shifts [n, K, 2] float64, (rows, columns) in HR pixels; their values are the kernels' business."""
    if not isinstance(shifts, torch.Tensor):
        raise TypeError("shifts must be a torch.Tensor")
    if shifts.dtype != torch.float64:
        raise TypeError(f"shifts must be torch.float64 (got {shifts.dtype})")
    if not shifts.is_cuda:
        raise InrDeviceError(f"shifts is on {shifts.device}: the kernels only run on a HIP device (there is no CPU fallback)")
    if tuple(shifts.shape) != (n, K, 2) or not shifts.is_contiguous():
        raise ValueError(f"shifts must be a contiguous [{n}, {K}, 2] tensor (got {tuple(shifts.shape)})")
    return shifts


def frame_apply(x: torch.Tensor, shifts: torch.Tensor, factors, kernel, return_valid: bool = False):
    """``inr_frame_apply2d``: ``x`` [n, H, W] float64 and ``shifts`` [n, K, 2] float64 -> the frames ``A_k x`` [n, K, H/f0, W/f1], 0 at
    invalid data; ``return_valid``: also the validity mask, a bool tensor of that shape."""
    who = "frame_apply"
    _chk_images(x, "x")
    f0, f1, k = _block_kernel(who, kernel, factors)
    n, H, W = x.shape
    tv_hr_sides(who, (H, W), (f0, f1))
    if not isinstance(shifts, torch.Tensor) or shifts.dim() != 3:
        raise ValueError("frame_apply: shifts must be a [n, K, 2] tensor")
    K = int(shifts.shape[1])
    tvmf_frame_count(who, K)
    _chk_shifts(shifts, n, K)
    out = torch.empty((n, K, H // f0, W // f1), dtype=torch.float64, device=x.device)
    valid = torch.empty(out.shape, dtype=torch.uint8, device=x.device) if return_valid else None
    check(lib().inr_frame_apply2d(out.data_ptr(), _ptr(valid), x.data_ptr(), shifts.data_ptr(), n, K, H, W, f0, f1, k, _stream()),
          "inr_frame_apply2d")
    return (out, valid.bool()) if return_valid else out


def frame_adjoint(r: torch.Tensor, shifts: torch.Tensor, factors, kernel) -> torch.Tensor:
    """``inr_frame_adjoint2d``: ``r`` [n, K, h, w] float64 -> ``sum_k A_k^T r_k`` [n, f0 h, f1 w]."""
    who = "frame_adjoint"
    _chk_frames(r, "r")
    n, K, h, w = r.shape
    tvmf_frame_count(who, K)
    f0, f1, k = _block_kernel(who, kernel, factors)
    tv_hr_sides(who, (h * f0, w * f1), (f0, f1))
    _chk_shifts(shifts, n, K)
    out = torch.empty((n, h * f0, w * f1), dtype=torch.float64, device=r.device)
    check(lib().inr_frame_adjoint2d(out.data_ptr(), r.data_ptr(), shifts.data_ptr(), n, K, h * f0, w * f1, f0, f1, k, _stream()),
          "inr_frame_adjoint2d")
    return out


def tvmf_workspace_doubles(n: int, K: int, H: int, W: int, factors) -> int:
    """``inr_tvmf_workspace_doubles``; 0 for sizes ``inr_tvmf_solve2d`` refuses."""
    f0, f1 = (int(v) for v in factors)
    return int(lib().inr_tvmf_workspace_doubles(int(n), int(K), int(H), int(W), f0, f1))


def tvmf_solve(y: torch.Tensor, shifts: torch.Tensor, factors, kernel, lam: float, alpha: float, n_iter: int, weight=None, x0=None,
               workspace=None):
    """``inr_tvmf_solve2d`` / ``_f32`` by the dtype of ``y`` [n, K, h, w]: returns (x [n, f0 h, f1 w] of that dtype, energy [n],
    change [n], valid_fraction [n], all float64).  ``shifts`` [n, K, 2] float64 on the device; ``weight`` [n, K, h, w] and ``x0``
    [n, f0 h, f1 w] share the dtype of ``y``; ``workspace``: a float64 tensor."""
    who = "tvmf_solve"
    _chk_frames(y, "y", (torch.float32, torch.float64))
    n, K, h, w = y.shape
    tvmf_frame_count(who, K)
    f0, f1, k = _block_kernel(who, kernel, factors)
    H, W = h * f0, w * f1
    tv_hr_sides(who, (H, W), (f0, f1))
    _chk_shifts(shifts, n, K)
    lam, alpha, n_iter = _solve_scalars(who, lam, alpha, n_iter, TVSR3D_MAX_ITER)
    return _tv_solve("inr_tvmf_solve2d", y, _chk_frames, _chk_images, (H, W), weight, x0, workspace,
                     lambda: tvmf_workspace_doubles(n, K, H, W, (f0, f1)), (n, K, H, W, f0, f1, k, lam, alpha, n_iter), results=3,
                     after_y=(shifts.data_ptr(),))


# ---- multi-stack 3-D TV / Huber reconstruction with general slice profiles (include/inrhip.h) --------------------------
def _stack_tables(who, stacks, D, H, W):
    """``stacks``: a sequence of (f [3], taps (k0, k1, k2), o [3], n [3]) -> (S, M, the C arrays ``geometry`` int [S][12] and ``taps``, the
    per-stack shapes); refuses what the entry points would refuse."""
    tv_hr_sides(who, (D, H, W))
    stacks = list(stacks)
    tvms_stack_count(who, len(stacks))
    geo, taps, shapes = [], [], []
    for s, (f, ks, o, n) in enumerate(stacks):
        f, o, n = (tuple(int(v) for v in t) for t in (f, o, n))
        f, ks = tv_factors(f"{who}: stack {s}", f, 3), tv_kernel_factors(f"{who}: stack {s}", ks)
        o, n = tvms_offsets(f"{who}: stack {s}", o), tvms_lr_shape(f"{who}: stack {s}", n)
        taps.extend(v for k in ks for v in k)
        geo.extend(f + tuple(len(k) for k in ks) + o + n)
        shapes.append(n)
    M = sum(n[0] * n[1] * n[2] for n in shapes)
    return len(stacks), M, (C.c_int * len(geo))(*geo), _doubles(taps), shapes


def stack_apply(x: torch.Tensor, stacks, return_valid: bool = False):
    """``inr_tvms_apply``: ``x`` [n, D, H, W] float64 -> the data ``(A_s x)_s`` [n, M], 0 at invalid data; ``stacks`` as
    ``_stack_tables`` takes them; ``return_valid``: also the validity mask, a bool tensor [n, M]."""
    _chk_volumes(x, "x")
    n, D, H, W = x.shape
    S, M, geo, taps, _ = _stack_tables("stack_apply", stacks, D, H, W)
    out = torch.empty((n, M), dtype=torch.float64, device=x.device)
    valid = torch.empty(out.shape, dtype=torch.uint8, device=x.device) if return_valid else None
    check(lib().inr_tvms_apply(out.data_ptr(), _ptr(valid), x.data_ptr(), n, D, H, W, S, geo, taps, _stream()), "inr_tvms_apply")
    return (out, valid.bool()) if return_valid else out


def _chk_rows(t, name, dtypes, shape):
    """A contiguous device batch [n, M] = ``shape`` of one of ``dtypes`` (n None: any)."""
    n, M = shape
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)} (got {t.dtype})")
    if not t.is_cuda:
        raise InrDeviceError(f"{name} is on {t.device}: the kernels only run on a HIP device (there is no CPU fallback)")
    if t.dim() != 2 or not t.is_contiguous() or t.shape[1] != M or (n is not None and t.shape[0] != n):
        raise ValueError(f"{name} must be a contiguous [{'n' if n is None else n}, {M}] batch (got {tuple(t.shape)})")
    return t


def stack_adjoint(r: torch.Tensor, stacks, hr_shape) -> torch.Tensor:
    """``inr_tvms_adjoint``: ``r`` [n, M] float64 -> ``sum_s A_s^T r_s`` [n, D, H, W]."""
    D, H, W = tv_hr_shape3d("stack_adjoint", hr_shape)
    S, M, geo, taps, _ = _stack_tables("stack_adjoint", stacks, D, H, W)
    _chk_rows(r, "r", (torch.float64,), (None, M))
    n = r.shape[0]
    out = torch.empty((n, D, H, W), dtype=torch.float64, device=r.device)
    check(lib().inr_tvms_adjoint(out.data_ptr(), r.data_ptr(), n, D, H, W, S, geo, taps, _stream()), "inr_tvms_adjoint")
    return out


def tvms_workspace_doubles(n: int, D: int, H: int, W: int, stacks) -> int:
    """``inr_tvms_workspace_doubles``; 0 for sizes ``inr_tvms_solve`` refuses."""
    S, _, geo, _, _ = _stack_tables("tvms_workspace_doubles", stacks, int(D), int(H), int(W))
    return int(lib().inr_tvms_workspace_doubles(int(n), int(D), int(H), int(W), S, geo))


def tvms_solve(y: torch.Tensor, stacks, hr_shape, lam: float, alpha: float, n_iter: int, grad_weights=(1.0, 1.0, 1.0), weight=None,
               x0=None, workspace=None):
    """``inr_tvms_solve`` / ``_f32`` by the dtype of ``y`` [n, M]: returns (x [n, D, H, W] of that dtype, energy [n], change [n],
    valid_fraction [n], all float64).  ``stacks`` as ``_stack_tables`` takes them; ``weight`` [n, M] and ``x0`` [n, D, H, W] share the
    dtype of ``y``; ``workspace``: a float64 tensor."""
    who = "tvms_solve"
    D, H, W = tv_hr_shape3d(who, hr_shape)
    S, M, geo, taps, _ = _stack_tables(who, stacks, D, H, W)
    _chk_rows(y, "y", (torch.float32, torch.float64), (None, M))
    n = y.shape[0]
    lam, alpha, n_iter = _solve_scalars(who, lam, alpha, n_iter, TVSR3D_MAX_ITER)
    g = tv_grad_weights(who, grad_weights)
    return _tv_solve("inr_tvms_solve", y, _chk_rows, _chk_volumes, (D, H, W), weight, x0, workspace,
                     lambda: int(lib().inr_tvms_workspace_doubles(n, D, H, W, S, geo)),
                     (n, D, H, W, S, geo, taps, _doubles(g), lam, alpha, n_iter), results=3)


# ---- TV / Huber super-resolution under a dense separable operator (include/inrhip.h) -----------------------------------
def _chk_operators(operators, H, W, h, w):
    """The DEVICE operators (R0 [h, H], R1 [w, W]) float64, contiguous; their values are the kernels' business."""
    for name, r, shape in zip(("operators[0]", "operators[1]"), operators, ((h, H), (w, W))):
        if not isinstance(r, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if r.dtype != torch.float64:
            raise TypeError(f"{name} must be torch.float64 (got {r.dtype})")
        if not r.is_cuda:
            raise InrDeviceError(f"{name} is on {r.device}: the kernels only run on a HIP device (there is no CPU fallback)")
        if tuple(r.shape) != shape or not r.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {list(shape)} tensor (got {tuple(r.shape)})")
    return tuple(operators)


def _operator_sides(who, operators):
    """(H, W, h, w) from the shapes of the pair, each side 1 .. TVSR_MAX_SIDE."""
    (h, H), (w, W) = (tvop_operator_shape(who, f"operators[{i}]", getattr(r, "shape", ()))
                      for i, r in enumerate(tvop_operator_pair(who, operators)))
    return H, W, h, w


def tvop_workspace_doubles(n: int, H: int, W: int, h: int, w: int) -> int:
    """``inr_tvop_workspace_doubles``; 0 for sizes ``inr_tvop_solve2d`` refuses."""
    return int(lib().inr_tvop_workspace_doubles(int(n), int(H), int(W), int(h), int(w)))


def tvop_apply(x: torch.Tensor, operators, workspace=None) -> torch.Tensor:
    """``inr_tvop_apply``: ``x`` [n, H, W] float64 -> ``A x = R0 x R1^T`` [n, h, w]; ``operators`` = (R0 [h, H], R1 [w, W]), device
    float64; ``workspace``: a float64 tensor of ``tvop_workspace_doubles(n, H, W, h, w)``."""
    _chk_images(x, "x")
    H, W, h, w = _operator_sides("tvop_apply", operators)
    n = x.shape[0]
    if tuple(x.shape[1:]) != (H, W):
        raise ValueError(f"x has shape {tuple(x.shape)}, expected {(n, H, W)}")
    r0, r1 = _chk_operators(operators, H, W, h, w)
    out = torch.empty((n, h, w), dtype=torch.float64, device=x.device)
    if n == 0:
        return out
    workspace = _f64_workspace(workspace, tvop_workspace_doubles(n, H, W, h, w), x.device)
    check(lib().inr_tvop_apply(out.data_ptr(), x.data_ptr(), r0.data_ptr(), r1.data_ptr(), n, H, W, h, w, workspace.data_ptr(),
                               workspace.numel(), _stream()), "inr_tvop_apply")
    return out


def tvop_adjoint(r: torch.Tensor, operators, workspace=None) -> torch.Tensor:
    """``inr_tvop_adjoint``: ``r`` [n, h, w] float64 -> ``A^T r = R0^T r R1`` [n, H, W]; arguments as ``tvop_apply``."""
    _chk_images(r, "r")
    H, W, h, w = _operator_sides("tvop_adjoint", operators)
    n = r.shape[0]
    if tuple(r.shape[1:]) != (h, w):
        raise ValueError(f"r has shape {tuple(r.shape)}, expected {(n, h, w)}")
    r0, r1 = _chk_operators(operators, H, W, h, w)
    out = torch.empty((n, H, W), dtype=torch.float64, device=r.device)
    if n == 0:
        return out
    workspace = _f64_workspace(workspace, tvop_workspace_doubles(n, H, W, h, w), r.device)
    check(lib().inr_tvop_adjoint(out.data_ptr(), r.data_ptr(), r0.data_ptr(), r1.data_ptr(), n, H, W, h, w, workspace.data_ptr(),
                                 workspace.numel(), _stream()), "inr_tvop_adjoint")
    return out


def tvop_solve(y: torch.Tensor, operators, lam: float, alpha: float, n_iter: int, weight=None, x0=None, workspace=None):
    """``inr_tvop_solve2d`` / ``_f32`` by the dtype of ``y`` [n, h, w]: returns (x [n, H, W] of that dtype, energy [n] float64, change
    [n] float64).  ``operators`` = (R0 [h, H], R1 [w, W]), device float64, shared by the batch; ``weight`` [n, h, w] and ``x0``
    [n, H, W] share the dtype of ``y``; ``workspace``: a float64 tensor."""
    who = "tvop_solve"
    _chk_images(y, "y", (torch.float32, torch.float64))
    H, W, h, w = _operator_sides(who, operators)
    n = y.shape[0]
    if tuple(y.shape[1:]) != (h, w):
        raise ValueError(f"y has shape {tuple(y.shape)}, expected {(n, h, w)}")
    r0, r1 = _chk_operators(operators, H, W, h, w)
    lam, alpha, n_iter = _solve_scalars(who, lam, alpha, n_iter, TVSR3D_MAX_ITER)
    return _tv_solve("inr_tvop_solve2d", y, _chk_images, _chk_images, (H, W), weight, x0, workspace,
                     lambda: tvop_workspace_doubles(n, H, W, h, w), (r0.data_ptr(), r1.data_ptr(), n, H, W, h, w, lam, alpha, n_iter))


# ---- diagnostics ------------------------------------------------------------------------------------------
LAUNCH_FAMILIES = ("hp_pkd", "hp_pkc", "hp_tile", "hp_rc", "h3", "f32_pipe16", "f32_pipe", "f32_generic", "small_multi",
                   "small_step", "hp_narrow", "hp_fused_fwd", "hp_row", "small_batch")   # INR_LF_* of include/inrhip.h, in order
PIA_LAUNCH_FAMILIES = ("pia_fwd", "pia_dx", "pia_dw", "pia_head")                        # INR_PIA_LF_*, numbered from 0
JET_LAUNCH_FAMILIES = ("jet_input", "jet_layer", "jet_head")                             # INR_JET_LF_*, numbered from 0


def _family_counts(entry: str, names) -> dict:
    out = {}
    for i, name in enumerate(names):
        n = C.c_int64(0)
        check(getattr(lib(), entry)(i, C.byref(n)), entry)
        out[name] = int(n.value)
    return out


def launch_counts() -> dict:
    """Launches each kernel family has received since the last ``launch_counts_reset()`` (process-global)."""
    return _family_counts("inr_launch_count", LAUNCH_FAMILIES)


def pia_launch_counts() -> dict:
    """Launches each PIA kernel family has received since the last ``launch_counts_reset()``."""
    return _family_counts("inr_pia_launch_count", PIA_LAUNCH_FAMILIES)


def jet_launch_counts() -> dict:
    """Launches each derivative-kernel family has received since the last ``launch_counts_reset()``."""
    return _family_counts("inr_jet_launch_count", JET_LAUNCH_FAMILIES)


def launch_counts_reset():
    check(lib().inr_launch_counts_reset())


def debug_get(key: int) -> int:
    v = C.c_int(0)
    check(lib().inr_debug_get(int(key), C.byref(v)), "inr_debug_get")
    return int(v.value)


class debug_switch:
    """``with debug_switch(key, value): ...`` -- a diagnostic switch (process-global, include/inrhip.h) set for the block
    and put back to what it was, also when the block raises."""

    def __init__(self, key: int, value: int):
        self.key, self.value = int(key), int(value)

    def __enter__(self):
        self.old = debug_get(self.key)
        check(lib().inr_debug_set(self.key, self.value), "inr_debug_set")
        return self

    def __exit__(self, *exc):
        check(lib().inr_debug_set(self.key, self.old), "inr_debug_set")
        return False


# ---- measurement hooks ------------------------------------------------------------------------------------
def prof_enable(on: bool):
    check(lib().inr_prof_enable(1 if on else 0))


def prof_reset():
    check(lib().inr_prof_reset())


def prof_read(kernel_class: int):
    n = C.c_int64(0)
    ms = C.c_double(0.0)
    check(lib().inr_prof_read(int(kernel_class), C.byref(n), C.byref(ms)), "inr_prof_read")
    return int(n.value), float(ms.value)


def sincos_probe(x):
    _chk(x, "x")
    s = torch.empty_like(x)
    c = torch.empty_like(x)
    check(lib().inr_sincos_probe(s.data_ptr(), c.data_ptr(), x.data_ptr(), x.numel(), _stream()))
    return s, c
