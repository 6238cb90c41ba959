"""The WIRE complex-Gabor INR of the reference on the device: ``ComplexGaborLayer2D`` (INRmodel.py:66-120) and the network
``wiretest.ipynb`` cell 2 stacks from it.

Layer 0 holds two real ``Linear(in, H)`` (``linear``, ``scale_orth``), the hidden layers two complex ``Linear(H, H)`` each, the
head is a complex ``Linear(H, 1)`` whose real part is the output.  With ``lin = linear(h)``, ``orth = scale_orth(h)`` a layer
gives ``exp(1j * omega_0 * lin) * exp(-scale_0**2 * (|lin|**2 + |orth|**2))``; the kernels of ``csrc/wire.hip`` evaluate it
in real arithmetic.  Constructor signatures, RNG draw order, parameter names and ``state_dict()`` keys are the
reference's; initialisation is ``nn.Linear``'s default (the reference defines an ``init_weights`` it never calls).

``forward`` runs the inference kernels and carries no parameter gradients: training goes through ``WireFitter``, which makes the
parameters live views of one flat fp32 buffer (a complex tensor is its interleaved ``(re, im)`` pairs) and runs forward, MSE,
backward and Adam of many steps in one C call.  An input that requires grad gets the gradient with respect to ITSELF
(``inr_wire_forward_stash`` / ``inr_wire_input_grad``): the notebook's network does not detach its input (cell 2), and cell
10's PerturbNet phase -- ``drivers.fit_wire_with_perturbnet`` -- trains the PerturbNet through it.  There is no CPU path and
no layer-by-layer fallback.  ``derivatives`` gives value, coordinate gradient and Laplacian of a fitted network in forward mode
(``csrc/wire_deriv.hip``; nn_mri.py:205-221 over this stack), and ``inr.laplace`` serves a direct ``Wire`` output through it.
Served: ``out_features == 1``, ``hidden_features in {32, 64, 128, 256}``, ``hidden_layers <= 8``,
``in_features <= 1024``, ``trainable=False``; anything else raises.
"""
from __future__ import annotations

import ctypes as C
import weakref

import torch
from torch import nn

from . import ops
from ._lib import WireDesc, check, lib, shape_array
from .inr import _derivatives
from .flat import AdamOwner, AdamState, FlatParams, Workspace, WorkspacePool

HIDDEN_SIZES = (32, 64, 128, 256)
MAX_HIDDEN_LAYERS = 8
MAX_IN_FEATURES = 1024


def _check_shape(in_features, hidden_features, hidden_layers, out_features):
    if out_features != 1 or hidden_features not in HIDDEN_SIZES or not 0 <= hidden_layers <= MAX_HIDDEN_LAYERS or \
            not 1 <= in_features <= MAX_IN_FEATURES:
        raise ValueError("Wire: the complex-Gabor kernels serve out_features == 1, hidden_features in {32, 64, 128, 256}, "
                         f"hidden_layers <= 8, in_features <= 1024 (got in={in_features}, hidden={hidden_features}, "
                         f"layers={hidden_layers}, out={out_features}); there is no other path")


def _planes(x):
    """complex [n, H] -> float planes [n, 2H] = [re | im]"""
    return torch.cat([x.real, x.imag], dim=-1).contiguous()


class ComplexGaborLayer2D(nn.Module):
    """INRmodel.py:66-120.  ``omega_0`` / ``scale_0`` are float32 ``nn.Parameter``s of shape [1] that need no gradient (they
    are part of ``state_dict()`` and ``parameters()``); ``trainable=True`` is not served.  ``forward`` runs the layer kernel on
    tensors that need no gradient -- real ``[..., in]`` for a first layer, complex ``[..., H]`` otherwise (then
    ``in_features == out_features``) -- and returns a complex tensor; an input that requires grad raises: training goes through
    ``WireFitter``."""

    def __init__(self, in_features, out_features, bias=True, is_first=False, omega0=10.0, sigma0=10.0, trainable=False):
        super().__init__()
        if trainable:
            raise ValueError("ComplexGaborLayer2D: trainable omega_0 / scale_0 are not served (the reference never uses them)")
        if not bias:
            raise ValueError("ComplexGaborLayer2D: the kernels serve bias=True only")
        self.is_first = is_first
        self.in_features = in_features
        dtype = torch.float if is_first else torch.cfloat
        self.omega_0 = nn.Parameter(omega0 * torch.ones(1), False)
        self.scale_0 = nn.Parameter(sigma0 * torch.ones(1), False)
        self.linear = nn.Linear(in_features, out_features, bias=bias, dtype=dtype)
        self.scale_orth = nn.Linear(in_features, out_features, bias=bias, dtype=dtype)

    def kernel_parameters(self):
        return [self.linear.weight, self.linear.bias, self.scale_orth.weight, self.scale_orth.bias]

    def forward(self, input):
        if input.requires_grad:
            raise RuntimeError("ComplexGaborLayer2D.forward carries no autograd graph: train the network with WireFitter "
                               "(wire.fit_wire), or detach the input")
        ops.require_gpu()
        H, fin = self.linear.out_features, self.in_features
        if H not in HIDDEN_SIZES or not 1 <= fin <= MAX_IN_FEATURES or (not self.is_first and fin != H):
            raise ValueError(f"ComplexGaborLayer2D: the kernels serve out_features in {HIDDEN_SIZES}, in_features <= 1024 and "
                             f"square complex layers (got {fin} -> {H}, is_first={self.is_first})")
        if input.shape[-1] != fin or input.is_complex() == bool(self.is_first):
            raise ValueError(f"input must be {'real' if self.is_first else 'complex'} [..., {fin}], got {input.dtype} "
                             f"{tuple(input.shape)}")
        rows = input.detach().reshape(-1, fin)
        x = ops._chk(rows.contiguous() if self.is_first else _planes(rows), "input")
        if self.linear.weight.device != x.device:
            raise ops.InrDeviceError("ComplexGaborLayer2D: move the layer to the input's HIP device first (.cuda())")
        n = x.shape[0]
        tensors = [torch.view_as_real(p.detach()).contiguous() if p.is_complex() else p.detach().contiguous()
                   for p in self.kernel_parameters()]
        consts = torch.cat([self.omega_0.detach(), self.scale_0.detach()]).cpu()
        out = torch.empty((n, 2 * H), dtype=torch.float32, device=x.device)
        if n:
            need = lib().inr_wire_layer_workspace_bytes(n, x.shape[1], H)
            ws = ops._ws(need, x.device)
            check(lib().inr_wire_layer_forward(out.data_ptr(), x.data_ptr(), *[t.data_ptr() for t in tensors], n, fin, H,
                                               int(bool(self.is_first)), float(consts[0]), float(consts[1]), ws.data_ptr(),
                                               ws.numel(), ops._stream()), "inr_wire_layer_forward")
        return torch.complex(out[:, :H], out[:, H:]).reshape(*input.shape[:-1], H)


def wire_param_layout(desc):
    """(total floats, offsets in kernel order: per layer linear.weight, linear.bias, scale_orth.weight, scale_orth.bias, then
    the head's weight and bias)."""
    return ops.param_layout(lib().inr_wire_param_count, lib().inr_wire_param_offsets, desc, 4 * (desc.hidden_layers + 1) + 2)


WS_INFER, WS_TRAIN, WS_INPUT_GRAD = 0, 1, 2      # inr_wire_workspace_bytes' third argument (include/inrhip.h)


class _WireInputFn(torch.autograd.Function):
    """``y = Wire(x)`` differentiated with respect to ``x`` ONLY: the forward is ``inr_wire_forward_stash`` (the kernels and bits
    of ``inr_wire_forward``, with the stash kept), the backward ``inr_wire_input_grad``.  The parameters are not inputs of this
    function, so their ``.grad`` stay untouched.  The stash workspace is held from the forward to its ONE backward, which
    consumes it and hands the buffer back to ``pool``."""

    @staticmethod
    def forward(ctx, x, desc, flat, pool):
        n = x.shape[0]
        need = lib().inr_wire_workspace_bytes(C.byref(desc), n, WS_INPUT_GRAD)
        if need == 0:
            check(-1, "inr_wire_workspace_bytes")
        ws, _ = pool.take(need, x.device)
        y = torch.empty(n, dtype=torch.float32, device=x.device)
        check(lib().inr_wire_forward_stash(C.byref(desc), flat.data_ptr(), x.data_ptr(), n, y.data_ptr(), ws.data_ptr(), ws.numel(),
                                           ops._stream()), "inr_wire_forward_stash")
        ctx.desc, ctx.flat, ctx.pool, ctx.ws, ctx.shape = desc, flat, pool, ws, tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        if ctx.ws is None:
            raise RuntimeError("Wire's input gradient runs ONE backward per forward (its stash workspace went back to the pool after "
                               "the first): call the model again for a second backward")
        n, fin = ctx.shape
        gy = ops._chk(gy.contiguous(), "grad_output")
        dx = torch.empty((n, fin), dtype=torch.float32, device=gy.device)
        check(lib().inr_wire_input_grad(C.byref(ctx.desc), ctx.flat.data_ptr(), gy.data_ptr(), n, dx.data_ptr(), ctx.ws.data_ptr(),
                                        ctx.ws.numel(), ops._stream()), "inr_wire_input_grad")
        ctx.pool.give_back(ctx.ws)
        ctx.ws = None
        return dx, None, None, None


class Wire(nn.Module):
    """The network of wiretest.ipynb cell 2 (there named ``Siren``): ``ComplexGaborLayer2D(in, H, is_first=True)``,
    ``hidden_layers`` complex layers, a complex ``final_linear``; ``forward`` returns the real part, ``[..., 1]``.  ``scale`` is
    every layer's ``sigma0``.  ``final_linear`` is registered before ``net`` and is also ``net``'s last module, as in the
    notebook, so ``state_dict()`` lists the head under both names.

    ``forward`` on an input that requires grad is differentiable with respect to that INPUT only (cell 2 does not detach it; the
    gradient flows on into ``input_mapping`` and the PerturbNet): same kernels, same output bits, ONE backward per forward -- a
    second raises.  The parameters never receive a ``.grad`` from it; they are trained by ``WireFitter``."""

    def __init__(self, in_features, hidden_features, hidden_layers, out_features, first_omega_0=10, hidden_omega_0=30.,
                 scale=10.0):
        super().__init__()
        _check_shape(in_features, hidden_features, hidden_layers, out_features)
        self.in_features, self.hidden_features, self.hidden_layers = in_features, hidden_features, hidden_layers
        self.out_features = out_features
        self._input_grad_pool = WorkspacePool()      # the stash workspace of a forward whose input requires grad, until its backward
        net = [ComplexGaborLayer2D(in_features, hidden_features, omega0=first_omega_0, sigma0=scale, is_first=True,
                                   trainable=False)]
        for _ in range(hidden_layers):
            net.append(ComplexGaborLayer2D(hidden_features, hidden_features, is_first=False, omega0=hidden_omega_0, sigma0=scale))
        self.final_linear = nn.Linear(hidden_features, out_features, dtype=torch.cfloat)
        net.append(self.final_linear)
        self.net = nn.Sequential(*net)

    def kernel_parameters(self):
        """Parameters in the order of the kernels' flat buffer (``omega_0`` / ``scale_0`` are not in it)."""
        out = []
        for k in range(self.hidden_layers + 1):
            out += self.net[k].kernel_parameters()
        return out + [self.final_linear.weight, self.final_linear.bias]

    def desc(self):
        """The kernels' descriptor from the parameters' CURRENT values (one device read).  Hidden layers whose ``omega_0`` /
        ``scale_0`` differ among themselves raise: the descriptor has one pair for all of them."""
        consts = torch.stack([torch.cat([self.net[k].omega_0.detach(), self.net[k].scale_0.detach()])
                              for k in range(self.hidden_layers + 1)]).cpu()
        hidden = consts[1:] if self.hidden_layers else consts[:1]
        if not bool((hidden == hidden[0]).all()):
            raise ValueError("Wire: the hidden layers' omega_0 / scale_0 differ among themselves; the kernels take one pair")
        return WireDesc(self.in_features, self.hidden_features, self.hidden_layers, 1, float(consts[0, 0]), float(hidden[0, 0]),
                        float(consts[0, 1]), float(hidden[0, 1]))

    def _flat(self, desc):
        """The flat buffer the kernels read: the fitter's live one when the parameters are its views, else a packed copy."""
        fitter = getattr(self, "_fitter", None)
        if fitter is not None and fitter.owns(self):
            return fitter.flat
        params = self.kernel_parameters()
        if not params[0].is_cuda:
            raise ops.InrDeviceError("Wire: move the model to the HIP device first (model.cuda())")
        total, offsets = wire_param_layout(desc)
        return FlatParams(total, offsets).pack(params)

    def forward(self, coords):
        ops.require_gpu()
        wants_grad = coords.requires_grad and torch.is_grad_enabled()
        x = coords if wants_grad else coords.detach()
        x = ops._chk(x.reshape(-1, coords.shape[-1]).contiguous(), "coords")
        if x.shape[1] != self.in_features:
            raise ValueError(f"coords must be [..., {self.in_features}], got {tuple(coords.shape)}")
        desc = self.desc()
        flat = self._flat(desc)
        if flat.device != x.device:
            raise ops.InrDeviceError("Wire: move the model to the input's HIP device first (model.cuda())")
        n = x.shape[0]
        if wants_grad and n:
            y = _WireInputFn.apply(x, desc, flat, self._input_grad_pool)
        else:
            y = torch.empty(n, dtype=torch.float32, device=x.device)
            if n:
                need = lib().inr_wire_workspace_bytes(C.byref(desc), n, WS_INFER)
                if need == 0:
                    check(-1, "inr_wire_workspace_bytes")
                ws = ops._ws(need, x.device)
                check(lib().inr_wire_forward(C.byref(desc), flat.data_ptr(), x.data_ptr(), n, y.data_ptr(), ws.data_ptr(),
                                             ws.numel(), ops._stream()), "inr_wire_forward")
        y = y.reshape(*coords.shape[:-1], 1)
        if coords.requires_grad and coords.shape[-1] <= 4:
            # where this output came from, for `inr.laplace`: the backward of _WireInputFn is a plain kernel call and leaves no
            # graph to differentiate a second time (as Siren.forward does)
            y._wire_origin = (weakref.ref(self), coords)
        return y


class WireFitter(AdamOwner):
    """wiretest.ipynb cell 10's plain branch (forward, ``((y - t)**2).mean()``, backward, ``torch.optim.Adam(lr=5e-5).step()``)
    as ``inr_wire_fit``: ``n_steps`` steps per call, no host read.  The model's weights become views of one flat fp32 buffer
    (complex tensors through ``torch.view_as_complex``), so ``state_dict()`` keeps seeing live values; Adam state lives here,
    which lets a fit be continued.  Adam treats a complex parameter as its two reals, as torch does; the head bias's
    imaginary part has zero gradient and never moves."""

    def __init__(self, model: Wire, lr=5e-5, betas=(0.9, 0.999), eps=1e-8):
        ops.require_gpu()
        self.model = model
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.desc = model.desc()
        self.total, self.offsets = wire_param_layout(self.desc)
        self.params = FlatParams(self.total, self.offsets)
        self._workspace = Workspace()
        self._adopt()
        self.adam = AdamState(self.flat)

    @property
    def flat(self):
        return self.params.flat

    def _adopt(self):
        params = self.model.kernel_parameters()
        if not params[0].is_cuda:
            raise ops.InrDeviceError("move the model to the HIP device first (model.cuda())")
        self.params.adopt(params)
        self.desc = self.model.desc()
        self.model._fitter = self

    def owns(self, model):
        return model is self.model and self.params.owns(model.kernel_parameters())

    def _ws(self, n):
        need = lib().inr_wire_workspace_bytes(C.byref(self.desc), int(n), 1)
        if need == 0:
            check(-1, "inr_wire_workspace_bytes")
        return self._workspace.grow(need, self.flat.device)

    def _inputs(self, model_input, target, weight):
        if not self.owns(self.model):
            self._adopt()                             # moved / reloaded: re-flatten (Adam state and step count are kept)
        x = ops._chk(model_input.detach().reshape(-1, model_input.shape[-1]).contiguous(), "model_input")
        t = ops._chk(target.detach().reshape(-1).contiguous(), "target")
        w = None if weight is None else ops._chk(weight.detach().reshape(-1).contiguous(), "weight")
        if x.shape[1] != self.model.in_features or x.shape[0] == 0 or t.numel() != x.shape[0] or \
                (w is not None and w.numel() != x.shape[0]):
            raise ValueError(f"model_input must be [n >= 1, {self.model.in_features}] with n target (and weight) values")
        return x, t, w

    def step(self, model_input, target, n_steps=1, weight=None):
        """Run ``n_steps`` fit steps; returns the per-step losses (before each update) as a device tensor, no sync."""
        x, t, w = self._inputs(model_input, target, weight)
        n_steps = int(n_steps)
        losses = torch.empty(max(n_steps, 1), dtype=torch.float32, device=x.device)
        ws = self._ws(x.shape[0])
        check(lib().inr_wire_fit(C.byref(self.desc), self.flat.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(),
                                 self.v.data_ptr(), x.data_ptr(), t.data_ptr(), ops._ptr(w), x.shape[0], self.step_count + 1,
                                 n_steps, self.lr, self.betas[0], self.betas[1], self.eps, losses.data_ptr(), ws.data_ptr(),
                                 ws.numel(), ops._stream()), "inr_wire_fit")
        self.step_count += n_steps
        return losses[:n_steps]

    def loss_grad(self, model_input, target, weight=None):
        """``(loss [1], flat gradient)`` of ``mean(w (f(x) - t)**2)``; the gradient is ``self.grads`` (``split`` carves it)."""
        x, t, w = self._inputs(model_input, target, weight)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        ws = self._ws(x.shape[0])
        check(lib().inr_wire_loss_grad(C.byref(self.desc), self.flat.data_ptr(), self.grads.data_ptr(), x.data_ptr(), t.data_ptr(),
                                       ops._ptr(w), x.shape[0], loss.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()),
              "inr_wire_loss_grad")
        return loss, self.grads

    def split(self, flat):
        """Views of a flat vector per tensor, in ``kernel_parameters()`` order (complex where the parameter is)."""
        return self.params.split(flat)

    def release_workspace(self):
        self._workspace.release()


def fit_wire(model: Wire, model_input, target, steps, lr=5e-5, weight=None, chunk=250, fitter=None):
    """A full fit in chunks of ``chunk`` steps, in the shape of ``inr.fit_siren``.  Returns (fitter, losses tensor)."""
    fitter = fitter or WireFitter(model, lr=lr)
    out, done = [], 0
    while done < steps:
        k = min(chunk, steps - done)
        out.append(fitter.step(model_input, target, k, weight))
        done += k
    return fitter, (torch.cat(out) if out else torch.empty(0))


def reconstruct(model: Wire, shape, B=None, clamp_min=0.0, chunk_rows=1 << 16):
    """``clamp(INR(input_mapping(get_mgrid(shape), B)), min=0).view(shape)`` (wiretest.ipynb cells 9-10) as one C call; grid
    and Fourier features are produced chunk by chunk on the device.  ``B=None`` feeds the raw coordinates;
    ``clamp_min=None`` skips the clamp.  Bit-identical to ``model(input_mapping(get_mgrid(shape), B))`` whatever the chunk."""
    dev = ops.require_gpu()
    desc = model.desc()
    flat = model._flat(desc)
    shape = tuple(int(s) for s in shape)
    total = 1
    for s in shape:
        total *= s
    Bd = None if B is None else ops._chk(B.detach().to(flat.device, torch.float32).contiguous(), "B")
    if Bd is not None and (Bd.dim() != 2 or Bd.shape[1] != len(shape)):
        raise ValueError(f"B must be [m, {len(shape)}], got {tuple(Bd.shape)}")
    chunk = max(1, min(int(chunk_rows), total))
    need = lib().inr_wire_reconstruct_workspace_bytes(C.byref(desc), chunk)
    if need == 0:
        check(-1, "inr_wire_reconstruct_workspace_bytes")
    ws = ops._ws(need, dev)
    y = torch.empty(total, dtype=torch.float32, device=flat.device)
    check(lib().inr_wire_reconstruct(C.byref(desc), flat.data_ptr(), shape_array(shape), len(shape), ops._ptr(Bd),
                                     0 if Bd is None else Bd.shape[0], y.data_ptr(), int(clamp_min is not None),
                                     float(clamp_min or 0.0), chunk, ws.data_ptr(), ws.numel(), ops._stream()), "inr_wire_reconstruct")
    return y.view(*shape)


def derivatives(model: Wire, coords=None, *, shape=None, B=None, laplacian=True, d_tangent=None, chunk_rows=1 << 15):
    """Value, coordinate gradient and Laplacian of ``model(input_mapping(coords, B))``, evaluated in forward mode by the
    ``inr_wire_derivatives`` kernels: what nn_mri.py:205-221 ``gradient`` / ``laplace`` obtain from two ``autograd.grad`` passes
    with ``create_graph=True`` over the notebook's network (cell 2 does not detach its input), without a stash of activations,
    so it runs on a re-sampling grid of millions of rows.  The WIRE counterpart of ``inr.derivatives``, with its shapes and units:

    exactly one of ``coords`` ([..., d] rows, d <= 4) and ``shape`` (the dense grid ``get_mgrid(shape)``, generated on the
    device) is given.  Returns ``inr.Derivatives(value, gradient, laplacian)`` of device tensors: for ``coords`` of shape
    ``lead + (d,)`` they have shapes ``lead``, ``lead + (d_tangent,)``, ``lead``; on a grid ``shape``, ``shape + (d_tangent,)``,
    ``shape``.  ``laplacian=False`` skips the second-order accumulator (the field is ``None``).  ``d_tangent`` (default d)
    differentiates along the leading axes only: a DWI grid (x, y, z, b) takes 3, and the Laplacian then sums over those axes.
    ``B=None`` feeds the raw coordinates (``in_features == d``); otherwise ``in_features == 2 * len(B)``.

    Derivatives are with respect to the NORMALISED ``[-1, 1]`` coordinates of ``get_mgrid``: multiply ``gradient[..., a]`` by
    ``2 / (n_a - 1)`` for units per voxel along an axis of ``n_a`` samples, a second derivative by its square.  The value is the
    raw network output (no clamp); it agrees with ``model(...)`` to rounding, not bit for bit (another tile shape).  The results
    carry no graph."""
    def desc_and_flat():
        ops.require_gpu()
        desc = model.desc()
        return desc, model._flat(desc)

    return _derivatives(ops.wire_derivatives, desc_and_flat, coords, shape, B, laplacian, d_tangent, chunk_rows)
