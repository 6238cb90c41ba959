"""The PIA physics-informed autoencoder on the device (the class half of the reference's PIA.py).

Mirrors ``PIA`` (PIA.py:16-155), ``get_batch`` (PIA.py:171-213), ``detect_PIDS_slice`` (PIA.py:286-327) and ``ADC_slice``
(PIA.py:157-169): same constructor signature and defaults, same submodule layout (so ``state_dict()`` keys and the initial
weights drawn after ``torch.manual_seed`` are the reference's), same return dtypes (``D`` float64; ``T2``, ``v``, ``signal``
float32).  ``forward`` runs on the HIP kernels of ``csrc/pia.hip`` -- ``inr_pia_forward_train`` /
``inr_pia_backward_train`` under autograd, ``inr_pia_forward`` otherwise; ``PiaFitter.step`` is the fused step
``inr_pia_fit_step``.  There is no CPU path: without a HIP device ``forward`` raises ``InrDeviceError``.

The kernels serve the shapes of ``inr_pia_desc_t`` (include/inrhip.h): 16 signals, widths that are multiples of 16, a last
width of 256 or 512, ``predictor_depth == 1``, and integer ``T2_mean`` / ``T2_delta`` (the reference's ``T2`` is float32
because those two are int64 tensors; float tables would make it float64 there, which the kernels do not reproduce).
"""
from __future__ import annotations

import ctypes as C
from typing import List

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import ops
from ._lib import PiaDesc, check, lib
from .flat import AdamOwner, AdamState, FlatParams, Workspace, WorkspacePool


def _as_desc(model) -> PiaDesc:
    d = PiaDesc()
    d.n_signals = int(model.number_of_signals)
    d.n_hidden = len(model.hidden_dims)
    for i, h in enumerate(model.hidden_dims[:8]):
        d.hidden[i] = int(h)
    d.predictor_depth = int(model.predictor_depth)
    d.n_b, d.n_te = len(model.b_values), len(model.TE_values)
    d.leaky_slope = 0.01
    for i, b in enumerate(model.b_values[:8]):
        d.b_values[i] = float(b)
    for i, t in enumerate(model.TE_values[:8]):
        d.te_values[i] = float(t)
    for name in ("D_mean", "D_delta", "T2_mean", "T2_delta"):
        t = getattr(model, name)
        # the reference's output dtypes follow these tables: float64 D tables make D float64, integer T2 tables leave T2 float32
        if name.startswith("D") and t.dtype != torch.float64:
            raise ValueError(f"{name} must be a float64 table (got {t.dtype}): the kernels return D in float64, as the reference "
                             "does for float tables")
        if name.startswith("T2") and (t.dtype.is_floating_point or t.dtype.is_complex):
            raise ValueError(f"{name} must be an integer table (got {t.dtype}): with float tables the reference's T2 is float64, "
                             "which the kernels do not reproduce")
        vals = t.detach().cpu().numpy().astype(np.float64).reshape(-1)
        if vals.size != 3:
            raise ValueError(f"{name} must have three entries")
        for c in range(3):
            getattr(d, name)[c] = float(vals[c])
    return d


def pia_param_layout(desc: PiaDesc):
    """(total, offsets) of the flat parameter buffer: the tensors of ``named_parameters()`` back to back, unpadded."""
    return ops.param_layout(lib().inr_pia_param_count, lib().inr_pia_param_offsets, desc,
                            2 * desc.n_hidden + 3 * (2 * desc.predictor_depth + 2))


class _PiaState:
    """The flat parameter buffer the module's parameters are views of, and the stash workspace of a pending forward."""

    def __init__(self, model):
        self.model = model
        self.desc = None
        self.params = FlatParams(0, [])               # owns nothing: the first ensure() replaces it
        self.pool = WorkspacePool()

    @property
    def flat(self):
        return self.params.flat

    def ensure(self):
        params = list(self.model.parameters())
        if self.params.owns(params):
            return
        self.desc = _as_desc(self.model)              # re-adoption reads the model's tables again
        total, self.offsets = pia_param_layout(self.desc)
        assert len(self.offsets) == len(params) and total == sum(p.numel() for p in params)
        self.params = FlatParams(total, self.offsets)
        self.params.adopt(params, zero=False)         # (the layout has no padding)

    def split(self, flat):
        return self.params.split(flat)

    def workspace(self, n, training, device):
        need = lib().inr_pia_workspace_bytes(C.byref(self.desc), int(n), int(training))
        if need == 0:
            check(-1, "inr_pia_workspace_bytes")
        return self.pool.take(need, device)[0]

    def give_back(self, ws):
        self.pool.give_back(ws)


def _outputs(n, dev):
    return (torch.empty((n, 16), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float64, device=dev),
            torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev))


class _PiaFn(torch.autograd.Function):
    """``model(x)`` under autograd: one call enqueues the forward with its stash, one the whole backward."""

    @staticmethod
    def forward(ctx, state, x, *params):
        n = x.shape[0]
        ws = state.workspace(n, True, x.device)
        signal, D, T2, v = _outputs(n, x.device)
        check(lib().inr_pia_forward_train(C.byref(state.desc), state.flat.data_ptr(), x.data_ptr(), n, signal.data_ptr(),
                                          D.data_ptr(), T2.data_ptr(), v.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()),
              "inr_pia_forward_train")
        ctx.state, ctx.ws = state, ws
        ctx.params, ctx.versions = params, [state.flat._version] + [p._version for p in params]
        ctx.save_for_backward(x)             # autograd then refuses an x changed in place before backward
        ctx.set_materialize_grads(False)
        return signal, D, T2, v

    @staticmethod
    def backward(ctx, g_signal, g_D, g_T2, g_v):
        state, ws = ctx.state, ctx.ws
        if ws is None:
            raise RuntimeError("PIA: backward through the same forward twice (the stash is handed over once)")
        (x,) = ctx.saved_tensors
        if [state.flat._version] + [p._version for p in ctx.params] != ctx.versions:
            raise RuntimeError("PIA: a parameter was modified in place between forward and backward (the backward kernels read "
                               "the weights the forward ran on)")
        gs = [None if g is None else g.to(dt).contiguous()
              for g, dt in ((g_signal, torch.float32), (g_D, torch.float64), (g_T2, torch.float32), (g_v, torch.float32))]
        grads = torch.empty_like(state.flat)
        check(lib().inr_pia_backward_train(C.byref(state.desc), state.flat.data_ptr(), grads.data_ptr(), x.data_ptr(),
                                           ops._ptr(gs[0]), ops._ptr(gs[1]), ops._ptr(gs[2]), ops._ptr(gs[3]), x.shape[0],
                                           ws.data_ptr(), ws.numel(), ops._stream()), "inr_pia_backward_train")
        ctx.ws = None
        state.give_back(ws)
        return (None, None, *state.split(grads))


class PIA(nn.Module):
    """PIA.py:16-155.  Same constructor, submodules, methods and return values as the reference class."""

    def __init__(self, number_of_signals=16, D_mean=[0.5, 1.2, 2.85], T2_mean=[45, 70, 750], D_delta=[0.2, 0.5, 0.15],
                 T2_delta=[25, 30, 250], b_values=[0, 150, 1000, 1500], TE_values=[0, 13, 93, 143],
                 hidden_dims: List = None, predictor_depth=1):
        super().__init__()
        device = "cuda" if torch.cuda.is_available() else "cpu"
        if hidden_dims is None:
            hidden_dims = [32, 64, 128, 256, 512]
        self.number_of_signals = number_of_signals
        self.number_of_compartments = 3
        self.hidden_dims = list(hidden_dims)
        self.predictor_depth = predictor_depth
        self.D_mean = torch.from_numpy(np.asarray(D_mean)).to(device)
        self.T2_mean = torch.from_numpy(np.asarray(T2_mean)).to(device)
        self.D_delta = torch.from_numpy(np.asarray(D_delta)).to(device)
        self.T2_delta = torch.from_numpy(np.asarray(T2_delta)).to(device)
        self.b_values = b_values
        self.TE_values = TE_values
        self.softmax = torch.nn.Softmax(dim=1)
        self.relu = nn.ReLU()

        # nn.Linear creation order is the reference's, so the same torch seed draws the same weights
        modules, in_channels = [], number_of_signals
        for h_dim in hidden_dims:
            modules.append(nn.Sequential(nn.Linear(in_channels, h_dim), nn.LeakyReLU()))
            in_channels = h_dim
        self.encoder = nn.Sequential(*modules).to(device)

        def predictor():
            layers = [nn.Sequential(nn.Linear(hidden_dims[-1], hidden_dims[-1]), nn.LeakyReLU()) for _ in range(predictor_depth)]
            layers.append(nn.Linear(hidden_dims[-1], self.number_of_compartments))
            return nn.Sequential(*layers).to(device)

        self.D_predictor = predictor()
        self.T2_predictor = predictor()
        self.v_predictor = predictor()
        self._state = _PiaState(self)

    def _run(self, x):
        dev = ops.require_gpu()
        if not torch.is_tensor(x):
            raise TypeError("x must be a torch.Tensor")
        if x.dim() != 2 or x.shape[1] != self.number_of_signals:
            raise ValueError(f"x must be [n, {self.number_of_signals}], got {tuple(x.shape)}")
        ops._chk(x, "x")
        if x.requires_grad and torch.is_grad_enabled():
            raise ValueError("PIA: the kernels give no gradient with respect to the input x (detach it)")
        if next(self.parameters()).device != x.device:
            raise ops.InrDeviceError("PIA: move the model to the input's HIP device first (model.cuda())")
        st = self._state
        st.ensure()
        params = list(self.parameters())
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _PiaFn.apply(st, x, *params)
        return pia_forward(st, x, device=dev)

    def encode(self, x):
        """PIA.py:97-110: ``[D (float64), T2, v]``."""
        _, D, T2, v = self._run(x)
        return [D, T2, v]

    def decode(self, D, T2, v):
        """PIA.py:112-130 as a stand-alone method: latent codes -> signals, in the reference's tensor expressions and dtypes
        (the float64 sum is rounded into a float32 tensor, then scaled by 1000).  ``forward`` does not come through here: its
        decoder is part of the head kernel."""
        signal = torch.zeros((D.shape[0], self.number_of_signals), device=D.device)
        D, T2, v = D.T, T2.T, v.T
        ctr = 0
        for b in self.b_values:
            for TE in self.TE_values:
                signal[:, ctr] = sum(v[c] * torch.exp(-b / 1000 * D[c]) * torch.exp(-TE / T2[c]) for c in range(3))
                ctr += 1
        return 1000 * signal

    def forward(self, x):
        signal, D, T2, v = self._run(x)
        return [signal, x, D, T2, v]

    def loss_function(self, recons, x, PIDS, tissue_available=False):
        """PIA.py:138-155.  ``tissue_available=False``: ``mean(PIDS * (signal - x) ** 2)``, the loss the class is trained with
        (``PiaFitter.step`` is its fused form).

        ``tissue_available=True`` reproduces the reference's VALUE for the same inputs, as it is written there:
        ``mse(signal) + mse(D) + 1e-4 mse(T2) + 0.2 kl_div(v_pred, v_true)``, with ``F.kl_div`` fed probabilities, not
        log-probabilities, exactly as the reference does (not corrected here).  In the reference this branch cannot be
        trained: ``pred_D`` is float64, a float32 ``true_D`` makes ``backward()`` raise "Found dtype Float but expected
        Double".  Here its gradients are whatever autograd gives through ``inr_pia_backward_train`` once the caller passes a
        float64 ``true_D``; there is no fused supervised step."""
        if tissue_available:
            pred_signal, pred_D, pred_T2, pred_v = recons
            true_signal, true_D, true_T2, true_v = x
            return (F.mse_loss(pred_signal, true_signal) + F.mse_loss(pred_D, true_D) + 0.0001 * F.mse_loss(pred_T2, true_T2)
                    + 0.2 * F.kl_div(pred_v, true_v))
        return torch.mean(PIDS * (recons - x) ** 2)


def pia_forward(state: _PiaState, x: torch.Tensor, chunk_rows: int = 32768, device=None, want_signal: bool = True):
    """``inr_pia_forward``: no stash, ``chunk_rows`` rows at a time.  Returns (signal or None, D, T2, v)."""
    n = x.shape[0]
    dev = device or x.device
    signal, D, T2, v = _outputs(n, dev)
    if n == 0:
        return signal, D, T2, v
    chunk = max(1, min(int(chunk_rows), n))
    ws = state.workspace(chunk, False, dev)
    check(lib().inr_pia_forward(C.byref(state.desc), state.flat.data_ptr(), x.data_ptr(), n, signal.data_ptr() if want_signal else 0,
                                D.data_ptr(), T2.data_ptr(), v.data_ptr(), chunk, ws.data_ptr(), ws.numel(), ops._stream()),
          "inr_pia_forward")
    state.give_back(ws)
    return (signal if want_signal else None), D, T2, v


class PiaFitter(AdamOwner):
    """The fused training step of a ``PIA`` (``inr_pia_fit_step``): forward, ``mean(pids * (signal - x) ** 2)``, backward,
    fixed-order gradient reduction and Adam in one enqueue, the loss left on the device."""

    def __init__(self, model: PIA, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        ops.require_gpu()
        self.model = model
        if not next(model.parameters()).is_cuda:
            raise ops.InrDeviceError("PiaFitter: the model must live on a HIP device (model.cuda())")
        self.state = model._state
        self.state.ensure()
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.adam = AdamState(self.state.flat)
        self._ws = Workspace()

    steps_done = AdamOwner.step_count

    def step(self, x: torch.Tensor, pids: torch.Tensor = None) -> torch.Tensor:
        """One step on the batch ``x`` [n, 16] (weights ``pids`` [n, 16], default 1).  Returns the loss before the update as a
        one-element device tensor (no host synchronisation)."""
        ops._chk(x, "x")
        if x.dim() != 2 or x.shape[1] != 16:
            raise ValueError(f"x must be [n, 16], got {tuple(x.shape)}")
        if pids is not None:
            ops._chk(pids, "pids", x.shape)
        st = self.state
        st.ensure()
        n = x.shape[0]
        need = lib().inr_pia_workspace_bytes(C.byref(st.desc), n, 1)
        if need == 0:
            check(-1, "inr_pia_workspace_bytes")
        ws = self._ws.grow(need, x.device)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        self.steps_done += 1
        check(lib().inr_pia_fit_step(C.byref(st.desc), st.flat.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(),
                                     self.v.data_ptr(), x.data_ptr(), ops._ptr(pids), n, self.steps_done, self.lr, self.betas[0],
                                     self.betas[1], self.eps, loss.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()),
              "inr_pia_fit_step")
        return loss

    def encode_volume(self, signals, chunk_rows: int = 32768):
        """Encode every voxel: ``signals`` [..., 16] (array or tensor, the decoder's units) -> device tensors
        ``D`` [..., 3] float64, ``T2`` [..., 3], ``v`` [..., 3]."""
        dev = ops.require_gpu()
        sig = signals if torch.is_tensor(signals) else torch.from_numpy(np.ascontiguousarray(signals))
        if sig.shape[-1] != 16:
            raise ValueError(f"signals must be [..., 16], got {tuple(sig.shape)}")
        lead = tuple(sig.shape[:-1])
        x = sig.to(dev, torch.float32).reshape(-1, 16).contiguous()
        self.state.ensure()
        _, D, T2, v = pia_forward(self.state, x, chunk_rows=chunk_rows, device=dev, want_signal=False)
        return D.reshape(lead + (3,)), T2.reshape(lead + (3,)), v.reshape(lead + (3,))


def get_batch(batch_size=16, noise_sdt=0.1):
    """PIA.py:171-213: one synthetic training batch.  Draws come from NumPy's global generator in the reference's order (nine
    uniform vectors, then the noise matrix), so the same ``np.random.seed`` gives the same batch; the per-sample loop is one
    array expression with the reference's operation order.  Returns float32 CPU tensors
    ``(noisy signal [n, 16], D [n, 3], T2 [n, 3], v [n, 3], clean signal [n, 16])``."""
    b_values = [0, 150, 1000, 1500]
    TE_values = [0, 13, 93, 143]
    nb = np.array([-b / 1000 for b in b_values for _ in TE_values])
    nte = np.array([float(-TE) for _ in b_values for TE in TE_values])
    lows_highs = ((0.3, 0.7), (0.7, 1.7), (2.7, 3), (20, 70), (40, 100), (500, 1000), (0, 1), (0, 1), (0, 1))
    draws = [np.random.uniform(lo, hi, batch_size) for lo, hi in lows_highs]
    D = np.asarray(draws[0:3])
    T2 = np.asarray(draws[3:6])
    total = draws[6] + draws[7] + draws[8]
    v = np.asarray([draws[6] / total, draws[7] / total, draws[8] / total])
    comp = [v[c][:, None] * np.exp(nb[None, :] * D[c][:, None]) * np.exp(nte[None, :] / T2[c][:, None]) for c in range(3)]
    signal = comp[0] + comp[1] + comp[2]
    noise = np.random.normal(0, noise_sdt, signal.shape)
    return (1000 * torch.from_numpy(signal + noise).float(), torch.from_numpy(D.T).float(), torch.from_numpy(T2.T).float(),
            torch.from_numpy(v.T).float(), 1000 * torch.from_numpy(signal).float())


def detect_PIDS_slice(b, S):
    """PIA.py:286-327 on the device (``inr_pids_slice``): ``S`` [rows, cols, 4, 4] -> float64 maps ``PIDS_ADC1`` [rows, cols]
    (ADC > 3), ``PIDS_ADC2`` (ADC < 0), ``PIDS_b_decay`` [rows, cols, 4, 3], ``PIDS_TE_decay`` [rows, cols, 4, 3].  As in the
    reference, the left neighbour of a decay comparison is truncated toward zero first."""
    dev = ops.require_gpu()
    S = np.asarray(S.detach().cpu() if torch.is_tensor(S) else S, dtype=np.float64)
    if S.ndim != 4 or S.shape[2:] != (4, 4):
        raise ValueError(f"S must be [rows, cols, 4, 4], got {S.shape}")
    bv = np.asarray(b, dtype=np.float64).reshape(-1)
    if bv.size != 4:
        raise ValueError("b must hold four values")
    rows, cols = S.shape[:2]
    npix = rows * cols
    Sd = torch.from_numpy(np.ascontiguousarray(S)).to(dev)
    bd = torch.from_numpy(bv).to(dev)
    a1 = torch.empty(npix, dtype=torch.float32, device=dev)
    a2 = torch.empty(npix, dtype=torch.float32, device=dev)
    bdec = torch.empty((npix, 4, 3), dtype=torch.float32, device=dev)
    tdec = torch.empty((npix, 4, 3), dtype=torch.float32, device=dev)
    if npix:
        check(lib().inr_pids_slice(a1.data_ptr(), a2.data_ptr(), bdec.data_ptr(), tdec.data_ptr(), Sd.data_ptr(), bd.data_ptr(),
                                   npix, ops._stream()), "inr_pids_slice")
    return (a1.cpu().numpy().astype(np.float64).reshape(rows, cols), a2.cpu().numpy().astype(np.float64).reshape(rows, cols),
            bdec.cpu().numpy().astype(np.float64).reshape(rows, cols, 4, 3),
            tdec.cpu().numpy().astype(np.float64).reshape(rows, cols, 4, 3))


def ADC_slice(bvalues, slicedata):
    """PIA.py:157-169: the least-squares ADC of ``log(y + 1e-7)`` over ``b / 1000`` clipped to [0, 3]; ``slicedata``
    [rows, cols, n_b] -> float64 [rows, cols].  The fit is ``inr_adc_map``; only the lower clip differs from ``calculate_ADC``."""
    from . import metrics
    dev = ops.require_gpu()
    data = torch.as_tensor(np.asarray(slicedata), dtype=torch.float32).to(dev).contiguous()
    adc = metrics.calculate_ADC_device(np.asarray(bvalues, dtype=np.float64).reshape(-1), data)
    return np.clip(adc.cpu().numpy().astype(np.float64), 0.0, 3.0)
