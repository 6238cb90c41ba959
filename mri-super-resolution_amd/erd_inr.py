"""The soft-ERD INR family of the reference's ``INR_ERD.py`` (and ``prepare_qual_images.py``) on the device.

``ErdSiren`` mirrors ``Siren`` of INR_ERD.py:28-67: a SIREN trunk closed by ``Linear + ReLU``, a ReLU head, and an in-module
coordinate perturbation; same constructor signature, RNG draw order and module registration order, so ``state_dict()`` keys
and the weights drawn after ``torch.manual_seed`` are the reference's.  ``ErdFitter`` runs its two training phases
(INR_ERD.py:198-217 pre-training until the loss falls below a threshold, INR_ERD.py:252-273 the dual-learning-rate
fine-tuning step) on the fused kernels of ``csrc/erd_siren.hip``; ``soft_erd`` is the weighting of INR_ERD.py:143-158 /
225-235.  There is no CPU path and no layer-by-layer fallback: shapes outside ``out_features == 1``, ``in_features <= 8``,
``hidden_features in {64, 128}``, ``hidden_layers <= 8`` raise.
"""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np
import torch
from torch import nn

from . import ops
from ._lib import INR_ERD_COLLAPSED, INR_ERD_CONVERGED, INR_ERD_RUNNING, check, lib
from .contrast import eps, mag      # INR_ERD.py:25-26, the same two constants as master.py:42-43
from .flat import AdamOwner, AdamState, FlatParams, Workspace
from .inr import SineLayer

STATE_NAMES = {INR_ERD_RUNNING: "running", INR_ERD_CONVERGED: "converged", INR_ERD_COLLAPSED: "collapsed"}


def _check_shape(in_features, hidden_features, hidden_layers, out_features):
    if out_features != 1 or not 1 <= in_features <= 8 or hidden_features not in (64, 128) or not 0 <= hidden_layers <= 8:
        raise ValueError("ErdSiren: the soft-ERD kernels serve out_features == 1, in_features <= 8, hidden_features in "
                         f"{{64, 128}}, hidden_layers <= 8 (got in={in_features}, hidden={hidden_features}, "
                         f"layers={hidden_layers}, out={out_features}); there is no other path")


def erd_param_layout(desc):
    """(total, [(w_off, b_off)] per tensor in kernel order: trunk layers, head, perturb_linear, perturb_linear2, group_b)."""
    total, offs = ops.param_layout(lib().inr_erd_param_count, lib().inr_erd_param_offsets, desc, 2 * (desc.hidden_layers + 5) + 1)
    return total, list(zip(offs[0:-1:2], offs[1:-1:2])), offs[-1]


class ErdSiren(nn.Module):
    """INR_ERD.py:28-67.  ``forward(coords, sample=0, eps=0)``: the coordinates are detached; with ``perturb`` the scalar
    ``p = eps * tanh(perturb_linear2(tanh(perturb_linear([coords, sample]))))`` ([N, 1]) is broadcast-added to every
    coordinate component, then trunk, head and ReLU.  ``sample`` enters as the plain integer cast to float.

    The reference reads a module-level ``model_input`` inside ``forward`` (INR_ERD.py:59); at every call site it equals
    ``coords``, and that is how it is defined here.  ``perturb_init='default'`` keeps ``nn.Linear``'s own initialisation of the
    two perturb layers (prepare_qual_images.py's variant) instead of U(+-sqrt(6 / H) / omega) (INR_ERD.py:49-51).
    ``forward`` runs the inference kernel and carries no autograd graph: training goes through ``ErdFitter``."""

    def __init__(self, in_features, hidden_features, hidden_layers, out_features=1, first_omega_0=30., hidden_omega_0=30.,
                 perturb=False, perturb_init="reference"):
        super().__init__()
        _check_shape(in_features, hidden_features, hidden_layers, out_features)
        if perturb_init not in ("reference", "default"):
            raise ValueError("perturb_init must be 'reference' or 'default'")
        self.in_features, self.hidden_features, self.hidden_layers = in_features, hidden_features, hidden_layers
        self.first_omega_0, self.hidden_omega_0 = float(first_omega_0), float(hidden_omega_0)
        # draw and registration order of INR_ERD.py:34-53: the trunk's layers are created first but `net` becomes a
        # registered module only after `relu` and `final_linear`
        net = [SineLayer(in_features, hidden_features, is_first=True, omega_0=first_omega_0)]
        self.relu = nn.ReLU()
        for _ in range(hidden_layers):
            net.append(SineLayer(hidden_features, hidden_features, is_first=False, omega_0=hidden_omega_0))
        net.append(nn.Linear(hidden_features, hidden_features))
        net.append(nn.ReLU())
        self.final_linear = nn.Linear(hidden_features, out_features)
        bound = np.sqrt(6 / hidden_features) / hidden_omega_0
        with torch.no_grad():
            self.final_linear.weight.uniform_(-bound, bound)
        self.net = nn.Sequential(*net)
        self.perturb_linear = nn.Linear(in_features + 1, hidden_features)
        self.perturb_linear2 = nn.Linear(hidden_features, out_features)
        if perturb_init == "reference":
            with torch.no_grad():
                self.perturb_linear.weight.uniform_(-bound, bound)
                self.perturb_linear2.weight.uniform_(-bound, bound)
        self.tanh = nn.Tanh()
        self.perturb = perturb
        self.perturb_init = perturb_init

    def desc(self):
        return ops.make_desc(self.in_features, self.hidden_features, self.hidden_layers, 1, self.first_omega_0, self.hidden_omega_0)

    def kernel_parameters(self):
        """Parameters in the order of the kernels' flat buffer: trunk layers, head, perturb_linear, perturb_linear2."""
        out = []
        for k in range(self.hidden_layers + 1):
            out += [self.net[k].linear.weight, self.net[k].linear.bias]
        out += [self.net[self.hidden_layers + 1].weight, self.net[self.hidden_layers + 1].bias]
        out += [self.final_linear.weight, self.final_linear.bias, self.perturb_linear.weight, self.perturb_linear.bias,
                self.perturb_linear2.weight, self.perturb_linear2.bias]
        return out

    def _flat(self):
        """The flat buffer the kernels read: the fitter's live one when the parameters are its views, else a packed copy."""
        fitter = getattr(self, "_fitter", None)
        if fitter is not None and fitter.owns(self):
            return fitter.flat
        total, offsets, _ = erd_param_layout(self.desc())
        return FlatParams(total, itertools.chain.from_iterable(offsets)).pack(self.kernel_parameters())

    def forward(self, coords, sample=0, eps=0, chunk_rows=1 << 16):
        ops.require_gpu()
        x = ops._chk(coords.detach().reshape(-1, coords.shape[-1]).contiguous(), "coords")
        if x.shape[1] != self.in_features:
            raise ValueError(f"coords must be [..., {self.in_features}], got {tuple(coords.shape)}")
        if next(self.parameters()).device != x.device:
            raise ops.InrDeviceError("ErdSiren: move the model to the input's HIP device first (model.cuda())")
        y = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        desc = self.desc()
        flat = self._flat()
        check(lib().inr_erd_forward(C.byref(desc), flat.data_ptr(), x.data_ptr(), x.shape[0], y.data_ptr(), int(sample),
                                    float(eps), int(bool(self.perturb)), int(chunk_rows), ops._stream()), "inr_erd_forward")
        return y.reshape(*coords.shape[:-1], 1)


def soft_erd(values, b0, noise_level, mul=1000, slope=20, min_temp=2.0):
    """Soft-ERD weights and weighted mean (INR_ERD.py:143-158, 225-235) for every pixel in one launch, float64.
    ``values`` [..., K] acquisitions per pixel, ``b0`` [...]; returns ``(weights [..., K], mean_image [...])`` as float64 numpy
    arrays.  ``temp = max(mul * exp(-slope * mean / b0), min_temp)``; where ``mean > 2 * noise_level`` the weights are
    ``exp(x / temp)`` -- unnormalised, as the reference passes them to the loss -- and the mean image is the softmax-weighted
    mean; elsewhere ``1 / K`` and the plain mean.  Non-finite weights (the reference's ``RuntimeWarning`` branch, which its
    ``try`` never catches) raise ``ValueError``."""
    dev = ops.require_gpu()
    values = np.ascontiguousarray(values, dtype=np.float64)
    b0 = np.ascontiguousarray(b0, dtype=np.float64)
    if values.shape[:-1] != b0.shape:
        raise ValueError(f"values {values.shape} must be b0's shape {b0.shape} plus an acquisition axis")
    K = values.shape[-1]
    n = int(b0.size)
    v = torch.from_numpy(values.reshape(n, K)).to(dev)
    b = torch.from_numpy(b0.reshape(n)).to(dev)
    w = torch.empty((n, K), dtype=torch.float64, device=dev)
    mean = torch.empty(n, dtype=torch.float64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().inr_soft_erd(w.data_ptr(), mean.data_ptr(), v.data_ptr(), b.data_ptr(), n, K, float(noise_level), float(mul),
                             float(slope), float(min_temp), bad.data_ptr(), ops._stream()), "inr_soft_erd")
    n_bad = int(bad.item())
    if n_bad:
        raise ValueError(f"soft_erd: {n_bad} non-finite weights (exp(x / temp) overflowed): rescale the signal or raise min_temp")
    return w.cpu().numpy().reshape(values.shape), mean.cpu().numpy().reshape(b0.shape)


def noise_level(b3, noise_center, _slice):
    """INR_ERD.py:140-142: population std of the 5 x 5 window [c-3:c+2] of one slice, over sqrt(2 - pi / 2)."""
    c0, c1 = noise_center
    return np.std(b3[c0 - 3:c0 + 2, c1 - 3:c1 + 2, _slice]) / np.sqrt(2 - np.pi / 2)


def calc_adc(dwi, b0, b):
    """INR_ERD.py:98-100: ADC in 1e-3 mm^2/s.  Not ``contrast.calc_adc``: master.py:49-51 scales by ``mag * mag``."""
    return -np.log((dwi / (b0 + eps)) + eps) / b * mag


def calculate_CNR_SNR(case, image):
    """INR_ERD.py:102-124: ``(log10 SNR_c, log10 CNR, S_c, S_b, S_c / S_b)`` from the 3 x 3 squares around the lesion and its
    contralateral point and the 5 x 5 noise square."""
    cc_x, cc_y = case.cancer_loc
    cb_x, cb_y = case.contralateral_loc
    cn_x, cn_y = case.noise
    Sc = image[cc_x - 1:cc_x + 2, cc_y - 1:cc_y + 2].mean()
    Sb = image[cb_x - 1:cb_x + 2, cb_y - 1:cb_y + 2].mean()
    N = np.std(image[cn_x - 2:cn_x + 3, cn_y - 2:cn_y + 3])
    SNRc, SNRb = Sc / (N + 1e-7), Sb / (N + 1e-7)
    return np.log10(SNRc), np.log10(abs(SNRc - SNRb)), Sc, Sb, Sc / Sb


class ErdFitter(AdamOwner):
    """The two training phases of INR_ERD.py on the fused kernels.  The model's parameters become views of one flat buffer
    (kernel order, every tensor padded to 16 bytes); Adam state lives here.  The reference creates a fresh optimizer for each
    phase (INR_ERD.py:196, 252-255): ``pretrain`` always starts from a zeroed one -- its Adam runs over the perturb branch too,
    with zero gradients, which moves nothing only while that branch's moments are zero -- and ``finetune`` does unless told
    otherwise.

    Where the methods differ from a bare transcription: they take the coordinate rows as their first argument (the reference
    reads them from its dataset object), and ``mean_reconstruction`` takes the acquisition count and ``eps`` beside the
    shape.  ``finetune`` and ``mean_reconstruction`` run WITH the perturbation whatever ``model.perturb`` says, which is
    prepare_qual_images.py's behaviour; INR_ERD.py itself builds its ``Siren`` with ``perturb=False`` and never switches it
    on, so its fine-tuning step and mean reconstruction see no perturbation and its ``perturb_linear*`` tensors never move.
    For that, call the model and ``loss_grad(perturb=False)`` directly."""

    DEFAULT_MAX_STEPS = 200_000      # the reference's `while` has no bound; this guard is ~10x what its fits take

    def __init__(self, model: ErdSiren, betas=(0.9, 0.999), adam_eps=1e-8, make_model=None):
        ops.require_gpu()
        self.model = model
        self.betas, self.adam_eps = (float(betas[0]), float(betas[1])), float(adam_eps)
        self.make_model = make_model
        self.desc = model.desc()
        self.total, self.offsets, self.group_b = erd_param_layout(self.desc)
        self.params = FlatParams(self.total, itertools.chain.from_iterable(self.offsets))
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
        self.model._fitter = self

    def owns(self, model):
        return model is self.model and self.params.owns(model.kernel_parameters())

    def reset_optimizer(self):
        self.adam.reset()

    def _ws(self, n):
        need = lib().inr_erd_workspace_bytes(C.byref(self.desc), int(n))
        if need == 0:
            check(-1, "inr_erd_workspace_bytes")
        return self._workspace.grow(need, self.flat.device)

    def _rows(self, coords):
        if not self.owns(self.model):
            self._adopt()                             # moved / reloaded: re-flatten (the optimizer state is kept)
        return ops._chk(coords.detach().reshape(-1, coords.shape[-1]).contiguous(), "coords")

    def pretrain_steps(self, x, t, max_steps, lr, threshold, status):
        """Enqueue up to ``max_steps`` steps on the device-resident ``status`` (no host read)."""
        ws = self._ws(x.shape[0])
        check(lib().inr_erd_pretrain(C.byref(self.desc), self.flat.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(),
                                     self.v.data_ptr(), x.data_ptr(), t.data_ptr(), x.shape[0], self.step_count + 1, int(max_steps),
                                     float(lr), self.betas[0], self.betas[1], self.adam_eps, float(threshold), status.data_ptr(),
                                     ws.data_ptr(), ws.numel(), ops._stream()), "inr_erd_pretrain")

    @staticmethod
    def new_status(device):
        return torch.zeros(4, dtype=torch.int32, device=device)       # {RUNNING, 0 steps, 0.0, 0.0}

    @staticmethod
    def read_status(status):
        host = status.cpu()
        return {"state": int(host[0]), "steps_done": int(host[1]), "last_loss": float(host[2:3].view(torch.float32)[0]),
                "y_max": float(host[3:4].view(torch.float32)[0])}

    def pretrain(self, coords, target, lr=3e-4, threshold=2e-5, max_steps=None, check_every=64, max_reseeds=16):
        """INR_ERD.py:198-217: Adam steps on ``mean((f(x) - target)^2)`` until the loss of a step's forward is not above
        ``threshold`` (that step is still applied, and is the last).  If a step's forward gives all-zero outputs the model and
        the optimizer are re-initialised (``make_model()``, default: a new ``ErdSiren`` of the same shape drawn from the
        current torch RNG) and the loop goes on, as the reference does.  The host reads the status block every
        ``check_every`` steps only.  ``max_steps`` (default ``DEFAULT_MAX_STEPS`` = 200,000, over all re-seeds) is a guard
        the reference lacks.  The optimizer state is zeroed on entry.  Returns ``{"state", "steps", "last_loss", "reseeds"}``; ``steps`` counts every step taken."""
        max_steps = self.DEFAULT_MAX_STEPS if max_steps is None else int(max_steps)
        self.reset_optimizer()                        # INR_ERD.py:196: a fresh Adam in front of the loop
        x = self._rows(coords)
        t = ops._chk(target.detach().reshape(-1).contiguous(), "target")
        total_steps, reseeds = 0, 0
        status = self.new_status(x.device)
        info = {"state": INR_ERD_RUNNING, "steps_done": 0, "last_loss": float("nan"), "y_max": 0.0}
        while total_steps + info["steps_done"] < max_steps:
            chunk = min(int(check_every), max_steps - total_steps - info["steps_done"])
            self.pretrain_steps(x, t, chunk, lr, threshold, status)
            info = self.read_status(status)
            self.step_count = info["steps_done"]
            if info["state"] == INR_ERD_CONVERGED:
                break
            if info["state"] == INR_ERD_COLLAPSED:
                if reseeds >= max_reseeds:
                    break
                reseeds += 1
                total_steps += info["steps_done"]
                self.reseed()
                status = self.new_status(x.device)
                info = {"state": INR_ERD_RUNNING, "steps_done": 0, "last_loss": info["last_loss"], "y_max": 0.0}
        return {"state": STATE_NAMES[info["state"]], "steps": total_steps + info["steps_done"], "last_loss": info["last_loss"],
                "reseeds": reseeds}

    def reseed(self):
        """A freshly initialised network and optimizer (INR_ERD.py:212-217), written into the live parameter buffer."""
        m = self.model
        fresh = self.make_model() if self.make_model else ErdSiren(
            m.in_features, m.hidden_features, m.hidden_layers, 1, m.first_omega_0, m.hidden_omega_0, perturb=m.perturb,
            perturb_init=m.perturb_init)
        with torch.no_grad():
            for dst, src in zip(m.kernel_parameters(), fresh.kernel_parameters()):
                dst.copy_(src.to(dst.device))
        self.reset_optimizer()

    def finetune(self, coords, targets, weights, steps=1, lr_perturb=3e-4, lr_net=1e-7, eps=1.0 / 128.0, new_optimizers=True):
        """INR_ERD.py:252-273, ``steps`` times: ``loss = sum_s mean(w_s (f(x; s, eps) - g_s)^2)`` over the acquisitions, one
        Adam step with ``lr_perturb`` on the perturb branch and ``lr_net`` on trunk + head.  Defaults are INR_ERD.py's (one
        step, 3e-4 / 1e-7); prepare_qual_images.py's 502 steps and 1e-5 go through the arguments.  The perturbation is on in
        this phase whatever ``model.perturb`` says.  ``targets`` / ``weights``: [K, N] (weights may be None).  Returns the
        per-step losses (device tensor)."""
        x = self._rows(coords)
        K = targets.shape[0]
        t = ops._chk(targets.detach().reshape(K, -1).contiguous(), "targets")
        w = None if weights is None else ops._chk(weights.detach().reshape(K, -1).contiguous(), "weights")
        if t.shape[1] != x.shape[0] or (w is not None and w.shape != t.shape):
            raise ValueError("targets / weights must be [K, N] for N coordinate rows")
        if new_optimizers:
            self.reset_optimizer()
        losses = torch.empty(max(int(steps), 1), dtype=torch.float32, device=x.device)
        ws = self._ws(x.shape[0])
        check(lib().inr_erd_finetune(C.byref(self.desc), self.flat.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(),
                                     self.v.data_ptr(), x.data_ptr(), t.data_ptr(), ops._ptr(w), K, x.shape[0], float(eps),
                                     self.step_count + 1, int(steps), float(lr_perturb), float(lr_net), self.betas[0],
                                     self.betas[1], self.adam_eps, losses.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()),
              "inr_erd_finetune")
        self.step_count += int(steps)
        return losses[:int(steps)]

    def loss_grad(self, coords, target, weight=None, sample=0, eps=0.0, perturb=False, accumulate=False):
        """Loss and flat gradient of one acquisition (``inr_erd_loss_grad``); ``accumulate`` adds to the previous calls'."""
        x = self._rows(coords)
        t = ops._chk(target.detach().reshape(-1).contiguous(), "target")
        w = None if weight is None else ops._chk(weight.detach().reshape(-1).contiguous(), "weight")
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        ws = self._ws(x.shape[0])
        check(lib().inr_erd_loss_grad(C.byref(self.desc), self.flat.data_ptr(), self.grads.data_ptr(), x.data_ptr(), t.data_ptr(),
                                      ops._ptr(w), x.shape[0], int(sample), float(eps), int(bool(perturb)), int(bool(accumulate)),
                                      loss.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()), "inr_erd_loss_grad")
        return loss, self.grads

    def adam_step(self, lr_net, lr_perturb):
        """One dual-group Adam step on ``self.grads`` (``inr_erd_adam_step``)."""
        check(lib().inr_erd_adam_step(C.byref(self.desc), self.flat.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(),
                                      self.v.data_ptr(), self.step_count + 1, float(lr_net), float(lr_perturb), self.betas[0],
                                      self.betas[1], self.adam_eps, ops._stream()), "inr_erd_adam_step")
        self.step_count += 1

    def split(self, flat):
        """Views of a flat vector per tensor, in ``kernel_parameters()`` order."""
        return self.params.split(flat)

    def mean_reconstruction(self, shape, n_acquisitions, eps=1.0 / 128.0):
        """INR_ERD.py:276-282: the mean over acquisitions of ``f(x; s, eps)`` on the grid ``shape`` (any size: the network
        is continuous), as a float64 numpy image."""
        grid = ops.mgrid(tuple(int(s) for s in shape))
        was = self.model.perturb
        self.model.perturb = True
        try:
            acc = np.zeros(tuple(int(s) for s in shape))
            for s in range(int(n_acquisitions)):
                acc += self.model(grid, s, eps).reshape(*shape).cpu().numpy()
        finally:
            self.model.perturb = was
        return acc / int(n_acquisitions)
