"""The voxel-footprint forward model of a SIREN fit (csrc/footprint.hip).

Every other fit of this package treats a training voxel as a point sample of the continuous image.  An acquired voxel is an
average of the object over its footprint -- the in-plane voxel area and the slice profile -- so here a datum is a weighted
average of the network over ``K`` sub-sample positions::

    p_i  = sum_k w_k * INR(x_i + delta_k)
    loss = mean_i(wt_i * (p_i - t_i)^2)

and the fitted function is the de-blurred image.  ``Footprint`` holds the quadrature rule (offsets and weights, formed on the host
in float64, once per fit); ``footprint_inputs`` / ``footprint_forward`` expand coordinates and average predictions on the device;
``FootprintSirenFitter`` runs whole steps in one call of ``inr_siren_fit_footprint``.  Sub-sample ``k`` of datum ``i`` is row
``i*K + k`` everywhere.
"""
from __future__ import annotations

import itertools
import math

import numpy as np
import torch

from . import ops
from .inr import Siren, SirenFitter, input_mapping

MAX_SAMPLES = ops.FOOTPRINT_MAX_SAMPLES
_FWHM_PER_SIGMA = 2.354820045


def _per_axis(value, d, name, kind=float):
    vals = [kind(v) for v in (value if np.ndim(value) else [value] * d)]
    if len(vals) != d:
        raise ValueError(f"{name} has {len(vals)} entries for {d} axes")
    return vals


def _tensor_rule(axes):
    """The tensor product of per-axis rules [(nodes, weights), ...], last axis fastest."""
    offsets = np.array(list(itertools.product(*[nodes for nodes, _ in axes])), dtype=np.float64).reshape(-1, len(axes))
    weights = np.array([math.prod(ws) for ws in itertools.product(*[w for _, w in axes])], dtype=np.float64)
    return offsets, weights


class Footprint:
    """``K`` sub-sample offsets ``delta_k`` [K, d] (in the coordinates the network is fitted in) and their weights [K],
    ``sum(weights) == 1``.  ``count`` is K."""

    def __init__(self, offsets, weights):
        offsets = np.asarray(offsets, dtype=np.float64)
        weights = np.asarray(weights, dtype=np.float64)
        if offsets.ndim != 2 or weights.ndim != 1 or offsets.shape[0] != weights.shape[0]:
            raise ValueError(f"offsets {offsets.shape} and weights {weights.shape} must be [K, d] and [K]")
        if not 1 <= offsets.shape[0] <= MAX_SAMPLES:
            raise ValueError(f"a footprint has 1 .. {MAX_SAMPLES} sub-samples (got {offsets.shape[0]})")
        if not 1 <= offsets.shape[1] <= 4:
            raise ValueError(f"a footprint has 1 .. 4 axes (got {offsets.shape[1]})")
        if not (np.isfinite(offsets).all() and np.isfinite(weights).all()):
            raise ValueError("footprint offsets and weights must be finite")
        if abs(float(weights.sum()) - 1.0) > 1e-6:
            raise ValueError(f"footprint weights must sum to 1 (got {float(weights.sum())!r})")
        self.offsets, self.weights = offsets, weights
        self._device = {}

    @property
    def count(self) -> int:
        return int(self.weights.shape[0])

    @property
    def dim(self) -> int:
        return int(self.offsets.shape[1])

    def tensors(self, device):
        """(offsets [K, d], weights [K]) as float32 tensors on ``device`` (made once per device)."""
        key = str(device)
        if key not in self._device:
            self._device[key] = (torch.from_numpy(self.offsets.astype(np.float32)).to(device).contiguous(),
                                 torch.from_numpy(self.weights.astype(np.float32)).to(device).contiguous())
        return self._device[key]

    @classmethod
    def point(cls, d: int) -> "Footprint":
        """The single-sample footprint: the point model."""
        return cls(np.zeros((1, int(d))), np.ones(1))

    @classmethod
    def box(cls, widths, samples, spacing) -> "Footprint":
        """A box of ``widths[a]`` units on axis a, ``samples[a]`` midpoint nodes ``((j + 0.5)/S - 0.5) * width * spacing[a]`` of
        weight ``1/S`` each; ``spacing[a]`` is the normalised length of one unit (``2/(s_a - 1)`` for ``get_mgrid(shape)``).
        With ``S`` equal to the width in fine-grid steps this is the discrete block mean.  Width 0 or one sample: one node at 0."""
        d = len(widths)
        samples, spacing = _per_axis(samples, d, "samples", int), _per_axis(spacing, d, "spacing")
        axes = []
        for width, S, h in zip((float(w) for w in widths), samples, spacing):
            if S < 1 or width < 0 or not math.isfinite(width):
                raise ValueError(f"box footprint: width >= 0 and samples >= 1 per axis (got {width}, {S})")
            if S == 1 or width == 0:
                axes.append(([0.0], [1.0]))
            else:
                axes.append(([((j + 0.5) / S - 0.5) * width * h for j in range(S)], [1.0 / S] * S))
        return cls(*_tensor_rule(axes))

    @classmethod
    def gaussian(cls, fwhm, samples, spacing) -> "Footprint":
        """A Gaussian profile of full width at half maximum ``fwhm[a]`` units on axis a by Gauss-Hermite quadrature with
        ``samples[a]`` nodes: ``u = sqrt(2) sigma xi``, ``w = omega / sqrt(pi)``, ``sigma = fwhm / 2.354820045``."""
        d = len(fwhm)
        samples, spacing = _per_axis(samples, d, "samples", int), _per_axis(spacing, d, "spacing")
        axes = []
        for width, S, h in zip((float(w) for w in fwhm), samples, spacing):
            if S < 1 or width < 0 or not math.isfinite(width):
                raise ValueError(f"gaussian footprint: fwhm >= 0 and samples >= 1 per axis (got {width}, {S})")
            if S == 1 or width == 0:
                axes.append(([0.0], [1.0]))
            else:
                xi, omega = np.polynomial.hermite.hermgauss(S)
                sigma = width / _FWHM_PER_SIGMA
                axes.append(((math.sqrt(2.0) * sigma * h * xi).tolist(), (omega / math.sqrt(math.pi)).tolist()))
        return cls(*_tensor_rule(axes))


# ---- the 2 x ... block-mean data model of the drivers (data preparation: NumPy on the host) -------------------------------------------
def block_means(volume, upscale_axes: int = 2):
    """The mean of every 2 x ... block over the first ``upscale_axes`` axes (which must be even)."""
    volume = np.asarray(volume)
    up = range(min(upscale_axes, volume.ndim))
    if any(volume.shape[a] % 2 for a in up):
        raise ValueError(f"block means need even up-scaled axes (got shape {volume.shape})")
    blocks = [k for a in up for k in (volume.shape[a] // 2, 2)] + list(volume.shape[len(up):])
    return np.ascontiguousarray(volume.reshape(blocks).mean(axis=tuple(2 * a + 1 for a in up)))


def block_centres(hr_shape, upscale_axes: int = 2):
    """Where those means sit, [prod(lr_shape), d] float32 on the device: the block centres ``-1 + (2j + 0.5) * 2/(S_a - 1)`` of the HR
    grid's ``get_mgrid`` frame on the up-scaled axes, the HR coordinates on the others (NOT ``get_mgrid(lr_shape)``, whose end
    points sit elsewhere: this placement is what keeps an evaluation on ``hr_shape`` aligned with the data)."""
    axes = [-1.0 + (2.0 * np.arange(s // 2) + 0.5) * (2.0 / (s - 1)) if a < upscale_axes else np.linspace(-1.0, 1.0, s)
            for a, s in enumerate(hr_shape)]
    coords = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, len(hr_shape))
    return torch.from_numpy(coords.astype(np.float32)).to(ops.require_gpu())


def block_footprint(hr_shape, upscale_axes: int = 2, samples: int = 2) -> Footprint:
    """The footprint of such a block: 2 HR steps wide with ``samples`` midpoint nodes on every up-scaled axis (2: the four ... HR
    samples themselves), a point on the others."""
    d = len(hr_shape)
    return Footprint.box([2 if a < upscale_axes else 0 for a in range(d)], [samples if a < upscale_axes else 1 for a in range(d)],
                         [2.0 / (s - 1) if s > 1 else 0.0 for s in hr_shape])


def _chk_footprint(coords, footprint):
    if not isinstance(footprint, Footprint):
        raise TypeError("footprint must be a Footprint")
    if coords.dim() != 2 or coords.shape[1] != footprint.dim:
        raise ValueError(f"coords {tuple(coords.shape)} must be [n, {footprint.dim}] for this footprint")


def footprint_inputs(coords, B, footprint: Footprint):
    """The network inputs of every sub-sample: ``coords`` [n, d] -> [n*K, 2m] (``input_mapping`` of ``coords[i] + delta_k`` in
    row ``i*K + k``; [n*K, d] when ``B is None``)."""
    ops.require_gpu()
    _chk_footprint(coords, footprint)
    offsets, _ = footprint.tensors(coords.device)
    return input_mapping(ops.footprint_expand(coords.detach().contiguous(), offsets), B)


def footprint_forward(model: Siren, coords, B, footprint: Footprint, chunk_rows: int = 1 << 20):
    """``p`` [n]: what the forward model predicts for data at ``coords``, without gradients (inference and diagnostics)."""
    ops.require_gpu()
    _chk_footprint(coords, footprint)
    _, weights = footprint.tensors(coords.device)
    K = footprint.count
    per_chunk = max(1, int(chunk_rows) // K)
    out = []
    with torch.no_grad():
        for lo in range(0, coords.shape[0], per_chunk):
            y = model(footprint_inputs(coords[lo:lo + per_chunk], B, footprint))
            y = y[0] if isinstance(y, tuple) else y
            out.append(ops.footprint_reduce(y.reshape(-1).contiguous(), weights))
    return torch.cat(out) if out else torch.empty(0, dtype=torch.float32, device=coords.device)


class FootprintSirenFitter(SirenFitter):
    """``SirenFitter`` under the footprint forward model: ``step`` takes the inputs of all ``n*K`` sub-samples
    (``footprint_inputs``) and one target per datum, and enqueues ``n_steps`` full-batch steps by ONE call of
    ``inr_siren_fit_footprint``.  Served: the networks ``inr_siren_hp_eligible`` serves (every sine layer a multiple of 32 wide,
    hidden 128 / 256 / 512 / 1024, one output); anything else raises ``ValueError`` here.  ``step_cycle`` and
    ``fit_cycle_batch``, which are point-sampled, refuse this fitter."""
    batch_ok = False

    def __init__(self, model: Siren, footprint: Footprint, lr=1e-4, betas=(0.9, 0.999), eps=1e-8):
        if not isinstance(footprint, Footprint):
            raise TypeError("footprint must be a Footprint")
        super().__init__(model, lr=lr, betas=betas, eps=eps)
        if not ops.siren_hp_eligible(self.desc):
            raise ValueError("FootprintSirenFitter does not serve this network (inr_siren_hp_eligible: every sine layer a multiple "
                             "of 32 wide, hidden 128 / 256 / 512 / 1024, one output)")
        self.footprint = footprint

    def _ws(self, x):
        need = 4 * ops.siren_fit_footprint_workspace_floats(self.desc, x.shape[0] // self.footprint.count, self.footprint.count)
        return self._workspace.grow(need, x.device)

    def step(self, model_input_sub, target, n_steps=1, weight=None):
        """Run ``n_steps`` fit steps; returns the per-step losses as a device tensor (no sync)."""
        self._check_views()
        x = model_input_sub.detach().reshape(-1, model_input_sub.shape[-1]).contiguous()
        t = target.detach().reshape(-1).contiguous()
        w = None if weight is None else weight.detach().reshape(-1).contiguous()
        K = self.footprint.count
        if x.shape[0] != t.numel() * K:
            raise ValueError(f"model_input_sub has {x.shape[0]} rows, expected len(target) * K = {t.numel()} * {K}")
        _, fw = self.footprint.tensors(x.device)
        losses = torch.empty(max(int(n_steps), 1), dtype=torch.float32, device=x.device)
        ops.siren_fit_footprint(self.desc, self.flat, self.grads, self.m, self.v, x, t, w, fw, self.step_count + 1, int(n_steps),
                                self.lr, self.betas[0], self.betas[1], self.eps, losses, self._ws(x))
        self.step_count += int(n_steps)
        return losses[:n_steps]

    def step_cycle(self, model_input, targets, n_steps, weights=None, first_acq=0):
        raise NotImplementedError("FootprintSirenFitter.step_cycle: the footprint forward model serves single-target fits (step) only")
