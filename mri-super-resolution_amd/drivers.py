"""Callers on either side of the hot path: the reference's driver loops restated on the fused entry points.

* ``fit_volume``  -- superresDWI.py:84-162 / superresHybrid.py:79-125 for one N-D volume: max-normalise, LR =
  every second in-plane sample, Fourier features, ``Siren(2m, 512, 3, 1)``, Adam 1e-4, full-batch MSE fit, dense
  re-sampling at twice the HR in-plane grid ("x4" w.r.t. the LR grid), clamp at 0, PSNR/SSIM against the HR volume.
* ``fit_slice_ensemble`` -- master.py:130-160: small raw-coordinate SIREN on K acquisitions of one 2-D slice, one
  weighted optimizer step per acquisition per epoch, snapshot-ensemble of the last ``seg`` epochs at x1 and
  x``scale``.
* ``fit_wire_with_perturbnet`` -- wiretest.ipynb cell 10: the WIRE network's plain fit and its PerturbNet tail, the gradient
  flowing through the network's input into the PerturbNet.
* ``fit_hybrid`` -- superresHybrid.py:57-140: one 4-D (x, y, z, b) fit per echo time, re-scaling, normalisation by
  the (b = 0, TE = 0) image and the three-compartment fit of one slice (``pia.hybrid_fit_device``).
* ``run_volumes`` -- the patient loop (superresDWI.py:29) partitioned over one-process-per-GPU ranks with a final
  metric gather (``dist.py``).

Everything numerical runs on the HIP kernels; these functions only orchestrate.
"""
from __future__ import annotations

import threading
import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import dist as inr_dist
from . import matio, metrics, ops
from .footprint import (Footprint, FootprintSirenFitter, block_centres, block_footprint, block_means, footprint_forward,
                        footprint_inputs)
from .inr import PN, ImageFitting_set, ShardedSirenFitter, Siren, SirenFitter, fit_cycle_batch, input_mapping, reconstruct


def load_mat_volume(path: str, key: Optional[str] = None) -> np.ndarray:
    """Reads one array from a MATLAB v5 ``.mat`` (``anon_data/patNN_mean_b0.mat``: key ``data_mean_b0``)."""
    data = matio.loadmat(path)
    if key is None:
        keys = [k for k, v in data.items() if not k.startswith("__") and isinstance(v, np.ndarray) and v.ndim >= 2]
        if len(keys) != 1:
            raise KeyError(f"{path}: pass key=, candidates are {keys}")
        key = keys[0]
    return np.asarray(data[key])


def fourier_matrix(dim: int, mapping_size: int = 128, scale: float = 0.5, seed: Optional[int] = None) -> np.ndarray:
    """superresDWI.py:102-106: ``np.random.normal(size=(mapping_size, dim)) * scale`` as fp32 (seeded if asked)."""
    rng = np.random if seed is None else np.random.RandomState(seed)
    return (rng.normal(size=(mapping_size, dim)) * scale).astype(np.float32)


_INIT_LOCK = threading.Lock()      # torch.manual_seed + weight draws of one fit (see _fit_volume_once)
FIT_OK, FIT_RESEEDED, FIT_FAILED, FIT_ERROR = 0, 1, 2, 3      # record["status"]: see fit_volume / run_volumes


def fit_health(last_loss: float, recon: Optional[torch.Tensor] = None) -> str:
    """The reference's only recovery logic, generalised: ``INR_ERD.py:211-217`` / ``prepare_qual_images.py:176-182`` re-create
    the network when its whole output is zero (``if not model_output...max()``: a dead fit).  Here a fit is unhealthy when its
    loss is not finite ("nan": full-batch Adam can diverge) or when the clamped reconstruction is zero everywhere or not finite
    ("collapsed").  Returns "ok", "nan" or "collapsed"."""
    if last_loss is not None and not np.isfinite(last_loss):
        return "nan"
    if recon is not None and recon.numel():
        top = float(recon.max())
        if not np.isfinite(top) or not bool(torch.isfinite(recon).all()):
            return "nan"
        if top <= 0.0:
            return "collapsed"
    return "ok"


def fit_volume(volume: np.ndarray, steps: int = 2500, *, seed: Optional[int] = 0, max_reseeds: int = 1, group=None,
               _fault=None, **kwargs) -> Dict[str, object]:
    """``_fit_volume_once`` (the fit itself: arguments there) under the reference's failure rule (``fit_health``): a fit whose
    loss went non-finite or whose reconstruction collapsed to zero is run again from another seed (``seed + 7919 * attempt``: new
    Fourier matrix and new weights, as the reference re-creates its network), at most ``max_reseeds`` times.  The result carries
    ``status`` (FIT_OK, FIT_RESEEDED = healthy after a re-seed, FIT_FAILED = still unhealthy), ``health`` and ``reseeds``.
    A fit shared by a rank group re-seeds on the loss only (every member sees the same all-reduced loss and must take the same
    decision; the reconstruction exists on the group's first rank alone).  ``_fault(attempt)``: test hook (returns "nan" to
    poison that attempt's targets)."""
    attempt = 0
    while True:
        s = None if seed is None else seed + 7919 * attempt
        res = _fit_volume_once(volume, steps, seed=s, group=group, _poison=bool(_fault and _fault(attempt) == "nan"), **kwargs)
        shared = group is not None and inr_dist.is_shared(torch.distributed.get_world_size(group))
        health = fit_health(res.get("final_loss"), None if shared else res.get("_recon_probe"))
        res.pop("_recon_probe", None)
        res["health"], res["reseeds"] = health, attempt
        if health == "ok":
            res["status"] = FIT_RESEEDED if attempt else FIT_OK
            return res
        if attempt >= max_reseeds:
            res["status"] = FIT_FAILED
            return res
        attempt += 1


def _fit_volume_once(volume: np.ndarray, steps: int = 2500, hidden_features: int = 512, hidden_layers: int = 3,
                     mapping_size: int = 128, ff_scale: float = 0.5, lr: float = 1e-4, seed: Optional[int] = 0,
                     downsample: bool = True, upscale_axes: int = 2, evaluate: bool = True, chunk_steps: int = 250,
                     return_recon: bool = True, normalize: bool = True, group=None, _poison: bool = False,
                     lr_model: str = "decimate", footprint=None) -> Dict[str, object]:
    """One INR super-resolution fit of an N-D volume (first ``upscale_axes`` axes are in-plane).

    ``downsample=True``: the volume is the HR ground truth, training uses ``vol[::2, ::2, ...]`` and the result is
    evaluated on the HR grid (PSNR, mean per-slice SSIM by the reference protocol) as well as re-sampled at 2x the
    HR in-plane size.  ``downsample=False``: the volume itself is the training grid and is re-sampled at 2x.
    ``group``: a process group whose ranks fit this ONE volume together, each on its contiguous share of the rows
    (``ShardedSirenFitter``); every member ends with identical weights, only the group's first rank re-samples and
    evaluates (the others return timings and the final loss).
    ``lr_model``: how the training data come from the HR volume.  "decimate" (default): every second sample.  "average" (needs
    ``downsample=True`` and even up-scaled axes): the mean of every 2 x ... block over the up-scaled axes, placed at the block
    centres in the HR grid's ``get_mgrid`` frame, so that the evaluation on ``hr_shape`` is aligned with the data.
    ``footprint``: the forward model of a datum (``footprint.py``).  None (default): a point sample.  "box" (with "average"): the
    block itself, ``Footprint.box`` 2 HR steps wide with 2 samples on every up-scaled axis.  A ``Footprint``: the caller's own rule
    in the coordinates of the training grid (e.g. a Gaussian slice profile along z with ``downsample=False``).  With either
    argument the result gains ``lr_model``, ``footprint_samples`` (K) and ``lr_consistency_psnr_db`` (the forward model's
    prediction against the training data, data range 1).  A footprint cannot be combined with ``group``.
    """
    if lr_model not in ("decimate", "average"):
        raise ValueError(f"lr_model must be 'decimate' or 'average' (got {lr_model!r})")
    if footprint is not None and not isinstance(footprint, Footprint) and footprint != "box":
        raise ValueError(f"footprint must be None, 'box' or a Footprint (got {footprint!r})")
    if footprint is not None and group is not None:
        raise ValueError("a footprint fit cannot be shared by a rank group (group=): the sharded fitter is point-sampled")
    if isinstance(footprint, str) and lr_model != "average":
        raise ValueError("footprint='box' is the 2 x ... block of lr_model='average'")
    vol = np.ascontiguousarray(volume, dtype=np.float32)
    vmax = float(vol.max()) if normalize else 1.0       # superresHybrid normalises per (b, TE) before stacking (:57-63)
    vol = np.ascontiguousarray(vol / vmax)                                                     # superresDWI.py:50-55
    sl = tuple(slice(None, None, 2) if a < upscale_axes else slice(None) for a in range(vol.ndim))
    lr_vol = np.ascontiguousarray(vol[sl]) if downsample else vol
    hr_shape = vol.shape
    if lr_model == "average":
        if not downsample or any(s % 2 for s in hr_shape[:upscale_axes]):
            raise ValueError("lr_model='average' needs downsample=True and even up-scaled axes")
        lr_vol = block_means(vol, upscale_axes)
    if isinstance(footprint, str):
        footprint = block_footprint(hr_shape, upscale_axes)
    if footprint is not None and footprint.dim != vol.ndim:
        raise ValueError(f"the footprint has {footprint.dim} axes, the volume {vol.ndim}")
    test_shape = tuple(2 * s if a < upscale_axes else s for a, s in enumerate(hr_shape))
    # (seeding torch's global generator and drawing the weights from it is one critical section: `run_volumes(concurrent=k)` runs
    #  several fits of this process at once, and each must get the weights its seed gives a fit that runs alone)
    shared = group is not None and inr_dist.is_shared(torch.distributed.get_world_size(group))
    _INIT_LOCK.acquire()
    try:
        if seed is not None:
            torch.manual_seed(seed)
        B = torch.from_numpy(fourier_matrix(vol.ndim, mapping_size, ff_scale, seed)).cuda()
        if not shared:
            model = Siren(2 * mapping_size, hidden_features, hidden_layers, 1).cuda()
    finally:
        _INIT_LOCK.release()
    if shared:
        # one fit, several ranks: everybody uses the first rank's Fourier matrix (the weights follow in the fitter)
        src = torch.distributed.get_global_rank(group, 0)
        if torch.distributed.get_backend(group) == "nccl":
            torch.distributed.broadcast(B, src=src, group=group)
        else:
            Bh = B.cpu()
            torch.distributed.broadcast(Bh, src=src, group=group)
            B.copy_(Bh)
        model = Siren(2 * mapping_size, hidden_features, hidden_layers, 1).cuda()      # (the draw order of a shared fit: B, broadcast, weights)
    if lr_model == "average":
        coords = block_centres(hr_shape, upscale_axes)      # (in the HR grid's frame, not get_mgrid(lr_shape))
        pixels = torch.from_numpy(lr_vol).cuda().reshape(-1, 1)
    else:
        data = ImageFitting_set([lr_vol])
        coords, pixels = data.coords[0], data.pixels[0]
    # built once per fit (superresDWI.py:122)
    model_input = input_mapping(coords, B) if footprint is None else footprint_inputs(coords, B, footprint)
    if _poison:
        pixels = pixels * float("nan")
    data_pixels = pixels        # (all of them: a shared fit trains on its slice)
    g_size = torch.distributed.get_world_size(group) if group is not None else 1
    g_rank = torch.distributed.get_rank(group) if group is not None else 0
    torch.cuda.current_stream().synchronize()      # (this fit's stream: fits may run side by side)
    t0 = time.perf_counter()
    if shared:
        n_rows = model_input.shape[0]
        lo, hi = n_rows * g_rank // g_size, n_rows * (g_rank + 1) // g_size
        model_input, pixels = model_input[lo:hi].contiguous(), pixels[lo:hi].contiguous()
        fitter = ShardedSirenFitter(model, global_rows=n_rows, lr=lr, group=group)
    elif footprint is not None:
        fitter = FootprintSirenFitter(model, footprint, lr=lr)
    else:
        fitter = SirenFitter(model, lr=lr)
    losses = []
    done = 0
    while done < steps:
        k = min(chunk_steps, steps - done)
        losses.append(fitter.step(model_input, pixels, k))
        done += k
        if not bool(torch.isfinite(losses[-1][-1])):     # diverged: the remaining steps cannot bring it back (fit_volume re-seeds)
            break
    torch.cuda.current_stream().synchronize()
    t_fit = time.perf_counter() - t0
    fitter.release_workspace()
    if g_rank != 0:      # a partner of a sharded fit: the group's first rank owns re-sampling and evaluation
        return {"n_coords": int(lr_vol.size), "steps": int(steps), "t_fit": t_fit, "t_recon": 0.0,
                "final_loss": float(torch.cat(losses)[-1]) if steps else None,
                "first_loss": float(losses[0][0]) if steps else None, "model": model, "B": B, "partner": True}
    t0 = time.perf_counter()
    recon = reconstruct(model, test_shape, B)                            # superresDWI.py:125-126,161
    torch.cuda.current_stream().synchronize()
    t_rec = time.perf_counter() - t0
    out: Dict[str, object] = {
        "n_coords": int(lr_vol.size), "steps": int(steps), "t_fit": t_fit, "t_recon": t_rec,
        "train_voxels_per_s": lr_vol.size * steps / t_fit, "recon_voxels_per_s": recon.numel() / t_rec,
        "e2e_voxels_per_s": recon.numel() / (t_fit + t_rec), "final_loss": float(torch.cat(losses)[-1]) if steps else None,
        "first_loss": float(losses[0][0]) if steps else None, "test_shape": test_shape, "scale_back": vmax,
    }
    if lr_model != "decimate" or footprint is not None:
        fp = footprint if footprint is not None else Footprint.point(vol.ndim)
        out["lr_model"], out["footprint_samples"] = lr_model, fp.count
        pred = footprint_forward(model, coords, B, fp)
        out["lr_consistency_psnr_db"] = float(metrics.psnr(data_pixels.reshape(1, -1), pred.reshape(1, -1), 1.0))
    if evaluate and downsample:
        hr = torch.from_numpy(vol).cuda()
        sr = reconstruct(model, hr_shape, B)                             # SR_recon on the HR grid (superresDWI.py:162)
        out["psnr_db"] = float(metrics.psnr(hr, sr, 1.0))
        if vol.ndim >= 2:
            # per 2-D slice over the trailing axes, reference protocol (superresDWI.py:179-186)
            perm = tuple(range(2, vol.ndim)) + (0, 1)
            hs, ss = hr.permute(perm).contiguous(), sr.permute(perm).contiguous()
            ok = hs.amax(dim=(-2, -1)) > 0
            vals = metrics.ssim_reference_protocol(hs[ok].contiguous(), ss[ok].contiguous().clamp_min(1e-30)) \
                if vol.ndim > 2 else metrics.ssim_reference_protocol(hs, ss)
            out["ssim_mean"] = float(vals.mean())
    if return_recon:
        out["recon"] = recon
    out["_recon_probe"] = recon          # (fit_volume's health check; dropped there)
    out["model"] = model
    out["B"] = B
    return out


def acquisition_products(hybrid_raw_norm, te: int = 0) -> np.ndarray:
    """superresDWI.py:57-76 (``Pool(32).starmap(calculate_combinations, ...)`` over every voxel, each task pickling the
    whole volume) as ONE device kernel: ``hybrid_raw_norm[b][te]`` (b = 0: [X, Y, Z] or [X, Y, Z, 1]; b = 1..3:
    [X, Y, Z, n_b]) -> ``acquisitions`` [X, Y, Z, 4, n1*n2*n3] float64 on the host, combination index in
    itertools.product order (SRDWI.py:143-152)."""
    dev = ops.require_gpu()
    raws = [torch.from_numpy(np.ascontiguousarray(hybrid_raw_norm[b][te], dtype=np.float32)).to(dev) for b in range(4)]
    if raws[0].dim() == 4:
        raws[0] = raws[0][..., 0].contiguous()
    return ops.acquisition_products(*raws).cpu().numpy().astype(np.float64)


def fit_with_perturbnet(INR: Siren, B: torch.Tensor, mean_dataset: ImageFitting_set, acquisitions: Sequence[np.ndarray],
                        number_of_epochs: int = 2500, pertubation_epochs: int = 10, PN_dim: int = 128, lr: float = 1e-4,
                        perturb_lr: float = 1e-6, eps: float = 1 / 128., perturb_net: Optional[PN] = None):
    """superresDWI.py:108-156: ``number_of_epochs - pertubation_epochs`` full-batch INR steps on the mean image (one fused
    call), then the alternating tail: odd epochs one more INR step, even epochs one PerturbNet step per acquisition
    (``loss(INR(input_mapping(PN(x, sample, eps))), acquisition_sample)``, Adam lr 1e-6 on the PerturbNet only).
    All K acquisition targets are uploaded once and stay on the device (the reference copies one per step, :148).

    With the SRDWI flavour ``Siren.forward`` detaches its input (SRDWI.py:88): no gradient reaches the PerturbNet and
    ``perturb_optim.step()`` changes nothing -- kept exactly so (the loss is still evaluated).  With
    ``Siren(flavor='INRmodel')`` (INRmodel.py:147, inrDWI.py) the gradient flows INR input -> Fourier features -> PN.
    Returns the per-step INR losses (host list) and leaves the trained PerturbNet in ``fit_with_perturbnet.last_pn``."""
    f = fit_with_perturbnet
    losses, f.last_pn, f.last_pn_losses, _, _ = _fit_perturbnet(
        INR, SirenFitter(INR, lr=lr), B, mean_dataset, acquisitions, number_of_epochs, pertubation_epochs, PN_dim, perturb_lr,
        eps, perturb_net, clear_inr_grads=True)
    return losses


def _fit_perturbnet(INR, fitter, B, mean_dataset, acquisitions, number_of_epochs, pertubation_epochs, PN_dim, perturb_lr, eps,
                    perturb_net, clear_inr_grads):
    """The schedule ``fit_with_perturbnet`` and ``fit_wire_with_perturbnet`` share: ``fitter`` steps ``INR`` on the mean image,
    the PerturbNet is stepped through ``INR``'s autograd function with ``ops.adam_step`` -- only where every one of its tensors
    received a gradient (a SIREN of the SRDWI flavour detaches its input; a WIRE network never does).  ``clear_inr_grads``
    drops what that backward left on ``INR.parameters()``.  Returns ``(INR losses, PerturbNet, its losses, its Adam state --
    the (m, v) pair of each tensor --, its update count)``."""
    model_input = input_mapping(mean_dataset.coords[0], B)
    target = mean_dataset.pixels[0]
    dataset = ImageFitting_set(list(acquisitions))                                        # K device-resident targets
    dimension = len(dataset.shape)
    pn = perturb_net if perturb_net is not None else PN(in_features=model_input.shape[1], hidden_features=PN_dim,
                                                         dimension=dimension).cuda()
    head = max(number_of_epochs - pertubation_epochs, 0)
    losses = [fitter.step(model_input, target, head)] if head else []
    pn_params = [p for p in pn.parameters()]
    pn_state = [(torch.zeros_like(p), torch.zeros_like(p)) for p in pn_params]
    pn_steps, pn_losses = 0, []
    for ctr in range(head, number_of_epochs):
        if ctr % 2:
            losses.append(fitter.step(model_input, target, 1))
            continue
        for sample in range(len(dataset)):
            ground_truth = dataset.pixels[sample]
            perturbed_input = input_mapping(pn(model_input, sample, eps), B)
            model_output = INR(perturbed_input)
            loss = ((model_output - ground_truth) ** 2).mean()
            for p in pn_params:                                                           # perturb_optim.zero_grad()
                p.grad = None
            loss.backward()
            pn_losses.append(loss.detach())
            if all(p.grad is not None for p in pn_params):
                pn_steps += 1
                for p, (m, v) in zip(pn_params, pn_state):                                # perturb_optim.step()
                    ops.adam_step(p.data, p.grad.contiguous(), m, v, pn_steps, perturb_lr)
            if clear_inr_grads:
                for p in INR.parameters():                                                # inr_optim.zero_grad() of the next
                    p.grad = None                                                         # INR step clears these (:136)
    return ([float(v) for v in torch.cat(losses).cpu()] if losses else []), pn, [float(l) for l in pn_losses], pn_state, pn_steps


def fit_wire_with_perturbnet(INR, B: torch.Tensor, mean_dataset: ImageFitting_set, acquisitions: Sequence[np.ndarray],
                             number_of_epochs: int = 2500, pertubation_epochs: int = 3, PN_dim: int = 128, lr: float = 5e-5,
                             perturb_lr: float = 1e-6, eps: float = 1 / 128., perturb_net: Optional[PN] = None, fitter=None):
    """wiretest.ipynb cell 10 for the WIRE network (``wire.Wire``), literally: the first ``number_of_epochs -
    pertubation_epochs`` epochs are plain Adam steps on the mean image (ONE ``WireFitter.step`` call); in the tail, odd epochs
    take one more INR step and even epochs one PerturbNet step per acquisition product --
    ``loss(INR(input_mapping(PN(model_input, sample, eps), B)), acquisition_sample)`` with Adam(``perturb_lr``) on the PerturbNet
    only.  The notebook's network does not detach its input (cell 2), so the gradient really flows WIRE input
    (``inr_wire_input_grad``) -> Fourier features (``_FourierFn``) -> PerturbNet (``_PNFn``); the loss is torch's MSE, the update
    ``ops.adam_step`` on each PerturbNet tensor.  The INR's parameters get no gradient in that branch (the notebook's next
    ``inr_optim.zero_grad()`` would discard it).  All K targets are uploaded once.

    Returns the per-step INR losses (host list); leaves the PerturbNet in ``fit_wire_with_perturbnet.last_pn``, its per-step
    losses in ``.last_pn_losses`` and its Adam state, the ``(m, v)`` pair of each tensor, in ``.last_pn_state`` (``.last_pn_steps``
    counts the updates).  ``fitter``: a ``WireFitter`` of ``INR`` to continue."""
    from . import wire
    f = fit_wire_with_perturbnet
    losses, f.last_pn, f.last_pn_losses, f.last_pn_state, f.last_pn_steps = _fit_perturbnet(
        INR, fitter if fitter is not None else wire.WireFitter(INR, lr=lr), B, mean_dataset, acquisitions, number_of_epochs,
        pertubation_epochs, PN_dim, perturb_lr, eps, perturb_net, clear_inr_grads=False)
    return losses


def _slice_inputs(acquisitions, weights):
    """One direction's acquisitions -> (side, [K, N] device targets ``2*img-1``, [K, N] device weights or None)."""
    imgs = [np.asarray(a, np.float32) for a in acquisitions]
    side = imgs[0].shape[0]
    if any(a.shape != (side, side) for a in imgs):
        raise ValueError("acquisitions must be square 2-D images of one size")
    # all acquisitions resident as ONE [K, N] tensor: a whole epoch (one weighted Adam step per acquisition) -- and every
    # epoch before the averaging window -- is a single call (inr_siren_fit_cycle), not 2 K launches per epoch
    targets = torch.stack([(2.0 * torch.from_numpy(a) - 1.0).reshape(-1) for a in imgs]).cuda()
    wts = None if weights is None else torch.stack([torch.from_numpy(np.asarray(w, np.float32)).reshape(-1)
                                                    for w in weights]).cuda()
    return side, targets, wts


def _fit_slices(models, side, inputs, total_steps, seg, scale, lr, divide_by):
    """The schedule of master.py:130-160 for one or more already drawn models of one side length and one acquisition count:
    one model steps through ``SirenFitter.step_cycle``, several through ``fit_cycle_batch`` (shared persistent launches).
    ``seconds`` is the wall time of the whole group."""
    n_acq = inputs[0][1].shape[0]
    coords = ImageFitting_set([np.zeros((side, side), np.float32)]).coords[0]          # get_mgrid(side, 2)
    fitters = [SirenFitter(model, lr=lr) for model in models]
    predicted = [torch.zeros(side, side, dtype=torch.float64, device="cuda") for _ in models]
    large = [torch.zeros(side * scale, side * scale, dtype=torch.float64, device="cuda") for _ in models]
    targets = [t for _, t, _ in inputs]
    wts = [w for _, _, w in inputs]

    def epochs(n_steps):
        if len(fitters) == 1:
            fitters[0].step_cycle(coords, targets[0], n_steps, wts[0])
        else:
            fit_cycle_batch(fitters, coords, targets, n_steps, weights=wts)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    quiet = max(0, total_steps - seg)                                     # epochs before the first snapshot
    if quiet:
        epochs(quiet * n_acq)
    for step in range(quiet, total_steps):
        epochs(n_acq)
        if step >= total_steps - seg:                                     # master.py:149-160
            for k, model in enumerate(models):
                predicted[k] += reconstruct(model, (side, side), None, clamp_min=None).double()
                large[k] += reconstruct(model, (side * scale, side * scale), None, clamp_min=None).double()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # master.py:162-164 divides by args.seg whatever the number of snapshots taken (step >= total - seg gives seg of them
    # when total_steps >= seg); `divide_by` reproduces that literally
    n_snap = divide_by if divide_by is not None else min(seg, total_steps)
    return [{"predicted": (predicted[k] / max(n_snap, 1)).cpu().numpy(), "large": (large[k] / max(n_snap, 1)).cpu().numpy(),
             "seconds": dt, "optimizer_steps": total_steps * n_acq,
             "train_voxels_per_s": total_steps * n_acq * side * side / dt, "model": model} for k, model in enumerate(models)]


def fit_slice_ensemble(acquisitions: Sequence[np.ndarray], weights: Optional[Sequence[np.ndarray]] = None,
                       total_steps: int = 3000, seg: int = 150, scale: int = 3, hidden_features: int = 64,
                       hidden_layers: int = 6, lr: float = 3e-4, seed: Optional[int] = 0,
                       divide_by: Optional[int] = None) -> Dict[str, object]:
    """master.py:130-160 for one gradient direction: raw 2-D coordinates -> Siren(2, H, L, 1); per epoch one weighted
    Adam step per acquisition (targets are ``2*img-1``, nn_mri.py:174-180); the outputs of the last ``seg`` epochs at
    the native and the x``scale`` grid are averaged.  Returns float64 host arrays like the reference."""
    side, targets, wts = _slice_inputs(acquisitions, weights)
    if seed is not None:
        torch.manual_seed(seed)
    model = Siren(2, hidden_features, hidden_layers, 1).cuda()
    return _fit_slices([model], side, [(side, targets, wts)], total_steps, seg, scale, lr, divide_by)[0]


def fit_slice_ensembles(jobs: Sequence[tuple], total_steps: int = 3000, seg: int = 150, scale: int = 3,
                        hidden_features: int = 64, hidden_layers: int = 6, lr: float = 3e-4, seed: Optional[int] = 0,
                        divide_by: Optional[int] = None) -> List[Dict[str, object]]:
    """``fit_slice_ensemble`` for several directions (``jobs``: a list of ``(acquisitions, weights)``, all of one side
    length) with the fits sharing launches: returns what calling ``fit_slice_ensemble`` on each job in order returns.

    The K models are drawn from torch's global generator in job order before any fitting (after ``torch.manual_seed(seed)``
    per model when ``seed`` is set, as the sequential calls do), so they start from the weights of the sequential run.  The
    persistent kernel advances all problems of a launch in lockstep, so only jobs with the same number of acquisitions fit
    together (``fit_cycle_batch`` over the quiet phase and every window epoch, then ``reconstruct`` per model); a job whose
    acquisition count no other job shares is fitted on its own, sequentially.  ``seconds`` of a job is the wall time of the
    group it was fitted in."""
    jobs = list(jobs)
    if not jobs:
        return []
    inputs = [_slice_inputs(acqs, wts) for acqs, wts in jobs]
    if len({side for side, _, _ in inputs}) > 1:
        raise ValueError("fit_slice_ensembles: all jobs must have one side length")
    models = []
    for _ in jobs:
        if seed is not None:
            torch.manual_seed(seed)
        models.append(Siren(2, hidden_features, hidden_layers, 1).cuda())
    groups: Dict[int, List[int]] = {}
    for k, (_, targets, _) in enumerate(inputs):
        groups.setdefault(int(targets.shape[0]), []).append(k)
    out: List[Optional[Dict[str, object]]] = [None] * len(jobs)
    for members in groups.values():
        res = _fit_slices([models[k] for k in members], inputs[0][0], [inputs[k] for k in members], total_steps, seg, scale,
                          lr, divide_by)
        for k, r in zip(members, res):
            out[k] = r
    return out


RECORD_KEYS = ("job", "n_coords", "steps", "t_fit", "t_recon", "psnr_db", "ssim_mean", "final_loss", "status", "reseeds", "rank",
               "requeued", "first_loss")      # first_loss: the loss of the step-0 weights (a fit's own yardstick for "it went down")


def hybrid_te_groups(world_size: int) -> List[List[int]]:
    """Which ranks fit which of the four echo times (superresHybrid.py:79): with four or more ranks every TE gets its own
    contiguous group (8 ranks: pairs, each pair row-shards its fit); with fewer, TE ``t`` goes to rank ``t % world``."""
    if world_size >= 4:
        return inr_dist._split_ranks(world_size, [1.0] * 4)
    return [[te % max(world_size, 1)] for te in range(4)]


def _sum_over_ranks(t: torch.Tensor) -> None:
    if torch.distributed.get_backend() == "nccl":
        torch.distributed.all_reduce(t)
    else:
        h = t.cpu()
        torch.distributed.all_reduce(h)
        t.copy_(h)


def fit_hybrid(hybrid_raw: np.ndarray, roi: Optional[Sequence[int]] = None, slice_index: Optional[int] = None,
               steps: int = 2500, seed: Optional[int] = 0, distributed: bool = False, gather_recon: bool = False,
               target_dtype=None, estimator: str = "curve_fit", pia_steps: int = 2000, pia_batch: int = 512,
               pia_noise: float = 0.02, pia_lr: float = 1e-4, **fit_kwargs) -> Dict[str, object]:
    """superresHybrid.py:57-140.  ``hybrid_raw``: [X, Y, Z, 4 (b), 4 (TE)].  Per echo time one 4-D INR fit of the
    ROI (LR = every second in-plane voxel, coordinates (x, y, z, b)), re-sampled at twice the ROI size; the 16
    re-scaled images are normalised by the (b=0, TE=0) one (x1000) and one z-slice goes through the three-compartment
    fit.  Returns the device tensor ``recon_hybrid`` [2sx, 2sy, Z, 4, 4] and numpy maps ``D``, ``T2``, ``v``
    [2sx, 2sy, 3] plus timings.

    ``distributed=True`` (inside an initialised process group): the four TE fits are independent, so they are placed on the
    ranks by ``hybrid_te_groups`` (a group of several ranks row-shards its fit); the only exchange is ONE all-reduce of
    the z-slice that feeds the three-compartment fit ([2sx, 2sy, 4, 4]; every rank contributes the echo times it owns,
    zeros elsewhere), after which every rank runs the same hybrid fit.  ``recon_hybrid`` holds the owned echo times only
    unless ``gather_recon`` asks for a second all-reduce of the whole tensor.
    ``target_dtype=np.float16``: the normalised volume is held in half precision (BASELINE config 5) and widened per fit.

    ``estimator="pia"`` replaces the per-voxel least-squares fit of one slice by the amortised estimator of the same maps: a
    ``PIA`` autoencoder is trained for ``pia_steps`` fused steps on ``get_batch(pia_batch, pia_noise)`` batches (``seed`` also
    seeds its initial weights and NumPy's global generator, which ``get_batch`` draws from) and then encodes EVERY voxel of
    the super-resolved volume: ``D``, ``T2``, ``v`` are [2sx, 2sy, Z, 3].  ``pids`` holds the four ``detect_PIDS_slice`` maps
    of slice ``slice_index``; ``pia_loss_before`` / ``pia_loss_after`` the unsupervised loss on one held-out batch before and
    after training, ``model`` the trained ``PIA`` module itself (live, on the device); there is no ``status``.  The two estimators are different methods: their maps are not expected to agree."""
    from . import pia
    if estimator not in ("curve_fit", "pia"):
        raise ValueError(f"estimator must be 'curve_fit' or 'pia', got {estimator!r}")
    raw = np.asarray(hybrid_raw, dtype=np.float32)
    if raw.ndim != 5 or raw.shape[3] != 4 or raw.shape[4] != 4:
        raise ValueError(f"hybrid_raw must be [X, Y, Z, 4, 4], got {raw.shape}")
    x0, x1, y0, y1 = roi if roi is not None else (0, raw.shape[0], 0, raw.shape[1])
    maxes = raw.reshape(-1, 4, 4).max(axis=0)                                              # superresHybrid.py:57-63
    norm = raw / maxes
    sx, sy, nz = x1 - x0, y1 - y0, raw.shape[2]
    recon_hybrid = torch.empty((2 * sx, 2 * sy, nz, 4, 4), dtype=torch.float32, device="cuda")
    scale = torch.from_numpy(maxes).cuda()
    t_fit = t_recon = 0.0
    losses = []
    if target_dtype is not None:
        norm = norm.astype(target_dtype)
    spread = distributed and torch.distributed.is_initialized() and inr_dist.is_shared(torch.distributed.get_world_size())
    if estimator == "pia" and spread and not gather_recon:                                 # before any fit runs
        raise ValueError("estimator='pia' encodes the whole volume: pass gather_recon=True when the echo times are spread")
    rank = torch.distributed.get_rank() if spread else 0
    te_ranks = hybrid_te_groups(torch.distributed.get_world_size()) if spread else [[0]] * 4
    # (group creation is collective over the default group: every rank asks for every group, in the same order; cached)
    te_groups = [inr_dist.rank_group(r) if spread else None for r in te_ranks]
    if spread:
        recon_hybrid.zero_()
    owned = []
    for te in range(4):                                                                    # superresHybrid.py:79
        if rank not in te_ranks[te]:
            losses.append(float("nan"))
            continue
        vol = np.ascontiguousarray(norm[x0:x1, y0:y1, :, :, te], dtype=np.float32)         # (x, y, z, b)
        res = fit_volume(vol, steps=steps, seed=None if seed is None else seed + te, evaluate=False, normalize=False,
                         group=te_groups[te], **fit_kwargs)
        t_fit += res["t_fit"]
        t_recon += res["t_recon"]
        losses.append(res["final_loss"])
        if not res.get("partner"):
            recon_hybrid[..., te] = res["recon"] * scale[:, te]                            # superresHybrid.py:121-122
            owned.append(te)
    k = nz // 2 if slice_index is None else int(slice_index)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if spread:
        if gather_recon:
            _sum_over_ranks(recon_hybrid)
            sl = recon_hybrid[:, :, k].double()
        else:
            plane = recon_hybrid[:, :, k].contiguous()                                     # owned echo times, zeros elsewhere
            _sum_over_ranks(plane)
            sl = plane.double()
    else:
        sl = recon_hybrid[:, :, k].double()                                                # [2sx, 2sy, 4, 4]
    signals = (1000.0 * sl / (sl[..., 0:1, 0:1] + 1e-7)).reshape(-1, 16)                   # superresHybrid.py:131-138
    if estimator == "pia":
        out = _pia_maps(recon_hybrid, signals, (2 * sx, 2 * sy), seed, pia_steps, pia_batch, pia_noise, pia_lr)
        out.update({"recon_hybrid": recon_hybrid, "signals": signals, "t_fit": t_fit, "t_recon": t_recon, "final_losses": losses,
                    "slice_index": k, "owned_te": owned, "estimator": "pia"})
        return out
    fit = pia.hybrid_fit_device(signals)
    x = fit["params"].cpu().numpy()
    t_hybrid = time.perf_counter() - t0
    shape = (2 * sx, 2 * sy, 3)
    v = np.concatenate([x[:, 6:8], 1 - x[:, 6:7] - x[:, 7:8]], axis=1)
    return {"recon_hybrid": recon_hybrid, "signals": signals, "D": x[:, 0:3].reshape(shape), "T2": x[:, 3:6].reshape(shape),
            "v": v.reshape(shape), "status": fit["status"].cpu().numpy().reshape(shape[:2]), "t_fit": t_fit,
            "t_recon": t_recon, "t_hybrid_fit": t_hybrid, "final_losses": losses, "slice_index": k, "owned_te": owned}


def _pia_maps(recon_hybrid, slice_signals, plane, seed, steps, batch, noise, lr):
    """The ``estimator="pia"`` half of ``fit_hybrid``: train a PIA on synthetic batches, encode the whole volume."""
    from . import pia, pia_net
    if seed is not None:
        torch.manual_seed(seed)
        np.random.seed(seed)
    model = pia_net.PIA().cuda()
    fitter = pia_net.PiaFitter(model, lr=lr)
    held_out = pia_net.get_batch(batch, noise)[0].cuda()

    def held_out_loss():
        with torch.no_grad():
            return float(model.loss_function(model(held_out)[0], held_out, 1.0))

    before = held_out_loss()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step_losses = [fitter.step(pia_net.get_batch(batch, noise)[0].cuda()) for _ in range(int(steps))]
    torch.cuda.synchronize()
    t_train = time.perf_counter() - t0
    after = held_out_loss()
    vol = recon_hybrid.reshape(recon_hybrid.shape[:3] + (16,))
    vol_signals = (1000.0 * vol / (vol[..., 0:1] + 1e-7)).contiguous()                     # superresHybrid.py:131-138, every voxel
    t0 = time.perf_counter()
    D, T2, v = fitter.encode_volume(vol_signals)
    torch.cuda.synchronize()
    t_encode = time.perf_counter() - t0
    maps = pia_net.detect_PIDS_slice(np.asarray(pia.BVALS), slice_signals.reshape(plane + (4, 4)).cpu().numpy())
    return {"D": D.cpu().numpy(), "T2": T2.cpu().numpy(), "v": v.cpu().numpy(),
            "pids": dict(zip(("PIDS_ADC1", "PIDS_ADC2", "PIDS_b_decay", "PIDS_TE_decay"), maps)),
            "pia_loss_before": before, "pia_loss_after": after,
            "pia_step_losses": torch.cat(step_losses).cpu().numpy() if step_losses else np.zeros(0, np.float32),
            "t_pia_train": t_train, "t_pia_encode": t_encode, "t_hybrid_fit": t_train + t_encode, "model": model}


def plan_volumes(volumes: Sequence[np.ndarray], steps: int, world: int, allow_sharding: bool = True, **fit_kwargs):
    """The schedule ``run_volumes`` follows (same on every rank, no communication).  For the reference's network
    (Siren(256, 512, 3, 1): the defaults of ``fit_volume``) the planner prices a job with the MEASURED step-time table of
    ``dist.StepTimeModel`` -- a step is not linear in the rows, which is what decides whether row-sharding pays -- otherwise
    with rows x steps."""
    rows = [float(np.prod([-(-s // 2) if a < 2 else s for a, s in enumerate(v.shape)])) for v in volumes]
    costs = [r * steps for r in rows]
    # priced by the measured step-time table for the reference's network, by the linear model derived from it for any other shape
    # (dist.StepTimeModel.for_network); a job list that does not train on the half-resolution grid keeps rows x steps
    shard_time = None
    if fit_kwargs.get("downsample", True):
        model = inr_dist.StepTimeModel.for_network(2 * fit_kwargs.get("mapping_size", 128), fit_kwargs.get("hidden_features", 512),
                                                   fit_kwargs.get("hidden_layers", 3))
        shard_time = lambda j, k: model.fit_seconds(rows[j], steps, k)     # noqa: E731
    if allow_sharding and world > 1:
        plan = inr_dist.plan_fits(costs, world, shard_time=shard_time)
    else:
        whole = inr_dist.partition_fits([shard_time(j, 1) for j in range(len(rows))] if shard_time else costs, world)
        t = (lambda j: shard_time(j, 1)) if shard_time else (lambda j: costs[j])
        loads = [sum(t(j) for j in jobs) for jobs in whole]
        plan = {"gangs": [], "whole": whole, "makespan": max(loads, default=0.0), "loads": loads}
    plan["one_rank"] = sum(shard_time(j, 1) for j in range(len(rows))) if shard_time else sum(costs)
    plan["unit"] = "seconds (measured step-time table, modelled all-reduce)" if shard_time else "rows x steps"
    return plan


class FitError(RuntimeError):
    """``run_volumes``: fits that raised on their rank and that no surviving rank could take over (``.records`` = all records)."""

    def __init__(self, message, records):
        super().__init__(message)
        self.records = records


def run_volumes(volumes: Sequence[np.ndarray], steps: int = 2500, allow_sharding: bool = True, stats: Optional[dict] = None,
                fit_fn=None, requeue: bool = True, concurrent: int = 1, errors: str = "raise", plan: Optional[dict] = None,
                **fit_kwargs) -> List[Dict[str, float]]:
    """Fits every volume once over the ranks of the current process group and returns the gathered per-fit metric
    records on every rank (one RCCL all_gather).  Schedule: ``plan_volumes`` / ``dist.plan_fits`` -- the volumes that do not
    fill a whole round are fitted first, each row-sharded over its own group of ranks, the rest are packed whole (LPT);
    ``allow_sharding=False`` is plain LPT packing (no collective on the data path at all).  ``stats`` (a dict) receives the
    plan and this rank's busy seconds.  ``plan``: a schedule of ``dist.plan_fits`` form (``{"gangs": [(job, ranks), ...], "whole": [[job,
    ...] per rank]}``) to follow instead of the one ``plan_volumes`` would price -- every rank must pass the same one.

    Failure handling (the job list is idempotent -- one record per fit).  Every record carries ``status``:
    FIT_OK, FIT_RESEEDED (the fit diverged or collapsed and a re-seeded run was healthy: ``fit_volume``), FIT_FAILED (unhealthy
    after the re-seeds: kept, marked, metrics as measured) or FIT_ERROR (the fit RAISED on its rank -- a device error, an
    allocation failure).  With ``requeue`` the whole-volume fits that ended in FIT_ERROR are dealt, longest first, to the ranks
    that reported no error (the survivors; every rank derives the same assignment from the gathered records), run there and
    gathered once more; ``requeued`` = 1 marks their records.  Only RUNTIME failures are turned into records (``RuntimeError`` and
    its subclasses: device errors, ``InrHipError``, ``torch.cuda.OutOfMemoryError``); a programming error (``TypeError`` from a bad
    keyword, ``ValueError``, ...) propagates at once, as does any failure when this process is the whole job (world 1: nobody could
    take the fit over, the first exception is re-raised after the loop).  ``errors="raise"`` (default): records still FIT_ERROR after
    the re-queue raise ``FitError`` on every rank (all ranks hold the same gathered records, so all raise); ``errors="record"`` returns
    them, NaN metrics and all.  A fit shared by a rank group is not re-queued: a member that
    raises mid-fit leaves its partners in the gradient all-reduce, which this layer cannot repair -- the exception propagates.
    ``fit_fn(volume, steps=..., return_recon=False, **fit_kwargs)`` replaces ``fit_volume`` (tests of the scheduling itself).

    ``concurrent`` (default 1): whole-volume fits a rank runs side by side, each on a host thread and HIP stream of its own.  A fit
    of a few thousand rows keeps a chip busy a fifth of the time (one 64 x 128 tile per CU and launch, 13 launches per step): two at
    once measured 1.41 x the aggregate rate at 4,096 rows, 1.26 x at 16,384 (``tools/concurrent_small.py``); volumes that fill the
    chip gain nothing.  Every fit keeps the bits it has alone (seeded draws are one critical section, kernels are per stream)."""
    world = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
    rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
    fit = fit_fn or fit_volume
    if plan is None:
        plan = plan_volumes(volumes, steps, world, allow_sharding, **fit_kwargs)
    else:
        jobs = sorted([j for j, _ in plan["gangs"]] + [j for w in plan["whole"] for j in w])
        if jobs != list(range(len(volumes))) or len(plan["whole"]) != world:
            raise ValueError("plan must place every volume exactly once and list the whole-volume jobs of every rank")
    local = []
    t_start = time.perf_counter()
    nan = float("nan")

    def record(job, res, requeued=0.0):
        local.append({"job": job, "n_coords": res["n_coords"], "steps": steps, "t_fit": res["t_fit"],
                      "t_recon": res["t_recon"], "psnr_db": res.get("psnr_db", nan),
                      "ssim_mean": res.get("ssim_mean", nan),
                      "final_loss": nan if res.get("final_loss") is None else res["final_loss"],
                      "first_loss": nan if res.get("first_loss") is None else res["first_loss"],
                      "status": float(res.get("status", FIT_OK)), "reseeds": float(res.get("reseeds", 0)), "rank": float(rank),
                      "requeued": requeued})

    if errors not in ("raise", "record"):
        raise ValueError(f"errors must be 'raise' or 'record', got {errors!r}")
    raised = []

    def run_whole(job, requeued=0.0):
        try:
            record(job, fit(volumes[job], steps=steps, return_recon=False, **fit_kwargs), requeued)
        except RuntimeError as e:      # device / library / allocation failures; the record says so, the survivors take the job over
            import sys
            raised.append(e)
            print(f"[run_volumes] rank {rank}: fit of volume {job} raised {type(e).__name__}: {e}", file=sys.stderr)
            record(job, {"n_coords": float(np.asarray(volumes[job]).size), "t_fit": nan, "t_recon": nan, "final_loss": nan,
                         "status": FIT_ERROR}, requeued)

    # gang phase: every rank creates every group (new_group is collective over the default group), then works in its own
    groups = [(job, ranks, inr_dist.rank_group(ranks)) for job, ranks in plan["gangs"]]
    for job, ranks, grp in groups:
        if rank in ranks:
            res = fit(volumes[job], steps=steps, return_recon=False, group=grp, **fit_kwargs)
            if not res.get("partner"):
                record(job, res)
    whole = list(plan["whole"][rank])
    # (networks small enough for the persistent cooperative kernel -- grid barriers over co-resident blocks: siren_small.hip -- are
    #  never run side by side: two such launches could each hold part of the chip and wait for the rest.  Small fits share the
    #  chip safely only inside ONE cooperative launch: inr.fit_cycle_batch / fit_slice_ensembles, inr_siren_fit_cycle_batch)
    cooperative = fit_kwargs.get("hidden_features", 512) in (32, 64) and 2 * fit_kwargs.get("mapping_size", 128) <= 32
    if int(concurrent) > 1 and len(whole) > 1 and torch.cuda.is_available() and not cooperative:
        from concurrent.futures import ThreadPoolExecutor
        first = len(local)
        tls = threading.local()

        def on_own_stream(job):
            if not hasattr(tls, "stream"):
                tls.stream = torch.cuda.Stream()
            with torch.cuda.stream(tls.stream):
                run_whole(job)
                tls.stream.synchronize()

        torch.cuda.synchronize()                           # (the side streams start behind whatever the caller enqueued)
        with ThreadPoolExecutor(max_workers=min(int(concurrent), len(whole))) as pool:
            list(pool.map(on_own_stream, whole))
        local[first:] = sorted(local[first:], key=lambda r: whole.index(r["job"]))      # (records in the order of the sequential run)
    else:
        for job in whole:
            run_whole(job)
    if stats is not None:
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        stats["busy_s"] = time.perf_counter() - t_start
        stats["plan"] = plan
    max_jobs = max((len(p) for p in plan["whole"]), default=0) + 1
    records = inr_dist.gather_job_records(local, RECORD_KEYS, max_jobs)
    failed = sorted((r for r in records if r["status"] == FIT_ERROR), key=lambda r: (-r["n_coords"], r["job"]))
    if requeue and failed:
        bad_ranks = {int(r["rank"]) for r in failed}
        survivors = [k for k in range(world) if k not in bad_ranks]
        if survivors:
            busy = {k: sum(r["t_fit"] for r in records if int(r["rank"]) == k and r["t_fit"] == r["t_fit"]) for k in survivors}
            mine = []
            for r in failed:                               # longest first, each to the survivor that is free first
                k = min(survivors, key=lambda q: (busy[q], q))
                busy[k] += r["n_coords"] * steps / 5.5e7      # (seconds at the fused step's ~55 M coordinate-steps/s)
                if k == rank:
                    mine.append(int(r["job"]))
            local.clear()
            for job in mine:
                run_whole(job, requeued=1.0)
            second = inr_dist.gather_job_records(local, RECORD_KEYS, len(failed))
            redone = {int(r["job"]): r for r in second}
            records = [redone.get(int(r["job"]), r) if r["status"] == FIT_ERROR else r for r in records]
            if stats is not None:
                stats["requeued"] = sorted(redone)
    records = sorted(records, key=lambda r: r["job"])
    still = [int(r["job"]) for r in records if r["status"] == FIT_ERROR]
    if still and errors == "raise":
        if world == 1 and raised:
            raise raised[0]                                # single process: the caller sees the exception itself
        raise FitError(f"run_volumes: fits of volumes {still} raised and no rank could take them over "
                       f"(errors='record' returns the NaN records instead)", records)
    return records


# ---------------------------------------------------------------------------------------------------
# INR_ERD.py:170-303 -- the soft-ERD INR of one (seed, case): pre-train on the soft-ERD mean image, one dual-learning-rate
# fine-tuning step on the weighted acquisitions, mean reconstruction, four rows of SNR / CNR figures
# ---------------------------------------------------------------------------------------------------
def erd_inr_case(case, seed, scale=1, hidden_features=128, hidden_layers=3, pretrain_lr=3e-4, threshold=2e-5, max_steps=None,
                 finetune_steps=1, lr_perturb=3e-4, lr_net=1e-7, perturb_eps=1.0 / 128.0, mul=1000, slope=20):
    """``case`` carries ``pt_id, b, cancer_loc, contralateral_loc, noise, cancer_slice`` and the arrays ``b0`` [X, Y, Z] and
    ``b3`` [X, Y, Z, K].  Returns ``(rows, info)``: the four CSV rows of INR_ERD.py:293-296 and what the fit did.  Targets are
    normalised as the reference's dataset does (nn_mri.py:174-180: pixel -> 2 pixel - 1).  ``scale`` > 1 evaluates the mean
    reconstruction on a ``scale`` times finer grid (the landmarks scale with it); 1 is the reference's grid.
    One difference from INR_ERD.py as written, beside the collapse-wins rule of the pre-training loop: the model is built with
    ``perturb=True``, so the fine-tuning step and the mean reconstruction run with the coordinate perturbation
    (prepare_qual_images.py's behaviour).  INR_ERD.py builds its ``Siren`` with ``perturb=False`` and never switches it on: there
    both run unperturbed and the ``perturb_linear*`` tensors never move."""
    from . import erd_inr

    dev = ops.require_gpu()
    sl = case.cancer_slice
    b = case.b[3]
    b0 = np.asarray(case.b0[:, :, sl], dtype=np.float64)
    dwi = np.asarray(case.b3[:, :, sl, :], dtype=np.float64)
    K = dwi.shape[-1]
    level = erd_inr.noise_level(case.b3, case.noise, sl)
    weights, mean_image = erd_inr.soft_erd(dwi, b0, level, mul=mul, slope=slope)

    model = erd_inr.ErdSiren(in_features=2, out_features=1, hidden_features=hidden_features, hidden_layers=hidden_layers,
                             perturb=True).to(dev)
    fitter = erd_inr.ErdFitter(model)
    coords = ops.mgrid(b0.shape)
    norm = lambda a: torch.from_numpy(2.0 * np.asarray(a, dtype=np.float32) - 1.0).reshape(-1).to(dev)      # noqa: E731
    pre = fitter.pretrain(coords, norm(mean_image), lr=pretrain_lr, threshold=threshold, max_steps=max_steps)
    targets = torch.stack([norm(dwi[:, :, a]) for a in range(K)])
    wts = torch.stack([torch.from_numpy(weights[:, :, a].astype(np.float32)).reshape(-1) for a in range(K)]).to(dev)
    losses = fitter.finetune(coords, targets, wts, steps=finetune_steps, lr_perturb=lr_perturb, lr_net=lr_net, eps=perturb_eps)

    img = dwi.mean(-1)
    out_shape = tuple(int(s) * int(scale) for s in b0.shape)
    mean_recon = fitter.mean_reconstruction(out_shape, K, eps=perturb_eps)
    adc_in = erd_inr.calc_adc(img, b0, b)
    b0_out = b0 if scale == 1 else np.kron(b0, np.ones((scale, scale)))
    adc_out = erd_inr.calc_adc(mean_recon, b0_out, b)

    from types import SimpleNamespace
    scaled = SimpleNamespace(cancer_loc=tuple(int(v) * int(scale) for v in case.cancer_loc),
                             contralateral_loc=tuple(int(v) * int(scale) for v in case.contralateral_loc),
                             noise=tuple(int(v) * int(scale) for v in case.noise))
    rows = []
    for image, at, kind, tag, digits in ((img, case, "DWI", "orig", 3), (mean_recon, scaled, "DWI", "recon", 3),
                                         (adc_in, case, "ADC", "orig", 3), (adc_out, scaled, "ADC", "recon", 4)):
        rows.append([str(seed)] + [round(float(v), digits) for v in erd_inr.calculate_CNR_SNR(at, image)] + [case.pt_id, kind, tag])
    info = {"pretrain": pre, "finetune_loss": float(losses[-1]) if finetune_steps else float("nan"), "noise_level": float(level),
            "mean_recon": mean_recon, "model": model}
    return rows, info


# ---------------------------------------------------------------------------------------------------
# prepare_qual_images.py:147-300 -- the low-resolution (reader) study of one slice: fit the soft-ERD INR to the half-resolution
# acquisitions, re-sample it on the full grid, and set it beside the low-resolution image, its interpolation and the full image
# ---------------------------------------------------------------------------------------------------
QUAL_PANELS = ("low", "interpolated", "SR", "base")


def low_res_study(case, slice_index, seed, hidden_features=128, hidden_layers=3, pretrain_lr=3e-4, threshold=2e-5,
                  max_steps=None, finetune_steps=502, lr_perturb=1e-5, lr_net=1e-7, perturb_eps=1.0 / 128.0, mul=1000, slope=20):
    """``case`` as for ``erd_inr_case``; ``slice_index`` the slice of ``b0`` [X, Y, Z] / ``b3`` [X, Y, Z, K] to study.  Returns
    ``(maps, label, info)``:

    ``maps``: float64 images ``low`` (the acquisition mean down-scaled by 0.5 with the anti-aliasing Gaussian,
    ``baselines.rescale2d``), ``interpolated`` (``low`` re-sampled linearly to the full grid), ``SR`` (the mean over acquisitions of the
    fitted network on the full grid) and ``base`` (the acquisition mean itself), and the ADC maps ``adc_low, adc_interpolated,
    adc_superres, adc_gold`` of prepare_qual_images.py:266-273 -- the two full-grid ones of the low-resolution data against the
    down- and up-scaled ``b0``, the gold one against ``b0``.
    ``label``: ``{"pt", "image", "1" .. "4"}``, the row of ``labels.csv`` without its file name: the four panel names in an order
    drawn from ``random.Random`` seeded with (``seed``, patient, slice).
    ``info``: what the fit did.

    The model is pre-trained on ``low`` (threshold 2e-5), the soft-ERD weights come from the low-resolution stack with the noise
    level of the FULL-resolution ``b3`` at the cancer slice (as the script takes it), and ``finetune_steps`` = 502 steps run at
    1e-5 / 1e-7 with ``eps = 1/128``.  As in ``erd_inr_case``: targets are normalised pixel -> 2 pixel - 1 (nn_mri.py:174-180) and
    the network's output is used as it is; a pre-training step that both converges and collapses counts as a collapse.
    Where this differs from the script: the full grid is the slice's own shape, not the constant 128 (the two coincide on the
    script's 128 x 128 data), so ``interpolated`` and the up-scaled ``b0`` are ``resize`` to that shape -- ``rescale(., 2)`` whenever
    the sides are even; the script's unseeded ``random.sample`` is seeded; and the PNG figure is not drawn."""
    import random

    from . import baselines, erd_inr

    dev = ops.require_gpu()
    sl = int(slice_index)
    b = case.b[3]
    b0 = np.asarray(case.b0[:, :, sl], dtype=np.float64)
    dwi = np.asarray(case.b3[:, :, sl, :], dtype=np.float64)
    K = dwi.shape[-1]
    base = dwi.mean(-1)
    # every image is a skimage call of its own (its own clip range): the mean, the K acquisitions, b0 -- one launch chain
    stack = np.concatenate([base[None], np.moveaxis(dwi, -1, 0), b0[None]])
    out_hw = np.round(0.5 * np.asarray(base.shape, dtype=np.float64)).astype(np.int64)
    lows = baselines._resize("low_res_study", stack, out_hw, 1, "reflect", True, True, group_axes=0)
    low, low_all, b0_low = lows[0], np.moveaxis(lows[1:K + 1], 0, -1), lows[K + 1]
    level = erd_inr.noise_level(case.b3, case.noise, case.cancer_slice)
    weights, _ = erd_inr.soft_erd(low_all, b0_low, level, mul=mul, slope=slope)

    model = erd_inr.ErdSiren(in_features=2, out_features=1, hidden_features=hidden_features, hidden_layers=hidden_layers,
                             perturb=True).to(dev)
    fitter = erd_inr.ErdFitter(model)
    coords = ops.mgrid(low.shape)
    norm = lambda a: torch.from_numpy(2.0 * np.asarray(a, dtype=np.float32) - 1.0).reshape(-1).to(dev)      # noqa: E731
    pre = fitter.pretrain(coords, norm(low), lr=pretrain_lr, threshold=threshold, max_steps=max_steps)
    targets = torch.stack([norm(low_all[:, :, a]) for a in range(K)])
    wts = torch.stack([torch.from_numpy(weights[:, :, a].astype(np.float32)).reshape(-1) for a in range(K)]).to(dev)
    losses = fitter.finetune(coords, targets, wts, steps=finetune_steps, lr_perturb=lr_perturb, lr_net=lr_net, eps=perturb_eps)
    sr = fitter.mean_reconstruction(base.shape, K, eps=perturb_eps)

    ups = baselines._resize("low_res_study", np.stack([low, b0_low]), base.shape, 1, "reflect", True, True, group_axes=0)
    interpolated, b0_up = ups[0], ups[1]
    maps = {"low": low, "interpolated": interpolated, "SR": sr, "base": base,
            "adc_low": erd_inr.calc_adc(low, b0_low, b), "adc_interpolated": erd_inr.calc_adc(interpolated, b0_up, b),
            "adc_superres": erd_inr.calc_adc(sr, b0_up, b), "adc_gold": erd_inr.calc_adc(base, b0, b)}
    order = random.Random(f"{seed}:{case.pt_id}:{sl}").sample(range(4), 4)          # prepare_qual_images.py:276
    label = {"pt": case.pt_id, "image": str(sl)}
    label.update({str(order[k] + 1): QUAL_PANELS[k] for k in range(4)})
    info = {"pretrain": pre, "finetune_loss": float(losses[-1]) if finetune_steps else float("nan"), "noise_level": float(level),
            "b0_low": b0_low, "b0_up": b0_up, "model": model}
    return maps, label, info


# ---------------------------------------------------------------------------------------------------
# david.py:31-91 -- AutoERD on whole slices, the plain and the ERD-accepted mean of every gradient direction, their ADC maps and
# the lesion-contrast table
# ---------------------------------------------------------------------------------------------------
DAVID_METRICS = ("C", "CNR")
DAVID_DIRECTIONS = ("x", "y", "z")


def david_rows(case, res, k: int):
    """The rows of david.py:70-91 -- ``(image, direction, acquisition, metric, value)`` in the reference's order -- from maps laid
    out as ``erd.erd_volume`` returns them for ``case.dwi[:, :, slices, :]``; ``k`` is the cancer slice's position in ``slices``.
    Host-side: ``contrast.calculate_contrast(case, 1, image, 0)`` per image."""
    from . import contrast

    sizes = [int(g) for g in np.asarray(case.acquisitions).reshape(-1)]
    rows = []
    first = 0
    for g, size in enumerate(sizes):
        name = DAVID_DIRECTIONS[g] if g < len(DAVID_DIRECTIONS) else str(g)
        for acq in range(first, first + size):
            images = (("DWI", np.asarray(case.dwi)[:, :, case.cancer_slice, acq]), ("ADC", res.adc[:, :, k, acq]))
            values = [contrast.calculate_contrast(case, 1, im, 0) for _, im in images]
            for inx, metric in enumerate(DAVID_METRICS):
                rows.extend((image, name, acq, metric, v[inx]) for (image, _), v in zip(images, values))
        first += size
        images = (("DWI", res.direction_mean[g, :, :, k]), ("ADC", res.direction_adc[g, :, :, k]),
                  ("DWI_ERD", res.accepted_mean[g, :, :, k]), ("ADC_ERD", res.accepted_adc[g, :, :, k]))
        values = [contrast.calculate_contrast(case, 1, im, 0) for _, im in images]
        for inx, metric in enumerate(DAVID_METRICS):
            rows.extend((image, name, "mean", metric, v[inx]) for (image, _), v in zip(images, values))
    return rows


def david_study(case, rule: int = 1, slices="cancer"):
    """``case`` is a ``contrast.case``.  One ``erd.erd_volume`` call over ``slices`` (``"cancer"``, ``"all"`` or slice indices,
    which must include the cancer slice: the landmarks of the table belong to it) clusters every pixel (``rule`` 1 or 2; 0 uses
    ``case.accept`` as it is), clears ``case.accept`` for the rejected acquisitions as david.py:55 does, and forms the means and
    ADC maps.  The contrast numbers are computed host-side with ``contrast.calculate_contrast(case, 1, image, 0)`` on the cancer
    slice, as the reference does.  Returns ``{"rows", "maps", "slices"}``: ``rows`` are ``(image, direction, acquisition, metric,
    value)`` in the reference's order (david.py:70-91); ``maps`` holds float64 ``direction_mean, accepted_mean, direction_adc,
    accepted_adc`` [G, X, Y, len(slices)], ``adc`` [X, Y, len(slices), n] and ``accept`` (as ``erd_volume`` returns it)."""
    from . import erd

    idx = erd.case_slices(case, slices)
    if int(case.cancer_slice) not in idx:
        raise ValueError(f"slices {idx} must include the cancer slice {case.cancer_slice}: the contrast landmarks belong to it")
    emap = accept = None
    if rule == 2:
        if case.erd is None:
            raise ValueError("--erd 2 needs the patient's ERD map (pat<NN>_ERD.mat: ADC_alldata_mm_ERD)")
        emap = np.asarray(case.erd)[:, :, idx]
    if rule == 0:
        accept = np.asarray(case.accept)[:, :, idx, :]
    res = erd.erd_volume(np.asarray(case.dwi)[:, :, idx, :], np.asarray(case.b0)[:, :, idx], case.acquisitions, case.b, rule=rule,
                         erd_map=emap, accept=accept, per_acquisition_adc=True)
    if rule != 0:
        block = case.accept[:, :, idx, :]
        block[res.accept == 0] = 0
        case.accept[:, :, idx, :] = block
    rows = david_rows(case, res, idx.index(int(case.cancer_slice)))
    return {"rows": rows, "maps": res._asdict(), "slices": idx}


# ---------------------------------------------------------------------------------------------------
# The through-plane study: thick slices from thin ones by a slice profile, and back by four methods -- scored, since
# here the thin slices are the ground truth that ``--transverse_length`` never had
# ---------------------------------------------------------------------------------------------------
THROUGH_PLANE_METHODS = ("replicate", "spline", "zerofill", "tv3d")


NLM_STARTS = ("replicate", "spline")


def check_through_plane(factor=2, profile="mean", fwhm=None, tv_lambda=3e-3, tv_huber=0.1, tv_iters=300, tv_gz=1.0, with_inr=False,
                        footprint="point", number_of_epochs=2500, with_nlm=False, nlm_start="replicate", nlm_iters=2, nlm_search=2,
                        nlm_patch=1):
    """What ``through_plane_study`` cannot serve, by name; touches neither the input nor the device."""
    who = "through_plane_study"
    if with_nlm:
        from . import baselines
        if nlm_start not in NLM_STARTS:
            raise ValueError(f"{who}: nlm_start must be 'replicate' or 'spline' (got {nlm_start!r})")
        ops.nlm_radii(who, nlm_search, nlm_patch)
        ops.nlm_schedule(who, baselines.NLM_DEFAULT_LEVELS, nlm_iters, 1.0)
    if int(factor) != factor or not 2 <= factor <= ops.TVSR_MAX_FACTOR:
        raise ValueError(f"{who}: factor is the number of thin slices per thick one, 2 .. {ops.TVSR_MAX_FACTOR} (got {factor!r})")
    if profile not in ("mean", "gaussian"):
        raise ValueError(f"{who}: profile must be 'mean' or 'gaussian' (got {profile!r})")
    if profile == "gaussian" and (fwhm is None or not 0.0 < float(fwhm) < float("inf")):
        raise ValueError(f"{who}: the gaussian profile needs a finite fwhm > 0, in thick slices (got {fwhm!r})")
    for name, value in (("tv_lambda", tv_lambda), ("tv_huber", tv_huber), ("tv_gz", tv_gz)):
        if not 0.0 <= float(value) < float("inf"):
            raise ValueError(f"{who}: {name} must be finite and >= 0 (got {value!r})")
    if int(tv_iters) != tv_iters or not 1 <= tv_iters <= ops.TVSR3D_MAX_ITER:
        raise ValueError(f"{who}: tv_iters must be 1 .. 100,000 (got {tv_iters!r})")
    if footprint not in ("point", "box"):
        raise ValueError(f"{who}: footprint must be 'point' or 'box' (got {footprint!r})")
    if with_inr:
        if factor != 2 or profile != "mean":
            raise ValueError(f"{who}: with_inr fits fit_volume's lr_model='average', the mean of 2 slices: factor 2 and the mean "
                             f"profile only (got factor {factor}, profile {profile!r})")
        if int(number_of_epochs) != number_of_epochs or number_of_epochs < 1:
            raise ValueError(f"{who}: number_of_epochs must be >= 1 (got {number_of_epochs!r})")


def through_plane_study(volume, factor=2, profile="mean", fwhm=None, tv_lambda=None, tv_huber=None, tv_iters=None, tv_gz=1.0,
                        with_inr=False, footprint="point", number_of_epochs=2500, seed=0, with_nlm=False, nlm_start="replicate",
                        nlm_iters=None, nlm_search=None, nlm_patch=None):
    """``volume`` [X, Y, Z, B] (or [X, Y, Z]) in [0, 1], thin slices along Z: the thick slices ``block_apply3d(HR, (factor, 1, 1),
    profile)`` of Z trimmed to a multiple of ``factor``, and their reconstructions on the thin slices, all on the device:
    ``replicate`` (every thick slice ``factor`` times), ``spline`` (``baselines.resize_z``, the cubic spline along z of
    ``--transverse_length``), ``zerofill`` (``baselines.fourier_resample`` along z, ``align='center'``, ``boundary='mirror'``,
    clamped at 0) and ``tv3d`` (``baselines.tv_superres3d`` with the profile in its operator and gradient weights ``(tv_gz, 1, 1)``;
    the ``TV3D_DEFAULT_*`` where an argument is None).  ``with_inr``: also ``sr``, ``fit_volume`` as it is on the z-first volume
    (``upscale_axes=1, lr_model='average'``, ``footprint`` 'point' -> None or 'box'), for factor 2 and the mean profile only.
    Returns ``{"volumes", "psnr", "ssim", "consistency", "kernel"}``: fp32 device stacks [Z, B, X, Y] (``hr``, ``thick`` [Z /
    factor, ...] and the methods), PSNR (data range 1) and SSIM by the reference protocol [Z, B] per method, and the PSNR of
    ``A tv3d`` against the thick slices.  ``with_nlm``: also ``nlm``, ``baselines.nlm_upsample`` with the profile in its mean
    correction, ``NLM_DEFAULT_LEVELS`` and ``nlm_iters`` passes per level (the ``NLM_DEFAULT_*`` where an argument is None), from the
    replication (``nlm_start='replicate'``) or from the spline above after one mean correction (``'spline'``); the result gains
    ``nlm_consistency``, the PSNR of ``A nlm`` against the thick slices."""
    from . import baselines

    lam = baselines.TV3D_DEFAULT_LAMBDA if tv_lambda is None else tv_lambda
    huber = baselines.TV3D_DEFAULT_HUBER if tv_huber is None else tv_huber
    iters = baselines.TV3D_DEFAULT_ITERS if tv_iters is None else tv_iters
    n_iters = baselines.NLM_DEFAULT_ITERS if nlm_iters is None else nlm_iters
    n_search = baselines.NLM_DEFAULT_SEARCH if nlm_search is None else nlm_search
    n_patch = baselines.NLM_DEFAULT_PATCH if nlm_patch is None else nlm_patch
    check_through_plane(factor, profile, fwhm, lam, huber, iters, tv_gz, with_inr, footprint, number_of_epochs, with_nlm, nlm_start,
                        n_iters, n_search, n_patch)
    vol = np.asarray(volume)
    if vol.ndim == 3:
        vol = vol[..., None]
    if vol.ndim != 4:
        raise ValueError(f"through_plane_study: the volume is [X, Y, Z, B] or [X, Y, Z] (got {vol.shape})")
    Z = vol.shape[2] - vol.shape[2] % factor
    if Z // factor < 4:
        raise ValueError(f"through_plane_study: {vol.shape[2]} slices make {Z // factor} thick slices of {factor}; the cubic spline along z "
                         f"needs at least 4")
    vol = vol[:, :, :Z]
    dev = ops.require_gpu()
    hr = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(dev).permute(3, 2, 0, 1).contiguous()     # [B, Z, X, Y]
    kernel = (baselines.slice_profile(factor, profile, fwhm if profile == "gaussian" else None), np.ones(1), np.ones(1))
    f = (factor, 1, 1)
    thick = baselines.block_apply3d(hr, f, kernel)
    recon = {"replicate": thick.repeat_interleave(factor, dim=1),
             "spline": baselines.resize_z(thick.permute(0, 2, 3, 1).contiguous(), Z).permute(0, 3, 1, 2).float().contiguous(),
             "zerofill": baselines.fourier_resample(thick, Z, axis=1, align="center", boundary="mirror").clamp_min(0),
             "tv3d": baselines.tv_superres3d(thick, f, kernel, lam, huber, int(iters), (float(tv_gz), 1.0, 1.0))}
    consistency = float(metrics.psnr(thick, baselines.block_apply3d(recon["tv3d"], f, kernel), 1.0))
    extra = {}
    if with_nlm:
        start = None
        if nlm_start == "spline":                                     # one mean correction: A start = thick
            residual = baselines.block_apply3d(recon["spline"], f, kernel) - thick
            start = (recon["spline"] - residual.repeat_interleave(factor, dim=1)).contiguous()
        recon["nlm"] = baselines.nlm_upsample(thick, f, kernel, baselines.NLM_DEFAULT_LEVELS, int(n_iters), n_search, n_patch, x0=start)
        extra["nlm_consistency"] = float(metrics.psnr(thick, baselines.block_apply3d(recon["nlm"], f, kernel), 1.0))
    info = {}
    if with_inr:
        zfirst = np.ascontiguousarray(np.moveaxis(vol, 2, 0))                                                      # [Z, X, Y, B]
        res = fit_volume(zfirst, steps=int(number_of_epochs), seed=seed, upscale_axes=1, lr_model="average",
                         footprint=None if footprint == "point" else "box", return_recon=False)
        sr = reconstruct(res["model"], zfirst.shape, res["B"]) * float(res["scale_back"])                          # on the thin slices
        recon["sr"] = sr.permute(3, 0, 1, 2).contiguous()
        info = {"inr_status": res["status"], "inr_final_loss": res["final_loss"], "inr_footprint_samples": res["footprint_samples"],
                "inr_lr_consistency_psnr_db": res["lr_consistency_psnr_db"]}
    stack = lambda t: t.permute(1, 0, 2, 3).contiguous()                                                           # [Z, B, X, Y]
    hs = stack(hr)
    ok = hs.amax(dim=(-2, -1)) > 0
    safe = lambda t: torch.where(ok[..., None, None], t, torch.ones_like(t)).clamp_min(1e-30)    # empty slices: finite, ignored
    volumes = {"hr": hs, "thick": stack(thick)}
    psnr, ssim = {}, {}
    for name, v in recon.items():
        volumes[name] = stack(v)
        psnr[name] = float(metrics.psnr(hs, volumes[name], 1.0))
        ssim[name] = metrics.ssim_reference_protocol(safe(hs), safe(volumes[name])).cpu().numpy()
    return {"volumes": volumes, "psnr": psnr, "ssim": ssim, "consistency": consistency, "kernel": kernel, "valid": ok.cpu().numpy(),
            "info": info, **extra}


# ---------------------------------------------------------------------------------------------------
MULTI_STACK_DESIGNS = ("shifted", "orthogonal", "overlap")
MULTI_STACK_TRIM = 2            # thin slices left out of the PSNR at either end of the volume


def check_multi_stack(design="shifted", factor=2, noise=0.0, fwhm=None, tv_lambda=0.01, tv_huber=0.01, tv_iters=300, tv_gz=1.0):
    """What ``multi_stack_study`` cannot serve, by name; touches neither the input nor the device."""
    who = "multi_stack_study"
    if design not in MULTI_STACK_DESIGNS:
        raise ValueError(f"{who}: design must be one of {', '.join(MULTI_STACK_DESIGNS)} (got {design!r})")
    if isinstance(factor, bool) or int(factor) != factor or not 2 <= factor <= ops.TVSR_MAX_FACTOR:
        raise ValueError(f"{who}: factor is the slice thickness in thin slices, 2 .. {ops.TVSR_MAX_FACTOR} (got {factor!r})")
    if not 0.0 <= float(noise) < float("inf"):
        raise ValueError(f"{who}: noise must be finite and >= 0 (got {noise!r})")
    if fwhm is not None:
        if design != "overlap":
            raise ValueError(f"{who}: fwhm belongs to design='overlap' (got design={design!r})")
        if not 0.0 < float(fwhm) < float("inf"):
            raise ValueError(f"{who}: fwhm must be finite and > 0, in thick slices (got {fwhm!r})")
    for name, value in (("tv_lambda", tv_lambda), ("tv_huber", tv_huber), ("tv_gz", tv_gz)):
        if not 0.0 <= float(value) < float("inf"):
            raise ValueError(f"{who}: {name} must be finite and >= 0 (got {value!r})")
    if int(tv_iters) != tv_iters or not 1 <= tv_iters <= ops.TVSR3D_MAX_ITER:
        raise ValueError(f"{who}: tv_iters must be 1 .. 100,000 (got {tv_iters!r})")


def multi_stack_designs(design, factor=2, fwhm=None):
    """The stacks of a design as ``baselines.stack_geometry`` records, thin slices along axis 0: ``shifted`` -- two axial stacks of
    thickness ``factor``, the second displaced by ``factor // 2`` thin slices; ``orthogonal`` -- axial, coronal and sagittal, each
    thick by ``factor`` on its own axis; ``overlap`` -- one axial stack with ``2 * factor`` Gaussian taps (``fwhm`` thick slices,
    default 1) at spacing ``factor``.  -> (names, geometries)."""
    from . import baselines
    one, mean = np.ones(1), np.full(factor, 1.0 / factor)
    if design == "shifted":
        return ("axial", "axial_shifted"), [baselines.stack_geometry((factor, 1, 1), (mean, one, one)),
                                            baselines.stack_geometry((factor, 1, 1), (mean, one, one), (factor // 2, 0, 0))]
    if design == "orthogonal":
        return ("axial", "coronal", "sagittal"), [baselines.stack_geometry((factor, 1, 1), (mean, one, one)),
                                                  baselines.stack_geometry((1, factor, 1), (one, mean, one)),
                                                  baselines.stack_geometry((1, 1, factor), (one, one, mean))]
    taps = baselines.profile_taps(2 * factor, factor, "gaussian", 1.0 if fwhm is None else fwhm)
    return ("axial_overlap",), [baselines.stack_geometry((factor, 1, 1), (taps, one, one))]


def multi_stack_study(volume, design, factor=2, noise=0.0, seed=0, fwhm=None, tv_lambda=None, tv_huber=None, tv_iters=None, tv_gz=1.0):
    """``volume`` [Z, X, Y] in [0, 1], thin slices along Z: the stacks of ``design`` (``multi_stack_designs``) formed from the thin
    slices by ``baselines.stack_apply`` -- plus Gaussian noise of ``noise`` drawn from ``np.random.default_rng(seed)``, the stacks in
    order --, and their reconstructions on the thin slices, all float64 on the device: every stack alone by
    ``baselines.tv_superres_stacks`` (``<name>``) and, where it is a block stack that tiles the volume, also by
    ``baselines.tv_superres3d`` (``<name>_tv3d``); ``mean``, the voxel-wise mean of the single-stack solves; ``joint``, all stacks in one
    solve.  Gradient weights ``(tv_gz, 1, 1)``; the ``TVMS_DEFAULT_*`` where an argument is None (they belong to three stacks at noise
    0.02).  Returns ``{"volumes", "stacks", "geometries", "names", "psnr", "ssim", "valid", "info"}``: float64 device volumes [Z, X, Y]
    (``hr`` and the methods), the stacks' data, PSNR (data range 1) over the thin slices ``MULTI_STACK_TRIM:-MULTI_STACK_TRIM`` -- the end
    slices, which a displaced stack does not cover, are left out -- and SSIM by the reference protocol [Z] per method."""
    from . import baselines

    lam = baselines.TVMS_DEFAULT_LAMBDA if tv_lambda is None else tv_lambda
    huber = baselines.TVMS_DEFAULT_HUBER if tv_huber is None else tv_huber
    iters = baselines.TVMS_DEFAULT_ITERS if tv_iters is None else tv_iters
    check_multi_stack(design, factor, noise, fwhm, lam, huber, iters, tv_gz)
    vol = np.asarray(volume, dtype=np.float64)
    if vol.ndim != 3:
        raise ValueError(f"multi_stack_study: the volume is [Z, X, Y] (got {vol.shape})")
    if vol.shape[0] < 2 * MULTI_STACK_TRIM + 2 * factor:
        raise ValueError(f"multi_stack_study: {vol.shape[0]} slices are too few for thick slices of {factor} and a margin of "
                         f"{MULTI_STACK_TRIM}")
    dev = ops.require_gpu()
    hr = torch.from_numpy(np.ascontiguousarray(vol)).to(dev)
    names, geos = multi_stack_designs(design, int(factor), fwhm)
    rng = np.random.default_rng(seed)
    stacks = []
    for geo in geos:
        y = baselines.stack_apply(hr, geo)
        if noise > 0:
            y = y + float(noise) * torch.from_numpy(rng.standard_normal(tuple(y.shape))).to(dev)
        stacks.append(y.contiguous())
    g = (float(tv_gz), 1.0, 1.0)
    recon, info = {}, {}
    for name, geo, y in zip(names, geos, stacks):
        recon[name], meta = baselines.tv_superres_stacks([y], [geo], vol.shape, lam, huber, int(iters), g, return_info=True)
        info[name] = {k: float(v) for k, v in meta.items()}
        block = all(len(k) == f for k, f in zip(geo.kernels, geo.factors)) and geo.offsets == (0, 0, 0)
        if block and all(n * f == N for n, f, N in zip(y.shape, geo.factors, vol.shape)):
            recon[name + "_tv3d"] = baselines.tv_superres3d(y, geo.factors, geo.kernels, lam, huber, int(iters), g)
    if len(names) > 1:
        recon["mean"] = sum(recon[name] for name in names) / float(len(names))
        recon["joint"], meta = baselines.tv_superres_stacks(stacks, geos, vol.shape, lam, huber, int(iters), g, return_info=True)
        info["joint"] = {k: float(v) for k, v in meta.items()}
    ok = hr.amax(dim=(-2, -1)) > 0
    safe = lambda t: torch.where(ok[..., None, None], t, torch.ones_like(t)).clamp_min(1e-30).float()   # empty slices: finite, ignored
    core = slice(MULTI_STACK_TRIM, vol.shape[0] - MULTI_STACK_TRIM)
    psnr, ssim = {}, {}
    for name, v in recon.items():
        psnr[name] = float(-10.0 * torch.log10(((hr[core] - v[core]) ** 2).mean()))
        ssim[name] = metrics.ssim_reference_protocol(safe(hr), safe(v)).cpu().numpy()
    return {"volumes": {"hr": hr, **recon}, "stacks": stacks, "geometries": geos, "names": names, "psnr": psnr, "ssim": ssim,
            "valid": ok.cpu().numpy(), "info": info}


# ---------------------------------------------------------------------------------------------------
MULTI_FRAME_METHODS =("replicate", "tv", "ignored", "estimated", "true")
MULTI_FRAME_MARGIN = 4


def check_multi_frame(factor=2, frames=8, max_shift=1.5, noise=0.02, kernel="mean", tv_lambda=0.01, tv_huber=0.03, tv_iters=300,
                      upsample=4):
    """What ``multi_frame_study`` cannot serve, by name; touches neither the input nor the device."""
    who = "multi_frame_study"
    if int(factor) != factor or not 1 <= factor <= ops.TVSR_MAX_FACTOR:
        raise ValueError(f"{who}: factor is the block side of a LR pixel, 1 .. {ops.TVSR_MAX_FACTOR} (got {factor!r})")
    if int(frames) != frames or not 1 <= frames <= ops.TVMF_MAX_FRAMES:
        raise ValueError(f"{who}: frames must be 1 .. {ops.TVMF_MAX_FRAMES} (got {frames!r})")
    if not 0.0 <= float(max_shift) <= 64.0:
        raise ValueError(f"{who}: max_shift must lie in 0 .. 64 HR pixels (got {max_shift!r})")
    if not 0.0 <= float(noise) < float("inf"):
        raise ValueError(f"{who}: noise must be finite and >= 0 (got {noise!r})")
    if kernel not in ("mean", "decimate"):
        raise ValueError(f"{who}: kernel must be 'mean' or 'decimate' (got {kernel!r})")
    for name, value in (("tv_lambda", tv_lambda), ("tv_huber", tv_huber)):
        if not 0.0 <= float(value) < float("inf"):
            raise ValueError(f"{who}: {name} must be finite and >= 0 (got {value!r})")
    if int(tv_iters) != tv_iters or not 1 <= tv_iters <= ops.TVSR3D_MAX_ITER:
        raise ValueError(f"{who}: tv_iters must be 1 .. 100,000 (got {tv_iters!r})")
    if int(upsample) != upsample or not 1 <= upsample <= 16:
        raise ValueError(f"{who}: upsample must be 1 .. 16 (got {upsample!r})")


def simulate_frames(hr, factors, shifts, kernel="mean"):
    """The noiseless frames [n, K, h, w] of the device images ``hr`` [n, H, W] displaced by ``shifts`` [n, K, 2] (HR pixels), with
    ZEROS beyond the border so that every datum is defined: ``baselines.frame_apply`` of the image padded by whole blocks, cut back."""
    from . import baselines
    f0, f1 = factors
    reach = float(np.abs(np.asarray(shifts)).max()) + 1.0 if np.size(shifts) else 1.0
    p0, p1 = f0 * int(np.ceil(reach / f0)), f1 * int(np.ceil(reach / f1))
    big = torch.nn.functional.pad(hr, (p1, p1, p0, p0))
    out = baselines.frame_apply(big, factors, np.asarray(shifts, np.float64), kernel)
    return out[..., p0 // f0:p0 // f0 + hr.shape[-2] // f0, p1 // f1:p1 // f1 + hr.shape[-1] // f1].contiguous()


def multi_frame_study(slices, factor=2, frames=8, max_shift=1.5, noise=0.02, seed=0, kernel="mean", tv_lambda=None, tv_huber=None,
                      tv_iters=None, upsample=4, true_shifts=False, slice_ids=None):
    """``slices`` [Z, R, R] in [0, 1]: per slice ``frames`` acquisitions, each the ``factor`` x ``factor`` block operator of the slice
    displaced by a shift drawn uniformly in +- ``max_shift`` HR pixels (frame 0 at rest) plus Gaussian noise of ``noise`` -- slice z
    (``slice_ids[i]`` for row i where given, else i) draws its shifts, then its noise, from ``np.random.default_rng(seed * 1000 + z)``
    --, and five reconstructions on the device:
    ``replicate`` (block replication of frame 0), ``tv`` (``baselines.tv_superres`` of frame 0, its defaults), ``ignored`` (all frames,
    shifts taken as zero), ``estimated`` (``baselines.estimate_shifts`` at ``upsample``, searched over ``max_shift`` + 1 HR pixels; the
    true shifts with ``true_shifts``) and ``true``, the last three by ``baselines.tv_superres_multi`` (the ``TVMF_DEFAULT_*`` where an
    argument is None).  Returns ``{"images", "frames", "shifts", "estimate", "psnr", "ssim", "shift_error", "info"}``: float64 device
    stacks, PSNR inside a margin of 4 pixels and SSIM (data range 1) [Z] per method, and max |estimate - shifts| [Z]."""
    from . import baselines

    lam = baselines.TVMF_DEFAULT_LAMBDA if tv_lambda is None else tv_lambda
    huber = baselines.TVMF_DEFAULT_HUBER if tv_huber is None else tv_huber
    iters = baselines.TVMF_DEFAULT_ITERS if tv_iters is None else tv_iters
    check_multi_frame(factor, frames, max_shift, noise, kernel, lam, huber, iters, upsample)
    vol = np.asarray(slices, np.float64)
    m = MULTI_FRAME_MARGIN
    if vol.ndim != 3 or vol.shape[1] % factor or vol.shape[2] % factor or min(vol.shape[1:]) - 2 * m < 7:
        raise ValueError(f"multi_frame_study: slices are [Z, rows, columns], whole blocks of {factor} and at least {7 + 2 * m} pixels "
                         f"a side (got {vol.shape})")
    Z, K, f = vol.shape[0], int(frames), (int(factor), int(factor))
    h, w = vol.shape[1] // factor, vol.shape[2] // factor
    shifts, eta = np.zeros((Z, K, 2)), np.zeros((Z, K, h, w))
    ids = list(range(Z)) if slice_ids is None else [int(v) for v in slice_ids]
    if len(ids) != Z or min(ids) < 0:
        raise ValueError(f"multi_frame_study: slice_ids are one index >= 0 per slice (got {slice_ids!r} for {Z} slices)")
    for z in range(Z):
        rng = np.random.default_rng(int(seed) * 1000 + ids[z])
        shifts[z] = rng.uniform(-max_shift, max_shift, (K, 2))
        shifts[z, 0] = 0.0
        eta[z] = noise * rng.standard_normal((K, h, w))
    dev = ops.require_gpu()
    hr = torch.from_numpy(vol).to(dev)
    y = simulate_frames(hr, f, shifts, kernel) + torch.from_numpy(eta).to(dev)
    true = torch.from_numpy(shifts).to(dev)
    est = true if true_shifts else baselines.estimate_shifts(y, f, int(upsample), (float(max_shift) + 1.0) / factor)
    solve = lambda s: baselines.tv_superres_multi(y, f, s, kernel, lam, huber, int(iters), return_info=True)
    images = {"replicate": y[:, 0].repeat_interleave(factor, dim=1).repeat_interleave(factor, dim=2),
              "tv": baselines.tv_superres(y[:, 0].contiguous(), f, kernel)}
    info = {}
    for name, s in (("ignored", torch.zeros_like(true)), ("estimated", est), ("true", true)):
        images[name], res = solve(s)
        info[name] = {k: v.cpu().numpy() for k, v in res.items()}
    crop = lambda t: t[:, m:-m, m:-m].float().contiguous()
    psnr = {name: metrics.psnr(crop(hr), crop(v), 1.0, per_image=True).cpu().numpy() for name, v in images.items()}
    ssim = {name: metrics.ssim(crop(hr), crop(v), 1.0).cpu().numpy() for name, v in images.items()}
    return {"images": images, "hr": hr, "frames": y, "shifts": true, "estimate": est, "psnr": psnr, "ssim": ssim,
            "shift_error": (est - true).abs().amax(dim=(1, 2)).cpu().numpy(), "info": info}


# ---------------------------------------------------------------------------------------------------
ACQUISITION_MODELS = ("kspace", "gaussian", "block")
ACQUISITION_METHODS = ("spline", "zerofill", "tv_block", "tv_operator")


def check_acquisition_model(model="kspace", side=50, factor=None, lr_side=None, fwhm=None, noise=0.02, tv_lambda=3e-3, tv_huber=0.03,
                            tv_iters=500):
    """What ``acquisition_model_study`` cannot serve, by name; touches neither the input nor the device.  Returns the LR side: ``side
    / factor`` (``factor`` defaults to 2) or ``lr_side``, which may be any whole number -- the ratio need not be one."""
    who = "acquisition_model_study"
    if model not in ACQUISITION_MODELS:
        raise ValueError(f"{who}: model must be one of {', '.join(ACQUISITION_MODELS)} (got {model!r})")
    if isinstance(side, bool) or int(side) != side or not 7 <= side <= ops.TVSR_MAX_SIDE:
        raise ValueError(f"{who}: the HR side is 7 .. {ops.TVSR_MAX_SIDE} pixels (got {side!r})")
    if factor is not None and lr_side is not None:
        raise ValueError(f"{who}: give factor or lr_side, not both (got {factor!r} and {lr_side!r})")
    if lr_side is None:
        factor = 2 if factor is None else factor
        if isinstance(factor, bool) or int(factor) != factor or not 1 <= factor <= ops.TVSR_MAX_FACTOR or side % int(factor):
            raise ValueError(f"{who}: factor is 1 .. {ops.TVSR_MAX_FACTOR} and divides the HR side {side} (got {factor!r})")
        m = int(side) // int(factor)
    else:
        if isinstance(lr_side, bool) or int(lr_side) != lr_side or not 2 <= lr_side <= ops.TVSR_MAX_SIDE:
            raise ValueError(f"{who}: lr_side is 2 .. {ops.TVSR_MAX_SIDE} pixels (got {lr_side!r})")
        m = int(lr_side)
    if model == "block" and (side % m or side // m > ops.TVSR_MAX_FACTOR):
        raise ValueError(f"{who}: model='block' needs a whole number of blocks of at most {ops.TVSR_MAX_FACTOR} pixels ({side} -> {m})")
    if fwhm is not None:
        if model != "gaussian":
            raise ValueError(f"{who}: fwhm belongs to model='gaussian' (got model={model!r})")
        if not 0.0 < float(fwhm) < float("inf"):
            raise ValueError(f"{who}: fwhm must be finite and > 0, in LR pixels (got {fwhm!r})")
    if not 0.0 <= float(noise) < float("inf"):
        raise ValueError(f"{who}: noise must be finite and >= 0 (got {noise!r})")
    for name, value in (("tv_lambda", tv_lambda), ("tv_huber", tv_huber)):
        if not 0.0 <= float(value) < float("inf"):
            raise ValueError(f"{who}: {name} must be finite and >= 0 (got {value!r})")
    if int(tv_iters) != tv_iters or not 1 <= tv_iters <= ops.TVSR3D_MAX_ITER:
        raise ValueError(f"{who}: tv_iters must be 1 .. 100,000 (got {tv_iters!r})")
    return m


def acquisition_operators(model, side, lr_side, fwhm=None):
    """The pair (R0, R1) [lr_side][side] of float64 ndarrays that makes the LR data of ``acquisition_model_study``: 'kspace' is
    ``fourier_operator(align='center', boundary='mirror')``, 'gaussian' ``psf_operator`` of ``fwhm`` LR pixels (default 1.2), 'block'
    the block mean."""
    from . import baselines
    if model == "kspace":
        op = baselines.fourier_operator(side, lr_side, "center", "mirror")
    elif model == "gaussian":
        op = baselines.psf_operator(side, lr_side, 1.2 if fwhm is None else fwhm, "gaussian")
    else:
        op = baselines.block_operator(side, side // lr_side, "mean")
    return op, op.copy()


def acquisition_model_study(slices, model="kspace", factor=None, lr_side=None, fwhm=None, noise=0.02, seed=0, tv_lambda=None,
                            tv_huber=None, tv_iters=None, slice_ids=None, with_degibbs=False):
    """``slices`` [Z, R, R] in [0, 1]: the LR slices [Z, m, m] are made with the operator of ``model`` (``acquisition_operators``) plus
    Gaussian noise of ``noise`` -- slice z (``slice_ids[i]`` for row i where given, else i) draws it from
    ``np.random.default_rng(seed * 1000 + z)`` --, and reconstructed on the device by
    ``spline`` (``baselines.rescale`` for a whole ratio, else ``baselines.resize``), ``zerofill`` (``baselines.fourier_resize``, 'center' /
    'mirror'), ``tv_block`` (``baselines.tv_superres`` with the mean kernel: the model every other study assumes; absent when the ratio is
    no whole number of blocks) and ``tv_operator`` (``baselines.tv_superres_operator`` with the operator that made the data).  Both TV
    rows share ``tv_lambda``, ``tv_huber`` and ``tv_iters`` (the ``TVOP_DEFAULT_*`` where None): they differ in the forward model alone.
    ``with_degibbs`` adds ``degibbs_zerofill`` and ``degibbs_spline``: the LR slices unrung on their own grid (``denoise.degibbs`` at its
    defaults; the LR side must be at least 9), then re-sampled as ``zerofill`` and ``spline`` are.
    Returns ``{"images", "hr", "lr", "operators", "methods", "psnr", "ssim", "consistency", "info"}``: float64 device stacks, PSNR and
    SSIM (data range 1) [Z] per method, and the PSNR of ``A tv_operator`` against the LR data [Z]."""
    from . import baselines

    lam = baselines.TVOP_DEFAULT_LAMBDA if tv_lambda is None else tv_lambda
    huber = baselines.TVOP_DEFAULT_HUBER if tv_huber is None else tv_huber
    iters = baselines.TVOP_DEFAULT_ITERS if tv_iters is None else tv_iters
    vol = np.asarray(slices, np.float64)
    if vol.ndim != 3 or vol.shape[1] != vol.shape[2]:
        raise ValueError(f"acquisition_model_study: slices are [Z, R, R] (got {vol.shape})")
    Z, R = vol.shape[0], vol.shape[1]
    m = check_acquisition_model(model, R, factor, lr_side, fwhm, noise, lam, huber, iters)
    if with_degibbs:
        ops.degibbs_params("acquisition_model_study: with_degibbs", (m, m), ops.DEGIBBS_DEFAULT_SHIFTS, ops.DEGIBBS_DEFAULT_WINDOW)
    ids = list(range(Z)) if slice_ids is None else [int(v) for v in slice_ids]
    if len(ids) != Z or (Z and min(ids) < 0):
        raise ValueError(f"acquisition_model_study: slice_ids are one index >= 0 per slice (got {slice_ids!r} for {Z} slices)")
    eta = np.stack([noise * np.random.default_rng(int(seed) * 1000 + z).standard_normal((m, m)) for z in ids])
    dev = ops.require_gpu()
    pair = tuple(torch.from_numpy(r).to(dev) for r in acquisition_operators(model, R, m, fwhm))
    hr = torch.from_numpy(vol).to(dev)
    y = baselines.operator_apply(hr, pair) + torch.from_numpy(eta).to(dev)
    whole = R % m == 0 and R // m <= ops.TVSR_MAX_FACTOR
    spline = lambda t: (baselines.rescale(t.float().contiguous(), R // m) if R % m == 0 else baselines.resize(t.float().contiguous(), (R, R))).double()
    images = {"spline": spline(y), "zerofill": baselines.fourier_resize(y, (R, R), "center", "mirror")}
    info = {}
    if whole:
        images["tv_block"], res = baselines.tv_superres(y, (R // m, R // m), "mean", lam, huber, int(iters), return_info=True)
        info["tv_block"] = {k: v.cpu().numpy() for k, v in res.items()}
    images["tv_operator"], res = baselines.tv_superres_operator(y, pair, lam, huber, int(iters), return_info=True)
    info["tv_operator"] = {k: v.cpu().numpy() for k, v in res.items()}
    if with_degibbs:
        from . import denoise
        unrung = denoise.degibbs(y.contiguous())
        images["degibbs_zerofill"] = baselines.fourier_resize(unrung, (R, R), "center", "mirror")
        images["degibbs_spline"] = spline(unrung)
    f32 = lambda t: t.float().contiguous()
    psnr = {name: metrics.psnr(f32(hr), f32(v), 1.0, per_image=True).cpu().numpy() for name, v in images.items()}
    ssim = {name: metrics.ssim(f32(hr), f32(v), 1.0).cpu().numpy() for name, v in images.items()}
    consistency = metrics.psnr(f32(y), f32(baselines.operator_apply(images["tv_operator"], pair)), 1.0, per_image=True).cpu().numpy()
    return {"images": images, "hr": hr, "lr": y, "operators": pair, "methods": tuple(images), "psnr": psnr, "ssim": ssim,
            "consistency": consistency, "info": info}


# ---- the joint b-value study: one prior over the b-values of a slice against one per image ----------------------------
JOINT_METHODS = ("replicate", "tv", "tv_joint")
SYNTHETIC_B = (0.0, 150.0, 1000.0, 1500.0)


def check_joint_bvalues(side=50, n_b=4, factor=2, kernel="mean", noise=0.02, tv_lambda=3e-3, tv_joint_lambda=0.048, tv_huber=0.01,
                        tv_iters=300, weights="equal"):
    """What ``joint_bvalue_study`` cannot serve, by name; touches neither the input nor the device.  Returns the LR side."""
    who = "joint_bvalue_study"
    if isinstance(side, bool) or int(side) != side or not 7 <= side <= ops.TVSR_MAX_SIDE:
        raise ValueError(f"{who}: the HR side is 7 .. {ops.TVSR_MAX_SIDE} pixels (got {side!r})")
    if isinstance(n_b, bool) or int(n_b) != n_b or not 2 <= n_b <= ops.TVJ_MAX_CHANNELS:
        raise ValueError(f"{who}: a group is 2 .. {ops.TVJ_MAX_CHANNELS} b-values (got {n_b!r})")
    if isinstance(factor, bool) or int(factor) != factor or not 1 <= factor <= ops.TVSR_MAX_FACTOR or side % int(factor) or \
            side // int(factor) < 7:
        raise ValueError(f"{who}: factor is 1 .. {ops.TVSR_MAX_FACTOR}, divides the HR side {side} and leaves >= 7 LR pixels (got {factor!r})")
    if kernel not in ("mean", "decimate"):
        raise ValueError(f"{who}: kernel must be 'mean' or 'decimate' (got {kernel!r})")
    if not 0.0 <= float(noise) < float("inf"):
        raise ValueError(f"{who}: noise must be finite and >= 0 (got {noise!r})")
    for name, value in (("tv_lambda", tv_lambda), ("tv_joint_lambda", tv_joint_lambda), ("tv_huber", tv_huber)):
        if not 0.0 <= float(value) < float("inf"):
            raise ValueError(f"{who}: {name} must be finite and >= 0 (got {value!r})")
    if int(tv_iters) != tv_iters or not 1 <= tv_iters <= ops.TVSR3D_MAX_ITER:
        raise ValueError(f"{who}: tv_iters must be 1 .. 100,000 (got {tv_iters!r})")
    if weights not in ("equal", "sqrt_signal"):
        raise ValueError(f"{who}: weights must be 'equal' or 'sqrt_signal' (got {weights!r})")
    return int(side) // int(factor)


def check_adc_model(bvalues=SYNTHETIC_B, lam=None, weight=None, iters=None):
    """What the ``tv_adc`` row of ``joint_bvalue_study`` cannot serve, by name; touches no device.  -> (lam, weight, iters), the
    ``ADC_DEFAULT_*`` where None."""
    from . import baselines

    who = "joint_bvalue_study"
    lam = baselines.ADC_DEFAULT_LAMBDA if lam is None else lam
    weight = baselines.ADC_DEFAULT_MAP_WEIGHTS[1] if weight is None else weight
    iters = baselines.ADC_DEFAULT_ITERS if iters is None else iters
    b = np.asarray(bvalues, np.float64).reshape(-1)
    if not (np.isfinite(b).all() and (b >= 0).all()) or np.ptp(b) == 0:
        raise ValueError(f"{who}: the S0 / ADC model needs finite b-values >= 0 that are not all equal (got {b.tolist()})")
    if not 0.0 <= float(lam) < float("inf"):
        raise ValueError(f"{who}: tv_adc_lambda must be finite and >= 0 (got {lam!r})")
    if not 0.0 <= float(weight) <= 1.0:
        raise ValueError(f"{who}: tv_adc_weight must be within [0, 1] (got {weight!r})")
    if int(iters) != iters or not 1 <= iters <= ops.TVSR3D_MAX_ITER:
        raise ValueError(f"{who}: tv_adc_iters must be 1 .. 100,000 (got {iters!r})")
    return float(lam), float(weight), int(iters)


def synthetic_decay(slices, bvalues=SYNTHETIC_B):
    """``slices`` [Z, R, R] in [0, 1] -> [Z, B, R, R]: a mono-exponential decay whose ADC is high where the in-plane smoothed image
    (Gaussian, sigma 1) is dark, ``0.6e-3 + 1.8e-3 (1 - smooth / max)``: the study case of DESIGN.md 4q."""
    from scipy.ndimage import gaussian_filter
    roi = np.asarray(slices, np.float64)
    adc = 0.6e-3 + 1.8e-3 * (1 - np.clip(gaussian_filter(roi, (0, 1, 1)) / roi.max(), 0, 1))
    b = np.asarray(bvalues, np.float64)
    return roi[:, None] * np.exp(-b[None, :, None, None] * adc[:, None])


def loglinear_adc(x, bvalues):
    """ADC [..., H, W] of the device stack ``x`` [..., B, H, W]: minus the least-squares slope of log(max(x, 1e-3)) over b, fp64."""
    b = torch.as_tensor(np.asarray(bvalues, np.float64), device=x.device)
    bc = (b - b.mean())[:, None, None]
    return -(bc * torch.log(x.double().clamp_min(1e-3))).sum(dim=-3) / (bc * bc).sum()


def joint_bvalue_study(hr, bvalues, factor=2, kernel="mean", noise=0.02, seed=0, tv_lambda=None, tv_joint_lambda=None, tv_huber=None,
                       tv_iters=None, weights="equal", slice_ids=None, adc_model=None):
    """``hr`` [Z, B, R, R] in [0, 1], the B b-values of Z slices: the LR stack [Z, B, m, m] is ``baselines.block_apply`` under ``kernel``
    plus Gaussian noise of ``noise`` -- slice z (``slice_ids[i]`` where given, else i) draws its [B, m, m] from
    ``np.random.default_rng(seed * 1000 + z)`` --, reconstructed on the device by ``replicate`` (block replication), ``tv``
    (``baselines.tv_superres``, every image on its own, ``tv_lambda``: ``TV_DEFAULT_LAMBDA`` where None) and ``tv_joint``
    (``baselines.tv_superres_joint``, B the channel axis, ``tv_joint_lambda`` and ``channel_weights(lr, weights)``); both share
    ``tv_huber`` and ``tv_iters`` (the ``TVJ_DEFAULT_*`` where None).  Returns ``{"images", "hr", "lr", "methods", "psnr", "ssim"``
    [Z, B] per method (data range 1), ``"psnr_b"`` [B] and ``"psnr_all"`` per method, ``"adc"`` [Z, R, R] per method and of ``hr``
    (``loglinear_adc``), ``"adc_rmse"`` per method inside ``b_min image > 0.25 max``, ``"mask"``, ``"channel_weights"``, ``"info"}``.
    ``adc_model`` (a dict with any of ``lam``, ``weight``, ``iters``; the ``ADC_DEFAULT_*`` where missing): also the method ``tv_adc``,
    ``baselines.tv_superres_adc`` on the same LR stack -- its images are the model's, ``baselines.adc_signal`` of the two
    maps; ``adc["tv_adc"]`` and ``adc_rmse["tv_adc"]`` are the SOLVER'S map, and ``"adc_loglinear"`` / ``"adc_rmse_loglinear"`` hold the
    log-linear fit of its images beside it; ``"s0"`` the b = 0 map.  Without it every entry is what it was."""
    from . import baselines

    lam = baselines.TV_DEFAULT_LAMBDA if tv_lambda is None else tv_lambda
    lam_j = baselines.TVJ_DEFAULT_LAMBDA if tv_joint_lambda is None else tv_joint_lambda
    huber = baselines.TVJ_DEFAULT_HUBER if tv_huber is None else tv_huber
    iters = baselines.TVJ_DEFAULT_ITERS if tv_iters is None else tv_iters
    vol = np.asarray(hr, np.float64)
    if vol.ndim != 4 or vol.shape[2] != vol.shape[3]:
        raise ValueError(f"joint_bvalue_study: hr is [Z, B, R, R] (got {vol.shape})")
    Z, B, R = vol.shape[0], vol.shape[1], vol.shape[2]
    b = np.asarray(bvalues, np.float64).reshape(-1)
    if b.size != B or np.ptp(b) == 0 or not np.isfinite(b).all():
        raise ValueError(f"joint_bvalue_study: bvalues are {B} finite values that are not all equal (got {b.tolist()})")
    m = check_joint_bvalues(R, B, factor, kernel, noise, lam, lam_j, huber, iters, weights)
    if adc_model is not None:
        model_args = check_adc_model(b, **adc_model)
    ids = list(range(Z)) if slice_ids is None else [int(v) for v in slice_ids]
    if len(ids) != Z or (Z and min(ids) < 0):
        raise ValueError(f"joint_bvalue_study: slice_ids are one index >= 0 per slice (got {slice_ids!r} for {Z} slices)")
    f = int(factor)
    eta = np.stack([noise * np.random.default_rng(int(seed) * 1000 + z).standard_normal((B, m, m)) for z in ids])
    dev = ops.require_gpu()
    hr_d = torch.from_numpy(vol).to(dev)
    y = baselines.block_apply(hr_d, (f, f), kernel) + torch.from_numpy(eta).to(dev)
    mu = baselines.channel_weights(y, weights)
    images, info = {"replicate": y.repeat_interleave(f, dim=-2).repeat_interleave(f, dim=-1).contiguous()}, {}
    images["tv"], res = baselines.tv_superres(y, (f, f), kernel, lam, huber, int(iters), return_info=True)
    info["tv"] = {k: v.cpu().numpy() for k, v in res.items()}
    images["tv_joint"], res = baselines.tv_superres_joint(y, (f, f), kernel, lam_j, huber, int(iters), mu, return_info=True)
    info["tv_joint"] = {k: v.cpu().numpy() for k, v in res.items()}
    if adc_model is not None:
        s0, adc_map, res = baselines.tv_superres_adc(y, b.tolist(), (f, f), kernel, model_args[0], baselines.ADC_DEFAULT_HUBER, model_args[2],
                                                     (1.0, model_args[1]), return_info=True)
        images["tv_adc"] = baselines.adc_signal(s0.contiguous(), adc_map.contiguous(), b.tolist())
        info["tv_adc"] = {k: v.cpu().numpy() for k, v in res.items()}
    f32 = lambda t: t.float().contiguous()
    per_b = lambda t: f32(t.transpose(0, 1)).reshape(B, Z * R, R)
    psnr = {name: metrics.psnr(f32(hr_d), f32(v), 1.0, per_image=True).cpu().numpy().reshape(Z, B) for name, v in images.items()}
    ssim = {name: metrics.ssim(f32(hr_d), f32(v), 1.0).cpu().numpy().reshape(Z, B) for name, v in images.items()}
    psnr_b = {name: metrics.psnr(per_b(hr_d), per_b(v), 1.0, per_image=True).cpu().numpy() for name, v in images.items()}
    psnr_all = {name: float(metrics.psnr(f32(hr_d), f32(v), 1.0)) for name, v in images.items()}
    b0 = hr_d[:, int(np.argmin(b))]
    mask = b0 > 0.25 * b0.max()
    adc = {name: loglinear_adc(v, b) for name, v in images.items()}
    adc["hr"] = loglinear_adc(hr_d, b)
    rmse = lambda a: float(((a - adc["hr"])[mask] ** 2).mean().sqrt())
    out = {}
    if adc_model is not None:                  # the solver's own map; the log-linear fit of its images stands beside it
        out = {"adc_loglinear": {"tv_adc": adc["tv_adc"]}, "adc_rmse_loglinear": {"tv_adc": rmse(adc["tv_adc"])}, "s0": {"tv_adc": s0}}
        adc["tv_adc"] = adc_map.double()
    adc_rmse = {name: rmse(adc[name]) for name in images}
    out.update({"images": images, "hr": hr_d, "lr": y, "methods": tuple(images), "psnr": psnr, "ssim": ssim, "psnr_b": psnr_b,
                "psnr_all": psnr_all, "adc": adc, "adc_rmse": adc_rmse, "mask": mask, "channel_weights": mu, "info": info})
    return out


# ---- the second-order study: does TGV remove the terraces of TV on smoothly varying intensity? ------------------------
SECOND_ORDER_METHODS = ("replicate", "tv", "tgv")
FLAT_THRESHOLD = 1e-3


def check_second_order(rows=48, cols=48, factor=2, kernel="mean", noise=0.02, tv_lambda=3e-3, tv_huber=0.3, tgv_lambda=0.005, tgv_ratio=0.5,
                       tgv_huber=0.0, iters=300):
    """What ``second_order_study`` cannot serve, by name; touches neither the input nor the device.  Returns the LR sides."""
    who = "second_order_study"
    for name, side in (("rows", rows), ("cols", cols)):
        if isinstance(side, bool) or int(side) != side or not 2 <= side <= ops.TVSR_MAX_SIDE:
            raise ValueError(f"{who}: the HR image has 2 .. {ops.TVSR_MAX_SIDE} {name} (got {side!r})")
    if isinstance(factor, bool) or int(factor) != factor or not 1 <= factor <= ops.TVSR_MAX_FACTOR or rows % int(factor) or cols % int(factor):
        raise ValueError(f"{who}: factor is 1 .. {ops.TVSR_MAX_FACTOR} and divides the HR sides {rows} x {cols} (got {factor!r})")
    if kernel not in ("mean", "decimate"):
        raise ValueError(f"{who}: kernel must be 'mean' or 'decimate' (got {kernel!r})")
    if not 0.0 <= float(noise) < float("inf"):
        raise ValueError(f"{who}: noise must be finite and >= 0 (got {noise!r})")
    for name, value in (("tv_lambda", tv_lambda), ("tv_huber", tv_huber), ("tgv_lambda", tgv_lambda), ("tgv_huber", tgv_huber)):
        if not 0.0 <= float(value) < float("inf"):
            raise ValueError(f"{who}: {name} must be finite and >= 0 (got {value!r})")
    if not 0.0 < float(tgv_ratio) < float("inf"):
        raise ValueError(f"{who}: tgv_ratio must be finite and > 0 (got {tgv_ratio!r})")
    if int(iters) != iters or not 1 <= iters <= ops.TVSR3D_MAX_ITER:
        raise ValueError(f"{who}: iters must be 1 .. 100,000 (got {iters!r})")
    return int(rows) // int(factor), int(cols) // int(factor)


def second_order_phantom(n=48):
    """A ramp, a quadratic and a disc, [n, n] float64 in (0, 1]: ``0.2 + 0.5 i + 0.2 j^2 + 0.25 [(i - 0.4)^2 + (j - 0.55)^2 < 0.04]`` with
    ``i, j = index / (n - 1)``, divided by its maximum -- smooth intensity that a first-order prior terraces."""
    t = np.arange(n) / (n - 1.0)
    i, j = t[:, None], t[None, :]
    x = 0.2 + 0.5 * i + 0.2 * j ** 2 + 0.25 * ((i - 0.4) ** 2 + (j - 0.55) ** 2 < 0.04)
    return x / x.max()


def flat_area_index(x, threshold=FLAT_THRESHOLD):
    """The share of the interior pixels of every image of the device stack ``x`` [..., H, W] whose forward-difference gradient
    magnitude is below ``threshold``: a flat-area index of staircasing (fp64; the last row and column have no full gradient)."""
    x = x.double()
    g0 = x[..., 1:, :-1] - x[..., :-1, :-1]
    g1 = x[..., :-1, 1:] - x[..., :-1, :-1]
    return ((g0 * g0 + g1 * g1).sqrt() < threshold).double().mean(dim=(-2, -1))


def second_order_study(hr, factor=2, kernel="mean", noise=0.02, seed=0, tv_lambda=None, tv_huber=None, tgv_lambda=None, tgv_ratio=None,
                       tgv_huber=None, iters=None, slice_ids=None):
    """``hr`` [Z, H, W] in [0, 1]: the LR stack [Z, h, w] is ``baselines.block_apply`` under ``kernel`` plus Gaussian noise of ``noise``
    -- slice z (``slice_ids[i]`` where given, else i) draws its [h, w] from ``np.random.default_rng(seed * 1000 + z)`` --,
    reconstructed on the device by ``replicate`` (block replication), ``tv`` (``baselines.tv_superres`` with ``tv_lambda``, ``tv_huber``:
    the ``TV_DEFAULT_*`` where None) and ``tgv`` (``baselines.tgv_superres`` with ``tgv_lambda``, ``tgv_ratio``, ``tgv_huber``: the
    ``TGV_DEFAULT_*`` where None), all with ``iters`` iterations (``TGV_DEFAULT_ITERS``).  Returns ``{"images", "hr", "lr", "methods",
    "psnr", "ssim", "flat"`` [Z] per method (data range 1; ``flat`` also of ``hr``: ``flat_area_index``), ``"psnr_all"`` per method,
    ``"info"}``."""
    from . import baselines

    lam = baselines.TV_DEFAULT_LAMBDA if tv_lambda is None else tv_lambda
    huber = baselines.TV_DEFAULT_HUBER if tv_huber is None else tv_huber
    lam_g = baselines.TGV_DEFAULT_LAMBDA if tgv_lambda is None else tgv_lambda
    ratio = baselines.TGV_DEFAULT_RATIO if tgv_ratio is None else tgv_ratio
    huber_g = baselines.TGV_DEFAULT_HUBER if tgv_huber is None else tgv_huber
    iters = baselines.TGV_DEFAULT_ITERS if iters is None else iters
    vol = np.asarray(hr, np.float64)
    if vol.ndim != 3:
        raise ValueError(f"second_order_study: hr is [Z, H, W] (got {vol.shape})")
    Z, H, W = vol.shape
    h, w = check_second_order(H, W, factor, kernel, noise, lam, huber, lam_g, ratio, huber_g, iters)
    ids = list(range(Z)) if slice_ids is None else [int(v) for v in slice_ids]
    if len(ids) != Z or (Z and min(ids) < 0):
        raise ValueError(f"second_order_study: slice_ids are one index >= 0 per slice (got {slice_ids!r} for {Z} slices)")
    f = int(factor)
    eta = np.stack([noise * np.random.default_rng(int(seed) * 1000 + z).standard_normal((h, w)) for z in ids])
    dev = ops.require_gpu()
    hr_d = torch.from_numpy(vol).to(dev)
    y = baselines.block_apply(hr_d, (f, f), kernel) + torch.from_numpy(eta).to(dev)
    images, info = {"replicate": y.repeat_interleave(f, dim=-2).repeat_interleave(f, dim=-1).contiguous()}, {}
    images["tv"], res = baselines.tv_superres(y, (f, f), kernel, lam, huber, int(iters), return_info=True)
    info["tv"] = {k: v.cpu().numpy() for k, v in res.items()}
    images["tgv"], res = baselines.tgv_superres(y, (f, f), kernel, lam_g, ratio, huber_g, int(iters), return_info=True)
    info["tgv"] = {k: v.cpu().numpy() for k, v in res.items()}
    f32 = lambda t: t.float().contiguous()
    psnr = {name: metrics.psnr(f32(hr_d), f32(v), 1.0, per_image=True).cpu().numpy() for name, v in images.items()}
    ssim = {name: metrics.ssim(f32(hr_d), f32(v), 1.0).cpu().numpy() for name, v in images.items()}
    psnr_all = {name: float(metrics.psnr(f32(hr_d), f32(v), 1.0)) for name, v in images.items()}
    flat = {name: flat_area_index(v).cpu().numpy() for name, v in images.items()}
    flat["hr"] = flat_area_index(hr_d).cpu().numpy()
    return {"images": images, "hr": hr_d, "lr": y, "methods": tuple(images), "psnr": psnr, "ssim": ssim, "flat": flat,
            "psnr_all": psnr_all, "info": info}
