#!/usr/bin/env python3
"""``superresDWI.py`` of the reference (implicit-neural-representations/superresDWI.py) on the MI355X path.

``.mat`` in -> ``recon`` (x2 the HR in-plane grid = "x4" w.r.t. the LR training grid) and ``SR_recon`` (HR grid) out as
``.mat`` + ``.npy``, plus ``ssim_scores.csv`` with the reference's header ``Pt_id, b-value, slice, SSIM-spline, SSIM-SR``
(superresDWI.py:27,186-187) and a PSNR/SSIM summary (``metrics.json``).

The reference hard-codes its patient list, paths and hyper-parameters (superresDWI.py:26-34,84-91); here the same NAMES are
flags with the same defaults: ``--number_of_epochs 2500 --pertubation_epochs 10 --hidden_dim 512 --num_layers 3 --PN_dim 128
--roi_start 40 --roi_end 90 --mapping_size 128 --scale 0.5``.  Inputs:
  * a ``master.mat`` with ``hybrid_raw`` ([b][TE] cell of [X, Y, Z, acquisitions]) and ``b`` -- the reference's format: the
    acquisition products, the mean image, the INR fit, the PerturbNet phase (superresDWI.py:44-156);
  * any ``.mat`` holding one volume [X, Y, Z] or [X, Y, Z, b] (e.g. ``anon_data/patNN_mean_b0.mat``, key ``data_mean_b0``):
    the same fit and evaluation without a PerturbNet phase (there are no single acquisitions to perturb towards).
Two optional products of the same fit (default off, so a plain run writes exactly the files above):
  * ``--transverse_length T``: through-plane super-resolution (superresDWI.py:217-241; the reference hard-codes T = 100).
    ``coronal.mat`` holds ``coronal_sr`` [2R, 2R, T] -- the INR on a (2R, 2R, T, 1) grid, b index 0, NOT clamped
    (superresDWI.py:221) --, ``coronal_spline`` [R, R, T] -- the not-a-knot cubic spline of the HR ROI along z,
    ``resize_array(mean_img[..., 0], T)`` (SRDWI.py:132-141) on the device -- and ``transverse_length``; ``coronal.npy`` holds
    ``coronal_sr``.  Needs >= 4 slices (the cubic spline's minimum); ``metrics.json`` gains ``t_coronal_s``.
  * ``--adc``: ``adc.mat`` with ``adc_sr``, ``adc_spline``, ``adc_hr`` [2R, 2R, Z] and ``b`` (superresDWI.py:189-206): per slice,
    calculate_ADC of the x2 SR volume, of the x4 spline of the LR ROI and of the x2 spline of the HR ROI, each b-image
    multiplied back by ``maxes[b, 1]`` (TE index 1; for a plain volume the per-b maxima it was divided by).  Needs >= 2
    distinct b-values.
  * ``--derivative_maps``: ``derivatives.mat`` with ``grad_mag`` and ``laplacian``, both of ``recon``'s shape [2R, 2R, Z, B] (one
    map per b-image): the fitted network differentiated exactly on the grid of ``recon`` (nn_mri.py:205-221 ``gradient`` /
    ``laplace``, evaluated in forward mode by ``inr.derivatives``) along the in-plane and through-plane axes -- not along the
    b-value axis.  ``grad_mag = sqrt(sum_i (dy/dx_i)^2)``, ``laplacian = sum_i d^2y/dx_i^2``, of the un-clamped network, in the
    normalised [-1, 1] coordinates of ``get_mgrid`` (times ``2 / (n_i - 1)`` per axis and order for per-voxel units).
  * ``--zerofill [--zerofill_apodize A]``: the interpolation an MR scanner applies, next to the spline:
    ``baselines.fourier_resize(HR[::2, ::2], HR.shape, 'sample', 'mirror', A)`` clamped at 0 -- k-space zero-filling on the grid of the
    decimation (LR sample j sits on HR sample 2j; ``rescale`` places pixel centres, half an LR pixel off), with the mirrored boundary
    a cropped ROI needs.  ``ssim_scores_zerofill.csv`` holds the rows of ``ssim_scores.csv`` under the same protocol with the header
    ``Pt_id, b-value, slice, SSIM-zerofill, SSIM-SR``; ``metrics.json`` gains ``psnr_zerofill_db`` and ``ssim_zerofill_mean``; with
    ``--adc``, ``adc.mat`` gains ``adc_zerofill`` on the grid of ``adc_spline`` (x4 of the LR ROI).  Needs an even ROI side.
  * ``--lr_model average [--footprint box [--footprint_samples S]]``: the low-resolution image is the mean of every 2 x 2 block of the
    HR ROI (what a scanner with twice the in-plane voxel size acquires) instead of every second pixel, placed at the block centres
    in the HR grid's frame; the spline baseline is then ``baselines.rescale(LR, 2)`` of THAT image (pixel-centre placement is right
    for block means).  ``--footprint box`` also fits under the matching forward model -- a datum is the average of the network over
    S x S midpoint nodes of its 2 x 2 HR pixels (``footprint.py``, ``inr_siren_fit_footprint``) -- so that the fitted function is the
    de-blurred image; ``--footprint point`` (default) fits point samples at the block centres.  ``metrics.json`` gains ``lr_model``,
    ``footprint``, ``footprint_samples`` (K) and ``lr_consistency_psnr_db`` (the forward model against the LR data, data range 1).
    Refused: ``--footprint box`` without ``--lr_model average``; either with ``--model wire``; ``--lr_model average`` with
    ``--zerofill`` (defined on the decimation grid), an odd ROI side, or ``hybrid_raw`` and ``--pertubation_epochs > 0`` (the
    PerturbNet phase is point-sampled).
  * ``--tv_baseline [--tv_lambda L --tv_huber A --tv_iters N]``: the classical model-based reconstruction next to the spline -- no
    network, the SAME forward operator as the low-resolution data (``--lr_model decimate``: the decimation, LR sample j on HR sample
    2j; ``--lr_model average``: the 2 x 2 block mean) and a TV (A = 0) / Huber prior: ``baselines.tv_superres(LR, (2, 2), kernel, L, A,
    N)`` on the LR ROI, every slice and b-image in one launch (``inr_tvsr_solve2d_f32``).  ``ssim_scores_tv.csv`` holds
    the rows of ``ssim_scores.csv`` under the same protocol with the header ``Pt_id, b-value, slice, SSIM-tv, SSIM-SR``;
    ``metrics.json`` gains ``psnr_tv_db``, ``ssim_tv_mean`` and ``tv_consistency_psnr_db`` (``A x`` against the LR data, data range 1);
    with ``--adc``, ``adc.mat`` gains ``adc_tv`` on the grid of the HR ROI ([R, R, Z]).  It does not touch the fit, so it goes with
    ``--zerofill`` and ``--model wire``.  Refused before the input is loaded: an odd ROI side, L < 0, A < 0, N outside 1 .. 100,000.
  * ``--tv_joint [--tv_joint_lambda LJ --tv_joint_weights equal|sqrt_signal]`` (with ``--tv_baseline``): the same reconstruction with
    ONE prior over the b-values of a slice -- the [Z, B, R/2, R/2] LR stack with B as the channel axis,
    ``baselines.tv_superres_joint(LR, (2, 2), kernel, LJ, A, N, channel_weights)``, one workgroup per slice (``inr_tvj_solve2d_f32``,
    DESIGN.md 4q), with ``--tv_huber`` and ``--tv_iters``.  ``ssim_scores_tv_joint.csv`` (``Pt_id, b-value, slice, SSIM-tv-joint,
    SSIM-SR``); ``metrics.json`` gains ``psnr_tv_joint_db``, ``ssim_tv_joint_mean`` and ``tv_joint_consistency_psnr_db``; with ``--adc``,
    ``adc.mat`` gains ``adc_tv_joint``.  Refused: without ``--tv_baseline``, LJ < 0 (before the input is loaded), an input with fewer
    than 2 b-values or more than 16 (before the fit).
  * ``--tv_adc [--tv_adc_lambda LA --tv_adc_weight M --tv_adc_iters NA]`` (with ``--tv_baseline``): the S0 / ADC maps of every slice as
    the unknowns of ONE solve over its b-values, ``baselines.tv_superres_adc(Y, b, (2, 2), kernel, LA, huber, NA, (1, M))``
    (``inr_tvadc_solve2d_f32``) with the file's b-values; ``Y`` is the LR stack in the signal's own units, every b-image
    times ``maxes[b, 1]`` over the largest of them (as is, where the file has a single TE).  The model's images ``s0 exp(-b adc)``, back
    in the units of the stack, are scored like the other TV rows: ``ssim_scores_tv_adc.csv`` (``Pt_id, b-value, slice, SSIM-tv-adc,
    SSIM-SR``); ``metrics.json`` gains ``psnr_tv_adc_db``, ``ssim_tv_adc_mean`` and ``tv_adc_consistency_psnr_db``; with ``--adc``,
    ``adc.mat`` gains ``adc_tv_adc`` -- the solver's own map, no log-linear fit of its images -- and ``s0_tv_adc``.  Refused: without
    ``--tv_baseline``, LA < 0, M outside [0, 1], NA outside 1 .. 100,000 (before the input is loaded), an input without 2 .. 16
    distinct, non-negative b-values (once it is known).
  * ``--tv_tgv [--tv_tgv_lambda LG --tv_tgv_ratio R]`` (with ``--tv_baseline``): the same [Z, B, R/2, R/2] stack, every image on its
    own, under the second-order TGV prior, which does not terrace smooth intensity:
    ``baselines.tgv_superres(LR, (2, 2), kernel, LG, R, A, N)`` (``inr_tgv_solve2d_f32``), with ``--tv_huber`` and
    ``--tv_iters``.  ``ssim_scores_tv_tgv.csv`` (``Pt_id, b-value, slice, SSIM-tv-tgv, SSIM-SR``); ``metrics.json`` gains
    ``psnr_tv_tgv_db``, ``ssim_tv_tgv_mean`` and ``tv_tgv_consistency_psnr_db``; with ``--adc``, ``adc.mat`` gains ``adc_tv_tgv``.
    Refused before the input is loaded: without ``--tv_baseline``, LG < 0, R <= 0.
  * ``--nlm_baseline [--nlm_iters N --nlm_search S --nlm_patch P]``: the non-local upsampling of Manjon et al. 2010
    (``baselines.nlm_upsample``) of the same LR stack, every b-value's [Z, R/2, R/2] volume by the factors (1, 2, 2) under
    the forward model of ``--lr_model``: ``ssim_scores_nlm.csv``, ``psnr_nlm_db`` / ``ssim_nlm_mean`` / ``nlm_consistency_psnr_db`` in
    ``metrics.json``, ``adc_nlm`` in ``adc.mat`` with ``--adc``.  Refused before the input is loaded: an odd ROI side, radii out of range.
    ``--denoise nlm`` filters the raw stack by ``denoise.nlm_stack`` under MP-PCA's noise map and records the keys of ``--denoise mppca``.
  * ``--denoise mppca [--denoise_window a b c]``: MP-PCA denoising (``denoise.mppca``, ``inr_mppca_denoise``) of the raw
    stack before the per-cell normalisation of ``load_input_and_scale`` -- for ``hybrid_raw`` every acquisition of every [b][TE] cell is
    a measurement (``denoise.stack_hybrid``), for a plain volume the b axis is; the window's sides are over (X, Y, Z), default 5 5 5,
    and a side larger than its axis is refused.  ``metrics.json`` gains ``denoise``, ``denoise_window`` and ``denoise_sigma_median``
    (the median of the noise map, in the units of the file).  Without the flag every output is bit for bit what it was.
  * ``--degibbs``: Gibbs-ringing removal by local sub-voxel shifts (``denoise.degibbs``, ``inr_degibbs2d``) of the (X, Y)
    planes of the raw stack, after ``--denoise`` and before the per-cell normalisation -- the order of ``dwidenoise`` and
    ``mrdegibbs``.  The data must lie on the acquired grid (scanner-interpolated or partial-Fourier data ring at another period).
    ``metrics.json`` gains ``degibbs`` and ``degibbs_mean_abs_shift`` (pixels).  Without the flag every output is what it was.
``--model wire`` fits the complex-Gabor network of wiretest.ipynb (cells 2, 7) instead of the SIREN: ``hidden_features =
hidden_dim // 2`` (cell 7), ``omega_0 = --wire_omega`` and ``scale_0 = --wire_scale`` for every layer (1.2 both, cell 7), the
plain fit on the mean image (cell 10's first branch) through ``wire.fit_wire``; re-sampling, the SSIM CSV,
``--transverse_length`` and ``--adc`` go through ``wire.reconstruct``.  ``--wire_derivative_maps`` writes the ``derivatives.mat``
described above from the WIRE network (``wire.derivatives``, the forward-mode kernels of the Gabor layer; same keys, shapes,
axes and units); without ``--model wire`` it is refused before any device work, and ``--derivative_maps``, the SIREN's flag,
stays refused under ``--model wire``.  So is the PerturbNet phase HERE: the notebook's whole loop, PerturbNet tail included, is
``scripts/wiretest.py`` (same flags, the notebook's defaults, built from this module's functions).  The default
``--model siren`` is the path described above, unchanged.
R = roi_end - roi_start.  Plots (superresDWI.py:164-233) are outside the build's scope.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import time

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))
import mri_super_resolution_amd as inr  # noqa: E402
from mri_super_resolution_amd import baselines, drivers, matio, metrics, ops, reports, wire  # noqa: E402
from mri_super_resolution_amd import denoise as denoise_mod  # noqa: E402
from mri_super_resolution_amd import footprint as footprint_mod  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="INR super-resolution of diffusion MRI volumes (superresDWI.py protocol)")
    p.add_argument("--data", nargs="+", required=True, help=".mat file(s): master.mat (hybrid_raw) or a plain volume")
    p.add_argument("--key", default=None, help="variable holding the volume (default: hybrid_raw, else the only array)")
    p.add_argument("--pt_id", nargs="*", default=None, help="patient ids for the CSV (default: digits of the file name)")
    p.add_argument("--output_address", default="SR_results", help="output directory (one sub-directory per patient)")
    p.add_argument("--number_of_epochs", type=int, default=2500)
    p.add_argument("--pertubation_epochs", type=int, default=10)
    p.add_argument("--hidden_dim", type=int, default=512)
    p.add_argument("--num_layers", type=int, default=3)
    p.add_argument("--PN_dim", type=int, default=128)
    p.add_argument("--roi_start", type=int, default=40)
    p.add_argument("--roi_end", type=int, default=90)
    p.add_argument("--mapping_size", type=int, default=128)
    p.add_argument("--scale", type=float, default=0.5, help="sigma of the Gaussian Fourier features")
    p.add_argument("--learning_rate", type=float, default=1e-4)
    p.add_argument("--seed", type=int, default=None, help="seeds numpy (Fourier matrix) and torch (weights); default: unseeded")
    p.add_argument("--transverse_length", type=int, default=0,
                   help="also write coronal.mat / coronal.npy: the INR and a cubic spline on T slices along z (superresDWI.py:"
                        "217-241, where T = 100 is hard-coded); default 0 = off")
    p.add_argument("--adc", action="store_true",
                   help="also write adc.mat: ADC maps of SR, spline and HR (superresDWI.py:189-206); needs >= 2 b-values")
    p.add_argument("--zerofill", action="store_true",
                   help="also score the k-space zero-fill baseline (Fourier re-sampling of every second HR pixel, mirrored boundary): "
                        "ssim_scores_zerofill.csv, psnr_zerofill_db / ssim_zerofill_mean in metrics.json, adc_zerofill with --adc")
    p.add_argument("--zerofill_apodize", type=float, default=0.0,
                   help="--zerofill: Tukey window over the kept band, 0 (none, the default) .. 1 (Hann)")
    p.add_argument("--tv_baseline", action="store_true",
                   help="also score the model-based TV / Huber reconstruction of the LR ROI under the forward model of --lr_model: "
                        "ssim_scores_tv.csv, psnr_tv_db / ssim_tv_mean / tv_consistency_psnr_db in metrics.json, adc_tv with --adc")
    p.add_argument("--tv_lambda", type=float, default=baselines.TV_DEFAULT_LAMBDA,
                   help="--tv_baseline: weight of the prior (data in [0, 1]; default from the sweep of DESIGN.md 4l)")
    p.add_argument("--tv_huber", type=float, default=baselines.TV_DEFAULT_HUBER,
                   help="--tv_baseline: Huber threshold on the gradient magnitude; 0 = plain isotropic TV")
    p.add_argument("--tv_iters", type=int, default=baselines.TV_DEFAULT_ITERS, help="--tv_baseline: Chambolle-Pock iterations, 1 .. 100,000")
    p.add_argument("--tv_joint", action="store_true",
                   help="--tv_baseline: also score the channel-coupled reconstruction, one prior over the b-values of a slice (needs >= 2 "
                        "b-values): ssim_scores_tv_joint.csv, psnr_tv_joint_db / ssim_tv_joint_mean / tv_joint_consistency_psnr_db in "
                        "metrics.json, adc_tv_joint with --adc; uses --tv_huber and --tv_iters")
    p.add_argument("--tv_joint_lambda", type=float, default=baselines.TVJ_DEFAULT_LAMBDA,
                   help="--tv_joint: weight of the coupled prior (default from the sweep of DESIGN.md 4q)")
    p.add_argument("--tv_joint_weights", choices=("equal", "sqrt_signal"), default="equal",
                   help="--tv_joint: the channel weights of the coupled norm (baselines.channel_weights)")
    p.add_argument("--tv_adc", action="store_true",
                   help="with --tv_baseline: also the model-based S0 / ADC reconstruction, whose unknowns are the two parameter maps of a "
                        "slice: ssim_scores_tv_adc.csv, psnr_tv_adc_db / ssim_tv_adc_mean / tv_adc_consistency_psnr_db in metrics.json, "
                        "adc_tv_adc and s0_tv_adc with --adc (needs 2 .. 16 distinct b-values)")
    p.add_argument("--tv_adc_lambda", type=float, default=baselines.ADC_DEFAULT_LAMBDA,
                   help="--tv_adc: weight of the prior on the maps (default from the sweep of DESIGN.md 4t)")
    p.add_argument("--tv_adc_weight", type=float, default=baselines.ADC_DEFAULT_MAP_WEIGHTS[1],
                   help="--tv_adc: weight of the normalised ADC map in the prior, within [0, 1]")
    p.add_argument("--tv_adc_iters", type=int, default=baselines.ADC_DEFAULT_ITERS, help="--tv_adc: iterations, 1 .. 100,000")
    p.add_argument("--tv_tgv", action="store_true",
                   help="with --tv_baseline: also the second-order TGV reconstruction, which does not terrace smooth intensity: "
                        "ssim_scores_tv_tgv.csv, psnr_tv_tgv_db / ssim_tv_tgv_mean / tv_tgv_consistency_psnr_db in metrics.json, "
                        "adc_tv_tgv with --adc; uses --tv_huber and --tv_iters")
    p.add_argument("--tv_tgv_lambda", type=float, default=baselines.TGV_DEFAULT_LAMBDA,
                   help="--tv_tgv: weight of the first-order term (default from the sweep of DESIGN.md 4r)")
    p.add_argument("--tv_tgv_ratio", type=float, default=baselines.TGV_DEFAULT_RATIO,
                   help="--tv_tgv: second-order weight / first-order weight, > 0")
    p.add_argument("--nlm_baseline", action="store_true",
                   help="also score the non-local upsampling of the LR ROI (baselines.nlm_upsample on the [B, Z, R/2, R/2] volumes, "
                        "factors (1, 2, 2), the forward model of --lr_model): ssim_scores_nlm.csv, psnr_nlm_db / ssim_nlm_mean / "
                        "nlm_consistency_psnr_db in metrics.json, adc_nlm with --adc")
    p.add_argument("--nlm_iters", type=int, default=baselines.NLM_DEFAULT_ITERS, help="--nlm_baseline: passes per level")
    p.add_argument("--nlm_search", type=int, default=baselines.NLM_DEFAULT_SEARCH, help="--nlm_baseline: search radius, 0 .. 5")
    p.add_argument("--nlm_patch", type=int, default=baselines.NLM_DEFAULT_PATCH, help="--nlm_baseline: patch radius, 0 .. 2")
    p.add_argument("--derivative_maps", action="store_true",
                   help="also write derivatives.mat: gradient magnitude and Laplacian of the fitted network on recon's grid, "
                        "along the spatial axes (nn_mri.py:205-221)")
    p.add_argument("--model", choices=("siren", "wire"), default="siren",
                   help="network family: the SIREN of superresDWI.py, or the complex-Gabor WIRE network of wiretest.ipynb "
                        "(hidden_features = hidden_dim // 2; no PerturbNet phase; derivative maps through "
                        "--wire_derivative_maps)")
    p.add_argument("--wire_derivative_maps", action="store_true",
                   help="--model wire: also write derivatives.mat (grad_mag, laplacian on recon's grid, along the spatial axes) "
                        "from the WIRE network's forward-mode derivative kernels")
    p.add_argument("--lr_model", choices=("decimate", "average"), default="decimate",
                   help="how the low-resolution image comes from the HR ROI: every second pixel (superresDWI.py:94), or the mean of "
                        "every 2 x 2 block at the block centres")
    p.add_argument("--footprint", choices=("point", "box"), default="point",
                   help="--lr_model average: the forward model of a low-resolution pixel in the fit: a point sample, or the average "
                        "of the network over its 2 x 2 HR pixels")
    p.add_argument("--footprint_samples", type=int, default=2,
                   help="--footprint box: midpoint nodes per in-plane axis (2 = the discrete block mean on the HR grid; at most 8)")
    p.add_argument("--denoise", choices=("none", "mppca", "nlm"), default="none",
                   help="denoise the raw stack before the per-cell normalisation: MP-PCA over the acquisitions of hybrid_raw (or the b "
                        "axis of a plain volume), or (nlm) non-local means of the raw stack under MP-PCA's noise map; metrics.json "
                        "gains denoise, denoise_window and denoise_sigma_median")
    p.add_argument("--denoise_window", type=int, nargs=3, default=list(denoise_mod.DEFAULT_WINDOW), metavar=("A", "B", "C"),
                   help="--denoise mppca: odd window sides over (X, Y, Z), each at most its axis")
    p.add_argument("--degibbs", action="store_true",
                   help="unring the (X, Y) planes of the raw stack (after --denoise, before the per-cell normalisation); metrics.json "
                        "gains degibbs and degibbs_mean_abs_shift")
    p.add_argument("--wire_omega", type=float, default=1.2, help="--model wire: omega_0 of every layer (wiretest.ipynb cell 7)")
    p.add_argument("--wire_scale", type=float, default=1.2, help="--model wire: scale_0 of every layer (wiretest.ipynb cell 7)")
    return p


def _patient_id(path):
    m = re.findall(r"\d+", os.path.basename(path))
    return m[0] if m else os.path.splitext(os.path.basename(path))[0]


def load_input(path, key=None):
    """-> (mean_img [X, Y, Z, B] float64, acquisitions or None, bvalues, maxes or None)."""
    return load_input_and_scale(path, key)[:4]


def load_input_and_scale(path, key=None, refuse_acquisitions=None, denoise=None, degibbs=None):
    """``load_input`` plus the per-b factors [B] that turn ``mean_img`` back into signal for the ADC maps: ``maxes[:, 1]``
    (TE index 1, superresDWI.py:193-195; None when ``hybrid_raw`` has a single TE) or, for a plain volume, the per-b maxima it
    was divided by.  ``refuse_acquisitions``: the reason for which an input with single acquisitions (``hybrid_raw``) is
    refused (``_check_model``) -- raised before their products are formed on the device.  ``denoise``: None, or a dict with ``window``
    (and optionally ``estimator``): the raw stack is MP-PCA denoised before anything is divided by a maximum, and the dict receives
    ``sigma_median``, the median of the noise map in the file's units.  ``degibbs``: None, or a dict (optionally with ``nshifts``): the (X,
    Y) planes of the raw stack are unrung (``denoise.degibbs``) after the denoising and before anything is divided by a maximum, and
    the dict receives ``mean_abs_shift`` (pixels)."""
    data = matio.loadmat(path)
    if key is None and "hybrid_raw" in data:
        key = "hybrid_raw"
    if key is None:
        keys = [k for k, v in data.items() if isinstance(v, np.ndarray) and v.dtype != object and v.ndim >= 3]
        if len(keys) != 1:
            raise KeyError(f"{path}: pass --key, candidates are {keys}")
        key = keys[0]
    arr = data[key]
    if arr.dtype == object:                                           # hybrid_raw: superresDWI.py:44-83
        if refuse_acquisitions:
            raise ValueError(f"{path}: {refuse_acquisitions}")
        raw = [[np.asarray(arr[b][te], np.float64) for te in range(arr.shape[1])] for b in range(arr.shape[0])]
        if denoise is not None:
            clean, info = denoise_mod.mppca(denoise_mod.stack_hybrid(raw), denoise["window"], estimator=denoise.get("estimator", "exp2"),
                                            return_info=True)
            if denoise.get("method") == "nlm":                          # the projection is discarded, the noise map kept
                clean = denoise_mod.nlm_stack(denoise_mod.stack_hybrid(raw), info["sigma"])
            raw = denoise_mod.unstack_hybrid(clean, raw)
            denoise["sigma_median"] = float(np.median(info["sigma"]))
        if degibbs is not None:
            clean, info = denoise_mod.degibbs(denoise_mod.stack_hybrid(raw), (1, 2), degibbs.get("nshifts", denoise_mod.DEGIBBS_DEFAULT_SHIFTS),
                                              return_info=True)
            raw = denoise_mod.unstack_hybrid(clean, raw)
            degibbs["mean_abs_shift"] = float(np.abs(info["shift"]).mean())
        maxes = np.array([[raw[b][te].max() for te in range(len(raw[b]))] for b in range(len(raw))])
        norm = [[raw[b][te] / maxes[b, te] for te in range(len(raw[b]))] for b in range(len(raw))]
        acq = drivers.acquisition_products(norm)                       # [X, Y, Z, B, K]
        bvals = np.asarray(data["b"], np.float64).reshape(-1) if "b" in data else np.arange(acq.shape[3], dtype=np.float64)
        return acq.mean(axis=-1), acq, bvals, maxes, (maxes[:, 1] if maxes.shape[1] > 1 else None)
    vol = np.asarray(arr, np.float64)
    if vol.ndim == 3:
        vol = vol[..., None]
    if denoise is not None:
        noisy = vol
        vol, info = denoise_mod.mppca(vol, denoise["window"], estimator=denoise.get("estimator", "exp2"), return_info=True,
                                      measurement_axis=-1)
        if denoise.get("method") == "nlm":
            vol = np.ascontiguousarray(np.moveaxis(denoise_mod.nlm_stack(np.ascontiguousarray(np.moveaxis(noisy, -1, 0)), info["sigma"]), 0, -1))
        denoise["sigma_median"] = float(np.median(info["sigma"]))
    if degibbs is not None:
        vol, info = denoise_mod.degibbs(vol, (0, 1), degibbs.get("nshifts", denoise_mod.DEGIBBS_DEFAULT_SHIFTS), return_info=True)
        degibbs["mean_abs_shift"] = float(np.abs(info["shift"]).mean())
    per_b_max = vol.reshape(-1, vol.shape[-1]).max(axis=0)
    vol = vol / per_b_max                                                # per-b normalisation (superresDWI.py:50-55)
    bvals = np.asarray(data["b"], np.float64).reshape(-1) if "b" in data else np.zeros(vol.shape[-1])
    return vol, None, bvals, None, per_b_max


def run_patient(path, pt_id, args, check_model=None, fit=None):
    """One patient.  ``check_model`` / ``fit``: another driver's refusals and fit on this driver's loading, re-sampling and
    outputs (``scripts/wiretest.py``); ``fit(args, INR, B, mean_dataset, model_input, target, acq_lr)`` returns the losses and
    what it adds to ``metrics.json`` (``acq_lr``: the K low-resolution acquisition products, None for a plain volume).  A hook that
    fits other LR data than this function forms says so with an attribute ``changes_lr_data = True``: ``--tv_baseline``, which solves on
    this function's LR ROI, is then refused; any other hook leaves it alone."""
    out_dir = os.path.join(args.output_address, f"pat{pt_id}")
    os.makedirs(out_dir, exist_ok=True)
    # (the footprint flags are refused for every caller of this function: another driver's ``check_model`` replaces ``_check_model``)
    refuse_acquisitions = _check_footprint(args, external_fit=fit is not None)
    _check_tv(args, fit)
    _check_nlm(args, fit)
    refuse_acquisitions = (check_model or _check_model)(args) or refuse_acquisitions
    denoise = ({"window": tuple(args.denoise_window), "method": args.denoise} if getattr(args, "denoise", "none") in ("mppca", "nlm")
               else None)
    degibbs = {} if getattr(args, "degibbs", False) else None
    mean_img, acq, bvalues, maxes, signal_scale = load_input_and_scale(path, args.key, refuse_acquisitions, denoise, degibbs)
    r0, r1 = args.roi_start, args.roi_end
    if r1 > min(mean_img.shape[:2]) or r0 < 0 or r1 - r0 < 14:
        raise ValueError(f"ROI {r0}:{r1} does not fit the {mean_img.shape[:2]} slices (SSIM needs >= 7 x 7 LR pixels)")
    _check_optional_outputs(args, path, mean_img, bvalues, signal_scale)
    if args.seed is not None:
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
    hr_img = mean_img[r0:r1, r0:r1]                                                       # :100,128
    average = getattr(args, "lr_model", "decimate") == "average"
    if average:
        lr_img = footprint_mod.block_means(hr_img)
    else:
        lr_img = mean_img[r0:r1:2, r0:r1:2]                                               # superresDWI.py:94,97
    mean_dataset = inr.ImageFitting_set([lr_img])
    dimension = len(mean_dataset.shape)
    B = torch.from_numpy(np.random.normal(size=(args.mapping_size, dimension)) * args.scale).float().cuda()   # :105-106
    if args.model == "wire":                                                              # wiretest.ipynb cell 7
        INR = wire.Wire(in_features=2 * args.mapping_size, out_features=1, hidden_features=args.hidden_dim // 2,
                        hidden_layers=args.num_layers, first_omega_0=args.wire_omega, hidden_omega_0=args.wire_omega,
                        scale=args.wire_scale).cuda()
        reconstruct = wire.reconstruct
    else:
        INR = inr.Siren(in_features=2 * args.mapping_size, out_features=1, hidden_features=args.hidden_dim,
                        hidden_layers=args.num_layers).cuda()
        reconstruct = inr.reconstruct
    footprint = None
    if average:
        coords, footprint = _average_model(args, hr_img.shape)
        model_input = inr.footprint_inputs(coords, B, footprint)
    else:
        model_input = inr.input_mapping(mean_dataset.coords[0], B)
    target = mean_dataset.pixels[0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit_summary = {}
    if fit is not None:
        acq_lr = None if acq is None else [acq[r0:r1:2, r0:r1:2, :, :, k] for k in range(acq.shape[-1])]
        losses, fit_summary = fit(args, INR, B, mean_dataset, model_input, target, acq_lr)
    elif args.model == "wire":                                # the plain fit on the mean image (wiretest.ipynb cell 10)
        fitter, losses = wire.fit_wire(INR, model_input, target, args.number_of_epochs, lr=args.learning_rate)
    elif average:                                             # (K = 1, the point footprint, is the plain fit at the block centres)
        fitter = inr.FootprintSirenFitter(INR, footprint, lr=args.learning_rate) if footprint.count > 1 else None
        fitter, losses = inr.fit_siren(INR, model_input, target, args.number_of_epochs, lr=args.learning_rate, fitter=fitter)
    elif acq is None:
        fitter, losses = inr.fit_siren(INR, model_input, target, args.number_of_epochs, lr=args.learning_rate)
    else:
        acq_lr = [acq[r0:r1:2, r0:r1:2, :, :, k] for k in range(acq.shape[-1])]
        losses = drivers.fit_with_perturbnet(INR, B, mean_dataset, acq_lr, args.number_of_epochs, args.pertubation_epochs,
                                             PN_dim=args.PN_dim, lr=args.learning_rate)
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    hr_shape = tuple(hr_img.shape)
    test_shape = (hr_shape[0] * 2, hr_shape[1] * 2) + hr_shape[2:]                         # :125
    t0 = time.perf_counter()
    recon = reconstruct(INR, test_shape, B)                                               # :161
    SR_recon = reconstruct(INR, hr_shape, B)                                              # :162
    torch.cuda.synchronize()
    t_rec = time.perf_counter() - t0

    hr_d = torch.from_numpy(np.ascontiguousarray(hr_img, dtype=np.float32)).cuda()
    nz, nb = hr_shape[2], hr_shape[3]
    # [Z, B, X, Y] stacks of 2-D slices; spline baseline from every second HR pixel, x2 (superresDWI.py:181)
    hs = hr_d.permute(2, 3, 0, 1).contiguous()
    ss = SR_recon.permute(2, 3, 0, 1).contiguous()
    if average:     # the baseline sees what the fit saw: the block means, whose pixel centres are where `rescale` places them
        ls = torch.from_numpy(np.ascontiguousarray(lr_img, dtype=np.float32)).cuda().permute(2, 3, 0, 1).contiguous()
    else:
        ls = hs[:, :, ::2, ::2].contiguous()
    sp = baselines.rescale(ls, 2)
    ok = hs.amax(dim=(-2, -1)) > 0
    safe = lambda t: torch.where(ok[..., None, None], t, torch.ones_like(t)).clamp_min(1e-30)   # empty slices: finite, ignored
    ssim_spline = metrics.ssim_reference_protocol(safe(hs), safe(sp)).cpu().numpy()
    ssim_sr = metrics.ssim_reference_protocol(safe(hs), safe(ss)).cpu().numpy()
    zf = _zerofill(hs, 2, args.zerofill_apodize) if getattr(args, "zerofill", False) else None
    tv = _tv_baseline(ls, args, average) if getattr(args, "tv_baseline", False) else None
    tvj = _tv_joint(ls, args, average) if getattr(args, "tv_joint", False) else None
    tgv = _tv_tgv(ls, args, average) if getattr(args, "tv_tgv", False) else None
    tva = _tv_adc(ls, args, average, bvalues, signal_scale) if getattr(args, "tv_adc", False) else None
    nlm = _nlm_baseline(ls, args, average) if getattr(args, "nlm_baseline", False) else None
    with reports.SsimCsv(os.path.join(out_dir, "ssim_scores.csv")) as csv:
        for _slice in range(nz):
            for b in range(nb):
                csv.row(pt_id, bvalues[b] if b < len(bvalues) else b, _slice, float(ssim_spline[_slice, b]),
                        float(ssim_sr[_slice, b]))
    okn = ok.cpu().numpy()
    summary = {
        "pt_id": str(pt_id), "input": os.path.abspath(path), "lr_shape": list(lr_img.shape), "test_shape": list(test_shape),
        "n_coords": int(lr_img.size), "steps": int(args.number_of_epochs), "t_fit_s": t_fit, "t_recon_s": t_rec,
        "train_voxels_per_s": lr_img.size * args.number_of_epochs / max(t_fit, 1e-9),
        "final_loss": float(losses[-1]) if len(losses) else None,
        "psnr_db": float(metrics.psnr(hr_d, SR_recon, 1.0)),
        "psnr_spline_db": float(metrics.psnr(hs, sp, 1.0)),
        "ssim_sr_mean": float(ssim_sr[okn].mean()), "ssim_spline_mean": float(ssim_spline[okn].mean()),
    }
    if zf is not None:
        ssim_zf = metrics.ssim_reference_protocol(safe(hs), safe(zf)).cpu().numpy()
        with reports.SsimCsv(os.path.join(out_dir, "ssim_scores_zerofill.csv"), reports.SSIM_ZEROFILL_HEADER) as csv:
            for _slice in range(nz):
                for b in range(nb):
                    csv.row(pt_id, bvalues[b] if b < len(bvalues) else b, _slice, float(ssim_zf[_slice, b]), float(ssim_sr[_slice, b]))
        summary["psnr_zerofill_db"] = float(metrics.psnr(hs, zf, 1.0))
        summary["ssim_zerofill_mean"] = float(ssim_zf[okn].mean())
    if tv is not None:
        ssim_tv = metrics.ssim_reference_protocol(safe(hs), safe(tv)).cpu().numpy()
        with reports.SsimCsv(os.path.join(out_dir, "ssim_scores_tv.csv"), reports.SSIM_TV_HEADER) as csv:
            for _slice in range(nz):
                for b in range(nb):
                    csv.row(pt_id, bvalues[b] if b < len(bvalues) else b, _slice, float(ssim_tv[_slice, b]), float(ssim_sr[_slice, b]))
        summary["psnr_tv_db"] = float(metrics.psnr(hs, tv, 1.0))
        summary["ssim_tv_mean"] = float(ssim_tv[okn].mean())
        summary["tv_consistency_psnr_db"] = float(metrics.psnr(ls, baselines.block_apply(tv, (2, 2), _tv_kernel(average)), 1.0))
    if tvj is not None:
        ssim_tvj = metrics.ssim_reference_protocol(safe(hs), safe(tvj)).cpu().numpy()
        with reports.SsimCsv(os.path.join(out_dir, "ssim_scores_tv_joint.csv"), reports.SSIM_TV_JOINT_HEADER) as csv:
            for _slice in range(nz):
                for b in range(nb):
                    csv.row(pt_id, bvalues[b] if b < len(bvalues) else b, _slice, float(ssim_tvj[_slice, b]), float(ssim_sr[_slice, b]))
        summary["psnr_tv_joint_db"] = float(metrics.psnr(hs, tvj, 1.0))
        summary["ssim_tv_joint_mean"] = float(ssim_tvj[okn].mean())
        summary["tv_joint_consistency_psnr_db"] = float(metrics.psnr(ls, baselines.block_apply(tvj, (2, 2), _tv_kernel(average)), 1.0))
    if tgv is not None:
        ssim_tgv = metrics.ssim_reference_protocol(safe(hs), safe(tgv)).cpu().numpy()
        with reports.SsimCsv(os.path.join(out_dir, "ssim_scores_tv_tgv.csv"), reports.SSIM_TV_TGV_HEADER) as csv:
            for _slice in range(nz):
                for b in range(nb):
                    csv.row(pt_id, bvalues[b] if b < len(bvalues) else b, _slice, float(ssim_tgv[_slice, b]), float(ssim_sr[_slice, b]))
        summary["psnr_tv_tgv_db"] = float(metrics.psnr(hs, tgv, 1.0))
        summary["ssim_tv_tgv_mean"] = float(ssim_tgv[okn].mean())
        summary["tv_tgv_consistency_psnr_db"] = float(metrics.psnr(ls, baselines.block_apply(tgv, (2, 2), _tv_kernel(average)), 1.0))
    if tva is not None:
        ssim_tva = metrics.ssim_reference_protocol(safe(hs), safe(tva["images"])).cpu().numpy()
        with reports.SsimCsv(os.path.join(out_dir, "ssim_scores_tv_adc.csv"), reports.SSIM_TV_ADC_HEADER) as csv:
            for _slice in range(nz):
                for b in range(nb):
                    csv.row(pt_id, bvalues[b] if b < len(bvalues) else b, _slice, float(ssim_tva[_slice, b]), float(ssim_sr[_slice, b]))
        summary["psnr_tv_adc_db"] = float(metrics.psnr(hs, tva["images"], 1.0))
        summary["ssim_tv_adc_mean"] = float(ssim_tva[okn].mean())
        summary["tv_adc_consistency_psnr_db"] = float(metrics.psnr(ls, baselines.block_apply(tva["images"], (2, 2), _tv_kernel(average)), 1.0))
    if nlm is not None:
        ssim_nlm = metrics.ssim_reference_protocol(safe(hs), safe(nlm)).cpu().numpy()
        with reports.SsimCsv(os.path.join(out_dir, "ssim_scores_nlm.csv"), reports.SSIM_NLM_HEADER) as csv:
            for _slice in range(nz):
                for b in range(nb):
                    csv.row(pt_id, bvalues[b] if b < len(bvalues) else b, _slice, float(ssim_nlm[_slice, b]), float(ssim_sr[_slice, b]))
        summary["psnr_nlm_db"] = float(metrics.psnr(hs, nlm, 1.0))
        summary["ssim_nlm_mean"] = float(ssim_nlm[okn].mean())
        summary["nlm_consistency_psnr_db"] = float(metrics.psnr(ls, baselines.block_apply(nlm, (2, 2), _tv_kernel(average)), 1.0))
    if average:
        pred = inr.footprint_forward(INR, coords, B, footprint)
        summary.update({"lr_model": "average", "footprint": args.footprint, "footprint_samples": footprint.count,
                        "lr_consistency_psnr_db": float(metrics.psnr(target.reshape(1, -1), pred.reshape(1, -1), 1.0))})
    if denoise is not None:
        summary.update({"denoise": denoise["method"], "denoise_window": list(denoise["window"]), "denoise_sigma_median": denoise["sigma_median"]})
    if degibbs is not None:
        summary.update({"degibbs": True, "degibbs_mean_abs_shift": degibbs["mean_abs_shift"]})
    summary.update(fit_summary)
    if args.transverse_length:
        coronal, summary["t_coronal_s"] = _coronal(INR, B, mean_img, test_shape, args, reconstruct)
        matio.savemat(os.path.join(out_dir, "coronal.mat"), coronal)
        np.save(os.path.join(out_dir, "coronal.npy"), coronal["coronal_sr"])
    if args.adc:
        adc_vars = _adc_maps(recon, hs, bvalues, signal_scale, args.zerofill_apodize if zf is not None else None, ls, tv, tvj, tgv, nlm)
        if tva is not None:                                                         # [Z, R, R] -> [R, R, Z], the layout of the other maps
            adc_vars["adc_tv_adc"] = tva["adc"].permute(1, 2, 0).contiguous().cpu().numpy()
            adc_vars["s0_tv_adc"] = (tva["s0"] * tva["unit"]).permute(1, 2, 0).contiguous().cpu().numpy()
        matio.savemat(os.path.join(out_dir, "adc.mat"), adc_vars)
    if args.derivative_maps:
        matio.savemat(os.path.join(out_dir, "derivatives.mat"), _derivative_maps(INR, B, test_shape))
    if args.wire_derivative_maps:
        matio.savemat(os.path.join(out_dir, "derivatives.mat"), _derivative_maps(INR, B, test_shape, wire.derivatives))
    rec_h, sr_h = recon.cpu().numpy(), SR_recon.cpu().numpy()
    out_vars = {"recon": rec_h, "SR_recon": sr_h, "b": np.asarray(bvalues, np.float64)}
    if maxes is not None:
        out_vars["maxes"] = maxes
    matio.savemat(os.path.join(out_dir, "recon.mat"), out_vars)
    np.save(os.path.join(out_dir, "recon.npy"), rec_h)
    with open(os.path.join(out_dir, "metrics.json"), "w") as fh:
        json.dump(summary, fh, indent=1)
    print(json.dumps(summary))
    return summary


def _average_model(args, hr_shape):
    """``--lr_model average``: the coordinates of the LR data -- the centres of the 2 x 2 in-plane blocks in the HR grid's frame -- and
    the footprint of ``--footprint``."""
    if args.footprint == "box":
        footprint = footprint_mod.block_footprint(hr_shape, 2, int(args.footprint_samples))
    else:
        footprint = inr.Footprint.point(len(hr_shape))
    return footprint_mod.block_centres(hr_shape), footprint


def _check_footprint(args, external_fit=False):
    """``--lr_model`` / ``--footprint``: the combinations nothing serves, before the input is loaded and anything touches the device
    (``run_patient`` calls it whichever driver's ``check_model`` it was given).  ``external_fit``: the fit is another driver's hook,
    which knows neither the block-centre coordinates nor the ``n*K`` rows of a footprint.
    Returns the reason for which an input with single acquisitions is to be refused (None: it is served)."""
    lr_model, footprint = getattr(args, "lr_model", "decimate"), getattr(args, "footprint", "point")
    if footprint == "box" and lr_model != "average":
        raise ValueError("--footprint box is the 2 x 2 block of --lr_model average: pass --lr_model average with it")
    if lr_model != "average":
        return None
    if args.model == "wire":
        raise ValueError("--lr_model average / --footprint box run on the SIREN's fit kernels: not with --model wire")
    if external_fit:
        raise ValueError("--lr_model average / --footprint box are superresDWI's own fit: another driver's fit is point-sampled on "
                         "the decimation grid")
    if getattr(args, "zerofill", False):
        raise ValueError("--lr_model average cannot be combined with --zerofill: zero-filling is defined on the decimation grid "
                         "(LR sample j on HR sample 2j)")
    if (args.roi_end - args.roi_start) % 2:
        raise ValueError(f"--lr_model average takes 2 x 2 block means and needs an even ROI side (got {args.roi_end - args.roi_start})")
    if footprint == "box" and not 1 <= args.footprint_samples <= 8:
        raise ValueError(f"--footprint_samples must be 1 .. 8 per axis (S x S <= 64 sub-samples; got {args.footprint_samples})")
    if args.pertubation_epochs > 0:
        return ("holds single acquisitions, and --pertubation_epochs > 0 asks for the PerturbNet phase, which is point-sampled: "
                "with --lr_model average pass --pertubation_epochs 0 to fit the mean image only")
    return None


def _check_model(args):
    """``--model wire``: refuses what has no WIRE kernels, before the input is loaded and anything touches the device.
    Returns the reason for which an input with single acquisitions is to be refused (None: it is served)."""
    if args.model != "wire":
        if getattr(args, "wire_derivative_maps", False):
            raise ValueError("--wire_derivative_maps differentiates the WIRE network and needs --model wire; the SIREN's maps are "
                             "--derivative_maps")
        return None
    _check_wire(args)
    if args.pertubation_epochs > 0:
        return ("holds single acquisitions, and --pertubation_epochs > 0 asks for the PerturbNet phase: it needs the "
                "network's input gradient through the Fourier map, which this driver does not run for --model wire "
                "(scripts/wiretest.py, the notebook's own loop, does); "
                "pass --pertubation_epochs 0 to fit the mean image only")
    return None


def _check_wire(args):
    """The outputs and shapes no WIRE kernel serves (also ``scripts/wiretest.py``'s refusals).  ``--derivative_maps`` is the SIREN's
    flag and keeps its refusal; the WIRE network's maps are ``--wire_derivative_maps``."""
    if args.derivative_maps:
        raise ValueError("--derivative_maps needs the forward-mode derivative kernels, which exist for the SIREN only: "
                         "there are no derivative maps of a WIRE network (--model wire)")
    if args.hidden_dim // 2 not in wire.HIDDEN_SIZES or not 0 <= args.num_layers <= wire.MAX_HIDDEN_LAYERS or \
            not 1 <= 2 * args.mapping_size <= wire.MAX_IN_FEATURES:
        raise ValueError(f"--model wire serves hidden_dim // 2 in {wire.HIDDEN_SIZES}, num_layers <= {wire.MAX_HIDDEN_LAYERS} "
                         f"and 2 * mapping_size <= {wire.MAX_IN_FEATURES} (got hidden_dim {args.hidden_dim}, num_layers "
                         f"{args.num_layers}, mapping_size {args.mapping_size})")


def _check_optional_outputs(args, path, mean_img, bvalues, signal_scale):
    """Refuses --transverse_length / --adc / --tv_joint / --tv_adc on an input that cannot give them, before the fit starts."""
    nz, nb = mean_img.shape[2], mean_img.shape[3]
    if args.transverse_length < 0:
        raise ValueError(f"--transverse_length must be >= 0 (got {args.transverse_length})")
    if args.transverse_length and nz < 4:
        raise ValueError(f"--transverse_length: the through-plane cubic spline needs at least 4 slices (scipy interp1d "
                         f"kind='cubic'); {path} has {nz}")
    if getattr(args, "zerofill", False):
        if not 0.0 <= args.zerofill_apodize <= 1.0:
            raise ValueError(f"--zerofill_apodize must be in [0, 1] (got {args.zerofill_apodize})")
        if (args.roi_end - args.roi_start) % 2:
            raise ValueError(f"--zerofill re-samples every second pixel of the ROI back onto its grid with a mirrored boundary, which "
                             f"needs an even ROI side (got {args.roi_end - args.roi_start})")
    if getattr(args, "tv_joint", False) and not 2 <= nb <= baselines.ops.TVJ_MAX_CHANNELS:
        raise ValueError(f"--tv_joint couples the b-values of a slice and needs 2 .. {baselines.ops.TVJ_MAX_CHANNELS} of them; {path} "
                         f"has {nb}")
    if getattr(args, "tv_adc", False):
        b = np.asarray(bvalues, np.float64).reshape(-1)
        if not 2 <= nb <= baselines.ops.TVJ_MAX_CHANNELS:
            raise ValueError(f"--tv_adc fits one decay over the b-values of a slice and needs 2 .. {baselines.ops.TVJ_MAX_CHANNELS} of them; "
                             f"{path} has {nb}")
        if len(b) != nb or not np.isfinite(b).all() or (b < 0).any() or np.ptp(b) == 0:
            raise ValueError(f"--tv_adc needs {nb} distinct, finite b-values >= 0 (variable 'b'); {path} gives {list(bvalues)}")
    if args.adc:
        if nb < 2:
            raise ValueError(f"--adc needs at least 2 b-values; {path} has {nb}")
        if len(bvalues) != nb or np.ptp(bvalues) == 0:
            raise ValueError(f"--adc needs {nb} distinct b-values (variable 'b'); {path} gives {list(bvalues)}")
        if signal_scale is None:
            raise ValueError(f"--adc rescales by maxes[b, 1] (TE index 1, superresDWI.py:193); {path} has a single TE")


def _coronal(INR, B, mean_img, test_shape, args, reconstruct=inr.reconstruct):
    """superresDWI.py:217-241: the INR on a (2R, 2R, T, 1) grid -- the size-1 last axis puts b at -1, b index 0 -- without the
    clamp (:221), and the cubic spline of the HR ROI's b = 0 image along z (:231; the spline runs per line, so cropping the ROI
    first changes nothing).  -> (variables of coronal.mat, seconds)."""
    T = int(args.transverse_length)
    r0, r1 = args.roi_start, args.roi_end
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sr = reconstruct(INR, (test_shape[0], test_shape[1], T, 1), B, clamp_min=None)[..., 0]
    hr0 = torch.from_numpy(np.ascontiguousarray(mean_img[r0:r1, r0:r1, :, 0], dtype=np.float64)).cuda()
    spline = baselines.resize_z(hr0, T)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    return {"coronal_sr": sr.cpu().numpy(), "coronal_spline": spline.cpu().numpy(), "transverse_length": T}, t


def _zerofill(hs, factor, apodize):
    """Every second pixel of the [.., R, R] stack ``hs`` re-sampled to ``factor`` times its grid by k-space zero-filling, sample 0 on
    sample 0, mirrored boundary, clamped at 0 (a magnitude image)."""
    lr = hs[..., ::2, ::2].contiguous()
    return baselines.fourier_resize(lr, (factor * lr.shape[-2], factor * lr.shape[-1]), 'sample', 'mirror', apodize).clamp_min(0)


def _tv_kernel(average):
    """The block kernel of the LR model: the 2 x 2 mean of ``--lr_model average``, else the decimation (LR sample j on HR sample 2j)."""
    return "mean" if average else "decimate"


def _tv_baseline(ls, args, average):
    """``--tv_baseline``: the [Z, B, R/2, R/2] LR stack ``ls`` -> the [Z, B, R, R] TV / Huber reconstruction under the LR model's operator."""
    return baselines.tv_superres(ls, (2, 2), _tv_kernel(average), args.tv_lambda, args.tv_huber, args.tv_iters)


def _tv_joint(ls, args, average):
    """``--tv_joint``: the [Z, B, R/2, R/2] LR stack ``ls`` -> the [Z, B, R, R] reconstruction with one prior over the B channels of a
    slice; the weights of ``sqrt_signal`` are one host read of B means, before the solve."""
    mu = baselines.channel_weights(ls, args.tv_joint_weights)
    return baselines.tv_superres_joint(ls, (2, 2), _tv_kernel(average), args.tv_joint_lambda, args.tv_huber, args.tv_iters, mu)


def _tv_tgv(ls, args, average):
    """``--tv_tgv``: the [Z, B, R/2, R/2] LR stack ``ls`` -> the [Z, B, R, R] second-order TGV reconstruction, every image on its own,
    under the LR model's operator."""
    return baselines.tgv_superres(ls, (2, 2), _tv_kernel(average), args.tv_tgv_lambda, args.tv_tgv_ratio, args.tv_huber, args.tv_iters)


def _tv_adc(ls, args, average, bvalues, signal_scale):
    """``--tv_adc``: the [Z, B, R/2, R/2] LR stack ``ls`` -> {"s0", "adc" [Z, R, R], "images" [Z, B, R, R], "unit"}: the maps of the
    mono-exponential model solved on the stack in the signal's own units -- every b-image times its ``signal_scale`` over the largest
    (``unit``), so that the data stay within [0, 1] --, and the model's images back in the units of ``ls``."""
    scale = torch.ones(ls.shape[1], dtype=ls.dtype, device=ls.device) if signal_scale is None else \
        torch.as_tensor(np.asarray(signal_scale, np.float32), device=ls.device)
    unit = float(scale.max())
    rel = (scale / unit)[None, :, None, None]
    s0, adc = baselines.tv_superres_adc((ls * rel).contiguous(), [float(v) for v in bvalues], (2, 2), _tv_kernel(average), args.tv_adc_lambda,
                                        baselines.ADC_DEFAULT_HUBER, args.tv_adc_iters, (1.0, args.tv_adc_weight))
    images = baselines.adc_signal(s0.contiguous(), adc.contiguous(), [float(v) for v in bvalues]) / rel
    return {"s0": s0, "adc": adc, "images": images.contiguous(), "unit": unit}


def _nlm_baseline(ls, args, average):
    """``--nlm_baseline``: the [Z, B, R/2, R/2] LR stack ``ls`` -> the [Z, B, R, R] non-local upsampling: every b-value's [Z, R/2, R/2]
    volume by the factors (1, 2, 2) under the LR model's operator."""
    k = [1.0, 0.0] if not average else [0.5, 0.5]
    out = baselines.nlm_upsample(ls.permute(1, 0, 2, 3).contiguous(), (1, 2, 2), ([1.0], k, k), baselines.NLM_DEFAULT_LEVELS, args.nlm_iters,
                                 args.nlm_search, args.nlm_patch)
    return out.permute(1, 0, 2, 3).contiguous()


def _check_nlm(args, fit=None):
    """``--nlm_baseline``: what it cannot serve, before the input is loaded and anything touches the device."""
    if not getattr(args, "nlm_baseline", False):
        return
    if (args.roi_end - args.roi_start) % 2:
        raise ValueError(f"--nlm_baseline solves for 2 x 2 HR pixels per LR pixel and needs an even ROI side (got "
                         f"{args.roi_end - args.roi_start})")
    ops.nlm_radii("--nlm_baseline", args.nlm_search, args.nlm_patch)
    ops.nlm_schedule("--nlm_baseline", baselines.NLM_DEFAULT_LEVELS, args.nlm_iters, 1.0)
    if fit is not None and getattr(fit, "changes_lr_data", False):
        raise ValueError("--nlm_baseline solves on the LR ROI this driver forms: not with a fit hook that changes the LR data "
                         "(changes_lr_data)")


def _check_tv(args, fit=None):
    """``--tv_baseline`` / ``--tv_joint`` / ``--tv_tgv`` / ``--tv_adc``: what they cannot serve, before the input is loaded and anything touches the
    device."""
    if getattr(args, "tv_tgv", False):
        if not getattr(args, "tv_baseline", False):
            raise ValueError("--tv_tgv is scored beside the first-order reconstruction: pass --tv_baseline with it")
        if not 0.0 <= args.tv_tgv_lambda < float("inf"):
            raise ValueError(f"--tv_tgv_lambda must be finite and >= 0 (got {args.tv_tgv_lambda})")
        if not 0.0 < args.tv_tgv_ratio < float("inf"):
            raise ValueError(f"--tv_tgv_ratio must be finite and > 0 (got {args.tv_tgv_ratio})")
    if getattr(args, "tv_adc", False):
        if not getattr(args, "tv_baseline", False):
            raise ValueError("--tv_adc is scored beside the per-channel reconstruction: pass --tv_baseline with it")
        if not 0.0 <= args.tv_adc_lambda < float("inf"):
            raise ValueError(f"--tv_adc_lambda must be finite and >= 0 (got {args.tv_adc_lambda})")
        if not 0.0 <= args.tv_adc_weight <= 1.0:
            raise ValueError(f"--tv_adc_weight must be within [0, 1] (got {args.tv_adc_weight})")
        if not 1 <= args.tv_adc_iters <= 100000:
            raise ValueError(f"--tv_adc_iters must be 1 .. 100,000 (got {args.tv_adc_iters})")
    if getattr(args, "tv_joint", False):
        if not getattr(args, "tv_baseline", False):
            raise ValueError("--tv_joint is scored beside the per-channel reconstruction: pass --tv_baseline with it")
        if not 0.0 <= args.tv_joint_lambda < float("inf"):
            raise ValueError(f"--tv_joint_lambda must be finite and >= 0 (got {args.tv_joint_lambda})")
        if args.tv_joint_weights not in ("equal", "sqrt_signal"):
            raise ValueError(f"--tv_joint_weights must be equal or sqrt_signal (got {args.tv_joint_weights})")
    if not getattr(args, "tv_baseline", False):
        return
    if (args.roi_end - args.roi_start) % 2:
        raise ValueError(f"--tv_baseline solves for 2 x 2 HR pixels per LR pixel and needs an even ROI side (got "
                         f"{args.roi_end - args.roi_start})")
    if not 0.0 <= args.tv_lambda < float("inf"):
        raise ValueError(f"--tv_lambda must be finite and >= 0 (got {args.tv_lambda})")
    if not 0.0 <= args.tv_huber < float("inf"):
        raise ValueError(f"--tv_huber must be finite and >= 0 (got {args.tv_huber})")
    if not 1 <= args.tv_iters <= 100000:
        raise ValueError(f"--tv_iters must be 1 .. 100,000 (got {args.tv_iters})")
    if fit is not None and getattr(fit, "changes_lr_data", False):
        raise ValueError("--tv_baseline solves on the LR ROI this driver forms: not with a fit hook that changes the LR data "
                         "(changes_lr_data)")


def _adc_maps(recon, hs, bvalues, signal_scale, zerofill_apodize=None, ls=None, tv=None, tvj=None, tgv=None, nlm=None):
    """superresDWI.py:189-206 for all slices in one batch: every b-image times maxes[b, 1], then calculate_ADC per pixel, of
    the x2 SR volume, the x4 spline of the LR ROI and the x2 spline of the HR ROI.  ``hs`` is the HR ROI as [Z, B, R, R].
    ``zerofill_apodize`` (not None): also ``adc_zerofill``, the x4 zero-fill of the LR ROI, on the grid of ``adc_spline``.
    ``ls``: the LR ROI as [Z, B, R/2, R/2] (default: every second pixel of ``hs``; ``--lr_model average``: the block means).
    ``tv`` / ``tvj`` / ``tgv`` (not None): also ``adc_tv`` / ``adc_tv_joint`` / ``adc_tv_tgv`` of the [Z, B, R, R] TV / TGV
    reconstructions, on the grid of the HR ROI; ``nlm`` (not None): also ``adc_nlm`` of the non-local upsampling, on that grid."""
    scale = torch.as_tensor(np.asarray(signal_scale, np.float32), device=recon.device)
    to_xyzb = lambda t: t.permute(2, 3, 0, 1).contiguous()                       # [Z, B, 2R, 2R] -> [2R, 2R, Z, B]
    stacks = {"adc_sr": recon,
              "adc_spline": to_xyzb(baselines.rescale(hs[:, :, ::2, ::2].contiguous() if ls is None else ls, 4)),
              "adc_hr": to_xyzb(baselines.rescale(hs, 2))}
    if zerofill_apodize is not None:
        stacks["adc_zerofill"] = to_xyzb(_zerofill(hs, 4, zerofill_apodize))
    if tv is not None:
        stacks["adc_tv"] = to_xyzb(tv)
    if tvj is not None:
        stacks["adc_tv_joint"] = to_xyzb(tvj)
    if tgv is not None:
        stacks["adc_tv_tgv"] = to_xyzb(tgv)
    if nlm is not None:
        stacks["adc_nlm"] = to_xyzb(nlm)
    out ={k: metrics.calculate_ADC_device(bvalues, (v * scale).contiguous()).cpu().numpy() for k, v in stacks.items()}
    out["b"] = np.asarray(bvalues, np.float64)
    return out


def _derivative_maps(INR, B, test_shape, derivatives=inr.derivatives):
    """nn_mri.py:205-221 on the grid of ``recon``: tangents along the three spatial axes only (the b-value axis is the last of the
    grid and is not differentiated along).  ``derivatives``: ``inr.derivatives`` or ``wire.derivatives``, by the network."""
    d = derivatives(INR, shape=test_shape, B=B, d_tangent=min(3, len(test_shape)))
    grad_mag = torch.sqrt((d.gradient * d.gradient).sum(dim=-1))
    return {"grad_mag": grad_mag.cpu().numpy(), "laplacian": d.laplacian.cpu().numpy()}


SUMMARY_KEYS = ("job", "n_coords", "steps", "t_fit_s", "t_recon_s", "train_voxels_per_s", "final_loss", "psnr_db",
                "psnr_spline_db", "ssim_sr_mean", "ssim_spline_mean")


def main(argv=None, parser=None, run=None):
    """``parser`` / ``run``: another driver's flags and per-patient function on this loop (``scripts/wiretest.py``).
    The patient loop (superresDWI.py:29).  Under ``torchrun`` (one process per GPU, WORLD_SIZE > 1) the patients are dealt
    over the ranks -- longest first by file size, the same deterministic ``dist.partition_fits`` schedule on every rank, no
    data-path collective --, every rank writes the outputs of its own patients, and ONE all_gather (RCCL) hands every rank
    the numeric summaries of all of them (rank 0 prints the list)."""
    args = (parser or build_parser()).parse_args(argv)
    run_patient = run or globals()["run_patient"]
    ids = args.pt_id if args.pt_id else [_patient_id(p) for p in args.data]
    if len(ids) != len(args.data):
        raise SystemExit("--pt_id needs one id per --data file")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return [run_patient(p, i, args) for p, i in zip(args.data, ids)]
    import torch.distributed as dist
    from mri_super_resolution_amd import dist as inr_dist
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(os.environ.get("INR_BACKEND", "nccl"))
    rank = dist.get_rank()
    plan = inr_dist.partition_fits([float(os.path.getsize(p)) for p in args.data], world)
    local = []
    for job in plan[rank]:
        s = run_patient(args.data[job], ids[job], args)
        local.append({**{k: float(s[k]) for k in SUMMARY_KEYS if k != "job"}, "job": float(job)})
    max_jobs = max(len(p) for p in plan)
    records = sorted(inr_dist.gather_job_records(local, SUMMARY_KEYS, max_jobs), key=lambda r: r["job"])
    out = [{**r, "pt_id": str(ids[int(r["job"])]), "input": os.path.abspath(args.data[int(r["job"])]),
            "rank": next(k for k, jobs in enumerate(plan) if int(r["job"]) in jobs)} for r in records]
    if rank == 0:
        print(json.dumps({"patients": out, "world_size": world}))
    return out


if __name__ == "__main__":
    main()
