#!/usr/bin/env python3
"""``multi-image-super-resolution/master.py`` of the reference on the MI355X path: per patient the cancer slice of the DWI series
``[X, Y, Z, T]`` is cast to uint16 and multiplied by 256 (master.py:40-42), ``sample_size = 25`` random 9-acquisition subsets are
super-resolved x3 by ``RAMS(3, 32, 3, 9, 8, 12)`` through ``predict_tensor`` and averaged (:43-52), and the ADC map is
``-log(mean / (rescale(b0, 3) + eps) + eps) / b * 1e6`` (:53-57).  The 25 forwards run as ONE batched call.

Flags: the reference's three (master.py:13-15: ``--out_folder``, ``--out_img_folder``, ``--exp_name``) with the same names and
defaults, plus what the reference hard-codes or leaves undefined: ``--data_dir`` / ``--cases`` (the patient table ``cases`` that
master.py:1 imports was never published: a JSON list of ``case`` constructor arguments, as for ``scripts/master.py``),
``--ssim`` (adds ``cssim_vs_rescaled`` to every case record: the shift-tolerant SSIM of ``utils/loss.py:131-177`` between the
super-resolved mean and the x3 linear rescale of the acquisition mean of the same slice -- there is no high-resolution label at
inference, so this is a structure-agreement figure; without the flag nothing is computed or written differently),
``--register`` / ``--register_max_shift N`` (the slice's acquisitions are laid on acquisition 0 by masked cross-correlation within
``N`` pixels, default 8, and a cubic-spline shift -- ``register_imgset`` of ``utils/preprocessing.py:138-161`` with all-clear masks,
whose first-maximum rule picks acquisition 0 -- before the uint16 cast, and every case record gains ``shifts`` [T, 2]; master.py
averages its subsets without ever aligning them, and without the flag nothing is computed or written differently),
``--weights`` (an ``.npz`` of the network's variables, ``RAMS.save_weights``: the checkpoint under ``ckpt/RED_RAMS`` that
master.py:27-33 restores is shipped WITHOUT its ``*.data-00001-of-00002`` shard and there is no TensorFlow here to read one --
without ``--weights`` the network keeps its random initialisation and the script says so), ``--sample_size`` (25) and ``--seed``
(the reference draws the subsets from the unseeded ``random`` module) and ``--tv_multiframe`` with ``--tv_lambda --tv_huber --tv_iters
--tv_upsample`` (the classical multi-frame comparator, DESIGN.md 4n: ALL acquisitions of the slice divided by their maximum, their
sub-pixel shifts against acquisition 0 by ``baselines.estimate_shifts``, ``baselines.tv_superres_multi`` at x3 with the mean kernel,
scaled back -- ``DWI_tvmf.npy`` / ``ADC_tvmf.npy`` and the same two keys in ``images.mat``, ``tvmf_shifts``, ``tvmf_energy`` and
``tvmf_valid_fraction`` in the case record, ``cssim_tvmf_vs_rescaled`` with ``--ssim``; the RAMS path is not touched, and without the
flag nothing is computed or written differently).  ``save_dicom`` (master.py:58-62) is replaced by
``<out_img_folder>/<exp_name>/<pt_no>/images.mat`` + ``DWI_mean.npy`` / ``ADC_mean.npy`` (DICOM export is out of scope).
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))
from mri_super_resolution_amd import baselines, contrast, matio, registration  # noqa: E402
from mri_super_resolution_amd.rams import RAMS, predict_tensor, ssim_per_image  # noqa: E402

SCALE = 3           # master.py:20-26
FILTERS = 32
KERNEL_SIZE = 3
CHANNELS = 9
R = 8
N = 12
eps = 1e-7


def build_parser():
    parser = argparse.ArgumentParser(description='Superresolution of DWI/ADC maps with Multi-image SR')
    parser.add_argument('--out_folder', default='../experiments.mi/', help='directory to save the quantitative results')
    parser.add_argument('--out_img_folder', default='../output_images.mi/', help='directory to save the images')
    parser.add_argument('--exp_name', default='sr2', help='name of the experiment')
    parser.add_argument('--data_dir', default='../anon_data', help='directory of patNN_alldata / _mean_b0 .mat files')
    parser.add_argument('--cases', default=None, help='JSON file: list of {pt_id, b, cancer_loc, contralateral_loc, noise, '
                                                      'cancer_slice, acquisitions}')
    parser.add_argument('--weights', default=None, help='.npz of the RAMS variables (<layer>/v|g|b); random initialisation otherwise')
    parser.add_argument('--sample_size', type=int, default=25, help='random 9-acquisition subsets per case (master.py:44)')
    parser.add_argument('--seed', type=int, default=None, help='seed of the subset draws (the reference draws unseeded)')
    parser.add_argument('--ssim', action='store_true', help='add cssim_vs_rescaled (cSSIM, utils/loss.py:131-177, of the mean '
                                                            'prediction against the rescaled acquisition mean) to every case record')
    parser.add_argument('--register', action='store_true', help='register the acquisitions of the slice to acquisition 0 before the '
                                                                'uint16 cast and add shifts [T, 2] to every case record')
    parser.add_argument('--register_max_shift', type=int, default=8, help='search window of --register in pixels per axis')
    parser.add_argument('--tv_multiframe', action='store_true', help='also reconstruct the slice x3 from ALL its acquisitions by '
                        'baselines.tv_superres_multi with estimated sub-pixel shifts: DWI_tvmf / ADC_tvmf beside the RAMS outputs')
    parser.add_argument('--tv_lambda', type=float, default=baselines.TVMF_DEFAULT_LAMBDA,
                        help='--tv_multiframe: weight of the prior (data scaled to [0, 1]; not divided by the number of acquisitions)')
    parser.add_argument('--tv_huber', type=float, default=baselines.TVMF_DEFAULT_HUBER, help='--tv_multiframe: Huber threshold; 0 = TV')
    parser.add_argument('--tv_iters', type=int, default=baselines.TVMF_DEFAULT_ITERS, help='--tv_multiframe: iterations, 1 .. 100,000')
    parser.add_argument('--tv_upsample', type=int, default=4, help='--tv_multiframe: up-sampling of the shift estimate, 1 .. 16 '
                        '(the step is 3 / this in HR pixels; the search window is --register_max_shift)')
    return parser


def check_tv_multiframe(args):
    """The refusals of the --tv_multiframe flags, before any case is loaded; without the flag its values are not looked at."""
    if not getattr(args, "tv_multiframe", False):
        return
    for name in ("tv_lambda", "tv_huber"):
        if not 0.0 <= getattr(args, name) < float("inf"):
            raise ValueError(f"--{name} must be finite and >= 0 (got {getattr(args, name)!r})")
    if not 1 <= args.tv_iters <= 100000:
        raise ValueError(f"--tv_iters must be 1 .. 100,000 (got {args.tv_iters})")
    if not 1 <= args.tv_upsample <= 16:
        raise ValueError(f"--tv_upsample must be 1 .. 16 (got {args.tv_upsample})")
    if args.register_max_shift < 0:
        raise ValueError(f"--register_max_shift must be >= 0 (got {args.register_max_shift})")


def tv_multiframe_case(case, scale=SCALE, lam=baselines.TVMF_DEFAULT_LAMBDA, huber=baselines.TVMF_DEFAULT_HUBER,
                       n_iter=baselines.TVMF_DEFAULT_ITERS, upsample=4, max_shift=8):
    """The classical multi-frame comparator of the RAMS mean: ALL acquisitions [X, Y, T] of the cancer slice, divided by their
    maximum, their shifts against acquisition 0 by ``baselines.estimate_shifts`` (in HR pixels, searched within ``max_shift`` LR
    pixels), ``baselines.tv_superres_multi`` at x``scale`` with the mean kernel, scaled back; the ADC by the formula of
    ``super_resolve_case``.  Returns ``(dwi [3X, 3Y] float64, adc, shifts [T, 2], info)``."""
    seq = np.asarray(case.dwi[:, :, case.cancer_slice, :], np.float64)
    top = float(seq.max())
    if not top > 0.0:
        raise ValueError(f"{case.pt_id}: the acquisitions of slice {case.cancer_slice} are all zero")
    frames = np.ascontiguousarray(seq.transpose(2, 0, 1)) / top
    shifts = baselines.estimate_shifts(frames, (scale, scale), upsample, max_shift)
    x, info = baselines.tv_superres_multi(frames, (scale, scale), shifts, "mean", lam, huber, n_iter, return_info=True)
    dwi = x * top
    b0 = np.asarray(case.b0[:, :, case.cancer_slice], np.float64)
    b0_scaled = baselines.rescale(b0, scale, anti_aliasing=False)
    adc = -np.log((dwi / (b0_scaled + eps)) + eps) / case.b
    adc *= 1000000
    return dwi, adc, shifts, info


def register_slice(case, max_shift=8):
    """The acquisitions [X, Y, T] of the cancer slice laid on acquisition 0 (all masks clear: the first of the equal clearances is
    the reference); returns ``(registered float64 [X, Y, T], shifts [T, 2])``."""
    seq = np.asarray(case.dwi[:, :, case.cancer_slice, :], np.float64)
    reg, _, shifts = registration.register_imgset(seq, np.ones(seq.shape), max_shift=max_shift, return_shifts=True)
    return np.clip(reg, 0.0, None), shifts                                                  # the cubic overshoots: the cast is unsigned


def super_resolve_case(model, case, sample_size=25, rng=random, low_res_seq=None):
    """master.py:38-57 for one patient; returns ``(mean_pred [3X, 3Y] float64, adc_large, subsets)``.  ``low_res_seq`` replaces the
    slice's acquisitions [X, Y, T] (``register_slice``)."""
    _low_res_seq = case.dwi
    num_acq = _low_res_seq.shape[3]
    if low_res_seq is None:
        low_res_seq = _low_res_seq[:, :, case.cancer_slice, :]
    lor = np.expand_dims(low_res_seq, 0).astype('uint16')
    lor = lor * 256
    channels = model.cfg["channels"]
    if num_acq < channels:
        raise ValueError(f"{case.pt_id}: {num_acq} acquisitions, the network takes {channels} per forward")
    subsets = [rng.sample(list(range(num_acq)), channels) for _ in range(sample_size)]
    batch = np.concatenate([lor[:, :, :, inx] for inx in subsets], axis=0)                  # the 25 forwards as one batch
    sr = predict_tensor(model, batch)[:, :, :, 0]
    mean_pred = sr.double().sum(dim=0).cpu().numpy() / sample_size                          # mean_pred += img; /= sample_size
    b0 = np.asarray(case.b0[:, :, case.cancer_slice], np.float64)
    b0_scaled = baselines.rescale(b0, model.cfg["scale"], anti_aliasing=False)              # master.py:55
    adc_large = -np.log((mean_pred / (b0_scaled + eps)) + eps) / case.b
    adc_large *= 1000000
    return mean_pred, adc_large, subsets


def cssim_vs_rescaled(mean_pred, case, scale):
    """cSSIM (7 x 7 shifts, all pixels clear) of the super-resolved mean against the linear x``scale`` rescale of the acquisition
    mean of the same x256 uint16 slice, on the central square of a non-square slice."""
    lor = case.dwi[:, :, case.cancer_slice, :].astype('uint16') * 256                        # master.py:40-42
    ref = baselines.rescale(lor.astype(np.float64).mean(axis=-1), scale, anti_aliasing=False)
    s = min(mean_pred.shape)
    r0, c0 = (mean_pred.shape[0] - s) // 2, (mean_pred.shape[1] - s) // 2
    crop = lambda a: np.ascontiguousarray(a[r0:r0 + s, c0:c0 + s], np.float32)[None]
    return float(ssim_per_image(crop(ref), crop(mean_pred), np.ones((1, s, s), np.float32), size_image=s)[0])


def run(args, cases):
    check_tv_multiframe(args)
    rams_network = RAMS(scale=SCALE, filters=FILTERS, kernel_size=KERNEL_SIZE, channels=CHANNELS, r=R, N=N, seed=0)
    if args.weights:
        rams_network.load_weights(args.weights)
    else:
        print("note: no --weights given -- the network keeps its random initialisation (the reference's checkpoints under "
              "ckpt/RED_RAMS are shipped without their data shard; convert a complete one to .npz with RAMS.save_weights' layout)",
              file=sys.stderr)
    rng = random.Random(args.seed) if args.seed is not None else random
    os.makedirs(args.out_folder, exist_ok=True)
    summary = []
    for case in cases:
        t0 = time.perf_counter()
        shifts = None
        if getattr(args, "register", False):
            registered, shifts = register_slice(case, args.register_max_shift)
            mean_pred, adc_large, subsets = super_resolve_case(rams_network, case, args.sample_size, rng, low_res_seq=registered)
        else:
            mean_pred, adc_large, subsets = super_resolve_case(rams_network, case, args.sample_size, rng)
        dt = time.perf_counter() - t0
        pt_no = case.pt_id.split('-')[-1]
        out_dir = os.path.join(args.out_img_folder, args.exp_name, pt_no)
        os.makedirs(out_dir, exist_ok=True)
        np.save(os.path.join(out_dir, 'DWI_mean.npy'), mean_pred)                            # instead of save_dicom (:58-62)
        np.save(os.path.join(out_dir, 'ADC_mean.npy'), adc_large)
        images = {'DWI_mean': mean_pred, 'ADC_mean': adc_large}
        tvmf = None
        if getattr(args, "tv_multiframe", False):
            tvmf = tv_multiframe_case(case, rams_network.cfg["scale"], args.tv_lambda, args.tv_huber, args.tv_iters, args.tv_upsample,
                                      args.register_max_shift)
            np.save(os.path.join(out_dir, 'DWI_tvmf.npy'), tvmf[0])
            np.save(os.path.join(out_dir, 'ADC_tvmf.npy'), tvmf[1])
            images.update(DWI_tvmf=tvmf[0], ADC_tvmf=tvmf[1])
        matio.savemat(os.path.join(out_dir, 'images.mat'), images)
        summary.append({"patient": pt_no, "shape": list(mean_pred.shape), "sample_size": args.sample_size, "seconds": dt,
                        "subsets": subsets, "out_dir": out_dir})
        if getattr(args, "ssim", False):
            summary[-1]["cssim_vs_rescaled"] = cssim_vs_rescaled(mean_pred, case, rams_network.cfg["scale"])
        if shifts is not None:
            summary[-1]["shifts"] = np.asarray(shifts).tolist()
        if tvmf is not None:
            summary[-1].update(tvmf_shifts=np.asarray(tvmf[2]).tolist(), tvmf_energy=float(tvmf[3]["energy"]),
                               tvmf_valid_fraction=float(tvmf[3]["valid_fraction"]))
            if getattr(args, "ssim", False):                                                 # on the x256 scale of the RAMS mean
                summary[-1]["cssim_tvmf_vs_rescaled"] = cssim_vs_rescaled(tvmf[0] * 256.0, case, rams_network.cfg["scale"])
    with open(os.path.join(args.out_folder, args.exp_name + '.json'), 'w') as fh:
        json.dump({"weights": args.weights, "cases": summary}, fh)
    return {"cases": summary, "weights": args.weights}


def load_cases(args):
    if args.cases is None:
        return list(contrast.cases)
    with open(args.cases) as fh:
        specs = json.load(fh)
    return [contrast.case(s['pt_id'], s['b'], tuple(s['cancer_loc']), tuple(s['contralateral_loc']), tuple(s['noise']),
                          s['cancer_slice'], np.asarray(s['acquisitions']), data_dir=args.data_dir) for s in specs]


def main(argv=None):
    args = build_parser().parse_args(argv)
    cases = load_cases(args)
    if not cases:
        raise SystemExit("no cases: pass --cases cases.json (the reference's module-level `cases` list was never published)")
    out = run(args, cases)
    print(json.dumps({"cases": [{k: v for k, v in c.items() if k != "subsets"} for c in out["cases"]], "weights": out["weights"]}))
    return out


if __name__ == "__main__":
    main()
