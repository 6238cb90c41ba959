"""The joint b-value study: what does a TV / Huber reconstruction of a DWI slice gain from ONE prior over its b-values?

``superresDWI --tv_baseline`` regularises every b-image of a slice on its own.  This driver makes noisy LR slices of a 4-D volume with
a ground truth and scores the same prior per image and coupled: it loads and normalises a volume as ``superresDWI`` does (a 4-D volume
with its variable ``b``), crops the in-plane ROI, and makes of every slice and b-value one LR image with the block operator of
``--kernel`` (``mean``, the default, or ``decimate``) at ``--factor`` (default 2) plus Gaussian noise of ``--noise`` (``--seed``; slice z
draws from ``default_rng(seed * 1000 + z)``).  ``--synthetic_adc`` takes a 3-D volume (or the first b-value of a 4-D one) instead and
gives it a mono-exponential decay over b = 0 / 150 / 1000 / 1500 whose ADC is high where the smoothed image is dark
(``drivers.synthetic_decay``), the study case of the design note.  The LR stack is reconstructed on the device by

  replicate  block replication;
  tv         ``baselines.tv_superres`` with ``--tv_lambda``: every image on its own;
  tv_joint   ``baselines.tv_superres_joint`` with ``--tv_joint_lambda`` and the channel weights of ``--weights``: the b-values of a
             slice are the channels of one group.

``--with_adc_model [--tv_adc_lambda LA --tv_adc_weight M --tv_adc_iters NA]`` adds

  tv_adc     ``baselines.tv_superres_adc``: the S0 / ADC maps of a slice are the unknowns; its images are the model's,
             ``s0 exp(-b adc)``, and its ``adc_rmse_tv_adc`` is the SOLVER'S map against the HR data's; ``adc_rmse_loglinear_tv_adc`` is the
             log-linear fit of its images, for comparison.  ``joint_bvalues.mat`` gains ``s0_tv_adc`` and ``adc_loglinear_tv_adc``.

Without the flag every output is byte for byte what it was.  Both TV rows use ``--tv_huber --tv_iters``.  Per patient, under ``<output_address>/pat<id>/``: ``joint_bvalues.csv`` (one row per slice
and b-value: ``Pt_id, b-value, slice``, then ``SSIM-<method>`` and ``PSNR-<method>`` for the three methods), ``metrics.json``
(``psnr_<method>_db`` over everything, ``psnr_<method>_b<value>_db`` per b-value, ``ssim_<method>_mean``, ``adc_rmse_<method>``: the RMSE
of the log-linear ADC against the HR data's inside ``b_min image > 0.25 max``, the channel weights and the arguments) and
``joint_bvalues.mat`` (``hr``, ``lr`` and the reconstructions [X, Y, Z, B], the ADC maps [X, Y, Z], ``b``).  Every flag is checked
before the input is loaded."""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from mri_super_resolution_amd import baselines, drivers, matio
from mri_super_resolution_amd.scripts.superresDWI import _patient_id, load_input_and_scale


def build_parser():
    p = argparse.ArgumentParser(description="Joint b-value study: TV / Huber per image against one prior over the b-values of a slice")
    p.add_argument("--data", nargs="+", required=True, help=".mat file(s): a 4-D volume with 'b' (3-D with --synthetic_adc)")
    p.add_argument("--key", default=None, help="variable holding the volume (default: hybrid_raw, else the only array)")
    p.add_argument("--pt_id", nargs="*", default=None, help="patient ids for the CSV (default: digits of the file name)")
    p.add_argument("--output_address", default="JB_results", help="output directory (one sub-directory per patient)")
    p.add_argument("--factor", type=int, default=2, help="HR pixels per LR pixel and axis, 1 .. 8")
    p.add_argument("--kernel", choices=("mean", "decimate"), default="mean", help="the block operator that makes the LR images")
    p.add_argument("--noise", type=float, default=0.02, help="sigma of the noise added to every LR image (data in [0, 1])")
    p.add_argument("--seed", type=int, default=0, help="seeds the noise")
    p.add_argument("--tv_lambda", type=float, default=baselines.TV_DEFAULT_LAMBDA, help="weight of the per-image prior")
    p.add_argument("--tv_joint_lambda", type=float, default=baselines.TVJ_DEFAULT_LAMBDA,
                   help="weight of the coupled prior (the sweep of DESIGN.md 4q)")
    p.add_argument("--tv_huber", type=float, default=baselines.TVJ_DEFAULT_HUBER,
                   help="Huber threshold on the gradient magnitude of both TV rows; 0 = plain isotropic TV")
    p.add_argument("--tv_iters", type=int, default=baselines.TVJ_DEFAULT_ITERS, help="Chambolle-Pock iterations, 1 .. 100,000")
    p.add_argument("--weights", choices=("equal", "sqrt_signal"), default="equal", help="channel weights of the coupled norm")
    p.add_argument("--roi_start", type=int, default=40)
    p.add_argument("--roi_end", type=int, default=90)
    p.add_argument("--slices", type=int, nargs="*", default=None, help="slice indexes (default: every slice)")
    p.add_argument("--synthetic_adc", action="store_true",
                   help="give a 3-D volume a mono-exponential decay over b = 0 / 150 / 1000 / 1500 (the study case)")
    p.add_argument("--with_adc_model", action="store_true",
                   help="add the row tv_adc: the S0 / ADC maps as the unknowns of one solve per slice (DESIGN.md 4t)")
    p.add_argument("--tv_adc_lambda", type=float, default=baselines.ADC_DEFAULT_LAMBDA, help="--with_adc_model: weight of the prior on the maps")
    p.add_argument("--tv_adc_weight", type=float, default=baselines.ADC_DEFAULT_MAP_WEIGHTS[1],
                   help="--with_adc_model: weight of the normalised ADC map in the prior, within [0, 1]")
    p.add_argument("--tv_adc_iters", type=int, default=baselines.ADC_DEFAULT_ITERS, help="--with_adc_model: iterations, 1 .. 100,000")
    return p


def _adc_model(args):
    return dict(lam=args.tv_adc_lambda, weight=args.tv_adc_weight, iters=args.tv_adc_iters) if args.with_adc_model else None


def check_args(args, n_b=None):
    """Every refusal of the flags, before the input is loaded and anything touches the device; returns the LR side."""
    if args.roi_start < 0 or args.roi_end <= args.roi_start:
        raise ValueError(f"ROI {args.roi_start}:{args.roi_end}: 0 <= roi_start < roi_end")
    n_b = (len(drivers.SYNTHETIC_B) if args.synthetic_adc else 2) if n_b is None else n_b
    m = drivers.check_joint_bvalues(args.roi_end - args.roi_start, n_b, args.factor, args.kernel, args.noise, args.tv_lambda,
                                    args.tv_joint_lambda, args.tv_huber, args.tv_iters, args.weights)
    if args.with_adc_model:
        drivers.check_adc_model(**_adc_model(args))
    if args.slices is not None and (not args.slices or min(args.slices) < 0):
        raise ValueError(f"--slices are indexes >= 0 (got {args.slices})")
    return m


def run_patient(path, pt_id, args):
    check_args(args)
    mean_img, _, bvalues, _, _ = load_input_and_scale(path, args.key)
    r0, r1 = args.roi_start, args.roi_end
    if r1 > min(mean_img.shape[:2]):
        raise ValueError(f"ROI {r0}:{r1} does not fit the {mean_img.shape[:2]} slices")
    which = list(range(mean_img.shape[2])) if args.slices is None else list(args.slices)
    if max(which) >= mean_img.shape[2]:
        raise ValueError(f"--slices {which}: the volume has {mean_img.shape[2]} slices")
    roi = np.ascontiguousarray(mean_img[r0:r1, r0:r1].transpose(2, 3, 0, 1), dtype=np.float64)[which]           # [Z, B, R, R]
    if args.synthetic_adc:
        b = np.asarray(drivers.SYNTHETIC_B, np.float64)
        hr = drivers.synthetic_decay(roi[:, 0] / roi[:, 0].max(), b)           # the selected ROI divided by its maximum
    else:
        b = np.asarray(bvalues, np.float64).reshape(-1)
        if roi.shape[1] < 2 or b.size != roi.shape[1] or np.ptp(b) == 0:
            raise ValueError(f"joint_bvalues needs a 4-D volume with >= 2 distinct b-values (variable 'b'); {path} has {roi.shape[1]} "
                             f"b-image(s) and b = {b.tolist()}: pass --synthetic_adc to give a 3-D volume a decay")
        hr = roi
    check_args(args, hr.shape[1])
    out_dir = os.path.join(args.output_address, f"pat{pt_id}")
    os.makedirs(out_dir, exist_ok=True)
    # slice z of the volume draws from seed * 1000 + z whatever --slices selects
    res = drivers.joint_bvalue_study(hr, b, args.factor, args.kernel, args.noise, args.seed, args.tv_lambda, args.tv_joint_lambda,
                                     args.tv_huber, args.tv_iters, args.weights, slice_ids=which, adc_model=_adc_model(args))
    methods = res["methods"]
    with open(os.path.join(out_dir, "joint_bvalues.csv"), "w") as fh:
        fh.write(", ".join(["Pt_id", "b-value", "slice"] + [f"SSIM-{name}" for name in methods] + [f"PSNR-{name}" for name in methods]) + "\n")
        for i, z in enumerate(which):
            for j in range(len(b)):
                fh.write(f"{pt_id}, {float(b[j])}, {z}, " + ", ".join([str(float(res["ssim"][name][i, j])) for name in methods] +
                                                                      [str(float(res["psnr"][name][i, j])) for name in methods]) + "\n")
    summary = {"pt_id": str(pt_id), "input": os.path.abspath(path), "roi": [r0, r1], "slices": which, "b": b.tolist(),
               "synthetic_adc": bool(args.synthetic_adc), "factor": int(args.factor), "kernel": args.kernel, "noise": args.noise,
               "seed": int(args.seed), "tv_lambda": args.tv_lambda, "tv_joint_lambda": args.tv_joint_lambda, "tv_huber": args.tv_huber,
               "tv_iters": int(args.tv_iters), "weights": args.weights, "channel_weights": [float(v) for v in res["channel_weights"]],
               "methods": list(methods)}
    if args.with_adc_model:
        summary.update(tv_adc_lambda=args.tv_adc_lambda, tv_adc_weight=args.tv_adc_weight, tv_adc_iters=int(args.tv_adc_iters))
    for name in methods:
        summary[f"psnr_{name}_db"] = res["psnr_all"][name]
        for j in range(len(b)):
            summary[f"psnr_{name}_b{b[j]:g}_db"] = float(res["psnr_b"][name][j])
        summary[f"ssim_{name}_mean"] = float(res["ssim"][name].mean())
        summary[f"adc_rmse_{name}"] = res["adc_rmse"][name]
    summary["tv_joint_energy_mean"] = float(res["info"]["tv_joint"]["energy"].mean())
    if args.with_adc_model:
        summary["adc_rmse_loglinear_tv_adc"] = res["adc_rmse_loglinear"]["tv_adc"]
        summary["tv_adc_energy_mean"] = float(res["info"]["tv_adc"]["energy"].mean())
    host = lambda t: t.cpu().numpy()
    mat = {name: host(res["images"][name]).transpose(2, 3, 0, 1) for name in methods}                                 # [X, Y, Z, B]
    mat.update({f"adc_{name}": host(v).transpose(1, 2, 0) for name, v in res["adc"].items()})                          # [X, Y, Z]
    if args.with_adc_model:
        mat.update(s0_tv_adc=host(res["s0"]["tv_adc"]).transpose(1, 2, 0), adc_loglinear_tv_adc=host(res["adc_loglinear"]["tv_adc"]).transpose(1, 2, 0))
    mat.update(hr=host(res["hr"]).transpose(2, 3, 0, 1), lr=host(res["lr"]).transpose(2, 3, 0, 1), b=b,
               slices=np.asarray(which, np.float64))
    matio.savemat(os.path.join(out_dir, "joint_bvalues.mat"), mat)
    with open(os.path.join(out_dir, "metrics.json"), "w") as fh:
        json.dump(summary, fh, indent=1)
    print(json.dumps(summary))
    return summary


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    ids = args.pt_id if args.pt_id else [_patient_id(p) for p in args.data]
    if len(ids) != len(args.data):
        raise SystemExit("--pt_id needs one id per --data file")
    return [run_patient(p, i, args) for p, i in zip(args.data, ids)]


if __name__ == "__main__":
    main()
