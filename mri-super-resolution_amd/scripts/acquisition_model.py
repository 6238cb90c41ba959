"""The acquisition-model study: what does a TV / Huber reconstruction gain from the forward model the data were made with?

Every other study of this project scores "TV" with the block mean as its forward model, whatever made the data.  This driver makes
the data three ways and scores the same prior with and without the right model, with a ground truth: it loads and normalises a volume
as ``superresDWI`` does, crops the in-plane ROI at the b-value ``--b_index``, and makes of every slice one LR slice with ``--model``

  kspace     k-space truncation, ``baselines.fourier_operator(align='center', boundary='mirror')``;
  gaussian   a Gaussian point-spread function of ``--fwhm`` LR pixels (default 1.2), ``baselines.psf_operator``;
  block      the block mean, ``baselines.block_operator``,

to ``side / --factor`` pixels a side (default 2) or to ``--lr_side`` pixels, which need not divide the side, plus Gaussian noise of
``--noise`` (``--seed``; slice z draws from ``default_rng(seed * 1000 + z)``) -- and reconstructs the slice on the device by

  spline       ``baselines.rescale`` (a whole ratio) or ``baselines.resize``;
  zerofill     ``baselines.fourier_resize``, 'center' / 'mirror';
  tv_block     ``baselines.tv_superres`` with the mean kernel -- skipped, and absent from every output, when the ratio is no whole
               number of blocks;
  tv_operator  ``baselines.tv_superres_operator`` with the operator that made the data;
  degibbs_zerofill, degibbs_spline   only with ``--with_degibbs``: the LR slice unrung on its own grid (``denoise.degibbs``, Gibbs-ringing
               removal by local sub-voxel shifts; the LR side must be at least 9), then re-sampled as ``zerofill`` /
               ``spline`` are.  For ``--model kspace``, whose LR slices ring by construction, this is the study that step exists for.

Both TV rows use ``--tv_lambda --tv_huber --tv_iters``.  Per patient, under ``<output_address>/pat<id>/``: ``acquisition_model.csv``
(one row per slice: ``Pt_id, b-value, slice``, ``SSIM-<method>`` for the methods that ran), ``metrics.json`` (``psnr_<method>_db`` and
``ssim_<method>_mean`` over the slices, ``tv_operator_consistency_psnr_db``: the PSNR of ``A tv_operator`` against the LR data, and
the arguments) and ``acquisition_model.mat`` (``hr``, ``lr`` and the reconstructions [X, Y, Z], the operators ``R0`` / ``R1``).  Every
flag is checked before the input is loaded."""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from mri_super_resolution_amd import baselines, drivers, matio, ops
from mri_super_resolution_amd.scripts.superresDWI import _patient_id, load_input_and_scale


def build_parser():
    p = argparse.ArgumentParser(description="Acquisition-model study: LR slices by k-space truncation, a Gaussian PSF or block means, and back")
    p.add_argument("--data", nargs="+", required=True, help=".mat file(s): master.mat (hybrid_raw) or a plain volume")
    p.add_argument("--key", default=None, help="variable holding the volume (default: hybrid_raw, else the only array)")
    p.add_argument("--pt_id", nargs="*", default=None, help="patient ids for the CSV (default: digits of the file name)")
    p.add_argument("--output_address", default="AM_results", help="output directory (one sub-directory per patient)")
    p.add_argument("--model", choices=drivers.ACQUISITION_MODELS, required=True, help="how the LR slices are made")
    p.add_argument("--factor", type=int, default=None, help="HR pixels per LR pixel and axis, 1 .. 8 (default 2)")
    p.add_argument("--lr_side", type=int, default=None, help="instead of --factor: the LR side in pixels; it need not divide the ROI")
    p.add_argument("--fwhm", type=float, default=None, help="--model gaussian: full width at half maximum in LR pixels (default 1.2)")
    p.add_argument("--noise", type=float, default=0.02, help="sigma of the noise added to every LR slice (data in [0, 1])")
    p.add_argument("--seed", type=int, default=0, help="seeds the noise")
    p.add_argument("--tv_lambda", type=float, default=baselines.TVOP_DEFAULT_LAMBDA,
                   help="weight of the prior of both TV rows (data in [0, 1] at noise 0.02: the sweep of DESIGN.md 4p)")
    p.add_argument("--tv_huber", type=float, default=baselines.TVOP_DEFAULT_HUBER,
                   help="Huber threshold on the gradient magnitude; 0 = plain isotropic TV")
    p.add_argument("--tv_iters", type=int, default=baselines.TVOP_DEFAULT_ITERS, help="Chambolle-Pock iterations, 1 .. 100,000")
    p.add_argument("--roi_start", type=int, default=40)
    p.add_argument("--roi_end", type=int, default=90)
    p.add_argument("--slices", type=int, nargs="*", default=None, help="slice indexes (default: every slice)")
    p.add_argument("--b_index", type=int, default=0, help="which b-value of the volume is studied")
    p.add_argument("--with_degibbs", action="store_true",
                   help="add the rows degibbs_zerofill and degibbs_spline: unring the LR slice (denoise.degibbs), then re-sample")
    return p


def check_args(args):
    """Every refusal of the flags, before the input is loaded and anything touches the device; returns the LR side."""
    if args.roi_start < 0 or args.roi_end <= args.roi_start:
        raise ValueError(f"ROI {args.roi_start}:{args.roi_end}: 0 <= roi_start < roi_end")
    m = drivers.check_acquisition_model(args.model, args.roi_end - args.roi_start, args.factor, args.lr_side, args.fwhm, args.noise,
                                        args.tv_lambda, args.tv_huber, args.tv_iters)
    if args.slices is not None and (not args.slices or min(args.slices) < 0):
        raise ValueError(f"--slices are indexes >= 0 (got {args.slices})")
    if args.b_index < 0:
        raise ValueError(f"--b_index must be >= 0 (got {args.b_index})")
    if getattr(args, "with_degibbs", False):
        ops.degibbs_params("--with_degibbs", (m, m), ops.DEGIBBS_DEFAULT_SHIFTS, ops.DEGIBBS_DEFAULT_WINDOW)
    return m


def run_patient(path, pt_id, args):
    m = check_args(args)
    mean_img, _, bvalues, _, _ = load_input_and_scale(path, args.key)
    r0, r1 = args.roi_start, args.roi_end
    if r1 > min(mean_img.shape[:2]):
        raise ValueError(f"ROI {r0}:{r1} does not fit the {mean_img.shape[:2]} slices")
    if args.b_index >= mean_img.shape[3]:
        raise ValueError(f"--b_index {args.b_index}: the volume has {mean_img.shape[3]} b-values")
    which = list(range(mean_img.shape[2])) if args.slices is None else list(args.slices)
    if max(which) >= mean_img.shape[2]:
        raise ValueError(f"--slices {which}: the volume has {mean_img.shape[2]} slices")
    out_dir = os.path.join(args.output_address, f"pat{pt_id}")
    os.makedirs(out_dir, exist_ok=True)
    slices = np.ascontiguousarray(mean_img[r0:r1, r0:r1, :, args.b_index].transpose(2, 0, 1))[which]
    # slice z of the volume draws from seed * 1000 + z whatever --slices selects
    res = drivers.acquisition_model_study(slices, args.model, args.factor, args.lr_side, args.fwhm, args.noise, args.seed, args.tv_lambda,
                                          args.tv_huber, args.tv_iters, slice_ids=which,
                                          with_degibbs=getattr(args, "with_degibbs", False))
    methods = res["methods"]
    b_value = float(bvalues[args.b_index]) if args.b_index < len(bvalues) else float(args.b_index)
    with open(os.path.join(out_dir, "acquisition_model.csv"), "w") as fh:
        fh.write(", ".join(["Pt_id", "b-value", "slice"] + [f"SSIM-{name}" for name in methods]) + "\n")
        for i, z in enumerate(which):
            fh.write(f"{pt_id}, {b_value}, {z}, " + ", ".join(str(float(res["ssim"][name][i])) for name in methods) + "\n")
    summary = {"pt_id": str(pt_id), "input": os.path.abspath(path), "roi": [r0, r1], "slices": which, "b_index": int(args.b_index),
               "b_value": b_value, "model": args.model, "factor": args.factor, "lr_side": int(m), "fwhm": args.fwhm, "noise": args.noise,
               "seed": int(args.seed), "tv_lambda": args.tv_lambda, "tv_huber": args.tv_huber, "tv_iters": int(args.tv_iters),
               "methods": list(methods)}
    for name in methods:
        summary[f"psnr_{name}_db"] = float(res["psnr"][name].mean())
        summary[f"ssim_{name}_mean"] = float(res["ssim"][name].mean())
    summary["tv_operator_consistency_psnr_db"] = float(res["consistency"].mean())
    summary["tv_operator_energy_mean"] = float(res["info"]["tv_operator"]["energy"].mean())
    host = lambda t: t.cpu().numpy()
    mat = {name: host(res["images"][name]).transpose(1, 2, 0) for name in methods}                                    # [X, Y, Z]
    mat.update(hr=host(res["hr"]).transpose(1, 2, 0), lr=host(res["lr"]).transpose(1, 2, 0), R0=host(res["operators"][0]),
               R1=host(res["operators"][1]), slices=np.asarray(which, np.float64))
    matio.savemat(os.path.join(out_dir, "acquisition_model.mat"), mat)
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
