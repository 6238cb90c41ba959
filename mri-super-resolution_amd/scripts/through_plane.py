"""The through-plane study: how well are thin slices recovered from thick ones?

A DWI voxel is anisotropic -- the slice is its thick direction --, and ``superresDWI --transverse_length`` writes a through-plane
re-sampling that nothing can score, because it has no ground truth.  This driver makes one: it loads and normalises a volume as
``superresDWI`` does, crops the in-plane ROI, trims Z to a multiple of ``--factor`` F, forms thick slices with a slice profile
(``baselines.block_apply3d(HR, (F, 1, 1), profile)``: the mean of F thin slices, or a Gaussian of ``--fwhm`` thick slices sampled at
the thin slices' centres) and reconstructs the thin slices on the device by

  replicate   every thick slice F times;
  spline      the cubic spline along z that ``--transverse_length`` uses (``baselines.resize_z``);
  zerofill    k-space zero-filling along z (``baselines.fourier_resample``, ``align='center'``, ``boundary='mirror'``, clamped at 0);
  tv3d        ``baselines.tv_superres3d``: the profile in the operator, a 3-D TV / Huber prior (``--tv_lambda --tv_huber --tv_iters``,
              ``--tv_gz`` the weight of the slice direction's differences: in-plane spacing / slice spacing);
  SR          with ``--with_inr``: ``drivers.fit_volume`` as it is on the z-first volume (``upscale_axes=1, lr_model='average'``,
              ``--footprint point|box``) -- for ``--factor 2 --profile mean`` only, the one forward model that fit has.
  nlm         with ``--with_nlm``: ``baselines.nlm_upsample`` (non-local upsampling): non-local-means passes at falling
              strengths, each followed by the mean correction under the profile; ``--nlm_start replicate|spline`` (the spline after
              one mean correction), ``--nlm_iters`` passes per level, ``--nlm_search`` / ``--nlm_patch`` the radii.

Per patient, under ``<output_address>/pat<id>/``: ``through_plane.csv`` (one row per slice and b-value: ``Pt_id, b-value, slice,
SSIM-replicate, SSIM-spline, SSIM-zerofill, SSIM-tv3d[, SSIM-SR]``, SSIM by the reference protocol), ``metrics.json``
(``psnr_<method>_db``, ``ssim_<method>_mean``, ``tv3d_consistency_psnr_db``: ``A tv3d`` against the thick slices) and
``through_plane.mat`` (the volumes, [X, Y, Z, B]).  ``--with_nlm`` adds the column ``SSIM-nlm``, ``psnr_nlm_db``, ``ssim_nlm_mean``,
``nlm_consistency_psnr_db``, the ``nlm_*`` settings and the volume ``nlm``; without it every output is what it was.  Every flag is checked before the input is loaded; a volume that makes fewer than 4
thick slices is refused (the cubic spline needs 4 samples)."""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from mri_super_resolution_amd import baselines, drivers, matio, reports
from mri_super_resolution_amd.scripts.superresDWI import _patient_id, load_input_and_scale


def build_parser():
    p = argparse.ArgumentParser(description="Through-plane super-resolution study: thick slices from thin ones, and back")
    p.add_argument("--data", nargs="+", required=True, help=".mat file(s): master.mat (hybrid_raw) or a plain volume")
    p.add_argument("--key", default=None, help="variable holding the volume (default: hybrid_raw, else the only array)")
    p.add_argument("--pt_id", nargs="*", default=None, help="patient ids for the CSV (default: digits of the file name)")
    p.add_argument("--output_address", default="TP_results", help="output directory (one sub-directory per patient)")
    p.add_argument("--roi_start", type=int, default=40)
    p.add_argument("--roi_end", type=int, default=90)
    p.add_argument("--factor", type=int, default=2, help="thin slices per thick slice, 2 .. 8")
    p.add_argument("--profile", choices=("mean", "gaussian"), default="mean", help="the slice profile of a thick slice")
    p.add_argument("--fwhm", type=float, default=1.0, help="--profile gaussian: full width at half maximum, in thick slices")
    p.add_argument("--tv_lambda", type=float, default=baselines.TV3D_DEFAULT_LAMBDA,
                   help="tv3d: weight of the prior (data in [0, 1]; default from the sweep of DESIGN.md 4m)")
    p.add_argument("--tv_huber", type=float, default=baselines.TV3D_DEFAULT_HUBER,
                   help="tv3d: Huber threshold on the gradient magnitude; 0 = plain isotropic TV")
    p.add_argument("--tv_iters", type=int, default=baselines.TV3D_DEFAULT_ITERS, help="tv3d: Chambolle-Pock iterations, 1 .. 100,000")
    p.add_argument("--tv_gz", type=float, default=baselines.TV3D_DEFAULT_GRAD_WEIGHTS[0],
                   help="tv3d: weight of the differences along z (in-plane spacing / slice spacing; 0 uncouples the slices)")
    p.add_argument("--with_inr", action="store_true", help="also fit the SIREN of fit_volume along z (--factor 2 --profile mean only)")
    p.add_argument("--footprint", choices=("point", "box"), default="point",
                   help="--with_inr: the forward model of a thick slice in the fit: a point sample at its centre, or the mean of the "
                        "network over its two thin slices")
    p.add_argument("--number_of_epochs", type=int, default=2500, help="--with_inr: steps of the fit")
    p.add_argument("--seed", type=int, default=0, help="--with_inr: seeds the Fourier matrix and the weights")
    p.add_argument("--with_nlm", action="store_true", help="also the non-local upsampling of baselines.nlm_upsample (method nlm)")
    p.add_argument("--nlm_start", choices=drivers.NLM_STARTS, default="replicate",
                   help="--with_nlm: start from the replication, or from the spline after one mean correction")
    p.add_argument("--nlm_iters", type=int, default=baselines.NLM_DEFAULT_ITERS, help="--with_nlm: passes per level")
    p.add_argument("--nlm_search", type=int, default=baselines.NLM_DEFAULT_SEARCH, help="--with_nlm: search radius, 0 .. 5")
    p.add_argument("--nlm_patch", type=int, default=baselines.NLM_DEFAULT_PATCH, help="--with_nlm: patch radius, 0 .. 2")
    return p


def check_args(args):
    """Every refusal of the flags, before the input is loaded and anything touches the device."""
    drivers.check_through_plane(args.factor, args.profile, args.fwhm, args.tv_lambda, args.tv_huber, args.tv_iters, args.tv_gz,
                                args.with_inr, args.footprint, args.number_of_epochs, args.with_nlm, args.nlm_start, args.nlm_iters,
                                args.nlm_search, args.nlm_patch)
    if args.roi_start < 0 or args.roi_end - args.roi_start < 7:
        raise ValueError(f"ROI {args.roi_start}:{args.roi_end}: SSIM needs >= 7 x 7 pixels")


def run_patient(path, pt_id, args):
    check_args(args)
    mean_img, _, bvalues, _, _ = load_input_and_scale(path, args.key)
    r0, r1 = args.roi_start, args.roi_end
    if r1 > min(mean_img.shape[:2]):
        raise ValueError(f"ROI {r0}:{r1} does not fit the {mean_img.shape[:2]} slices")
    out_dir = os.path.join(args.output_address, f"pat{pt_id}")
    os.makedirs(out_dir, exist_ok=True)
    res = drivers.through_plane_study(mean_img[r0:r1, r0:r1], args.factor, args.profile, args.fwhm, args.tv_lambda, args.tv_huber,
                                      args.tv_iters, args.tv_gz, args.with_inr, args.footprint, args.number_of_epochs, args.seed,
                                      args.with_nlm, args.nlm_start, args.nlm_iters, args.nlm_search, args.nlm_patch)
    methods = list(drivers.THROUGH_PLANE_METHODS) + (["sr"] if args.with_inr else []) + (["nlm"] if args.with_nlm else [])
    columns = list(reports.THROUGH_PLANE_COLUMNS) + (["SSIM-SR"] if args.with_inr else []) + (["SSIM-nlm"] if args.with_nlm else [])
    nz, nb = res["ssim"]["tv3d"].shape
    with open(os.path.join(out_dir, "through_plane.csv"), "w") as fh:
        fh.write(", ".join(["Pt_id", "b-value", "slice"] + columns) + "\n")
        for z in range(nz):
            for b in range(nb):
                scores = ", ".join(str(float(res["ssim"][m][z, b])) for m in methods)
                fh.write(f"{pt_id}, {bvalues[b] if b < len(bvalues) else b}, {z}, {scores}\n")
    summary = {"pt_id": str(pt_id), "input": os.path.abspath(path), "hr_shape": list(res["volumes"]["hr"].shape),
               "factor": int(args.factor), "profile": args.profile, "slice_profile": [float(v) for v in res["kernel"][0]],
               "tv_lambda": args.tv_lambda, "tv_huber": args.tv_huber, "tv_iters": int(args.tv_iters), "tv_gz": args.tv_gz}
    for m in methods:
        summary[f"psnr_{m}_db"] = res["psnr"][m]
        summary[f"ssim_{m}_mean"] = float(res["ssim"][m][res["valid"]].mean())
        if m == "tv3d":
            summary["tv3d_consistency_psnr_db"] = res["consistency"]
        if m == "nlm":
            summary["nlm_consistency_psnr_db"] = res["nlm_consistency"]
            summary.update({"nlm_start": args.nlm_start, "nlm_iters": int(args.nlm_iters), "nlm_search": int(args.nlm_search),
                            "nlm_patch": int(args.nlm_patch)})
    summary.update(res["info"])
    to_xyzb = lambda t: t.permute(2, 3, 0, 1).contiguous().cpu().numpy()                       # [Z, B, X, Y] -> [X, Y, Z, B]
    mat = {name: to_xyzb(v) for name, v in res["volumes"].items()}
    mat["b"] = np.asarray(bvalues, np.float64)
    matio.savemat(os.path.join(out_dir, "through_plane.mat"), mat)
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
