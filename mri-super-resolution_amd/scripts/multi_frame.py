"""The multi-frame study: what do several sub-pixel-shifted acquisitions of a slice hold that one does not?

The multi-image methods of the reference (RAMS on 9 acquisitions, the PerturbNet phase, the 8 acquisitions per direction of
master.py) rest on the assumption that several acquisitions of one slice, each displaced by a fraction of a pixel, together hold
more resolution than any one of them.  This driver measures how much a classical reconstruction gets out of that, with a ground
truth: it loads and normalises a volume as ``superresDWI`` does, crops the in-plane ROI (first b-value), and makes of every slice
``--frames`` acquisitions -- the ``--factor`` x ``--factor`` block operator (``--kernel mean|decimate``) of the slice displaced by a
shift drawn uniformly in +- ``--max_shift`` HR pixels (frame 0 at rest), plus Gaussian noise of ``--noise`` (``--seed``; slice z
draws from ``default_rng(seed * 1000 + z)``) -- and reconstructs the slice on the device by

  replicate   block replication of frame 0;
  tv          ``baselines.tv_superres`` of frame 0 alone, with its defaults;
  ignored     all frames with their shifts taken as zero (the TV reconstruction of their mean: register-to-whole-pixels-and-average);
  estimated   all frames with the shifts ``baselines.estimate_shifts`` finds at ``--upsample`` (``--true_shifts``: the true ones);
  true        all frames with the shifts they were made with,

the last three by ``baselines.tv_superres_multi`` (``--tv_lambda --tv_huber --tv_iters``).  Per patient, under
``<output_address>/pat<id>/``: ``multi_frame.csv`` (one row per slice: ``Pt_id, slice``, ``PSNR-<row>`` inside a margin of 4 pixels and
``SSIM-<row>`` for the five rows, ``shift-error``: max |estimate - truth| in HR pixels), ``metrics.json`` (``psnr_<row>_db`` and
``ssim_<row>_mean`` over the slices, ``shift_error_mean`` / ``shift_error_max``) and ``multi_frame.mat`` (``hr``, the five
reconstructions [X, Y, Z], ``frames`` [x, y, K, Z], ``shifts`` and ``estimate`` [Z, K, 2]).  Every flag is checked before the input
is loaded."""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from mri_super_resolution_amd import baselines, drivers, matio
from mri_super_resolution_amd.scripts.superresDWI import _patient_id, load_input_and_scale


def build_parser():
    p = argparse.ArgumentParser(description="Multi-frame super-resolution study: shifted, block-averaged, noisy frames, and back")
    p.add_argument("--data", nargs="+", required=True, help=".mat file(s): master.mat (hybrid_raw) or a plain volume")
    p.add_argument("--key", default=None, help="variable holding the volume (default: hybrid_raw, else the only array)")
    p.add_argument("--pt_id", nargs="*", default=None, help="patient ids for the CSV (default: digits of the file name)")
    p.add_argument("--output_address", default="MF_results", help="output directory (one sub-directory per patient)")
    p.add_argument("--roi_start", type=int, default=30)
    p.add_argument("--roi_end", type=int, default=102)
    p.add_argument("--slices", type=int, nargs="*", default=None, help="slice indexes (default: every slice)")
    p.add_argument("--factor", type=int, default=2, help="HR pixels per LR pixel and axis, 1 .. 8")
    p.add_argument("--frames", type=int, default=8, help="acquisitions per slice, 1 .. 64")
    p.add_argument("--max_shift", type=float, default=1.5, help="the shifts are uniform in +- this many HR pixels")
    p.add_argument("--noise", type=float, default=0.02, help="sigma of the noise added to every frame (data in [0, 1])")
    p.add_argument("--seed", type=int, default=0, help="seeds the shifts and the noise")
    p.add_argument("--kernel", choices=("mean", "decimate"), default="mean", help="the block operator of a LR pixel")
    p.add_argument("--tv_lambda", type=float, default=baselines.TVMF_DEFAULT_LAMBDA,
                   help="weight of the prior (not divided by --frames; default from the sweep of DESIGN.md 4n)")
    p.add_argument("--tv_huber", type=float, default=baselines.TVMF_DEFAULT_HUBER,
                   help="Huber threshold on the gradient magnitude; 0 = plain isotropic TV")
    p.add_argument("--tv_iters", type=int, default=baselines.TVMF_DEFAULT_ITERS, help="Chambolle-Pock iterations, 1 .. 100,000")
    p.add_argument("--upsample", type=int, default=4, help="shift estimate: Fourier up-sampling of the frames; the step is factor / this")
    p.add_argument("--true_shifts", action="store_true", help="skip the estimate: the 'estimated' row uses the true shifts")
    return p


def check_args(args):
    """Every refusal of the flags, before the input is loaded and anything touches the device."""
    drivers.check_multi_frame(args.factor, args.frames, args.max_shift, args.noise, args.kernel, args.tv_lambda, args.tv_huber,
                              args.tv_iters, args.upsample)
    side = args.roi_end - args.roi_start
    if args.roi_start < 0 or side - 2 * drivers.MULTI_FRAME_MARGIN < 7 or side % args.factor:
        raise ValueError(f"ROI {args.roi_start}:{args.roi_end}: a side of whole {args.factor}-blocks with >= 7 pixels inside the margin "
                         f"of {drivers.MULTI_FRAME_MARGIN}")
    if args.slices is not None and (not args.slices or min(args.slices) < 0):
        raise ValueError(f"--slices are indexes >= 0 (got {args.slices})")


def run_patient(path, pt_id, args):
    check_args(args)
    mean_img = load_input_and_scale(path, args.key)[0]
    r0, r1 = args.roi_start, args.roi_end
    if r1 > min(mean_img.shape[:2]):
        raise ValueError(f"ROI {r0}:{r1} does not fit the {mean_img.shape[:2]} slices")
    which = list(range(mean_img.shape[2])) if args.slices is None else list(args.slices)
    if max(which) >= mean_img.shape[2]:
        raise ValueError(f"--slices {which}: the volume has {mean_img.shape[2]} slices")
    out_dir = os.path.join(args.output_address, f"pat{pt_id}")
    os.makedirs(out_dir, exist_ok=True)
    slices = np.ascontiguousarray(mean_img[r0:r1, r0:r1, :, 0].transpose(2, 0, 1))[which]
    # slice z of the volume draws from seed * 1000 + z whatever --slices selects
    res = drivers.multi_frame_study(slices, args.factor, args.frames, args.max_shift, args.noise, args.seed, args.kernel, args.tv_lambda,
                                    args.tv_huber, args.tv_iters, args.upsample, args.true_shifts, slice_ids=which)
    methods = drivers.MULTI_FRAME_METHODS
    with open(os.path.join(out_dir, "multi_frame.csv"), "w") as fh:
        fh.write(", ".join(["Pt_id", "slice"] + [f"PSNR-{m}" for m in methods] + [f"SSIM-{m}" for m in methods] + ["shift-error"]) + "\n")
        for i, z in enumerate(which):
            scores = [float(res["psnr"][m][i]) for m in methods] + [float(res["ssim"][m][i]) for m in methods] + \
                [float(res["shift_error"][i])]
            fh.write(f"{pt_id}, {z}, " + ", ".join(str(v) for v in scores) + "\n")
    summary = {"pt_id": str(pt_id), "input": os.path.abspath(path), "roi": [r0, r1], "slices": which, "factor": int(args.factor),
               "frames": int(args.frames), "max_shift": args.max_shift, "noise": args.noise, "seed": int(args.seed), "kernel": args.kernel,
               "tv_lambda": args.tv_lambda, "tv_huber": args.tv_huber, "tv_iters": int(args.tv_iters), "upsample": int(args.upsample),
               "true_shifts": bool(args.true_shifts)}
    for m in methods:
        summary[f"psnr_{m}_db"] = float(res["psnr"][m].mean())
        summary[f"ssim_{m}_mean"] = float(res["ssim"][m].mean())
    summary["shift_error_mean"], summary["shift_error_max"] = float(res["shift_error"].mean()), float(res["shift_error"].max())
    summary["valid_fraction_mean"] = float(res["info"]["estimated"]["valid_fraction"].mean())
    host = lambda t: t.cpu().numpy()
    mat = {m: host(res["images"][m]).transpose(1, 2, 0) for m in methods}                                        # [X, Y, Z]
    mat.update(hr=host(res["hr"]).transpose(1, 2, 0), frames=host(res["frames"]).transpose(2, 3, 1, 0), shifts=host(res["shifts"]),
               estimate=host(res["estimate"]), slices=np.asarray(which, np.float64))
    matio.savemat(os.path.join(out_dir, "multi_frame.mat"), mat)
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
