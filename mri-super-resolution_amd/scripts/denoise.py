#!/usr/bin/env python3
"""MP-PCA denoising of the raw acquisition stack of a ``master.mat``: the step between the scanner's file and every fit.

    python -m mri_super_resolution_amd.scripts.denoise --data master.mat --out clean.mat [--window 5 5 5] [--estimator exp2]
                                                       [--key hybrid_raw] [--degibbs [--degibbs_shifts N]]
                                                       [--method mppca|nlm [--nlm_beta B --nlm_search S --nlm_patch P --nlm_rician]]

The reference's later driver (inrDWI.py:44) reads ``hybrid_raw_clean``, the ``hybrid_raw`` cell after a denoising step made outside its
tree.  This script makes it: every acquisition of every [b][TE] cell of ``--key`` is one measurement of ONE stack
(``denoise.stack_hybrid``), ``denoise.mppca`` (``inr_mppca_denoise``) denoises it over a window of ``--window`` voxels
along (X, Y, Z), and the result goes back into the cell's layout.  ``--out`` holds ``<key>_clean`` in that layout, ``sigma`` (the noise
map [X, Y, Z], in the file's units), ``rank`` (signal components per voxel, int32) and every other variable of the input file as it was;
it is what ``superresDWI --key hybrid_raw_clean`` accepts.  A plain volume [X, Y, Z, B] under ``--key`` is denoised along its last axis.
A window side larger than its axis is refused, not shrunk.  ``--degibbs`` unrings the (X, Y) planes of every measurement after MP-PCA
(``denoise.degibbs``, Gibbs-ringing removal by local sub-voxel shifts with ``--degibbs_shifts`` shifts per side, DESIGN.md 4v -- the
order of ``dwidenoise`` and ``mrdegibbs``; the data must lie on the acquired grid) and writes that as ``<key>_clean``; the summary gains
``degibbs`` and ``degibbs_mean_abs_shift``.  Without the flag every output is what it was.  ``--method nlm`` keeps MP-PCA for its noise
map and discards its projection: the raw stack is filtered by ``denoise.nlm(stack, sigma, guide="mean")`` (non-local means, DESIGN.md 4w;
``--nlm_beta --nlm_search --nlm_patch --nlm_rician``) in groups of at most 16 measurements in the stack's order, and that is written as
``<key>_clean``; ``sigma`` and ``rank`` are written as before, the summary gains ``method`` and the ``nlm_*`` settings.  The default,
``--method mppca``, changes nothing."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))
from mri_super_resolution_amd import denoise, matio, ops  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="MP-PCA denoising of the acquisition stack of a master.mat")
    p.add_argument("--data", required=True, help="the input .mat (MAT-5)")
    p.add_argument("--out", required=True, help="the .mat to write")
    p.add_argument("--key", default="hybrid_raw", help="the [b][TE] cell (or plain [X, Y, Z, B] volume) to denoise")
    p.add_argument("--window", type=int, nargs=3, default=list(denoise.DEFAULT_WINDOW), metavar=("A", "B", "C"),
                   help="odd window sides over (X, Y, Z), each at most its axis")
    p.add_argument("--estimator", choices=denoise.ESTIMATORS, default="exp2", help="the cutoff estimator")
    p.add_argument("--method", choices=("mppca", "nlm"), default="mppca",
                   help="what denoises the stack: the MP-PCA projection, or non-local means under MP-PCA's noise map")
    p.add_argument("--nlm_beta", type=float, default=1.0, help="--method nlm: the strength is 2 beta sigma^2")
    p.add_argument("--nlm_search", type=int, default=3, help="--method nlm: search radius, 0 .. 5")
    p.add_argument("--nlm_patch", type=int, default=1, help="--method nlm: patch radius, 0 .. 2")
    p.add_argument("--nlm_rician", action="store_true", help="--method nlm: Rician bias correction (magnitude data)")
    p.add_argument("--degibbs", action="store_true", help="unring the (X, Y) planes of every measurement after MP-PCA")
    p.add_argument("--degibbs_shifts", type=int, default=denoise.DEGIBBS_DEFAULT_SHIFTS, help="--degibbs: sub-pixel shifts per side, 1 .. 64")
    return p


def check_args(args):
    """Every refusal of the NLM flags, before the input is loaded and anything touches the device."""
    if args.method == "nlm":
        ops.nlm_radii("denoise", args.nlm_search, args.nlm_patch)
        if not 0.0 < args.nlm_beta < float("inf"):
            raise ValueError(f"denoise: --nlm_beta must be finite and > 0 (got {args.nlm_beta!r})")


def nlm_stack(stack, sigma, args):
    """``denoise.nlm_stack`` of the raw stack [M, X, Y, Z] with the flags' settings."""
    return denoise.nlm_stack(stack, sigma, args.nlm_beta, args.nlm_search, args.nlm_patch, args.nlm_rician)


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    data = matio.loadmat(args.data)
    if args.key not in data:
        raise KeyError(f"{args.data}: no variable '{args.key}' (it holds {[k for k in data if not k.startswith('__')]})")
    raw = data[args.key]
    if isinstance(raw, np.ndarray) and raw.dtype == object:
        cell = np.empty(raw.shape, dtype=object)
        for idx in np.ndindex(raw.shape):
            cell[idx] = np.asarray(raw[idx], np.float64)
        stack = denoise.stack_hybrid(cell)
        clean, info = denoise.mppca(stack, args.window, estimator=args.estimator, return_info=True)
        if args.method == "nlm":                                         # MP-PCA's projection is discarded, its noise map kept
            clean = nlm_stack(stack, info["sigma"], args)
        if args.degibbs:                                                 # [M, X, Y, Z]: the (X, Y) planes
            clean, gibbs = denoise.degibbs(clean, (1, 2), args.degibbs_shifts, return_info=True)
        clean = denoise.unstack_hybrid(clean, cell)
        M = stack.shape[0]
    else:
        vol = np.asarray(raw, np.float64)
        if vol.ndim != 4:
            raise ValueError(f"{args.data}: '{args.key}' must be a [b][TE] cell or a volume [X, Y, Z, B] (got shape {vol.shape})")
        clean, info = denoise.mppca(vol, args.window, estimator=args.estimator, return_info=True, measurement_axis=-1)
        if args.method == "nlm":
            clean = np.ascontiguousarray(np.moveaxis(nlm_stack(np.ascontiguousarray(np.moveaxis(vol, -1, 0)), info["sigma"], args), 0, -1))
        if args.degibbs:                                                 # [X, Y, Z, M]
            clean, gibbs = denoise.degibbs(clean, (0, 1), args.degibbs_shifts, return_info=True)
        M = vol.shape[-1]
    out = {k: v for k, v in data.items() if not k.startswith("__")}
    out[f"{args.key}_clean"] = clean
    out["sigma"] = info["sigma"]
    out["rank"] = info["rank"]
    matio.savemat(args.out, out)
    summary = {"input": os.path.abspath(args.data), "output": os.path.abspath(args.out), "key": args.key, "measurements": int(M),
               "window": [int(w) for w in args.window], "estimator": args.estimator, "sigma_median": float(np.median(info["sigma"])),
               "rank_histogram": np.bincount(info["rank"].reshape(-1).clip(min=0)).tolist(),
               "unconverged": int((info["rank"] == -2).sum())}
    if args.method == "nlm":
        summary.update({"method": "nlm", "nlm_beta": args.nlm_beta, "nlm_search": int(args.nlm_search), "nlm_patch": int(args.nlm_patch),
                        "nlm_rician": bool(args.nlm_rician)})
    if args.degibbs:
        summary.update({"degibbs": True, "degibbs_mean_abs_shift": float(np.abs(gibbs["shift"]).mean())})
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
