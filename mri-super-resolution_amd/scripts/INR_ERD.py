#!/usr/bin/env python3
"""``INR_ERD.py`` of the reference (implicit-neural-representations/INR_ERD.py:162-324) on the MI355X path: for every seed and
case the soft-ERD mean image of the cancer slice is computed, a ReLU-headed SIREN (2 -> 128 x 3 -> 1) is pre-trained on it
until the loss falls below 2e-5 (the stop test runs on the device), one fine-tuning step with two learning rates fits the
soft-ERD-weighted acquisitions through the coordinate perturbation, and the SNR / CNR figures of the mean DWI, the mean
reconstruction and their ADC maps go to ``experiments.csv`` (``seed,SNR_c,SNR_b,S_c,S_b,CR,pt,img,pre_post``, four rows per
(seed, case), appended as the reference does).

What the reference hard-codes is a flag here, and the first two are required: ``--data_dir``
(``<data_dir>/<patient number>/no_aver/bigImage.mat`` with ``b0, b1, b2, b3``), ``--cases`` (a JSON list of
``{pt_id, erc, cancer_loc, contralateral_loc, noise, cancer_slice}``: the patient table is the user's to supply), ``--scale`` (grid of the mean reconstruction, 1 = the reference), ``--seeds`` (10),
``--out`` and ``--max_steps`` (a guard on the pre-training loop, which the reference lacks).  Model files are not written.

Two differences from the reference's loop as written.  Its model is built with ``perturb=False`` and never switched on, so its
fine-tuning step and mean reconstruction run without the coordinate perturbation; here the model is built with
``perturb=True`` (prepare_qual_images.py's behaviour), which is what the two-learning-rate step is for.  And a pre-training step
that both converges and collapses ends the reference's loop with a freshly initialised network; here the collapse wins and the
loop goes on.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from csv import writer

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))
from mri_super_resolution_amd import drivers, matio  # noqa: E402

HEADER_CSV = ["seed", "SNR_c", "SNR_b", "S_c", "S_b", "CR", "pt", "img", "pre_post"]      # INR_ERD.py:164
CASE_KEYS = ("pt_id", "erc", "cancer_loc", "contralateral_loc", "noise", "cancer_slice")

class case:
    """INR_ERD.py:69-95: one patient; ``b`` follows ``erc``; ``b0 .. b3`` come from ``bigImage.mat``."""

    def __init__(self, pt_id, erc, cancer_loc, contralateral_loc, noise, cancer_slice, data_dir):
        self.pt_id, self.cancer_loc, self.contralateral_loc = pt_id, tuple(cancer_loc), tuple(contralateral_loc)
        self.noise, self.cancer_slice = tuple(noise), int(cancer_slice)
        self.b = (0, 150, 1000, 1500) if erc else (0, 300, 600, 900)
        mat = matio.loadmat(os.path.join(data_dir, pt_id.split("-")[-1], "no_aver", "bigImage.mat"))
        self.b0, self.b1, self.b2, self.b3 = (mat[k] for k in ("b0", "b1", "b2", "b3"))


def build_parser():
    parser = argparse.ArgumentParser(description="soft-ERD INR (INR_ERD.py) on the MI355X kernels")
    parser.add_argument("--data_dir", required=True, help="root of <pt_no>/no_aver/bigImage.mat")
    parser.add_argument("--cases", default=None, help="required: "
                        "JSON list of {pt_id, erc, cancer_loc, contralateral_loc, noise, cancer_slice}")
    parser.add_argument("--scale", type=int, default=1, help="grid factor of the mean reconstruction (1 = the reference)")
    parser.add_argument("--seeds", type=int, default=10, help="number of seeds (INR_ERD.py:170)")
    parser.add_argument("--out", default="experiments.csv", help="CSV file, appended to")
    parser.add_argument("--max_steps", type=int, default=None, help="guard on the pre-training loop (default 200,000)")
    return parser


def load_case_specs(path):
    if path is None:
        raise SystemExit("no cases: pass --cases cases.json (a list of {" + ", ".join(CASE_KEYS) + "})")
    with open(path) as f:
        specs = json.load(f)
    for s in specs:
        missing = [k for k in CASE_KEYS if k not in s]
        if missing:
            raise ValueError(f"--cases: entry {s.get('pt_id', '?')} lacks {missing}")
    return specs


def write_header(filename):
    with open(filename, "a", newline="") as f:
        writer(f).writerow(HEADER_CSV)


def run(args, cases):
    write_header(args.out)
    summary = []
    for seed in range(args.seeds):
        for _case in cases:
            print(_case.pt_id)
            torch.manual_seed(seed)        # the reference leaves the RNG unseeded: its `seed` only labels the repetition
            rows, info = drivers.erd_inr_case(_case, seed, scale=args.scale, max_steps=args.max_steps)
            with open(args.out, "a", newline="") as f:
                w = writer(f)
                for row in rows:
                    w.writerow(row)
            summary.append({"seed": seed, "pt": _case.pt_id, **info["pretrain"], "finetune_loss": info["finetune_loss"]})
            print(summary[-1])
    return summary


def main(argv=None):
    args = build_parser().parse_args(argv)
    cases = [case(data_dir=args.data_dir, **{k: s[k] for k in CASE_KEYS}) for s in load_case_specs(args.cases)]
    return run(args, cases)


if __name__ == "__main__":
    main()
