#!/usr/bin/env python3
"""``david.py`` of the reference (implicit-neural-representations/david.py) on the MI355X path: per patient, AutoERD on every
pixel of the cancer slice -- or, with ``--slices all``, of every slice ("This will be conducted on all slides later",
david.py:44) -- then per gradient direction the plain mean and the ERD-accepted mean of the acquisitions, the ADC map of both and
of every single acquisition, and the lesion contrast of each image in ``<out_folder>/<experiment_name>.csv``
(``patient,image,direction,acquisition,metric,performance``, david.py:37).  Clustering, means and ADC maps are one launch of
``csrc/erd_volume.hip`` per patient (``drivers.david_study``); the contrast numbers are computed on the host, as the reference
computes them.

Flags: the reference's two (``--out_folder``, ``--experiment_name``) with the same names and defaults, plus ``--data_dir`` and
``--cases`` as in ``scripts/master.py`` (the module-level ``cases`` list the reference imports was never published), ``--erd 1|2``
(the reference hard-codes majority voting, 1), ``--slices cancer|all`` and ``--save_maps`` (``<out_folder>/david_<pt>.mat``: the
maps of all chosen slices).  With ``--slices all`` the table is still the cancer slice's -- the landmarks belong to it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))
from mri_super_resolution_amd import drivers, matio, reports  # noqa: E402
from mri_super_resolution_amd.scripts.master import load_cases  # noqa: E402


def build_parser():
    parser = argparse.ArgumentParser(description='DAVID')
    parser.add_argument('--out_folder', default='../experiments/', help='directory to save the quantitative results')
    parser.add_argument('--experiment_name', default='david', help='name of the experiment')
    parser.add_argument('--data_dir', default='../anon_data', help='directory of patNN_alldata / _mean_b0 / _ERD .mat files')
    parser.add_argument('--cases', default=None, help='JSON file: list of {pt_id, b, cancer_loc, contralateral_loc, noise, '
                                                      'cancer_slice, acquisitions}')
    parser.add_argument('--erd', type=int, default=1, choices=(1, 2), help='AutoERD rule: 1 = majority voting (the reference), '
                                                                           '2 = intensity-cognisant')
    parser.add_argument('--slices', default='cancer', choices=('cancer', 'all'), help='slices to cluster and to form maps of')
    parser.add_argument('--save_maps', action='store_true', help='write the maps of the chosen slices to david_<pt>.mat')
    return parser


def run(args, cases):
    os.makedirs(args.out_folder, exist_ok=True)
    csv = reports.DavidCsv(os.path.join(args.out_folder, args.experiment_name + '.csv'))
    written = []
    for case in cases:
        pt_no = case.pt_id.split('-')[-1]
        print(case.pt_id)
        print('Conducting Auto-ERD with Agglomerative Clustering...')
        study = drivers.david_study(case, rule=args.erd, slices=args.slices)
        csv.rows(pt_no, study["rows"])
        if args.save_maps:
            path = os.path.join(args.out_folder, f'david_{pt_no}.mat')
            maps = {k: v for k, v in study["maps"].items() if v is not None}
            maps["slices"] = np.asarray(study["slices"], np.int64)
            matio.savemat(path, maps)
            written.append(path)
    return {"csv": csv.path, "maps": written}


def main(argv=None):
    args = build_parser().parse_args(argv)
    cases = load_cases(args)
    if not cases:
        raise SystemExit("no cases: pass --cases cases.json (the reference's module-level `cases` list was never published)")
    out = run(args, cases)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
