#!/usr/bin/env python3
"""Writes tests/golden/reader_study_crops.npz: the four uint8 401 x 401 panels that perceptual_similarity.m cuts out of the
reference's figures 291.png and 292.png (implicit-neural-representations/perceptual_similarity_tests/randomized images/), their
label rows, and the scores that tests/perceptual_common.py -- the float64 restatement of the definitions, NOT MATLAB -- gives for
them with the .m file's data ranges (255 on the crops, 1 after the high-pass).

    python tools/make_perceptual_golden.py <perceptual_similarity_tests folder of the reference> [--figures 291 292]

Runs on the host only (PIL, NumPy, SciPy); needs the reference tree, which the tests do not."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mri_super_resolution_amd.scripts import perceptual_similarity as script  # noqa: E402
from tests import perceptual_common as pc  # noqa: E402

MAX_BYTES = 1000000


def collect(folder, figures):
    rows = {r[1]: r for r in script.read_labels(os.path.join(folder, "labels.csv"))[1:]}
    data = {"figures": np.array(figures, dtype=np.int64)}
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None
    for fig in figures:
        row = rows[str(fig)]
        with Image.open(os.path.join(folder, "randomized images", f"{fig}.png")) as im:
            gray = script.rgb2gray_uint8(np.asarray(im))
        panels = script.crop_panels(gray, row[4:8])
        data[f"{fig}/label_row"] = np.array(row)
        for name in script.PANEL_NAMES:
            assert panels[name].shape == (401, 401) and panels[name].dtype == np.uint8
            data[f"{fig}/{name}"] = panels[name]
        scores = pc.reader_study_scores(panels["interpolated"], panels["SR"], panels["base"], 255.0, 1.0)
        for key, val in scores.items():
            data[f"{fig}/score/{key}"] = np.float64(val)
            print(fig, key, repr(val))
    return data


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("folder")
    ap.add_argument("--figures", type=int, nargs="+", default=[291, 292])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "reader_study_crops.npz"))
    args = ap.parse_args(argv)
    figures = list(args.figures)
    while True:
        np.savez_compressed(args.out, **collect(args.folder, figures))
        size = os.path.getsize(args.out)
        print(f"{args.out}: {size} bytes, figures {figures}")
        if size < MAX_BYTES or len(figures) == 1:
            break
        figures = figures[:-1]       # drop the last figure rather than commit a large file
    if size >= MAX_BYTES:
        raise SystemExit(f"{args.out} is {size} bytes even with one figure")


if __name__ == "__main__":
    main()
