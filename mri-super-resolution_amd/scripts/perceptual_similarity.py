#!/usr/bin/env python3
"""``perceptual_similarity.m`` of the reference (implicit-neural-representations/perceptual_similarity_tests/) on the MI355X path: the
scores of the reader-study panels.  For every slice: SSIM (Gaussian window), MSE and MS-SSIM of ``interpolated`` against ``base`` and
of ``SR`` against ``base``, on the images as they are and after the 3 x 3 high-pass of HPF.m, and the high-frequency gain
(perceptual_similarity.m:41-52); then, per score, both means, both standard deviations and a paired t-test (:65-68).  The scores are
HIP kernels (``perceptual.reader_study_scores``); the t-test is ``scipy.stats.ttest_rel`` on the host.  No figure is drawn.

The scores follow the DEFINITIONS of DESIGN.md 4g (MATLAB's documented defaults); no MATLAB output was ever compared against.
FSIM and SR-SIM (perceptual_similarity.m:53-54) are NOT computed and have no column: FSIM.m and SR_SIM.m are third-party files under a
research-only licence that this project does not restate.

Two sources:

``--qual_dir DIR``   the output of scripts/prepare_qual_images.py: ``labels.csv`` and ``<file>.mat``.  The four panels are taken BY
    NAME from the ``.mat`` file and used as the floats they are.  ``data_range`` and the high-passed ``data_range`` both default to the
    slice's ``base.max()``; ``--data_range`` overrides both.  This DIFFERS from the ``.m`` file, which reads 8-bit screen captures of
    the rendered figure (so its images are quantised, cropped to the centre and scored with L = 255, and L = 1 after the high-pass).
``--png_dir DIR [--labels labels.csv] [--rows 2:66]``   the reference's own route: ``<file>.png`` figures, gray =
    ``round(0.2989 R + 0.5870 G + 0.1140 B)`` as uint8, rows 381:1390, the four panels 1011 columns wide from columns 751, 1964, 4390,
    3177 named by label columns 5..8 BY POSITION, each cropped to 300:700 in both axes (all 1-based, inclusive).  ``data_range`` is 255
    on the crops and 1 on the high-passed images: MATLAB's class rule (uint8 -> 255, single -> 1), kept as it is.

Outputs in ``--out_dir``: ``scores.csv`` (``file, pt, image, index, filter, interpolated, SR``; one ``hf_gain`` row per file with
the gain under ``SR``) and ``summary.csv`` (per index and filter: n, the means, the standard deviations (n - 1), the t-test's p).
"""
from __future__ import annotations

import argparse
import csv
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))

START_COLUMNS = (751, 1964, 4390, 3177)     # perceptual_similarity.m:5, 1-based
PANEL_WIDTH = 1761 - 751 + 1                # :6, :27  x(:, index:index+diff)
FIGURE_ROWS = (381, 1390)                   # :24
CROP = (300, 700)                           # :28
PANEL_NAMES = ("low", "interpolated", "SR", "base")
INDICES, FILTERS = ("ssim", "mse", "ms_ssim"), ("raw", "hpf")
SCORE_COLUMNS = ["file", "pt", "image", "index", "filter", "interpolated", "SR"]
SUMMARY_COLUMNS = ["index", "filter", "n", "mean_interpolated", "mean_SR", "std_interpolated", "std_SR", "p"]
NOT_COMPUTED = ("FSIM and SR-SIM (perceptual_similarity.m:53-54) are not computed: FSIM.m and SR_SIM.m are third-party files under a "
                "research-only licence")


def build_parser():
    parser = argparse.ArgumentParser(description="reader-study scores (perceptual_similarity.m) on the MI355X kernels")
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument("--qual_dir", help="folder written by prepare_qual_images.py: labels.csv and <file>.mat")
    src.add_argument("--png_dir", help="folder of the reference's <file>.png figures")
    parser.add_argument("--labels", default=None, help="labels.csv (default: <dir>/labels.csv)")
    parser.add_argument("--rows", default=None, help="1-based inclusive rows of labels.csv, the header being row 1 "
                        "(default: 2:66 with --png_dir as in the .m file, every row with --qual_dir)")
    parser.add_argument("--data_range", type=float, default=None, help="--qual_dir only: L for the raw and the high-passed scores")
    parser.add_argument("--out_dir", default="perceptual", help="folder of scores.csv and summary.csv")
    parser.add_argument("--parse_only", action="store_true", help="read, crop and report the slices; no device work, no output")
    return parser


def rgb2gray_uint8(rgb: np.ndarray) -> np.ndarray:
    """``round(0.2989 R + 0.5870 G + 0.1140 B)`` as uint8 (halves round up, as MATLAB's ``round`` does for positive values)"""
    rgb = np.asarray(rgb)
    if rgb.ndim == 2:
        return rgb.astype(np.uint8)
    g = 0.2989 * rgb[..., 0].astype(np.float64) + 0.5870 * rgb[..., 1].astype(np.float64) + 0.1140 * rgb[..., 2].astype(np.float64)
    return np.clip(np.floor(g + 0.5), 0, 255).astype(np.uint8)


def read_labels(path: str):
    """every row of the file as a list of strings, the header included"""
    with open(path, newline="") as f:
        return [row for row in csv.reader(f) if row]


def select_rows(rows, spec):
    """``"a:b"``: the 1-based inclusive rows a..b of the file (row 1 is the header), clipped to the file"""
    if spec is None:
        return rows[1:]
    a, b = (int(v) for v in spec.split(":"))
    if a < 2 or b < a:
        raise ValueError(f"--rows {spec}: need 2 <= first <= last (row 1 is the header)")
    return rows[a - 1:b]


def crop_panels(gray: np.ndarray, names):
    """the four 401 x 401 crops of one gray figure; ``names``: label columns 5..8, by position"""
    need_h, need_w = FIGURE_ROWS[1], max(START_COLUMNS) - 1 + PANEL_WIDTH
    if gray.shape[0] < need_h or gray.shape[1] < need_w:
        raise ValueError(f"figure of {gray.shape[0]} x {gray.shape[1]} pixels: at least {need_h} x {need_w} needed")
    x = gray[FIGURE_ROWS[0] - 1:FIGURE_ROWS[1]]
    out = {}
    for start, name in zip(START_COLUMNS, names):
        panel = x[:, start - 1:start - 1 + PANEL_WIDTH]
        key = name if name in ("base", "interpolated", "low") else "SR"        # the .m file's else branch
        out[key] = np.ascontiguousarray(panel[CROP[0] - 1:CROP[1], CROP[0] - 1:CROP[1]])
    return out


def load_png_dir(png_dir, labels=None, rows="2:66"):
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None
    slices = []
    for row in select_rows(read_labels(labels or os.path.join(png_dir, "labels.csv")), rows or "2:66"):
        with Image.open(os.path.join(png_dir, f"{row[1]}.png")) as im:
            gray = rgb2gray_uint8(np.asarray(im.convert("RGB") if im.mode not in ("L", "RGB", "RGBA") else im))
        panels = crop_panels(gray, row[4:8])
        missing = [p for p in ("interpolated", "SR", "base") if p not in panels]
        if missing:
            raise ValueError(f"{row[1]}.png: labels {row[4:8]} name no {missing} panel")
        slices.append({"file": row[1], "pt": row[2], "image": row[3], "panels": panels, "data_range": 255.0, "hpf_data_range": 1.0})
    return slices


def load_qual_dir(qual_dir, labels=None, rows=None, data_range=None):
    from mri_super_resolution_amd import matio
    table = read_labels(labels or os.path.join(qual_dir, "labels.csv"))
    col = {name: i for i, name in enumerate(table[0])}
    for name in ("file", "pt", "image"):
        if name not in col:
            raise ValueError(f"labels.csv has no column {name!r} (header {table[0]})")
    slices = []
    for row in select_rows(table, rows):
        mat = matio.loadmat(os.path.join(qual_dir, f"{row[col['file']]}.mat"))
        panels = {}
        for name in PANEL_NAMES:
            if name not in mat:
                raise ValueError(f"{row[col['file']]}.mat holds no {name!r}")
            panels[name] = np.asarray(mat[name], dtype=np.float64)
        rng = float(data_range) if data_range is not None else float(panels["base"].max())
        if not rng > 0:
            raise ValueError(f"{row[col['file']]}.mat: data_range {rng} (base.max()) is not positive; pass --data_range")
        slices.append({"file": row[col["file"]], "pt": row[col["pt"]], "image": row[col["image"]], "panels": panels,
                       "data_range": rng, "hpf_data_range": rng})
    return slices


def _device_scorer(inter, sr, base, data_range, hpf_data_range):
    from mri_super_resolution_amd import perceptual
    return perceptual.reader_study_scores(inter, sr, base, data_range, hpf_data_range)


def score_slices(slices, scorer=None):
    """``scorer(inter, sr, base, data_range, hpf_data_range)`` -> the dict of ``perceptual.reader_study_scores`` on [n, H, W] float32
    arrays; slices of one shape and one pair of ranges go through it as one batch.  Returns one dict of floats per slice."""
    scorer = scorer or _device_scorer
    groups, out = {}, [None] * len(slices)
    for i, s in enumerate(slices):
        groups.setdefault((s["panels"]["base"].shape, s["data_range"], s["hpf_data_range"]), []).append(i)
    for (_, rng, hrng), members in groups.items():
        stack = lambda name: np.stack([np.asarray(slices[i]["panels"][name], dtype=np.float32) for i in members])     # noqa: E731
        res = scorer(stack("interpolated"), stack("SR"), stack("base"), rng, hrng)
        for k, i in enumerate(members):
            out[i] = {key: float(np.asarray(val).reshape(-1)[k]) for key, val in res.items()}
    return out


def score_rows(slices, scores):
    rows = []
    for s, sc in zip(slices, scores):
        head = [s["file"], s["pt"], s["image"]]
        for index in INDICES:
            for filt in FILTERS:
                rows.append(head + [index, filt, repr(sc[f"{index}_{filt}_interpolated"]), repr(sc[f"{index}_{filt}_SR"])])
        rows.append(head + ["hf_gain", "hpf", "", repr(sc["hf_gain"])])
    return rows


def summary_rows(scores):
    """per (index, filter): n, both means, both standard deviations (n - 1), and the paired t-test's p (perceptual_similarity.m:68)"""
    from scipy import stats
    rows = []
    for index in INDICES:
        for filt in FILTERS:
            a = np.array([sc[f"{index}_{filt}_interpolated"] for sc in scores], dtype=np.float64)
            b = np.array([sc[f"{index}_{filt}_SR"] for sc in scores], dtype=np.float64)
            n = len(a)
            std = lambda v: float(np.std(v, ddof=1)) if n > 1 else float("nan")      # noqa: E731
            with np.errstate(all="ignore"):
                p = float(stats.ttest_rel(a, b).pvalue) if n > 1 else float("nan")
            rows.append([index, filt, n, repr(float(a.mean())), repr(float(b.mean())), repr(std(a)), repr(std(b)), repr(p)])
    return rows


def write_csv(path, header, rows):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(header)
        w.writerows(rows)


def run(args, scorer=None):
    if args.png_dir:
        if args.data_range is not None:
            raise ValueError("--data_range goes with --qual_dir: the PNG route keeps MATLAB's class rule (255 on the crops, 1 after the "
                             "high-pass)")
        slices = load_png_dir(args.png_dir, args.labels, args.rows)
    else:
        slices = load_qual_dir(args.qual_dir, args.labels, args.rows, args.data_range)
    if not slices:
        raise ValueError("no slices selected")
    print(f"{len(slices)} slices: files {slices[0]['file']} .. {slices[-1]['file']}, panels "
          f"{'x'.join(str(v) for v in slices[0]['panels']['base'].shape)} {slices[0]['panels']['base'].dtype}")
    if args.parse_only:
        return slices, None
    scores = score_slices(slices, scorer)
    os.makedirs(args.out_dir, exist_ok=True)
    write_csv(os.path.join(args.out_dir, "scores.csv"), SCORE_COLUMNS, score_rows(slices, scores))
    summary = summary_rows(scores)
    write_csv(os.path.join(args.out_dir, "summary.csv"), SUMMARY_COLUMNS, summary)
    for row in summary:
        print(dict(zip(SUMMARY_COLUMNS, row)))
    print(NOT_COMPUTED)
    return slices, scores


def main(argv=None, scorer=None):
    return run(build_parser().parse_args(argv), scorer)


if __name__ == "__main__":
    main()
