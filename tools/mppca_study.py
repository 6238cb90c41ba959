"""GPU box: what MP-PCA denoising does to a known phantom, and how far the kernel is from its float64 restatement:
    python tools/mppca_study.py [--out profiles/mppca_study.txt] [--parity_out profiles/mppca_parity.txt]
Quality: the phantom of tests/mppca_common.py (three spatial components with exponential decay curves, Gaussian noise 0.05) as a
[M, 12, 48, 48] stack, M = 16 and M = 40, seeds 0 .. 2, over the windows (1, 5, 5), (3, 5, 5), (5, 5, 5) and both estimators: the RMSE
against the clean stack over the input's, the median of sigma and the histogram of the rank, on the device.  Parity: the five cases of
the tests, the kernel's largest deviation from the restatement beside d_ref (the restatement against itself with the measurement rows
reversed) for ``out`` and ``sigma``; the tests hold the kernel to 32 d_ref."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOWS = ((1, 5, 5), (3, 5, 5), (5, 5, 5))
SHAPE = (12, 48, 48)
SEEDS = (0, 1, 2)


def quality():
    import numpy as np

    from mri_super_resolution_amd import denoise
    from tests import mppca_common as P

    lines = []
    for M in (16, 40):
        for window in WINDOWS:
            for estimator in ("exp2", "exp1"):
                ratios, medians, hist = [], [], np.zeros(0, np.int64)
                for seed in SEEDS:
                    clean, noisy = P.phantom(M, SHAPE, P.SIGMA, np.random.default_rng(seed))
                    out, info = denoise.mppca(noisy, window, estimator=estimator, return_info=True)
                    assert (info["rank"] >= 0).all()
                    ratios.append(P.rmse(out, clean) / P.rmse(noisy, clean))
                    medians.append(float(np.median(info["sigma"])))
                    h = np.bincount(info["rank"].reshape(-1))
                    hist = h + np.pad(hist, (0, len(h) - len(hist))) if len(h) >= len(hist) else hist + np.pad(h, (0, len(hist) - len(h)))
                share = ", ".join(f"{k}: {100.0 * v / hist.sum():.1f} %" for k, v in enumerate(hist) if v)
                lines.append(f"M = {M} window {window} {estimator}: RMSE out / in {np.mean(ratios):.3f} ({min(ratios):.3f} .. {max(ratios):.3f}), median "
                             f"sigma {np.mean(medians):.4f} (true {P.SIGMA}), rank {{{share}}}")
    return lines


def parity():
    import numpy as np
    import torch

    from mri_super_resolution_amd import ops
    from tests import mppca_common as P

    lines = []
    for index, case in enumerate(P.cases()):
        want = P.reference(index)
        d_out, d_sigma = P.reference_spread(index)
        out, sigma, rank = ops.mppca_denoise(torch.from_numpy(np.array(case["noisy"])).cuda(), case["window"])
        e_out = float(np.abs(out.cpu().numpy() - want[0]).max())
        e_sigma = float(np.abs(sigma.cpu().numpy() - want[1]).max())
        lines.append(f"{P.CASE_IDS[index]}: out: kernel {e_out:.3e}, d_ref {d_out:.3e} ({e_out / d_out:.2f} d_ref); sigma: kernel {e_sigma:.3e}, d_ref "
                     f"{d_sigma:.3e} ({e_sigma / d_sigma:.2f} d_ref); max|x| {np.abs(case['noisy']).max():.2f}; rank differs at "
                     f"{int((rank.cpu().numpy() != want[2]).sum())} of {want[2].size} voxels (smallest margin {want[3].min():.2e})")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mppca_study.txt"))
    ap.add_argument("--parity_out", default=os.path.join(ROOT, "profiles", "mppca_parity.txt"))
    args = ap.parse_args()
    for path, lines in ((args.parity_out, parity()), (args.out, quality())):
        text = "\n".join(lines) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(text)
        print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
