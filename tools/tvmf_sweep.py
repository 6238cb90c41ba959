"""CPU: the sweep behind the defaults of baselines.tv_superres_multi / scripts/multi_frame:
    python tools/tvmf_sweep.py
The float64 restatement (tests/tvmf_common.py) on tests/golden/pat07_volume.npz, ROI 30:102 divided by its maximum, slices 10 / 14 /
18: 8 frames of 2 x 2 block means, shifts uniform in +- 1.5 HR pixels, noise 0.02, the draws of the study at its seed; 300 iterations
with the TRUE shifts from the block replication of frame 0; PSNR inside a margin of 4 pixels per (lambda, alpha), then the iteration
count at the best pair.  The method of tools/tv_sweep.py: a coarse grid, then past its edge where the best sits on it.  No other
column -- not the single-frame TV, not an INR -- is ever looked at."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import tvmf_common as M  # noqa: E402

GRID = [(lam, alpha) for lam in (0.005, 0.01, 0.02, 0.04, 0.08) for alpha in (0.0, 0.03, 0.1, 0.3)]
ITERS = (100, 300, 1000)

vol = M.pat07_roi(*M.STUDY_ROI)
cases = [(vol[z],) + M.study_frames(vol[z], M.STUDY_SEED * 1000 + z) for z in M.STUDY_SLICES]


def score(lam, alpha, n_iter):
    return [M.margin_psnr(hr, M.solve(frames, M.STUDY_FACTORS, shifts, "mean", lam, alpha, n_iter)) for hr, shifts, frames in cases]


best = None
for lam, alpha in GRID:
    s = score(lam, alpha, 300)
    print(f"lambda {lam:g} alpha {alpha:g}: " + " ".join(f"{v:.3f}" for v in s) + f"  mean {np.mean(s):.3f}", flush=True)
    if best is None or np.mean(s) > best[0]:
        best = (float(np.mean(s)), lam, alpha)
print(f"best of the grid: lambda {best[1]:g} alpha {best[2]:g}, mean {best[0]:.3f} dB", flush=True)
for n in ITERS:
    s = score(best[1], best[2], n)
    print(f"lambda {best[1]:g} alpha {best[2]:g} iterations {n}: " + " ".join(f"{v:.3f}" for v in s) + f"  mean {np.mean(s):.3f}", flush=True)
