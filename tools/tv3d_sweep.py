"""CPU: the sweep behind the defaults of baselines.tv_superres3d / scripts/through_plane:
    python tools/tv3d_sweep.py
The float64 restatement (tests/tvsr3d_common.py) on tests/golden/pat07_volume.npz, ROI 40:90 divided by its maximum, all 28 slices:
thick slices = the mean of 2 thin ones (factor 2, the mean profile), block replication start; PSNR against the 28 thin slices per
(lambda, alpha, weight of the slice direction's differences, iterations), beside slice replication and linear interpolation along z.
The method of tools/tv_sweep.py: a coarse grid, then past its edge where the best sits on it.  No INR column is ever looked at."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import tvsr3d_common as T  # noqa: E402

F = (2, 1, 1)
GRID = [(lam, alpha, gz) for gz in (1.0, 0.5) for lam in (1e-3, 3e-3, 1e-2) for alpha in (0.0, 0.03, 0.1, 0.3)] + \
       [(3e-3, 0.1, gz) for gz in (2.0, 0.25)] + [(3e-3, 0.1, 1e-9)]   # the slice direction's weight past the grid; "z-only" is below
ITERS = (100, 300, 1000)

vol = T.pat07_roi()                                                   # [28, 50, 50]
y = T.apply_A(vol, T.block_table(T.block_factors("mean", F)))          # [14, 50, 50]
print(f"slice replication {T.psnr(vol, T.replicate(y, F)):.3f} dB", flush=True)
centres = (np.arange(28) + 0.5) / 2 - 0.5                             # thin-slice centres on the thick-slice index axis
lo = np.clip(np.floor(centres).astype(int), 0, 12)
t = np.clip(centres - lo, 0.0, 1.0)[:, None, None]
print(f"linear along z {T.psnr(vol, (1 - t) * y[lo] + t * y[lo + 1]):.3f} dB", flush=True)
for lam, alpha, gz in GRID:
    scores = " ".join(f"{T.psnr(vol, T.solve(y, F, 'mean', lam, alpha, n, (gz, 1.0, 1.0))):.3f}" for n in ITERS)
    print(f"lambda {lam:g} alpha {alpha:g} gz {gz:g} iterations {'/'.join(map(str, ITERS))}: {scores}", flush=True)
# the prior along z alone: in-plane weights 1e-9
scores = " ".join(f"{T.psnr(vol, T.solve(y, F, 'mean', 3e-3, 0.1, n, (1.0, 1e-9, 1e-9))):.3f}" for n in ITERS)
print(f"lambda 0.003 alpha 0.1 g (1, 1e-9, 1e-9) iterations {'/'.join(map(str, ITERS))}: {scores}", flush=True)
