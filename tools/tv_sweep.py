"""CPU: the sweep behind the defaults of baselines.tv_superres / superresDWI --tv_baseline:
    python tools/tv_sweep.py
The float64 restatement (tests/tvsr_common.py) on tests/golden/pat07_volume.npz, ROI 40:90 divided by its maximum, all 28 slices, 2 x 2
block means and every second pixel, block replication start: PSNR against the HR ROI per (lambda, alpha, iterations).  The SR column
of the driver is never looked at."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import tvsr_common as T  # noqa: E402

GRID = [(lam, alpha) for lam in (1e-4, 3e-4, 1e-3, 3e-3, 1e-2) for alpha in (0.0, 0.03, 0.1, 0.3)] + \
       [(lam, alpha) for lam in (3e-3, 1e-2, 3e-2) for alpha in (1.0, 3.0)]         # the extension: past the edge of the first grid
ITERS = (100, 300, 1000)

vol = T.pat07_roi()
for kernel in ("mean", "decimate"):
    y = T.apply_A(vol, T.block_kernel(kernel, (2, 2)))
    print(f"{kernel}: block replication {T.psnr(vol, T.replicate(y, (2, 2))):.3f} dB", flush=True)
    for lam, alpha in GRID:
        scores = " ".join(f"{T.psnr(vol, T.solve(y, (2, 2), kernel, lam, alpha, n)):.3f}" for n in ITERS)
        print(f"{kernel} lambda {lam:g} alpha {alpha:g} iterations {'/'.join(map(str, ITERS))}: {scores}", flush=True)
