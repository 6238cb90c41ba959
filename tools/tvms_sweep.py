"""CPU: the sweep behind the defaults of baselines.tv_superres_stacks / scripts/multi_stack:
    python tools/tvms_sweep.py
The float64 restatement (tests/tvms_common.py) on tests/golden/pat07_volume.npz, ROI 40:90 divided by its maximum, all 28 slices: the
orthogonal three-stack design at thickness 2 (axial, coronal, sagittal; the mean profile), Gaussian noise of 0.02 on every stack
(seed 0), the back-projection start, 300 iterations; PSNR of the joint solve against the thin slices 2 .. 25 per (lambda, alpha).
The method of tools/tv_sweep.py: a grid wide enough that the best pair lies inside it, not on its edge.  The objective is not
divided by the number of stacks, so the pair belongs to THREE stacks at THIS noise.  No other column is ever looked at."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import tvms_common as M  # noqa: E402

LAMBDAS = (1e-3, 3e-3, 6e-3, 1e-2, 2e-2, 3e-2, 6e-2)
ALPHAS = (0.0, 0.01, 0.03, 0.1, 0.3)
NOISE, SEED, ITERS = 0.02, 0, 300

vol = M.pat07_roi(*M.STUDY_ROI)                                        # [28, 50, 50]
stacks = M.design_stacks("orthogonal", vol.shape)
ys = M.study_data(vol, stacks, NOISE, SEED)
print(f"back-projection {M.trim_psnr(vol, M.backproject(ys, stacks, vol.shape)):.3f} dB", flush=True)
best = (-1.0, None)
for lam in LAMBDAS:
    row = []
    for alpha in ALPHAS:
        score = M.trim_psnr(vol, M.solve(ys, stacks, vol.shape, lam, alpha, ITERS))
        best = max(best, (score, (lam, alpha)))
        row.append(f"{score:.3f}")
    print(f"lambda {lam:g} alpha {'/'.join(f'{a:g}' for a in ALPHAS)}: {' '.join(row)}", flush=True)
print(f"best {best[0]:.3f} dB at lambda {best[1][0]:g} alpha {best[1][1]:g}; on the edge of the grid: "
      f"{best[1][0] in (LAMBDAS[0], LAMBDAS[-1]) or best[1][1] == ALPHAS[-1]}")
