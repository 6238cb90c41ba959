"""CPU: the sweep behind the defaults of baselines.tv_superres_joint / scripts/joint_bvalues:
    python tools/tvj_sweep.py
The float64 restatement (tests/tvj_common.py) on the study case: tests/golden/pat07_volume.npz, ROI 40:90 divided by its maximum, slices
10 / 14 / 18, a synthetic mono-exponential decay over b = 0 / 150 / 1000 / 1500, 2 x 2 block means, noise 0.02 drawn from
default_rng(seed), seeds 0 .. 2; 300 iterations, equal channel weights, lambda over {3, 6, 12, 24, 48}e-3 and Huber over {0.01, 0.03,
0.1}, for the coupled prior and for the per-channel one.  The criterion is the RMSE of the log-linear ADC against the HR data's inside
b0 > 0.25 max, mean over the seeds; beside it the PSNR of the b = 0 and b = 1500 images and of all channels.  The coupled defaults are
the best pair of the coupled grid; the per-channel grid is printed to say what the coupling is worth at each solver's own best pair and
what the coupled defaults cost on b = 0.  No other column is looked at."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import tvj_common as J  # noqa: E402
from tests import tvsr_common as T  # noqa: E402

LAMBDAS = (3e-3, 6e-3, 12e-3, 24e-3, 48e-3)
HUBERS = (0.01, 0.03, 0.1)
SEEDS = (0, 1, 2)
ITERS = (100, 300, 1000)

cases = [J.study_case(seed) for seed in SEEDS]


def score(coupling, lam, huber, n_iter=J.STUDY_ITERS):
    """-> mean over the seeds of (ADC RMSE, b = 0 PSNR, b = 1500 PSNR, all-channel PSNR)."""
    rows = []
    for hr, y, b in cases:
        x = J.solve_joint(y, (2, 2), "mean", lam, huber, n_iter, coupling=coupling)
        last, every, rmse = J.study_scores(x, hr, b)
        rows.append((rmse, T.psnr(hr[:, 0], x[:, 0]), last, every))
    return np.mean(rows, axis=0)


best = {}
table = {}
for coupling in ("joint", "none"):
    for lam in LAMBDAS:
        for huber in HUBERS:
            s = table[(coupling, lam, huber)] = score(coupling, lam, huber)
            print(f"{coupling} lambda {lam:g} huber {huber:g}: ADC RMSE {s[0]:.4e}  PSNR b0 {s[1]:.3f}  b1500 {s[2]:.3f}  all {s[3]:.3f}", flush=True)
            if coupling not in best or s[0] < best[coupling][0]:
                best[coupling] = (float(s[0]), lam, huber)
    r, lam, huber = best[coupling]
    print(f"{coupling}: best of the grid lambda {lam:g} huber {huber:g}, ADC RMSE {r:.4e}", flush=True)
(_, lj, hj), (_, ln, hn) = best["joint"], best["none"]
sj, sn = table[("joint", lj, hj)], table[("none", ln, hn)]
b0_best = max(table[("joint", lam, huber)][1] for lam in LAMBDAS for huber in HUBERS)
print(f"coupled defaults lambda {lj:g} huber {hj:g}: ADC RMSE {sj[0]:.4e} against the per-channel best {sn[0]:.4e} "
      f"({100 * (sj[0] / sn[0] - 1):+.1f} %); b = 0 PSNR {sj[1]:.3f} dB, {b0_best - sj[1]:.3f} dB below the coupled grid's best b = 0 "
      f"PSNR {b0_best:.3f} and {sn[1] - sj[1]:+.3f} dB against the per-channel pair's {sn[1]:.3f}", flush=True)
for n in ITERS:
    s = score("joint", lj, hj, n)
    print(f"joint lambda {lj:g} huber {hj:g} iterations {n}: ADC RMSE {s[0]:.4e}  PSNR b0 {s[1]:.3f}  b1500 {s[2]:.3f}  all {s[3]:.3f}", flush=True)
rep = np.mean([(J.study_scores(T.replicate(y, (2, 2)), hr, b)[2], T.psnr(hr, T.replicate(y, (2, 2)))) for hr, y, b in cases], axis=0)
print(f"block replication: ADC RMSE {rep[0]:.4e}  PSNR all {rep[1]:.3f}", flush=True)
