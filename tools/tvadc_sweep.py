"""CPU: the sweep behind the defaults of baselines.tv_superres_adc:
    python tools/tvadc_sweep.py [iterations of the grid, default 3000]
The float64 restatement (tests/tvadc_common.py) on the study case of tools/tvj_sweep.py: tests/golden/pat07_volume.npz, ROI 40:90 divided
by its maximum, slices 10 / 14 / 18, a synthetic mono-exponential decay over b = 0 / 150 / 1000 / 1500, 2 x 2 block means, noise 0.02 drawn
from default_rng(seed), seeds 0 .. 2.  3,000 iterations from the default start, s_max 1.5, adc_max 4e-3, adc0 1e-3, mu_s = 1; lambda over
{2.5, 5, 10, 20}e-3, the weight mu_d of the normalised ADC over {0.05, 0.1, 0.2, 0.5}, Huber over {0.01, 0.03}, both couplings.  The
criterion is the RMSE of the SOLVER'S ADC map against the true map inside b0 > 0.25 max, mean over the seeds, among the points whose
b = 0 PSNR does not fall below the per-channel solver's (tvj_common.solve_joint, coupling "none", 300 iterations) at ITS best ADC pair of
tvj_sweep's grid.  If the best point sits on the edge of the lambda or the weight axis the grid is extended ONCE by a factor of two in
that direction.  Then the iteration count at the chosen point, 1,000 / 3,000 / 10,000: the iteration is slow, and stopping it early
is a regulariser of its own, so the grid is read at the iteration count the defaults carry.  No other column is looked at."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import tvadc_common as A  # noqa: E402
from tests import tvj_common as J  # noqa: E402

LAMBDAS = [2.5e-3, 5e-3, 10e-3, 20e-3]
WEIGHTS = [0.05, 0.1, 0.2, 0.5]
HUBERS = (0.01, 0.03)
SEEDS = (0, 1, 2)
ITERS = (1000, 3000, 10000)
SWEEP_ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 3000

hr, _, adc_true = A.study_truth()
data = np.stack([J.study_case(seed)[1] for seed in SEEDS])          # [seed, 3, 4, 25, 25]: the seeds solved as one batch


def score(coupling, lam, weight, huber, n_iter=SWEEP_ITERS):
    """-> mean over the seeds of (ADC RMSE of the solver's map, b = 0 PSNR, b = 1500 PSNR of the model's images)."""
    s, adc = A.solve_adc(data, A.STUDY_B, (2, 2), "mean", lam, huber, n_iter, (1.0, weight), coupling)
    rows = [A.map_scores(s[i], adc[i], hr, adc_true) for i in range(len(SEEDS))]
    return np.mean([(r[2], r[0], r[1]) for r in rows], axis=0)


# the per-channel solver at its own best pair: the bar the b = 0 image has to clear
per_channel = {}
for lam in (3e-3, 6e-3, 12e-3, 24e-3, 48e-3):
    for huber in (0.01, 0.03, 0.1):
        x = J.solve_joint(data, (2, 2), "mean", lam, huber, J.STUDY_ITERS, coupling="none")
        rows = [A.image_scores(x[i], hr, adc_true) for i in range(len(SEEDS))]
        per_channel[(lam, huber)] = np.mean([(r[2], r[0], r[1]) for r in rows], axis=0)
        print(f"per channel lambda {lam:g} huber {huber:g}: ADC RMSE {per_channel[(lam, huber)][0]:.4e}  PSNR b0 {per_channel[(lam, huber)][1]:.3f}  "
              f"b1500 {per_channel[(lam, huber)][2]:.3f}", flush=True)
pc_pair = min(per_channel, key=lambda key: per_channel[key][0])
pc_rmse, bar, pc_last = per_channel[pc_pair]
print(f"per channel: best pair lambda {pc_pair[0]:g} huber {pc_pair[1]:g}, ADC RMSE {pc_rmse:.4e}, b = 0 PSNR {bar:.3f} dB: the bar", flush=True)

table = {}


def run(lams, weights):
    for coupling in ("joint", "none"):
        for huber in HUBERS:
            for lam in lams:
                for weight in weights:
                    key = (coupling, lam, weight, huber)
                    if key in table:
                        continue
                    r = table[key] = score(*key)
                    print(f"{coupling} lambda {lam:g} weight {weight:g} huber {huber:g}: ADC RMSE {r[0]:.4e}  PSNR b0 {r[1]:.3f}  b1500 {r[2]:.3f}"
                          f"{'' if r[1] >= bar else '  (b0 below the bar)'}", flush=True)


def best_point():
    allowed = {key: r for key, r in table.items() if r[1] >= bar}
    return min(allowed, key=lambda key: allowed[key][0])


run(LAMBDAS, WEIGHTS)
best = best_point()
print(f"best of the grid: {best[0]} lambda {best[1]:g} weight {best[2]:g} huber {best[3]:g}, ADC RMSE {table[best][0]:.4e}, b0 "
      f"{table[best][1]:.3f} dB", flush=True)
more_l, more_w = list(LAMBDAS), list(WEIGHTS)
if best[1] == min(LAMBDAS):
    more_l.insert(0, best[1] / 2)
if best[1] == max(LAMBDAS):
    more_l.append(best[1] * 2)
if best[2] == min(WEIGHTS):
    more_w.insert(0, best[2] / 2)
if best[2] == max(WEIGHTS):
    more_w.append(min(1.0, best[2] * 2))
if (more_l, more_w) != (LAMBDAS, WEIGHTS):
    print(f"the best point sits on the edge: the grid is extended once to lambda {more_l} weight {more_w}", flush=True)
    run(more_l, more_w)
    best = best_point()
    edge = best[1] in (min(more_l), max(more_l)) or best[2] in (min(more_w), max(more_w))
    print(f"best of the extended grid: {best[0]} lambda {best[1]:g} weight {best[2]:g} huber {best[3]:g}, ADC RMSE {table[best][0]:.4e}, b0 "
          f"{table[best][1]:.3f} dB; {'still on the edge' if edge else 'inside the grid'}", flush=True)
r = table[best]
print(f"chosen: ADC RMSE {r[0]:.4e} against the per-channel best {pc_rmse:.4e} ({100 * (r[0] / pc_rmse - 1):+.1f} %); b = 0 PSNR {r[1]:.3f} dB "
      f"({r[1] - bar:+.3f} against the bar), b = 1500 PSNR {r[2]:.3f} dB against {pc_last:.3f}", flush=True)
for n in ITERS:
    r = score(*best, n_iter=n)
    print(f"{best[0]} lambda {best[1]:g} weight {best[2]:g} huber {best[3]:g} iterations {n}: ADC RMSE {r[0]:.4e}  PSNR b0 {r[1]:.3f}  b1500 {r[2]:.3f}",
          flush=True)
# the log-linear fit of the model's images at the chosen point, for comparison with the map itself
s, adc = A.solve_adc(data, A.STUDY_B, (2, 2), "mean", best[1], best[3], SWEEP_ITERS, (1.0, best[2]), best[0])
fit = np.mean([A.image_scores(A.model(s[i], adc[i], A.STUDY_B), hr, adc_true)[2] for i in range(len(SEEDS))])
print(f"log-linear fit of the model's images at the chosen point: ADC RMSE {fit:.4e}", flush=True)
