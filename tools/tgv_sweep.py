"""CPU: the sweep behind the defaults of baselines.tgv_superres / scripts/second_order:
    python tools/tgv_sweep.py
The float64 restatement (tests/tgv_common.py) on two cases, 2 x 2 block means, noise 0.02 drawn from default_rng(seed), seeds 0 .. 2,
300 iterations:
  pat07    the study case of tools/tvj_sweep.py restricted to its b = 0 channel: tests/golden/pat07_volume.npz, ROI 40:90 divided by
           its maximum, slices 10 / 14 / 18;
  phantom  the 48 x 48 ramp / quadratic / disc of the tests (tgv_common.phantom).
lambda x ratio (1, 2, 4) x Huber (0, 0.03) for the TGV prior, beside the first-order prior (tests/tvsr_common.py) over the same lambdas
and Huber thresholds.  Per row: PSNR and Gaussian SSIM (tests/perceptual_common.py) against the HR image, mean over slices and seeds,
and the flat-area index -- the share of interior pixels with |grad x| < 1e-3, beside the HR image's own; it is reported, not gated.
The defaults are the (lambda, ratio) pair -- with its Huber threshold -- of the best mean PSNR on pat07.  If that pair sits on an edge
of the lambda or ratio grid, the grid is extended ONCE on that side and the run says so."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import perceptual_common as P  # noqa: E402
from tests import tgv_common as G  # noqa: E402
from tests import tvj_common as J  # noqa: E402
from tests import tvsr_common as T  # noqa: E402

LAMBDAS = [2.5e-3, 5e-3, 1e-2, 2e-2, 4e-2]
RATIOS = [1.0, 2.0, 4.0]
HUBERS = (0.0, 0.03)
SEEDS = (0, 1, 2)
ITERS = 300


def pat07_case(seed):
    hr, y, _ = J.study_case(seed)
    return hr[:, 0], y[:, 0]


def phantom_case(seed):
    hr, y = G.phantom_data(seed)
    return hr[None], y[None]


CASES = {"pat07": [pat07_case(s) for s in SEEDS], "phantom": [phantom_case(s) for s in SEEDS]}


def scores(name, solve):
    """-> mean over the seeds of (PSNR, SSIM, flat-area index) of ``solve(y)`` against the HR images of case ``name``."""
    rows = []
    for hr, y in CASES[name]:
        x = solve(y)
        rows.append((T.psnr(hr, x), np.mean([P.ssim_gauss(a, b)[0] for a, b in zip(hr, x)]), G.flat_share(x)))
    return np.mean(rows, axis=0)


def show(label, s):
    print(f"{label}: " + "  ".join(f"{name} PSNR {s[name][0]:.3f} SSIM {s[name][1]:.4f} flat {s[name][2]:.3f}" for name in CASES), flush=True)


def tgv_row(table, lam, ratio, huber):
    if (lam, ratio, huber) not in table:
        table[(lam, ratio, huber)] = {name: scores(name, lambda y: G.solve(y, (2, 2), "mean", lam, ratio, huber, ITERS)) for name in CASES}
        show(f"tgv lambda {lam:g} ratio {ratio:g} huber {huber:g}", table[(lam, ratio, huber)])


def tv_row(table, lam, huber):
    if (lam, huber) not in table:
        table[(lam, huber)] = {name: scores(name, lambda y: T.solve(y, (2, 2), "mean", lam, huber, ITERS)) for name in CASES}
        show(f"tv  lambda {lam:g} huber {huber:g}", table[(lam, huber)])


def best_of(table):
    return max(table, key=lambda key: table[key]["pat07"][0])


for name in CASES:
    print(f"{name}: HR flat-area index {np.mean([G.flat_share(hr) for hr, _ in CASES[name]]):.3f}; block replication PSNR "
          f"{scores(name, lambda y: T.replicate(y, (2, 2)))[0]:.3f}", flush=True)
tgv, tv = {}, {}
for lam in LAMBDAS:
    for huber in HUBERS:
        tv_row(tv, lam, huber)
        for ratio in RATIOS:
            tgv_row(tgv, lam, ratio, huber)
lam, ratio, huber = best_of(tgv)
extended = []
if lam in (LAMBDAS[0], LAMBDAS[-1]):
    extended.append(("lambda", lam / 2 if lam == LAMBDAS[0] else lam * 2))
    LAMBDAS.append(extended[-1][1])
if ratio in (RATIOS[0], RATIOS[-1]):
    extended.append(("ratio", ratio / 2 if ratio == RATIOS[0] else ratio * 2))
    RATIOS.append(extended[-1][1])
if extended:
    print(f"the best pair (lambda {lam:g}, ratio {ratio:g}) sits on a grid edge: extending once by " +
          ", ".join(f"{axis} {value:g}" for axis, value in extended), flush=True)
    for lam in LAMBDAS:
        for huber in HUBERS:
            tv_row(tv, lam, huber)
            for ratio in RATIOS:
                tgv_row(tgv, lam, ratio, huber)
    lam, ratio, huber = best_of(tgv)
lt, ht = best_of(tv)
print(f"tgv: best mean PSNR on pat07 at lambda {lam:g} ratio {ratio:g} huber {huber:g}: {tgv[(lam, ratio, huber)]['pat07'][0]:.3f} dB "
      f"(phantom {tgv[(lam, ratio, huber)]['phantom'][0]:.3f} dB); tv: best at lambda {lt:g} huber {ht:g}: {tv[(lt, ht)]['pat07'][0]:.3f} dB "
      f"(phantom {tv[(lt, ht)]['phantom'][0]:.3f} dB); TGV - TV on pat07 {tgv[(lam, ratio, huber)]['pat07'][0] - tv[(lt, ht)]['pat07'][0]:+.3f} dB",
      flush=True)
bp = max(tgv, key=lambda key: tgv[key]["phantom"][0])
bt = max(tv, key=lambda key: tv[key]["phantom"][0])
print(f"phantom: tgv best at lambda {bp[0]:g} ratio {bp[1]:g} huber {bp[2]:g}: {tgv[bp]['phantom'][0]:.3f} dB; tv best at lambda {bt[0]:g} huber "
      f"{bt[1]:g}: {tv[bt]['phantom'][0]:.3f} dB", flush=True)
