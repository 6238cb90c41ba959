"""Batched small-net fits (inr.fit_cycle_batch, one cooperative launch carrying several problems) against the same fits one
after the other (SirenFitter.step_cycle each), master.py's regime: 60x60 slice, weighted loss, 3 acquisitions per fit.
Prints, for K = 1 .. 4 fits of Siren(2,64,6,1) and Siren(2,32,2,1): wall microseconds per optimizer step of the whole group
and the aggregate fit-steps per second, sequential vs batched.  Median of 3 timed repeats after a warm-up.
    python tools/small_batch_time.py [side] [steps]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mri_super_resolution_amd as inr  # noqa: E402
from mri_super_resolution_amd import ops  # noqa: E402

side = int(sys.argv[1]) if len(sys.argv) > 1 else 60
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
n = side * side
N_ACQ = 3
coords = inr.ImageFitting_set([np.zeros((side, side), np.float32)]).coords[0]


def fitters(hidden, layers, K):
    out = []
    for k in range(K):
        torch.manual_seed(k)
        out.append(inr.SirenFitter(inr.Siren(2, hidden, layers, 1).cuda(), lr=3e-4))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


print(f"N={n} rows, {steps} steps per fit, {N_ACQ} acquisitions (weighted), device {torch.cuda.get_device_name(0)}")
print(f"{'net':>16} {'K':>2} {'seq us/step':>12} {'batch us/step':>14} {'seq fit-steps/s':>16} {'batch fit-steps/s':>18} "
      f"{'gain':>6} {'launches':>9}")
for hidden, layers in ((64, 6), (32, 2)):
    for K in (1, 2, 3, 4):
        torch.manual_seed(100)
        tg = [torch.rand(N_ACQ, n, device="cuda") * 2 - 1 for _ in range(K)]
        wt = [torch.rand(N_ACQ, n, device="cuda") for _ in range(K)]
        seq_f, bat_f = fitters(hidden, layers, K), fitters(hidden, layers, K)

        def seq(s):
            for f, t, w in zip(seq_f, tg, wt):
                f.step_cycle(coords, t, s, w)

        def bat(s):
            inr.fit_cycle_batch(bat_f, coords, tg, s, weights=wt)

        seq(64)
        bat(64)
        t_seq = statistics.median(timed(lambda: seq(steps)) for _ in range(3))
        ops.launch_counts_reset()
        t_bat = statistics.median(timed(lambda: bat(steps)) for _ in range(3))
        launches = ops.launch_counts()["small_batch"] // 3
        print(f"{f'Siren(2,{hidden},{layers},1)':>16} {K:>2} {1e6 * t_seq / steps:>12.1f} {1e6 * t_bat / steps:>14.1f} "
              f"{K * steps / t_seq:>16.0f} {K * steps / t_bat:>18.0f} {t_seq / t_bat:>5.2f}x {launches:>9}")
