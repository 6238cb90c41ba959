"""GPU box: ms per step of the footprint fit (FootprintSirenFitter: training forward, footprint loss, backward, Adam as four paths per
step) against SirenFitter.step on the same number of plain rows -- the same GEMM work --, and the time of one
ops.footprint_loss_grad call between device events (two launches and three allocations: host-issued call time, not kernel time):
    python tools/footprint_time.py [rows ...]        (default 114688 524288; K = 1, 4, 12; Siren(256, 512, 3, 1))
The two fitters are timed alternately, three windows each, and the median is printed."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mri_super_resolution_amd as inr  # noqa: E402
from mri_super_resolution_amd import ops  # noqa: E402


def window(fitter, args, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fitter.step(*args, n_steps=k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def loss_call_ms(n, K, fw):
    y, t = torch.rand(n * K, device="cuda"), torch.rand(n, device="cuda")
    for _ in range(3):
        ops.footprint_loss_grad(y, t, None, fw)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 50
    a.record()
    for _ in range(reps):
        ops.footprint_loss_grad(y, t, None, fw)      # (allocations, the loss kernel and the one-block sum of its partials)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


for rows in [int(a) for a in sys.argv[1:]] or [114688, 524288]:
    k = 20 if rows > 200000 else 60
    for K in (1, 4, 12):
        n = rows // K
        fp = inr.Footprint(np.zeros((K, 2)), np.full(K, 1.0 / K))
        x = torch.rand(n * K, 256, device="cuda") * 2 - 1
        t = torch.rand(n, device="cuda")
        t_plain = torch.rand(n * K, 1, device="cuda")
        torch.manual_seed(0)
        foot = inr.FootprintSirenFitter(inr.Siren(256, 512, 3, 1).cuda(), fp, lr=1e-4)
        torch.manual_seed(0)
        plain = inr.SirenFitter(inr.Siren(256, 512, 3, 1).cuda(), lr=1e-4)
        foot.step(x, t, n_steps=3)
        plain.step(x, t_plain, n_steps=3)
        a, b = [], []
        for _ in range(3):
            a.append(window(foot, (x, t), k))
            b.append(window(plain, (x, t_plain), k))
        a, b = float(np.median(a)), float(np.median(b))
        lk = loss_call_ms(n, K, fp.tensors(x.device)[1])
        print(f"rows {n * K} (n {n} x K {K}): footprint fit {a:.3f} ms/step, plain fit on the same rows {b:.3f} ms/step, ratio {a / b:.3f}; "
              f"one ops.footprint_loss_grad call {lk * 1e3:.1f} us", flush=True)
        del foot, plain, x
        torch.cuda.empty_cache()
