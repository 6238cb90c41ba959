#!/usr/bin/env python3
"""Milliseconds per pre-training step of the soft-ERD INR (ErdSiren(2, 128, 3), fused step + reduce/Adam/status kernels, stop
test on the device) at 64 x 64 and 128 x 128, beside the closest figure of the generic path in the same process: a plain
Siren(2, 128, 3, 1) step through SirenFitter (layer-by-layer kernels).  Reported, not gated."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mri_super_resolution_amd as inr  # noqa: E402
from mri_super_resolution_amd import erd_inr  # noqa: E402


def timed(fn, steps):
    fn(steps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main(steps=200):
    for side in (64, 128):
        coords = inr.get_mgrid(side, 2)
        target = torch.rand(side * side, device="cuda")
        torch.manual_seed(0)
        f = erd_inr.ErdFitter(erd_inr.ErdSiren(2, 128, 3).cuda())
        status = f.new_status(coords.device)

        def erd(n):
            f.pretrain_steps(coords, target, n, 3e-4, -1.0, status)
            f.step_count += n
        torch.manual_seed(0)
        g = inr.SirenFitter(inr.Siren(2, 128, 3, 1).cuda(), lr=3e-4)
        t_erd = timed(erd, steps)
        info = f.read_status(status)        # a collapsed or converged fit would have turned the timed launches into no-ops
        assert info["state"] == 0 and info["steps_done"] == 2 * steps, info
        print(f"{side}x{side} H=128 L=3: soft-ERD fused pre-training step {t_erd:.4f} ms/step ({info['steps_done']} steps applied, loss {info['last_loss']:.4f}); "
              f"plain Siren(2,128,3,1) generic step {timed(lambda n: g.step(coords, target.reshape(-1, 1), n_steps=n), steps):.4f} ms/step")


if __name__ == "__main__":
    main()
