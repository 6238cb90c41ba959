#!/usr/bin/env python3
"""Milliseconds per fit step of the WIRE complex-Gabor network of wiretest.ipynb (512 -> 128 x (1 + 3) -> 1, omega_0 = scale_0
= 1.2, Adam lr 5e-5) through ``WireFitter`` at N = 18,900 rows (the notebook's 15 x 15 x 21 x 4 training grid) and N = 52,500.
A second leg times ONE PerturbNet step of cell 10 at 18,900 rows -- PN(512, 128, 4) -> input_mapping (B [256, 4]) -> the
network (``inr_wire_forward_stash``) -> torch MSE -> backward (``inr_wire_input_grad``, ``_FourierFn``, ``_PNFn``) -> Adam on the
PerturbNet's four tensors -- beside one plain fit step at the same rows, in the same run.
Reported, not gated.  The notebook's own progress bar shows 43.6 it/s at 18,900 rows on an unnamed GPU: context, not a target."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mri_super_resolution_amd as inr  # noqa: E402
from mri_super_resolution_amd import ops, wire  # noqa: E402


def timed(fn, steps):
    fn(steps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def perturbnet_leg(steps, n=18_900):
    torch.manual_seed(0)
    model = wire.Wire(512, 128, 3, 1, first_omega_0=1.2, hidden_omega_0=1.2, scale=1.2).cuda()
    fitter = wire.WireFitter(model, lr=5e-5)
    pn = inr.PN(512, 128, 4).cuda()
    B = (torch.randn(256, 4) * 0.5).cuda()
    x = inr.input_mapping(torch.rand(n, 4, device="cuda") * 2 - 1, B)
    target = torch.rand(n, 1, device="cuda")
    params = list(pn.parameters())
    state = [(torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    count = [0]

    def pn_steps(k):
        for _ in range(k):
            loss = ((model(inr.input_mapping(pn(x, 1, 1 / 128.), B)) - target) ** 2).mean()
            for p in params:
                p.grad = None
            loss.backward()
            count[0] += 1
            for p, (m, v) in zip(params, state):
                ops.adam_step(p.data, p.grad.contiguous(), m, v, count[0], 1e-6)

    ms_pn = timed(pn_steps, steps)
    ms_fit = timed(lambda k: fitter.step(x, target, k), steps)
    print(f"N={n} 512->128x(1+3)->1: one PerturbNet step {ms_pn:.3f} ms beside one plain fit step {ms_fit:.3f} ms "
          f"(ratio {ms_pn / ms_fit:.2f})")


def main(steps=50):
    for n in (18_900, 52_500):
        torch.manual_seed(0)
        model = wire.Wire(512, 128, 3, 1, first_omega_0=1.2, hidden_omega_0=1.2, scale=1.2).cuda()
        fitter = wire.WireFitter(model, lr=5e-5)
        proj = torch.randn(n, 256, device="cuda")
        x = torch.cat([torch.sin(proj), torch.cos(proj)], -1).contiguous()
        target = torch.rand(n, device="cuda")
        ms = timed(lambda k: fitter.step(x, target, k), steps)
        loss = float(fitter.step(x, target, 1)[0])
        print(f"N={n} 512->128x(1+3)->1: WIRE fused fit {ms:.3f} ms/step ({1e3 / ms:.1f} it/s), loss after {fitter.step_count} steps "
              f"{loss:.5f}")
    perturbnet_leg(steps)


if __name__ == "__main__":
    main()
