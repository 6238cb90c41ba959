#!/usr/bin/env python3
"""Time the forward-mode derivative kernels of the WIRE network (wire.derivatives, csrc/wire_deriv.hip) on dense grids, beside the
same network in plain complex64 torch under double-backward autograd (the reference's route, nn_mri.py:205-221 over the stack of
wiretest.ipynb cell 2) on the same GPU, and beside wire.reconstruct (the value alone) on the same grid.

    python tools/wire_deriv_time.py [output file]        # prints and writes profiles/wire_deriv_time.txt (or the file named)

Default network: the notebook's, Wire(512, 128, 3, 1) with 256 Fourier frequencies and omega_0 = scale_0 = 1.2; grids
128 x 128 x 24 x 4 (tangents along the three spatial axes, as superresDWI --wire_derivative_maps runs it) and 256 x 256 x 28 (all
three axes).  Value + gradient + Laplacian of every grid point; medians of host-timed synchronised calls.
The torch stack works through the grid in chunks of 65,536 rows (its graph of a first backward pass has to fit).  Not gated; the
figures are what a run recorded."""
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mri_super_resolution_amd as inr  # noqa: E402
from mri_super_resolution_amd import wire  # noqa: E402

TORCH_CHUNK = 65536
M, HIDDEN, LAYERS, OMEGA, SCALE = 256, 128, 3, 1.2, 1.2


def median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def torch_derivatives(model, B, coords, dt):
    """y, gradient and Laplacian (over the dt leading axes) of the stack in plain complex64 torch by double-backward autograd."""
    P = {k: v.detach() for k, v in model.state_dict().items()}
    out = []
    for r in range(0, coords.shape[0], TORCH_CHUNK):
        x = coords[r:r + TORCH_CHUNK].clone().requires_grad_(True)
        p = (2.0 * math.pi * x) @ B.T
        h = torch.cat([torch.sin(p), torch.cos(p)], dim=-1)
        for k in range(LAYERS + 1):
            lin = h @ P[f"net.{k}.linear.weight"].T + P[f"net.{k}.linear.bias"]
            orth = h @ P[f"net.{k}.scale_orth.weight"].T + P[f"net.{k}.scale_orth.bias"]
            h = torch.exp(1j * OMEGA * lin) * torch.exp(-SCALE * SCALE * (lin.abs().square() + orth.abs().square()))
        y = (h @ P["final_linear.weight"].T + P["final_linear.bias"]).real
        g = torch.autograd.grad(y.sum(), x, create_graph=True)[0]
        lap = 0.
        for i in range(dt):
            lap = lap + torch.autograd.grad(g[:, i].sum(), x, retain_graph=i + 1 < dt)[0][:, i]
        out.append((y.detach(), g.detach(), lap))
    return out


def main(argv):
    out = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "wire_deriv_time.txt")
    lines = [f"device {torch.cuda.get_device_name(0)}; Wire({2 * M}, {HIDDEN}, {LAYERS}, 1), m = {M}, omega_0 = scale_0 = 1.2; value + "
             "gradient + Laplacian on a dense grid; medians, host timer around a synchronised call"]
    torch.manual_seed(0)
    model = wire.Wire(2 * M, HIDDEN, LAYERS, 1, first_omega_0=OMEGA, hidden_omega_0=OMEGA, scale=SCALE).cuda()
    for shape, dt in (((128, 128, 24, 4), 3), ((256, 256, 28), 3)):
        d = len(shape)
        rows = math.prod(shape)
        B = (torch.randn(M, d) * 0.5).cuda()
        ours = median_ms(lambda: wire.derivatives(model, shape=shape, B=B, d_tangent=dt), warmup=1, iters=5)
        value = median_ms(lambda: wire.reconstruct(model, shape, B, clamp_min=None), warmup=1, iters=5)
        coords = inr.get_mgrid(shape)
        theirs = median_ms(lambda: torch_derivatives(model, B, coords, dt), warmup=1, iters=2)
        lines.append(f"grid {'x'.join(map(str, shape))} ({rows} rows, {dt} tangents): hip forward mode {ours:9.2f} ms ({rows / ours / 1e3:7.3f} M rows/s; "
                     f"5 timed)   wire.reconstruct (value only) {value:9.2f} ms   torch complex64 double-backward {theirs:9.2f} ms "
                     f"({rows / theirs / 1e3:7.3f} M rows/s; 2 timed)   torch/hip {theirs / ours:5.2f}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv)
