#!/usr/bin/env python3
"""Time the forward-mode derivative kernels (inr.derivatives, csrc/jet.hip) on dense grids, beside a plain-torch float32 SIREN of
the same architecture under double-backward autograd (the reference's route, nn_mri.py:205-221) on the same GPU.

    python tools/jet_time.py [output file]        # prints and writes profiles/jet_time.txt (or the file named)

Default network Siren(256, 512, 3, 1) with 128 Fourier frequencies; grids 128 x 128 x 24 x 4 (tangents along the three spatial
axes, as superresDWI --derivative_maps runs it) and 256 x 256 x 28 (all three axes).  Value + gradient + Laplacian of every grid
point; medians of host-timed synchronised calls.  The torch module works through the grid in chunks of 65,536 rows (its graph of
a first backward pass has to fit).  Not gated; the figures are what a run recorded."""
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mri_super_resolution_amd as inr  # noqa: E402

TORCH_CHUNK = 65536


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


def torch_derivatives(weights, B, coords, dt):
    """y, gradient and Laplacian (over the dt leading axes) of a plain float32 SIREN by double-backward autograd, chunk by chunk."""
    out = []
    for r in range(0, coords.shape[0], TORCH_CHUNK):
        x = coords[r:r + TORCH_CHUNK].clone().requires_grad_(True)
        p = 2.0 * math.pi * x @ B.T
        a = torch.cat([torch.sin(p), torch.cos(p)], dim=-1)
        for W, b in weights[:-1]:
            a = torch.sin(30.0 * (a @ W.T + b))
        y = a @ weights[-1][0].T + weights[-1][1]
        g = torch.autograd.grad(y.sum(), x, create_graph=True)[0]
        lap = 0.
        for i in range(dt):
            lap = lap + torch.autograd.grad(g[:, i].sum(), x, retain_graph=i + 1 < dt)[0][:, i]
        out.append((y.detach(), g.detach(), lap))
    return out


def main(argv):
    out = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "jet_time.txt")
    lines = [f"device {torch.cuda.get_device_name(0)}; Siren(256, 512, 3, 1), m = 128; value + gradient + Laplacian on a dense grid; "
             "medians, host timer around a synchronised call"]
    torch.manual_seed(0)
    model = inr.Siren(256, 512, 3, 1).cuda()
    params = [p.detach() for p in model.layer_parameters()]
    weights = [(params[2 * l], params[2 * l + 1]) for l in range(len(params) // 2)]
    for shape, dt in (((128, 128, 24, 4), 3), ((256, 256, 28), 3)):
        d = len(shape)
        rows = math.prod(shape)
        B = (torch.randn(128, d) * 0.5).cuda()
        ours = median_ms(lambda: inr.derivatives(model, shape=shape, B=B, d_tangent=dt), warmup=1, iters=5)
        coords = inr.get_mgrid(shape)
        theirs = median_ms(lambda: torch_derivatives(weights, B, coords, dt), warmup=1, iters=2)
        lines.append(f"grid {'x'.join(map(str, shape))} ({rows} rows, {dt} tangents): hip forward mode {ours:9.2f} ms ({rows / ours / 1e3:7.3f} M rows/s; "
                     f"5 timed)   torch float32 double-backward {theirs:9.2f} ms ({rows / theirs / 1e3:7.3f} M rows/s; 2 timed)   "
                     f"torch/hip {theirs / ours:5.2f}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv)
