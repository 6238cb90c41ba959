#!/usr/bin/env python3
"""Time the PIA kernels against a plain-torch module of the same architecture on the same GPU.

    python tools/pia_time.py            # prints and writes profiles/pia_time.txt

Fused step (ms, median of 50 timed iterations after 10 warm-up) at batch 512 / 4,096 / 65,536 and rows/s of
`encode_volume` at 128 x 128 x 24 and 256 x 256 x 96 voxels; beside each the same quantity for `TorchPIA` below --
nn.Linear, LeakyReLU and the decoder as float32 tensor ops with torch.optim.Adam: what a user gets without these kernels.
"""
import os
import statistics
import sys
import time

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mri_super_resolution_amd import pia_net  # noqa: E402


class TorchPIA(nn.Module):
    def __init__(self):
        super().__init__()
        dims = [16, 32, 64, 128, 256, 512]
        self.encoder = nn.Sequential(*[nn.Sequential(nn.Linear(i, o), nn.LeakyReLU()) for i, o in zip(dims[:-1], dims[1:])])
        self.heads = nn.ModuleList([nn.Sequential(nn.Linear(512, 512), nn.LeakyReLU(), nn.Linear(512, 3)) for _ in range(3)])
        self.register_buffer("Dm", torch.tensor([0.5, 1.2, 2.85]))
        self.register_buffer("Dd", torch.tensor([0.2, 0.5, 0.15]))
        self.register_buffer("Tm", torch.tensor([45.0, 70.0, 750.0]))
        self.register_buffer("Td", torch.tensor([25.0, 30.0, 250.0]))
        self.register_buffer("nb", torch.tensor([-b / 1000 for b in (0, 150, 1000, 1500) for _ in range(4)]))
        self.register_buffer("te", torch.tensor([float(t) for _ in range(4) for t in (0, 13, 93, 143)]))

    def encode(self, x):
        h = self.encoder(x)
        return (self.Dm + self.Dd * torch.tanh(self.heads[0](h)), self.Tm + self.Td * torch.tanh(self.heads[1](h)),
                torch.softmax(self.heads[2](h), dim=1))

    def forward(self, x):
        D, T2, v = self.encode(x)
        S = (v[:, :, None] * torch.exp(self.nb[None, None, :] * D[:, :, None]) * torch.exp(-self.te[None, None, :] / T2[:, :, None])).sum(1)
        return 1000 * S


def median_ms(fn, warmup=10, iters=50):
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


def main():
    lines = [f"device {torch.cuda.get_device_name(0)}; medians, host timer around a synchronised call; fused step: 50 timed "
             "iterations after 10 warm-up; encode_volume: 3 warm-up, timed iterations as stated per row"]
    torch.manual_seed(0)
    model = pia_net.PIA().cuda()
    fitter = pia_net.PiaFitter(model, lr=1e-4)
    ref = TorchPIA().cuda()
    opt = torch.optim.Adam(ref.parameters(), lr=1e-4)

    def torch_step(x):
        loss = torch.mean((ref(x) - x) ** 2)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    np.random.seed(0)
    for n in (512, 4096, 65536):
        x = pia_net.get_batch(n, 0.02)[0].cuda()
        ours = median_ms(lambda: fitter.step(x))
        theirs = median_ms(lambda: torch_step(x))
        lines.append(f"fused step  batch {n:6d}: hip {ours:9.3f} ms   torch {theirs:9.3f} ms   torch/hip {theirs / ours:5.2f}")
    for shape in ((128, 128, 24), (256, 256, 96)):
        n = int(np.prod(shape))
        x = pia_net.get_batch(4096, 0.02)[0].cuda().repeat((n + 4095) // 4096, 1)[:n].contiguous()

        def torch_encode():
            with torch.no_grad():
                for r in range(0, n, 262144):
                    ref.encode(x[r:r + 262144])

        iters = 50 if n < 1_000_000 else 10
        ours = median_ms(lambda: fitter.encode_volume(x), warmup=3, iters=iters)
        theirs = median_ms(torch_encode, warmup=3, iters=iters)
        lines.append(f"encode_volume {shape[0]}x{shape[1]}x{shape[2]} ({n} rows, {iters} timed): hip {n / ours / 1e3:8.3f} M rows/s ({ours:8.2f} ms)   "
                     f"torch {n / theirs / 1e3:8.3f} M rows/s ({theirs:8.2f} ms)   hip/torch speed {theirs / ours:5.2f}")
    text = "\n".join(lines)
    print(text)
    out = os.path.join(ROOT, "profiles", "pia_time.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
