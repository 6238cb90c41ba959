#!/usr/bin/env python3
"""Writes tests/golden/wire_inrmodel.npz: outputs, loss, gradients and a 20-step Adam trajectory of the REFERENCE's own
complex-Gabor layer, for tests/test_wire_cpu.py to hold tests/wire_common.py's restatement to and for tests/test_gpu_wire.py
to hold the kernels to.

    python tools/make_wire_golden.py <reference dir holding INRmodel.py> [output.npz]

Imports ``ComplexGaborLayer2D`` and ``input_mapping`` from the reference's ``INRmodel``, stacks the layer into the network
wiretest.ipynb trains (first layer, hidden layers, complex head, real part out) and evaluates it in double precision: real
tensors become float64, complex ones complex128 (casting the whole module to one dtype would make the first layer's real
weights complex and let Adam move imaginary parts the network does not have).  The case: 333 rows, d = 3 coordinates,
m = 16 Fourier frequencies, hidden width 32, one hidden layer, omega_0 = scale_0 = float32(1.2), seed 0.  The file holds data
only (about 100 KB): inputs, the float32 weights as drawn (complex ones as float pairs), and float64 results.  Runs on the
host; no GPU needed."""
import os
import sys

import numpy as np
import torch
from torch import nn

ROWS, D, M, HIDDEN, LAYERS, OMEGA, SCALE, STEPS, LR = 333, 3, 16, 32, 1, 1.2, 1.2, 20, 5e-5


def pairs(t):
    """A tensor as a real array: a complex one as its interleaved (re, im) pairs [..., 2]."""
    t = t.detach()
    return (torch.view_as_real(t) if t.is_complex() else t).numpy().copy()


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(argv[1]))
    import INRmodel
    out = argv[2] if len(argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                     "wire_inrmodel.npz")

    class Net(nn.Module):     # the composition the notebook trains: head registered first, and again as the stack's last module
        def __init__(self):
            super().__init__()
            net = [INRmodel.ComplexGaborLayer2D(2 * M, HIDDEN, omega0=OMEGA, sigma0=SCALE, is_first=True, trainable=False)]
            for _ in range(LAYERS):
                net.append(INRmodel.ComplexGaborLayer2D(HIDDEN, HIDDEN, is_first=False, omega0=OMEGA, sigma0=SCALE))
            self.final_linear = nn.Linear(HIDDEN, 1, dtype=torch.cfloat)
            net.append(self.final_linear)
            self.net = nn.Sequential(*net)

        def forward(self, x):
            return self.net(x).real

    torch.manual_seed(0)
    model = Net()
    coords = torch.rand(ROWS, D) * 2 - 1
    B = (torch.randn(M, D) * 0.5).float()
    target = torch.rand(ROWS, 1)
    feats = INRmodel.input_mapping(coords, B).float()
    data = {"coords": coords.numpy(), "B": B.numpy(), "x": feats.numpy(), "target": target.numpy()[:, 0],
            "keys": np.asarray(list(model.state_dict().keys()))}
    for k, v in model.state_dict().items():
        data["w/" + k] = pairs(v)
    for p in model.parameters():
        p.data = p.data.to(torch.complex128 if p.is_complex() else torch.float64)
    x, t = feats.double(), target.double()
    y = model(x)
    loss = ((y - t) ** 2).mean()
    loss.backward()
    data["y"] = y.detach().numpy()[:, 0]
    data["loss"] = np.asarray(loss.item())
    for k, p in model.named_parameters():
        if p.requires_grad:
            data["g/" + k] = pairs(p.grad)
    optim = torch.optim.Adam(lr=LR, params=list(model.parameters()))
    losses = []
    for _ in range(STEPS):
        loss = ((model(x) - t) ** 2).mean()
        optim.zero_grad()
        loss.backward()
        optim.step()
        losses.append(loss.item())
    data["traj_losses"] = np.asarray(losses)
    data["traj_y"] = model(x).detach().numpy()[:, 0]
    np.savez(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv)
