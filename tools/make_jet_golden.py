#!/usr/bin/env python3
"""Writes tests/golden/jet_inrmodel.npz: value, coordinate gradient and Laplacian of the REFERENCE's own network, for
tests/test_jet_cpu.py to hold tests/jet_common.py's restatement to.

    python tools/make_jet_golden.py <reference dir holding INRmodel.py> [output.npz]

Imports ``Siren`` and ``input_mapping`` from the reference's ``INRmodel`` (the flavour whose forward does not detach its input),
casts the seeded module to float64 and differentiates it with the three autograd helpers below -- the definitions of
nn_mri.py:205-221.  The case is the one of test_gpu_jet.py's case b: 1,023 rows of the 11 x 31 x 3 grid, d = 3, m = 16 Fourier
frequencies, hidden width 64, two hidden layers.  The file holds data only (about 100 KB): the float32 parameters, B, the rows and
the float64 results.  Runs on the host; no GPU needed."""
import os
import sys

import numpy as np
import torch


def gradient(y, x):
    return torch.autograd.grad(y, [x], grad_outputs=torch.ones_like(y), create_graph=True)[0]


def divergence(y, x):
    return sum(torch.autograd.grad(y[..., i], x, torch.ones_like(y[..., i]), create_graph=True)[0][..., i:i + 1]
               for i in range(y.shape[-1]))


def laplace(y, x):
    return divergence(gradient(y, x), x)


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(argv[1]))
    import INRmodel
    out = argv[2] if len(argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                     "jet_inrmodel.npz")
    d, m, hidden, hidden_layers, shape = 3, 16, 64, 2, (11, 31, 3)
    torch.manual_seed(20)
    net = INRmodel.Siren(in_features=2 * m, hidden_features=hidden, hidden_layers=hidden_layers, out_features=1)
    B = (torch.randn(m, d) * 0.5).float()
    x32 = INRmodel.get_mgrid(shape).float()
    assert tuple(x32.shape) == (1023, d)
    data = {"shape": np.asarray(shape, np.int64), "B": B.numpy(), "x": x32.numpy()}
    layers = [mod.linear if hasattr(mod, "linear") else mod for mod in net.net]
    for l, lin in enumerate(layers):
        data[f"W{l}"] = lin.weight.detach().numpy().copy()
        data[f"b{l}"] = lin.bias.detach().numpy().copy()
    net = net.double()
    x = x32.double().requires_grad_(True)
    y = net(INRmodel.input_mapping(x, B.double()))
    data["y"] = y.detach().numpy()[:, 0]
    data["grad"] = gradient(y, x).detach().numpy()
    data["lap"] = laplace(y, x).detach().numpy()[:, 0]
    np.savez(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv)
