#!/usr/bin/env python3
"""Writes tests/golden/wire_deriv.npz: value, coordinate gradient and Laplacian of the REFERENCE's own complex-Gabor network, for
tests/test_wire_deriv_cpu.py to hold tests/wire_deriv_common.py's restatement to and for tests/test_gpu_wire_deriv.py to hold the
forward-mode kernels of csrc/wire_deriv.hip to.

    python tools/make_wire_deriv_golden.py <reference dir holding INRmodel.py> [output.npz]

Imports ``ComplexGaborLayer2D``, ``input_mapping`` and ``get_mgrid`` from the reference's ``INRmodel``, stacks the layer as
wiretest.ipynb cell 2 does (the input is NOT detached there) and differentiates y = INR(input_mapping(x, B)) with respect to the
coordinates x the way nn_mri.py:205-221 does: ``gradient`` is one ``autograd.grad`` with create_graph=True, ``laplace`` its
divergence, a second ``autograd.grad`` per axis.  Everything in double precision: real tensors float64, complex ones complex128
(as tools/make_wire_pn_golden.py).  The case: a 3 x 3 x 37 grid (333 rows, d = 3, tangents along all three axes), m = 8 Fourier
frequencies (in_features 16), hidden width 32, one hidden layer, omega_0 = scale_0 = float32(1.2), seed 0.  The file holds
  * the float32 weights as drawn (``w/``), ``x`` = get_mgrid((3, 3, 37)) and ``B``;
  * ``y`` [333], ``grad`` [333, 3], ``lap`` [333] of the float64 run;
  * ``noise/y``, ``noise/grad``, ``noise/lap``: the reference's own float32 (complex64) run against its float64 run, as relative
    L2 -- the arithmetic noise of plain float32 on this problem.  The figures are printed too.
Data only, about 50 KB.  Runs on the host; no GPU needed."""
import copy
import os
import sys

import numpy as np
import torch
from torch import nn

GRID, D, M, HIDDEN, LAYERS, OMEGA, SCALE = (3, 3, 37), 3, 8, 32, 1, 1.2, 1.2


def pairs(t):
    """A tensor as a real array: a complex one as its interleaved (re, im) pairs [..., 2]."""
    t = t.detach()
    return (torch.view_as_real(t) if t.is_complex() else t).numpy().copy()


def rel_l2(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def to_double(module):
    for p in module.parameters():
        p.data = p.data.to(torch.complex128 if p.is_complex() else torch.float64)
    return module


def evaluate(INRmodel, model, x, B):
    """nn_mri.py:205-221 on y = model(input_mapping(x, B)), in the precision of the module and tensors handed in."""
    x = x.clone().requires_grad_(True)
    y = model(INRmodel.input_mapping(x, B))[:, 0]
    (g,) = torch.autograd.grad(y, [x], grad_outputs=torch.ones_like(y), create_graph=True)          # gradient
    lap = 0.
    for i in range(D):                                                                              # divergence
        lap = lap + torch.autograd.grad(g[..., i], x, torch.ones_like(g[..., i]), create_graph=True)[0][..., i]
    return {"y": y.detach().numpy().copy(), "grad": g.detach().numpy().copy(), "lap": lap.detach().numpy().copy()}


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(argv[1]))
    import INRmodel
    torch.Tensor.cuda = lambda self, *a, **k: self               # get_mgrid / input_mapping stay on the host
    out = argv[2] if len(argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                     "wire_deriv.npz")

    class Net(nn.Module):     # wiretest.ipynb cell 2: head registered first, and again as the stack's last module; no detach
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
    x = INRmodel.get_mgrid(GRID).float()
    B = (torch.randn(M, D) * 0.5).float()
    data = {"x": x.numpy(), "B": B.numpy(), "keys": np.asarray(list(model.state_dict().keys()))}
    for k, v in model.state_dict().items():
        data["w/" + k] = pairs(v)
    single = evaluate(INRmodel, copy.deepcopy(model), x, B)
    double = evaluate(INRmodel, to_double(model), x.double(), B.double())
    data.update(double)
    for k in ("y", "grad", "lap"):
        data["noise/" + k] = np.asarray(rel_l2(single[k], double[k]))
        print(f"float32 against float64 of the reference: {k:6s} rel-L2 {rel_l2(single[k], double[k]):.3e}   max|.| "
              f"{np.abs(double[k]).max():.3e}")
    np.savez(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv)
