#!/usr/bin/env python3
"""Writes tests/golden/wire_pn.npz: the gradient of the REFERENCE's own complex-Gabor network with respect to its input, and
the PerturbNet phase of wiretest.ipynb cell 10 built on it, for tests/test_wire_pn_cpu.py to hold tests/wire_pn_common.py's
restatement to and for tests/test_gpu_wire_pn.py to hold the kernels to.

    python tools/make_wire_pn_golden.py <reference dir holding INRmodel.py> [output.npz]

Imports ``ComplexGaborLayer2D``, ``PN``, ``input_mapping`` and ``get_mgrid`` from the reference's ``INRmodel``, stacks the layer
as wiretest.ipynb cell 2 does (the input is NOT detached there) and evaluates everything in double precision: real tensors
float64, complex ones complex128 (as tools/make_wire_golden.py).  ``PN.forward`` hard-codes ``.cuda()``: an identity shim
keeps it on the host, the way tests/golden/pn.npz was made.  The case: a 3 x 3 x 37 grid (333 rows, d = 3), m = 8 Fourier
frequencies (in_features 16), hidden width 32, one hidden layer, omega_0 = scale_0 = float32(1.2), PerturbNet width 32,
eps = 1/128, K = 2 acquisitions, seed 0.  The file holds
  * the float32 weights as drawn (``w/`` the network, ``pn/`` the PerturbNet), ``coords``, ``B``, ``x`` = input_mapping(coords, B),
    ``eps``, the acquisitions ``acq`` [2, 3, 3, 37] and their mean ``mean``;
  * ``gy``, ``y`` and ``dx`` = d(sum gy y)/dx at x;
  * ``step_loss`` and ``step_g/*``: loss and the four PerturbNet gradients of ONE PerturbNet step (sample 1);
  * ``sched_pn_losses``, ``sched_inr_losses`` and ``sched_m/*``: cell 10's loop with number_of_epochs = pertubation_epochs = 4
    (epochs 0 and 2: a PerturbNet step per acquisition, Adam lr 1e-6; epochs 1 and 3: an INR step, Adam lr 5e-5) -- the four
    PerturbNet losses, the two INR losses and the PerturbNet's first-moment state ``exp_avg`` after it;
  * ``noise/*``: the reference's own float32 (complex64) run of each of these against its float64 run, as relative L2 -- the
    arithmetic noise the GPU test's bounds are held to (at least 20 x above it).  The figures are printed too.
Data only, about 100 KB.  Runs on the host; no GPU needed."""
import copy
import os
import sys

import numpy as np
import torch
from torch import nn

GRID, D, M, HIDDEN, LAYERS, OMEGA, SCALE, PN_DIM, K, EPS = (3, 3, 37), 3, 8, 32, 1, 1.2, 1.2, 32, 2, 1 / 128.
EPOCHS = PERT_EPOCHS = 4
LR, PN_LR = 5e-5, 1e-6


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


def evaluate(INRmodel, model, pn, x, B, gy, mean_t, acq_t):
    """Everything the fixture records, in the precision of the modules and tensors handed in."""
    out = {}
    xg = x.clone().requires_grad_(True)
    y = model(xg)
    (dx,) = torch.autograd.grad((y[:, 0] * gy).sum(), xg)
    out["y"], out["dx"] = y.detach().numpy()[:, 0].copy(), dx.numpy().copy()

    def pn_loss(sample):
        perturbed = INRmodel.input_mapping(pn.forward(x, sample, EPS), B)
        return ((model.forward(perturbed) - acq_t[sample]) ** 2).mean()

    loss = pn_loss(1)
    names = [n for n, _ in pn.named_parameters()]
    grads = torch.autograd.grad(loss, list(pn.parameters()))
    out["step_loss"] = np.asarray(loss.item())
    for n, g in zip(names, grads):
        out["step_g/" + n] = g.numpy().copy()

    model, pn = copy.deepcopy(model), copy.deepcopy(pn)          # the schedule moves both
    inr_optim = torch.optim.Adam(lr=LR, params=list(model.parameters()))
    perturb_optim = torch.optim.Adam(lr=PN_LR, params=list(pn.parameters()))
    pn_losses, inr_losses = [], []
    for ctr in range(EPOCHS):                                      # wiretest.ipynb cell 10
        if ctr < EPOCHS - PERT_EPOCHS or ctr % 2:
            loss = ((model.forward(x) - mean_t) ** 2).mean()
            inr_optim.zero_grad()
            loss.backward()
            inr_optim.step()
            inr_losses.append(loss.item())
        else:
            for sample in range(K):
                perturbed = INRmodel.input_mapping(pn.forward(x, sample, EPS), B)
                loss = ((model.forward(perturbed) - acq_t[sample]) ** 2).mean()
                perturb_optim.zero_grad()
                loss.backward()
                perturb_optim.step()
                pn_losses.append(loss.item())
    out["sched_pn_losses"], out["sched_inr_losses"] = np.asarray(pn_losses), np.asarray(inr_losses)
    for n, p in pn.named_parameters():
        out["sched_m/" + n] = perturb_optim.state[p]["exp_avg"].numpy().copy()
    return out


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(argv[1]))
    import INRmodel
    torch.Tensor.cuda = lambda self, *a, **k: self               # PN.forward's hard-coded .cuda()
    out = argv[2] if len(argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                     "wire_pn.npz")

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
    pn = INRmodel.PN(in_features=2 * M, hidden_features=PN_DIM, dimension=D)
    coords = INRmodel.get_mgrid(GRID).float()
    B = (torch.randn(M, D) * 0.5).float()
    acq = torch.rand(K, *GRID)
    gy = torch.randn(coords.shape[0]).float()
    feats = INRmodel.input_mapping(coords, B).float()
    mean = acq.mean(0)
    data = {"coords": coords.numpy(), "B": B.numpy(), "x": feats.numpy(), "eps": np.asarray(EPS), "acq": acq.numpy(),
            "mean": mean.numpy(), "gy": gy.numpy(), "keys": np.asarray(list(model.state_dict().keys()))}
    for k, v in model.state_dict().items():
        data["w/" + k] = pairs(v)
    for k, v in pn.state_dict().items():
        data["pn/" + k] = pairs(v)

    flat = lambda t: t.reshape(t.shape[0], -1, 1) if t.dim() == 4 else t.reshape(-1, 1)      # noqa: E731
    single = evaluate(INRmodel, copy.deepcopy(model), copy.deepcopy(pn), feats, B, gy, flat(mean), flat(acq))
    double = evaluate(INRmodel, to_double(model), to_double(pn), feats.double(), B.double(), gy.double(), flat(mean).double(),
                      flat(acq).double())
    data.update(double)
    groups = {"y": ["y"], "dx": ["dx"], "step_loss": ["step_loss"], "step_g": [k for k in double if k.startswith("step_g/")],
              "sched_pn_losses": ["sched_pn_losses"], "sched_inr_losses": ["sched_inr_losses"],
              "sched_m": [k for k in double if k.startswith("sched_m/")]}
    for name, keys in groups.items():
        worst = max(rel_l2(single[k], double[k]) for k in keys)
        data["noise/" + name] = np.asarray(worst)
        for k in keys:
            print(f"float32 against float64 of the reference: {k:40s} rel-L2 {rel_l2(single[k], double[k]):.3e}")
    np.savez(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv)
