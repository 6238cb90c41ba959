"""Shared by test_jet_cpu.py / test_gpu_jet.py: a plain-torch SIREN (with and without Fourier features) whose coordinate gradient and
Laplacian come from double-backward autograd in float64 -- an independent route to the numbers the forward-mode kernels of
csrc/jet.hip produce; it uses none of their formulas -- the same formulas restated in plain torch (``forward_jet``: their float32
evaluation on the host sets the Laplacian's tolerance), and seeded case builders."""
import math

import numpy as np
import torch

ROWS = 1023           # 31 x 33 = 11 x 31 x 3: a ragged last 64-row tile, and with chunk_rows = 256 four chunks, the last ragged
CHUNK = 256
OMEGA = 30.0


def mgrid_rows(shape):
    """get_mgrid(shape) on the host in float32 (torch.linspace, 'ij' meshgrid, last axis fastest)."""
    axes = [torch.linspace(-1, 1, steps=int(s)) for s in shape]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, len(shape)).contiguous()


def make_case(seed, d, hidden, hidden_layers, m=0, grid=None, scale=0.5):
    """Weights with the SIREN initialisation (SRDWI.py:48-56, 75-77), a Gaussian Fourier matrix B [m, d] (m = 0: none) and 1,023
    coordinate rows: the grid ``grid`` or seeded uniform rows in [-1, 1]^d.  Everything float32 on the host."""
    g = torch.Generator().manual_seed(seed)
    fin = 2 * m if m else d
    sizes = [(hidden, fin)] + [(hidden, hidden)] * hidden_layers + [(1, hidden)]
    weights = []
    for l, (fo, fi) in enumerate(sizes):
        bound = 1.0 / fi if l == 0 else math.sqrt(6.0 / fi) / OMEGA
        W = (torch.rand(fo, fi, generator=g) * 2 - 1) * bound
        b = (torch.rand(fo, generator=g) * 2 - 1) / math.sqrt(fi)
        weights.append((W.contiguous(), b.contiguous()))
    B = (torch.randn(m, d, generator=g) * scale).contiguous() if m else None
    x = mgrid_rows(grid) if grid is not None else (torch.rand(ROWS, d, generator=g) * 2 - 1).contiguous()
    assert x.shape == (ROWS, d)
    return {"d": d, "hidden": hidden, "hidden_layers": hidden_layers, "m": m, "in_features": fin, "weights": weights, "B": B, "x": x,
            "grid": grid}


CASES = {
    "a": dict(seed=11, d=2, hidden=64, hidden_layers=3, m=0, grid=(31, 33)),      # VALU first layer, J = 4
    "b": dict(seed=12, d=3, hidden=64, hidden_layers=2, m=16, grid=(11, 31, 3)),  # J = 5
    "c": dict(seed=13, d=4, hidden=128, hidden_layers=3, m=128),                  # J = 6, several K steps
    "d": dict(seed=14, d=3, hidden=512, hidden_layers=3, m=16),                   # several column tiles, K = 512
    "e": dict(seed=15, d=1, hidden=96, hidden_layers=1, m=0, grid=(1023,)),       # H no multiple of the 64-column tile; d = 1
}


def features(x, B):
    """INRmodel.py:171-176 ``input_mapping``."""
    if B is None:
        return x
    p = 2.0 * math.pi * x @ B.T
    return torch.cat([torch.sin(p), torch.cos(p)], dim=-1)


def network(weights, x, B, omega=OMEGA):
    a = features(x, B)
    for W, b in weights[:-1]:
        a = torch.sin(omega * (a @ W.T + b))
    W, b = weights[-1]
    return (a @ W.T + b)[:, 0]


def autograd_reference(case, d_tangent=None):
    """(y [n], grad [n, dt], lap [n]) in float64: gradient by one backward pass with create_graph=True, Laplacian by a second
    through each tangent component (rows are independent, so summing over rows before differentiating loses nothing)."""
    dt = case["d"] if d_tangent is None else d_tangent
    weights = [(W.double(), b.double()) for W, b in case["weights"]]
    B = None if case["B"] is None else case["B"].double()
    x = case["x"].double().requires_grad_(True)
    y = network(weights, x, B)
    g = torch.autograd.grad(y.sum(), x, create_graph=True)[0]
    lap = torch.zeros_like(y)
    for i in range(dt):
        lap = lap + torch.autograd.grad(g[:, i].sum(), x, retain_graph=True)[0][:, i]
    return y.detach(), g[:, :dt].detach(), lap.detach()


def forward_jet(case, dtype, d_tangent=None, omega=OMEGA):
    """The forward-mode formulas in plain torch on the host in ``dtype``: value a, tangents t_i, Laplacian
    accumulator q carried layer by layer.  In float64 it equals ``autograd_reference`` to rounding; its float32 deviation from
    float64 is the error plain float32 arithmetic makes on these formulas, which the Laplacian's tolerance is a multiple of."""
    dt = case["d"] if d_tangent is None else d_tangent
    x = case["x"].to(dtype)
    if case["B"] is None:
        a = x
        t = [torch.zeros_like(x) for _ in range(dt)]
        for i in range(dt):
            t[i][:, i] = 1
        q = torch.zeros_like(x)
    else:
        B = case["B"].to(dtype)
        p = 2.0 * math.pi * x @ B.T
        s, c = torch.sin(p), torch.cos(p)
        a = torch.cat([s, c], dim=-1)
        t = [torch.cat([2.0 * math.pi * B[:, i] * c, -2.0 * math.pi * B[:, i] * s], dim=-1) for i in range(dt)]
        nb = (2.0 * math.pi) ** 2 * (B[:, :dt] ** 2).sum(dim=1)
        q = torch.cat([-nb * s, -nb * c], dim=-1)
    for W, b in case["weights"][:-1]:
        W, b = W.to(dtype), b.to(dtype)
        z = a @ W.T + b
        u = [ti @ W.T for ti in t]
        r = q @ W.T
        s, c = torch.sin(omega * z), torch.cos(omega * z)
        su = sum(ui * ui for ui in u)
        a, t, q = s, [omega * c * ui for ui in u], omega * c * r - omega * omega * s * su
    W, b = case["weights"][-1]
    W, b = W.to(dtype), b.to(dtype)
    return (a @ W.T + b)[:, 0], torch.stack([(ti @ W.T)[:, 0] for ti in t], dim=-1), (q @ W.T)[:, 0]


def rel_l2(got, want):
    got, want = torch.as_tensor(got).double().cpu().reshape(-1), torch.as_tensor(want).double().cpu().reshape(-1)
    return float((got - want).norm() / want.norm())


def max_rel(got, want):
    got, want = torch.as_tensor(got).double().cpu().reshape(-1), torch.as_tensor(want).double().cpu().reshape(-1)
    return float((got - want).abs().max() / want.abs().max())


def on_device(case):
    """(desc, flat parameter buffer, x, B) on the GPU, laid out by inr_siren_param_offsets."""
    from mri_super_resolution_amd import ops
    desc = ops.make_desc(case["in_features"], case["hidden"], case["hidden_layers"], 1, OMEGA, OMEGA)
    total, offsets = ops.siren_param_layout(desc)
    flat = torch.zeros(total, dtype=torch.float32)
    for (w_off, b_off), (W, b) in zip(offsets, case["weights"]):
        flat[w_off:w_off + W.numel()] = W.reshape(-1)
        flat[b_off:b_off + b.numel()] = b
    B = None if case["B"] is None else case["B"].cuda()
    return desc, flat.cuda(), case["x"].cuda(), B
