"""Float64 restatement of the WIRE complex-Gabor network in REAL arithmetic (numpy), shared by test_wire_cpu.py and
test_gpu_wire.py: forward, loss and hand-written backward of DESIGN.md 4e, and torch's Adam on the parameters' real views.
tests/golden/wire_inrmodel.npz (tools/make_wire_golden.py: the reference's own layer under complex128 autograd) pins it; larger
shapes are checked against it.

Parameters travel as a dict under the module's state_dict names; a complex tensor is its (re, im) pairs ``[..., 2]``."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wire_inrmodel.npz")
OMEGA = SCALE = 1.2          # wiretest.ipynb cell 7


def golden():
    return np.load(GOLDEN)


def layer_keys(k):
    return [f"net.{k}.linear.weight", f"net.{k}.linear.bias", f"net.{k}.scale_orth.weight", f"net.{k}.scale_orth.bias"]


def param_keys(L):
    """Trainable tensors in the kernels' flat order."""
    return [key for k in range(L + 1) for key in layer_keys(k)] + ["final_linear.weight", "final_linear.bias"]


def leaves64(model):
    """{state_dict name: float64 array} of a module's tensors (complex ones as pairs), omega_0 / scale_0 included."""
    out = {}
    for k, v in model.state_dict().items():
        v = v.detach().cpu()
        out[k] = (torch.view_as_real(v) if v.is_complex() else v).numpy().astype(np.float64)
    return out


def golden_leaves(g):
    return {k[2:]: g[k].astype(np.float64) for k in g.files if k.startswith("w/")}


def _consts(P, k):
    """omega_0 and scale_0^2 of layer k: float32 VALUES, double arithmetic."""
    w, s = float(P[f"net.{k}.omega_0"][0]), float(P[f"net.{k}.scale_0"][0])
    return w, s * s


def _affine(hr, hi, W, b, first):
    if first:
        return hr @ W.T + b, None
    Wr, Wi = W[..., 0], W[..., 1]
    return hr @ Wr.T - hi @ Wi.T + b[:, 0], hr @ Wi.T + hi @ Wr.T + b[:, 1]


def forward64(P, x, L, stash=None):
    """y [n] of rows x [n, in]; ``stash`` (a list) receives per layer (hr, hi, lin_r, lin_i, orth_r, orth_i, out_r, out_i)."""
    hr, hi = np.asarray(x, np.float64), None
    for k in range(L + 1):
        lw, lb, ow, ob = (P[key] for key in layer_keys(k))
        w, s2 = _consts(P, k)
        lin_r, lin_i = _affine(hr, hi, lw, lb, k == 0)
        orth_r, orth_i = _affine(hr, hi, ow, ob, k == 0)
        if k == 0:
            lin_i, orth_i = np.zeros_like(lin_r), np.zeros_like(lin_r)
        A = np.exp(-w * lin_i - s2 * (lin_r ** 2 + lin_i ** 2 + orth_r ** 2 + orth_i ** 2))      # ONE exponential
        out_r, out_i = A * np.cos(w * lin_r), A * np.sin(w * lin_r)
        if stash is not None:
            stash.append((hr, hi, lin_r, lin_i, orth_r, orth_i, out_r, out_i))
        hr, hi = out_r, out_i
    hw, hb = P["final_linear.weight"], P["final_linear.bias"]
    y = hr @ hw[0, :, 0] - hi @ hw[0, :, 1] + hb[0, 0]
    if stash is not None:
        stash.append((hr, hi))
    return y


def loss_grad64(P, x, target, L, weight=None):
    """(y, loss, {name: gradient}) of mean(w (y - t)^2), torch's convention for complex tensors: grad = dL/dRe + i dL/dIm."""
    stash = []
    y = forward64(P, x, L, stash)
    n = y.shape[0]
    wgt = np.ones(n) if weight is None else np.asarray(weight, np.float64)
    loss = float(np.mean(wgt * (y - target) ** 2))
    gy = 2.0 * wgt * (y - target) / n
    G = {}
    hr, hi = stash.pop()
    hw = P["final_linear.weight"]
    G["final_linear.weight"] = np.stack([gy @ hr, -(gy @ hi)], -1)[None]
    G["final_linear.bias"] = np.array([[gy.sum(), 0.0]])
    Gr, Gi = np.outer(gy, hw[0, :, 0]), -np.outer(gy, hw[0, :, 1])
    for k in range(L, -1, -1):
        hr, hi, lin_r, lin_i, orth_r, orth_i, out_r, out_i = stash[k]
        w, s2 = _consts(P, k)
        Pm = Gr * out_r + Gi * out_i
        Qm = Gi * out_r - Gr * out_i
        d = {"linear": (-2 * s2 * lin_r * Pm + w * Qm, -(w + 2 * s2 * lin_i) * Pm),
             "scale_orth": (-2 * s2 * orth_r * Pm, -2 * s2 * orth_i * Pm)}
        dhr = dhi = 0.0
        for name, (dr, di) in d.items():
            W = P[f"net.{k}.{name}.weight"]
            if k == 0:
                G[f"net.0.{name}.weight"] = dr.T @ hr
                G[f"net.0.{name}.bias"] = dr.sum(0)
                continue
            G[f"net.{k}.{name}.weight"] = np.stack([dr.T @ hr + di.T @ hi, di.T @ hr - dr.T @ hi], -1)
            G[f"net.{k}.{name}.bias"] = np.stack([dr.sum(0), di.sum(0)], -1)
            Wr, Wi = W[..., 0], W[..., 1]
            dhr = dhr + dr @ Wr + di @ Wi
            dhi = dhi + di @ Wr - dr @ Wi
        Gr, Gi = dhr, dhi
    return y, loss, G


def adam_fit64(P, x, target, L, steps, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam on every trainable tensor's reals; returns (per-step losses, final y).  P is updated in place."""
    keys = param_keys(L)
    m = {k: np.zeros_like(P[k]) for k in keys}
    v = {k: np.zeros_like(P[k]) for k in keys}
    losses = []
    for step in range(1, steps + 1):
        _, loss, G = loss_grad64(P, x, target, L)
        losses.append(loss)
        for k in keys:
            m[k] = b1 * m[k] + (1 - b1) * G[k]
            v[k] = b2 * v[k] + (1 - b2) * G[k] ** 2
            P[k] = P[k] - lr / (1 - b1 ** step) * m[k] / (np.sqrt(v[k]) / np.sqrt(1 - b2 ** step) + eps)
    return np.asarray(losses), forward64(P, x, L)


def rel_l2(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def make_case(Wire, n, in_features, hidden, layers, seed, weighted=False, raw=False):
    """(model on the CPU, x [n, in] float32, target [n] float32, weight or None): omega_0 = scale_0 = 1.2 as in the notebook;
    inputs are Fourier features of random coordinates (raw: the coordinates themselves), targets uniform in [0, 1]."""
    torch.manual_seed(seed)
    model = Wire(in_features, hidden, layers, 1, first_omega_0=OMEGA, hidden_omega_0=OMEGA, scale=SCALE)
    g = torch.Generator().manual_seed(seed + 1000)
    if raw:
        x = torch.rand(n, in_features, generator=g) * 2 - 1
    else:
        half = in_features // 2
        proj = 2 * np.pi * (torch.rand(n, 3, generator=g) * 2 - 1) @ (torch.randn(half, 3, generator=g) * 0.5).T
        x = torch.cat([torch.sin(proj), torch.cos(proj)], -1)
    target = torch.rand(n, generator=g)
    weight = (0.5 + torch.rand(n, generator=g)) if weighted else None
    return model, x.float().contiguous(), target, weight
