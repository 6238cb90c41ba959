"""Float64 restatement, in REAL arithmetic (numpy), of the WIRE network's gradient with respect to its input and of the
PerturbNet phase of wiretest.ipynb cell 10 built on it: PN -> input_mapping -> WIRE -> MSE, the PerturbNet's gradients by
hand, torch's Adam on them, and the loop's odd / even epochs.  Shared by test_wire_pn_cpu.py and test_gpu_wire_pn.py;
tests/golden/wire_pn.npz (tools/make_wire_pn_golden.py: the reference's own layer, PN and input_mapping under complex128 /
float64 autograd) pins it, and larger shapes are checked against it.  The network's forward and parameter gradient are
tests/wire_common.py's.

PerturbNet parameters travel as a dict under its state_dict names."""
import os

import numpy as np

import wire_common as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wire_pn.npz")
PN_KEYS = ["perturb_linear.weight", "perturb_linear.bias", "perturb_linear2.weight", "perturb_linear2.bias"]


def golden():
    return np.load(GOLDEN)


def pn_leaves(g):
    return {k[3:]: g[k].astype(np.float64) for k in g.files if k.startswith("pn/")}


def input_grad64(P, x, gy, L):
    """(y [n], dx [n, in]) with dx = d(sum gy y)/dx: the backward of wire_common.loss_grad64, carried on through layer 0."""
    stash = []
    y = C.forward64(P, x, L, stash)
    stash.pop()
    hw = P["final_linear.weight"]
    gy = np.asarray(gy, np.float64)
    Gr, Gi = np.outer(gy, hw[0, :, 0]), -np.outer(gy, hw[0, :, 1])
    for k in range(L, -1, -1):
        _, _, lin_r, lin_i, orth_r, orth_i, out_r, out_i = stash[k]
        w, s2 = C._consts(P, k)
        Pm = Gr * out_r + Gi * out_i
        Qm = Gi * out_r - Gr * out_i
        d = {"linear": (-2 * s2 * lin_r * Pm + w * Qm, -(w + 2 * s2 * lin_i) * Pm),
             "scale_orth": (-2 * s2 * orth_r * Pm, -2 * s2 * orth_i * Pm)}
        dhr = dhi = 0.0
        for name, (dr, di) in d.items():
            W = P[f"net.{k}.{name}.weight"]
            if k == 0:
                dhr = dhr + dr @ W                      # real weights, real input: the imaginary planes end here
                continue
            Wr, Wi = W[..., 0], W[..., 1]
            dhr = dhr + dr @ Wr + di @ Wi
            dhi = dhi + di @ Wr - dr @ Wi
        Gr, Gi = dhr, dhi
    return y, Gr


def acq_value(sample):
    """``torch.tensor([sample / 10.], dtype=torch.float)``: a float32 VALUE."""
    return float(np.float32(sample / 10.))


def pn_forward64(Q, x, sample, eps):
    """(eps tanh(W2 tanh(W1 [x | sample / 10] + b1) + b2), what the backward needs)."""
    xa = np.concatenate([np.asarray(x, np.float64), np.full((x.shape[0], 1), acq_value(sample))], 1)
    h = np.tanh(xa @ Q["perturb_linear.weight"].T + Q["perturb_linear.bias"])
    t = np.tanh(h @ Q["perturb_linear2.weight"].T + Q["perturb_linear2.bias"])
    return eps * t, (xa, h, t)


def pn_backward64(Q, saved, g, eps):
    xa, h, t = saved
    dz2 = g * eps * (1 - t * t)
    dz1 = (dz2 @ Q["perturb_linear2.weight"]) * (1 - h * h)
    return {"perturb_linear.weight": dz1.T @ xa, "perturb_linear.bias": dz1.sum(0), "perturb_linear2.weight": dz2.T @ h,
            "perturb_linear2.bias": dz2.sum(0)}


def fourier64(x, B):
    p = (2.0 * np.pi * x) @ np.asarray(B, np.float64).T
    return np.concatenate([np.sin(p), np.cos(p)], -1)


def fourier_backward64(feats, B, g):
    m = B.shape[0]
    s, c = feats[:, :m], feats[:, m:]
    return 2.0 * np.pi * ((g[:, :m] * c - g[:, m:] * s) @ np.asarray(B, np.float64))


def pn_step64(P, Q, x, B, sample, eps, target, L):
    """Loss and the PerturbNet's four gradients of ``((INR(input_mapping(PN(x, sample, eps), B)) - target)**2).mean()``."""
    pert, saved = pn_forward64(Q, x, sample, eps)
    feats = fourier64(pert, B)
    y = C.forward64(P, feats, L)
    n = y.shape[0]
    loss = float(np.mean((y - target) ** 2))
    _, dfeats = input_grad64(P, feats, 2.0 * (y - target) / n, L)
    return loss, pn_backward64(Q, saved, fourier_backward64(feats, B, dfeats), eps)


class Adam64:
    """torch.optim.Adam on a dict of real arrays (complex tensors as their pairs), updated in place."""

    def __init__(self, keys, like, lr, b1=0.9, b2=0.999, eps=1e-8):
        self.keys, self.lr, self.b1, self.b2, self.eps, self.t = list(keys), lr, b1, b2, eps, 0
        self.m = {k: np.zeros_like(like[k]) for k in self.keys}
        self.v = {k: np.zeros_like(like[k]) for k in self.keys}

    def step(self, P, G):
        self.t += 1
        for k in self.keys:
            self.m[k] = self.b1 * self.m[k] + (1 - self.b1) * G[k]
            self.v[k] = self.b2 * self.v[k] + (1 - self.b2) * G[k] ** 2
            P[k] = P[k] - self.lr / (1 - self.b1 ** self.t) * self.m[k] / (np.sqrt(self.v[k]) / np.sqrt(1 - self.b2 ** self.t) + self.eps)


def schedule64(P, Q, x, B, eps, mean_target, acq_targets, L, number_of_epochs, pertubation_epochs, lr=5e-5, perturb_lr=1e-6):
    """wiretest.ipynb cell 10: (INR losses, PerturbNet losses, the PerturbNet's Adam first moments).  P and Q are updated in place."""
    inr_adam, pn_adam = Adam64(C.param_keys(L), P, lr), Adam64(PN_KEYS, Q, perturb_lr)
    inr_losses, pn_losses = [], []
    for ctr in range(number_of_epochs):
        if ctr < number_of_epochs - pertubation_epochs or ctr % 2:
            _, loss, G = C.loss_grad64(P, x, mean_target, L)
            inr_adam.step(P, G)
            inr_losses.append(loss)
        else:
            for sample in range(len(acq_targets)):
                loss, G = pn_step64(P, Q, x, B, sample, eps, acq_targets[sample], L)
                pn_adam.step(Q, G)
                pn_losses.append(loss)
    return np.asarray(inr_losses), np.asarray(pn_losses), pn_adam.m


def epoch_branches(number_of_epochs, pertubation_epochs):
    """Cell 10's branch per epoch, stated on its own: 'inr' or 'pn'."""
    return ["inr" if ctr < number_of_epochs - pertubation_epochs or ctr % 2 else "pn" for ctr in range(number_of_epochs)]
