"""Float64 restatement of the PIA autoencoder, written from the reference's behaviour (PIA.py:97-155) for the tests.

`forward64(params, x)` takes the 22 parameter tensors (any float dtype, `named_parameters()` order) and a batch, and
evaluates encoder, heads, encode and decode in float64 -- with the ONE float32 step the reference keeps even in a float64
model: `decode` sums the three compartments in float64, stores the sum into a float32 tensor and scales that by 1000
(PIA.py:120-130).  `loss_and_grads64` adds the unsupervised loss `mean(PIDS * (signal - x) ** 2)` and its gradients by
autograd.  tests/test_pia_net_cpu.py pins this file to the reference's own float64 run (tests/golden/pia_net.npz, 1e-12);
the GPU tests then compare the kernels against it at any batch size.
"""
import hashlib

import numpy as np
import torch

B_VALUES = (0, 150, 1000, 1500)
TE_VALUES = (0, 13, 93, 143)
D_MEAN, D_DELTA = (0.5, 1.2, 2.85), (0.2, 0.5, 0.15)
T2_MEAN, T2_DELTA = (45.0, 70.0, 750.0), (25.0, 30.0, 250.0)
HIDDEN = (32, 64, 128, 256, 512)
SLOPE = 0.01
PARAM_NAMES = [f"encoder.{l}.0.{k}" for l in range(5) for k in ("weight", "bias")] + \
    [f"{h}_predictor.{m}.{k}" for h in ("D", "T2", "v") for m in ("0.0", "1") for k in ("weight", "bias")]
PARAM_SHAPES = [s for l, (i, o) in enumerate(zip((16,) + HIDDEN[:-1], HIDDEN)) for s in ((o, i), (o,))] + \
    [s for _ in range(3) for s in ((512, 512), (512,), (3, 512), (3,))]
PARAM_COUNT = 968169
SMALL_HIDDEN = [32, 64, 128, 256]     # a non-default shape of the fixture: four encoder layers, 256-wide heads, its first SMALL_ROWS rows
SMALL_ROWS = 200


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sample(a, k=97):
    """The fixture's sampling rule (oracle/gen_golden.py): tensors of <= 512 elements whole, else every k-th element."""
    flat = np.asarray(a).reshape(-1)
    return flat if flat.size <= 512 else flat[::k]


def pids_map(n=512, seed=7):
    """The seeded, non-trivial PIDS weight map of the fixture: mostly ones, a quarter down-weighted, a tenth switched off."""
    rng = np.random.default_rng(seed)
    u = rng.random((n, 16))
    w = np.ones((n, 16), dtype=np.float32)
    w[u < 0.25] = 0.5
    w[u < 0.10] = 0.0
    return w


def leaky(z):
    return torch.where(z > 0, z, SLOPE * z)


def forward64(params, x, dtype=torch.float64, b_values=B_VALUES, te_values=TE_VALUES):
    """-> signal (float64 values of the float32-rounded decoder output), D, T2, v (float64).  `dtype=torch.float32` runs the
    layers in float32 instead (a diagnostic: how far plain float32 arithmetic is from float64 on a given batch).
    `b_values` / `te_values` are the acquisition tables (n_b * n_te == 16), b-major as PIA.py:123-124 walks them."""
    p = [t.to(dtype) for t in params]
    a = x.to(dtype)
    L = (len(p) - 12) // 2                        # encoder layers (5 for the default shape); predictor_depth 1
    for l in range(L):
        a = leaky(a @ p[2 * l].T + p[2 * l + 1])
    heads = []
    for j in range(3):
        w1, b1, w2, b2 = p[2 * L + 4 * j: 2 * L + 4 + 4 * j]
        heads.append(leaky(a @ w1.T + b1) @ w2.T + b2)
    dm, dd = torch.tensor(D_MEAN, dtype=torch.float64), torch.tensor(D_DELTA, dtype=torch.float64)
    tm, td = torch.tensor(T2_MEAN, dtype=torch.float64), torch.tensor(T2_DELTA, dtype=torch.float64)
    D = dm + dd * torch.tanh(heads[0]).double()
    T2 = tm + td * torch.tanh(heads[1]).double()
    v = torch.softmax(heads[2], dim=1).double()
    nb = torch.tensor([-b / 1000 for b in b_values for _ in te_values], dtype=torch.float64)
    te = torch.tensor([float(t) for _ in b_values for t in te_values], dtype=torch.float64)
    S = sum(v[:, c:c + 1] * torch.exp(nb[None, :] * D[:, c:c + 1]) * torch.exp(-te[None, :] / T2[:, c:c + 1]) for c in range(3))
    signal = (1000 * S.float()).double()          # the float32 tensor `decode` writes into
    return signal, D.double(), T2.double(), v.double()


def loss_and_grads64(params, x, pids, dtype=torch.float64, b_values=B_VALUES, te_values=TE_VALUES, functional=None):
    """Unsupervised loss (float64) and its gradients, one per parameter tensor, for float64 leaf copies of `params`.
    `functional(signal, D, T2, v) -> scalar` replaces the unsupervised loss when given (`pids` is then unused); a parameter
    the functional does not reach gets a zero gradient, which is what the backward kernels write for it."""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in params]
    signal, D, T2, v = forward64(leaves, x, dtype, b_values, te_values)
    if functional is None:
        loss = torch.mean(torch.as_tensor(pids).double() * (signal - x.double()) ** 2)
        grads = torch.autograd.grad(loss, leaves)
    else:
        loss = functional(signal, D, T2, v)
        grads = [torch.zeros_like(t) if g is None else g for g, t in zip(torch.autograd.grad(loss, leaves, allow_unused=True), leaves)]
    return loss.detach(), [g.detach() for g in grads], (signal.detach(), D.detach(), T2.detach(), v.detach())


KINK_EPS = 2.0 ** -18


def kink_rows(params, x, eps=KINK_EPS, b_values=B_VALUES, te_values=TE_VALUES):
    """(`b_values` / `te_values` are accepted for a uniform call signature and unused: every LeakyReLU lies below the decoder.)
    Rows of `x` on which the gradient is not defined at float32 resolution, judged by float64 alone.

    LeakyReLU has a kink at zero.  A pre-activation z = sum_k a_k w_k + b evaluated in float32 carries an error of up to
    K u sum_k |a_k w_k| (u = 2^-24, K <= 512 terms; about sqrt(K) u = 23 u when the roundings behave like a random walk), plus
    a few u per term from the float32 activations it is fed.  Where the float64 value satisfies |z| <= eps (sum_k |a_k w_k| + |b|)
    with eps = 64 u = 2^-18, a float32 evaluation -- the kernels', torch's, the reference's own -- may land on either side of
    zero, and the unit's derivative is then 1 or 0.01 by the luck of a summation order: on one such row (|z| = 1.5e-9 of the
    scale) the same float32 torch code gave both answers on two CPUs.  Such rows have no float64 "expected" gradient that a
    float32 implementation could be held to, so a gradient comparison leaves them out.  Returns a bool vector [rows]."""
    p = [t.double() for t in params]
    a = x.double()
    bad = torch.zeros(x.shape[0], dtype=torch.bool)

    def layer(a, w, b):
        z = a @ w.T + b
        scale = a.abs() @ w.abs().T + b.abs()
        return z, (z.abs() <= eps * scale).any(dim=1)

    L = (len(p) - 12) // 2
    for l in range(L):
        z, amb = layer(a, p[2 * l], p[2 * l + 1])
        bad |= amb
        a = leaky(z)
    for j in range(3):
        _, amb = layer(a, p[2 * L + 4 * j], p[2 * L + 1 + 4 * j])
        bad |= amb
    return bad


def rel_dev(a, ref):
    """max |a - ref| / max |ref|: the deviation measure of the fixture's `ref_err/*` entries."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))


def pids_slice_input(seed=3):
    """The seeded S [12, 12, 4 (b), 4 (TE)] of the fixture, in the reference's units (signals of order 1000): noisy
    three-compartment decays, with planted ties, neighbours just below / above an integer, and decays that do not hold."""
    rng = np.random.default_rng(seed)
    n = 144
    D = np.column_stack([rng.uniform(0.3, 0.7, n), rng.uniform(0.7, 1.7, n), rng.uniform(2.7, 3.0, n)])
    T2 = np.column_stack([rng.uniform(20, 70, n), rng.uniform(40, 100, n), rng.uniform(500, 1000, n)])
    v = rng.uniform(0.05, 1, (n, 3))
    v /= v.sum(axis=1, keepdims=True)
    b = np.array(B_VALUES, dtype=np.float64)[None, :, None, None]
    te = np.array(TE_VALUES, dtype=np.float64)[None, None, :, None]
    S = 1000 * (v[:, None, None, :] * np.exp(-b / 1000 * D[:, None, None, :]) * np.exp(-te / T2[:, None, None, :])).sum(-1)
    S = S + rng.normal(0, 15.0, S.shape)
    S = np.maximum(S, 0.5)                       # the logarithm of the ADC fit wants positive signals
    S[0:12, 1, 2] = S[0:12, 1, 1]                # ties along TE at b index 1
    S[12:24, 2, 3] = S[12:24, 1, 3]              # ties along b at TE index 3
    S[24:36, 0, 1] = np.floor(S[24:36, 0, 1]) + 0.999    # left neighbour just below an integer ...
    S[24:36, 0, 2] = np.floor(S[24:36, 0, 1]) + 0.5      # ... the value falls, yet stays above the truncated neighbour
    S[36:48, 2, 0] = np.floor(S[36:48, 2, 0]) + 1e-9     # left neighbour just above an integer
    S[36:48, 2, 1] = np.floor(S[36:48, 2, 0]) - 1e-9     # ... the value is just below it
    for k in (1, 2, 3):
        S[48:60, k, 0] = S[48:60, 0, 0] * (1 + 0.1 * k)    # signal rising with b: negative ADC
    S[60:72, 3, 0] = S[60:72, 0, 0] * 1e-3       # very steep decay: ADC above 3
    S[60:72, 2, 0] = S[60:72, 0, 0] * 2e-2
    S[60:72, 1, 0] = S[60:72, 0, 0] * 0.5
    return S.reshape(12, 12, 4, 4)
