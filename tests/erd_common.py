"""Float64 restatement of the soft-ERD INR family (ErdSiren and soft-ERD), written from the behaviour the project documents --
NOT from the reference's program text.  ``INR_ERD.py`` cannot be imported for a check (its ``nn_mri`` needs torchvision, PIL and
SimpleITK), so this family is pinned to this restatement, not to a run of the reference.

Model: trunk ``sin(omega (h W^T + b))`` for the first sine layer and ``hidden_layers`` more, then ``relu(h W^T + b)``; head
``relu(h w^T + b)``.  With ``perturb``: ``u = tanh([x, sample] W1^T + b1)``, ``p = eps tanh(u W2^T + b2)`` ([N, 1]) and the trunk
sees ``x + p`` (p added to every component).  Coordinates carry no gradient."""
import numpy as np
import torch

GRID = (31, 33)            # 1,023 rows: the last 32-row wave is ragged
K_ACQ = 3
EPS = 1.0 / 128.0
# seeds per (hidden_features, hidden_layers): chosen on the CPU, from the restatement alone, so that (a) at most 5 % of the rows
# lie within 1e-4 of a ReLU kink and (b) the case is well conditioned for float32 at all: the restatement run in plain float32
# lands within 3e-6 (a third of tier T2) of float64 on every gradient tensor.  Of seeds 0..7, several fail (b) by an order of
# magnitude -- the perturb-branch bias gradients are sums over the image that nearly cancel (seed 0 at 64 x 3: 4.2e-5 in
# plain float32 torch).  tests/test_erd_inr_cpu.py asserts (a) and (b).
SEEDS = {(64, 1): 4, (64, 3): 7, (128, 1): 6, (128, 3): 5}
F32_CONDITION = 3e-6


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def leaves64(model):
    """state_dict -> float64 leaf tensors (values of the float32 parameters)."""
    return {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}


def forward64(P, x, hidden_layers, sample=0, eps=0.0, perturb=False, first_omega=30.0, hidden_omega=30.0, dtype=torch.float64):
    """-> (y [N, 1], [ReLU-layer pre-activation, head pre-activation]).  ``dtype=torch.float32`` runs the same expressions in
    float32 (how far plain float32 arithmetic lands from float64 on a case)."""
    x = x.detach().to(dtype)
    P = {k: v.to(dtype) for k, v in P.items()}
    h = x
    if perturb:
        inp = torch.cat([x, torch.full((x.shape[0], 1), float(int(sample)), dtype=dtype)], dim=-1)
        u = torch.tanh(inp @ P["perturb_linear.weight"].T + P["perturb_linear.bias"])
        p = eps * torch.tanh(u @ P["perturb_linear2.weight"].T + P["perturb_linear2.bias"])
        h = x + p
    for k in range(hidden_layers + 1):
        omega = first_omega if k == 0 else hidden_omega
        h = torch.sin(omega * (h @ P[f"net.{k}.linear.weight"].T + P[f"net.{k}.linear.bias"]))
    z = h @ P[f"net.{hidden_layers + 1}.weight"].T + P[f"net.{hidden_layers + 1}.bias"]
    zh = torch.relu(z) @ P["final_linear.weight"].T + P["final_linear.bias"]
    return torch.relu(zh), [z, zh]


def kink_rows(pres, tol=1e-4):
    """Rows where any ReLU pre-activation lies within ``tol`` of that layer's largest absolute pre-activation from zero."""
    bad = torch.zeros(pres[0].shape[0], dtype=torch.bool)
    for z in pres:
        z = z.detach()
        bad |= (z.abs() < tol * z.abs().max()).any(dim=1)
    return bad


def loss64(P, x, target, weight, hidden_layers, sample, eps, perturb, dtype=torch.float64):
    y, pres = forward64(P, x, hidden_layers, sample, eps, perturb, dtype=dtype)
    return (weight.to(dtype).reshape(-1, 1) * (y - target.to(dtype).reshape(-1, 1)) ** 2).mean(), y, pres


def float32_gradient_error(P, x, targets, weights, hidden_layers, keys):
    """Largest per-tensor rel-L2 distance between the restatement's float32 and float64 autograd gradients over the acquisitions:
    how well plain float32 arithmetic is conditioned on this case."""
    return max(max(e) for e in float32_gradient_errors(P, x, targets, weights, hidden_layers, keys))


def float32_gradient_errors(P, x, targets, weights, hidden_layers, keys):
    """Per acquisition, per tensor of ``keys``: rel-L2 of the restatement's float32 gradient against its float64 one."""
    out = []
    for s in range(targets.shape[0]):
        g = {}
        for dt in (torch.float64, torch.float32):
            loss, _, _ = loss64(P, x, targets[s], weights[s], hidden_layers, s, EPS, True, dtype=dt)
            g[dt] = torch.autograd.grad(loss, [P[k] for k in keys])
        out.append([rel_l2(a.numpy(), b.numpy()) for a, b in zip(g[torch.float32], g[torch.float64])])
    return out


def grid_coords(shape=GRID):
    axes = [torch.linspace(-1, 1, s) for s in shape]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, len(shape)).float()


def make_case(model_cls, hidden, layers, perturb_scale=8.0, seed=None):
    """Model (CPU, float32 init from the pinned seed), coordinates, K targets and K positive weights.  The perturb layers'
    weights are scaled up so that the perturbation is not negligible beside the coordinate spacing."""
    torch.manual_seed(SEEDS[(hidden, layers)] if seed is None else seed)
    model = model_cls(2, hidden, layers, perturb=True)
    with torch.no_grad():
        model.perturb_linear.weight.mul_(perturb_scale)
        model.perturb_linear2.weight.mul_(perturb_scale)
        model.final_linear.bias.fill_(0.05)        # keeps a fair share of the ReLU head active at initialisation
    g = torch.Generator().manual_seed(100 + hidden + layers)
    x = grid_coords()
    targets = torch.rand(K_ACQ, x.shape[0], generator=g)
    weights = 0.5 + torch.rand(K_ACQ, x.shape[0], generator=g)
    return model, x, targets, weights


def masked_weights(P, x, weights, layers, perturb=True):
    """Weights with the kink rows of every acquisition set to 0 (they stay in the launch); returns (weights, masked fraction)."""
    out = weights.clone()
    frac = 0.0
    for s in range(weights.shape[0]):
        _, pres = forward64(P, x, layers, s, EPS, perturb)
        bad = kink_rows(pres)
        out[s, bad] = 0.0
        frac = max(frac, float(bad.float().mean()))
    return out, frac


def soft_erd_np(values, b0, noise_level, mul=1000.0, slope=20.0, min_temp=2.0):
    """numpy float64: temp = max(mul exp(-slope mean / b0), min_temp); where mean > 2 noise: w = exp(x / temp) (unnormalised),
    mean image = softmax-weighted mean (maximum subtracted); elsewhere w = 1 / K, mean image = mean."""
    values = np.asarray(values, dtype=np.float64)
    b0 = np.asarray(b0, dtype=np.float64)
    K = values.shape[-1]
    w = np.full(values.shape, 1.0 / K)
    mean = values.mean(axis=-1)
    img = mean.copy()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        temp = np.maximum(mul * np.exp(-slope * (mean / b0)), min_temp)
        hi = mean > 2 * noise_level
        t = temp[..., None]
        e = np.exp((values - values.max(axis=-1, keepdims=True)) / t)
        soft = (e * values).sum(axis=-1) / e.sum(axis=-1)
        w = np.where(hi[..., None], np.exp(values / t), w)
        img = np.where(hi, soft, img)
    return w, img, temp


def soft_erd_fixture(n=1023, K=8, seed=3):
    """Pixels covering the three branches: low signal (mean <= 2 noise), temperature clamped at min_temp, temperature above it;
    plus b0 == 0 pixels."""
    rng = np.random.default_rng(seed)
    b0 = rng.uniform(200.0, 900.0, n)
    frac = rng.uniform(0.02, 0.6, n)                       # mean / b0: exp(-20 * .) spans clamped and unclamped temperatures
    values = (b0 * frac)[:, None] * rng.uniform(0.8, 1.2, (n, K))
    low = rng.random(n) < 0.2
    values[low] = rng.uniform(0.0, 8.0, (int(low.sum()), K))
    b0[::97] = 0.0
    return values, b0, 5.0
