"""The multi-stack 3-D TV / Huber reconstruction of csrc/tvms.hip restated in float64 NumPy: the stack operator A_s
with its validity rule, the adjoint, the step bound, the back-projection, the objective and the Chambolle-Pock iteration with both
terms dual.  One volume at a time: x [D][H][W]; a stack is the tuple (f [3], taps (k0, k1, k2), o [3], n [3]) and its data are
[n0][n1][n2].  The differences, the divergence and the Huber function are tvsr3d_common's.  The tests compare the kernels with these
functions; nothing here imports the package."""
import functools

import numpy as np

from tests import tvsr3d_common as T3

diffs, div, huber, psnr, pat07_roi = T3.diffs, T3.div, T3.huber, T3.psnr, T3.pat07_roi


def stack(f, taps, o=(0, 0, 0), n=None, hr_shape=None):
    """(f, taps, o, n) with float64 taps; ``n`` defaults to ``default_shape``."""
    f, o = tuple(int(v) for v in f), tuple(int(v) for v in o)
    taps = tuple(np.asarray(k, np.float64) for k in taps)
    if n is None:
        n = default_shape(f, taps, o, hr_shape)
    return f, taps, o, tuple(int(v) for v in n)


def default_shape(f, taps, o, hr_shape):
    """Per axis max(1, floor((N - L - o) / f) + 1): the indices from 0 to the last whose footprint lies inside."""
    return tuple(max(1, (N - len(k) - oa) // fa + 1) for N, fa, k, oa in zip(hr_shape, f, taps, o))


def block_stack(factors, kernel, hr_shape):
    """The stack that is the block operator of tvsr3d_common: L = f, o = 0, n = N / f."""
    ks = T3.block_factors(kernel, factors)
    return stack(factors, ks, (0, 0, 0), tuple(N // f for N, f in zip(hr_shape, factors)))


def table(taps):
    """k[a][b][c] = (k1[b] * k2[c]) * k0[a]."""
    k0, k1, k2 = taps
    return (k1[None, :, None] * k2[None, None, :]) * k0[:, None, None]


def axis_valid(st, hr_shape):
    """Per axis the bool vector [n_a]: 0 <= o + f i and o + f i + L <= N."""
    f, taps, o, n = st
    out = []
    for a in range(3):
        start = o[a] + f[a] * np.arange(n[a])
        out.append((start >= 0) & (start + len(taps[a]) <= hr_shape[a]))
    return out


def valid_mask(st, hr_shape):
    v0, v1, v2 = axis_valid(st, hr_shape)
    return v0[:, None, None] & v1[None, :, None] & v2[None, None, :]


def _starts(st, hr_shape):
    f, _, o, _ = st
    return [o[a] + f[a] * np.flatnonzero(v) for a, v in enumerate(axis_valid(st, hr_shape))]


def apply(x, st):
    """A_s x [n0][n1][n2], 0 at invalid data; the terms in ascending (a, b, c)."""
    k = table(st[1])
    v = axis_valid(st, x.shape)
    s0, s1, s2 = _starts(st, x.shape)
    acc = np.zeros((len(s0), len(s1), len(s2)))
    for a in range(k.shape[0]):
        for b in range(k.shape[1]):
            for c in range(k.shape[2]):
                acc += k[a, b, c] * x[np.ix_(s0 + a, s1 + b, s2 + c)]
    out = np.zeros(st[3])
    out[np.ix_(*v)] = acc
    return out


def adjoint(r, st, hr_shape):
    """A_s^T r [D][H][W]: k[a][b][c] r[l][i][j] of every valid datum lands on voxel (o0 + f0 l + a, o1 + f1 i + b, o2 + f2 j + c)."""
    k = table(st[1])
    v = axis_valid(st, hr_shape)
    s0, s1, s2 = _starts(st, hr_shape)
    rv = np.asarray(r, np.float64)[np.ix_(*v)]
    out = np.zeros(hr_shape)
    for a in range(k.shape[0]):
        for b in range(k.shape[1]):
            for c in range(k.shape[2]):
                out[np.ix_(s0 + a, s1 + b, s2 + c)] += k[a, b, c] * rv
    return out


def apply_all(x, stacks):
    return [apply(x, st) for st in stacks]


def adjoint_all(rs, stacks, hr_shape):
    out = np.zeros(hr_shape)
    for r, st in zip(rs, stacks):
        out = out + adjoint(r, st, hr_shape)
    return out


def stack_bound(st):
    """c_s = prod_a (sum_t |k_a[t]|) (max_{r < f_a} sum_{t = r mod f_a} |k_a[t]|), the axes in the order 0, 1, 2, every sum ascending."""
    f, taps, _, _ = st
    c = 1.0
    for a in range(3):
        l1 = 0.0
        for v in taps[a]:
            l1 += abs(float(v))
        top = 0.0
        for r in range(f[a]):
            cls = 0.0
            for v in taps[a][r::f[a]]:
                cls += abs(float(v))
            top = max(top, cls)
        c = c * (l1 * top)
    return c


def step(stacks, hr_shape, g, lam):
    """(tau = sigma, the lambda in force): 1 / sqrt(4 sum g_a^2 + sum_{s live} c_s), the first sum in the order (1, 2, 0) over the axes
    longer than 1 (zero: the prior is off), the second over the stacks with a valid datum, ascending."""
    D, H, W = hr_shape
    s = 0.0
    if H > 1:
        s += g[1] * g[1]
    if W > 1:
        s += g[2] * g[2]
    if D > 1:
        s += g[0] * g[0]
    csum = 0.0
    for st in stacks:
        if valid_mask(st, hr_shape).any():
            csum += stack_bound(st)
    bound = 4.0 * s + csum
    return (1.0 / np.sqrt(bound) if bound > 0.0 else 1.0 / np.sqrt(8.0)), (lam if s > 0.0 else 0.0)


def weights(stacks, hr_shape, w=None):
    """The weights the solver works with, per stack: ``w`` (default 1) where a datum is valid and w > 0, else 0."""
    out = []
    for s, st in enumerate(stacks):
        valid = valid_mask(st, hr_shape)
        ws = np.ones(st[3]) if w is None else np.asarray(w[s], np.float64)
        with np.errstate(invalid="ignore"):
            out.append(np.where(valid & (ws > 0), ws, 0.0))
    return out


def backproject(ys, stacks, hr_shape, w=None):
    """(sum_s A_s^T y_s) / (sum_s A_s^T 1) over the usable data, 0 where the denominator is not > 0."""
    ww = weights(stacks, hr_shape, w)
    num = adjoint_all([np.where(u > 0, y, 0.0) for y, u in zip(ys, ww)], stacks, hr_shape)
    den = adjoint_all([(u > 0).astype(np.float64) for u in ww], stacks, hr_shape)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def energy(x, ys, stacks, lam, alpha, w=None, g=(1.0, 1.0, 1.0)):
    """1/2 sum_s sum w (A_s x - y_s)^2 + lam sum H_alpha(sqrt((g1 d1 x)^2 + (g2 d2 x)^2 + (g0 d0 x)^2)); data of weight 0 are not read."""
    ww = weights(stacks, x.shape, w)
    data = 0.0
    for y, u, st in zip(ys, ww, stacks):
        res = np.where(u > 0, apply(x, st) - np.where(u > 0, y, 0.0), 0.0)
        data += 0.5 * (u * res * res).sum()
    _, lam = step(stacks, x.shape, g, lam)
    if lam == 0:
        return data
    t0, t1, t2 = T3.grad(x, g)
    return data + lam * huber(np.sqrt((t1 * t1 + t2 * t2) + t0 * t0), alpha).sum()


def solve(ys, stacks, hr_shape, lam=3e-3, alpha=0.1, n_iter=300, g=(1.0, 1.0, 1.0), w=None, x0=None, return_info=False):
    """Chambolle-Pock with both terms dual, from x = xbar = x0 (default: the normalised back-projection), p = 0, q = 0."""
    hr_shape = tuple(hr_shape)
    ys = [np.asarray(y, np.float64) for y in ys]
    ww = weights(stacks, hr_shape, w)
    yy = [np.where(u > 0, y, 0.0) for y, u in zip(ys, ww)]
    safe = [np.where(u > 0, u, 1.0) for u in ww]
    tau, lam_on = step(stacks, hr_shape, g, lam)
    sigma = tau
    x = backproject(ys, stacks, hr_shape, w) if x0 is None else np.array(x0, np.float64)
    xbar = x.copy()
    p0, p1, p2 = np.zeros(hr_shape), np.zeros(hr_shape), np.zeros(hr_shape)
    q = [np.zeros(st[3]) for st in stacks]
    change = 0.0
    for _ in range(n_iter):
        if lam_on > 0:
            d0, d1, d2 = diffs(xbar)
            den = 1.0 + sigma * alpha / lam_on
            p1 = (p1 + sigma * (g[1] * d1)) / den
            p2 = (p2 + sigma * (g[2] * d2)) / den
            p0 = (p0 + sigma * (g[0] * d0)) / den
            s = np.maximum(1.0, np.sqrt((p1 * p1 + p2 * p2) + p0 * p0) / lam_on)
            p0, p1, p2 = p0 / s, p1 / s, p2 / s
        q = [np.where(u > 0, (qs + sigma * (apply(xbar, st) - y)) / (1.0 + sigma / sf), 0.0)
             for qs, y, u, sf, st in zip(q, yy, ww, safe, stacks)]
        xn = x - tau * (adjoint_all(q, stacks, hr_shape) - div(p0, p1, p2, g))
        change = np.abs(xn - x).max()
        xbar = 2.0 * xn - x
        x = xn
    if return_info:
        total = sum(int(np.prod(st[3])) for st in stacks)
        valid = sum(int(valid_mask(st, hr_shape).sum()) for st in stacks)
        return x, energy(x, ys, stacks, lam, alpha, w, g), change, valid / total
    return x


def power_norm_sq(st, hr_shape, n_iter=200, seed=0):
    """|A_s|^2 by power iteration on A_s^T A_s (a lower estimate)."""
    x = np.random.default_rng(seed).standard_normal(hr_shape)
    lam = 0.0
    for _ in range(n_iter):
        x = adjoint(apply(x, st), st, hr_shape)
        lam = np.linalg.norm(x)
        if lam == 0.0:
            return 0.0
        x = x / lam
    return lam


def lbfgs_minimum(ys, stacks, lam, alpha, w, shape, g=(1.0, 1.0, 1.0)):
    """The minimum of the Huber energy by L-BFGS-B with the analytic gradient (scipy), independent of the iteration."""
    from scipy.optimize import minimize
    ww = weights(stacks, shape, w)
    yy = [np.where(u > 0, y, 0.0) for y, u in zip(ys, ww)]

    def fun(z):
        x = z.reshape(shape)
        res = [apply(x, st) - y for st, y in zip(stacks, yy)]
        t0, t1, t2 = T3.grad(x, g)
        t = np.sqrt(t0 * t0 + t1 * t1 + t2 * t2)
        scale = np.where(t <= alpha, 1.0 / alpha, 1.0 / np.maximum(t, 1e-300))       # H'(t) / t
        e = sum(0.5 * (u * r * r).sum() for u, r in zip(ww, res)) + lam * huber(t, alpha).sum()
        grad = adjoint_all([u * r for u, r in zip(ww, res)], stacks, shape) - lam * div(scale * t0, scale * t1, scale * t2, g)
        return e, grad.ravel()

    z = backproject(ys, stacks, shape, w).ravel()
    for _ in range(5):                                                                # restarts: the memory is rebuilt at the iterate
        res = minimize(fun, z, jac=True, method="L-BFGS-B", options={"maxiter": 20000, "maxfun": 200000, "ftol": 0, "gtol": 1e-14,
                                                                     "maxcor": 50})
        z = res.x
    return float(res.fun)


# ---- the issue's cases ---------------------------------------------------------------------------------------------------------------
CASE_SHAPE = (7, 9, 10)
CASE_LAM, CASE_ALPHA = 0.05, 0.02
CASE_GRAD_WEIGHTS = ((1.0, 1.0, 1.0), (0.4, 1.0, 1.0))
ONE = np.ones(1)


def case_stacks():
    """Overlapping (running off the first slice), gapped, and column-thick running off both ends."""
    return [stack((2, 1, 1), ([.2, .3, .3, .2], ONE, ONE), (-1, 0, 0), (4, 9, 10)),
            stack((1, 3, 1), (ONE, [.5, .5], ONE), (0, 1, 0), (7, 3, 10)),
            stack((1, 1, 2), (ONE, ONE, [.25, .5, .25]), (0, 0, -1), (7, 9, 6))]


def limit_stack():
    """f = 8, L = 16 on an axis of 40 (hr shape (3, 40, 5))."""
    return (3, 40, 5), stack((1, 8, 1), (ONE, np.arange(1.0, 17.0) / 136.0, ONE), (0, 0, 0), hr_shape=(3, 40, 5))


def odd_stack():
    """f = 3, L = 5, o = -7 on the row axis of (3, 20, 4), with more indices than fit: the floor division on negatives."""
    return (3, 20, 4), stack((1, 3, 1), (ONE, [.1, .2, .4, .2, .1], ONE), (0, -7, 0), (3, 10, 4))


def case_data(seed=0):
    """-> (hr [7][9][10], ys, ws): the data of case_stacks, weights in [0.5, 1.5) with one zero weight."""
    rng = np.random.default_rng(seed)
    hr = rng.random(CASE_SHAPE)
    stacks = case_stacks()
    ys = apply_all(hr, stacks)
    ws = [0.5 + rng.random(st[3]) for st in stacks]
    ws[1][3, 1, 4] = 0.0
    return hr, ys, ws


# ---- the study --------------------------------------------------------------------------------------------------------------------------
STUDY_ROI, STUDY_LAM, STUDY_HUBER, STUDY_ITERS, STUDY_TRIM = (40, 90), 3e-3, 0.1, 300, 2


def profile_taps(length, spacing, kind="gaussian", fwhm=None):
    if kind == "mean":
        return np.full(length, 1.0 / length)
    sigma = fwhm / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    k = np.exp(-0.5 * (((2.0 * np.arange(length) + 1.0 - length) / (2.0 * spacing)) / sigma) ** 2)
    return k / k.sum()


def design_stacks(design, hr_shape, factor=2, fwhm=None):
    """The stacks of a study design on a volume of ``hr_shape``."""
    mean = np.full(factor, 1.0 / factor)
    if design == "shifted":
        return [stack((factor, 1, 1), (mean, ONE, ONE), (0, 0, 0), hr_shape=hr_shape),
                stack((factor, 1, 1), (mean, ONE, ONE), (factor // 2, 0, 0), hr_shape=hr_shape)]
    if design == "orthogonal":
        return [stack((factor, 1, 1), (mean, ONE, ONE), hr_shape=hr_shape), stack((1, factor, 1), (ONE, mean, ONE), hr_shape=hr_shape),
                stack((1, 1, factor), (ONE, ONE, mean), hr_shape=hr_shape)]
    if design == "overlap":
        k = profile_taps(2 * factor, factor, "gaussian", 1.0 if fwhm is None else fwhm)
        return [stack((factor, 1, 1), (k, ONE, ONE), hr_shape=hr_shape)]
    raise ValueError(design)


def study_data(volume, stacks, noise, seed):
    """The stacks' data from the thin slices, then the noise: one generator, the stacks in order."""
    rng = np.random.default_rng(seed)
    ys = apply_all(volume, stacks)
    return [y + noise * rng.standard_normal(y.shape) for y in ys] if noise > 0 else ys


def trim_psnr(ref, x, trim=STUDY_TRIM):
    c = slice(trim, -trim) if trim else slice(None)
    return psnr(ref[c], x[c])


@functools.lru_cache(maxsize=None)
def study_reference(design):
    """{name: (volume, PSNR over slices 2:-2)} of the restated study on pat07 ROI 40:90, no noise."""
    vol = pat07_roi(*STUDY_ROI)
    stacks = design_stacks(design, vol.shape)
    ys = study_data(vol, stacks, 0.0, 0)
    out = {}
    for s, (st, y) in enumerate(zip(stacks, ys)):
        out[f"stack{s}"] = solve([y], [st], vol.shape, STUDY_LAM, STUDY_HUBER, STUDY_ITERS)
    out["mean"] = sum(out[f"stack{s}"] for s in range(len(stacks))) / len(stacks)
    out["joint"] = solve(ys, stacks, vol.shape, STUDY_LAM, STUDY_HUBER, STUDY_ITERS)
    return {name: (x, trim_psnr(vol, x)) for name, x in out.items()}
