"""The second-order TGV super-resolution of csrc/tgv.hip restated in float64 NumPy: the symmetrised derivative E, the
1-D divergences, the objective and the Chambolle-Pock iteration, on the block operator, gradient and Huber function of
tests/tvsr_common.py.  Images are the trailing two axes, leading axes are a batch.  The tests compare the kernel with these functions;
nothing here imports the package.  CASE_* and case_data are the weighted 6 x 10 case of tvsr_common (factors (3, 2), one w = 0).
``solve`` takes ``dtype`` so that the same iteration can run in longdouble."""
import numpy as np

from tests.tvsr_common import (CASE_ALPHA, CASE_FACTORS, CASE_LAM, CASE_W, apply_A, apply_AT, block_kernel, case_data, grad, huber,  # noqa: F401
                                replicate)

STEP = 1.0 / np.sqrt(12.0)           # tau = sigma: |K|^2 <= 12 for K(x, v) = (grad x - v, Ev)


def d0(a):
    """Forward difference along the rows, zero last row."""
    out = np.zeros_like(a)
    out[..., :-1, :] = a[..., 1:, :] - a[..., :-1, :]
    return out


def d1(a):
    """Forward difference along the columns, zero last column."""
    out = np.zeros_like(a)
    out[..., :, :-1] = a[..., :, 1:] - a[..., :, :-1]
    return out


def div0(r):
    """-d0^T: r[i] - r[i - 1], the missing terms zero; the last row of r does not count (d0 is zero there)."""
    out = np.zeros_like(r)
    out[..., :-1, :] += r[..., :-1, :]
    out[..., 1:, :] -= r[..., :-1, :]
    return out


def div1(r):
    out = np.zeros_like(r)
    out[..., :, :-1] += r[..., :, :-1]
    out[..., :, 1:] -= r[..., :, :-1]
    return out


def sym_grad(v0, v1):
    """Ev = (e00, e11, e01) = (d0 v0, d1 v1, (d1 v0 + d0 v1) / 2)."""
    return d0(v0), d1(v1), (d1(v0) + d0(v1)) / 2.0


def frob(e00, e11, e01):
    """|Ev|_F: the off-diagonal entry counts twice."""
    return np.sqrt(e00 * e00 + e11 * e11 + 2.0 * (e01 * e01))


def K(x, v0, v1):
    """K(x, v) = (grad x - v, Ev) -> (p0, p1, r00, r11, r01)."""
    g0, g1 = grad(x)
    return (g0 - v0, g1 - v1) + sym_grad(v0, v1)


def KT(p0, p1, r00, r11, r01):
    """The adjoint of K for the inner product that counts r01 twice -> (x, v0, v1)."""
    return -(div0(p0) + div1(p1)), -p0 - (div0(r00) + div1(r01)), -p1 - (div1(r11) + div0(r01))


def energy(x, v0, v1, y, k, lam, ratio, alpha, w=None):
    """1/2 sum w (A x - y)^2 + lam sum H_alpha(|grad x - v|) + ratio lam sum |Ev|_F, per image."""
    r = apply_A(x, k) - y
    data = 0.5 * ((1.0 if w is None else w) * r * r).sum(axis=(-2, -1))
    if lam == 0:
        return data
    g0, g1 = grad(x)
    g0, g1 = g0 - v0, g1 - v1
    first = huber(np.sqrt(g0 * g0 + g1 * g1), alpha).sum(axis=(-2, -1))
    second = frob(*sym_grad(v0, v1)).sum(axis=(-2, -1))
    return data + lam * first + (ratio * lam) * second


def solve(y, factors, kernel="mean", lam=0.01, ratio=2.0, alpha=0.0, n_iter=100, w=None, x0=None, return_info=False,
          dtype=np.float64):
    """Chambolle-Pock, tau = sigma = 1/sqrt(12), from x = xbar = x0 (default: block replication of y), v = vbar = 0, p = 0, r = 0.
    -> x, or (x, v [..., 2, H, W], energy, change) with ``return_info``."""
    y = np.asarray(y, dtype)
    k = block_kernel(kernel, factors).astype(dtype)
    k2 = (k * k).sum()
    w = np.ones_like(y) if w is None else np.broadcast_to(np.asarray(w, dtype), y.shape)
    tau = sigma = dtype(1.0) / np.sqrt(dtype(12.0))
    lam1, lam0, alpha = dtype(lam), dtype(ratio) * dtype(lam), dtype(alpha)
    c = tau * w / (1.0 + tau * w * k2)
    x = replicate(y, factors) if x0 is None else np.array(x0, dtype)
    xbar = x.copy()
    v0, v1, vbar0, vbar1 = (np.zeros_like(x) for _ in range(4))
    p0, p1, r00, r11, r01 = (np.zeros_like(x) for _ in range(5))
    change = np.zeros(x.shape[:-2], dtype)
    ysafe = np.where(w == 0, 0.0, y)          # a missing datum is never read
    for _ in range(n_iter):
        if lam1 > 0:
            g0, g1 = grad(xbar)
            den = 1.0 + sigma * alpha / lam1
            p0 = (p0 + sigma * (g0 - vbar0)) / den
            p1 = (p1 + sigma * (g1 - vbar1)) / den
            s = np.maximum(1.0, np.sqrt(p0 * p0 + p1 * p1) / lam1)
            p0, p1 = p0 / s, p1 / s
            e00, e11, e01 = sym_grad(vbar0, vbar1)
            r00, r11, r01 = r00 + sigma * e00, r11 + sigma * e11, r01 + sigma * e01
            s = np.maximum(1.0, frob(r00, r11, r01) / lam0)
            r00, r11, r01 = r00 / s, r11 / s, r01 / s
        # div(p) in the order of tvsr_common.div
        d = np.zeros_like(p0)
        d[..., :-1, :] += p0[..., :-1, :]
        d[..., 1:, :] -= p0[..., :-1, :]
        d[..., :, :-1] += p1[..., :, :-1]
        d[..., :, 1:] -= p1[..., :, :-1]
        u = x + tau * d
        xn = u - apply_AT(c * (apply_A(u, k) - ysafe), k)
        change = np.abs(xn - x).max(axis=(-2, -1))
        xbar = 2.0 * xn - x
        x = xn
        if lam1 > 0:
            n0 = v0 + tau * (p0 + div0(r00) + div1(r01))
            n1 = v1 + tau * (p1 + div1(r11) + div0(r01))
            vbar0, vbar1 = 2.0 * n0 - v0, 2.0 * n1 - v1
            v0, v1 = n0, n1
    if return_info:
        return x, np.stack([v0, v1], axis=-3), energy(x, v0, v1, ysafe, k, lam1, dtype(ratio), alpha, w), change
    return x


def phantom(n=48):
    """A ramp, a quadratic and a disc: x = 0.2 + 0.5 i + 0.2 j^2 + 0.25 [(i - 0.4)^2 + (j - 0.55)^2 < 0.04], divided by its maximum."""
    t = np.arange(n) / (n - 1.0)
    i, j = t[:, None], t[None, :]
    x = 0.2 + 0.5 * i + 0.2 * j ** 2 + 0.25 * ((i - 0.4) ** 2 + (j - 0.55) ** 2 < 0.04)
    return x / x.max()


def phantom_data(seed, noise=0.02):
    """-> (HR phantom [48, 48], its 2 x 2 block mean plus noise [24, 24])."""
    hr = phantom()
    lr = apply_A(hr, block_kernel("mean", (2, 2)))
    return hr, lr + noise * np.random.default_rng(seed).standard_normal(lr.shape)


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def flat_share(x, thr=1e-3):
    """The share of interior pixels with |grad x| < thr: a flat-area index of staircasing."""
    g0, g1 = grad(np.asarray(x, np.float64))
    m = np.sqrt(g0 * g0 + g1 * g1)[..., :-1, :-1]
    return float((m < thr).mean())


def tgv_lbfgs_minimum(y, k, lam, ratio, alpha, eps, w, shape):
    """The minimum over (x, v) of the energy with lam0 |Ev|_F replaced by lam0 H_eps(|Ev|_F) (alpha > 0, eps > 0: smooth and convex),
    by L-BFGS-B with the analytic gradient, independent of the iteration.  -> (value m at the last iterate z, |gradient|_1 there): by
    convexity the minimum is at least m - |gradient|_1 |z* - z|_inf."""
    from scipy.optimize import minimize

    H, W = shape[-2:]
    n = H * W
    lam0 = ratio * lam

    def fun(z):
        x, v0, v1 = z[:n].reshape(H, W), z[n:2 * n].reshape(H, W), z[2 * n:].reshape(H, W)
        res = apply_A(x, k) - y
        g0, g1 = grad(x)
        g0, g1 = g0 - v0, g1 - v1
        t = np.sqrt(g0 * g0 + g1 * g1)
        s1 = np.where(t <= alpha, 1.0 / alpha, 1.0 / np.maximum(t, 1e-300))           # H'(t) / t
        e00, e11, e01 = sym_grad(v0, v1)
        f = frob(e00, e11, e01)
        s0 = np.where(f <= eps, 1.0 / eps, 1.0 / np.maximum(f, 1e-300))
        e = 0.5 * (w * res * res).sum() + lam * huber(t, alpha).sum() + lam0 * huber(f, eps).sum()
        gx, gv0, gv1 = KT(lam * s1 * g0, lam * s1 * g1, lam0 * s0 * e00, lam0 * s0 * e11, lam0 * s0 * e01)
        gx = gx + apply_AT(w * res, k)
        return e, np.concatenate([gx.ravel(), gv0.ravel(), gv1.ravel()])

    z = np.concatenate([replicate(y, k.shape).ravel(), np.zeros(2 * n)])
    for _ in range(5):
        res = minimize(fun, z, jac=True, method="L-BFGS-B", options={"maxiter": 20000, "maxfun": 200000, "ftol": 0, "gtol": 1e-14,
                                                                     "maxcor": 50})
        z = res.x
    return float(res.fun), float(np.abs(res.jac).sum())
