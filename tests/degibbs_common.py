"""The float64 restatement of Gibbs-ringing removal by local sub-voxel shifts (include/inrhip.h: inr_degibbs_lines, inr_degibbs2d;
DESIGN.md 4v; Kellner et al., MRM 2016), twice, the phantoms the tests share and the cases the issue fixes.  Nothing here runs on a
device.

The definition, for one periodic line x[0..n), nshifts = N and the window (w_min, w_max), all indices mod n: the candidates are the
shifts s_0 = 0, s_j = j / (2N), s_{N+j} = -j / (2N) (j = 1 .. N) in this order; x_s[i] is the band-limited interpolant at i + s (the
Nyquist bin of an even n split between +n/2 and -n/2), and the copy for s_0 is the line itself; d_s[i] = |x_s[i] - x_s[i-1]|, L_s[i] =
sum_t d_s[i - t], R_s[i] = sum_t d_s[i + t + 1] over t = w_min .. w_max ascending, tv_s = min(L_s, R_s); the choice is the first candidate
with the smallest tv, and the output interpolates the chosen copy back onto the grid.  An image is split by G1 = c_0 / (c_0 + c_1),
c_a(k) = 1 + cos(2 pi k / n_a) (1/2 where both vanish), into I1 = Re IDFT2(G1 DFT2(I)) and I0 = I - I1; out = U1(I1) + U0(I0).

The two paths: ``fft`` makes the copies and the split with np.fft (phase factor cos(pi s) at the Nyquist bin); ``dense`` forms the
table h_s(d) by the cosine sum in ascending k with the phase reduced in integers, multiplies by the circulant matrices, and splits with
the dense cosine / sine DFT matrices -- the kernel's sums in another order.  Their deviation ``d_ref`` is what a test allows the
kernel a multiple of."""
import functools

import numpy as np

EPS = 2.220446049250313e-16
NSHIFTS, WINDOW = 20, (1, 3)
MARGIN = 1e-10                 # choices are compared where the decision margin is at least this
MAX_EXCLUDED = 0.002           # of the samples of a case
BOUND_FACTOR = 32.0            # what tests/test_gpu_mppca.py gives another summation order of the same float64 sums

# id, (batch, H, W), noise (None: pure standard_normal)
CASES = (("ragged-even", (3, 24, 20), 0.02),
         ("odd", (2, 15, 33), 0.02),
         ("tile-edges", (1, 64, 70), 0.02),
         ("smallest", (2, 9, 9), 0.02),
         ("two-tiles", (1, 130, 40), 0.0),
         ("noise-only", (2, 32, 32), None))
CASE_IDS = tuple(c[0] for c in CASES)


def shifts(N):
    """The 2N + 1 candidate shifts in list order."""
    j = np.arange(1, N + 1)
    return np.concatenate([[0.0], j / (2 * N), -j / (2 * N)])


def copies_fft(x, N):
    """[2N + 1, ..., n]: the shifted copies of the lines ``x`` [..., n] by np.fft; copy 0 is ``x`` itself."""
    n = x.shape[-1]
    k = np.fft.fftfreq(n, 1.0 / n)
    X = np.fft.fft(x, axis=-1)
    out = [x]
    for s in shifts(N)[1:]:
        ph = np.exp(2j * np.pi * k * s / n)
        if n % 2 == 0:
            ph[n // 2] = np.cos(np.pi * s)
        out.append(np.fft.ifft(X * ph, axis=-1).real)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def table(n, N):
    """h [2N][n]: rows 0 .. N - 1 the shifts +j / (2N), rows N .. 2N - 1 the shifts -j / (2N); the cosine sum in ascending k, the phase
    pi ((k (2N d + j)) mod (2N n)) / (N n)."""
    D = 2 * N * n
    d = np.arange(n, dtype=np.int64)
    h = np.empty((2 * N, n))
    for sidx in range(2 * N):
        j = sidx + 1 if sidx < N else -(sidx - N + 1)
        q = (2 * N * d + j) % D
        s = np.zeros(n)
        for k in range(n // 2 + 1):
            c = 1.0 if k == 0 or 2 * k == n else 2.0
            s += c * np.cos(np.pi * (((k * q) % D) / (N * n)))
        h[sidx] = s / n
    h.setflags(write=False)
    return h


def copies_dense(x, N):
    """``copies_fft`` by products with the circulant matrices of ``table``."""
    n = x.shape[-1]
    h = table(n, N)
    i = np.arange(n)
    idx = (i[None, :] - i[:, None]) % n                      # [j][i] -> (i - j) mod n
    return np.stack([x] + [x @ h[sidx][idx] for sidx in range(2 * N)])


def choose(xs, N, window, max_abs):
    """(out, choice, margin) from the copies ``xs`` [2N + 1, ..., n]: ``choice`` the index in list order, ``margin`` (second smallest tv
    - smallest tv) / ``max_abs``."""
    w_min, w_max = window
    d = np.abs(xs - np.roll(xs, 1, axis=-1))
    L = np.zeros_like(d)
    R = np.zeros_like(d)
    for t in range(w_min, w_max + 1):
        L += np.roll(d, t, axis=-1)                          # d[i - t]
    for t in range(w_min, w_max + 1):
        R += np.roll(d, -(t + 1), axis=-1)                   # d[i + t + 1]
    tv = np.minimum(L, R)
    choice = np.argmin(tv, axis=0)                           # the first of equal minima
    two = np.partition(tv, 1, axis=0)[:2]
    margin = (two[1] - two[0]) / max_abs if max_abs > 0 else np.full(choice.shape, np.inf)
    s = shifts(N)[choice]
    pick = lambda a: np.take_along_axis(a, choice[None], axis=0)[0]
    c, left, right = pick(xs), pick(np.roll(xs, 1, axis=-1)), pick(np.roll(xs, -1, axis=-1))
    out = np.where(s > 0, (1 - s) * c + s * left, np.where(s < 0, (1 + s) * c - s * right, c))
    return out, choice.astype(np.int32), margin


def lines(x, N=NSHIFTS, window=WINDOW, path="fft", max_abs=None):
    """The line operation on ``x`` [..., n] along its last axis: (out, choice, margin)."""
    x = np.asarray(x, np.float64)
    xs = copies_fft(x, N) if path == "fft" else copies_dense(x, N)
    return choose(xs, N, window, float(np.abs(x).max()) if max_abs is None else max_abs)


def _c(n):
    c = 1.0 + np.cos(2 * np.pi * np.arange(n) / n)
    if n % 2 == 0:
        c[n // 2] = 0.0
    return c


def g1(H, W):
    c0, c1 = _c(H)[:, None], _c(W)[None, :]
    den = c0 + c1
    return np.where(den == 0, 0.5, c0 / np.where(den == 0, 1.0, den))


def _dft(n):
    k = np.arange(n, dtype=np.int64)
    ph = 2.0 * ((k[:, None] * k[None, :]) % n) / n
    return np.cos(np.pi * ph), np.sin(np.pi * ph)


def split(I, path="fft"):
    """(I1, I0) of the images ``I`` [..., H, W]."""
    I = np.asarray(I, np.float64)
    H, W = I.shape[-2:]
    G = g1(H, W)
    if path == "fft":
        I1 = np.fft.ifft2(G * np.fft.fft2(I)).real
    else:
        (C0, S0), (C1, S1) = _dft(H), _dft(W)
        P, Q = I @ C1, -(I @ S1)
        Xr, Xi = G * (C0 @ P + S0 @ Q), G * (C0 @ Q - S0 @ P)
        Yr, Yi = (C0 @ Xr - S0 @ Xi) / H, (S0 @ Xr + C0 @ Xi) / H
        I1 = (Yr @ C1 - Yi @ S1) / W
    return I1, I - I1


def degibbs2d(I, N=NSHIFTS, window=WINDOW, path="fft"):
    """(out, choice [2, ...], margin [2, ...]) of the images ``I`` [..., H, W]; index 0 is the pass along axis 0."""
    I = np.asarray(I, np.float64)
    top = float(np.abs(I).max())
    I1, I0 = split(I, path)
    o1, c1, m1 = lines(I1, N, window, path, top)
    o0, c0, m0 = lines(np.swapaxes(I0, -1, -2), N, window, path, top)
    sw = lambda a: np.swapaxes(a, -1, -2)
    return o1 + sw(o0), np.stack([sw(c0), c1]), np.stack([sw(m0), m1])


def flip_choice(choice, N):
    """The choice of the mirrored line: j <-> j + N."""
    c = np.asarray(choice)
    return np.where(c == 0, 0, np.where(c <= N, c + N, c - N))


# ---- phantoms -----------------------------------------------------------------------------------------------------------------------------
FINE = 8


def trunc(fine, H, W):
    """The central H x W crop of the centred 2-D spectrum of ``fine``, back in the image domain: what a scanner acquiring H x W samples
    of k-space shows."""
    F = np.fft.fftshift(np.fft.fft2(fine))
    h0, w0 = fine.shape[0] // 2 - H // 2, fine.shape[1] // 2 - W // 2
    crop = F[h0:h0 + H, w0:w0 + W]
    return np.fft.ifft2(np.fft.ifftshift(crop)).real * (H * W) / fine.size


def phantom(H, W):
    """An ellipse, plus a 0.6 disc, minus a 0.4 bar, plus a 0.2 x ramp, sampled FINE times finer than H x W."""
    y, x = np.meshgrid((np.arange(FINE * H) + 0.5) / (FINE * H) - 0.5, (np.arange(FINE * W) + 0.5) / (FINE * W) - 0.5, indexing="ij")
    p = 1.0 * ((x / 0.40) ** 2 + (y / 0.33) ** 2 < 1.0)
    p += 0.6 * ((x + 0.12) ** 2 + (y - 0.05) ** 2 < 0.11 ** 2)
    p -= 0.4 * ((np.abs(x - 0.15) < 0.04) & (np.abs(y) < 0.2))
    p += 0.2 * (x + 0.5) * (p > 0)
    return p


@functools.lru_cache(maxsize=None)
def case(name):
    """The images [batch, H, W] of a case: image k is (1 + 0.5 k) trunc(phantom) + noise standard_normal, drawn from default_rng(7)."""
    _, (batch, H, W), noise = CASES[CASE_IDS.index(name)]
    rng = np.random.default_rng(7)
    if noise is None:
        out = rng.standard_normal((batch, H, W))
    else:
        base = trunc(phantom(H, W), H, W)
        out = np.stack([(1 + 0.5 * k) * base + noise * rng.standard_normal((H, W)) for k in range(batch)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference2d(name, path="fft"):
    """(out, choice, margin) of ``degibbs2d`` on a case at the defaults, computed once."""
    return degibbs2d(case(name), NSHIFTS, WINDOW, path)


@functools.lru_cache(maxsize=None)
def reference_lines(name, path="fft"):
    """(out, choice, margin) of ``lines`` on the rows of a case ([batch * H, W]) at the defaults, computed once."""
    I = case(name)
    return lines(I.reshape(-1, I.shape[-1]), NSHIFTS, WINDOW, path)


def two_box(n):
    """(truth, rung, interior) of the two-box phantom on n x n: the piecewise-constant truth (box edges on pixel boundaries), its
    k-space truncation from a FINE times finer sampling, and the pixels at least 2 pixels from every edge."""
    truth = np.zeros((n, n))
    a, b = n // 4, n - n // 4
    truth[a:b, a:b] = 1.0
    truth[a + n // 8:b - n // 8, a + n // 8:n // 2] = 0.4
    fine = np.kron(truth, np.ones((FINE, FINE)))
    # the truncated image samples the fine grid at 8 i, the pixel's first fine sample: shift by the half pixel to its centre
    fine = np.roll(fine, (-(FINE // 2), -(FINE // 2)), axis=(0, 1))
    rung = trunc(fine, n, n)
    edge = np.zeros((n, n), bool)
    for ax in (0, 1):
        diff = truth != np.roll(truth, 1, axis=ax)
        edge |= diff | np.roll(diff, -1, axis=ax)
    near = edge.copy()
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            near |= np.roll(edge, (dy, dx), axis=(0, 1))
    return truth, rung, ~near


def error_ratio(truth, rung, unrung, interior):
    """mean |unrung - truth| over mean |rung - truth|, both over ``interior``."""
    return float(np.abs(unrung - truth)[interior].mean() / np.abs(rung - truth)[interior].mean())
