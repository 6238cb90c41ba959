"""Shared by tests/test_fourier_cpu.py and tests/test_gpu_fourier.py: Fourier (k-space zero-fill / truncation) re-sampling, twice.

``restated_operator`` is the dense operator of DESIGN.md 4j in plain float64 numpy, written from its formulas the way
csrc/fourier.hip evaluates them (the phase of every cosine reduced exactly in int64, the terms added in ascending k, a mirror
entry the sum of its two folded cosine sums).  It is the definition the kernels are written from.

The oracles never build an operator:
  * ``scipy.signal.resample`` for the periodic boundary with ``align='sample'`` and no window,
  * ``scipy.signal.resample`` of the explicitly mirrored line, cropped, for the mirror boundary with ``align='sample'``, no window,
  * ``trig_resample``: the trigonometric polynomial of the line evaluated at the output positions from its ``np.fft.fft``
    coefficients, for ``align='center'`` and for apodised cases -- of the mirrored line for their mirror forms.  It shares no
    helper with the restatement: its window and its bin weights are written out in place.
``oracle_resample`` picks among them; a device mismatch can so be told from a wrong restatement.
"""
import numpy as np
import scipy.signal

ALIGNS = ("sample", "center")
BOUNDARIES = ("periodic", "mirror")
PAIRS = [(5, 8), (8, 5), (8, 16), (16, 8), (7, 7), (8, 8), (25, 50), (50, 25), (26, 51), (1, 4), (4, 1)]      # (n, m) of the issue
MIRROR_SAMPLE_PAIRS = [(25, 50), (50, 25), (8, 24), (2, 4)]
GPU_EXTRA_PAIRS = [(17, 33), (33, 17), (130, 257)]       # ragged 16-tiles, a K loop of more than one stage
APODIZE = (0.0, 0.5, 1.0)
FP64_BOUND = 1e-12                    # of max(max|in|, max|want|): the project's fp64 bound


def mirror_sample_ok(n, m):
    return n >= 2 and ((2 * n - 2) * m) % n == 0


def tukey(k, L, alpha):
    """The window over the kept band: r = k / (L/2); 1 up to r = 1 - alpha, a raised cosine down to 0 at r = 1."""
    if alpha <= 0:
        return 1.0
    r = 2.0 * k / L
    return 1.0 if r <= 1.0 - alpha else 0.5 * (1.0 + np.cos(np.pi * (r - 1.0 + alpha) / alpha))


def nyquist_weight(En, Em):
    """c_k at k = L/2 of an even L: the input's own Nyquist bin counts once, two bins folded onto the output's count twice."""
    return 1.0 if min(En, Em) == En else 2.0


def _cos_sums(En, Em, rows, cols, center, apodize):
    """S[i, j] = sum_{k = 0..K} c_k w(k) cos(2 pi k (p_i - j) / En) of the periodic operator En -> Em, rows i, columns j."""
    L = min(En, Em)
    K = L // 2
    D = 2 * En * Em
    q = 2 * En * np.asarray(rows, np.int64)[:, None] - 2 * Em * np.asarray(cols, np.int64)[None, :] + ((En - Em) if center else 0)
    q = np.mod(q, D)                                     # cos(pi * k q / (En Em)): exact in int64
    S = np.zeros(q.shape)
    for k in range(K + 1):
        c = 1.0 if k == 0 else (nyquist_weight(En, Em) if 2 * k == L else 2.0)
        S += c * tukey(k, L, apodize) * np.cos(np.pi * (np.mod(k * q, D) / float(En * Em)))
    return S


def restated_operator(n, m, align="sample", boundary="mirror", apodize=0.0):
    """A [m][n] with y = A x."""
    assert align in ALIGNS and boundary in BOUNDARIES and 0.0 <= apodize <= 1.0
    center = align == "center"
    i, j = np.arange(m), np.arange(n)
    if boundary == "periodic":
        return _cos_sums(n, m, i, j, center, apodize) / n
    if center:                                            # [x, x[::-1]], period 2n -> 2m
        return (_cos_sums(2 * n, 2 * m, i, j, True, apodize) + _cos_sums(2 * n, 2 * m, i, 2 * n - 1 - j, True, apodize)) / (2 * n)
    assert mirror_sample_ok(n, m)                         # [x, x[n-2:0:-1]], period P = 2n - 2 -> P m / n
    P = 2 * n - 2
    M = P * m // n
    inner = ((j > 0) & (j < n - 1)).astype(np.float64)
    return (_cos_sums(P, M, i, j, False, apodize) + inner * _cos_sums(P, M, i, P - j, False, apodize)) / P


def restated_resize(img, out_hw, align="sample", boundary="mirror", apodize=0.0):
    """The trailing two axes of ``img``: Y = A_rows X A_cols^T."""
    img = np.asarray(img, np.float64)
    a_rows = restated_operator(img.shape[-2], out_hw[0], align, boundary, apodize)
    a_cols = restated_operator(img.shape[-1], out_hw[1], align, boundary, apodize)
    return a_rows @ img @ a_cols.T


def trig_resample(x, m, align="sample", apodize=0.0):
    """Axis 0 of ``x`` (period n) at p_i = i n / m + delta: (1/n) Re sum_k w(k) X_k exp(2 pi i k p / n) over the kept band."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    X = np.fft.fft(x, axis=0)
    L = min(n, m)
    p = np.arange(m) * (n / m) + ((n / m - 1) / 2 if align == "center" else 0.0)
    tail = (1,) * (x.ndim - 1)
    y = np.broadcast_to(X[0].real, (m,) + x.shape[1:]).copy()
    for k in range(1, L // 2 + 1):
        # the window and the bin weights are written out here, in other terms than the restatement's: cos^2 of the half angle
        # for the taper, and the +k and -k bins counted one by one (the input's own Nyquist bin is ONE bin and is counted once)
        r = k / (L / 2)
        window = 1.0 if apodize <= 0 or r <= 1 - apodize else np.cos(0.5 * np.pi * (r - 1 + apodize) / apodize) ** 2
        bins = 1 if (2 * k == n and n <= m) else 2
        y += bins * window * (X[k][None] * np.exp(2j * np.pi * k * p / n).reshape((m,) + tail)).real
    return y / n


def _periodic_oracle(x, m, align, apodize):
    if align == "sample" and apodize == 0.0:
        return scipy.signal.resample(x, m, axis=0)
    return trig_resample(x, m, align, apodize)


def oracle_resample(x, m, align="sample", boundary="mirror", apodize=0.0):
    """Axis 0 of ``x`` re-sampled to ``m`` points by the oracle of the module docstring."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    if boundary == "periodic":
        return _periodic_oracle(x, m, align, apodize)
    if align == "center":
        return _periodic_oracle(np.concatenate([x, x[::-1]], axis=0), 2 * m, align, apodize)[:m]
    assert mirror_sample_ok(n, m)
    ext = np.concatenate([x, x[n - 2:0:-1]], axis=0)
    return _periodic_oracle(ext, (2 * n - 2) * m // n, align, apodize)[:m]


def oracle_resize(img, out_hw, align="sample", boundary="mirror", apodize=0.0):
    """The trailing two axes of ``img``, one axis after the other through ``oracle_resample``."""
    img = np.asarray(img, np.float64)
    a = np.moveaxis(oracle_resample(np.moveaxis(img, -1, 0), out_hw[1], align, boundary, apodize), 0, -1)
    return np.moveaxis(oracle_resample(np.moveaxis(a, -2, 0), out_hw[0], align, boundary, apodize), 0, -2)


def bound(x, want, rel=FP64_BOUND):
    return rel * max(np.abs(x).max(), np.abs(want).max())


def lines(n, count=3, seed=0):
    """Unit-normal lines [n][count]."""
    return np.random.default_rng(seed + 1000 * n).standard_normal((n, count))
