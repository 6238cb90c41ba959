"""Float64 NumPy restatement of ``erd.erd_volume`` (david.py:44-91 for whole slices), written from the description of the
computation -- NOT from the reference's program text -- plus what its tests share.

Per pixel: the acceptance weights come from ``oracle.erd_oracle`` (rules 1 and 2; a pixel holding a non-finite value is not
clustered and keeps everything) or are the supplied ones (rule 0).  Per group of consecutive acquisitions, three sequential sums
in acquisition order, each from 0.0: ``sum_image += v``, ``sum_accepted += v * a``, ``sum_accepts += a``; then
``direction_mean = sum_image / size``, ``accepted_mean = sum_accepted / sum_accepts`` (0 / 0 = NaN) and
``adc(v) = -log(v / (b0 + 1e-7) + 1e-7) / b * 1000`` of both means and of every acquisition.

The ULP bound of the ADC comparisons.  Both sides feed bitwise equal arguments to ``log``; they differ by the two libraries'
``log`` errors and by the roundings of ``/ b`` and ``* 1000`` applied to slightly different values:

* device: the HIP math API documents the double-precision ``log`` of the device library (OCML) with a maximum error of 1 ULP
  (ROCm documentation, "HIP math API", double-precision mathematical functions);
* NumPy: float64 ``np.log`` is the C library's ``log`` -- the glibc manual ("Known Maximum Errors in Math Functions") lists 1 ULP
  for x86_64 -- or, on CPUs with AVX-512, NumPy's own AVX512F kernel, which NumPy documents as staying below 1 ULP;
* plus 2 for the two roundings that follow.
"""
import collections

import numpy as np

from oracle import erd_oracle as E

EPS = 1e-7
LOG_ULP_DEVICE = 1
LOG_ULP_NUMPY = 1
ADC_ULP = LOG_ULP_DEVICE + LOG_ULP_NUMPY + 2          # = 4

Restated = collections.namedtuple("Restated", "accept direction_mean accepted_mean direction_adc accepted_adc adc")


def adc(v, b0, b):
    with np.errstate(all="ignore"):
        ratio = np.asarray(v, np.float64) / (np.asarray(b0, np.float64) + EPS)
        out = -np.log(ratio + EPS) / float(b)
        return out * 1000.0


def accept_weights(dwi, rule, erd_map=None):
    """[..., n] -> int64 0 / 1, per pixel through the oracle; pixels with a non-finite value keep everything."""
    x = np.asarray(dwi, np.float64)
    n = x.shape[-1]
    flat = x.reshape(-1, n)
    em = None if erd_map is None else np.asarray(erd_map, np.float64).reshape(-1)
    out = np.ones(flat.shape, np.int64)
    for p in range(flat.shape[0]):
        if not np.isfinite(flat[p]).all():
            continue
        with np.errstate(all="ignore"):
            positive = True if em is None else bool(em[p] > 0)
        out[p] = E.accept_mask(flat[p], rule, n, positive)
    return out.reshape(x.shape)


def restate(dwi, b0, acquisitions, b, rule=1, erd_map=None, accept=None, known_accept=None):
    """``known_accept``: acceptance weights already computed for (dwi, rule, erd_map), to spare a second pass of the oracle."""
    x = np.asarray(dwi, np.float64)
    b0 = np.asarray(b0, np.float64)
    n = x.shape[-1]
    sizes = [int(g) for g in np.asarray(acquisitions).reshape(-1)]
    assert sum(sizes) == n and min(sizes) >= 1
    if rule == 0:
        acc = np.ones(x.shape) if accept is None else np.asarray(accept, np.float64)
    else:
        acc = known_accept if known_accept is not None else accept_weights(x, rule, erd_map)
    w = np.asarray(acc, np.float64)
    lead = x.shape[:-1]
    maps = np.empty((4, len(sizes)) + lead)
    first = 0
    with np.errstate(all="ignore"):
        for g, size in enumerate(sizes):
            sum_image, sum_accepted, sum_accepts = np.zeros(lead), np.zeros(lead), np.zeros(lead)
            for a in range(first, first + size):
                sum_image = sum_image + x[..., a]
                sum_accepted = sum_accepted + x[..., a] * w[..., a]
                sum_accepts = sum_accepts + w[..., a]
            first += size
            maps[0, g] = sum_image / size
            maps[1, g] = sum_accepted / sum_accepts
            maps[2, g] = adc(maps[0, g], b0, b)
            maps[3, g] = adc(maps[1, g], b0, b)
    return Restated(acc, maps[0], maps[1], maps[2], maps[3], adc(x, b0[..., None], b))


def extent_two_clusters(values):
    """The oracle's chain walk with every cluster distance taken from the clusters' (min, max) extents instead of an n x n
    matrix, and the cut taken as the members of the dropped slot at the last-found merge of the largest distance (the last of
    a stable sort by distance).  Boolean mask of one of the two clusters; None where no neighbour can be found."""
    x = np.asarray(values, np.float64).reshape(-1)
    n = x.size
    cmin, cmax = x.copy(), x.copy()
    member = [1 << i for i in range(n)]
    alive = [True] * n
    chain = []
    cut, cut_dist = 0, -np.inf
    with np.errstate(all="ignore"):
        for _ in range(n - 1):
            if not chain:
                chain.append(alive.index(True))
            while True:
                a = chain[-1]
                if len(chain) > 1:
                    b = chain[-2]
                    cur = max(cmax[a], cmax[b]) - min(cmin[a], cmin[b])
                else:
                    b, cur = -1, np.inf
                for i in range(n):
                    if not alive[i] or i == a:
                        continue
                    d = max(cmax[a], cmax[i]) - min(cmin[a], cmin[i])
                    if d < cur:
                        cur, b = d, i
                if b < 0:
                    return None
                if len(chain) > 1 and b == chain[-2]:
                    break
                assert len(chain) < n
                chain.append(b)
            del chain[-2:]
            lo, hi = (a, b) if a < b else (b, a)
            if cur >= cut_dist:
                cut_dist, cut = cur, member[lo]
            member[hi] |= member[lo]
            cmin[hi], cmax[hi] = min(cmin[lo], cmin[hi]), max(cmax[lo], cmax[hi])
            alive[lo] = False
    return np.asarray([bool((cut >> i) & 1) for i in range(n)])


def ulp_distance(a, b):
    """Element-wise distance in float64 ULPs (the number of representable values between); 0 where both are NaN, 2^62 where
    only one is."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)

    def ordered(v):
        i = np.ascontiguousarray(v).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i).astype(object)

    d = np.abs(ordered(a) - ordered(b))
    na, nb = np.isnan(a), np.isnan(b)
    d = np.where(na & nb, 0, np.where(na ^ nb, 2 ** 62, d))
    return d


def max_ulp(a, b):
    d = ulp_distance(a, b)
    return int(d.max()) if d.size else 0


def same_bits(a, b):
    """NaN positions equal and every other value bitwise equal (+0 and -0 differ)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


def planted_samples(n, pixels, seed):
    """[pixels, n] integer-valued samples (tie-rich) with planted outliers, all-equal pixels and two-valued pixels."""
    rng = np.random.default_rng(seed)
    x = np.round(rng.normal(300.0, 12.0, (pixels, n)))
    x[rng.random((pixels, n)) < 0.08] += 150.0
    x[rng.random((pixels, n)) < 0.04] *= 0.2
    x = np.round(x)
    x[3::17] = 250.0                                               # all-equal pixels
    two = rng.random((pixels, n)) < 0.5
    x[5::19] = np.where(two, 100.0, 400.0)[5::19]                  # two-valued pixels
    return x


def volume_case(shape, groups, seed, dropout_group=None):
    """(dwi [..., n], b0 [...]) with integer-valued signal, planted dropouts (in ``dropout_group`` the whole group is hit at some
    pixels), pixels with b0 == 0 and dwi == 0, and one negative value."""
    rng = np.random.default_rng(seed)
    lead, n = tuple(shape[:-1]), shape[-1]
    b0 = np.round(rng.uniform(600.0, 1200.0, lead))
    dwi = np.round(b0[..., None] * rng.uniform(0.25, 0.45, lead + (1,)) * (1 + 0.03 * rng.standard_normal(lead + (n,))))
    drop = rng.random(lead + (n,)) < 0.06
    dwi[drop] = np.round(dwi[drop] * 0.15)
    if dropout_group is not None:
        first = int(np.sum(groups[:dropout_group]))
        hit = rng.random(lead) < 0.3
        sl = slice(first, first + groups[dropout_group])
        dwi[..., sl] = np.where(hit[..., None], np.round(dwi[..., sl] * 0.1), dwi[..., sl])
    flat_b0, flat = b0.reshape(-1), dwi.reshape(-1, n)
    flat_b0[1] = 0.0                                               # b0 == 0 with signal
    flat_b0[2] = 0.0
    flat[2] = 0.0                                                  # b0 == 0 and dwi == 0
    flat[4, 0] = 0.0                                               # one zero acquisition
    flat[6, n - 1] = -7.0                                          # a negative value: log of a negative number
    return dwi, b0
