"""Float64 references, a-priori element-wise bounds and the case tables of the exact-fp32 GEMM tests (csrc/gemm_f32.hip).
Plain numpy, no GPU: imported by test_gemm_f32_cpu.py (which checks the bounds and the tables themselves) and by
test_gpu_gemm_f32.py (which holds the three kernels to them).

Three contractions, named as the entry points name them (``n`` rows, ``in_f`` / ``out_f`` layer widths):

  forward / tanh   C[n, out_f] = x[n, in_f] W[out_f, in_f]^T      K = in_f    A, B k-contiguous
  input_grad       C[n, in_f]  = dz[n, out_f] W[out_f, in_f]      K = out_f   A k-contiguous, B n-contiguous
  param_grad       C[out_f, in_f] = dz[n, out_f]^T x[n, in_f]     K = n       A m-contiguous, B n-contiguous

Every bound below is derived, none is measured: any summation order of K fp32 products with fp32 accumulation satisfies
|fl - Z| <= gamma_K * S with S the same contraction over absolute values; ``2 * (K + 4) * u * S`` doubles gamma_K for a matrix unit
that rounds its internal additions toward zero instead of to nearest.  The epilogue rows add the roundings the epilogue performs
(one per fp32 operation) and the stated figure of the device function: 5e-7 for the fast sin/cos (test_gpu_parity.py:
test_sincos_accuracy asserts it up to 3e6), 4 ulp of 1 for tanhf (the project states no figure for it, and the HIP documentation
installed next to the compiler holds none either).
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
SINCOS_ABS = 5e-7
TANH_ABS = 4 * 2.0 ** -23
OMEGA = 30.0
TANH_SCALE = 0.75
BM = BN = 128
BK = 32


# ---- references -----------------------------------------------------------------------------------------------------------------
def contraction(op, a, b):
    """(Z, S, K) in float64 of the contraction ``op`` over the fp32 operands ``a``, ``b`` (x, W / dz, W / dz, x)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if op in ("forward", "tanh"):
        return a @ b.T, np.abs(a) @ np.abs(b).T, a.shape[1]
    if op == "input_grad":
        return a @ b, np.abs(a) @ np.abs(b), a.shape[1]
    if op == "param_grad":
        return a.T @ b, np.abs(a).T @ np.abs(b), a.shape[0]
    raise ValueError(op)


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
def bound_plain(S, K):
    return 2 * (K + 4) * U * S


def bound_param(S, n, splits):
    """Row-split parameter gradient: the slab reduction adds at most ``splits`` roundings."""
    return 2 * (n + splits + 4) * U * S


def bound_mul(dzb, Z, mul):
    mul = np.asarray(mul, np.float64)
    return dzb * np.abs(mul) + U * np.abs(Z * mul)


def bound_sine_act(dzb, Z, b, w=OMEGA):
    return abs(w) * (dzb + 2 * U * (np.abs(Z) + np.abs(b))) + U * np.abs(w * (Z + b)) + SINCOS_ABS


def bound_sine_dact(dzb, Z, b, w=OMEGA):
    return abs(w) * bound_sine_act(dzb, Z, b, w) + U * abs(w)


def bound_tanh_act(dzb, Z, b, scale=TANH_SCALE):
    return abs(scale) * (dzb + U * (np.abs(Z) + np.abs(b))) + TANH_ABS * abs(scale)


def bound_tanh_stash(dzb, Z, b, scale=TANH_SCALE):
    return abs(scale) * (2 * (dzb + U * (np.abs(Z) + np.abs(b))) + 2 * TANH_ABS)


def bound_colsum(elem_bound, elem, n):
    """Bias sums (fused epilogue or the column-sum pass) of an [n, C] output with element bound ``elem_bound``."""
    return elem_bound.sum(0) + 2 * (n + 4) * U * np.abs(elem).sum(0)


def bound_colsum_input(dz, n):
    """gb = colsum(dz) of exact fp32 inputs."""
    return 2 * (n + 4) * U * np.abs(np.asarray(dz, np.float64)).sum(0)


# ---- the host rule, restated ----------------------------------------------------------------------------------------------------
def gemm_dims(op, n, in_f, out_f):
    """(M, N, K) of the launch."""
    return {"forward": (n, out_f, in_f), "tanh": (n, out_f, in_f), "input_grad": (n, in_f, out_f),
            "param_grad": (out_f, in_f, n)}[op]


def vector_loads(op, in_f, out_f, aligned=True):
    """``vec_ok`` of the entry points: both operands on 16 bytes, leading dimensions and contiguous extents multiples of 4."""
    if op in ("forward", "tanh"):
        return aligned and in_f % 4 == 0
    return aligned and in_f % 4 == 0 and out_f % 4 == 0


def expected_family(op, n, in_f, out_f, aligned=True, key0=0, key1=1):
    """The launch family ``launch_gemm`` (csrc/gemm_f32.hip) chooses for a stand-alone call with switch 3 at its default.
    A RESTATEMENT of that host rule, which must move with it: fast = vector loads, an output the float4 epilogue can write
    (N % 4 == 0, ldc = N, every epilogue array on 16 bytes), K % 32 == 0 where an operand is k-contiguous, switch 0 off; then
    switch 1 picks between the two pipelined kernels.  ``aligned``: every array of the call starts on 16 bytes.  The 2 GiB
    operand-window branches are left out (they need multi-GiB operands)."""
    _, N, K = gemm_dims(op, n, in_f, out_f)
    fast = vector_loads(op, in_f, out_f, aligned) and aligned and N % 4 == 0 and not key0
    if op != "param_grad":
        fast = fast and K % BK == 0
    if not fast:
        return "f32_generic"
    return "f32_pipe16" if key1 else "f32_pipe"


def param_splits(n, in_f, out_f):
    """``param_grad_splits`` (csrc/gemm_f32.hip), restated; must move with it."""
    tiles = -(-out_f // BM) * -(-in_f // BN)
    ksteps = -(-n // BK)
    s = max(1, min(-(-1024 // tiles), (ksteps + 7) // 8, 512))
    widest = max(out_f, in_f)
    rows_max = ((1 << 31) - 1) // (widest * 4) // BK * BK
    need = -(-n // rows_max) if rows_max > 0 else 1 << 30
    return min(max(s, need), 1 << 20)


def split_ranges(n, splits):
    """Row ranges of the slabs (``gemm_param_grad_slabs``: whole K-steps per split)."""
    per = -(-(-(-n // BK)) // splits) * BK
    return [(s * per, min(n, (s + 1) * per)) for s in range(splits)]


# ---- cases ----------------------------------------------------------------------------------------------------------------------
# misalign: which array of the call starts 4 bytes into a 16-byte line ("a" / "b": first / second operand; "bias", "mul", "out")
Case = namedtuple("Case", "op n in_f out_f misalign group")
KERNEL_SWITCHES = {"f32_pipe16": (0, 1), "f32_pipe": (0, 0), "f32_generic": (1, 1)}    # (switch 0, switch 1) that select a kernel

# (rows, K, N): every row count of {1, 63, 64, 65, 127, 128, 129, 257}, every K-tile count 1, 2, 3, 5, every output width of
# {4, 8, 60, 64, 68, 128, 132, 260} (a lane group cut by N, a wave half outside N, two and three column tiles, tile edges)
FAST_TRIPLES = [(1, 32, 4), (63, 64, 8), (64, 32, 60), (65, 96, 64), (127, 64, 68), (128, 160, 128), (129, 96, 132),
                (257, 160, 260), (128, 32, 132), (64, 96, 260), (65, 160, 8), (1, 64, 128)]
VEC_TRIPLES = [(65, 4, 64), (129, 36, 132), (64, 40, 8)]                                  # K in {4, 36, 40}: vector loads, generic
SCALAR_SHAPES = [(5, 1, 1), (65, 7, 3), (129, 33, 30), (64, 7, 130), (130, 33, 130), (63, 1, 30)]   # (n, in_f, out_f)
PARAM_WIDTHS = [(32, 64), (68, 132), (7, 30)]                                             # (in_f, out_f)
PARAM_ROWS = {1: 1, 77: 1, 1000: 4, 2081: 9}                                              # rows -> splits the rule must give
WIDTH_CLASS = [(n, i, o) for o in (30, 50, 130) for i in (32, 64) for n in (5, 129)]      # the float4 epilogue cut by N


def _shape(op, n, K, N):
    return (n, K, N) if op in ("forward", "tanh") else (n, N, K)        # -> (n, in_f, out_f)


def cases(op):
    """The table of one operation."""
    out = []
    if op == "param_grad":
        for in_f, out_f in PARAM_WIDTHS:
            out += [Case(op, n, in_f, out_f, None, "rows") for n in PARAM_ROWS]
        out += [Case(op, 77, 32, 64, "a", "misaligned"), Case(op, 77, 32, 64, "b", "misaligned")]
        return out
    out += [Case(op, *_shape(op, *t), None, "fast") for t in FAST_TRIPLES]
    out += [Case(op, *_shape(op, *t), None, "vector") for t in VEC_TRIPLES]
    out += [Case(op, *s, None, "scalar") for s in SCALAR_SHAPES]
    extra = ("bias",) if op != "input_grad" else ("mul", "out")
    out += [Case(op, *_shape(op, 65, 64, 68), m, "misaligned") for m in ("a", "b") + extra]
    if op != "input_grad":
        out += [Case(op, *s, None, "width") for s in WIDTH_CLASS]
    return out


Variant = namedtuple("Variant", "epilogue main bias")
# what the entry points can reach.  forward / tanh: main = stash wanted, bias = a bias given; input_grad: main = dact_prev given,
# bias = need_bias; param_grad: bias = gb wanted
VARIANTS = {
    "forward": [Variant("sine", False, True), Variant("sine", False, False), Variant("sine_stash", True, True),
                Variant("sine_stash", True, False)],
    "tanh": [Variant("tanh", False, True), Variant("tanh", False, False), Variant("tanh_stash", True, True),
             Variant("tanh_stash", True, False)],
    "input_grad": [Variant("mul", True, False), Variant("mul", True, True), Variant("plain", False, False),
                   Variant("plain", False, True)],
    "param_grad": [Variant("plain", None, False), Variant("plain", None, True)],
}


def all_aligned(c, v):
    """Whether every array the launch touches starts on 16 bytes: a misplaced bias / factor counts only where it is passed."""
    if c.misalign == "bias":
        return not v.bias
    if c.misalign == "mul":
        return not v.main
    return c.misalign is None


def runs(op, family):
    """[(case, variant, switch 0, switch 1)] that must launch ``family``: a call that takes the default kernel runs under each of
    the three switch settings, every other call at the defaults."""
    out = []
    for c in cases(op):
        for v in VARIANTS[op]:
            al = all_aligned(c, v)
            if expected_family(c.op, c.n, c.in_f, c.out_f, al) == "f32_pipe16":
                out.append((c, v, *KERNEL_SWITCHES[family]))
            elif family == "f32_generic":
                out.append((c, v, 0, 1))
    return out


def _seed(c):
    return [{"forward": 1, "tanh": 2, "input_grad": 3, "param_grad": 4}[c.op], c.n, c.in_f, c.out_f,
            {None: 0, "a": 1, "b": 2, "bias": 3, "mul": 4, "out": 5}[c.misalign]]


def make_inputs(c):
    """fp32 inputs of a case.  x (and the stashed factor's sign) uniform in [-1, 1]; W scaled to |z| <= 2 so that |omega * z|
    stays below about 60; dz carries per-row magnitudes exp(2 * randn).  In a parameter-gradient case the LAST row carries the
    largest magnitude: the ragged tail of the row contraction is where a K-loop goes wrong, and a tail row far below the
    others would sit inside the a-priori bound whatever the kernel did with it."""
    rng = np.random.default_rng(_seed(c))
    f32 = np.float32
    d = {}
    if c.op in ("forward", "tanh"):
        d["x"] = (rng.random((c.n, c.in_f)) * 2 - 1).astype(f32)
        d["W"] = ((rng.random((c.out_f, c.in_f)) * 2 - 1) * (2.0 / c.in_f)).astype(f32)
        d["b"] = ((rng.random(c.out_f) * 2 - 1) * 0.5).astype(f32)
        return d
    mag = np.exp(2 * rng.standard_normal((c.n, 1)))
    if c.op == "param_grad":
        i = int(mag.argmax())
        mag[[i, -1]] = mag[[-1, i]]
    d["dz"] = (rng.standard_normal((c.n, c.out_f)) * mag).astype(f32)
    if c.op == "input_grad":
        d["W"] = ((rng.random((c.out_f, c.in_f)) * 2 - 1) * (2.0 / c.in_f)).astype(f32)
        d["mul"] = ((rng.random((c.n, c.in_f)) * 2 - 1) * OMEGA).astype(f32)
    else:
        d["x"] = (rng.random((c.n, c.in_f)) * 2 - 1).astype(f32)
    return d


def operands(c, d):
    return {"forward": ("x", "W"), "tanh": ("x", "W"), "input_grad": ("dz", "W"), "param_grad": ("dz", "x")}[c.op]


_REF = {}


def reference(c):
    """Inputs, float64 results and bounds of a case, computed once and shared (treat as read-only).  Keys: ``inputs``; ``Z``,
    ``S``, ``K``, ``dzb`` (bound of the plain contraction); then per output name -> (float64 value, bound)."""
    if c in _REF:
        return _REF[c]
    d = make_inputs(c)
    a, b = (d[k] for k in operands(c, d))
    Z, S, K = contraction(c.op, a, b)
    r = {"inputs": d, "Z": Z, "S": S, "K": K, "out": {}}
    o = r["out"]
    if c.op == "param_grad":
        r["splits"] = param_splits(c.n, c.in_f, c.out_f)
        r["dzb"] = bound_param(S, c.n, r["splits"])
        o["gW"] = (Z, r["dzb"])
        o["gb"] = (np.asarray(d["dz"], np.float64).sum(0), bound_colsum_input(d["dz"], c.n))
    else:
        r["dzb"] = dzb = bound_plain(S, K)
    if c.op == "forward":
        for name, bias in (("", np.asarray(d["b"], np.float64)), ("_nobias", np.zeros(c.out_f))):
            arg = OMEGA * (Z + bias)
            o["act" + name] = (np.sin(arg), bound_sine_act(dzb, Z, bias))
            o["dact" + name] = (OMEGA * np.cos(arg), bound_sine_dact(dzb, Z, bias))
    elif c.op == "tanh":
        for name, bias in (("", np.asarray(d["b"], np.float64)), ("_nobias", np.zeros(c.out_f))):
            t = np.tanh(Z + bias)
            o["act" + name] = (TANH_SCALE * t, bound_tanh_act(dzb, Z, bias))
            o["dact" + name] = (TANH_SCALE * (1 - t * t), bound_tanh_stash(dzb, Z, bias))
    elif c.op == "input_grad":
        m = np.asarray(d["mul"], np.float64)
        o["plain"] = (Z, dzb)
        o["mul"] = (Z * m, bound_mul(dzb, Z, m))
        for k in ("plain", "mul"):
            o["gb_" + k] = (o[k][0].sum(0), bound_colsum(o[k][1], o[k][0], c.n))
    _REF[c] = r
    return r


def worst_ratio(got, want, S):
    """Largest err / (u * S) over the elements with S > 0 (the figure the tests print)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    ok = S > 0
    return float((err[ok] / (U * S[ok])).max()) if ok.any() else 0.0


def excess(got, want, bound):
    """How many elements leave the bound (NaN counts as leaving it), and the worst err / bound."""
    err = np.abs(np.asarray(got, np.float64) - want)
    bad = ~(err <= bound)
    worst = float(np.nanmax(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    return int(bad.sum()), worst
