"""The bounds and case tables of gemm_f32_common.py, checked without a GPU: an fp32 emulation of every case (one rounding per
term, two random k orders) stays inside the bounds with a wide margin, planted defects of the kinds kernels have leave them on
most of the elements they touch, and the restated dispatch rule covers every kernel family under every layout and epilogue.
This is the evidence that test_gpu_gemm_f32.py would notice a subtly wrong kernel, and would not flag a right one."""
import numpy as np
import pytest

import gemm_f32_common as G

F32, F64 = np.float32, np.float64
OPS = ("forward", "input_grad", "param_grad")


def _ab(c, d):
    """The contraction as A[M, K], B[N, K] in float64."""
    a, b = (d[k].astype(F64) for k in G.operands(c, d))
    if c.op in ("forward", "tanh"):
        return a, b
    if c.op == "input_grad":
        return a, b.T
    return a.T, b.T


def _dot(A, B, ks):
    acc = np.zeros((A.shape[0], B.shape[0]), F32)
    for k in ks:        # fp32 accumulator, exact product, one rounding per term
        acc = (acc.astype(F64) + np.outer(A[:, k], B[:, k])).astype(F32)
    return acc


def emulate(c, d, rng, A=None, B=None, drop_last=False):
    """fp32 result of the case's contraction in a random k order; a row-split parameter gradient sums its slabs in order."""
    if A is None:
        A, B = _ab(c, d)
    K = A.shape[1]
    ranges = G.split_ranges(c.n, G.param_splits(c.n, c.in_f, c.out_f)) if c.op == "param_grad" else [(0, K)]
    total = None
    for lo, hi in ranges:
        ks = lo + rng.permutation(hi - lo)
        if drop_last:
            ks = ks[ks != K - 1]
        part = _dot(A, B, ks)
        total = part if total is None else (total.astype(F64) + part).astype(F32)
    return total


def _fp32_epilogues(c, r, z):
    """The epilogues in fp32 numpy on the emulated accumulator ``z``: {output name: value}."""
    d, out = r["inputs"], {}
    if c.op == "input_grad":
        out["plain"] = z
        out["mul"] = z * d["mul"]
        return out
    for name, bias in (("", d["b"]), ("_nobias", np.zeros_like(d["b"]))):
        if c.op == "forward":
            arg = F32(G.OMEGA) * (z + bias)
            out["act" + name] = np.sin(arg.astype(F64)).astype(F32)         # (a correctly rounded sine: inside the 5e-7 allowance)
            out["dact" + name] = F32(G.OMEGA) * np.cos(arg.astype(F64)).astype(F32)
        else:
            t = np.tanh((z + bias).astype(F64)).astype(F32)
            out["act" + name] = F32(G.TANH_SCALE) * t
            out["dact" + name] = F32(G.TANH_SCALE) * (F32(1) - t * t)
    return out


@pytest.mark.parametrize("op", ("forward", "tanh", "input_grad", "param_grad"))
def test_fp32_emulation_stays_inside_the_bounds(op):
    worst = 0.0
    for c in G.cases(op):
        r = G.reference(c)
        rng = np.random.default_rng(7)
        for _ in range(2):
            z = emulate(c, r["inputs"], rng)
            bad, _ = G.excess(z, r["Z"], r["dzb"])
            assert bad == 0, c
            worst = max(worst, G.worst_ratio(z, r["Z"], r["S"]))
            if op != "param_grad":
                for name, got in _fp32_epilogues(c, r, z).items():
                    want, bound = r["out"][name]
                    assert G.excess(got, want, bound)[0] == 0, (c, name)
                    if op == "input_grad":      # the column sums, summed in fp32 row after row
                        s = np.zeros(got.shape[1], F32)
                        for row in got:
                            s = s + row
                        want, bound = r["out"]["gb_" + name]
                        assert G.excess(s, want, bound)[0] == 0, (c, "gb_" + name)
    print(f"{op}: largest err / (u * S) of the emulation = {worst:.2f} (allowed: 2 * (K + 4), K >= 1)")


def _defects(c, z):
    """[(name, corrupted copy, mask of the affected elements)] of an emulated result ``z``."""
    out = []
    M, N = z.shape
    if N >= 2:
        out.append(("shifted by one column", np.roll(z, 1, axis=1), np.ones_like(z, bool)))
    if M >= 2:
        row = M // 2 if M // 2 + 1 < M else 0
        bad, mask = z.copy(), np.zeros_like(z, bool)
        bad[row] = z[row + 1]
        mask[row] = True
        out.append(("one row taken from its neighbour", bad, mask))
    return out


@pytest.mark.parametrize("op", OPS)
def test_planted_defects_break_the_bounds(op):
    """Each defect leaves the bound on at least half of the elements it touches, in every case it applies to (a swap needs two
    k, a shift two columns, a row copy two rows)."""
    shares = {}
    for c in G.cases(op):
        r = G.reference(c)
        d = r["inputs"]
        rng = np.random.default_rng(11)
        A, B = _ab(c, d)
        K = A.shape[1]
        planted = _defects(c, emulate(c, d, rng))
        everywhere = np.ones_like(r["Z"], bool)
        planted.append(("last k term dropped", emulate(c, d, rng, drop_last=True), everywhere))
        if K >= 2:
            A2 = A.copy()
            A2[:, [K - 2, K - 1]] = A[:, [K - 1, K - 2]]
            planted.append(("two k columns of A swapped", emulate(c, d, rng, A2, B), everywhere))
        for name, bad, mask in planted:
            err = np.abs(bad.astype(F64) - r["Z"])
            share = float((err > r["dzb"])[mask].mean())
            shares.setdefault(name, []).append(share)
            assert share >= 0.5, (c, name, share)
    for name, s in shares.items():
        print(f"{op}: {name}: detected on {min(s):.2f} .. {max(s):.2f} of the affected elements")


@pytest.mark.parametrize("op", ("forward", "tanh"))
def test_planted_float4_epilogue_overrun_breaks_the_bounds(op):
    """The width class N % 4 != 0 on a float4 epilogue: the lane that holds the last two columns of a row also writes the first two
    of the next row, from a zero accumulator and a bias read past its end (taken as 0): act(row + 1, 0..1) = activation(0)."""
    for c in (c for c in G.cases(op) if c.group == "width"):
        r = G.reference(c)
        z = emulate(c, r["inputs"], np.random.default_rng(3))
        for name in ("act", "dact"):
            got = _fp32_epilogues(c, r, z)[name].copy()
            want, bound = r["out"][name]
            assert G.excess(got, want, bound)[0] == 0
            at_zero = {"act": 0.0, "dact": G.OMEGA if op == "forward" else G.TANH_SCALE}[name]
            got[1:, 0:2] = at_zero
            share = float((np.abs(got.astype(F64) - want) > bound)[1:, 0:2].mean()) if c.n > 1 else 1.0
            assert share >= 0.5, (c, name, share)


def test_param_splits_of_the_table():
    for in_f, out_f in G.PARAM_WIDTHS:
        assert [G.param_splits(n, in_f, out_f) for n in G.PARAM_ROWS] == [1, 1, 4, 9]
    assert G.split_ranges(2081, 9)[-1] == (2048, 2081)      # the last slab: one full K-step and a one-row K-step
    assert G.split_ranges(1000, 4) == [(0, 256), (256, 512), (512, 768), (768, 1000)]


def test_expected_family_rule():
    f = G.expected_family
    assert f("forward", 129, 96, 132) == "f32_pipe16" and f("forward", 129, 96, 132, key1=0) == "f32_pipe"
    assert f("forward", 129, 96, 132, key0=1) == "f32_generic" and f("forward", 129, 96, 132, aligned=False) == "f32_generic"
    # the float4 epilogue needs N % 4 == 0: forward N = out_f (no other condition looked at it before)
    assert all(f(op, 129, 32, o) == "f32_generic" for op in ("forward", "tanh") for o in (30, 50, 130))
    assert f("forward", 5, 36, 64) == "f32_generic" and f("input_grad", 5, 64, 36) == "f32_generic"     # K % 32
    assert f("input_grad", 5, 64, 32) == "f32_pipe16" and f("input_grad", 5, 130, 32) == "f32_generic"
    assert f("param_grad", 1, 32, 64) == "f32_pipe16" and f("param_grad", 77, 7, 30) == "f32_generic"


def test_tables_reach_every_kernel_layout_and_epilogue():
    """Each of the three families, the generic one with vector and with scalar loads, is launched under every (layout, epilogue)
    pair the entry points can reach; every value the issue of this table names occurs."""
    for op, variants in G.VARIANTS.items():
        for family, loads in (("f32_pipe16", True), ("f32_pipe", True), ("f32_generic", True), ("f32_generic", False)):
            seen = set()
            for c, v, k0, k1 in G.runs(op, family):
                al = G.all_aligned(c, v)
                assert G.expected_family(op, c.n, c.in_f, c.out_f, al, k0, k1) == family
                if G.vector_loads(op, c.in_f, c.out_f, al and c.misalign not in ("a", "b")) == loads:
                    seen.add(v)
            assert seen == set(variants), (op, family, loads)
    for op in ("forward", "tanh", "input_grad"):
        fast = [c for c in G.cases(op) if c.group == "fast"]
        dims = [G.gemm_dims(op, c.n, c.in_f, c.out_f) for c in fast]
        assert {m for m, _, _ in dims} == {1, 63, 64, 65, 127, 128, 129, 257}
        assert {k for _, _, k in dims} == {32, 64, 96, 160}
        assert {n for _, n, _ in dims} == {4, 8, 60, 64, 68, 128, 132, 260}
        assert {(1, 4, 32), (129, 132, 96), (257, 260, 160)} <= set(dims)
        assert {c.in_f for c in G.cases(op) if c.group == "scalar"} == {1, 7, 33}
        assert {c.out_f for c in G.cases(op) if c.group == "scalar"} == {1, 3, 30, 130}
    for op in ("forward", "tanh"):
        width = {(c.n, c.in_f, c.out_f) for c in G.cases(op) if c.group == "width"}
        assert width == {(n, i, o) for n in (5, 129) for i in (32, 64) for o in (30, 50, 130)}
        assert all(G.expected_family(op, *s) == "f32_generic" for s in width)
