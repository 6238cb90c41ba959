"""-m gpu: the three exact-fp32 GEMM kernels of csrc/gemm_f32.hip (gemm_f32_pipe16_kernel, gemm_f32_pipe_kernel behind
switch 1, gemm_f32_kernel with vector and with scalar loads), one contraction per call through the stand-alone layer entry
points, every output compared ELEMENT BY ELEMENT with float64 under the a-priori bounds of gemm_f32_common.py, and the launch
family of every call asserted against the restated host rule.  Switch 3 stays at its default, so no call takes the split-fp16
kernels.  test_gemm_f32_cpu.py shows what these bounds let through and what they catch.

Measured on an MI355X (gfx950), largest err / (u * S') over all cases, S' = the abs-sum of the contraction times the factors the
epilogue applies (the allowed figure is 2 * (K + 4) plus the epilogue's terms), and the largest err / bound:

  operation    kernel        calls   err / (u * S')   err / bound
  forward      f32_pipe16       50        3.97          0.049
  forward      f32_pipe         50        4.21          0.042
  forward      f32_generic     144      214.05          0.317
  tanh         f32_pipe16       50        4.16          0.039
  tanh         f32_pipe         50        3.77          0.040
  tanh         f32_generic     144      764.62          0.114
  input_grad   f32_pipe16       50        4.90          0.049
  input_grad   f32_pipe         50        4.90          0.048
  input_grad   f32_generic     100        4.90          0.135
  param_grad   f32_pipe16       16        5.48          0.082
  param_grad   f32_pipe         16        5.48          0.082
  param_grad   f32_generic      28        7.19          0.082

(The two large ratios belong to in_features = 1: S is one small product there, and the error is the absolute 3e-7 of the fast
sin/cos, or one ulp of tanhf, not the contraction's.)  The libm redo: sin within 8.7e-8, omega * cos within 2.1e-6 on both
pipelined kernels.  Siren(64, 50, 1, 1) / Siren(32, 130, 2, 1) on 129 rows: forward rel-L2 1.2e-7 / 4.0e-7, largest
|dy| / max|y| 1.9e-7 / 4.7e-7, gradients of the fused step rel-L2 1.5e-7 against float64 autograd.
"""
import numpy as np
import pytest
import torch

import gemm_f32_common as G
from mri_super_resolution_amd import ops

pytestmark = pytest.mark.gpu

FAMILIES = ("f32_pipe16", "f32_pipe", "f32_generic")
OPS = ("forward", "tanh", "input_grad", "param_grad")


def dev(a, misaligned=False):
    """The array on the device; ``misaligned``: starting 4 bytes into a 16-byte line (a slice of a 1-D buffer, viewed as the
    matrix: contiguous)."""
    a = np.ascontiguousarray(a, np.float32)
    if not misaligned:
        return torch.from_numpy(a).cuda()
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device="cuda")
    t = buf[1:1 + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


def host(t):
    return t.detach().cpu().numpy()


def device_inputs(c, d=None):
    d = G.reference(c)["inputs"] if d is None else d
    first, second = G.operands(c, d)
    wrong = {"a": first, "b": second, "bias": "b", "mul": "mul"}.get(c.misalign)
    return {k: dev(v, k == wrong) for k, v in d.items()}


def call(c, v, t):
    """One call of the entry point of the case; {output name of the reference: device tensor}."""
    tag = "" if v.bias else "_nobias"
    if c.op in ("forward", "tanh"):
        fn, scale = (ops.sine_layer_forward, G.OMEGA) if c.op == "forward" else (ops.tanh_layer_forward, G.TANH_SCALE)
        act, dact = fn(t["x"], t["W"], t["b"] if v.bias else None, scale, v.main)
        assert (dact is not None) == v.main
        return {"act" + tag: act, **({"dact" + tag: dact} if v.main else {})}
    if c.op == "input_grad":
        out = dev(np.zeros((c.n, c.in_f)), True) if c.misalign == "out" else None
        res = ops.sine_layer_backward_input(t["dz"], t["W"], t["mul"] if v.main else None, out=out, need_bias=v.bias)
        name = "mul" if v.main else "plain"
        return {name: res[0], "gb_" + name: res[1]} if v.bias else {name: res}
    gW, gb = ops.linear_param_grad(t["dz"], t["x"], v.bias)
    assert (gb is not None) == v.bias
    return {"gW": gW, **({"gb": gb} if v.bias else {})}


def ratio_scale(c, r, name):
    """S' of an output: the abs-sum of the contraction times the factors the epilogue applies (None for the bias sums)."""
    S = r["S"]
    if name.startswith("gb"):
        return None
    if c.op == "forward":
        return S * (G.OMEGA ** 2 if name.startswith("dact") else G.OMEGA)
    if c.op == "tanh":
        return S * G.TANH_SCALE * (2 if name.startswith("dact") else 1)
    if name == "mul":
        return S * np.abs(r["inputs"]["mul"].astype(np.float64))
    return S


def run_switched(k0, k1, fn):
    """``fn()`` under switches 0 and 1, with the launch counters of that call alone."""
    with ops.debug_switch(0, k0), ops.debug_switch(1, k1):
        ops.launch_counts_reset()
        out = fn()
        counts = ops.launch_counts()
    return out, counts


def assert_family(counts, family, what):
    assert counts["h3"] == 0, (what, counts)
    got = {f: counts[f] for f in FAMILIES}
    assert got == {f: int(f == family) for f in FAMILIES}, (what, family, got)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("op", OPS)
def test_every_case_against_float64(op, family):
    """Every case and variant of the table that must launch ``family``: exactly one launch of it and none of the other two, every
    output inside its bound element by element, and the same bits on a second call."""
    assert ops.debug_get(3) == 1
    table = G.runs(op, family)
    assert table
    worst_ratio, worst_excess, failures, tensors = 0.0, 0.0, [], {}
    try:
        for c, v, k0, k1 in table:
            if c not in tensors:
                tensors = {c: device_inputs(c)}
            r = G.reference(c)
            what = (tuple(c), tuple(v), k0, k1)
            out, counts = run_switched(k0, k1, lambda: call(c, v, tensors[c]))
            again, _ = run_switched(k0, k1, lambda: call(c, v, tensors[c]))
            assert_family(counts, family, what)
            for name, got in out.items():
                want, bound = r["out"][name]
                assert tuple(got.shape) == want.shape, (what, name)
                assert torch.equal(got, again[name]), (what, name, "second call differs")
                g = host(got)
                bad, ex = G.excess(g, want, bound)
                worst_excess = max(worst_excess, ex)
                scale = ratio_scale(c, r, name)
                if scale is not None:
                    worst_ratio = max(worst_ratio, G.worst_ratio(g, want, scale))
                if bad:
                    failures.append((what, name, bad, ex))
    finally:
        print(f"\n{op} on {family}: {len(table)} calls, largest err / (u * S') = {worst_ratio:.2f}, "
              f"largest err / bound = {worst_excess:.4f}")
    assert not failures, failures[:8]


@pytest.mark.parametrize("family", FAMILIES)
def test_input_grad_in_place_has_the_bits_of_out_of_place(family):
    """``out=dact_prev``: the epilogue reads the factor and writes the product at the same address."""
    table = [(c, v, k0, k1) for c, v, k0, k1 in G.runs("input_grad", family) if v.main and c.misalign is None]
    assert table
    for c, v, k0, k1 in table:
        t = device_inputs(c)

        def in_place():
            dp = t["mul"].clone()
            res = ops.sine_layer_backward_input(t["dz"], t["W"], dp, out=dp, need_bias=v.bias)
            return (res[0], res[1]) if v.bias else (res, None)

        (got, gb), counts = run_switched(k0, k1, in_place)
        want, _ = run_switched(k0, k1, lambda: call(c, v, t))
        assert_family(counts, family, tuple(c))
        assert torch.equal(got, want["mul"]), tuple(c)
        if v.bias:
            assert torch.equal(gb, want["gb_mul"]), tuple(c)


def test_zero_rows_launch_nothing():
    W = dev(np.ones((8, 32)))
    b = dev(np.zeros(8))
    x = torch.empty((0, 32), dtype=torch.float32, device="cuda")
    dz = torch.empty((0, 8), dtype=torch.float32, device="cuda")
    ops.launch_counts_reset()
    for fn in (ops.sine_layer_forward, ops.tanh_layer_forward):
        act, dact = fn(x, W, b, 30.0, True)
        assert tuple(act.shape) == (0, 8) and tuple(dact.shape) == (0, 8)
    out = ops.sine_layer_backward_input(dz, W, x.clone())
    out2, gb = ops.sine_layer_backward_input(dz, W, None, need_bias=True)
    assert tuple(out.shape) == (0, 32) and tuple(out2.shape) == (0, 32)
    assert tuple(gb.shape) == (32,) and torch.count_nonzero(gb) == 0
    assert sum(ops.launch_counts().values()) == 0


@pytest.mark.parametrize("family", ("f32_pipe16", "f32_pipe"))
def test_libm_redo_of_a_wave_tile(family):
    """One row whose arguments leave the fast sin/cos range (|omega * z| up to 3.9e6 > INR_SINCOS_FAST_LIMIT): the staged
    epilogue redoes the wave's tile through libm.  z of that row is exact (one non-zero term), so the row must match sin / omega *
    cos of the fp32 product omega * z to the 1e-6 test_sincos_accuracy allows beyond the fast range; every other row keeps the
    ordinary bound."""
    n, in_f, out_f, row = 130, 32, 64, 5
    rng = np.random.default_rng(5)
    x = (rng.random((n, in_f)) * 2 - 1).astype(np.float32)
    x[row] = 0
    x[row, 0] = 2.0 ** 16
    W = ((rng.random((out_f, in_f)) * 2 - 1) * (2.0 / in_f)).astype(np.float32)
    W[:, 0] = rng.integers(-128, 129, out_f) / 64.0
    W[0, 0], W[1, 0] = 2.0, -2.0
    b = np.zeros(out_f, np.float32)
    k0, k1 = G.KERNEL_SWITCHES[family]
    (act, dact), counts = run_switched(k0, k1, lambda: ops.sine_layer_forward(dev(x), dev(W), dev(b), G.OMEGA, True))
    assert_family(counts, family, "libm redo")
    act, dact = host(act), host(dact)
    Z, S, K = G.contraction("forward", x, W)
    arg = (np.float32(G.OMEGA) * (x[row, 0] * W[:, 0])).astype(np.float64)      # both products exact or rounded once, as on the device
    assert np.abs(arg).max() > 3.9e6 and (np.abs(arg) < 2.0 ** 20).any()
    e_s, e_c = np.abs(act[row] - np.sin(arg)).max(), np.abs(dact[row] - G.OMEGA * np.cos(arg)).max()
    print(f"\nlibm redo on {family}: row {row} sin err {e_s:.2e}, omega*cos err {e_c:.2e}")
    assert e_s <= 1e-6 and e_c <= 1e-6 * G.OMEGA
    rest = np.arange(n) != row
    dzb = G.bound_plain(S, K)
    assert G.excess(act[rest], np.sin(G.OMEGA * Z)[rest], G.bound_sine_act(dzb, Z, 0.0)[rest])[0] == 0
    assert G.excess(dact[rest], (G.OMEGA * np.cos(G.OMEGA * Z))[rest], G.bound_sine_dact(dzb, Z, 0.0)[rest])[0] == 0


@pytest.mark.parametrize("family", FAMILIES)
def test_nan_row_stays_in_its_row(family):
    """A NaN in one input row: NaN in exactly that output row, every other row inside its bound."""
    k0, k1 = G.KERNEL_SWITCHES[family]
    row = 7
    for op in ("forward", "tanh", "input_grad"):
        c = G.Case(op, 130, 32, 64, None, "nan") if op != "input_grad" else G.Case(op, 130, 64, 32, None, "nan")
        d = {k: v.copy() for k, v in G.make_inputs(c).items()}
        a, bname = G.operands(c, d)
        d[a][row, 3] = np.nan
        v = G.VARIANTS[op][2] if op != "input_grad" else G.VARIANTS[op][0]        # with stash and bias / with the factor
        t = device_inputs(c, d)
        out, counts = run_switched(k0, k1, lambda: call(c, v, t))
        assert_family(counts, family, (op, "nan"))
        clean = G.reference(c)                                   # the same inputs without the NaN: rows are independent
        rest = np.arange(c.n) != row
        for name, got in out.items():
            g = host(got)
            want, bound = clean["out"][name]
            assert np.isnan(g[row]).all(), (op, name)
            assert G.excess(g[rest], want[rest], bound[rest])[0] == 0, (op, name)


@pytest.mark.parametrize("fin,hidden,layers", [(64, 50, 1), (32, 130, 2)])
def test_networks_of_the_cut_width_class_end_to_end(fin, hidden, layers):
    """Networks whose first layer is fast-shaped (in_features % 32 == 0) and whose hidden width is no multiple of 4: whole forward
    and one fused lr = 0 step against the float64 oracle and float64 autograd on the same weights, y element by element (a
    corrupted activation column moves y by a large fraction of max|y|, rounding by ~1e-6 of it), and the families that ran."""
    import mri_super_resolution_amd as inr
    from oracle import inr_oracle as O
    n, T1, T2 = 129, 1e-5, 1e-5
    torch.manual_seed(fin + hidden)
    net = inr.Siren(fin, hidden, layers, 1).cuda()
    x = (torch.rand(n, fin, device="cuda") * 2 - 1).contiguous()
    t = torch.rand(n, 1, device="cuda")
    fitter = inr.SirenFitter(net, lr=0.0)
    n_sine = layers + 1

    def only_generic(counts, launches):
        assert {k: v for k, v in counts.items() if v} == {"f32_generic": launches}, counts

    ops.launch_counts_reset()
    loss = fitter.step(x, t.reshape(-1), n_steps=1)
    only_generic(ops.launch_counts(), 3 * n_sine - 1)            # forward and parameter gradient per layer, input gradient below the first
    desc, flat = inr.flat_parameters(net)
    ops.launch_counts_reset()
    got = host(ops.siren_forward(desc, flat, x))
    only_generic(ops.launch_counts(), n_sine)

    ws = [host(p) for p in net.layer_parameters()[0::2]]
    bs = [host(p) for p in net.layer_parameters()[1::2]]
    want = O.siren_forward(ws, bs, host(x).astype(np.float64), dtype=np.float64)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"\nSiren({fin}, {hidden}, {layers}, 1): forward rel-L2 {O.rel_l2(got, want):.2e}, max |dy| / max|y| {err:.2e}")
    assert O.rel_l2(got, want) < T1
    assert err <= 1e-4

    # float64 autograd on the same weights
    p64 = [torch.from_numpy(a.astype(np.float64)).requires_grad_() for pair in zip(ws, bs) for a in pair]
    a = torch.from_numpy(host(x).astype(np.float64))
    for l in range(n_sine):
        a = torch.sin(30.0 * (a @ p64[2 * l].T + p64[2 * l + 1]))
    y = a @ p64[-2].T + p64[-1]
    assert np.abs(y.detach().numpy() - want).max() <= 1e-10 * np.abs(want).max()      # the two float64 references agree
    l64 = ((y - torch.from_numpy(host(t).astype(np.float64))) ** 2).mean()
    l64.backward()
    auto = torch.cat([p.grad.reshape(-1) for p in p64])
    fused = torch.cat([fitter.grads[o:o + p.numel()] for (wo, bo), pw, pb in
                       zip(fitter.offsets, net.layer_parameters()[0::2], net.layer_parameters()[1::2])
                       for o, p in ((wo, pw), (bo, pb))]).double().cpu()
    g_err = ((fused - auto).norm() / auto.norm()).item()
    print(f"fused step: loss rel err {abs(loss[0].item() - l64.item()) / l64.item():.2e}, gradient rel-L2 {g_err:.2e}")
    assert abs(loss[0].item() - l64.item()) <= T2 * l64.item()
    assert g_err < T2
