"""The PIA kernels (csrc/pia.hip) at every tile, split and row class of tests/pia_shapes_common.py against the float64
restatement of tests/pia_net_common.py, which tests/test_pia_shapes_cpu.py pins to the reference's own float64 run on every one
of these cases (1e-12).  tests/test_pia_shapes_cpu.py also proves which kernel form each case runs.

Bound per tensor: FACTOR x max(that tensor's `ref_err`, the median `ref_err` of the case's tensors of the same kind), where
`ref_err` is what the REFERENCE's float32 run deviates from its float64 copy on the same case (tests/golden/pia_net_shapes.npz,
max |a - ref| / max |ref|).  FACTOR is the 4 of tests/test_gpu_pia_net.py: another summation order in the MFMA tiles and the
hardware's exp / tanh.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

from mri_super_resolution_amd import ops, pia_net

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pia_net_common as C  # noqa: E402
import pia_shapes_common as S  # noqa: E402

pytestmark = pytest.mark.gpu
FACTOR = 4.0
OUTS = ("signal", "D", "T2", "v")
_ID = lambda c: c.name


def _model(case, g):
    b_values, te_values = case.tables
    torch.manual_seed(0)
    m = pia_net.PIA(hidden_dims=list(case.hidden), b_values=list(b_values), TE_values=list(te_values))
    host = [p.detach().cpu().clone() for p in m.parameters()]
    assert S.params_sha([p.numpy() for p in host]) == str(g[f"{case.name}/init_sha"])
    return m.cuda(), host


def _names(m):
    return [n for n, _ in m.named_parameters()]


class _Report:
    """Prints every deviation beside its bound, collects the misses, remembers the worst ratio."""

    def __init__(self, case):
        self.case, self.fails, self.worst = case, [], (0.0, 0.0, "")

    def check(self, name, got, want, bound):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        if np.isnan(bound):                      # a tensor the functional does not reach: float64 says zero, so must the kernels
            nz = int(np.count_nonzero(got))
            print(f"{self.case.name} {name}: unreached, {nz} non-zero elements")
            assert not np.any(want)
            if nz:
                self.fails.append((name, nz, 0))
            return
        dev = C.rel_dev(got, want)
        print(f"{self.case.name} {name}: deviation {dev:.3e}, bound {bound:.3e}")
        if dev / bound > self.worst[0] / max(self.worst[1], 1e-300):
            self.worst = (dev, bound, name)
        if not dev <= bound:
            self.fails.append((name, dev, bound))

    def done(self):
        print(f"{self.case.name} WORST: {self.worst[2]} deviation {self.worst[0]:.3e} of bound {self.worst[1]:.3e}")
        assert not self.fails, self.fails


def _autograd_pass(m, x, pids):
    for p in m.parameters():
        p.grad = None
    ops.launch_counts_reset()
    out = m(x)
    loss = m.loss_function(out[0], x, pids)
    loss.backward()
    counts = ops.pia_launch_counts()
    return [out[0].detach(), out[2].detach(), out[3].detach(), out[4].detach()], loss.detach(), [p.grad.detach().clone() for p in m.parameters()], counts


def _fused_pass(m, x, pids):
    fitter = pia_net.PiaFitter(m, lr=0.0)        # lr 0: the step leaves the parameters alone, its gradients stay
    ops.launch_counts_reset()
    loss = fitter.step(x, pids)
    counts = ops.pia_launch_counts()
    assert sum(ops.launch_counts().values()) == 0, ops.launch_counts()
    return loss.clone(), [t.clone() for t in fitter.state.split(fitter.grads)], counts


def _training(case, g, filtered):
    m, host = _model(case, g)
    b_values, te_values = case.tables
    x, pids, flagged = S.case_inputs(case, host, pia_net.get_batch, filtered=filtered)
    if filtered:
        print(f"{case.name}: {flagged} of {S.pool_rows(case.rows)} pool rows lie on a LeakyReLU kink at float32 resolution")
        assert flagged <= S.MAX_FLAGGED * S.pool_rows(case.rows)
    want_loss, want_g, want_out = C.loss_and_grads64(host, x, pids, b_values=b_values, te_values=te_values)
    xd, pd = x.cuda(), pids.cuda()
    outs, loss, auto_g, c_auto = _autograd_pass(m, xd, pd)
    outs2, loss2, auto_g2, _ = _autograd_pass(m, xd, pd)
    fused_loss, fused_g, c_fused = _fused_pass(m, xd, pd)
    fused_loss2, fused_g2, _ = _fused_pass(m, xd, pd)
    assert all(torch.equal(p.detach().cpu(), h) for p, h in zip(m.parameters(), host)), "lr = 0 moved a parameter"
    assert c_auto == {**c_auto, **S.launch_counts(case, fused=False)}, c_auto
    assert c_fused == {**c_fused, **S.launch_counts(case, fused=True)}, c_fused
    # a second run is bit-equal
    assert torch.equal(loss, loss2) and all(torch.equal(a, b) for a, b in zip(outs, outs2))
    assert all(torch.equal(a, b) for a, b in zip(auto_g, auto_g2))
    assert torch.equal(fused_loss, fused_loss2) and all(torch.equal(a, b) for a, b in zip(fused_g, fused_g2))
    print(f"{case.name} loss: f64 {want_loss.item():.9e}, autograd {loss.item():.9e}, fused {fused_loss.item():.9e}")
    assert abs(fused_loss.item() - want_loss.item()) <= 1e-5 * want_loss.item()
    assert abs(loss.item() - want_loss.item()) <= 1e-5 * want_loss.item()
    return m, host, x, pids, outs, auto_g, fused_g, want_out, want_g


@pytest.mark.parametrize("case", S.TRAIN_CASES, ids=_ID)
def test_training_case_against_float64(golden, case):
    """Forward outputs and every gradient, on the autograd pair and on the fused step with lr = 0.

    Fused versus autograd gradients: the two passes run the same GEMMs and the same fixed-order reductions on the same
    activations; they differ in d loss / d signal alone, which the fused row kernel forms in float64 from the float32
    residual and torch's autograd forms in float32 (three roundings per element).  Both are therefore within their bound of
    float64, and of each other within the two bounds added; the count of elements that differ bit for bit is printed."""
    g = golden("pia_net_shapes.npz")
    m, host, x, pids, outs, auto_g, fused_g, want_out, want_g = _training(case, g, filtered=True)
    rep = _Report(case)
    for k, got, want, b in zip(OUTS, outs, want_out, S.bounds(g[f"{case.name}/ref_err_out"], FACTOR)):
        rep.check(f"forward {k}", got.cpu().numpy(), want.numpy(), b)
    for n, ga, gf, gw, b in zip(_names(m), auto_g, fused_g, want_g, S.bounds(g[f"{case.name}/ref_err_grad"], FACTOR)):
        rep.check(f"grad autograd {n}", ga.cpu().numpy(), gw.numpy(), b)
        rep.check(f"grad fused {n}", gf.cpu().numpy(), gw.numpy(), b)
        differ = int((ga != gf).sum())
        dev = C.rel_dev(gf.cpu().numpy(), ga.cpu().numpy())
        print(f"{case.name} fused vs autograd {n}: {differ} of {ga.numel()} elements differ, deviation {dev:.3e}, bound {2 * b:.3e}")
        if not dev <= 2 * b:
            rep.fails.append((f"fused vs autograd {n}", dev, 2 * b))
    rep.done()


def test_gradients_on_an_unfiltered_batch_follow_float32(golden):
    """C at 65 rows WITHOUT the kink filter, so that an error of the kernels beside a kink cannot hide behind it: per tensor the
    kernels may deviate from float64 by the usual bound of the filtered case, or by twice what the same layers run in float32
    torch on the host deviate from float64 on this batch, whichever is larger (tests/test_gpu_pia_net.py,
    test_gradients_on_the_unfiltered_ragged_batch_follow_float32)."""
    g = golden("pia_net_shapes.npz")
    case = S.UNFILTERED
    m, host, x, pids, outs, auto_g, fused_g, want_out, want_g = _training(case, g, filtered=False)
    print(f"{case.name} unfiltered: {int(C.kink_rows(host, x).sum())} of {case.rows} rows on a kink")
    _, host32_g, _ = C.loss_and_grads64(host, x, pids, dtype=torch.float32)
    rep = _Report(case)
    for n, ga, gf, gw, g32, b in zip(_names(m), auto_g, fused_g, want_g, host32_g, S.bounds(g[f"{case.name}/ref_err_grad"], FACTOR)):
        host_dev = C.rel_dev(g32.numpy(), gw.numpy())
        print(f"unfiltered {n}: float32 on the host deviates {host_dev:.3e}")
        rep.check(f"unfiltered autograd {n}", ga.cpu().numpy(), gw.numpy(), max(b, 2.0 * host_dev))
        rep.check(f"unfiltered fused {n}", gf.cpu().numpy(), gw.numpy(), max(b, 2.0 * host_dev))
    rep.done()


@pytest.mark.parametrize("case", S.FORWARD_CASES, ids=_ID)
def test_forward_case_against_float64(golden, case):
    """`pia_forward` with its default chunk of 32,768 rows (A at 32,773 rows: every big FWD tile, then a 5-row tail chunk), and
    the one-layer encoders.  The output is bit-equal to the run in chunks of 4,096 rows, and to `model(x)` without autograd."""
    g = golden("pia_net_shapes.npz")
    m, host = _model(case, g)
    x, _, _ = S.case_inputs(case, host, pia_net.get_batch)
    want = C.forward64(host, x)
    m._state.ensure()
    xd = x.cuda()
    ops.launch_counts_reset()
    got = pia_net.pia_forward(m._state, xd)
    c = ops.pia_launch_counts()
    chunks = S.cdiv(case.rows, S.FWD_CHUNK)
    assert c["pia_fwd"] == chunks * (len(case.hidden) + 1) and c["pia_head"] == chunks and c["pia_dx"] == c["pia_dw"] == 0, c
    for other in (pia_net.pia_forward(m._state, xd, chunk_rows=4096), pia_net.pia_forward(m._state, xd)):
        assert all(torch.equal(a, b) for a, b in zip(got, other))
    with torch.no_grad():
        out = m(xd)
    assert all(torch.equal(a, b) for a, b in zip(got, (out[0], out[2], out[3], out[4])))
    rep = _Report(case)
    for k, a, w, b in zip(OUTS, got, want, S.bounds(g[f"{case.name}/ref_err_out"], FACTOR)):
        rep.check(f"forward {k}", a.cpu().numpy(), w.numpy(), b)
    rep.done()


@pytest.mark.parametrize("shape", ["A", "B"])
def test_external_gradients_against_float64(golden, shape):
    """`inr_pia_backward_train` under seeded linear functionals sum(w * out) of signal alone, D alone (float64 weights), T2
    alone, v alone and all four: the absent gradients reach the kernel as null pointers.  Every parameter gradient against
    float64 autograd on the restatement; a tensor the functional does not reach must be exactly zero.  The all-four gradient
    equals the sum of the four single ones to float32 rounding: each of the five is within its bound b_i max |g64_i| of
    float64, and the float64 gradients add up exactly, so |g_all - sum_i g_i| <= b_all max |g64_all| + sum_i b_i max |g64_i|."""
    g = golden("pia_net_shapes.npz")
    grads, wants, bnds = {}, {}, {}
    for f in S.FUNCTIONALS:
        case = S.BY_NAME[f"functional_{shape}_129_{f}"]
        m, host = _model(case, g)
        x, pids, flagged = S.case_inputs(case, host, pia_net.get_batch)
        w = S.functional_weights(case.rows, case.seed)
        _, want_g, _ = C.loss_and_grads64(host, x, pids, functional=S.functional64(f, w))
        ops.launch_counts_reset()
        out = m(x.cuda())
        named = dict(zip(OUTS, (out[0], out[2], out[3], out[4])))
        assert named["D"].dtype == torch.float64 and w["D"].dtype == torch.float64
        loss = sum((w[k].cuda() * named[k]).sum() for k in S.functional_terms(f))
        loss.backward()
        c = ops.pia_launch_counts()
        assert c == {**c, **S.launch_counts(case, fused=False)}, c
        grads[f] = [p.grad.detach().cpu().numpy().astype(np.float64) for p in m.parameters()]
        wants[f] = [t.numpy() for t in want_g]
        bnds[f] = S.bounds(g[f"{case.name}/ref_err_grad"], FACTOR)
        rep = _Report(case)
        for n, got, want, b in zip(_names(m), grads[f], wants[f], bnds[f]):
            rep.check(f"grad {n}", got, want, b)
        rep.done()
    singles = [f for f in S.FUNCTIONALS if f != "all"]
    fails = []
    for i, n in enumerate(_names(m)):
        total = sum(grads[f][i] for f in singles)
        tol = sum(0.0 if np.isnan(bnds[f][i]) else bnds[f][i] * np.abs(wants[f][i]).max() for f in S.FUNCTIONALS)
        diff = float(np.abs(grads["all"][i] - total).max())
        print(f"functional_{shape} sum of the four vs all, {n}: max |difference| {diff:.3e}, tolerance {tol:.3e}")
        if not diff <= tol:
            fails.append((n, diff, tol))
    assert not fails, fails


@pytest.mark.parametrize("npix", S.PIDS_PIXELS)
def test_pids_slice_at_block_boundaries(golden, npix):
    """`inr_pids_slice` on slices of shape (1, n) around its 256-pixel block, with zeros, negatives (NaN logarithm: both ADC
    flags 0), exact ties and values just below / above an integer: bit-equal to the reference's `detect_PIDS_slice`."""
    g = golden("pia_net_shapes.npz")
    S_in = S.pids_slice_input(npix)
    maps = pia_net.detect_PIDS_slice(np.array(C.B_VALUES, dtype=np.float64), S_in)
    for name, got in zip(("adc1", "adc2", "b_decay", "te_decay"), maps):
        want = g[f"pids_slice/{npix}/{name}"].astype(np.float64)
        assert got.dtype == np.float64 and got.shape == want.shape, name
        print(f"pids_slice[{npix}] {name}: {int((got != want).sum())} of {got.size} entries differ")
        assert np.array_equal(got, want), name
    nan_log = (S_in[0, :, :, 0] + 1e-7 < 0).any(axis=1)
    assert not maps[0][0][nan_log].any() and not maps[1][0][nan_log].any()
