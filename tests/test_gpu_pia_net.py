"""The PIA autoencoder kernels (csrc/pia.hip) against the float64 restatement of tests/pia_net_common.py -- itself pinned to
the reference's own float64 run by tests/test_pia_net_cpu.py -- and against the reference's recorded float32 trajectory.

Bounds: a tensor may deviate from float64 by at most 4 x what the REFERENCE's float32 run deviates from its float64 copy
(`ref_err/*` of tests/golden/pia_net.npz, max |a - ref| / max |ref| per tensor).  The factor covers another summation order
in the MFMA tiles and the hardware's exp / tanh.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

from mri_super_resolution_amd import ops, pia_net

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pia_net_common as C  # noqa: E402

pytestmark = pytest.mark.gpu
FACTOR = 4.0
TRAJ_RTOL = 1e-4      # the repository's bound for SIREN trajectories against the reference (test_trajectory_50_steps_fused_vs_reference)


def _model():
    torch.manual_seed(0)
    return pia_net.PIA().cuda()


def _host_params(m):
    return [p.detach().cpu().clone() for p in m.parameters()]


def _check(name, got, want, bound):
    dev = C.rel_dev(got, want)
    print(f"{name}: deviation {dev:.3e}, bound {bound:.3e}")
    return dev <= bound, (name, dev, bound)


def test_forward_against_float64(golden):
    g = golden("pia_net.npz")
    m = _model()
    x = torch.from_numpy(g["batch/x"])
    want = dict(zip(("signal", "D", "T2", "v"), C.forward64(_host_params(m), x)[0:4]))
    ops.launch_counts_reset()
    with torch.no_grad():
        signal, x_out, D, T2, v = m(x.cuda())
    c = ops.pia_launch_counts()
    assert c["pia_fwd"] == 6 and c["pia_head"] == 1 and c["pia_dx"] == c["pia_dw"] == 0, c
    assert sum(ops.launch_counts().values()) == 0, ops.launch_counts()
    assert x_out.is_cuda and torch.equal(x_out.cpu(), x)
    got = {"signal": signal, "D": D, "T2": T2, "v": v}
    assert [str(got[k].dtype) for k in got] == [str(g[f"dtype/{k}"]) for k in got]
    fails = []
    for k in got:
        ok, info = _check(f"forward {k}", got[k].cpu().numpy(), want[k].numpy(), FACTOR * float(g[f"ref_err/{k}"]))
        if not ok:
            fails.append(info)
    assert not fails, fails
    D_, T2_, v_ = m.encode(x.cuda())
    assert torch.equal(D_, D) and torch.equal(T2_, T2) and torch.equal(v_, v)


@pytest.mark.parametrize("rows", [512, 4096 + 77])
def test_gradients_against_float64(golden, rows):
    """Autograd path (forward_train / backward_train) and the fused step's gradients, every parameter tensor, at the fixture's
    512 rows and at a ragged batch of 4,096 + 77 rows.

    The ragged batch is the first 4,173 rows of a seeded `get_batch` pool that `pia_net_common.kink_rows` does not flag: rows
    with a LeakyReLU input within float32 resolution of zero (judged by the float64 restatement alone, threshold from the
    format's precision) have a derivative that any float32 evaluation picks by rounding luck, so float64 is no yardstick for
    them.  An earlier form of this case kept such a row (|z| = 1.5e-9 of its scale): the kernels then deviated 5.0e-5 on
    T2_predictor.0.0.weight, and so did plain float32 torch on the same host, while the same torch code on another CPU did
    not.  The fixture's 512 rows are used as they are; how many of them the rule would flag is printed."""
    g = golden("pia_net.npz")
    m = _model()
    host = _host_params(m)
    if rows == 512:
        x, pids = torch.from_numpy(g["batch/x"]), torch.from_numpy(C.pids_map())
    else:
        np.random.seed(5)
        pool = pia_net.get_batch(rows + 1024, 0.02)[0]
        keep = ~C.kink_rows(host, pool)
        print(f"ragged pool: {int((~keep).sum())} of {pool.shape[0]} rows lie on a LeakyReLU kink at float32 resolution")
        assert int(keep.sum()) >= rows
        x, pids = pool[keep][:rows].contiguous(), torch.from_numpy(C.pids_map(rows, seed=11))
        assert x.shape[0] == rows and rows % 64 != 0
    print(f"rows on a kink in this batch: {int(C.kink_rows(host, x).sum())}")
    want_loss, want_g, _ = C.loss_and_grads64(host, x, pids)
    _, host32_g, _ = C.loss_and_grads64(host, x, pids, dtype=torch.float32)       # printed beside each figure, never a bound
    ops.launch_counts_reset()
    out = m(x.cuda())
    loss = m.loss_function(out[0], x.cuda(), pids.cuda())
    loss.backward()
    c = ops.pia_launch_counts()
    assert c["pia_fwd"] == 6 and c["pia_head"] == 2 and c["pia_dx"] == 5 and c["pia_dw"] == 6, c
    auto_g = [p.grad.detach().cpu().numpy() for p in m.parameters()]
    fitter = pia_net.PiaFitter(m, lr=0.0)                 # lr 0: the step leaves the parameters alone, its gradients stay
    ops.launch_counts_reset()
    fused_loss = fitter.step(x.cuda(), pids.cuda())
    c = ops.pia_launch_counts()
    assert c["pia_fwd"] == 6 and c["pia_head"] == 1 and c["pia_dx"] == 5 and c["pia_dw"] == 6, c
    assert sum(ops.launch_counts().values()) == 0, ops.launch_counts()
    fused_g = [t.cpu().numpy() for t in fitter.state.split(fitter.grads)]
    print(f"loss: f64 {want_loss.item():.9e}, autograd {loss.item():.9e}, fused {fused_loss.item():.9e}")
    assert abs(loss.item() - want_loss.item()) <= 1e-5 * want_loss.item()
    assert abs(fused_loss.item() - want_loss.item()) <= 1e-5 * want_loss.item()
    fails = []
    for n, ga, gf, gw, g32 in zip(C.PARAM_NAMES, auto_g, fused_g, want_g, host32_g):
        bound = FACTOR * float(g[f"ref_err/grad/{n}"])
        print(f"grad[{rows}] float32 layers on the host {n}: deviation {C.rel_dev(g32.numpy(), gw.numpy()):.3e}")
        for tag, got in (("autograd", ga), ("fused", gf)):
            ok, info = _check(f"grad[{rows}] {tag} {n}", got, gw.numpy(), bound)
            if not ok:
                fails.append(info)
    assert not fails, fails


def test_gradients_on_the_unfiltered_ragged_batch_follow_float32(golden):
    """The same 4,096 + 77 rows WITHOUT the kink filter, so that an error of the kernels next to a kink cannot hide behind it.
    This batch holds a T2-head unit whose float64 pre-activation is 1.5e-9 of its scale; float64 is no yardstick for its
    derivative, but plain float32 is: the same layers run in float32 torch on the host (`loss_and_grads64(dtype=float32)`)
    meet the same kink with the same number format.  Per tensor, the kernels' deviation from float64 may be at most the
    usual bound or twice the host float32 run's own deviation from float64, whichever is larger.  (Measured on the MI355X
    host: both deviate 5.0e-5 on T2_predictor.0.0.weight.  A host whose float32 sums land on float64's side of that unit
    would leave only the usual bound, which the kernels then need not meet: the case depends on the host's float32 BLAS.)"""
    g = golden("pia_net.npz")
    m = _model()
    host = _host_params(m)
    rows = 4096 + 77
    np.random.seed(5)
    x, pids = pia_net.get_batch(rows, 0.02)[0], torch.from_numpy(C.pids_map(rows, seed=11))
    print(f"rows on a kink in this batch: {int(C.kink_rows(host, x).sum())}")
    _, want_g, _ = C.loss_and_grads64(host, x, pids)
    _, host32_g, _ = C.loss_and_grads64(host, x, pids, dtype=torch.float32)
    m.loss_function(m(x.cuda())[0], x.cuda(), pids.cuda()).backward()
    auto_g = [p.grad.detach().cpu().numpy() for p in m.parameters()]
    fitter = pia_net.PiaFitter(m, lr=0.0)
    fitter.step(x.cuda(), pids.cuda())
    fused_g = [t.cpu().numpy() for t in fitter.state.split(fitter.grads)]
    fails = []
    for n, ga, gf, gw, g32 in zip(C.PARAM_NAMES, auto_g, fused_g, want_g, host32_g):
        host_dev = C.rel_dev(g32.numpy(), gw.numpy())
        bound = max(FACTOR * float(g[f"ref_err/grad/{n}"]), 2.0 * host_dev)
        print(f"unfiltered {n}: float32 on the host deviates {host_dev:.3e}")
        for tag, got in (("autograd", ga), ("fused", gf)):
            ok, info = _check(f"unfiltered {tag} {n}", got, gw.numpy(), bound)
            if not ok:
                fails.append(info)
    assert not fails, fails


def test_non_default_shape_against_float64(golden):
    """Four encoder layers and 256-wide heads (the narrow head kernel, another layer count), on the first rows of the
    fixture's batch: forward and every gradient, autograd and fused, against float64 with the fixture's `small/ref_err/*`
    (the reference's own float32-vs-float64 deviation for THIS shape and batch).  The shape is deep enough that the T2 head's
    tanh does not saturate: with two encoder layers the reference's own float32 T2 gradients are 25 % off float64."""
    g = golden("pia_net.npz")
    torch.manual_seed(0)
    m = pia_net.PIA(hidden_dims=list(C.SMALL_HIDDEN))
    names = [str(n) for n in g["small/param_names"]]
    assert [n for n, _ in m.named_parameters()] == names
    for n, p in m.named_parameters():
        assert C.sha(p.detach().cpu().numpy()) == str(g[f"small/init_sha/{n}"]), n
    m = m.cuda()
    host = _host_params(m)
    x = torch.from_numpy(g["batch/x"])[:C.SMALL_ROWS].contiguous()
    pids = torch.from_numpy(C.pids_map())[:C.SMALL_ROWS].contiguous()
    want_loss, want_g, want_out = C.loss_and_grads64(host, x, pids)
    assert abs(want_loss.item() - float(g["small/f64/loss"])) <= 1e-12 * want_loss.item()     # the restatement serves this shape
    for k, t in zip(("signal", "D", "T2", "v"), want_out):
        assert C.rel_dev(C.sample(t.numpy()), g[f"small/f64/{k}"]) <= 1e-12, k
    ops.launch_counts_reset()
    out = m(x.cuda())
    loss = m.loss_function(out[0], x.cuda(), pids.cuda())
    loss.backward()
    c = ops.pia_launch_counts()
    assert c["pia_fwd"] == 5 and c["pia_head"] == 2 and c["pia_dx"] == 4 and c["pia_dw"] == 5, c
    fails = []
    for k, got, want in zip(("signal", "D", "T2", "v"), (out[0], out[2], out[3], out[4]), want_out):
        ok, info = _check(f"small forward {k}", got.detach().cpu().numpy(), want.numpy(), FACTOR * float(g[f"small/ref_err/{k}"]))
        if not ok:
            fails.append(info)
    auto_g = [p.grad.detach().cpu().numpy() for p in m.parameters()]
    fitter = pia_net.PiaFitter(m, lr=0.0)
    fused_loss = fitter.step(x.cuda(), pids.cuda())
    fused_g = [t.cpu().numpy() for t in fitter.state.split(fitter.grads)]
    assert abs(fused_loss.item() - want_loss.item()) <= 1e-5 * want_loss.item()
    for n, ga, gf, gw in zip(names, auto_g, fused_g, want_g):
        assert C.rel_dev(C.sample(gw.numpy()), g[f"small/f64/grad/{n}"]) <= 1e-12, n
        for tag, got in (("autograd", ga), ("fused", gf)):
            ok, info = _check(f"small grad {tag} {n}", got, gw.numpy(), FACTOR * float(g[f"small/ref_err/grad/{n}"]))
            if not ok:
                fails.append(info)
    assert not fails, fails


def test_autograd_guards():
    """What the kernels cannot honour is refused: a gradient for x, weights changed between forward and backward, float T2 tables."""
    m = _model()
    x = torch.rand(8, 16, device="cuda") * 1000
    with pytest.raises(ValueError):
        m(x.clone().requires_grad_(True))
    out = m(x)
    with torch.no_grad():
        next(m.parameters()).mul_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        out[0].sum().backward()
    with pytest.raises(ValueError, match="integer table"):
        pia_net.PIA(T2_mean=[45.0, 70.0, 750.0]).cuda()(x)



def _batches():
    for it in range(20):
        np.random.seed(100 + it)
        yield pia_net.get_batch(512, 0.02)[0].cuda()


def test_fused_trajectory_against_reference(golden):
    g = golden("pia_net.npz")
    m = _model()
    pids = torch.from_numpy(C.pids_map()).cuda()
    fitter = pia_net.PiaFitter(m, lr=1e-3)
    losses = torch.cat([fitter.step(x, pids) for x in _batches()]).cpu().numpy().astype(np.float64)
    dev32 = np.max(np.abs(losses - g["traj/losses"]) / np.abs(g["traj/losses"]))
    dev64 = np.max(np.abs(losses - g["traj/losses_f64"]) / np.abs(g["traj/losses_f64"]))
    print(f"fused trajectory: vs reference f32 {dev32:.3e}, vs reference f64 {dev64:.3e}; reference f32 vs f64 "
          f"{float(g['traj/ref_err']):.3e}")
    print("losses", losses)
    assert dev32 <= TRAJ_RTOL, (dev32, dev64)
    worst = 0.0
    for n, p in m.named_parameters():
        worst = max(worst, C.rel_dev(C.sample(p.detach().cpu().numpy()), g[f"traj/final/{n}"]))
    print(f"final parameters: worst deviation {worst:.3e}, reference f32 vs f64 {float(g['traj/final_ref_err']):.3e}")
    assert worst <= FACTOR * float(g["traj/final_ref_err"])


def test_autograd_loop_matches_the_fused_step(golden):
    g = golden("pia_net.npz")
    pids = torch.from_numpy(C.pids_map()).cuda()
    m1 = _model()
    fitter = pia_net.PiaFitter(m1, lr=1e-3)
    fused = torch.cat([fitter.step(x, pids) for x in _batches()]).cpu().numpy().astype(np.float64)
    m2 = _model()
    opt = torch.optim.Adam(m2.parameters(), lr=1e-3)
    loop = []
    for x in _batches():
        loss = m2.loss_function(m2(x)[0], x, pids)
        opt.zero_grad()
        loss.backward()
        opt.step()
        loop.append(loss.item())
    loop = np.array(loop)
    dev = np.max(np.abs(loop - fused) / np.abs(fused))
    dev_ref = np.max(np.abs(loop - g["traj/losses"]) / np.abs(g["traj/losses"]))
    print(f"autograd loop vs fused {dev:.3e}; vs reference {dev_ref:.3e}")
    assert dev <= TRAJ_RTOL and dev_ref <= TRAJ_RTOL


def test_forward_is_chunk_invariant_and_fits_are_reproducible(golden):
    g = golden("pia_net.npz")
    m = _model()
    m._state.ensure()
    np.random.seed(9)
    x = pia_net.get_batch(1000, 0.02)[0].cuda()
    ref = pia_net.pia_forward(m._state, x, chunk_rows=1000)
    for chunk in (512, 100, 37):
        got = pia_net.pia_forward(m._state, x, chunk_rows=chunk)
        assert all(torch.equal(a, b) for a, b in zip(ref, got)), chunk
    fitter = pia_net.PiaFitter(m)
    D, T2, v = fitter.encode_volume(x.reshape(10, 100, 16).cpu().numpy(), chunk_rows=64)
    assert tuple(D.shape) == (10, 100, 3) and torch.equal(D.reshape(-1, 3), ref[1]) and torch.equal(v.reshape(-1, 3), ref[3])
    finals = []
    for _ in range(2):
        mm = _model()
        f = pia_net.PiaFitter(mm, lr=1e-3)
        ls = torch.cat([f.step(xb) for xb in list(_batches())[:6]])
        finals.append((ls.cpu(), f.state.flat.cpu().clone(), f.grads.cpu().clone()))
    assert all(torch.equal(a, b) for a, b in zip(*finals))


def test_supervised_loss_value(golden):
    g = golden("pia_net.npz")
    m = _model()
    np.random.seed(1)
    _, D, T2, v, _ = pia_net.get_batch(512, 0.02)
    x = torch.from_numpy(g["batch/x"]).cuda()
    with torch.no_grad():
        signal, _, pD, pT2, pv = m(x)
        val = m.loss_function([signal, pD, pT2, pv], [x, D.cuda(), T2.cuda(), v.cuda()], None, tissue_available=True)
    want = float(g["supervised_loss"])
    print(f"supervised loss {val.item():.12e}, reference {want:.12e}, relative {abs(val.item() - want) / want:.3e}")
    assert str(val.dtype) == str(g["supervised_dtype"])
    assert abs(val.item() - want) <= 1e-6 * want
    # with float64 targets for D the branch can be trained through the train pair (the reference's backward raises here)
    out = m(x)
    loss = m.loss_function([out[0], out[2], out[3], out[4]], [x, D.cuda().double(), T2.cuda(), v.cuda()], None, tissue_available=True)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


def test_pids_slice_and_adc_slice(golden):
    g = golden("pia_net.npz")
    S = g["pids_slice/S"]
    assert np.array_equal(S, C.pids_slice_input())
    bv = np.array(C.B_VALUES, dtype=np.float64)
    maps = pia_net.detect_PIDS_slice(bv, S)
    for name, got in zip(("adc1", "adc2", "b_decay", "te_decay"), maps):
        want = g[f"pids_slice/{name}"]
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(got, want), (name, int((got != want).sum()))
    assert 0 < maps[0].sum() and 0 < maps[1].sum() and 0 < maps[2].sum() < maps[2].size
    adc = pia_net.ADC_slice(bv, S[:, :, :, 0])
    print("ADC_slice max abs deviation", np.abs(adc - g["pids_slice/adc_slice"]).max())
    assert adc.shape == (12, 12) and np.abs(adc - g["pids_slice/adc_slice"]).max() <= 1e-6


def _phantom():
    from mri_super_resolution_amd import pia
    sig = pia.phantom_signals(16 * 16 * 4, noise=0.01, seed=2).reshape(16, 16, 4, 4, 4)
    amp = 0.5 + 0.05 * np.arange(4).reshape(1, 1, 4, 1, 1)
    return np.maximum(sig * amp, 1.0).astype(np.float32)


DRIVER_KW = dict(slice_index=1, steps=30, seed=0, hidden_features=64, hidden_layers=1, mapping_size=16)


def test_fit_hybrid_with_the_pia_estimator():
    from mri_super_resolution_amd import drivers
    res = drivers.fit_hybrid(_phantom(), estimator="pia", pia_steps=300, pia_batch=512, **DRIVER_KW)
    vol = tuple(res["recon_hybrid"].shape[:3])
    assert vol == (32, 32, 4)
    D, T2, v = res["D"], res["T2"], res["v"]
    assert D.shape == T2.shape == v.shape == vol + (3,) and D.dtype == np.float64 and T2.dtype == v.dtype == np.float32
    assert np.isfinite(D).all() and np.isfinite(T2).all() and np.isfinite(v).all()
    for c in range(3):
        assert np.all(np.abs(D[..., c] - C.D_MEAN[c]) <= C.D_DELTA[c] * (1 + 1e-12))
        assert np.all(np.abs(T2[..., c] - C.T2_MEAN[c]) <= C.T2_DELTA[c] * (1 + 1e-6))
    assert np.all(v >= 0) and np.abs(v.sum(-1) - 1).max() <= 1e-6
    print(f"pia loss on the held-out batch: {res['pia_loss_before']:.4e} -> {res['pia_loss_after']:.4e}")
    assert res["pia_loss_after"] < res["pia_loss_before"] and len(res["pia_step_losses"]) == 300
    assert res["pids"]["PIDS_ADC1"].shape == (32, 32) and res["pids"]["PIDS_TE_decay"].shape == (32, 32, 4, 3)
    assert "status" not in res and res["estimator"] == "pia"


def test_fit_hybrid_default_estimator_is_unchanged():
    from mri_super_resolution_amd import drivers
    a = drivers.fit_hybrid(_phantom(), **DRIVER_KW)
    b = drivers.fit_hybrid(_phantom(), estimator="curve_fit", **DRIVER_KW)
    assert sorted(a.keys()) == sorted(b.keys()) and "estimator" not in a
    assert torch.equal(a["recon_hybrid"], b["recon_hybrid"])
    for k in ("D", "T2", "v", "status"):
        assert np.array_equal(a[k], b[k]), k
    assert a["D"].shape == (32, 32, 3)
