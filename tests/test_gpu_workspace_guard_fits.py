"""The fitting entry points that take a workspace and that neither tests/test_gpu_workspace_guard.py nor
tests/test_gpu_workspace_guard_units.py calls: include/inrhip.h is the authority for that list.

The protocol is the one of tests/guard_common.py.  These entry points read AND write their parameter, gradient and Adam-moment
buffers, so those travel as in/out buffers: guarded, started from the same values for every call, compared bit for bit between the
call over a zeroed and the call over a 0xFF workspace and with what the public wrapper (``ops.*`` or the fitter class) leaves
behind.  Pure outputs (losses, predictions, a gradient the header says is written in full) are pre-filled with 0xFF as elsewhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.guard_common import DEV, POISON, Guarded, guard_case, same_bits
from mri_super_resolution_amd import _lib, erd_inr, ops, pia_net, rams, wire

pytestmark = pytest.mark.gpu
F32 = torch.float32
LR, B1, B2, EPS = 1e-4, 0.9, 0.999, 1e-8


def stream():
    return torch.cuda.current_stream().cuda_stream


def sym(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g) - 0.5) * 2 * scale).to(DEV)


def case(entry, need, outputs, inout, call, reference):
    return guard_case(entry, int(need), outputs, call, reference, last_error=_lib.lib().inr_last_error, inout=inout)


def siren(in_f, hidden, layers):
    desc = _lib.SirenDesc(in_f, hidden, layers, 1, 30.0, 30.0)
    return desc, sym(_lib.lib().inr_siren_param_count(C.byref(desc)), seed=9, scale=0.05)


def adam_start(params):
    zero = torch.zeros_like(params)
    return {"params": params, "grads": zero, "m": zero, "v": zero}


NETS = pytest.mark.parametrize("net,n", [((64, 128, 1), 300), ((2, 64, 2), 130)], ids=["layerwise_64x128", "persistent_2x64x2"])


@NETS
def test_siren_fit_cycle(net, n):
    lib = _lib.lib()
    desc, params = siren(*net)
    n_acq, first_acq, steps = 2, 1, 3
    x, targets, weights = sym(n, net[0], seed=1), sym(n_acq, n, seed=2), sym(n_acq, n, seed=3).abs()
    need = lib.inr_siren_fit_workspace_bytes(C.byref(desc), n)
    ref = {k: v.clone() for k, v in adam_start(params).items()}
    ref["losses"] = torch.empty(steps, device=DEV)
    ops.siren_fit_cycle(desc, ref["params"], ref["grads"], ref["m"], ref["v"], x, targets, weights, first_acq, 1, steps, LR, B1, B2, EPS,
                        ref["losses"])
    case("inr_siren_fit_cycle", need, {"losses": ((steps,), F32)}, adam_start(params),
         lambda ws, o: lib.inr_siren_fit_cycle(C.byref(desc), o["params"].ptr, o["grads"].ptr, o["m"].ptr, o["v"].ptr, x.data_ptr(),
                                               targets.data_ptr(), weights.data_ptr(), n_acq, first_acq, n, 1, steps, LR, B1, B2, EPS,
                                               o["losses"].ptr, ws.ptr, need, stream()), ref)


def test_siren_fit_cycle_batch():
    """Two fits that share persistent launches, each with a guarded workspace of its own: written by hand, because the protocol's
    helper carries one workspace."""
    lib = _lib.lib()
    desc, base = siren(2, 64, 2)
    K, n, steps = 2, 130, 3
    starts = [base, sym(base.numel(), seed=10, scale=0.05)]
    x = sym(n, 2, seed=1)
    targets = [sym(2, n, seed=2), sym(1, n, seed=3)]
    n_acq, first_acq = [2, 1], [1, 0]
    need = lib.inr_siren_fit_workspace_bytes(C.byref(desc), n)
    assert need > 0, lib.inr_last_error()
    ref = [{k: v.clone() for k, v in adam_start(p).items()} for p in starts]
    ref_losses = [torch.empty(steps, device=DEV) for _ in range(K)]
    ops.siren_fit_cycle_batch(desc, [r["params"] for r in ref], [r["grads"] for r in ref], [r["m"] for r in ref], [r["v"] for r in ref], x,
                              targets, None, first_acq, 1, steps, LR, B1, B2, EPS, ref_losses)
    runs = []
    for fill in (0x00, POISON):
        wss = [Guarded(need, torch.uint8, fill) for _ in range(K)]
        bufs = []
        for p in starts:
            b = {k: Guarded(v.shape, F32, 0x00) for k, v in adam_start(p).items()}
            for k, v in adam_start(p).items():
                b[k].view.copy_(v)
            b["losses"] = Guarded(steps, F32, POISON)
            bufs.append(b)

        def ptrs(items):
            return (C.c_void_p * K)(*items)
        rc = lib.inr_siren_fit_cycle_batch(C.byref(desc), K, *[ptrs([b[k].ptr for b in bufs]) for k in ("params", "grads", "m", "v")],
                                           x.data_ptr(), ptrs([t.data_ptr() for t in targets]), None, (C.c_int * K)(*n_acq),
                                           (C.c_int * K)(*first_acq), n, 1, steps, LR, B1, B2, EPS, ptrs([b["losses"].ptr for b in bufs]),
                                           ptrs([w.ptr for w in wss]), need, stream())
        assert rc == 0, (rc, lib.inr_last_error())
        assert all(w.intact() for w in wss), f"a fit wrote outside the {need} bytes its planner reports (pre-fill {fill:#04x})"
        assert all(g.intact() for b in bufs for g in b.values())
        runs.append(bufs)
    print(f"inr_siren_fit_cycle_batch: {K} workspaces of {need} bytes pre-filled with 0x00, 0xff; losses pre-filled with 0xff")
    for k in range(K):
        for name, g in runs[0][k].items():
            assert same_bits(g.view, runs[1][k][name].view), f"fit {k}: `{name}` depends on what the workspace held before the call"
            assert bool(torch.isfinite(g.view).all()), f"fit {k}: `{name}` is not finite"
            want = ref_losses[k] if name == "losses" else ref[k][name]
            assert same_bits(g.view, want), f"fit {k}: `{name}` differs from what ops.siren_fit_cycle_batch leaves"


@pytest.mark.parametrize("ex", [False, True], ids=["loss_grad", "loss_grad_ex"])
def test_siren_loss_grad(ex):
    lib = _lib.lib()
    desc, params = siren(64, 128, 1)
    n = 300
    x, t, w = sym(n, 64, seed=1), sym(n, 1, seed=2), sym(n, 1, seed=3).abs()
    need = lib.inr_siren_fit_workspace_bytes(C.byref(desc), n)
    ref = {"grads": torch.zeros_like(params), "loss": torch.empty(1, device=DEV)}
    ops.siren_loss_grad(desc, params, ref["grads"], x, t, w, 2 * n, ref["loss"])

    def call(ws, o):
        args = (C.byref(desc), params.data_ptr(), o["grads"].ptr, x.data_ptr(), t.data_ptr(), w.data_ptr(), n, 2 * n, o["loss"].ptr, ws.ptr, need)
        return lib.inr_siren_loss_grad_ex(*args, 0, stream()) if ex else lib.inr_siren_loss_grad(*args, stream())
    case("inr_siren_loss_grad" + ("_ex" if ex else ""), need, {"loss": ((1,), F32)}, {"grads": torch.zeros_like(params)}, call, ref)


def test_siren_forward_and_backward_train():
    """The pair shares one workspace: the forward leaves its stash there and the backward, which writes every element of the flat
    gradient, reads it."""
    lib = _lib.lib()
    desc, params = siren(64, 128, 1)
    assert ops.siren_hp_eligible(desc)
    n = 300
    x, gy = sym(n, 64, seed=1), sym(n, 1, seed=2)
    need = lib.inr_siren_fit_workspace_bytes(C.byref(desc), n)
    y, ws_ref = ops.siren_forward_train(desc, params, x)
    grads = ops.siren_backward_train(desc, params, torch.empty_like(params), gy, ws_ref)

    def call(ws, o):
        rc = lib.inr_siren_forward_train(C.byref(desc), params.data_ptr(), x.data_ptr(), o["y"].ptr, n, ws.ptr, need, 0, stream())
        return rc or lib.inr_siren_backward_train(C.byref(desc), params.data_ptr(), o["grads"].ptr, gy.data_ptr(), n, ws.ptr, need, stream())
    case("inr_siren_forward_train + inr_siren_backward_train", need, {"y": ((n, 1), F32), "grads": (tuple(params.shape), F32)}, None, call,
         {"y": y, "grads": grads})


def test_siren_fit_footprint():
    lib = _lib.lib()
    desc, params = siren(64, 128, 1)
    n, K, steps = 60, 5, 3
    x_sub, t, w = sym(n * K, 64, seed=1), sym(n, seed=2), sym(n, seed=3).abs()
    fw = torch.tensor([0.1, 0.2, 0.4, 0.2, 0.1], device=DEV)
    need = lib.inr_siren_fit_footprint_workspace_floats(C.byref(desc), n, K)
    ref = {k: v.clone() for k, v in adam_start(params).items()}
    ref["losses"] = torch.empty(steps, device=DEV)
    ops.siren_fit_footprint(desc, ref["params"], ref["grads"], ref["m"], ref["v"], x_sub, t, w, fw, 1, steps, LR, B1, B2, EPS, ref["losses"])
    case("inr_siren_fit_footprint", 4 * need, {"losses": ((steps,), F32)}, adam_start(params),
         lambda ws, o: lib.inr_siren_fit_footprint(C.byref(desc), o["params"].ptr, o["grads"].ptr, o["m"].ptr, o["v"].ptr, x_sub.data_ptr(),
                                                   t.data_ptr(), w.data_ptr(), fw.data_ptr(), n, K, 1, steps, LR, B1, B2, EPS, o["losses"].ptr,
                                                   ws.ptr, need, stream()), ref)


def test_siren_jet_grid():
    lib = _lib.lib()
    desc, params = siren(2, 32, 1)
    shape, chunk = (9, 7), 32
    n = shape[0] * shape[1]
    need = lib.inr_siren_jet_workspace_bytes(C.byref(desc), 2, 0, chunk, 1)

    def call(ws, o):
        return lib.inr_siren_jet_grid(C.byref(desc), params.data_ptr(), _lib.shape_array(shape), 2, 2, None, 0, o["y"].ptr,
                                      o["grad"].ptr if "grad" in o else None, o["lap"].ptr if "lap" in o else None, chunk, ws.ptr, need, stream())
    outs = {"y": ((n,), F32), "grad": ((n, 2), F32), "lap": ((n,), F32)}
    case("inr_siren_jet_grid", need, outs, None, call, dict(zip(outs, ops.siren_jet(desc, params, shape=shape, chunk_rows=chunk))))
    guard_case("inr_siren_jet_grid (nullable arguments null)", int(need), {"y": outs["y"]}, call, None, fills=(POISON,))


def test_wire_loss_grad():
    lib = _lib.lib()
    n = 100
    torch.manual_seed(5)
    fitter = wire.WireFitter(wire.Wire(3, 32, 1, 1).to(DEV))
    desc, params = fitter.desc, fitter.flat.clone()
    x, t, w = sym(n, 3, seed=1), sym(n, seed=2), sym(n, seed=3).abs()
    need = lib.inr_wire_workspace_bytes(C.byref(desc), n, 1)
    loss, grads = fitter.loss_grad(x, t, w)
    case("inr_wire_loss_grad", need, {"loss": ((1,), F32)}, {"grads": torch.zeros_like(params)},
         lambda ws, o: lib.inr_wire_loss_grad(C.byref(desc), params.data_ptr(), o["grads"].ptr, x.data_ptr(), t.data_ptr(), w.data_ptr(), n,
                                              o["loss"].ptr, ws.ptr, need, stream()), {"loss": loss, "grads": grads})


def test_rams_train_step():
    lib = _lib.lib()
    tr = rams.RamsTrainer(rams.RAMS(3, 32, 3, 9, 8, 1, seed=3))
    rng = np.random.default_rng(5)
    side = 16
    x = torch.from_numpy((rng.random((1, side, side, 9)) * 20000 + 2000).astype(np.float32)).to(DEV)
    hr = torch.from_numpy((rng.random((1, 3 * side, 3 * side)) * 20000 + 2000).astype(np.float32)).to(DEV)
    mask = torch.ones(1, 3 * side, 3 * side, device=DEV)
    desc = tr.model.desc
    need = lib.inr_rams_train_workspace_bytes(C.byref(desc), 1, side, side)
    start = {"params": tr.flat.clone(), "grads": tr.grads.clone(), "m": tr.m.clone(), "v": tr.v.clone()}
    step = tr.step_count + 1
    loss = tr.train_step(x, hr, mask)
    case("inr_rams_train_step", need, {"loss": ((1,), torch.float64)}, start,
         lambda ws, o: lib.inr_rams_train_step(C.byref(desc), o["params"].ptr, o["grads"].ptr, o["m"].ptr, o["v"].ptr, x.data_ptr(),
                                               hr.data_ptr(), mask.data_ptr(), o["loss"].ptr, 1, side, side, step, tr.lr, tr.b1, tr.b2, tr.eps,
                                               ws.ptr, need, stream()),
         {"params": tr.flat, "grads": tr.grads, "m": tr.m, "v": tr.v, "loss": loss})


def test_pia_forward_and_backward_train():
    """The pair shares one workspace; the backward writes every element of the flat gradient (parameter order, unpadded)."""
    lib = _lib.lib()
    n = 70
    torch.manual_seed(7)
    model = pia_net.PIA(hidden_dims=[256], predictor_depth=1)
    x, g = sym(n, 16, seed=1).abs() + 0.1, sym(n, 16, seed=2)
    signal, _, D, T2, v = model(x)
    (signal * g).sum().backward()
    ref_grads = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    desc, params = model._state.desc, model._state.flat
    need = lib.inr_pia_workspace_bytes(C.byref(desc), n, 1)

    def call(ws, o):
        rc = lib.inr_pia_forward_train(C.byref(desc), params.data_ptr(), x.data_ptr(), n, o["signal"].ptr, o["D"].ptr, o["T2"].ptr, o["v"].ptr,
                                       ws.ptr, need, stream())
        return rc or lib.inr_pia_backward_train(C.byref(desc), params.data_ptr(), o["grads"].ptr, x.data_ptr(), g.data_ptr(), None, None, None, n,
                                                ws.ptr, need, stream())
    outs = {"signal": ((n, 16), F32), "D": ((n, 3), torch.float64), "T2": ((n, 3), F32), "v": ((n, 3), F32), "grads": (tuple(params.shape), F32)}
    case("inr_pia_forward_train + inr_pia_backward_train", need, outs, None, call,
         {"signal": signal.detach(), "D": D.detach(), "T2": T2.detach(), "v": v.detach(), "grads": ref_grads})


def _erd_fitter():
    """A network whose outputs start positive: a head bias below zero would leave every output at the ReLU's 0, which the
    pre-training loop reports as COLLAPSED after its first step."""
    torch.manual_seed(3)
    model = erd_inr.ErdSiren(2, 64, 1).to(DEV)
    with torch.no_grad():
        model.final_linear.bias.fill_(0.1)
    return erd_inr.ErdFitter(model)


def test_erd_pretrain():
    lib = _lib.lib()
    n, steps, lr = 70, 3, 3e-4
    fitter = _erd_fitter()
    x, t = sym(n, 2, seed=1), sym(n, seed=2).abs()
    desc = fitter.desc
    need = lib.inr_erd_workspace_bytes(C.byref(desc), n)
    start = {"params": fitter.flat.clone(), "grads": fitter.grads.clone(), "m": fitter.m.clone(), "v": fitter.v.clone(),
             "status": fitter.new_status(DEV)}
    status = fitter.new_status(DEV)
    fitter.pretrain_steps(x, t, steps, lr, 0.0, status)
    case("inr_erd_pretrain", need, {}, start,
         lambda ws, o: lib.inr_erd_pretrain(C.byref(desc), o["params"].ptr, o["grads"].ptr, o["m"].ptr, o["v"].ptr, x.data_ptr(), t.data_ptr(), n,
                                            1, steps, lr, *fitter.betas, fitter.adam_eps, 0.0, o["status"].ptr, ws.ptr, need, stream()),
         {"params": fitter.flat, "grads": fitter.grads, "m": fitter.m, "v": fitter.v, "status": status})
    assert fitter.read_status(status)["steps_done"] == steps


def test_erd_finetune():
    lib = _lib.lib()
    n, K, steps, lr_perturb, lr_net, eps = 70, 3, 2, 3e-4, 1e-7, 1.0 / 128.0
    fitter = _erd_fitter()
    x, targets, weights = sym(n, 2, seed=1), sym(K, n, seed=2).abs(), sym(K, n, seed=3).abs()
    desc = fitter.desc
    need = lib.inr_erd_workspace_bytes(C.byref(desc), n)
    start = {"params": fitter.flat.clone(), "grads": fitter.grads.clone(), "m": fitter.m.clone(), "v": fitter.v.clone()}
    losses = fitter.finetune(x, targets, weights, steps, lr_perturb, lr_net, eps)

    def call(wts):
        return lambda ws, o: lib.inr_erd_finetune(C.byref(desc), o["params"].ptr, o["grads"].ptr, o["m"].ptr, o["v"].ptr, x.data_ptr(),
                                                  targets.data_ptr(), None if wts is None else wts.data_ptr(), K, n, eps, 1, steps, lr_perturb,
                                                  lr_net, *fitter.betas, fitter.adam_eps, o["losses"].ptr if "losses" in o else None, ws.ptr,
                                                  need, stream())
    case("inr_erd_finetune", need, {"losses": ((steps,), F32)}, start, call(weights),
         {"params": fitter.flat, "grads": fitter.grads, "m": fitter.m, "v": fitter.v, "losses": losses})
    guard_case("inr_erd_finetune (nullable arguments null)", int(need), {}, call(None), None, fills=(POISON,), inout=start)
