"""Every workspace view stays inside the bytes its planner reports.

Each case puts a workspace of exactly the planner's bytes between the two 0xA5 guards of tests/guard_common.py, passes
``workspace_bytes = planner bytes`` to ONE call per entry point and asserts that the call succeeds, that both guards are untouched and
that the outputs are finite.  The shapes are
the smallest at which a carve can still go wrong: a ragged last block, both block sizes of the small-network kernels, every
mode of a view.  Only allocated memory is read and written.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import guard_common
from mri_super_resolution_amd import _lib, rams

pytestmark = pytest.mark.gpu
ADAM = (1e-4, 0.9, 0.999, 1e-8)
DEV = "cuda:0"


class Guarded(guard_common.Guarded):
    """A zeroed workspace of `need` bytes between a guard head and a guard tail."""

    def __init__(self, need):
        assert need > 0, _lib.lib().inr_last_error()
        self.need = int(need)
        super().__init__(self.need, torch.uint8, 0x00, DEV)
        self.args = (self.ptr, self.need)


def run(ws, rc, *outputs):
    assert rc == 0, (rc, _lib.lib().inr_last_error())
    assert ws.intact(), "the call wrote outside the bytes its planner reports"
    for o in outputs:
        assert bool(torch.isfinite(o).all())


def stream():
    return torch.cuda.current_stream().cuda_stream


def rand(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g) - 0.5) * 2 * scale).to(DEV)


def siren(in_f, hidden, layers):
    desc = _lib.SirenDesc(in_f, hidden, layers, 1, 30.0, 30.0)
    total = _lib.lib().inr_siren_param_count(C.byref(desc))
    return desc, rand(total, scale=0.05)


def fit_once(desc, params, n, n_steps=2):
    lib = _lib.lib()
    ws = Guarded(lib.inr_siren_fit_workspace_bytes(C.byref(desc), n))
    p = params.clone()
    g, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    x, t = rand(n, desc.in_features, seed=1), rand(n, 1, seed=2)
    losses = torch.zeros(n_steps, device=DEV)
    rc = lib.inr_siren_fit(C.byref(desc), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), x.data_ptr(), t.data_ptr(), None, n, 1,
                           n_steps, *ADAM, losses.data_ptr(), *ws.args, stream())
    run(ws, rc, p, m, v, losses)


def forward_once(desc, params, n):
    lib = _lib.lib()
    ws = Guarded(lib.inr_siren_forward_workspace_bytes(C.byref(desc), n))
    x, y = rand(n, desc.in_features, seed=1), torch.empty(n, 1, device=DEV)
    rc = lib.inr_siren_forward(C.byref(desc), params.data_ptr(), x.data_ptr(), n, y.data_ptr(), 0, 0.0, *ws.args, stream())
    run(ws, rc, y)


@pytest.mark.parametrize("persistent", [1, 0])
@pytest.mark.parametrize("shape", [(2, 64, 2, 130), (2, 32, 1, 33)])
def test_siren_small_path(shape, persistent):
    """key 12: 1 = the persistent kernel's view, 0 = the two-launch step's"""
    lib = _lib.lib()
    desc, params = siren(*shape[:3])
    try:
        assert lib.inr_debug_set(12, persistent) == 0
        fit_once(desc, params, shape[3])
    finally:
        lib.inr_debug_reset()


@pytest.mark.parametrize("key,val", [(None, None), (7, 0), (0, 1)], ids=["hl32", "split", "generic"])
def test_siren_layerwise_paths(key, val):
    lib = _lib.lib()
    desc, params = siren(64, 128, 1)
    try:
        if key is not None:
            assert lib.inr_debug_set(key, val) == 0
        fit_once(desc, params, 300)
        forward_once(desc, params, 300)
    finally:
        lib.inr_debug_reset()


def test_siren_reconstruct():
    lib = _lib.lib()
    desc, params = siren(2, 64, 2)
    ws = Guarded(lib.inr_siren_reconstruct_workspace_bytes(C.byref(desc), 32))
    y = torch.empty(63, 1, device=DEV)
    rc = lib.inr_siren_reconstruct(C.byref(desc), params.data_ptr(), _lib.shape_array((9, 7)), 2, None, 0, y.data_ptr(), 0, 0.0, 32,
                                   *ws.args, stream())
    run(ws, rc, y)


def wire_net(n=100, in_f=3):
    desc = _lib.WireDesc(in_f, 32, 1, 1, 10.0, 10.0, 10.0, 10.0)
    total = _lib.lib().inr_wire_param_count(C.byref(desc))
    return desc, rand(total, scale=0.05), rand(n, in_f, seed=1)


def test_wire_fit():
    lib = _lib.lib()
    n = 100
    desc, p, x = wire_net(n)
    ws = Guarded(lib.inr_wire_workspace_bytes(C.byref(desc), n, 1))
    g, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    t, losses = rand(n, seed=2), torch.zeros(2, device=DEV)
    rc = lib.inr_wire_fit(C.byref(desc), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), x.data_ptr(), t.data_ptr(), None, n, 1, 2,
                          *ADAM, losses.data_ptr(), *ws.args, stream())
    run(ws, rc, p, g, losses)


def test_wire_forward_stash_and_input_grad():
    lib = _lib.lib()
    n = 100
    desc, p, x = wire_net(n)
    ws = Guarded(lib.inr_wire_workspace_bytes(C.byref(desc), n, 2))
    y, gy, dx = torch.empty(n, device=DEV), rand(n, seed=3), torch.empty(n, 3, device=DEV)
    run(ws, lib.inr_wire_forward_stash(C.byref(desc), p.data_ptr(), x.data_ptr(), n, y.data_ptr(), *ws.args, stream()), y)
    run(ws, lib.inr_wire_input_grad(C.byref(desc), p.data_ptr(), gy.data_ptr(), n, dx.data_ptr(), *ws.args, stream()), dx)


def test_wire_forward_and_layer_forward():
    lib = _lib.lib()
    n = 100
    desc, p, x = wire_net(n)
    ws = Guarded(lib.inr_wire_workspace_bytes(C.byref(desc), n, 0))
    y = torch.empty(n, device=DEV)
    run(ws, lib.inr_wire_forward(C.byref(desc), p.data_ptr(), x.data_ptr(), n, y.data_ptr(), *ws.args, stream()), y)
    ws = Guarded(lib.inr_wire_layer_workspace_bytes(n, 3, 32))
    lw, lb, ow, ob = rand(32, 3, scale=0.3, seed=4), rand(32, scale=0.3, seed=5), rand(32, 3, scale=0.3, seed=6), rand(32, scale=0.3, seed=7)
    out = torch.empty(n, 64, device=DEV)
    rc = lib.inr_wire_layer_forward(out.data_ptr(), x.data_ptr(), lw.data_ptr(), lb.data_ptr(), ow.data_ptr(), ob.data_ptr(), n, 3, 32, 1,
                                    10.0, 10.0, *ws.args, stream())
    run(ws, rc, out)


def pia_net():
    d = _lib.PiaDesc()
    d.n_signals, d.n_hidden, d.predictor_depth, d.n_b, d.n_te, d.leaky_slope = 16, 1, 1, 4, 4, 0.01
    d.hidden[0] = 256
    for i in range(4):
        d.b_values[i] = 500.0 * i
        d.te_values[i] = 60.0 + 20.0 * i
    for c in range(3):
        d.D_mean[c], d.D_delta[c], d.T2_mean[c], d.T2_delta[c] = 1.5, 1.0, 100.0, 50.0
    total = _lib.lib().inr_pia_param_count(C.byref(d))
    assert total > 0, _lib.lib().inr_last_error()
    return d, rand(total, scale=0.05), rand(70, 16, seed=1).abs() + 0.1


def test_pia_training_step():
    lib = _lib.lib()
    n = 70
    d, p, x = pia_net()
    ws = Guarded(lib.inr_pia_workspace_bytes(C.byref(d), n, 1))
    g, m, v, loss = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p), torch.zeros(1, device=DEV)
    rc = lib.inr_pia_fit_step(C.byref(d), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), x.data_ptr(), None, n, 1, *ADAM,
                              loss.data_ptr(), *ws.args, stream())
    run(ws, rc, p, g, loss)


def test_pia_forward():
    lib = _lib.lib()
    n = 70
    d, p, x = pia_net()
    ws = Guarded(lib.inr_pia_workspace_bytes(C.byref(d), n, 0))
    sig, D = torch.empty(n, 16, device=DEV), torch.empty(n, 3, dtype=torch.float64, device=DEV)
    T2, v = torch.empty(n, 3, device=DEV), torch.empty(n, 3, device=DEV)
    rc = lib.inr_pia_forward(C.byref(d), p.data_ptr(), x.data_ptr(), n, sig.data_ptr(), D.data_ptr(), T2.data_ptr(), v.data_ptr(), n,
                             *ws.args, stream())
    run(ws, rc, sig, D, T2, v)


def test_erd_loss_grad():
    lib = _lib.lib()
    n = 70
    desc = _lib.SirenDesc(2, 64, 1, 1, 30.0, 30.0)
    total = lib.inr_erd_param_count(C.byref(desc))
    p, g = rand(total, scale=0.05), torch.zeros(total, device=DEV)
    x, t, loss = rand(n, 2, seed=1), rand(n, seed=2), torch.zeros(1, device=DEV)
    ws = Guarded(lib.inr_erd_workspace_bytes(C.byref(desc), n))
    rc = lib.inr_erd_loss_grad(C.byref(desc), p.data_ptr(), g.data_ptr(), x.data_ptr(), t.data_ptr(), None, n, 0, 0.1, 1, 0, loss.data_ptr(),
                               *ws.args, stream())
    run(ws, rc, g, loss)


def test_jet_with_the_laplacian():
    lib = _lib.lib()
    n = 50
    desc, p = siren(2, 32, 1)
    x = rand(n, 2, seed=1)
    y, grad, lap = torch.empty(n, device=DEV), torch.empty(n, 2, device=DEV), torch.empty(n, device=DEV)
    ws = Guarded(lib.inr_siren_jet_workspace_bytes(C.byref(desc), 2, 0, 32, 1))
    rc = lib.inr_siren_jet(C.byref(desc), p.data_ptr(), x.data_ptr(), n, 2, 2, None, 0, y.data_ptr(), grad.data_ptr(), lap.data_ptr(), 32,
                           *ws.args, stream())
    run(ws, rc, y, grad, lap)


@pytest.mark.parametrize("with_grad", [False, True])
def test_cssim(with_grad):
    lib = _lib.lib()
    B, size, border = 2, 24, 3
    yt, yp = (rand(B, size, size, seed=1).abs() * 60000 + 500), (rand(B, size, size, seed=2).abs() * 60000 + 500)
    mk, out = torch.ones(B, size, size, device=DEV), torch.empty(B, dtype=torch.float64, device=DEV)
    if with_grad:
        ws = Guarded(lib.inr_rams_shift_ssim_grad_workspace_bytes(B, size, border))
        grad = torch.empty_like(yp)
        rc = lib.inr_rams_shift_ssim_grad(out.data_ptr(), grad.data_ptr(), yt.data_ptr(), yp.data_ptr(), mk.data_ptr(), None, B, size,
                                          border, 0, *ws.args, stream())
        run(ws, rc, out, grad)
    else:
        ws = Guarded(lib.inr_rams_shift_ssim_workspace_bytes(B, size, border))
        rc = lib.inr_rams_shift_ssim(out.data_ptr(), yt.data_ptr(), yp.data_ptr(), mk.data_ptr(), B, size, border, 0, *ws.args, stream())
        run(ws, rc, out)


@pytest.mark.parametrize("B", [1, 3])
def test_rams_forward(B):
    lib = _lib.lib()
    model = rams.RAMS(3, 32, 3, 9, 8, 1, seed=3)
    H, W = 13, 16
    x = torch.from_numpy((np.random.default_rng(B).random((B, H, W, 9)) * 30000 + 500).astype(np.float32)).to(DEV)
    out = torch.empty(B, 3 * H, 3 * W, 1, device=DEV)
    ws = Guarded(lib.inr_rams_workspace_bytes(C.byref(model.desc), B, H, W))
    rc = lib.inr_rams_forward(C.byref(model.desc), model.pack().data_ptr(), x.data_ptr(), out.data_ptr(), B, H, W, 0, *ws.args, stream())
    run(ws, rc, out)


def test_rams_training_step():
    lib = _lib.lib()
    tr = rams.RamsTrainer(rams.RAMS(3, 32, 3, 9, 8, 1, seed=3))
    rng = np.random.default_rng(5)
    side = 16
    x = torch.from_numpy((rng.random((1, side, side, 9)) * 20000 + 2000).astype(np.float32)).to(DEV)
    hr = torch.from_numpy((rng.random((1, 3 * side, 3 * side)) * 20000 + 2000).astype(np.float32)).to(DEV)
    mask, loss = torch.ones(1, 3 * side, 3 * side, device=DEV), torch.empty(1, dtype=torch.float64, device=DEV)
    ws = Guarded(lib.inr_rams_train_workspace_bytes(C.byref(tr.model.desc), 1, side, side))
    rc = lib.inr_rams_train_grads(C.byref(tr.model.desc), tr.flat.data_ptr(), tr.grads.data_ptr(), x.data_ptr(), hr.data_ptr(),
                                  mask.data_ptr(), loss.data_ptr(), None, 1, side, side, *ws.args, stream())
    run(ws, rc, loss, tr.grads)
