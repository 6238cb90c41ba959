"""CPU checks of the WIRE complex-Gabor family: the float64 real-arithmetic restatement (tests/wire_common.py) against the
fixture made from the reference's own layer (tools/make_wire_golden.py), the module's weights, keys and registration order
against the same fixture, the flat layout, and every refusal that has to come before any device work (fake device pointers
that are never dereferenced)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import wire_common as C
from mri_super_resolution_amd import _lib, drivers, matio
from mri_super_resolution_amd.flat import FlatParams
from mri_super_resolution_amd.scripts import superresDWI as dwi_script
from mri_super_resolution_amd.wire import ComplexGaborLayer2D, Wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("inr_wire_param_count", "inr_wire_param_offsets", "inr_wire_workspace_bytes", "inr_wire_layer_workspace_bytes",
         "inr_wire_layer_forward", "inr_wire_forward", "inr_wire_reconstruct_workspace_bytes", "inr_wire_reconstruct",
         "inr_wire_loss_grad", "inr_wire_fit")
TIGHT = 1e-12        # of each tensor's maximum


def _fake(k):
    return ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)


def _desc(in_f=32, hidden=32, layers=1, out=1):
    return _lib.WireDesc(in_f, hidden, layers, out, 1.2, 1.2, 1.2, 1.2)


def _close(got, want):
    return np.abs(np.asarray(got) - want).max() <= TIGHT * np.abs(want).max()


def test_fixture_holds_data_only_and_is_small():
    g = C.golden()
    assert os.path.getsize(C.GOLDEN) < 200_000
    assert g["x"].shape == (333, 32) and g["x"].dtype == np.float32 and g["coords"].shape == (333, 3) and g["B"].shape == (16, 3)
    assert g["traj_losses"].shape == (20,) and g["traj_y"].shape == (333,)
    for k in ("net.0.omega_0", "net.0.scale_0", "net.1.omega_0", "net.1.scale_0"):
        assert g["w/" + k].dtype == np.float32 and g["w/" + k][0] == np.float32(1.2)           # a float32 number, not 1.2


def test_restatement_agrees_with_the_reference_layer():
    g = C.golden()
    P = C.golden_leaves(g)
    y, loss, G = C.loss_grad64(P, g["x"], g["target"], 1)
    assert _close(y, g["y"]) and abs(loss - g["loss"]) <= TIGHT * g["loss"]
    for k in C.param_keys(1):
        assert G[k].shape == g["g/" + k].shape and _close(G[k], g["g/" + k]), k
    assert G["final_linear.bias"][0, 1] == 0.0 and g["g/final_linear.bias"][0, 1] == 0.0
    losses, y20 = C.adam_fit64(C.golden_leaves(g), g["x"], g["target"], 1, 20, 5e-5)
    assert _close(losses, g["traj_losses"]) and _close(y20, g["traj_y"])
    assert np.abs(y20 - g["y"]).max() > 1e-4                                                   # the trajectory moved


def test_wire_draws_the_fixture_weights_and_keeps_the_reference_keys():
    g = C.golden()
    torch.manual_seed(0)
    m = Wire(32, 32, 1, 1, first_omega_0=1.2, hidden_omega_0=1.2, scale=1.2)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert list(sd.keys())[:2] == ["final_linear.weight", "final_linear.bias"] and list(sd.keys())[-2:] == ["net.2.weight", "net.2.bias"]
    assert list(sd.keys())[2:8] == ["net.0." + n for n in ("omega_0", "scale_0", "linear.weight", "linear.bias", "scale_orth.weight",
                                                           "scale_orth.bias")]
    for k, v in sd.items():
        got = (torch.view_as_real(v) if v.is_complex() else v).numpy()
        assert got.dtype == np.float32 and np.array_equal(got, g["w/" + k]), k
    assert sd["net.0.linear.weight"].dtype == torch.float32 and sd["net.1.linear.weight"].dtype == torch.complex64
    assert sd["net.2.weight"].data_ptr() == sd["final_linear.weight"].data_ptr()
    names = [n for n, _ in m.named_parameters()]
    assert names[:2] == ["final_linear.weight", "final_linear.bias"] and len(names) == 14         # the alias is not counted twice
    assert not m.net[0].omega_0.requires_grad and not m.net[1].scale_0.requires_grad and m.net[0].omega_0.shape == (1,)


def test_load_state_dict_round_trip():
    torch.manual_seed(1)
    a = Wire(6, 64, 2, 1, 1.2, 1.5, 0.7)
    torch.manual_seed(2)
    b = Wire(6, 64, 2, 1)
    b.load_state_dict(a.state_dict())
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    d = b.desc()
    assert (d.first_omega, d.hidden_omega, d.first_scale, d.hidden_scale) == tuple(float(np.float32(v)) for v in (1.2, 1.5, 0.7, 0.7))
    with torch.no_grad():
        b.net[2].omega_0.fill_(3.0)
    with pytest.raises(ValueError, match="differ among themselves"):
        b.desc()


def test_drop_in_import():
    compat = os.path.join(ROOT, "mri-super-resolution_amd", "compat")
    sys.path.insert(0, compat)
    try:
        sys.modules.pop("INRmodel", None)
        from INRmodel import ComplexGaborLayer2D as dropped
    finally:
        sys.path.remove(compat)
    assert dropped is ComplexGaborLayer2D
    layer = dropped(8, 32, is_first=True, omega0=1.2, sigma0=1.2)
    assert list(layer.state_dict().keys()) == ["omega_0", "scale_0", "linear.weight", "linear.bias", "scale_orth.weight",
                                               "scale_orth.bias"]
    with pytest.raises(RuntimeError, match="WireFitter"):
        layer(torch.zeros(4, 8, requires_grad=True))


def test_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inrhip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name) and hasattr(_lib.lib(), name), name
    assert "inr_wire_desc_t" in text and ctypes.sizeof(_lib.WireDesc) == 32


@pytest.mark.parametrize("in_f,hidden,layers", [(32, 32, 1), (40, 64, 0), (3, 256, 3), (1024, 128, 8), (1, 32, 2)])
def test_parameter_layout(in_f, hidden, layers):
    """Documented order, every tensor on a 16-byte boundary, no overlap, omega_0 / scale_0 not in the buffer."""
    lib, desc = _lib.lib(), _desc(in_f, hidden, layers)
    n = 4 * (layers + 1) + 2
    offs = (ctypes.c_int64 * n)()
    assert lib.inr_wire_param_offsets(ctypes.byref(desc), offs, n) == 0
    assert lib.inr_wire_param_offsets(ctypes.byref(desc), offs, n - 1) == _lib.INR_E_INVALID
    offs = list(offs)
    sizes = []
    for l in range(layers + 1):
        sizes += [hidden * in_f, hidden] * 2 if l == 0 else [2 * hidden * hidden, 2 * hidden] * 2
    sizes += [2 * hidden, 2]
    assert offs[0] == 0 and all(o % 4 == 0 for o in offs)
    for k in range(n - 1):
        assert offs[k + 1] == offs[k] + (sizes[k] + 3) // 4 * 4, k                 # back to back up to the padding: no overlap
    assert lib.inr_wire_param_count(ctypes.byref(desc)) == offs[-1] + 4
    torch.manual_seed(0)
    m = Wire(in_f, hidden, layers, 1)
    assert [p.numel() * (2 if p.is_complex() else 1) for p in m.kernel_parameters()] == sizes


def test_flat_params_carve_complex_tensors_as_live_views():
    torch.manual_seed(0)
    m = Wire(5, 32, 1, 1)
    desc = _desc(5, 32, 1)
    n = 10
    offs = (ctypes.c_int64 * n)()
    assert _lib.lib().inr_wire_param_offsets(ctypes.byref(desc), offs, n) == 0
    fp = FlatParams(_lib.lib().inr_wire_param_count(ctypes.byref(desc)), list(offs))
    params = m.kernel_parameters()
    before = [p.detach().clone() for p in params]
    flat = fp.adopt(params)
    assert fp.owns(params) and flat.dtype == torch.float32
    for p, b, off in zip(params, before, offs):
        assert torch.equal(p.detach(), b) and p.dtype == b.dtype
        real = torch.view_as_real(p.detach()) if p.is_complex() else p.detach()
        assert torch.equal(flat[off:off + real.numel()], real.reshape(-1))
    flat[offs[4] + 1] = 7.0                                                         # the imaginary part of net.1.linear.weight[0, 0]
    assert m.net[1].linear.weight[0, 0].imag.item() == 7.0
    assert m.state_dict()["net.1.linear.weight"][0, 0].imag.item() == 7.0
    split = fp.split(torch.arange(flat.numel(), dtype=torch.float32))
    assert split[4].dtype == torch.complex64 and split[4][0, 1] == complex(offs[4] + 2, offs[4] + 3)
    assert split[0].dtype == torch.float32 and split[0].shape == (32, 5)


@pytest.mark.parametrize("kw", [dict(out_features=2), dict(hidden_features=48), dict(hidden_features=512), dict(hidden_features=16),
                                dict(in_features=1025), dict(in_features=0), dict(hidden_layers=9), dict(hidden_layers=-1)])
def test_unsupported_shapes_raise(kw):
    args = dict(in_features=32, hidden_features=64, hidden_layers=1, out_features=1)
    args.update(kw)
    with pytest.raises(ValueError):
        Wire(**args)
    lib = _lib.lib()
    desc = _desc(args["in_features"], args["hidden_features"], args["hidden_layers"], args["out_features"])
    offs = (ctypes.c_int64 * 64)()
    assert lib.inr_wire_param_count(ctypes.byref(desc)) == -1
    assert lib.inr_wire_param_offsets(ctypes.byref(desc), offs, 64) == _lib.INR_E_INVALID
    assert lib.inr_wire_workspace_bytes(ctypes.byref(desc), 1024, 1) == 0
    assert lib.inr_wire_reconstruct_workspace_bytes(ctypes.byref(desc), 1024) == 0
    assert lib.inr_wire_forward(ctypes.byref(desc), _fake(1), _fake(2), 8, _fake(3), _fake(4), 1 << 30, None) == _lib.INR_E_INVALID


def test_trainable_raises():
    with pytest.raises(ValueError, match="trainable"):
        ComplexGaborLayer2D(8, 32, is_first=True, trainable=True)


def test_argument_errors_are_refused_before_device_work():
    lib, desc = _lib.lib(), _desc()
    d = ctypes.byref(desc)
    n = 100
    inf, train = lib.inr_wire_workspace_bytes(d, n, 0), lib.inr_wire_workspace_bytes(d, n, 1)
    assert 0 < inf < train and lib.inr_wire_workspace_bytes(d, 0, 1) == 0 and lib.inr_wire_workspace_bytes(d, 1 << 40, 0) == 0
    assert lib.inr_wire_workspace_bytes(None, n, 0) == 0 and lib.inr_wire_param_count(None) == -1
    E, W, A = _lib.INR_E_INVALID, _lib.INR_E_WORKSPACE, _lib.INR_E_ALIGN
    odd = ctypes.c_void_p(0x7000_0000_0004)

    fwd = lambda p=_fake(1), x=_fake(2), rows=n, y=_fake(3), w=_fake(4), wb=inf, dd=d: lib.inr_wire_forward(dd, p, x, rows, y, w, wb, None)
    assert fwd(dd=None) == E and fwd(p=None) == E and fwd(x=None) == E and fwd(y=None) == E and fwd(rows=-1) == E
    assert b"bad row count" in lib.inr_last_error()
    assert fwd(w=None) == W and fwd(wb=inf - 1) == W
    assert b"workspace too small" in lib.inr_last_error()
    assert fwd(p=odd) == A and fwd(w=odd) == A

    shape = (ctypes.c_int64 * 3)(7, 5, 3)
    rws = lib.inr_wire_reconstruct_workspace_bytes(d, 64)
    assert rws > 0 and lib.inr_wire_reconstruct_workspace_bytes(d, 0) == 0
    rec = lambda p=_fake(1), sh=shape, dim=3, B=_fake(5), m=16, y=_fake(3), chunk=64, w=_fake(4), wb=rws: \
        lib.inr_wire_reconstruct(d, p, sh, dim, B, m, y, 1, 0.0, chunk, w, wb, None)
    assert rec(p=None) == E and rec(sh=None) == E and rec(y=None) == E and rec(dim=0) == E and rec(dim=9) == E and rec(chunk=0) == E
    assert rec(m=15) == E
    assert b"2*m" in lib.inr_last_error()
    assert rec(B=None) == E                                                        # raw coordinates need in_features == dim
    assert b"without B" in lib.inr_last_error()
    assert rec(sh=(ctypes.c_int64 * 3)(7, 0, 3)) == E
    assert rec(w=None) == W and rec(wb=rws - 1) == W and rec(w=odd) == A

    lg = lambda p=_fake(1), g=_fake(2), x=_fake(3), t=_fake(5), rows=n, w=_fake(4), wb=train: \
        lib.inr_wire_loss_grad(d, p, g, x, t, None, rows, _fake(6), w, wb, None)
    assert lg(p=None) == E and lg(g=None) == E and lg(x=None) == E and lg(t=None) == E and lg(rows=0) == E
    assert lg(w=None) == W and lg(wb=inf) == W and lg(g=odd) == A

    fit = lambda p=_fake(1), g=_fake(2), m=_fake(7), v=_fake(8), x=_fake(3), t=_fake(5), rows=n, first=1, steps=3, w=_fake(4), wb=train: \
        lib.inr_wire_fit(d, p, g, m, v, x, t, None, rows, first, steps, 5e-5, 0.9, 0.999, 1e-8, None, w, wb, None)
    assert fit(p=None) == E and fit(m=None) == E and fit(v=None) == E and fit(x=None) == E and fit(rows=0) == E
    assert fit(first=0) == E and fit(steps=-1) == E
    assert b"first_step" in lib.inr_last_error()
    assert fit(w=None) == W and fit(wb=train - 1) == W and fit(m=odd) == A

    lws = lib.inr_wire_layer_workspace_bytes(n, 32, 32)
    layer = lambda out=_fake(1), x=_fake(2), lw=_fake(3), fin=32, H=32, first=1, w=_fake(4), wb=lws: \
        lib.inr_wire_layer_forward(out, x, lw, _fake(5), _fake(6), _fake(7), n, fin, H, first, 1.2, 1.2, w, wb, None)
    assert layer(out=None) == E and layer(lw=None) == E and layer(H=48) == E and layer(fin=0) == E and layer(fin=16, first=0) == E
    assert b"in_features == out_features" in lib.inr_last_error()
    assert layer(w=None) == W and layer(wb=lws - 1) == W and layer(x=odd) == A


def _hybrid_raw():
    raw = np.empty((4, 2), dtype=object)
    for b in range(4):
        for te in range(2):
            raw[b, te] = np.ones((20, 20, 3, 1 if b == 0 else 2))
    return {"hybrid_raw": raw, "b": np.array([0.0, 150.0, 1000.0, 1500.0])}


def test_driver_refuses_what_wire_does_not_serve_before_any_device_call(tmp_path, monkeypatch):
    """--derivative_maps, and single acquisitions with a PerturbNet phase: refused before the input's acquisition products
    (the driver's first device work) are formed.  These run without a GPU."""
    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(drivers, "acquisition_products", no_device)
    monkeypatch.setattr(dwi_script.inr, "ImageFitting_set", no_device)
    vol = {"vol": np.random.default_rng(0).random((20, 20, 6, 4)) + 0.5, "b": np.array([0.0, 150.0, 1000.0, 1500.0])}
    plain = str(tmp_path / "pat03_vol.mat")
    matio.savemat(plain, vol)
    base = ["--output_address", str(tmp_path / "res"), "--number_of_epochs", "4", "--hidden_dim", "64", "--num_layers", "1",
            "--mapping_size", "8", "--roi_start", "2", "--roi_end", "18", "--model", "wire"]
    with pytest.raises(ValueError, match="no derivative maps of a WIRE network"):
        dwi_script.main(["--data", plain, "--derivative_maps", *base])
    with pytest.raises(ValueError, match="hidden_dim // 2"):
        dwi_script.main(["--data", plain, *base, "--hidden_dim", "96"])
    monkeypatch.setattr(matio, "loadmat", lambda path: _hybrid_raw())
    with pytest.raises(ValueError, match="PerturbNet phase"):
        dwi_script.main(["--data", "pat09_master.mat", *base])                    # --pertubation_epochs defaults to 10
    with pytest.raises(AssertionError, match="device work"):                      # without a PerturbNet phase the input is served
        dwi_script.main(["--data", "pat09_master.mat", *base, "--pertubation_epochs", "0"])


def test_new_flags_default_to_the_siren_path():
    args = dwi_script.build_parser().parse_args(["--data", "x.mat"])
    assert args.model == "siren" and args.wire_omega == 1.2 and args.wire_scale == 1.2
    assert dwi_script._check_model(args) is None
    args.derivative_maps = True
    assert dwi_script._check_model(args) is None                                  # the SIREN keeps its derivative maps
