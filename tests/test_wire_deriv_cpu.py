"""CPU-only checks of the WIRE derivative entry points (csrc/wire_deriv.hip; nn_mri.py:205-221 on the stack of wiretest.ipynb cell
2): the pin of tests/wire_deriv_common.py's float64 restatement to the reference's own network (tests/golden/wire_deriv.npz, written
by tools/make_wire_deriv_golden.py), the forward-mode formulas of DESIGN.md 4e against double-backward autograd on every case of
the GPU table, the C ABI names, the planner's values, every argument refusal with fake pointers and no device, and the Python and
driver refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import wire_deriv_common as wc
import mri_super_resolution_amd as inr
from mri_super_resolution_amd import _lib, drivers, matio, ops, wire
from mri_super_resolution_amd._build import LIB_PATH, SOURCES, build_library
from mri_super_resolution_amd.scripts import superresDWI as dwi_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["inr_wire_derivatives", "inr_wire_derivatives_grid", "inr_wire_derivatives_workspace_floats"]
INV, WS, AL = _lib.INR_E_INVALID, _lib.INR_E_WORKSPACE, _lib.INR_E_ALIGN

_REF = {}


def reference(name):
    """The case and its float64 double-backward reference, computed once and left unchanged."""
    if name not in _REF:
        case = wc.get_case(name)
        _REF[name] = (case, wc.autograd_reference(case))
    return _REF[name]


def fake(k):
    return ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)      # never dereferenced: the calls fail in validation


def test_restatement_is_pinned_to_the_reference_network(golden):
    """The plain complex stack and its double-backward derivatives against the reference's ComplexGaborLayer2D / input_mapping in
    float64 with the helpers of nn_mri.py:205-221, on the reference's own seeded weights: 1e-12 of each tensor's maximum."""
    g = golden("wire_deriv.npz")
    case, ref = reference("fixture")
    assert case["x"].shape == (333, 3) and torch.equal(case["x"], wc.mgrid_rows((3, 3, 37)))
    assert (case["m"], case["hidden"], case["layers"], case["dt"]) == (8, 32, 1, 3)
    desc = case["model"].desc()
    assert desc.first_omega == desc.hidden_omega == desc.first_scale == desc.hidden_scale == np.float32(1.2)
    for name, got in zip(("y", "grad", "lap"), ref):
        assert got.shape == g[name].shape and wc.max_rel(got, g[name]) <= 1e-12, name
    assert os.path.getsize(wc.GOLDEN) < 100_000
    for name in ("y", "grad", "lap"):          # the reference's own float32 noise on this case is far below the GPU tolerances
        assert 0 < float(g["noise/" + name]) < 2e-6, name


@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_forward_mode_formulas_equal_double_backward_in_float64(name):
    case, ref = reference(name)
    # a Gaussian window that underflows a whole output would let anything pass
    assert float(ref[0].abs().max()) >= 1e-3 and float(ref[1].norm()) > 0 and float(ref[2].norm()) > 0
    assert ref[1].shape == (case["x"].shape[0], case["dt"])
    for what, got, want in zip(("y", "grad", "lap"), wc.forward_formulas(case, torch.float64), ref):
        assert wc.max_rel(got, want) <= 1e-12, what


def test_d_tangent_sums_the_laplacian_over_the_leading_axes_only():
    case, ref = reference("notebook")          # d = 4, dt = 3
    full = wc.autograd_reference(case, 4)
    assert torch.equal(full[1][:, :3], ref[1]) and wc.rel_l2(full[2], ref[2]) > 1e-3
    for got, want in zip(wc.forward_formulas(case, torch.float64, 4), full):
        assert wc.max_rel(got, want) <= 1e-12


def test_new_header_names_signatures_and_exports():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inrhip.h")).read(), flags=re.S)
    declared = sorted(s for s in set(re.findall(r"\b(inr_[a-z0-9_]+)\s*\(", text)) if "derivatives" in s)
    assert declared == NEW
    assert sorted(k for k in _lib.SIGNATURES if "derivatives" in k) == NEW
    # names the closed lists of the older test files do not pick up
    assert not any("jet" in s or s.endswith("_workspace_bytes") for s in NEW)
    assert "wire_deriv.hip" in SOURCES
    build_library()
    handle = ctypes.CDLL(LIB_PATH)
    for s in NEW:
        assert hasattr(handle, s), s
    # the workspace is counted in floats with an int64_t, in the planner and in both entry points
    assert _lib.SIGNATURES[NEW[2]][0] is ctypes.c_int64
    for s in NEW[:2]:
        argtypes = _lib.SIGNATURES[s][1]
        assert argtypes[-3:] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert callable(ops.wire_derivatives) and callable(wire.derivatives)


def _q(desc, d, m, chunk, lap):
    return _lib.lib().inr_wire_derivatives_workspace_floats(ctypes.byref(desc), d, m, chunk, lap)


def wdesc(in_f, hidden, layers, out=1, consts=(1.2, 1.2, 1.2, 1.2)):
    return _lib.WireDesc(in_f, hidden, layers, out, *consts)


def test_planner_values_are_pinned():
    """(with, without the Laplacian) in floats: images [2][H][K0] + [4][H][2H] per hidden layer, 4H packed biases per layer, the
    input jets [J][chunk][K0] and two buffers [J][chunk][2H], J = 1 + d + lap, every region on a 256-byte boundary."""
    pinned = {((16, 32, 1), 3, 8, 256): (215296, 174336),
              ((32, 64, 2), 3, 16, 256): (439040, 365312),
              ((2, 32, 1), 2, 0, 256): (174336, 133376),
              ((40, 128, 1), 4, 20, 130): (597760, 522880),
              ((512, 128, 3), 4, 256, 32768): (201852928, 168298496)}
    for (shape, d, m, chunk), want in pinned.items():
        got = tuple(_q(wdesc(*shape), d, m, chunk, lap) for lap in (1, 0))
        assert got == want, (shape, got)
        assert 0 < got[1] < got[0]
    # the first one by hand
    assert 215296 == (2 * 32 * 32 + 128) + (8 * 32 * 32 + 128) + 5 * 256 * 32 + 2 * 5 * 256 * 64
    desc = wdesc(32, 64, 2)
    assert _q(desc, 3, 16, 512, 1) > _q(desc, 3, 16, 256, 1)


def test_planner_returns_zero_for_what_is_not_served():
    lib = _lib.lib()
    good = wdesc(32, 64, 2)
    assert _q(good, 3, 16, 256, 1) > 0
    assert lib.inr_wire_derivatives_workspace_floats(None, 3, 16, 256, 1) == 0
    for bad in (wdesc(32, 48, 2), wdesc(32, 512, 2), wdesc(32, 64, 9), wdesc(32, 64, 2, out=2), wdesc(2048, 64, 2),
                wdesc(32, 64, 2, consts=(float("inf"), 1.2, 1.2, 1.2))):
        assert _q(bad, 3, 16, 256, 1) == 0
    assert _q(good, 3, 15, 256, 1) == 0 and b"2*m" in lib.inr_last_error()           # in_features != 2m
    assert _q(good, 3, 0, 256, 1) == 0 and b"without B" in lib.inr_last_error()      # raw coordinates need in_features == d
    assert _q(good, 5, 16, 256, 1) == 0 and _q(good, 0, 16, 256, 1) == 0
    assert _q(good, 3, 16, 0, 1) == 0 and _q(good, 3, 16, 1 << 31, 1) == 0


def _rows(lib, desc, *, params=1, x=2, n=100, d=3, dt=None, B=3, m=16, y=4, grad=5, lap=6, chunk=64, ws=7, ws_floats=None):
    p = lambda k: None if k is None else fake(k)
    if ws_floats is None:
        ws_floats = _q(desc, d, m if B is not None else 0, min(chunk, n), 1)
    return lib.inr_wire_derivatives(ctypes.byref(desc), p(params), p(x), n, d, d if dt is None else dt, p(B), m, p(y), p(grad),
                                    p(lap), chunk, p(ws), ws_floats, None)


def _grid(lib, desc, *, params=1, shape=(5, 4, 5), dt=None, B=3, m=16, y=4, grad=5, lap=6, chunk=64, ws=7, ws_floats=None,
          null_shape=False):
    p = lambda k: None if k is None else fake(k)
    d = len(shape)
    if ws_floats is None:
        ws_floats = _q(desc, d, m if B is not None else 0, chunk, 1)
    return lib.inr_wire_derivatives_grid(ctypes.byref(desc), p(params), None if null_shape else _lib.shape_array(shape), d,
                                         d if dt is None else dt, p(B), m, p(y), p(grad), p(lap), chunk, p(ws), ws_floats, None)


def test_every_refusal_happens_before_any_device_work():
    lib = _lib.lib()
    good = wdesc(32, 64, 2)          # Fourier, m = 16
    raw = wdesc(3, 64, 2)

    def refused(rc, code, word):
        assert rc == code, (rc, lib.inr_last_error())
        assert word in lib.inr_last_error(), lib.inr_last_error()

    big = 1 << 40
    for call in (_rows, _grid):
        refused(call(lib, wdesc(32, 64, 2, out=2)), INV, b"out_features must be 1")
        for hidden in (48, 16, 512, 0):
            refused(call(lib, wdesc(32, hidden, 2), ws_floats=big), INV, b"hidden_features must be 32, 64, 128 or 256")
        refused(call(lib, wdesc(32, 64, 9), ws_floats=big), INV, b"hidden_layers")
        refused(call(lib, wdesc(32, 64, 2, consts=(1.2, float("nan"), 1.2, 1.2)), ws_floats=big), INV, b"finite")
        refused(call(lib, wdesc(30, 64, 2), ws_floats=big), INV, b"must equal 2*m")
        refused(call(lib, good, B=None), INV, b"without B in_features")           # in_features 32 != d
        refused(call(lib, raw, m=16), INV, b"must equal 2*m")                      # B given, in_features 3
        for name in ("params", "y"):
            refused(call(lib, good, **{name: None}), INV, b"null pointer")
        refused(call(lib, good, dt=0), INV, b"d_tangent")
        refused(call(lib, good, dt=4), INV, b"d_tangent")
        refused(call(lib, good, chunk=0), INV, b"chunk_rows")
        refused(call(lib, good, ws=None), WS, b"workspace too small")
        need = _q(good, 3, 16, 64, 1)
        refused(call(lib, good, ws_floats=need - 1), WS, b"workspace too small")     # exactly one float too few
        assert call(lib, good, ws_floats=need, params=None) == INV                    # (enough: the next refusal is another)
        # without the Laplacian, or without both, the planner's smaller value is enough -- and one float fewer is not
        need0 = _q(good, 3, 16, 64, 0)
        refused(call(lib, good, lap=None, ws_floats=need0 - 1), WS, b"workspace too small")
        refused(call(lib, raw, B=None, ws=None), WS, b"workspace too small")
    rc = lib.inr_wire_derivatives(None, fake(1), fake(2), 100, 3, 3, fake(3), 16, fake(4), None, None, 64, fake(7), big, None)
    refused(rc, INV, b"descriptor is null")
    refused(_rows(lib, good, x=None), INV, b"null pointer")
    refused(_rows(lib, good, n=-1), INV, b"bad row count")
    refused(_rows(lib, good, d=5, ws_floats=big), INV, b"coordinate axes")
    refused(_rows(lib, good, d=0, ws_floats=big), INV, b"coordinate axes")
    refused(_grid(lib, good, null_shape=True), INV, b"null pointer")
    refused(_grid(lib, good, shape=(5, 0, 5)), INV, b"shape[1]")
    refused(_grid(lib, good, shape=(2, 2, 2, 2, 2), ws_floats=big), INV, b"coordinate axes")
    # pointers off a 16-byte boundary
    odd = ctypes.c_void_p(0x7000_0000_0004)
    for call, second in ((lib.inr_wire_derivatives, (fake(2), 100, 3)), (lib.inr_wire_derivatives_grid, (_lib.shape_array((5, 4, 5)), 3))):
        rc = call(ctypes.byref(good), odd, *second, 3, fake(3), 16, fake(4), None, None, 64, fake(7), big, None)
        refused(rc, AL, b"params must be 16-byte aligned")
        rc = call(ctypes.byref(good), fake(1), *second, 3, fake(3), 16, fake(4), None, None, 64, odd, big, None)
        refused(rc, AL, b"workspace must be 16-byte aligned")
    # an empty call is valid and launches nothing
    assert _rows(lib, good, n=0, ws=None, ws_floats=0) == 0


def test_python_refusals_without_a_device(tmp_path, monkeypatch):
    torch.manual_seed(0)
    model = wire.Wire(2, 32, 1, 1)
    x = torch.rand(5, 2)
    with pytest.raises(ValueError, match="exactly one of coords and shape"):
        wire.derivatives(model)
    with pytest.raises(ValueError, match="exactly one of coords and shape"):
        wire.derivatives(model, x, shape=(3, 3))
    with pytest.raises(ValueError, match="exactly one of x and shape"):
        ops.wire_derivatives(model.desc(), torch.zeros(4))
    # laplace keeps refusing what is no direct output of a Siren or a Wire
    xg = x.clone().requires_grad_(True)
    with pytest.raises(TypeError, match="only for direct Siren outputs"):
        inr.laplace((xg * xg).sum(dim=-1, keepdim=True), xg)

    # --wire_derivative_maps without --model wire: refused before the input is loaded and anything touches the device
    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(drivers, "acquisition_products", no_device)
    monkeypatch.setattr(dwi_script.inr, "ImageFitting_set", no_device)
    monkeypatch.setattr(matio, "loadmat", no_device)
    base = ["--data", "pat03_vol.mat", "--output_address", str(tmp_path / "res"), "--number_of_epochs", "4", "--hidden_dim", "64",
            "--num_layers", "1", "--mapping_size", "8", "--roi_start", "2", "--roi_end", "18"]
    with pytest.raises(ValueError, match=r"--wire_derivative_maps.*needs --model wire.*--derivative_maps"):
        dwi_script.main([*base, "--wire_derivative_maps"])
    # under --model wire the flag passes the checks (the next thing the driver does is load the input) ...
    with pytest.raises(AssertionError, match="device work"):
        dwi_script.main([*base, "--model", "wire", "--wire_derivative_maps"])
    # ... and the SIREN's flag stays refused there
    with pytest.raises(ValueError, match="no derivative maps of a WIRE network"):
        dwi_script.main([*base, "--model", "wire", "--derivative_maps"])
    args = dwi_script.build_parser().parse_args(["--data", "x.mat"])
    assert args.wire_derivative_maps is False and dwi_script._check_model(args) is None
