"""-m gpu: the forward-mode derivative kernels of the WIRE network (csrc/wire_deriv.hip; nn_mri.py:205-221 on the stack of
wiretest.ipynb cell 2) against the float64 double-backward restatement of tests/wire_deriv_common.py, their bit-equalities, the
workspace guard, the Python surface (wire.derivatives, inr.laplace on a Wire output) and the superresDWI --wire_derivative_maps
product.

Shapes: the case table of wire_deriv_common.CASES -- the smallest at which the 32-row x 32-unit tiles, the K blocks of 32 and the
chunks can go wrong --, each with chunk_rows = 256 unless it has fewer rows.
Tolerances (the rule of tests/test_gpu_jet.py), always against the float64 restatement: y and the gradient relative L2 <= 1e-5; the
Laplacian relative L2 <= max(1e-5, 4 x the deviation of the same formulas in plain float32 torch on the host from float64, measured
here on the same case)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import wire_deriv_common as wc
import mri_super_resolution_amd as inr
from mri_super_resolution_amd import _lib, matio, ops, wire
from mri_super_resolution_amd.scripts import superresDWI as dwi_script

pytestmark = pytest.mark.gpu
T1 = 1e-5

_CACHE = {}


def host_case(name):
    """The case, its float64 reference and the float32 deviation of the formulas, computed once and left unchanged."""
    if name not in _CACHE:
        case = wc.get_case(name)
        ref = wc.autograd_reference(case)
        f32 = wc.forward_formulas(case, torch.float32)
        _CACHE[name] = (case, ref, wc.rel_l2(f32[2], ref[2]))
    return _CACHE[name]


def run(case, **kw):
    desc, flat, x, B = wc.on_device(case)
    kw.setdefault("d_tangent", case["dt"])
    kw.setdefault("chunk_rows", wc.CHUNK)
    if "shape" not in kw:
        kw.setdefault("x", x)
    return ops.wire_derivatives(desc, flat, B=B, **kw)


def check_accuracy(tag, got, ref, dev32):
    """``got`` = (y, grad, lap) of one call; an output the call was not asked for (None) has no error."""
    errs = tuple(0.0 if out is None else wc.rel_l2(out, want) for out, want in zip(got, ref))
    lap_bound = max(T1, 4 * dev32)
    print(f"wire derivatives {tag}: rel-L2 y {errs[0]:.3e} grad {errs[1]:.3e} lap {errs[2]:.3e} (float32 host formulas "
          f"{dev32:.3e}, lap bound {lap_bound:.3e})")
    assert errs[0] <= T1 and errs[1] <= T1, errs
    assert errs[2] <= lap_bound, errs


@pytest.mark.parametrize("name", list(wc.CASES))
def test_accuracy_against_float64_double_backward(name):
    case, ref, dev32 = host_case(name)
    n = case["x"].shape[0]
    assert float(ref[0].abs().max()) >= 1e-3 and float(ref[1].norm()) > 0 and float(ref[2].norm()) > 0
    got = run(case, chunk_rows=min(wc.CHUNK, n))
    assert tuple(got[0].shape) == (n,) and tuple(got[1].shape) == (n, case["dt"]) and tuple(got[2].shape) == (n,)
    check_accuracy(name, got, ref, dev32)
    # the value against the inference forward: other kernels (another tile shape), both within T1 of float64
    desc, flat, x, B = wc.on_device(case)
    feats = x if B is None else ops.fourier_map(x, B)
    y_fwd = case["model"](feats)[:, 0]
    print(f"wire derivatives {name}: y bit-equal with inr_wire_forward: {bool(torch.equal(y_fwd, got[0]))}, rel-L2 "
          f"{wc.rel_l2(got[0], y_fwd):.3e}")
    assert wc.rel_l2(got[0], y_fwd) <= 2 * T1


def test_fixture_case_meets_the_reference_values(golden):
    g = golden("wire_deriv.npz")
    case, _, dev32 = host_case("fixture")
    check_accuracy("fixture against the reference's own values", run(case),
                   tuple(torch.from_numpy(g[k]) for k in ("y", "grad", "lap")), dev32)


def test_bits_do_not_depend_on_chunking_position_repetition_or_requested_outputs():
    case, _, _ = host_case("ragged")
    n = case["x"].shape[0]
    assert n == 1023
    y, g, lap = run(case)
    for other in (run(case), run(case, chunk_rows=n)):           # a second run; one chunk
        assert torch.equal(other[0], y) and torch.equal(other[1], g) and torch.equal(other[2], lap)
    _, _, x, _ = wc.on_device(case)
    sub = run(case, x=x[37:170].contiguous())                    # other places in the chunk and in the tiles
    assert torch.equal(sub[0], y[37:170]) and torch.equal(sub[1], g[37:170]) and torch.equal(sub[2], lap[37:170])
    y1, g1, lap1 = run(case, want_lap=False)
    assert lap1 is None and torch.equal(y1, y) and torch.equal(g1, g)
    y2, g2, lap2 = run(case, want_grad=False)
    assert g2 is None and torch.equal(y2, y) and torch.equal(lap2, lap)
    y3, g3, lap3 = run(case, want_grad=False, want_lap=False)
    assert g3 is None and lap3 is None and torch.equal(y3, y)
    assert bool(torch.isfinite(lap).all()) and float(lap.abs().max()) > 1.0


def test_grid_entry_point_is_bit_equal_with_explicit_rows():
    for name in ("ragged", "raw"):                                # Fourier features and raw coordinates
        case, ref, dev32 = host_case(name)
        _, _, x, _ = wc.on_device(case)
        assert torch.equal(inr.get_mgrid(case["grid"]), x)
        rows = run(case)
        grid = run(case, shape=case["grid"])
        for a, b in zip(grid, rows):
            assert torch.equal(a, b)
        check_accuracy(f"{name} (grid)", grid, ref, dev32)


@pytest.mark.parametrize("dt", [1, 2, 3, 4])
def test_d_tangent_names_the_leading_axes(dt):
    """Case j6 (four axes) with tangents along the ``dt`` leading ones: the gradient equals those columns of the full call bit for
    bit, and the Laplacian the float64 restatement summed over those axes only.  Each ``dt`` runs with the Laplacian, without it
    and without either derivative: together every (tangents, Laplacian) pair the layer kernel is built for, each against
    float64."""
    case, ref, _ = host_case("j6")
    n = case["x"].shape[0]
    full = run(case)
    y, g, lap = run(case, d_tangent=dt)
    assert tuple(g.shape) == (n, dt)
    assert torch.equal(y, full[0]) and torch.equal(g, full[1][:, :dt].contiguous())
    ref_dt = wc.autograd_reference(case, dt)
    dev32 = wc.rel_l2(wc.forward_formulas(case, torch.float32, dt)[2], ref_dt[2])
    check_accuracy(f"j6 (d_tangent = {dt})", (y, g, lap), ref_dt, dev32)
    if dt < case["d"]:
        assert wc.rel_l2(ref_dt[2], ref[2]) > 1e-2    # the axes left out do contribute: the two Laplacians differ
    no_lap = run(case, d_tangent=dt, want_lap=False)
    assert no_lap[2] is None
    check_accuracy(f"j6 (d_tangent = {dt}, no Laplacian)", no_lap, ref_dt, dev32)
    value = run(case, d_tangent=dt, want_grad=False, want_lap=False)
    assert value[1] is None and value[2] is None
    check_accuracy("j6 (value only)", value, ref_dt, dev32)


def test_workspace_guard_tail_stays_intact():
    """The planner's floats plus 4096 bytes of 0xA5 behind them: one rows call and one grid call leave the tail as it was."""
    case, _, _ = host_case("ragged")
    desc, flat, x, B = wc.on_device(case)
    n, d, dt, m = x.shape[0], case["d"], case["dt"], case["m"]
    lib = _lib.lib()
    floats = int(lib.inr_wire_derivatives_workspace_floats(ctypes.byref(desc), d, m, wc.CHUNK, 1))
    assert floats > 0
    for form in ("rows", "grid"):
        ws = torch.full((4 * floats + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        y = torch.empty(n, device="cuda")
        g = torch.empty(n, dt, device="cuda")
        lap = torch.empty(n, device="cuda")
        if form == "rows":
            rc = lib.inr_wire_derivatives(ctypes.byref(desc), flat.data_ptr(), x.data_ptr(), n, d, dt, B.data_ptr(), m, y.data_ptr(),
                                          g.data_ptr(), lap.data_ptr(), wc.CHUNK, ws.data_ptr(), floats, ops._stream())
        else:
            rc = lib.inr_wire_derivatives_grid(ctypes.byref(desc), flat.data_ptr(), _lib.shape_array(case["grid"]), d, dt,
                                               B.data_ptr(), m, y.data_ptr(), g.data_ptr(), lap.data_ptr(), wc.CHUNK, ws.data_ptr(),
                                               floats, ops._stream())
        assert rc == 0, lib.inr_last_error()
        torch.cuda.synchronize()
        assert bool((ws[4 * floats:] == 0xA5).all()), form
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(lap).all())


def test_derivatives_shapes_through_coords_or_shape():
    case, _, _ = host_case("ragged")
    model, B, shape = case["model"].cuda(), case["B"].cuda(), case["grid"]
    by_shape = wire.derivatives(model, shape=shape, B=B, d_tangent=2, chunk_rows=wc.CHUNK)
    by_rows = wire.derivatives(model, inr.get_mgrid(shape), B=B, d_tangent=2, chunk_rows=wc.CHUNK)
    assert isinstance(by_shape, inr.Derivatives)
    assert tuple(by_shape.value.shape) == shape and tuple(by_shape.gradient.shape) == shape + (2,)
    assert tuple(by_shape.laplacian.shape) == shape and tuple(by_rows.gradient.shape) == (1023, 2)
    assert tuple(by_rows.value.shape) == (1023,) and tuple(by_rows.laplacian.shape) == (1023,)
    for a, b in zip(by_shape, by_rows):
        assert torch.equal(a.reshape(-1), b.reshape(-1)) and not a.requires_grad
    full = wire.derivatives(model, shape=shape, B=B)
    assert tuple(full.gradient.shape) == shape + (3,) and torch.equal(full.gradient[..., :2], by_shape.gradient)
    no_lap = wire.derivatives(model, shape=shape, B=B, d_tangent=2, laplacian=False)
    assert no_lap.laplacian is None and torch.equal(no_lap.gradient, by_shape.gradient)


def test_laplace_and_gradient_on_a_direct_wire_output():
    case, ref, dev32 = host_case("raw")
    model = case["model"].cuda()
    x = case["x"].cuda().clone().requires_grad_(True)
    y = model(x)
    lap = inr.laplace(y, x)
    d = wire.derivatives(model, x)
    assert tuple(lap.shape) == (357, 1) and not lap.requires_grad
    assert torch.equal(lap[:, 0], d.laplacian)
    check_accuracy("laplace(Wire(2, 32, 1, 1))", (d.value, d.gradient, lap[:, 0]), ref, dev32)
    # the autograd route (stash, backward kernels) and the forward-mode route are different kernels computing the same quantity
    g_autograd = inr.gradient(y, x).detach()
    assert tuple(g_autograd.shape) == (357, 2)
    print(f"wire derivatives: autograd gradient against the forward-mode one rel-L2 {wc.rel_l2(g_autograd, d.gradient):.3e}")
    assert wc.rel_l2(g_autograd, d.gradient) <= T1 and wc.rel_l2(g_autograd, ref[1]) <= T1
    # a transformed output or another input: the named error
    with pytest.raises(TypeError, match="only for direct Siren outputs"):
        inr.laplace(2 * y, x)
    with pytest.raises(TypeError, match="only for direct Siren outputs"):
        inr.laplace(model(x), x.detach().clone().requires_grad_(True))
    # an output computed without a graph (input requires grad, grad mode off) is served all the same
    with torch.no_grad():
        assert torch.equal(inr.laplace(model(x), x), lap)


# ---- the driver ---------------------------------------------------------------------------------------------------------
def test_superresDWI_wire_derivative_maps(tmp_path):
    X = Y = 16
    Z, NB = 4, 4
    gx, gy, gz = np.meshgrid(np.linspace(0, 1, X), np.linspace(0, 1, Y), np.linspace(0, 1, Z), indexing="ij")
    vol = np.stack([300 * (1.2 + np.sin(3 * gx + gz) * np.cos(2 * gy)) * np.exp(-0.5 * b) for b in range(NB)], axis=-1)
    path = str(tmp_path / "pat070_vol.mat")
    matio.savemat(path, {"vol": vol, "b": np.array([0.0, 150.0, 1000.0, 1500.0])})
    net = ["--model", "wire", "--pertubation_epochs", "0", "--number_of_epochs", "20", "--hidden_dim", "64", "--num_layers", "2",
           "--mapping_size", "16", "--roi_start", "0", "--roi_end", "16", "--seed", "0"]
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    dwi_script.main(["--data", path, "--output_address", on, *net, "--wire_derivative_maps"])
    dwi_script.main(["--data", path, "--output_address", off, *net])
    d_on, d_off = os.path.join(on, "pat070"), os.path.join(off, "pat070")
    base = ["metrics.json", "recon.mat", "recon.npy", "ssim_scores.csv"]
    assert sorted(os.listdir(d_off)) == base and sorted(os.listdir(d_on)) == sorted(base + ["derivatives.mat"])
    recon = matio.loadmat(os.path.join(d_on, "recon.mat"))["recon"]
    assert recon.shape == (2 * X, 2 * Y, Z, NB)
    assert np.array_equal(recon, matio.loadmat(os.path.join(d_off, "recon.mat"))["recon"])
    maps = matio.loadmat(os.path.join(d_on, "derivatives.mat"))
    for key in ("grad_mag", "laplacian"):
        assert maps[key].shape == recon.shape and np.isfinite(maps[key]).all(), key
    assert (maps["grad_mag"] >= 0).all() and maps["grad_mag"].max() > 0 and np.abs(maps["laplacian"]).max() > 0
