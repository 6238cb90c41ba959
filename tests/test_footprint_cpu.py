"""CPU: the surface of the voxel-footprint forward model -- header, exports, ctypes table, workspace plans, every argument refusal
of csrc/footprint.hip before device work (fake pointers that are never dereferenced), the quadrature rules of ``Footprint``, the
driver flags and the device refusals of the Python entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mri_super_resolution_amd as inr
from mri_super_resolution_amd import _lib, drivers, matio
from mri_super_resolution_amd._build import LIB_PATH, SOURCES, build_library
from mri_super_resolution_amd.footprint import Footprint
from mri_super_resolution_amd.scripts import superresDWI as dwi_script
from mri_super_resolution_amd.scripts import wiretest as wt_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("inr_footprint_expand", "inr_footprint_reduce", "inr_footprint_loss_workspace_floats", "inr_footprint_loss_grad",
       "inr_siren_fit_footprint_workspace_floats", "inr_siren_fit_footprint")
E, W, A = _lib.INR_E_INVALID, _lib.INR_E_WORKSPACE, _lib.INR_E_ALIGN
MAX_ROWS = (1 << 31) - 256


def _fake(k, odd=0):
    return ctypes.c_void_p(0x7000_0000_0000 + 4096 * k + odd)      # never dereferenced: the calls fail in validation


def _desc(in_f=256, hidden=512, layers=3, out_f=1):
    return ctypes.byref(_lib.SirenDesc(in_f, hidden, layers, out_f, 30.0, 30.0))


def test_every_new_symbol_is_declared_exported_and_bound():
    build_library()
    assert "footprint.hip" in SOURCES
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inrhip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared in inrhip.h"
        assert hasattr(handle, name), f"{name} not exported"
        assert name in _lib.SIGNATURES, f"{name} not bound"
    # workspaces are (pointer, count in floats), planners end in _workspace_floats
    assert _lib.SIGNATURES["inr_footprint_loss_grad"][1][-3:-1] == [ctypes.c_void_p, ctypes.c_int64]
    assert _lib.SIGNATURES["inr_siren_fit_footprint"][1][-3:-1] == [ctypes.c_void_p, ctypes.c_int64]
    assert "#define INR_FOOTPRINT_MAX_SAMPLES 64" in text and inr.ops.FOOTPRINT_MAX_SAMPLES == 64


def test_planner_relations():
    lib = _lib.lib()
    plan = lib.inr_siren_fit_footprint_workspace_floats
    for n, K in ((1031, 4), (4096, 1), (1, 64), (28672, 12)):
        assert plan(_desc(), n, K) * 4 >= lib.inr_siren_fit_workspace_bytes(_desc(), n * K) + 8 * n * K, (n, K)
    assert plan(_desc(hidden=128, layers=1), 100, 4) > 0
    assert plan(_desc(hidden=64), 1031, 4) == 0                 # not served by the pre-split kernels
    assert plan(_desc(out_f=2), 1031, 4) == 0
    assert plan(_desc(), 1031, 65) == 0 and plan(_desc(), 1031, 0) == 0 and plan(_desc(), 0, 4) == 0
    assert plan(_desc(), MAX_ROWS // 4 + 1, 4) == 0 and plan(None, 1031, 4) == 0
    loss_plan = lib.inr_footprint_loss_workspace_floats
    assert loss_plan(1) >= 1 and loss_plan(4099) >= 1 and loss_plan(0) == 0 and loss_plan(MAX_ROWS + 1) == 0
    assert loss_plan(1 << 30) <= 4096                           # a fixed grid: the partials do not grow with n


def test_element_kernels_refuse_bad_arguments_before_device_work():
    lib = _lib.lib()
    expand = lambda out=_fake(1), x=_fake(2), off=_fake(3), n=67, d=2, K=3: lib.inr_footprint_expand(out, x, off, n, d, K, None)
    assert expand(out=None) == E and expand(x=None) == E and expand(off=None) == E
    assert b"null pointer" in lib.inr_last_error()
    assert expand(d=0) == E and expand(d=5) == E and b"coordinates per row" in lib.inr_last_error()
    assert expand(n=0) == E and b"datum count" in lib.inr_last_error()
    assert expand(K=0) == E and expand(K=65) == E and b"sub-samples" in lib.inr_last_error()
    assert expand(n=MAX_ROWS // 4 + 1, K=4) == E and b"too many rows" in lib.inr_last_error()

    reduce = lambda pred=_fake(1), y=_fake(2), fw=_fake(3), n=67, K=3: lib.inr_footprint_reduce(pred, y, fw, n, K, None)
    assert reduce(pred=None) == E and reduce(y=None) == E and reduce(fw=None) == E
    assert reduce(n=0) == E and reduce(n=-1) == E and reduce(K=0) == E and reduce(K=65) == E
    assert reduce(n=MAX_ROWS, K=2) == E and b"inr_footprint_reduce: too many rows" in lib.inr_last_error()

    n = 4099
    floats = lib.inr_footprint_loss_workspace_floats(n)
    lg = lambda gy=_fake(1), loss=_fake(2), pred=None, y=_fake(3), t=_fake(4), wt=None, fw=_fake(5), n=n, K=5, ct=0, ws=_fake(6), \
        wf=floats: lib.inr_footprint_loss_grad(gy, loss, pred, y, t, wt, fw, n, K, ct, ws, wf, None)
    assert lg(gy=None) == E and lg(loss=None) == E and lg(y=None) == E and lg(t=None) == E and lg(fw=None) == E
    assert lg(n=0) == E and lg(K=0) == E and lg(K=65) == E
    assert lg(ct=n - 1) == E and b"count_total" in lib.inr_last_error()
    assert lg(ws=None) == W and lg(wf=floats - 1) == W and lg(wf=-1) == W and b"workspace too small" in lib.inr_last_error()
    assert lg(ws=_fake(6, 4)) == A and b"16-byte aligned" in lib.inr_last_error()


def test_fit_refuses_bad_arguments_before_device_work():
    lib = _lib.lib()
    n, K = 1031, 4
    floats = lib.inr_siren_fit_footprint_workspace_floats(_desc(), n, K)
    assert floats > 0

    def fit(desc=None, p=_fake(1), g=_fake(2), m=_fake(3), v=_fake(4), x=_fake(5), t=_fake(6), wt=None, fw=_fake(7), n=n, K=K,
            first=1, steps=2, losses=None, ws=_fake(8), wf=floats):
        return lib.inr_siren_fit_footprint(desc or _desc(), p, g, m, v, x, t, wt, fw, n, K, first, steps, 1e-4, 0.9, 0.999, 1e-8,
                                           losses, ws, wf, None)

    for name in ("p", "g", "m", "v", "x", "t", "fw"):
        assert fit(**{name: None}) == E and b"null pointer" in lib.inr_last_error(), name
    assert fit(n=0) == E and fit(K=0) == E and fit(K=65) == E and b"sub-samples" in lib.inr_last_error()
    assert fit(n=MAX_ROWS // 4 + 1) == E and b"too many rows" in lib.inr_last_error()
    assert fit(first=0) == E and fit(steps=-1) == E and b"first_step" in lib.inr_last_error()
    assert fit(desc=_desc(in_f=0)) == E and b"bad siren descriptor" in lib.inr_last_error()
    for bad in (_desc(hidden=64), _desc(out_f=2), _desc(in_f=2, hidden=128)):        # what inr_siren_hp_eligible does not serve
        assert fit(desc=bad) == E and b"inr_siren_hp_eligible" in lib.inr_last_error()
    assert fit(ws=None) == W and fit(wf=floats - 1) == W and b"workspace too small" in lib.inr_last_error()
    assert fit(ws=_fake(8, 4)) == A and fit(p=_fake(1, 4)) == A and fit(g=_fake(2, 8)) == A and fit(x=_fake(5, 4)) == A
    assert b"16-byte aligned" in lib.inr_last_error()


def _moments(fp):
    w, x = fp.weights, fp.offsets
    mean = (w[:, None] * x).sum(axis=0)
    return w.sum(), mean, (w[:, None] * x * x).sum(axis=0)


def test_footprint_rules():
    spacing = (2.0 / 63, 2.0 / 49, 2.0 / 21)
    point = Footprint.point(3)
    assert point.count == 1 and point.offsets.shape == (1, 3) and not point.offsets.any() and point.weights.tolist() == [1.0]
    for widths, samples in (((2, 2, 0), (2, 2, 1)), ((2, 3, 4), (4, 3, 5)), ((1.5, 0, 2), (3, 4, 1)), ((2, 2, 2), (1, 1, 1))):
        fp = Footprint.box(widths, samples, spacing)
        total, mean, var = _moments(fp)
        live = [1 if (s == 1 or w == 0) else s for w, s in zip(widths, samples)]
        assert fp.count == int(np.prod(live)) and fp.offsets.shape == (fp.count, 3) and fp.dim == 3
        assert abs(total - 1.0) < 1e-12 and np.abs(mean).max() < 1e-12
        for a in range(3):
            want = (widths[a] * spacing[a]) ** 2 * (1.0 - 1.0 / live[a] ** 2) / 12.0 if live[a] > 1 else 0.0
            assert abs(var[a] - want) < 1e-12, (widths, samples, a)
    for fwhm, samples in (((2.0, 0, 3.0), (3, 2, 5)), ((1.0, 1.0, 1.0), (2, 2, 2)), ((0, 0, 2.5), (1, 1, 7))):
        fp = Footprint.gaussian(fwhm, samples, spacing)
        total, mean, var = _moments(fp)
        assert abs(total - 1.0) < 1e-12 and np.abs(mean).max() < 1e-12
        for a in range(3):
            sigma = fwhm[a] / 2.354820045 * spacing[a] if samples[a] > 1 else 0.0
            assert abs(var[a] - sigma ** 2) < 1e-12, (fwhm, samples, a)
    # the 2 x 2 block of HR pixels: nodes on the four HR samples around the block centre
    h = (2.0 / 63, 2.0 / 31)
    fp = Footprint.box((2, 2), (2, 2), h)
    want = [[-0.5 * h[0], -0.5 * h[1]], [-0.5 * h[0], 0.5 * h[1]], [0.5 * h[0], -0.5 * h[1]], [0.5 * h[0], 0.5 * h[1]]]
    assert np.allclose(fp.offsets, want, rtol=0, atol=1e-17) and fp.weights.tolist() == [0.25] * 4      # last axis fastest
    fp = Footprint.box((2, 4), (2, 3), 1.0)
    assert np.allclose(fp.offsets[:3, 0], -0.5) and np.allclose(fp.offsets[:3, 1], [-4 / 3, 0, 4 / 3]) and fp.count == 6
    fp = Footprint.gaussian((2.0, 1.0), (2, 3), 1.0)
    assert np.all(np.diff(fp.offsets[:3, 1]) > 0) and len(set(fp.offsets[:3, 0])) == 1
    assert Footprint.box((2, 2), 2, 0.1).count == 4                                                       # scalars apply to every axis


def test_footprint_validation():
    ok_off, ok_w = np.zeros((2, 2)), np.array([0.5, 0.5])
    for off, w in ((np.zeros(2), ok_w), (ok_off, np.ones((2, 1)) / 2), (np.zeros((3, 2)), ok_w), (np.zeros((0, 2)), np.zeros(0)),
                   (np.zeros((65, 2)), np.full(65, 1 / 65)), (np.zeros((2, 5)), ok_w), (np.zeros((2, 0)), ok_w),
                   (np.array([[0.0, np.nan], [0, 0]]), ok_w), (ok_off, np.array([np.inf, 0.5])), (ok_off, np.array([0.5, 0.6])),
                   (ok_off, np.array([0.5, 0.5 - 3e-6]))):
        with pytest.raises(ValueError):
            Footprint(off, w)
    Footprint(ok_off, np.array([0.5, 0.5 - 5e-7]))                        # within 1e-6
    assert Footprint(np.zeros((64, 4)), np.full(64, 1 / 64)).count == 64
    for bad in (lambda: Footprint.box((2, 2), (2, 2, 2), 1.0), lambda: Footprint.box((2, 2), (2, 0), 1.0),
                lambda: Footprint.box((2, -1), (2, 2), 1.0), lambda: Footprint.box((2, 2), (2, 2), (1.0,)),
                lambda: Footprint.box((2, 2), (9, 9), 1.0), lambda: Footprint.gaussian((1.0, 1.0), (0, 2), 1.0),
                lambda: Footprint.gaussian((1.0, float("nan")), (2, 2), 1.0), lambda: Footprint.gaussian((1.0,), (2, 2), 1.0)):
        with pytest.raises(ValueError):
            bad()


def _hybrid_raw():
    raw = np.empty((4, 2), dtype=object)
    for b in range(4):
        for te in range(2):
            raw[b, te] = np.ones((20, 20, 3, 1 if b == 0 else 2))
    return {"hybrid_raw": raw, "b": np.array([0.0, 150.0, 1000.0, 1500.0])}


def test_driver_flags_default_off_and_refuse_what_nothing_serves(tmp_path, monkeypatch):
    """Every refusal is reached while the flags are checked: before the input is loaded and before any device work."""
    args = dwi_script.build_parser().parse_args(["--data", "x.mat"])
    assert args.lr_model == "decimate" and args.footprint == "point" and args.footprint_samples == 2
    assert dwi_script._check_model(args) is None
    with pytest.raises(SystemExit):
        dwi_script.build_parser().parse_args(["--data", "x.mat", "--lr_model", "blur"])
    with pytest.raises(SystemExit):
        dwi_script.build_parser().parse_args(["--data", "x.mat", "--footprint", "gauss"])

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(drivers, "acquisition_products", no_device)
    monkeypatch.setattr(dwi_script.inr, "ImageFitting_set", no_device)
    plain = str(tmp_path / "pat03_vol.mat")
    matio.savemat(plain, {"vol": np.random.default_rng(0).random((20, 20, 2)) + 0.5})
    run = lambda data, r1, *flags: dwi_script.main(["--data", data, "--output_address", str(tmp_path / "res"), "--number_of_epochs", "1",
                                                    "--hidden_dim", "128", "--num_layers", "1", "--mapping_size", "16", "--roi_start", "2",
                                                    "--roi_end", str(r1), *flags])
    with pytest.raises(ValueError, match="--footprint box.*--lr_model average"):
        run(plain, 18, "--footprint", "box")
    with pytest.raises(ValueError, match="--lr_model average.*--model wire"):
        run(plain, 18, "--lr_model", "average", "--model", "wire")
    with pytest.raises(ValueError, match="--lr_model average.*--model wire"):
        run(plain, 18, "--lr_model", "average", "--footprint", "box", "--model", "wire")
    with pytest.raises(ValueError, match="--footprint box.*--lr_model average"):
        run(plain, 18, "--footprint", "box", "--model", "wire")
    with pytest.raises(ValueError, match="--lr_model average.*--zerofill"):
        run(plain, 18, "--lr_model", "average", "--zerofill")
    with pytest.raises(ValueError, match="--lr_model average.*even ROI side.*15"):
        run(plain, 17, "--lr_model", "average")
    with pytest.raises(ValueError, match="--footprint_samples must be 1 .. 8"):
        run(plain, 18, "--lr_model", "average", "--footprint", "box", "--footprint_samples", "9")
    monkeypatch.setattr(matio, "loadmat", lambda path: _hybrid_raw())
    with pytest.raises(ValueError, match="PerturbNet phase.*point-sampled.*--lr_model average"):
        run("pat09_master.mat", 18, "--lr_model", "average")                          # --pertubation_epochs defaults to 10
    with pytest.raises(AssertionError, match="device work"):                          # without that phase the input is served
        run("pat09_master.mat", 18, "--lr_model", "average", "--pertubation_epochs", "0")


def test_wiretest_and_other_fit_hooks_refuse_the_flags_they_inherit(tmp_path, monkeypatch):
    """scripts/wiretest.py builds its parser from superresDWI's and replaces ``_check_model``: the refusals must not depend on it."""
    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(drivers, "acquisition_products", no_device)
    monkeypatch.setattr(dwi_script.inr, "ImageFitting_set", no_device)
    monkeypatch.setattr(matio, "loadmat", no_device)                                  # refused before the input is even read
    args = wt_script.build_parser().parse_args(["--data", "x.mat"])
    assert args.lr_model == "decimate" and args.footprint == "point" and args.model == "wire"
    base = ["--data", "pat09_master.mat", "--output_address", str(tmp_path / "res"), "--number_of_epochs", "4", "--roi_start", "2",
            "--roi_end", "18"]
    with pytest.raises(ValueError, match="--lr_model average.*--model wire"):
        wt_script.main(base + ["--lr_model", "average"])
    with pytest.raises(ValueError, match="--lr_model average.*--model wire"):
        wt_script.main(base + ["--lr_model", "average", "--footprint", "box", "--pertubation_epochs", "0"])
    with pytest.raises(ValueError, match="--footprint box.*--lr_model average"):
        wt_script.main(base + ["--footprint", "box"])
    with pytest.raises(AssertionError, match="device work"):                          # without the flags the input is read
        wt_script.main(base)
    # any other driver's fit hook on the SIREN: it knows neither the block centres nor the n*K rows
    args = dwi_script.build_parser().parse_args(base + ["--lr_model", "average"])
    hook = lambda *a: no_device()
    with pytest.raises(ValueError, match="--lr_model average / --footprint box.*another driver's fit"):
        dwi_script.run_patient("pat09_master.mat", "09", args, fit=hook)
    with pytest.raises(ValueError, match="--lr_model average / --footprint box.*another driver's fit"):
        dwi_script.run_patient("pat09_master.mat", "09", args, check_model=lambda a: None, fit=hook)


def test_fit_cycle_batch_refuses_a_footprint_fitter():
    class Fake(inr.FootprintSirenFitter):
        def __init__(self):                                                           # (no device: only the class matters here)
            pass

    assert inr.SirenFitter.batch_ok and not inr.FootprintSirenFitter.batch_ok
    with pytest.raises(TypeError, match="point-sampled SirenFitter.*Fake"):
        inr.fit_cycle_batch([Fake()], None, [None], 1)


def test_fit_volume_refuses_bad_combinations_before_device_work():
    vol = np.random.default_rng(0).random((9, 8, 2)).astype(np.float32)
    fit = lambda **kw: drivers._fit_volume_once(vol, 1, hidden_features=128, hidden_layers=1, **kw)
    with pytest.raises(ValueError, match="lr_model must be"):
        fit(lr_model="blur")
    with pytest.raises(ValueError, match="footprint must be"):
        fit(footprint="gauss")
    with pytest.raises(ValueError, match="footprint='box'.*lr_model='average'"):
        fit(footprint="box")
    with pytest.raises(ValueError, match="rank group"):
        fit(lr_model="average", footprint="box", group=object())
    with pytest.raises(ValueError, match="even up-scaled axes"):
        fit(lr_model="average")
    with pytest.raises(ValueError, match="downsample=True"):
        drivers._fit_volume_once(vol[:8], 1, lr_model="average", downsample=False)
    with pytest.raises(ValueError, match="2 axes, the volume 3"):
        fit(footprint=Footprint.point(2))


def test_python_entry_points_refuse_cpu_tensors():
    fp = Footprint.box((2, 2), (2, 2), 2.0 / 63)
    with pytest.raises(inr.InrDeviceError):
        inr.footprint_inputs(torch.zeros(5, 2), torch.zeros(8, 2), fp)
    with pytest.raises(inr.InrDeviceError):
        inr.footprint_forward(inr.Siren(16, 128, 1, 1), torch.zeros(5, 2), torch.zeros(8, 2), fp)
    torch.manual_seed(0)
    with pytest.raises(inr.InrDeviceError):
        inr.FootprintSirenFitter(inr.Siren(256, 128, 1, 1), fp)
    with pytest.raises(TypeError):
        inr.FootprintSirenFitter(inr.Siren(256, 128, 1, 1), "box")
