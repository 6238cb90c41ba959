"""CPU-only checks of the through-plane spline entry point (inr_resize_z_cubic) and of the superresDWI options built on it:
the symbols are declared, exported and bound; every argument error is refused before any device work (fake device pointers
that are never dereferenced); the driver refuses --transverse_length / --adc on inputs that cannot give them before it fits."""
import ctypes
import os
import re

import numpy as np
import pytest

from mri_super_resolution_amd import _lib, baselines, matio
from mri_super_resolution_amd.scripts import superresDWI as dwi_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("inr_resize_z_cubic_workspace_bytes", "inr_resize_z_cubic")


def _fake(k):
    return ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)


def test_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inrhip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name) and hasattr(_lib.lib(), name), name


def test_workspace_bytes():
    lib = _lib.lib()
    assert lib.inr_resize_z_cubic_workspace_bytes(128 * 128, 24) == 128 * 128 * 24 * 8
    assert lib.inr_resize_z_cubic_workspace_bytes(1, 4) == 32
    assert lib.inr_resize_z_cubic_workspace_bytes(0, 0) >= 8          # never 0: a valid allocation size


def test_argument_errors_are_refused_before_device_work():
    lib = _lib.lib()
    ws = lib.inr_resize_z_cubic_workspace_bytes(10, 8)
    call = lambda out, inp, lines, n_in, n_out, w=_fake(3), wb=ws: lib.inr_resize_z_cubic(out, inp, lines, n_in, n_out, w, wb, None)
    assert call(None, _fake(2), 10, 8, 9) == _lib.INR_E_INVALID
    assert b"null pointer" in lib.inr_last_error()
    assert call(_fake(1), None, 10, 8, 9) == _lib.INR_E_INVALID
    for lines, n_in, n_out in ((0, 8, 9), (-1, 8, 9), (10, 0, 9), (10, -2, 9), (10, 8, 0), (10, 8, -5)):
        assert call(_fake(1), _fake(2), lines, n_in, n_out) == _lib.INR_E_INVALID, (lines, n_in, n_out)
        assert b"bad sizes" in lib.inr_last_error()
    assert call(_fake(1), _fake(2), 10, 3, 9) == _lib.INR_E_INVALID          # scipy refuses a cubic spline through 3 points too
    assert b"at least 4 samples" in lib.inr_last_error()
    assert call(_fake(1), _fake(2), 10, 8, 9, w=None) == _lib.INR_E_WORKSPACE
    assert call(_fake(1), _fake(2), 10, 8, 9, wb=ws - 8) == _lib.INR_E_WORKSPACE
    assert b"workspace too small" in lib.inr_last_error()
    assert call(_fake(1), _fake(2), 10, 8193, 9, wb=lib.inr_resize_z_cubic_workspace_bytes(10, 8193)) == _lib.INR_E_INVALID
    assert b"8192" in lib.inr_last_error()


def test_resize_z_refuses_other_kinds():
    with pytest.raises(ValueError, match="cubic"):
        baselines.resize_z(np.zeros((3, 8)), 9, kind="linear")


def test_new_flags_default_off():
    args = dwi_script.build_parser().parse_args(["--data", "x.mat"])
    assert args.transverse_length == 0 and args.adc is False


def _plain(tmp_path, shape, with_b=True, name="pat03_vol.mat"):
    vol = np.random.default_rng(0).random(shape) + 0.5
    data = {"vol": vol}
    if with_b:
        data["b"] = np.array([0.0, 150.0, 1000.0, 1500.0])[: (shape[3] if len(shape) == 4 else 1)]
    path = str(tmp_path / name)
    matio.savemat(path, data)
    return path, vol


def test_load_input_keeps_its_tuple_and_the_new_helper_returns_the_per_b_maxima(tmp_path):
    path, vol = _plain(tmp_path, (20, 20, 5, 4))
    old = dwi_script.load_input(path)
    assert len(old) == 4 and old[1] is None and old[3] is None
    mean_img, acq, bvals, maxes, scale = dwi_script.load_input_and_scale(path)
    assert np.array_equal(mean_img, old[0]) and np.array_equal(bvals, old[2]) and acq is None and maxes is None
    assert np.array_equal(scale, vol.reshape(-1, 4).max(axis=0))
    assert np.allclose(mean_img * scale, vol, rtol=1e-15, atol=0)


def _run(tmp_path, path, *flags):
    return dwi_script.main(["--data", path, "--output_address", str(tmp_path / "res"), "--number_of_epochs", "1",
                            "--hidden_dim", "16", "--num_layers", "1", "--mapping_size", "8", "--roi_start", "2",
                            "--roi_end", "18", *flags])


def test_driver_refuses_the_options_on_inputs_that_cannot_give_them(tmp_path):
    """All refused while checking the input, before any device work (these run without a GPU)."""
    two_slices, _ = _plain(tmp_path, (20, 20, 2, 4), name="pat01_vol.mat")
    with pytest.raises(ValueError, match="at least 4 slices"):
        _run(tmp_path, two_slices, "--transverse_length", "100")
    one_b, _ = _plain(tmp_path, (20, 20, 6), name="pat02_vol.mat")
    with pytest.raises(ValueError, match="at least 2 b-values"):
        _run(tmp_path, one_b, "--adc")
    no_b, _ = _plain(tmp_path, (20, 20, 6, 4), with_b=False, name="pat04_vol.mat")
    with pytest.raises(ValueError, match="distinct b-values"):
        _run(tmp_path, no_b, "--adc")
    ok, _ = _plain(tmp_path, (20, 20, 6, 4), name="pat05_vol.mat")
    with pytest.raises(ValueError, match=">= 0"):
        _run(tmp_path, ok, "--transverse_length", "-1")
