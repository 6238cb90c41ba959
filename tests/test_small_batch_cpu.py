"""CPU-only checks of the batched small-network fit entry point (inr_siren_fit_cycle_batch): it is declared, exported and
bound, the launch-family table grew by one, and every argument error is refused before any device work (fake device
pointers that are never dereferenced)."""
import ctypes
import os
import re

import pytest

from mri_super_resolution_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p


def test_batch_entry_point_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inrhip.h")).read(), flags=re.S)
    assert re.search(r"\binr_siren_fit_cycle_batch\s*\(", text)
    assert re.search(r"#define\s+INR_LF_SMALL_BATCH\s+13\b", text)
    assert re.search(r"#define\s+INR_LF_COUNT\s+14\b", text)
    assert "inr_siren_fit_cycle_batch" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "inr_siren_fit_cycle_batch")
    assert hasattr(_lib.lib(), "inr_siren_fit_cycle_batch")


def test_launch_family_count_and_name():
    assert _lib.INR_LF_COUNT == 14
    assert len(ops.LAUNCH_FAMILIES) == 14 and ops.LAUNCH_FAMILIES[13] == "small_batch"
    n = ctypes.c_int64(-1)
    assert _lib.lib().inr_launch_count(13, ctypes.byref(n)) == 0
    assert _lib.lib().inr_launch_count(14, ctypes.byref(n)) == _lib.INR_E_INVALID


def _fake(k, misalign=0):
    return 0x7000_0000_0000 + 4096 * k + misalign


def _arr(vals, ctype=P):
    return (ctype * len(vals))(*vals)


def _call(n_fits=2, params=None, workspaces=None, n_acq=None, first_acq=None, x=None, drop=None, null_entry=None,
          misalign=None):
    """A call that is valid except for what the arguments change."""
    lib = _lib.lib()
    desc = _lib.SirenDesc(2, 64, 6, 1, 30.0, 30.0)
    n = 3600
    wsb = lib.inr_siren_fit_workspace_bytes(ctypes.byref(desc), n)
    k = max(n_fits, 1)
    arrays = {
        "params": params or [_fake(10 + i) for i in range(k)],
        "grads": [_fake(30 + i) for i in range(k)],
        "m": [_fake(50 + i) for i in range(k)],
        "v": [_fake(70 + i) for i in range(k)],
        "targets": [_fake(90 + i) for i in range(k)],
        "workspaces": workspaces or [_fake(200 + 64 * i) for i in range(k)],
    }
    if null_entry:
        arrays[null_entry][k - 1] = None
    if misalign:
        arrays[misalign][0] += 4
    c = {name: _arr(v) for name, v in arrays.items()}
    na = _arr(n_acq or [3] * k, ctypes.c_int)
    fa = _arr(first_acq or [0] * k, ctypes.c_int)
    if drop == "n_acq":
        na = None
    if drop in c:
        c[drop] = None
    rc = lib.inr_siren_fit_cycle_batch(ctypes.byref(desc), n_fits, c["params"], c["grads"], c["m"], c["v"],
                                       _fake(1) if x is None else x, c["targets"], None, na, fa, n, 1, 10, 3e-4, 0.9, 0.999,
                                       1e-8, None, c["workspaces"], wsb, None)
    return rc, lib.inr_last_error().decode()


@pytest.mark.parametrize("case, kwargs, message", [
    ("n_fits", dict(n_fits=0), "n_fits must be >= 1"),
    ("null params array", dict(drop="params"), "null array"),
    ("null workspaces array", dict(drop="workspaces"), "null array"),
    ("null n_acq array", dict(drop="n_acq"), "null array"),
    ("null x", dict(x=0), "x is null"),
    ("null params entry", dict(null_entry="params"), "fit 1 has a null"),
    ("null targets entry", dict(null_entry="targets"), "fit 1 has a null"),
    ("null workspace entry", dict(null_entry="workspaces"), "fit 1 has a null"),
    ("shared params", dict(params=[_fake(10), _fake(10)]), "fits 0 and 1 share one params buffer"),
    ("shared workspace", dict(workspaces=[_fake(200), _fake(200)]), "fits 0 and 1 share one workspace"),
    ("misaligned params", dict(misalign="params"), "fit 0: params / grads / workspace are not 16-byte aligned"),
    ("misaligned workspace", dict(misalign="workspaces"), "fit 0: params / grads / workspace are not 16-byte aligned"),
    ("misaligned x", dict(x=_fake(1, 8)), "x is not 16-byte aligned"),
    ("n_acq < 1", dict(n_acq=[3, 0]), "fit 1: need n_acq >= 1"),
    ("first_acq >= n_acq", dict(first_acq=[0, 3]), "fit 1: need n_acq >= 1 and 0 <= first_acq < n_acq"),
    ("first_acq < 0", dict(first_acq=[-1, 0]), "fit 0: need n_acq >= 1"),
])
def test_validation_refuses_before_device_work(case, kwargs, message):
    rc, err = _call(**kwargs)
    assert rc == _lib.INR_E_INVALID, (case, rc, err)
    assert message in err, (case, err)
    assert err.startswith("inr_siren_fit_cycle_batch"), err


def test_workspace_size_is_checked():
    lib = _lib.lib()
    desc = _lib.SirenDesc(2, 64, 6, 1, 30.0, 30.0)
    wsb = lib.inr_siren_fit_workspace_bytes(ctypes.byref(desc), 3600)
    one = lambda k: _arr([_fake(k)])
    rc = lib.inr_siren_fit_cycle_batch(ctypes.byref(desc), 1, one(10), one(11), one(12), one(13), _fake(1), one(14), None,
                                       _arr([1], ctypes.c_int), _arr([0], ctypes.c_int), 3600, 1, 10, 3e-4, 0.9, 0.999, 1e-8,
                                       None, one(200), wsb - 16, None)
    assert rc == _lib.INR_E_WORKSPACE and b"workspace too small" in lib.inr_last_error()
