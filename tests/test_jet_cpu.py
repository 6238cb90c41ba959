"""CPU-only checks of the derivative entry points (csrc/jet.hip, nn_mri.py:205-221): the new C ABI names, every argument refusal
with fake pointers and no device, the workspace query, the compat exports, ``laplace``'s refusal of foreign tensors, and the pin of
tests/jet_common.py's float64 restatement to the reference's own network (tests/golden/jet_inrmodel.npz, written by
tools/make_jet_golden.py from the reference's INRmodel.Siren)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import jet_common as jc
import mri_super_resolution_amd as inr
from mri_super_resolution_amd import _lib
from mri_super_resolution_amd._build import LIB_PATH, SOURCES, build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["inr_jet_launch_count", "inr_siren_jet", "inr_siren_jet_grid", "inr_siren_jet_workspace_bytes"]


def fake(k):
    return ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)      # never dereferenced: the calls fail in validation


def test_new_header_names_signatures_and_exports():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inrhip.h")).read(), flags=re.S)
    declared = sorted(s for s in set(re.findall(r"\b(inr_[a-z0-9_]+)\s*\(", text)) if "jet" in s)
    assert declared == NEW
    assert sorted(k for k in _lib.SIGNATURES if "jet" in k) == NEW
    assert "jet.hip" in SOURCES
    build_library()
    handle = ctypes.CDLL(LIB_PATH)
    for s in NEW:
        assert hasattr(handle, s), s
    for name, value in (("INR_JET_LF_INPUT", 0), ("INR_JET_LF_LAYER", 1), ("INR_JET_LF_HEAD", 2), ("INR_JET_LF_COUNT", 3)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name
        assert getattr(_lib, name) == value


def test_launch_count_table_is_its_own():
    lib = _lib.lib()
    n = ctypes.c_int64(-1)
    assert lib.inr_launch_counts_reset() == 0
    for fam in range(_lib.INR_JET_LF_COUNT):
        assert lib.inr_jet_launch_count(fam, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.inr_jet_launch_count(_lib.INR_JET_LF_COUNT, ctypes.byref(n)) == _lib.INR_E_INVALID
    assert lib.inr_jet_launch_count(-1, ctypes.byref(n)) == _lib.INR_E_INVALID
    assert lib.inr_jet_launch_count(0, None) == _lib.INR_E_INVALID and b"inr_jet_launch_count" in lib.inr_last_error()
    # the INR_LF_* table keeps its size
    assert lib.inr_launch_count(_lib.INR_LF_COUNT, ctypes.byref(n)) == _lib.INR_E_INVALID and _lib.INR_LF_COUNT == 14


def _jet(lib, desc, *, params=1, x=2, n=100, d=3, dt=None, B=3, m=16, y=4, grad=5, lap=6, chunk=64, ws=7, ws_bytes=None):
    p = lambda k: None if k is None else fake(k)
    if ws_bytes is None:
        ws_bytes = lib.inr_siren_jet_workspace_bytes(ctypes.byref(desc), d, m if B is not None else 0, min(chunk, n), 1)
    return lib.inr_siren_jet(ctypes.byref(desc), p(params), p(x), n, d, d if dt is None else dt, p(B), m, p(y), p(grad), p(lap), chunk,
                             p(ws), ws_bytes, None)


def _jet_grid(lib, desc, *, params=1, shape=(5, 4, 5), dt=None, B=3, m=16, y=4, grad=5, lap=6, chunk=64, ws=7, ws_bytes=None,
              null_shape=False):
    p = lambda k: None if k is None else fake(k)
    d = len(shape)
    if ws_bytes is None:
        ws_bytes = lib.inr_siren_jet_workspace_bytes(ctypes.byref(desc), d, m if B is not None else 0, chunk, 1)
    return lib.inr_siren_jet_grid(ctypes.byref(desc), p(params), None if null_shape else _lib.shape_array(shape), d,
                                  d if dt is None else dt, p(B), m, p(y), p(grad), p(lap), chunk, p(ws), ws_bytes, None)


def test_every_refusal_happens_before_any_device_work():
    lib = _lib.lib()
    good = _lib.SirenDesc(32, 64, 2, 1, 30.0, 30.0)          # Fourier, m = 16
    raw = _lib.SirenDesc(3, 64, 2, 1, 30.0, 30.0)
    INV, WS, AL = _lib.INR_E_INVALID, _lib.INR_E_WORKSPACE, _lib.INR_E_ALIGN

    def refused(rc, code, word):
        assert rc == code, (rc, lib.inr_last_error())
        assert word in lib.inr_last_error(), lib.inr_last_error()

    for call in (_jet, _jet_grid):
        refused(call(lib, _lib.SirenDesc(32, 64, 2, 2, 30.0, 30.0)), INV, b"out_features must be 1")
        refused(call(lib, _lib.SirenDesc(32, 64, 0, 1, 30.0, 30.0)), INV, b"at least one hidden layer")
        for hidden in (48, 16, 1056, 0):
            refused(call(lib, _lib.SirenDesc(32, hidden, 2, 1, 30.0, 30.0)), INV, b"multiple of 32 up to 1024")
        refused(call(lib, _lib.SirenDesc(30, 64, 2, 1, 30.0, 30.0)), INV, b"must equal 2*m")
        refused(call(lib, good, B=None), INV, b"without B in_features")           # in_features 32 != d
        refused(call(lib, raw, m=16), INV, b"must equal 2*m")                      # B given, in_features 3
        for name in ("params", "y"):
            refused(call(lib, good, **{name: None}), INV, b"null pointer")
        refused(call(lib, good, dt=0), INV, b"d_tangent")
        refused(call(lib, good, dt=4), INV, b"d_tangent")
        refused(call(lib, good, chunk=0), INV, b"chunk_rows")
        refused(call(lib, good, ws=None), WS, b"workspace too small")
        need = lib.inr_siren_jet_workspace_bytes(ctypes.byref(good), 3, 16, 64, 1)
        refused(call(lib, good, ws_bytes=need - 1), WS, b"workspace too small")
    rc = lib.inr_siren_jet(None, fake(1), fake(2), 100, 3, 3, fake(3), 16, fake(4), None, None, 64, fake(7), 1 << 30, None)
    refused(rc, INV, b"descriptor is null")
    refused(_jet(lib, good, x=None), INV, b"null pointer")
    refused(_jet(lib, good, n=-1), INV, b"bad row count")
    refused(_jet(lib, good, d=5, ws_bytes=1 << 30), INV, b"coordinate axes")
    refused(_jet(lib, good, d=0, ws_bytes=1 << 30), INV, b"coordinate axes")
    refused(_jet_grid(lib, good, null_shape=True), INV, b"null pointer")
    refused(_jet_grid(lib, good, shape=(5, 0, 5)), INV, b"shape[1]")
    refused(_jet_grid(lib, good, shape=(2, 2, 2, 2, 2), ws_bytes=1 << 30), INV, b"coordinate axes")
    # pointers off a 16-byte boundary
    odd = ctypes.c_void_p(0x7000_0000_0004)
    rc = lib.inr_siren_jet(ctypes.byref(good), odd, fake(2), 100, 3, 3, fake(3), 16, fake(4), None, None, 64, fake(7), 1 << 30, None)
    refused(rc, AL, b"params must be 16-byte aligned")
    rc = lib.inr_siren_jet(ctypes.byref(good), fake(1), fake(2), 100, 3, 3, fake(3), 16, fake(4), None, None, 64, odd, 1 << 30, None)
    refused(rc, AL, b"workspace must be 16-byte aligned")
    # an empty call is valid and launches nothing
    assert _jet(lib, good, n=0, ws=None, ws_bytes=0) == 0


def test_workspace_query_grows_with_chunk_rows_and_with_the_laplacian():
    lib = _lib.lib()
    q = lambda desc, d, m, chunk, lap: lib.inr_siren_jet_workspace_bytes(ctypes.byref(desc), d, m, chunk, lap)
    desc = _lib.SirenDesc(256, 512, 3, 1, 30.0, 30.0)
    assert 0 < q(desc, 4, 128, 256, 0) < q(desc, 4, 128, 256, 1) < q(desc, 4, 128, 512, 1)
    assert q(desc, 4, 128, 1024, 1) == 2 * q(desc, 4, 128, 512, 1)
    # two buffers of J planes of chunk_rows x max(hidden, features) floats
    assert q(desc, 4, 128, 256, 1) == 2 * 6 * 256 * 512 * 4 and q(desc, 4, 128, 256, 0) == 2 * 5 * 256 * 512 * 4
    assert q(desc, 3, 128, 256, 1) == 2 * 5 * 256 * 512 * 4
    wide_in = _lib.SirenDesc(200, 64, 1, 1, 30.0, 30.0)       # 2m = 200 features: planes padded to 224 columns
    assert q(wide_in, 2, 100, 128, 1) == 2 * 4 * 128 * 224 * 4
    raw = _lib.SirenDesc(2, 64, 3, 1, 30.0, 30.0)
    assert q(raw, 2, 0, 256, 1) == 2 * 4 * 256 * 64 * 4
    # shapes the kernels do not serve, or a bad chunk: 0
    assert q(_lib.SirenDesc(2, 48, 3, 1, 30.0, 30.0), 2, 0, 256, 1) == 0
    assert q(raw, 3, 0, 256, 1) == 0 and q(raw, 2, 0, 0, 1) == 0 and q(desc, 4, 100, 256, 1) == 0
    assert lib.inr_siren_jet_workspace_bytes(None, 2, 0, 256, 1) == 0


def test_compat_nn_mri_exports_the_derivative_helpers():
    sys.path.insert(0, os.path.join(ROOT, "mri-super-resolution_amd", "compat"))
    try:
        import nn_mri
    finally:
        sys.path.pop(0)
    for name in ("gradient", "divergence", "laplace"):
        assert getattr(nn_mri, name) is getattr(inr, name)
    # the autograd forms on plain torch tensors: y = sum(x^2) -> gradient 2x; divergence of x^2 is sum 2x
    x = torch.tensor([[0.5, -1.0, 2.0]], requires_grad=True)
    assert torch.allclose(nn_mri.gradient((x * x).sum(dim=-1, keepdim=True), x), 2 * x)
    assert torch.allclose(nn_mri.divergence(x * x, x), (2 * x).sum(dim=-1, keepdim=True))


def test_laplace_refuses_tensors_that_are_not_direct_siren_outputs():
    x = torch.rand(5, 2, requires_grad=True)
    for y in ((x * x).sum(dim=-1, keepdim=True), torch.zeros(5, 1)):
        with pytest.raises(TypeError, match=r"only for direct Siren outputs.*inr\.derivatives"):
            inr.laplace(y, x)
    with pytest.raises(ValueError, match="exactly one of coords and shape"):
        inr.derivatives(inr.Siren(2, 32, 1, 1))
    with pytest.raises(ValueError, match="exactly one of coords and shape"):
        inr.derivatives(inr.Siren(2, 32, 1, 1), x, shape=(3, 3))


def _golden_case(g):
    n = sum(1 for k in g.files if k.startswith("W"))
    return {"d": 3, "m": 16, "B": torch.from_numpy(g["B"]), "x": torch.from_numpy(g["x"]),
            "weights": [(torch.from_numpy(g[f"W{l}"]), torch.from_numpy(g[f"b{l}"])) for l in range(n)]}


def test_restatement_is_pinned_to_the_reference_network(golden):
    """tests/jet_common.py's plain SIREN and its double-backward derivatives against the reference's INRmodel.Siren in float64 with
    the helpers of nn_mri.py:205-221 (tools/make_jet_golden.py), on the reference's own seeded weights: 1e-12 of each tensor's
    maximum.  The forward-mode formulas in float64 meet the same bound."""
    g = golden("jet_inrmodel.npz")
    case = _golden_case(g)
    assert case["x"].shape == (jc.ROWS, 3) and torch.equal(case["x"], jc.mgrid_rows(tuple(g["shape"])))
    assert len(case["weights"]) == 4 and case["weights"][0][0].shape == (64, 32)
    want = (g["y"], g["grad"], g["lap"])
    for name, got, ref in zip(("y", "grad", "lap"), jc.autograd_reference(case), want):
        assert jc.max_rel(got, ref) <= 1e-12, name
    for name, got, ref in zip(("y", "grad", "lap"), jc.forward_jet(case, torch.float64), want):
        assert jc.max_rel(got, ref) <= 1e-12, name
    assert np.abs(g["lap"]).max() > 1.0 and np.abs(g["grad"]).max() > 0.1      # not a degenerate case


@pytest.mark.parametrize("name", sorted(jc.CASES))
def test_forward_mode_formulas_equal_double_backward_in_float64(name):
    case = jc.make_case(**jc.CASES[name])
    dts = (case["d"],) if name != "c" else (4, 3)
    for dt in dts:
        ref = jc.autograd_reference(case, dt)
        for what, got, want in zip(("y", "grad", "lap"), jc.forward_jet(case, torch.float64, dt), ref):
            assert jc.max_rel(got, want) <= 1e-12, (what, dt)
