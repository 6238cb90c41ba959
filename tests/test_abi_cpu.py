"""CPU-only checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/inrhip.h declares, the ctypes table covers them all, host-side construction matches the
reference bit for bit, and the product path refuses to run without a HIP device."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest
import torch

import mri_super_resolution_amd as inr
from mri_super_resolution_amd import _lib
from mri_super_resolution_amd._build import LIB_PATH, build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def header_symbols():
    text = open(os.path.join(ROOT, "include", "inrhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(inr_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_and_exports_every_declared_symbol():
    build_library()
    assert os.path.exists(LIB_PATH)
    handle = ctypes.CDLL(LIB_PATH)
    syms = header_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(handle, s), f"{s} declared in inrhip.h but not exported"
    assert sorted(_lib.SIGNATURES.keys()) == syms
    assert _lib.lib().inr_version() == 1


def test_host_only_entry_points_without_gpu():
    lib = _lib.lib()
    desc = _lib.SirenDesc(256, 512, 3, 1, 30.0, 30.0)
    total = lib.inr_siren_param_count(ctypes.byref(desc))
    assert total == 256 * 512 + 512 + 3 * (512 * 512 + 512) + 512 + 4
    offs = (ctypes.c_int64 * 10)()
    assert lib.inr_siren_param_offsets(ctypes.byref(desc), offs) == 0
    assert list(offs)[:4] == [0, 131072, 131584, 131584 + 262144]
    assert all(o % 4 == 0 for o in offs)
    assert lib.inr_siren_fit_workspace_bytes(ctypes.byref(desc), 4096) > 8 * 4096 * 512 * 4
    # exact planner values (fit, forward, reconstruct), recorded before the workspace views replaced the hand-written carves:
    # a view that sizes a workspace differently from what callers have allocated so far is a bug
    small = _lib.SirenDesc(2, 64, 6, 1, 30.0, 30.0)
    planners = (lib.inr_siren_fit_workspace_bytes, lib.inr_siren_forward_workspace_bytes,
                lib.inr_siren_reconstruct_workspace_bytes)
    assert [f(ctypes.byref(desc), 4096) for f in planners] == [139270656, 28315904, 32510208]
    assert [f(ctypes.byref(small), 3600) for f in planners] == [25527040, 2074112, 2103040]
    bad = _lib.SirenDesc(0, 512, 3, 1, 30.0, 30.0)
    assert lib.inr_siren_param_count(ctypes.byref(bad)) == -1
    assert b"bad siren descriptor" in lib.inr_last_error()
    # argument validation happens before any device work
    assert lib.inr_mgrid(None, None, 2, 0, 4, None) == -1
    assert lib.inr_adam_step(None, None, None, None, 4, 1, 1e-4, 0.9, 0.999, 1e-8, None) == -1


def test_reuse_flags_are_refused_on_a_workspace_that_does_not_hold_the_image():
    """inr_siren_loss_grad_ex(flags): INR_REUSE_INPUT_IMAGE / INR_REUSE_TARGET_STATS on a workspace whose last call was not for
    the same (n, x) / (target, weight) returns INR_E_INVALID before any device work (a host-side stamp per workspace)."""
    lib = _lib.lib()
    desc = _lib.SirenDesc(256, 512, 3, 1, 30.0, 30.0)
    n = 4096
    wsb = lib.inr_siren_fit_workspace_bytes(ctypes.byref(desc), n)
    fake = lambda k: ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)      # never dereferenced: the call fails in validation
    for flags in (1, 2, 3):
        rc = lib.inr_siren_loss_grad_ex(ctypes.byref(desc), fake(1), fake(2), fake(3), fake(4), None, n, 0, fake(5), fake(6), wsb,
                                        flags, None)
        assert rc == -1 and b"REUSE" in lib.inr_last_error()
    assert lib.inr_siren_loss_grad_ex(ctypes.byref(desc), fake(1), fake(2), fake(3), fake(4), None, n, 0, fake(5), fake(6), wsb,
                                      4, None) == -1 and b"unknown flags" in lib.inr_last_error()


@pytest.mark.parametrize("flavor", ["SRDWI", "INRmodel"])
def test_siren_init_is_bit_identical_to_reference(golden, flavor):
    g = golden("siren512_step0.npz")
    torch.manual_seed(0)
    net = inr.Siren(256, 512, 3, 1, flavor=flavor)
    names = [n for n, _ in net.named_parameters()]
    assert names == [k.split("/", 2)[2] for k in g.files if k.startswith(f"{flavor}/init_sha/")]
    for n, p in net.named_parameters():
        assert sha(p.detach().numpy()) == str(g[f"{flavor}/init_sha/{n}"]), n
    keys = list(net.state_dict().keys())
    assert "net.4.weight" in keys and "final_linear.bias" in keys and "net.0.linear.weight" in keys


def test_small_siren_init_and_state_dict_roundtrip(golden):
    s = golden("siren64_2d.npz")
    torch.manual_seed(0)
    net = inr.Siren(2, 64, 6, 1)
    for n, p in net.named_parameters():
        assert np.array_equal(p.detach().numpy(), s[f"init/{n}"]), n
    m = golden("model_pt.npz")
    sd = {k.replace("__", "."): torch.from_numpy(m[k]) for k in m.files if k.startswith("net__")}
    net2 = inr.Siren(2, 64, 3, 1)
    missing, unexpected = net2.load_state_dict(sd, strict=False)
    assert unexpected == [] and set(missing) == {"final_linear.weight", "final_linear.bias"}
    assert torch.equal(net2.final_linear.weight, sd["net.4.weight"])  # alias of the shared head


def test_no_cpu_fallback():
    torch.manual_seed(0)
    net = inr.Siren(2, 16, 1, 1)
    if torch.cuda.is_available():
        pytest.skip("GPU present: the refusal path is exercised on the CPU runner")
    with pytest.raises(inr.InrDeviceError):
        net(torch.zeros(4, 2))
    with pytest.raises(inr.InrDeviceError):
        inr.get_mgrid((4, 4))
    with pytest.raises(inr.InrDeviceError):
        inr.ImageFitting_set([np.zeros((4, 4))])
    with pytest.raises(inr.InrDeviceError):
        inr.SirenFitter(net)
    with pytest.raises(inr.InrDeviceError):
        inr.input_mapping(torch.zeros(4, 2), torch.zeros(8, 2))


def test_host_helpers(golden):
    h = golden("helpers.npz")
    assert np.allclose(inr.calculate_ADC(h["bvals"], h["slicedata"]), h["adc"], rtol=1e-9, atol=1e-12)
    assert np.allclose(inr.resize_array(h["resize_in"], 9), h["resize_out"], rtol=1e-12, atol=1e-12)
    raw = [[np.full((2, 2, 2), 0.5)] * 2] + [[np.arange(2 * 2 * 2 * 3, dtype=float).reshape(2, 2, 2, 3) + b] * 2
                                             for b in (1, 2, 3)]
    combos = inr.calculate_combinations((1, 0, 1), raw)
    assert combos.shape == (4, 27)
    assert combos[0].tolist() == [0.5] * 27


def test_compat_modules_import():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "mri-super-resolution_amd", "compat"))
    try:
        import INRmodel
        import SRDWI
        import nn_mri
    finally:
        sys.path.pop(0)
    for name in ("calculate_combinations", "ImageFitting_set", "Siren", "PN", "get_mgrid", "input_mapping",
                 "calculate_ADC", "resize_array"):
        assert hasattr(SRDWI, name) and hasattr(INRmodel, name)
    for name in ("ImageFitting_set", "Siren", "get_mgrid", "SineLayer", "PN", "input_mapping"):
        assert hasattr(nn_mri, name)
    torch.manual_seed(0)
    a = INRmodel.Siren(8, 16, 1, 1)
    assert a.flavor == "INRmodel" and list(dict(a.named_parameters()))[0] == "final_linear.weight"
    assert nn_mri.Siren(2, 8, 1, 1).return_coords is True


def test_per_source_compiler_flags_name_real_sources_and_reach_the_source_hash():
    """`_build.SOURCE_FLAGS` (both GEMM translation units are compiled without packed fp32 VALU instructions) must name sources that
    exist -- a typo would silently build the default feature set -- and the compiler flags are part of what bench.py's kernel-source
    hash covers (a tracked PMC summary measured with other flags must read as stale)."""
    import hashlib
    import bench
    from mri_super_resolution_amd import _build
    assert set(_build.SOURCE_FLAGS) <= set(_build.SOURCES)
    for unit in ("gemm_f32.hip", "gemm_hp.hip"):
        assert unit in _build.SOURCE_FLAGS and "-packed-fp32-ops" in _build.SOURCE_FLAGS[unit], unit
    h = hashlib.sha256()
    csrc = os.path.join(os.path.dirname(_build.__file__), "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".inc", ".h")):
            with open(os.path.join(csrc, f), "rb") as fh:
                h.update(f.encode() + b"\0" + fh.read())
    without_flags = h.hexdigest()[:16]
    assert bench.source_hash() != without_flags and len(bench.source_hash()) == 16


def test_debug_switches_are_validated_readable_and_resettable():
    """The diagnostic switches: unknown keys and out-of-range values are refused, a value can be read back, and one call
    restores every default (what tests/conftest.py does after each test)."""
    lib = _lib.lib()
    v = ctypes.c_int(-7)
    assert lib.inr_debug_get(10, ctypes.byref(v)) == 0 and v.value == 2
    assert lib.inr_debug_set(10, 1) == 0
    assert lib.inr_debug_get(10, ctypes.byref(v)) == 0 and v.value == 1
    assert lib.inr_debug_set(10, 3) == _lib.INR_E_INVALID and b"takes 0 .. 2" in lib.inr_last_error()
    assert lib.inr_debug_set(4, 1) == _lib.INR_E_INVALID and b"unknown key" in lib.inr_last_error()
    assert lib.inr_debug_get(99, ctypes.byref(v)) == _lib.INR_E_INVALID
    for key, val in ((0, 1), (3, 0), (7, 0), (12, 0), (14, 5), (16, 0), (17, 1), (18, 0), (21, 8), (22, 128), (23, 64), (24, 0), (25, 0)):
        assert lib.inr_debug_set(key, val) == 0, key
    assert lib.inr_debug_set(24, 3) == _lib.INR_E_INVALID and lib.inr_debug_set(23, 5000) == _lib.INR_E_INVALID
    # key 32: the test-only cap on the persistent grids, 0 (no cap) .. 2^20
    for val in (1, 7, 1 << 20, 0, 3):
        assert lib.inr_debug_set(32, val) == 0, val
        assert lib.inr_debug_get(32, ctypes.byref(v)) == 0 and v.value == val
    for bad in (-1, (1 << 20) + 1):
        assert lib.inr_debug_set(32, bad) == _lib.INR_E_INVALID and b"takes 0 .. 1048576" in lib.inr_last_error(), bad
    assert lib.inr_debug_get(32, ctypes.byref(v)) == 0 and v.value == 3
    assert lib.inr_debug_reset() == 0
    for key, default in ((0, 0), (1, 1), (2, 1), (3, 1), (5, 1), (6, 1), (7, 1), (10, 2), (11, 0), (12, 1), (13, 0), (14, 2),
                         (15, 42), (16, 1), (17, 0), (18, 1), (19, 0), (20, 1), (21, 16), (22, 256), (23, 0), (24, 2), (25, 1), (26, 600000), (27, 0), (28, 1024), (29, 192), (30, 1), (31, 768),
                         (32, 0)):
        assert lib.inr_debug_get(key, ctypes.byref(v)) == 0 and v.value == default, (key, v.value)
    n = ctypes.c_int64(-1)
    assert lib.inr_launch_counts_reset() == 0
    for fam in range(_lib.INR_LF_COUNT):
        assert lib.inr_launch_count(fam, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.inr_launch_count(_lib.INR_LF_COUNT, ctypes.byref(n)) == _lib.INR_E_INVALID


def test_launch_counters_share_one_reset_and_keep_their_id_ranges():
    """Every launch family reads 0 through its own entry point after one reset; the accepted ids are exactly 0..13 and 32..35
    (inr_launch_count), 0..3 (inr_pia_launch_count) and 0..2 (inr_jet_launch_count) -- the table's internal PIA / jet bases,
    which start where the ERD ids end, are not reachable -- and a null `count` is refused everywhere."""
    lib = _lib.lib()
    n = ctypes.c_int64(-1)
    assert lib.inr_launch_counts_reset() == 0
    for entry, ids in ((lib.inr_launch_count, list(range(14)) + [32, 33, 34, 35]), (lib.inr_pia_launch_count, range(4)),
                       (lib.inr_jet_launch_count, range(3))):
        for fam in ids:
            n.value = -1
            assert entry(fam, ctypes.byref(n)) == 0 and n.value == 0, fam
            assert entry(fam, None) == _lib.INR_E_INVALID, fam
    pia_base, jet_base = 36, 36 + _lib.INR_PIA_LF_COUNT
    for bad in [-1, 14, 31, 36] + list(range(pia_base, jet_base + _lib.INR_JET_LF_COUNT + 1)):
        assert lib.inr_launch_count(bad, ctypes.byref(n)) == _lib.INR_E_INVALID, bad
    assert lib.inr_pia_launch_count(4, ctypes.byref(n)) == _lib.INR_E_INVALID
    assert lib.inr_pia_launch_count(-1, ctypes.byref(n)) == _lib.INR_E_INVALID
    assert lib.inr_jet_launch_count(3, ctypes.byref(n)) == _lib.INR_E_INVALID
