"""No device: the float64 restatement of Gibbs-ringing removal by local sub-voxel shifts (tests/degibbs_common.py) -- that its two
paths choose the same shifts, its symmetries, that the split sums to the image, that it removes ringing from a truncated phantom --, the
new symbols, and the refusals of inr_degibbs_lines / inr_degibbs2d and of the Python layer, all before any device work."""
import ctypes
import re

import numpy as np
import pytest
import torch

from tests import degibbs_common as G
from mri_super_resolution_amd import _lib, denoise, ops

PHANTOM_RATIO_BOUND = 0.5      # the prototype of the definition measured 0.09 and 0.23; the bound leaves twice the worse one
NEW_SYMBOLS = ("inr_degibbs_lines", "inr_degibbs_lines_f32", "inr_degibbs2d", "inr_degibbs2d_f32", "inr_degibbs_lines_workspace_doubles",
               "inr_degibbs2d_workspace_doubles")


def _fake(k):
    return ctypes.c_void_p(0x7000_0000_0000 + (1 << 32) * k)      # never dereferenced: every call here fails in validation


@pytest.mark.parametrize("name", G.CASE_IDS)
def test_the_two_paths_choose_the_same_shifts(name):
    for ref in (G.reference_lines, G.reference2d):
        (of, cf, mf), (od, cd, md) = ref(name, "fft"), ref(name, "dense")
        decided = (mf >= G.MARGIN) & (md >= G.MARGIN)
        if ref is G.reference2d:                              # both passes of a pixel must be decided
            decided = np.broadcast_to(decided.all(axis=0), cf.shape)
        top = float(np.abs(G.case(name)).max())
        d_ref = float(np.abs(of - od).max())
        print(f"{name} {ref.__name__}: undecided {1 - decided.mean():.2e}, smallest margin {min(mf.min(), md.min()):.2e}, d_ref {d_ref:.2e}, "
              f"max|x| {top:.3f}")
        assert 1 - decided.mean() <= G.MAX_EXCLUDED
        assert np.array_equal(cf[decided], cd[decided])
        assert d_ref <= 64 * 4 * G.EPS * top                  # two orders of the same sums of some n terms of size max|x|


def test_flipping_a_line_mirrors_the_result():
    x = G.case("ragged-even").reshape(-1, 20)
    out, choice, margin = G.lines(x)
    fout, fchoice, fmargin = G.lines(x[:, ::-1])
    decided = (margin >= G.MARGIN) & (fmargin[:, ::-1] >= G.MARGIN)
    assert decided.mean() >= 1 - G.MAX_EXCLUDED
    assert np.array_equal(fchoice[:, ::-1][decided], G.flip_choice(choice, G.NSHIFTS)[decided])
    assert np.abs(fout[:, ::-1] - out)[decided].max() <= 32 * 4 * G.EPS * np.abs(x).max()


@pytest.mark.parametrize("path", ("fft", "dense"))
def test_the_split_sums_to_the_image(path):
    for name in ("ragged-even", "odd"):
        I = G.case(name)
        I1, I0 = G.split(I, path)
        assert np.abs((I0 + I1) - I).max() <= 2 * G.EPS * np.abs(I).max()     # I0 = fl(I - I1): one rounding each way
    assert G.g1(24, 20)[12, 10] == 0.5 and G.g1(24, 20)[0, 0] == 0.5
    assert G.g1(24, 20)[12, 0] == 0.0 and G.g1(24, 20)[0, 10] == 1.0


@pytest.mark.parametrize("path", ("fft", "dense"))
def test_constant_and_zero_lines_come_back_bit_for_bit_with_choice_zero(path):
    x = np.stack([np.full(21, 0.7), np.zeros(21), np.full(21, -3.25e5)])
    out, choice, _ = G.lines(x, path=path)
    assert out.tobytes() == x.tobytes() and not choice.any()


@pytest.mark.parametrize("n", (48, 32))
def test_the_restatement_removes_the_ringing_of_a_truncated_two_box_phantom(n):
    truth, rung, interior = G.two_box(n)
    out, _, _ = G.degibbs2d(rung)
    ratio = G.error_ratio(truth, rung, out, interior)
    print(f"two-box {n} x {n}: mean |error| over {int(interior.sum())} interior pixels {np.abs(rung - truth)[interior].mean():.3e} -> "
          f"ratio {ratio:.3f}")
    assert ratio <= PHANTOM_RATIO_BOUND


def test_the_new_symbols_are_declared_exported_and_bound():
    from tests.test_abi_cpu import header_symbols
    from mri_super_resolution_amd._build import LIB_PATH
    handle = ctypes.CDLL(LIB_PATH)
    declared = header_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(handle, s), s
    assert (_lib.INR_DEGIBBS_MAX_LINE, _lib.INR_DEGIBBS_MAX_SHIFTS, _lib.INR_DEGIBBS_MAX_WINDOW) == (1024, 64, 8)
    assert _lib.lib().inr_version() == 1


GOOD = dict(out=1, choice=2, inp=3, count=4, a=24, b=20, nshifts=20, w_min=1, w_max=3)
REFUSALS = (
    ("null pointer", dict(out=None)),
    ("null pointer", dict(inp=None)),
    ("bad sizes", dict(count=-1)),
    ("nshifts must be 1 .. 64 \\(got 0\\)", dict(nshifts=0)),
    ("nshifts must be 1 .. 64 \\(got 65\\)", dict(nshifts=65)),
    ("1 <= w_min <= w_max <= 8 \\(got 0, 3\\)", dict(w_min=0)),
    ("1 <= w_min <= w_max <= 8 \\(got 4, 3\\)", dict(w_min=4)),
    ("1 <= w_min <= w_max <= 8 \\(got 1, 9\\)", dict(w_max=9)),
    ("2 w_max \\+ 3 = 9 .. 1024 samples \\(got 8\\)", dict(b=8)),
    ("2 w_max \\+ 3 = 9 .. 1024 samples \\(got 1025\\)", dict(b=1025)),
    ("2 w_max \\+ 3 = 19 .. 1024 samples \\(got 18\\)", dict(b=18, w_max=8)),
    ("out must not overlap in", dict(out=3)),
)


@pytest.mark.parametrize("entry", ("inr_degibbs_lines", "inr_degibbs_lines_f32", "inr_degibbs2d", "inr_degibbs2d_f32"))
def test_every_refusal_comes_with_its_code_and_message_before_any_device_work(entry):
    lib = _lib.lib()
    fn = getattr(lib, entry)
    two_d = "2d" in entry
    ptr = lambda v: None if v is None else _fake(v)

    def sizes_of(a):
        return (a["count"], a["a"], a["b"]) if two_d else (a["count"], a["b"])

    def plan_of(a):
        return (lib.inr_degibbs2d_workspace_doubles if two_d else lib.inr_degibbs_lines_workspace_doubles)(*sizes_of(a), 20)

    def call(a, ws_doubles):
        """Only ever with arguments that are refused, or with an empty batch: the pointers are fakes, and on a machine with a device a
        call that passed validation would launch on them."""
        return fn(ptr(a["out"]), ptr(a["choice"]), ptr(a["inp"]), *sizes_of(a), a["nshifts"], a["w_min"], a["w_max"], _fake(9), ws_doubles, None)

    for text, change in REFUSALS + ((("2 w_max \\+ 3 = 9 .. 1024 samples \\(got 1030\\)", dict(a=1030)),) if two_d else ()):
        a = dict(GOOD)
        a.update(change)
        rc = call(a, plan_of(a))
        msg = lib.inr_last_error().decode()
        assert rc == _lib.INR_E_INVALID, (change, rc, msg)
        assert re.search(text, msg) and entry in msg, (change, msg)
    # one double less than the plan: refused by name, before any launch (this machine may have no device)
    plan = plan_of(GOOD)
    assert plan > 0
    rc = call(dict(GOOD), plan - 1)
    assert rc == _lib.INR_E_WORKSPACE and "workspace too small" in lib.inr_last_error().decode() and entry in lib.inr_last_error().decode()
    assert fn(_fake(1), None, _fake(3), *((4, 24, 20) if two_d else (4, 20)), 20, 1, 3, None, 0, None) == _lib.INR_E_WORKSPACE
    # an empty batch succeeds and launches nothing
    a = dict(GOOD, count=0)
    assert call(a, plan_of(a)) == 0


def test_the_planners_return_zero_for_what_every_call_refuses_and_do_not_depend_on_nshifts():
    lib = _lib.lib()
    assert lib.inr_degibbs_lines_workspace_doubles(10, 64, 20) == lib.inr_degibbs_lines_workspace_doubles(10, 64, 1) == 128 * 64
    assert lib.inr_degibbs2d_workspace_doubles(3, 24, 20, 20) == lib.inr_degibbs2d_workspace_doubles(3, 24, 20, 64) > 6 * 3 * 24 * 20
    for args in ((-1, 64, 20), (10, 4, 20), (10, 1025, 20), (10, 64, 0), (10, 64, 65)):
        assert lib.inr_degibbs_lines_workspace_doubles(*args) == 0, args
    for args in ((-1, 24, 20, 20), (3, 4, 20, 20), (3, 24, 1025, 20), (3, 24, 20, 0), (3, 24, 20, 65)):
        assert lib.inr_degibbs2d_workspace_doubles(*args) == 0, args
    # a batch beyond the chunk is planned at the chunk: the workspace stops growing
    per = _lib.INR_DEGIBBS_CHUNK_DOUBLES // (9 * 9)
    assert lib.inr_degibbs2d_workspace_doubles(per, 9, 9, 20) == lib.inr_degibbs2d_workspace_doubles(4 * per, 9, 9, 20)
    assert lib.inr_degibbs2d_workspace_doubles(per - 1, 9, 9, 20) < lib.inr_degibbs2d_workspace_doubles(per, 9, 9, 20)


def test_python_refusals_come_by_name_and_before_the_device():
    x = np.zeros((3, 24, 20))
    for text, kw in (("lines of 2 w_max \\+ 3 = 9 .. 1024 samples \\(got 8\\)", dict(data=np.zeros((3, 24, 8)))),
                     ("lines of 2 w_max \\+ 3 = 9 .. 1024 samples \\(got 1025\\)", dict(data=np.zeros((2, 1025, 9)))),
                     ("nshifts must be 1 .. 64 \\(got 0\\)", dict(nshifts=0)),
                     ("nshifts must be 1 .. 64 \\(got 65\\)", dict(nshifts=65)),
                     ("window must be \\(w_min, w_max\\)", dict(window=(3, 1))),
                     ("window must be \\(w_min, w_max\\)", dict(window=(1, 2, 3))),
                     ("window must be \\(w_min, w_max\\)", dict(window=(0, 3))),
                     ("two different axes", dict(axes=(1, -2))),
                     ("out of range", dict(axes=(0, 3))),
                     ("at least 2 axes", dict(data=np.zeros(24)))):
        kw = dict(kw)
        data = kw.pop("data", x)
        with pytest.raises(ValueError, match=text):
            denoise.degibbs(data, **kw)
    for text, kw in (("\\(got 8\\)", dict(x=np.zeros((3, 8)))), ("nshifts", dict(nshifts=65)), ("window", dict(window=(2, 9))),
                     ("out of range", dict(axis=2))):
        kw = dict(kw)
        data = kw.pop("x", np.zeros((3, 20)))
        with pytest.raises(ValueError, match=text):
            denoise.degibbs_lines(data, **kw)
    for fn in (denoise.degibbs, denoise.degibbs_lines):
        with pytest.raises(TypeError, match="ndarray or a device tensor"):
            fn([[1.0]])
        with pytest.raises(TypeError, match="float16"):
            fn(np.zeros((24, 20), np.float16))
        with pytest.raises(TypeError, match="float32 or float64"):
            fn(torch.zeros(24, 20, dtype=torch.float16))


def test_there_is_no_cpu_fallback():
    for fn in (denoise.degibbs, denoise.degibbs_lines):
        with pytest.raises(ops.InrDeviceError):
            fn(torch.zeros(24, 20, dtype=torch.float64))
    with pytest.raises(ops.InrDeviceError):
        ops.degibbs2d(torch.zeros(1, 24, 20, dtype=torch.float64))
    with pytest.raises(ops.InrDeviceError):
        ops.degibbs_lines(torch.zeros(24, 20, dtype=torch.float64))
    if not torch.cuda.is_available():
        with pytest.raises(ops.InrDeviceError):
            denoise.degibbs(np.zeros((24, 20)))
