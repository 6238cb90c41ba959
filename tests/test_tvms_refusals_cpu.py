"""CPU: the surface of the multi-stack solver (header, exports, ctypes table, workspace plan) and every refusal of csrc/tvms.hip
before device work -- by status through the C ABI, with fake pointers that are never dereferenced -- and of the Python entry points,
by name."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mri_super_resolution_amd import _lib, baselines, drivers, ops
from mri_super_resolution_amd._build import LIB_PATH, SOURCE_FLAGS, SOURCES, build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("inr_tvms_apply", "inr_tvms_adjoint", "inr_tvms_workspace_doubles", "inr_tvms_solve", "inr_tvms_solve_f32")
# two stacks on 7 x 9 x 10: overlapping along the slices (L = 4 at spacing 2, offset -1), gapped along the rows
GEO = (2, 1, 1, 4, 1, 1, -1, 0, 0, 4, 9, 10,
       1, 3, 1, 1, 2, 1, 0, 1, 0, 7, 3, 10)
TAPS = (.2, .3, .3, .2, 1, 1, 1, .5, .5, 1)
M_DATA = 4 * 9 * 10 + 7 * 3 * 10


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _doubles(*v):
    return (ctypes.c_double * len(v))(*v)


def _geo(**change):
    """GEO with entries of stack 0 replaced: f0 .. n2 by name."""
    names = ("f0", "f1", "f2", "L0", "L1", "L2", "o0", "o1", "o2", "n0", "n1", "n2")
    g = list(GEO)
    for name, value in change.items():
        g[names.index(name)] = value
    return _ints(*g)


def test_header_library_and_ctypes_table_carry_the_symbols():
    text = open(os.path.join(ROOT, "include", "inrhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(inr_[a-z0-9_]+)\s*\(", code))
    build_library()
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(handle, name) and name in _lib.SIGNATURES, name
    assert sorted(k for k in _lib.SIGNATURES if k.startswith("inr_tvms_")) == sorted(NEW)
    assert "tvms.hip" in SOURCES and "-ffp-contract=off" in SOURCE_FLAGS["tvms.hip"]
    assert int(re.search(r"#define INR_TVMS_MAX_STACKS (\d+)", text).group(1)) == _lib.INR_TVMS_MAX_STACKS == ops.TVMS_MAX_STACKS == 8
    assert int(re.search(r"#define INR_TVMS_MAX_TAPS (\d+)", text).group(1)) == _lib.INR_TVMS_MAX_TAPS == ops.TVMS_MAX_TAPS == 16
    for name in ("stack_geometry", "profile_taps", "stack_apply", "stack_adjoint", "tv_superres_stacks"):
        assert callable(getattr(baselines, name))
    for name in ("stack_apply", "stack_adjoint", "tvms_solve", "tvms_workspace_doubles"):
        assert callable(getattr(ops, name))
    assert callable(drivers.multi_stack_study)
    unit = open(os.path.join(ROOT, "mri-super-resolution_amd", "csrc", "tvms.hip")).read()
    assert "a field is either read across threads or written by its owner alone" in unit and "STREAM ORDER IS THE BARRIER" in unit
    assert "atomic" not in re.sub(r"//.*", "", unit) and "hipLaunchCooperativeKernel" not in unit


def _plan(n, D, H, W, M):
    """x | xbar | p0 | p1 | p2, q, three partials per part (1,024 elements); every field rounded up to 16 bytes."""
    even = lambda doubles: doubles + doubles % 2
    parts = -(-(D * H * W + M) // 1024)
    return even(n * 5 * D * H * W) + even(n * M) + 3 * even(n * parts)


def test_workspace_plan():
    plan = _lib.lib().inr_tvms_workspace_doubles
    err = _lib.lib().inr_last_error
    assert plan(1, 7, 9, 10, 2, _ints(*GEO)) == _plan(1, 7, 9, 10, M_DATA)
    assert plan(3, 7, 9, 10, 2, _ints(*GEO)) == _plan(3, 7, 9, 10, M_DATA)
    assert plan(40, 7, 9, 10, 1, _ints(*GEO)) == _plan(40, 7, 9, 10, 360)
    assert plan(0, 7, 9, 10, 2, _ints(*GEO)) == plan(1, 7, 9, 10, 2, _ints(*GEO)) > 0
    stacks = [((2, 1, 1), ([.2, .3, .3, .2], [1.0], [1.0]), (-1, 0, 0), (4, 9, 10)), ((1, 3, 1), ([1.0], [.5, .5], [1.0]), (0, 1, 0), (7, 3, 10))]
    assert ops.tvms_workspace_doubles(3, 7, 9, 10, stacks) == _plan(3, 7, 9, 10, M_DATA)
    for args, text in (((-1, 7, 9, 10, 2, _ints(*GEO)), b"bad sizes (n_volumes"), ((1, 7, 9, 10, 0, _ints(*GEO)), b"stacks per volume are 1 .. 8"),
                       ((1, 7, 9, 10, 9, _ints(*(GEO * 5))), b"stacks per volume are 1 .. 8"), ((1, 7, 9, 10, 2, None), b"null pointer (geometry)"),
                       ((1, 0, 9, 10, 2, _ints(*GEO)), b"bad sizes (HR volumes"), ((1, 7, 9, 1025, 2, _ints(*GEO)), b"bad sizes (HR volumes"),
                       ((1, 7, 9, 10, 2, _geo(f0=9)), b"spacings are 1 .. 8"), ((1, 7, 9, 10, 2, _geo(L1=17)), b"tap counts are 1 .. 16"),
                       ((1, 7, 9, 10, 2, _geo(o2=(1 << 20) + 1)), b"offsets are within"), ((1, 7, 9, 10, 2, _geo(n0=2049)), b"LR extents are 1 .. 2048")):
        assert plan(*args) == 0 and b"inr_tvms_workspace_doubles" in err() and text in err(), (args[:5], err())


def test_every_refusal_comes_before_device_work():
    lib = _lib.lib()
    fake = lambda k: ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)      # never dereferenced: every call fails in validation
    err = lib.inr_last_error
    nan, inf = float("nan"), float("inf")
    geo, taps, ones = _ints(*GEO), _doubles(*TAPS), _doubles(1, 1, 1)
    need = lib.inr_tvms_workspace_doubles(2, 7, 9, 10, 2, geo)
    INV, WS, AL = _lib.INR_E_INVALID, _lib.INR_E_WORKSPACE, _lib.INR_E_ALIGN
    names = ("out", "energy", "change", "valid", "y", "weight", "x0", "n", "D", "H", "W", "S", "geo", "taps", "g", "lam", "alpha", "n_iter",
             "ws", "doubles", "stream")
    for call in (lib.inr_tvms_solve, lib.inr_tvms_solve_f32):
        who = call.__name__.encode()
        ok = [fake(0), fake(1), fake(2), fake(3), fake(4), None, None, 2, 7, 9, 10, 2, geo, taps, ones, 0.05, 0.02, 10, fake(6), need, None]

        def bad(code, text, **change):
            args = [change.get(name, value) for name, value in zip(names, ok)]
            assert call(*args) == code, (change, err())
            assert text in err() and who in err(), (change, err())

        bad(INV, b"null pointer", out=None)
        bad(INV, b"null pointer", y=None)
        bad(INV, b"null pointer (geometry)", geo=None)
        bad(INV, b"null pointer (taps)", taps=None)
        bad(INV, b"null pointer (grad_weights)", g=None)
        bad(INV, b"bad sizes (n_volumes", n=-1)
        bad(INV, b"stacks per volume are 1 .. 8", S=0)
        bad(INV, b"stacks per volume are 1 .. 8", S=9)
        for name, text, values in (("f0", b"spacings are 1 .. 8", (0, 9)), ("f2", b"spacings are 1 .. 8", (-1, 9)),
                                   ("L0", b"tap counts are 1 .. 16", (0, 17)), ("L1", b"tap counts are 1 .. 16", (0, 17)),
                                   ("o0", b"offsets are within", (-(1 << 20) - 1, (1 << 20) + 1)), ("o2", b"offsets are within", (1 << 30,)),
                                   ("n0", b"LR extents are 1 .. 2048", (0, 2049)), ("n2", b"LR extents are 1 .. 2048", (-3, 1 << 20))):
            for value in values:
                bad(INV, text, geo=_geo(**{name: value}))
        bad(INV, b"bad sizes (HR volumes", D=0)
        bad(INV, b"bad sizes (HR volumes", H=1025)
        bad(INV, b"bad sizes (HR volumes", W=-1)
        bad(INV, b"n_iter must be 0 .. 100000", n_iter=-1)
        bad(INV, b"n_iter must be 0 .. 100000", n_iter=100001)
        for name, text in (("lam", b"lambda must be finite and >= 0"), ("alpha", b"alpha must be finite and >= 0")):
            for value in (-1e-3, nan, inf):
                bad(INV, text, **{name: value})
        for g in ((-1, 1, 1), (1, nan, 1), (1, 1, inf)):
            bad(INV, b"gradient weights must be finite and >= 0", g=_doubles(*g))
        bad(INV, b"taps must be finite", taps=_doubles(.2, nan, .3, .2, 1, 1, 1, .5, .5, 1))
        bad(INV, b"taps must be finite", taps=_doubles(.2, .3, .3, .2, 1, 1, 1, .5, inf, 1))
        bad(INV, b"must sum to 1", taps=_doubles(.2, .3, .3, .3, 1, 1, 1, .5, .5, 1))
        bad(INV, b"must sum to 1", taps=_doubles(.2, .3, .3, .2, 1, 1, 1, .5, .5, 0))
        bad(WS, b"workspace too small", doubles=need - 1)
        bad(WS, b"workspace too small", ws=None)
        bad(AL, b"16-byte aligned", ws=ctypes.c_void_p(0x7000_0000_0008))
        # n_volumes = 0 succeeds and launches nothing; energy, change and valid_fraction are optional
        zero = list(ok)
        zero[7] = 0
        assert call(*zero) == 0
        zero[1] = zero[2] = zero[3] = None
        assert call(*zero) == 0
    # out, valid, in, n, D, H, W, S, geometry, taps, stream  /  out, in, n, D, H, W, S, geometry, taps, stream
    for call, ok in ((lib.inr_tvms_apply, [fake(0), None, fake(1), 2, 7, 9, 10, 2, geo, taps, None]),
                     (lib.inr_tvms_adjoint, [fake(0), fake(1), 2, 7, 9, 10, 2, geo, taps, None])):
        who = call.__name__.encode()
        base = len(ok) - 8                                                # the index of n
        sub = lambda i, v: ok[:i] + [v] + ok[i + 1:]
        for args, text in ((sub(0, None), b"null pointer"), (sub(base - 1, None), b"null pointer"), (sub(base + 5, None), b"null pointer (geometry)"),
                           (sub(base + 6, None), b"null pointer (taps)"), (sub(base, -1), b"bad sizes"), (sub(base + 4, 0), b"stacks per volume"),
                           (sub(base + 4, 9), b"stacks per volume"), (sub(base + 1, 2048), b"bad sizes (HR volumes"),
                           (sub(base + 5, _geo(f1=0)), b"spacings"), (sub(base + 5, _geo(L2=40)), b"tap counts"),
                           (sub(base + 5, _geo(o1=-(1 << 21))), b"offsets"), (sub(base + 5, _geo(n1=0)), b"LR extents"),
                           (sub(base + 6, _doubles(*([1.0] * 10))), b"sum to 1"), (sub(base + 6, _doubles(*([nan] * 10))), b"finite")):
            assert call(*args) == INV and text in err() and who in err(), (args, err())
        assert call(*sub(base, 0)) == 0


def test_python_entry_points_refuse_by_name():
    B = baselines
    geo = B.stack_geometry((2, 1, 1))
    assert geo.factors == (2, 1, 1) and geo.kernels == ((0.5, 0.5), (1.0,), (1.0,)) and geo.offsets == (0, 0, 0)
    assert isinstance(geo, tuple) and B.stack_geometry((2, 1, 1), "decimate", (1, 0, -3)) == ((2, 1, 1), ((1.0, 0.0), (1.0,), (1.0,)), (1, 0, -3))
    with pytest.raises(AttributeError):
        geo.factors = (1, 1, 1)
    long = B.stack_geometry((2, 1, 1), (np.full(16, 1 / 16), [1.0], [1.0]))
    assert len(long.kernels[0]) == 16 and B.default_lr_shape(long, (40, 5, 6)) == (13, 5, 6)
    for args, text in ((((2, 1),), "factors are \\(f0, f1, f2\\)"), (((2, 1, 9),), "factors are 1 .. 8"), (((2, 1, 1), "median"), "kernel must be"),
                       (((2, 1, 1), ([.5, .5], [1.0])), "triple of 1-D arrays"), (((2, 1, 1), (np.full(17, 1 / 17), [1.0], [1.0])), "1 .. 16 taps"),
                       (((2, 1, 1), ([.5, .6], [1.0], [1.0])), "k0 must be finite and sum to 1"),
                       (((2, 1, 1), ([.5, .5], [np.nan], [1.0])), "k1 must be finite and sum to 1"),
                       (((2, 1, 1), "mean", (0, 0)), "offsets are three whole numbers"), (((2, 1, 1), "mean", (0.5, 0, 0)), "offsets are three whole"),
                       (((2, 1, 1), "mean", (0, 0, (1 << 20) + 1)), "offsets are within")):
        with pytest.raises(ValueError, match=text):
            B.stack_geometry(*args)
    np.testing.assert_array_equal(B.profile_taps(2, 2, "gaussian", 1.0), B.slice_profile(2, "gaussian", 1.0))
    k = B.profile_taps(4, 2, "gaussian", 1.0)
    assert k.shape == (4,) and abs(k.sum() - 1) < 1e-15 and np.array_equal(k, k[::-1]) and k[1] > k[0]
    assert np.array_equal(B.profile_taps(3, 2, "mean"), np.full(3, 1 / 3))
    for args, text in (((0, 2), "length is an integer 1 .. 16"), ((17, 2), "length is an integer"), ((4, 9), "spacing is an integer 1 .. 8"),
                       ((4, 2, "gaussian"), "needs a finite fwhm"), ((4, 2, "mean", 1.0), "fwhm belongs to"), ((4, 2, "box"), "kind must be"),
                       ((4, 2, "gaussian", 1e-3), "too narrow")):
        with pytest.raises(ValueError, match=text):
            B.profile_taps(*args)
    x, y = np.ones((6, 5, 4)), np.ones((3, 5, 4))
    with pytest.raises(TypeError, match="stack_apply: geometry is a record"):
        B.stack_apply(x, ((2, 1, 1), "mean", (0, 0, 0)))
    with pytest.raises(ValueError, match="stack_apply needs at least 3-D"):
        B.stack_apply(np.ones((5, 4)), geo)
    with pytest.raises(ValueError, match="stack_apply: LR extents are 1 .. 2048"):
        B.stack_apply(x, geo, (3, 5, 2049))
    with pytest.raises(ValueError, match="stack_apply: an LR shape is"):
        B.stack_apply(x, geo, (3, 5))
    with pytest.raises(ValueError, match="stack_apply: HR volumes of 1 .. 1024"):
        B.stack_apply(np.ones((1, 1, 1025)), geo)
    with pytest.raises(TypeError, match="stack_apply takes an ndarray or a device tensor"):
        B.stack_apply([[1.0]], geo)
    with pytest.raises(ops.InrDeviceError, match="no CPU fallback"):
        B.stack_apply(torch.ones(6, 5, 4), geo)
    with pytest.raises(ValueError, match="stack_adjoint: hr_shape is"):
        B.stack_adjoint(y, geo, (6, 5))
    with pytest.raises(TypeError, match="stack_adjoint: geometry is a record"):
        B.stack_adjoint(y, None, (6, 5, 4))
    who = "tv_superres_stacks"
    for kwargs, kind, text in (({"lam": -1.0}, ValueError, "lam must be finite"), ({"lam": np.nan}, ValueError, "lam must be finite"),
                               ({"huber": np.inf}, ValueError, "huber must be finite"), ({"n_iter": 1.5}, ValueError, "n_iter must be an integer"),
                               ({"n_iter": 100001}, ValueError, "n_iter must be an integer"), ({"grad_weights": (1, 1)}, ValueError, "grad_weights are"),
                               ({"grad_weights": (1, -1, 1)}, ValueError, "grad_weights are"), ({"weight": y}, TypeError, "weight is a list"),
                               ({"weight": [np.ones((3, 5, 3))]}, ValueError, "weight 0 must have shape"),
                               ({"weight": [-y]}, ValueError, "weight must be >= 0"), ({"weight": [torch.ones(3, 5, 4)]}, TypeError, "weight must be given like stacks"),
                               ({"x0": np.ones((6, 5, 5))}, ValueError, "x0 must have shape"), ({"x0": torch.ones(6, 5, 4)}, TypeError, "x0 must be given like stacks")):
        with pytest.raises(kind, match=f"{who}: {text}"):
            B.tv_superres_stacks([y], [geo], (6, 5, 4), **kwargs)
    with pytest.raises(TypeError, match=f"{who}: stacks is a list"):
        B.tv_superres_stacks(y, [geo], (6, 5, 4))
    with pytest.raises(ValueError, match=f"{who}: 2 stacks for 1 geometries"):
        B.tv_superres_stacks([y, y], [geo], (6, 5, 4))
    with pytest.raises(ValueError, match=f"{who}: stacks per volume are 1 .. 8"):
        B.tv_superres_stacks([y] * 9, [geo] * 9, (6, 5, 4))
    with pytest.raises(TypeError, match=f"{who}: every geometry is a record"):
        B.tv_superres_stacks([y], [((2, 1, 1),)], (6, 5, 4))
    with pytest.raises(ValueError, match=f"{who}: hr_shape is"):
        B.tv_superres_stacks([y], [geo], (6, 5))
    with pytest.raises(ValueError, match=f"{who}: stack 1 must have the leading axes"):
        B.tv_superres_stacks([y, np.ones((2, 3, 5, 4))], [geo, geo], (6, 5, 4))
    with pytest.raises(ops.InrDeviceError, match="no CPU fallback"):
        B.tv_superres_stacks([torch.ones(3, 5, 4)], [geo], (6, 5, 4))


def test_the_study_refuses_by_name():
    vol = np.ones((8, 6, 6))
    for kwargs, text in (({"design": "diagonal"}, "design must be one of"), ({"factor": 1}, "factor is the slice thickness"),
                         ({"factor": 9}, "factor is the slice thickness"), ({"noise": -1.0}, "noise must be finite"),
                         ({"tv_lambda": -1.0}, "tv_lambda must be finite"), ({"tv_huber": np.nan}, "tv_huber must be finite"),
                         ({"tv_iters": 0}, "tv_iters must be 1 .. 100,000"), ({"tv_gz": -0.5}, "tv_gz must be finite"),
                         ({"fwhm": 0.0}, "fwhm must be finite and > 0"), ({"design": "shifted", "fwhm": 1.0}, "fwhm belongs to design='overlap'")):
        args = {"design": "overlap" if "fwhm" in kwargs and "design" not in kwargs else "shifted", **kwargs}
        with pytest.raises(ValueError, match=f"multi_stack_study: {text}"):
            drivers.multi_stack_study(vol, **args)
    with pytest.raises(ValueError, match="multi_stack_study: the volume is \\[Z, X, Y\\]"):
        drivers.multi_stack_study(np.ones((6, 6)), "shifted")
    with pytest.raises(ValueError, match="multi_stack_study: 3 slices"):
        drivers.multi_stack_study(np.ones((3, 6, 6)), "shifted", factor=2)
