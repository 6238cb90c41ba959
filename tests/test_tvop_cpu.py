"""CPU: the float64 restatement of the operator solver (tests/tvop_common.py) against its own checks -- the adjoint identity, the step
bound against the spectral norm, an independent minimum, the block solver's restatement, the same iteration in longdouble --, the
operator makers against it, the surface of csrc/tvop.hip (header, exports, ctypes table, workspace plan) and every refusal before
device work, by status through the C ABI with fake pointers that are never dereferenced and by name through the Python entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mri_super_resolution_amd import _lib, baselines, ops
from mri_super_resolution_amd._build import LIB_PATH, SOURCE_FLAGS, SOURCES, build_library
from tests import fourier_common as F
from tests import tvop_common as C
from tests import tvsr_common as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("inr_tvop_apply", "inr_tvop_adjoint", "inr_tvop_workspace_doubles", "inr_tvop_solve2d", "inr_tvop_solve2d_f32")


def _pairs(shape, lr_shape):
    return {"gaussian": C.gaussian_pair(shape, lr_shape), "fourier": C.fourier_pair(shape, lr_shape, "center", "mirror"),
            "fourier_periodic": C.fourier_pair(shape, lr_shape, "sample", "periodic"), "random": C.random_pair(shape, lr_shape, 1)}


def test_adjoint_identity_and_step_bound():
    rng = np.random.default_rng(0)
    for shape, lr_shape in C.SHAPES + [((50, 50), (25, 25))]:
        x, r = rng.standard_normal(shape), rng.standard_normal(lr_shape)
        for kind, (R0, R1) in _pairs(shape, lr_shape).items():
            lhs, rhs = (C.apply(x, R0, R1) * r).sum(), (x * C.adjoint(r, R0, R1)).sum()
            scale = np.abs(C.apply(x, R0, R1) * r).sum() + np.abs(x * C.adjoint(r, R0, R1)).sum()
            c0, c1 = C.norm_bound(R0), C.norm_bound(R1)
            n0, n1 = np.linalg.norm(R0, 2) ** 2, np.linalg.norm(R1, 2) ** 2
            print(f"{shape} -> {lr_shape} {kind}: dot test {abs(lhs - rhs) / scale:.2e}; c {c0:.3f} / {c1:.3f} against squared norms "
                  f"{n0:.3f} / {n1:.3f}")
            assert abs(lhs - rhs) <= 1e-12 * scale
            assert c0 >= n0 * (1 - 1e-12) and c1 >= n1 * (1 - 1e-12) and c0 * c1 >= n0 * n1 * (1 - 1e-12)
            assert C.step(R0, R1) == 1.0 / np.sqrt(8.0 + c0 * c1)


def test_the_restatement_reaches_an_independent_minimum():
    hr, y, w, (R0, R1) = C.case_data()
    low = C.lbfgs_minimum(y, R0, R1, C.CASE_LAM, C.CASE_ALPHA, w, C.CASE_SHAPE)
    x, e, change = C.solve(y, R0, R1, C.CASE_LAM, C.CASE_ALPHA, 1000, w=w, return_info=True)
    print(f"weighted Huber case: energy after 1,000 iterations {e:.15e}, L-BFGS-B minimum {low:.15e}, gap {(e - low) / low:.2e}, change "
          f"{change:.2e}")
    assert abs(e - low) <= 1e-9 * low
    # a datum of weight 0 is not read
    yp = y.copy()
    yp[2, 3] = np.nan
    assert w[2, 3] == 0 and np.array_equal(C.solve(yp, R0, R1, C.CASE_LAM, C.CASE_ALPHA, 30, w=w), C.solve(y, R0, R1, C.CASE_LAM, C.CASE_ALPHA, 30, w=w))


def test_the_restatement_agrees_with_the_block_solver():
    k0, k1 = np.full(3, 1.0 / 3.0), np.array([0.2, 0.8])
    k = np.outer(k0, k1)
    hr, _ = T.case_data()
    y = T.apply_A(hr, k)
    pair = (C.block_operator(6, 3, k0), C.block_operator(10, 2, k1))
    a, ea, _ = C.solve(y, *pair, T.CASE_LAM, T.CASE_ALPHA, 1000, w=T.CASE_W, return_info=True)
    b, eb, _ = T.solve(y, T.CASE_FACTORS, k, T.CASE_LAM, T.CASE_ALPHA, 1000, w=T.CASE_W, return_info=True)
    print(f"two restatements after 1,000 iterations: max|x diff| {np.abs(a - b).max():.2e}, energies rel diff {abs(ea[0] - eb[0]) / eb[0]:.2e}")
    assert np.abs(a - b).max() <= 1e-10 and abs(ea[0] - eb[0]) <= 1e-12 * eb[0]


def test_the_restatement_against_longdouble():
    """The restatement's own error: the same iteration in longdouble, on the shapes the GPU tests use.  It must sit orders inside
    the solver's bound of 1e-10 (measured: below 1e-15)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("longdouble is float64 on this platform")
    rng = np.random.default_rng(5)
    hr, y, w, pair = C.case_data()
    d = np.abs(C.solve(y, *pair, C.CASE_LAM, C.CASE_ALPHA, 300, w=w)
               - C.solve(y, *pair, C.CASE_LAM, C.CASE_ALPHA, 300, w=w, dtype=np.longdouble).astype(np.float64)).max()
    print(f"weighted case, 300 iterations: float64 against longdouble {d:.2e}")
    assert d <= 1e-13
    for shape, lr_shape in C.SHAPES:
        pair = C.random_pair(shape, lr_shape, 1)
        y = C.apply(rng.random(shape), *pair)
        x0 = rng.random(shape)
        d = np.abs(C.solve(y, *pair, 0.05, 0.05, 20, x0=x0) - C.solve(y, *pair, 0.05, 0.05, 20, x0=x0, dtype=np.longdouble).astype(np.float64)).max()
        print(f"{shape} -> {lr_shape}, 20 iterations: float64 against longdouble {d:.2e}")
        assert d <= 1e-13


def test_operator_makers_against_the_restatement():
    for n, m, fwhm in ((50, 25, 1.2), (100, 50, 1.0), (128, 100, 1.2), (12, 5, 1.2), (20, 7, 1.0), (33, 130, 1.0), (1, 1, 1.0), (384, 128, 2.0)):
        for kind in ("gaussian", "box"):
            op = baselines.psf_operator(n, m, fwhm, kind)
            want = C.psf_operator(n, m, fwhm, kind)
            assert op.shape == (m, n) and op.dtype == np.float64 and (op >= 0).all()
            assert np.abs(op.sum(axis=1) - 1.0).max() <= 1e-15 and np.abs(op - want).max() <= 1e-15, (n, m, kind)
            centre = (np.arange(m) + 0.5) * n / m - 0.5
            if n >= 3 * m / 2:                                  # away from the ends a row is symmetric about its centre
                mid = m // 2
                assert abs((op[mid] * np.arange(n)).sum() - centre[mid]) <= 1e-9 * n, (n, m, kind)
    assert np.allclose(baselines.psf_operator(12, 6, 1.0, "box"), baselines.block_operator(12, 2), atol=1e-15)
    rng = np.random.default_rng(1)
    x = rng.random((3, 12, 20))
    for f0, f1, k0, k1 in ((3, 2, "mean", "mean"), (2, 4, "decimate", "mean"), (3, 5, [0.2, 0.3, 0.5], [0.1, 0.2, 0.3, 0.25, 0.15])):
        R0, R1 = baselines.block_operator(12, f0, k0), baselines.block_operator(20, f1, k1)
        assert np.array_equal(R0, C.block_operator(12, f0, k0)) and R0.shape == (12 // f0, 12)
        k = np.outer(R0[0, :f0], R1[0, :f1])
        d = np.abs(C.apply(x, R0, R1) - T.apply_A(x, k)).max()
        print(f"block_operator {f0} x {f1}: against apply_A {d:.2e}")
        assert d <= 1e-15
    for args, text in (((0, 5, 1.0), "n is an integer"), ((5, 1025, 1.0), "m is an integer"), ((5.5, 5, 1.0), "n is an integer"),
                       ((10, 5, 0.0), "fwhm must be finite and > 0"), ((10, 5, np.nan), "fwhm must be finite"), ((10, 5, "wide"), "fwhm must be"),
                       ((10, 5, 1.0, "lorentz"), "kind must be"), ((100, 50, 1e-3), "fwhm 0.001 is too narrow")):
        with pytest.raises(ValueError, match=f"psf_operator: {text}"):
            baselines.psf_operator(*args)
    for args, text in (((12, 0), "f is an integer 1 .. 8"), ((12, 9), "f is an integer"), ((13, 2), "n is an integer 1 .. 1024 and a whole number of blocks of 2"), ((0, 2), "n is an integer"),
                       ((12, 2, "median"), "kernel must be"), ((12, 2, [1.0]), "must have 2 entries"), ((12, 2, [0.5, 0.6]), "finite and sum to 1"),
                       ((12, 2, [np.nan, 1.0]), "finite and sum to 1")):
        with pytest.raises(ValueError, match=f"block_operator: .*{text}"):
            baselines.block_operator(*args)


def test_header_library_and_ctypes_table_carry_the_symbols():
    text = open(os.path.join(ROOT, "include", "inrhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(inr_[a-z0-9_]+)\s*\(", code))
    build_library()
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(handle, name) and name in _lib.SIGNATURES, name
    assert sorted(k for k in _lib.SIGNATURES if k.startswith("inr_tvop_")) == sorted(NEW)
    assert "tvop.hip" in SOURCES and "-ffp-contract=off" in SOURCE_FLAGS["tvop.hip"]
    for name in ("tv_superres_operator", "operator_apply", "operator_adjoint", "psf_operator", "block_operator", "fourier_operator"):
        assert callable(getattr(baselines, name))
    for name in ("tvop_apply", "tvop_adjoint", "tvop_solve", "tvop_workspace_doubles"):
        assert callable(getattr(ops, name))
    assert (baselines.TVOP_DEFAULT_LAMBDA, baselines.TVOP_DEFAULT_HUBER, baselines.TVOP_DEFAULT_ITERS) == (3e-3, 0.03, 500)
    csrc = os.path.join(ROOT, "mri-super-resolution_amd", "csrc")
    unit = open(os.path.join(csrc, "tvop.hip")).read()
    assert "a field is either read across threads or written by its owner alone" in unit and "STREAM ORDER IS THE BARRIER" in unit
    assert "atomic" not in re.sub(r"//.*", "", unit) and "hipLaunchCooperativeKernel" not in unit
    # one definition of the tile loop: the MFMA lives in the shared header, both units include it
    fourier = open(os.path.join(csrc, "fourier.hip")).read()
    shared = open(os.path.join(csrc, "gemm_f64.h")).read()
    assert "__builtin_amdgcn_mfma_f64" in shared and "__builtin_amdgcn_mfma" not in unit and "__builtin_amdgcn_mfma" not in fourier
    assert '#include "gemm_f64.h"' in unit and '#include "gemm_f64.h"' in fourier and "gf_tile<" in unit and "gf_tile<" in fourier


def _plan(n, H, W, h, w):
    """tau, x | xbar | p0 | p1, q, the plane [h][W], the energy partials per LR and per HR tile, the change partials per HR tile;
    every field rounded up to 16 bytes."""
    even = lambda doubles: doubles + doubles % 2
    tiles = lambda a, b: -(-a // 64) * -(-b // 64)
    TL, TH = tiles(h, w), tiles(H, W)
    return 2 + even(n * 4 * H * W) + even(n * h * w) + even(n * h * W) + even(n * (TL + TH)) + even(n * TH)


def test_workspace_plan():
    plan = _lib.lib().inr_tvop_workspace_doubles
    err = _lib.lib().inr_last_error
    for n, H, W, h, w in ((1, 12, 20, 5, 7), (3, 12, 20, 5, 7), (40, 130, 70, 37, 33), (2, 37, 33, 130, 70), (1, 1, 70, 1, 33), (5, 1, 1, 1, 1),
                          (28, 50, 50, 25, 25), (1, 1024, 1024, 1024, 1024), (7, 3, 3, 3, 5)):
        assert plan(n, H, W, h, w) == ops.tvop_workspace_doubles(n, H, W, h, w) == _plan(n, H, W, h, w), (n, H, W, h, w)
    assert plan(0, 12, 20, 5, 7) == plan(1, 12, 20, 5, 7) > 0
    for args, text in (((-1, 12, 20, 5, 7), b"bad sizes (n_images"), ((1, 0, 20, 5, 7), b"height and width are 1 .. 1024"),
                       ((1, 12, 1025, 5, 7), b"height and width are 1 .. 1024"), ((1, 12, 20, 0, 7), b"lr_height and lr_width are 1 .. 1024"),
                       ((1, 12, 20, 5, 1025), b"lr_height and lr_width are 1 .. 1024"), ((1, 12, 20, -5, 7), b"lr_height and lr_width")):
        assert plan(*args) == 0 and b"inr_tvop_workspace_doubles" in err() and text in err(), (args, err())


def test_every_refusal_comes_before_device_work():
    lib = _lib.lib()
    fake = lambda k: ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)      # never dereferenced: every call fails in validation
    err = lib.inr_last_error
    nan, inf = float("nan"), float("inf")
    need = lib.inr_tvop_workspace_doubles(2, 12, 20, 5, 7)
    INV, WS, AL = _lib.INR_E_INVALID, _lib.INR_E_WORKSPACE, _lib.INR_E_ALIGN
    names = ("out", "energy", "change", "y", "weight", "x0", "r0", "r1", "n", "H", "W", "h", "w", "lam", "alpha", "n_iter", "ws", "doubles",
             "stream")
    for call in (lib.inr_tvop_solve2d, lib.inr_tvop_solve2d_f32):
        who = call.__name__.encode()
        ok = [fake(0), fake(1), fake(2), fake(3), None, None, fake(4), fake(5), 2, 12, 20, 5, 7, 0.05, 0.02, 10, fake(6), need, None]

        def bad(code, text, **change):
            args = [change.get(name, value) for name, value in zip(names, ok)]
            assert call(*args) == code, (change, err())
            assert text in err() and who in err(), (change, err())

        bad(INV, b"null pointer", out=None)
        bad(INV, b"null pointer", y=None)
        bad(INV, b"null pointer (r0 / r1)", r0=None)
        bad(INV, b"null pointer (r0 / r1)", r1=None)
        bad(INV, b"bad sizes (n_images", n=-1)
        for name, text in (("H", b"height and width"), ("W", b"height and width"), ("h", b"lr_height and lr_width"), ("w", b"lr_height and lr_width")):
            for value in (0, -1, 1025):
                bad(INV, text, **{name: value})
        bad(INV, b"n_iter must be 0 .. 100000", n_iter=-1)
        bad(INV, b"n_iter must be 0 .. 100000", n_iter=100001)
        for name, text in (("lam", b"lambda must be finite and >= 0"), ("alpha", b"alpha must be finite and >= 0")):
            for value in (-1e-3, nan, inf):
                bad(INV, text, **{name: value})
        bad(WS, b"workspace too small", doubles=need - 1)
        bad(WS, b"workspace too small", ws=None)
        bad(AL, b"16-byte aligned", ws=ctypes.c_void_p(0x7000_0000_0008))
        # n_images = 0 succeeds and launches nothing; energy and change are optional
        zero = list(ok)
        zero[8] = 0
        assert call(*zero) == 0
        zero[1] = zero[2] = None
        assert call(*zero) == 0
    # out, in, r0, r1, n, H, W, h, w, workspace, doubles, stream
    for call in (lib.inr_tvop_apply, lib.inr_tvop_adjoint):
        who = call.__name__.encode()
        ok = [fake(0), fake(1), fake(2), fake(3), 2, 12, 20, 5, 7, fake(6), need, None]
        sub = lambda i, v: ok[:i] + [v] + ok[i + 1:]
        for args, code, text in ((sub(0, None), INV, b"null pointer"), (sub(1, None), INV, b"null pointer"), (sub(2, None), INV, b"null pointer (r0 / r1)"),
                                 (sub(3, None), INV, b"null pointer (r0 / r1)"), (sub(4, -1), INV, b"bad sizes (n_images"),
                                 (sub(5, 0), INV, b"height and width"), (sub(6, 1025), INV, b"height and width"),
                                 (sub(7, 0), INV, b"lr_height and lr_width"), (sub(8, 2000), INV, b"lr_height and lr_width"),
                                 (sub(9, None), WS, b"workspace too small"), (sub(10, need - 1), WS, b"workspace too small"),
                                 (sub(9, ctypes.c_void_p(0x7000_0000_0008)), AL, b"16-byte aligned")):
            assert call(*args) == code and text in err() and who in err(), (args, err())
        assert call(*sub(4, 0)) == 0


def test_python_entry_points_refuse_by_name():
    B = baselines
    hr, y, w, pair = C.case_data()
    who = "tv_superres_operator"
    for kwargs, kind, text in (({"lam": -1.0}, ValueError, "lam must be finite"), ({"lam": np.nan}, ValueError, "lam must be finite"),
                               ({"huber": np.inf}, ValueError, "huber must be finite"), ({"n_iter": 1.5}, ValueError, "n_iter must be an integer"),
                               ({"n_iter": 100001}, ValueError, "n_iter must be an integer"), ({"weight": np.ones((5, 8))}, ValueError, "weight must have shape"),
                               ({"weight": -w}, ValueError, "weight must be finite and >= 0"), ({"weight": torch.ones(5, 7)}, TypeError, "weight must be given like lr"),
                               ({"x0": np.ones((12, 21))}, ValueError, "x0 must have shape"), ({"x0": torch.ones(12, 20)}, TypeError, "x0 must be given like lr")):
        with pytest.raises(kind, match=f"{who}: {text}"):
            B.tv_superres_operator(y, pair, **kwargs)
    bad_nan = pair[0].copy()
    bad_nan[0, 0] = np.nan
    for operators, kind, text in ((pair[0], ValueError, "operators are a pair"), ((pair[0],), ValueError, "operators are a pair"),
                                  ((pair[0].astype(np.float32), pair[1]), TypeError, r"operators\[0\] must be float64"),
                                  ((pair[0], pair[1].tolist()), TypeError, r"operators\[1\] must be a float64 ndarray or a device float64 tensor"),
                                  ((bad_nan, pair[1]), ValueError, r"operators\[0\] must be finite"),
                                  ((pair[0], pair[1][0]), ValueError, r"operators\[1\] must be 2-D"),
                                  ((np.ones((5, 1025)), pair[1]), ValueError, r"operators\[0\] must be 2-D with sides of 1 .. 1024"),
                                  ((pair[0], torch.from_numpy(pair[1])), ops.InrDeviceError, r"operators\[1\] is on cpu")):
        with pytest.raises(kind, match=f"{who}: {text}"):
            B.tv_superres_operator(y, operators)
    with pytest.raises(ValueError, match=f"{who}: the operators make LR images of 5 x 7"):
        B.tv_superres_operator(hr, pair)
    with pytest.raises(ValueError, match=f"{who} needs at least 2-D lr"):
        B.tv_superres_operator(y[0], pair)
    with pytest.raises(TypeError, match=f"{who} takes an ndarray or a device tensor"):
        B.tv_superres_operator(y.tolist(), pair)
    with pytest.raises(ops.InrDeviceError, match="no CPU fallback"):
        B.tv_superres_operator(torch.from_numpy(y), pair)
    with pytest.raises(ValueError, match="operator_apply: the operators take images of 12 x 20"):
        B.operator_apply(y, pair)
    with pytest.raises(ValueError, match="operator_adjoint: the operators take images of 5 x 7"):
        B.operator_adjoint(hr, pair)
    with pytest.raises(ValueError, match="operator_apply: operators are a pair"):
        B.operator_apply(hr, None)
    if not torch.cuda.is_available():
        with pytest.raises(ops.InrDeviceError):
            B.tv_superres_operator(y, pair)                   # there is no CPU fallback


def test_the_study_refuses_by_name_before_the_input_is_loaded(tmp_path):
    from mri_super_resolution_amd import drivers
    from mri_super_resolution_amd.scripts import acquisition_model as script
    who = "acquisition_model_study"
    assert drivers.check_acquisition_model("kspace", 50) == 25 and drivers.check_acquisition_model("kspace", 50, lr_side=20) == 20
    assert drivers.check_acquisition_model("block", 50, factor=5) == 10 and drivers.check_acquisition_model("gaussian", 28, fwhm=1.0) == 14
    assert drivers.check_acquisition_model("block", 50, lr_side=10) == 10
    assert drivers.ACQUISITION_MODELS == ("kspace", "gaussian", "block")
    assert drivers.ACQUISITION_METHODS == ("spline", "zerofill", "tv_block", "tv_operator")
    for kwargs, text in (({"model": "radial"}, "model must be one of"), ({"side": 6}, "the HR side is 7 .. 1024"), ({"side": 1025}, "the HR side is"),
                         ({"factor": 2, "lr_side": 25}, "give factor or lr_side, not both"), ({"factor": 0}, "factor is 1 .. 8"),
                         ({"factor": 9}, "factor is 1 .. 8"), ({"factor": 3}, "divides the HR side 50"), ({"factor": 2.5}, "factor is 1 .. 8"),
                         ({"lr_side": 1}, "lr_side is 2 .. 1024"), ({"lr_side": 1025}, "lr_side is 2 .. 1024"),
                         ({"model": "block", "lr_side": 20}, "model='block' needs a whole number of blocks"),
                         ({"model": "block", "lr_side": 5}, "model='block' needs a whole number of blocks"),
                         ({"fwhm": 1.2}, "fwhm belongs to model='gaussian'"), ({"model": "gaussian", "fwhm": 0.0}, "fwhm must be finite and > 0"),
                         ({"model": "gaussian", "fwhm": np.inf}, "fwhm must be finite"), ({"noise": -0.1}, "noise must be finite"),
                         ({"noise": np.nan}, "noise must be finite"), ({"tv_lambda": -1.0}, "tv_lambda must be finite"),
                         ({"tv_huber": np.inf}, "tv_huber must be finite"), ({"tv_iters": 0}, "tv_iters must be 1 .. 100,000"),
                         ({"tv_iters": 100001}, "tv_iters must be 1 .. 100,000")):
        args = {"model": "kspace", "side": 50, **kwargs}
        with pytest.raises(ValueError, match=f"{who}: .*{text}"):
            drivers.check_acquisition_model(**args)
    with pytest.raises(ValueError, match=f"{who}: slices are \\[Z, R, R\\]"):
        drivers.acquisition_model_study(np.ones((3, 20, 21)))
    with pytest.raises(ValueError, match=f"{who}: model must be one of"):
        drivers.acquisition_model_study(np.ones((3, 20, 20)), "spiral")
    # the script: every flag is refused before the input is loaded -- the file does not exist
    missing = str(tmp_path / "pat01_missing.mat")
    base = ["--data", missing, "--output_address", str(tmp_path / "out")]
    for flags, text in ((["--model", "kspace", "--factor", "2", "--lr_side", "20"], "give factor or lr_side"),
                        (["--model", "block", "--lr_side", "20"], "model='block' needs a whole number"),
                        (["--model", "kspace", "--fwhm", "1.2"], "fwhm belongs to"), (["--model", "gaussian", "--noise", "-1"], "noise must be"),
                        (["--model", "kspace", "--tv_iters", "0"], "tv_iters must be"), (["--model", "kspace", "--tv_lambda", "nan"], "tv_lambda must be"),
                        (["--model", "kspace", "--roi_start", "40", "--roi_end", "40"], "0 <= roi_start < roi_end"),
                        (["--model", "kspace", "--roi_start", "40", "--roi_end", "45"], "the HR side is 7"),
                        (["--model", "kspace", "--roi_start", "0", "--roi_end", "51"], "factor is 1 .. 8 and divides the HR side 51"),
                        (["--model", "kspace", "--slices", "-1"], "--slices are indexes >= 0"), (["--model", "kspace", "--b_index", "-1"], "--b_index must be")):
        with pytest.raises(ValueError, match=text):
            script.main(base + flags)
    with pytest.raises(SystemExit):
        script.main(base + ["--model", "spiral"])
    with pytest.raises(SystemExit):
        script.main(base)                                              # --model is required
    assert not os.path.exists(str(tmp_path / "out"))
    with pytest.raises((FileNotFoundError, OSError)):
        script.main(base + ["--model", "kspace"])                      # good flags: the first thing to fail is the load
