"""CPU: the S0 / ADC solver of csrc/tvadc.hip.  The float64 restatement the kernel is written from
(tests/tvadc_common.py) against itself -- extended precision, the bounded L-BFGS-B minimum of the stated energy from four starts, a
finite-difference check of the analytic gradient the minimiser uses -- and the surface: header, exports, ctypes table, workspace plan,
every refusal of the C entry points before device work with fake pointers that are never dereferenced, and the refusals of the Python
entry points and the drivers by name.  Every test prints what it measured before it asserts."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import tvadc_common as A
from tests import tvsr_common as T
from mri_super_resolution_amd import _lib, baselines, drivers, ops, reports
from mri_super_resolution_amd.scripts import joint_bvalues as jb_script
from mri_super_resolution_amd.scripts import superresDWI as dwi_script
from mri_super_resolution_amd._build import LIB_PATH, SOURCE_FLAGS, SOURCES, build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("inr_tvadc_workspace_doubles", "inr_tvadc_solve2d", "inr_tvadc_solve2d_f32", "inr_adc_signal", "inr_adc_signal_f32")


# ---- the restatement against itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coupling", ("joint", "none"))
def test_float64_restatement_agrees_with_extended_precision(coupling):
    """What licenses the 1e-10 bound of test_gpu_tvadc.py: the nonlinear iteration does not amplify rounding."""
    assert np.finfo(np.longdouble).nmant >= 63
    for n in (1, 2, 300, 1000):
        s, adc, _, _ = A.case_solve(n, coupling)
        sl, adcl, _, _ = A.case_solve(n, coupling, dtype=np.longdouble)
        err_s, err_u = float(np.abs(s - sl).max()), float(np.abs(adc - adcl).max() * A.CASE_B.max())
        print(f"{coupling}, {n} iterations: max|float64 - longdouble| s {err_s:.2e}, u {err_u:.2e} (bound 1e-13)")
        assert sl.dtype == adcl.dtype == np.longdouble and s.dtype == np.float64
        assert err_s <= 1e-13 and err_u <= 1e-13


def test_analytic_gradient_of_the_restated_objective_matches_central_differences():
    """The gradient L-BFGS-B is given: a wrong Jacobian sign or factor in it would move the reference minimum."""
    s, u, y, w = A.case_data()
    k = T.block_kernel("mean", A.CASE_FACTORS)
    beta = A.CASE_B / A.CASE_B.max()
    yd = np.where(w == 0, 0.0, y)
    rng = np.random.default_rng(3)
    s, u = s + 0.05 * rng.standard_normal(s.shape), u + 0.2 * rng.standard_normal(u.shape)
    for coupling in ("joint", "none"):
        f = lambda a, c: A.objective_and_gradient(a, c, beta, yd, k, A.CASE_LAM, A.CASE_ALPHA, w, A.CASE_MU, coupling)
        value, g_s, g_u = f(s, u)
        worst = 0.0
        for which, grad in ((0, g_s), (1, g_u)):
            for idx in ((0, 0, 0), (0, 2, 7), (0, 5, 9), (0, 3, 4)):
                step = np.zeros_like(s)
                step[idx] = 1e-6
                up = f(s + step, u)[0] if which == 0 else f(s, u + step)[0]
                down = f(s - step, u)[0] if which == 0 else f(s, u - step)[0]
                worst = max(worst, abs((up - down) / 2e-6 - grad[idx]))
        restated = float(A.energy_adc(s, u, beta, yd, k, A.CASE_LAM, A.CASE_ALPHA, w, A.CASE_MU, coupling)[0])
        print(f"{coupling}: max|central difference - analytic| = {worst:.2e} (bound 1e-8); objective {value:.12f} against energy_adc {restated:.12f}")
        assert worst <= 1e-8 and abs(value - restated) <= 1e-14


@pytest.mark.parametrize("coupling", ("joint", "none"))
def test_restated_iteration_reaches_the_lbfgs_minimum_from_four_starts(coupling):
    """Independent of the iteration: bounded L-BFGS-B with the analytic gradient from the solver's start and three random starts."""
    minimum, minima = A.case_minimum(coupling)
    e_start = float(A.case_solve(0, coupling)[2][0])
    ratios = {}
    for n in (3000, 10000):
        s, adc, e, change = A.case_solve(n, coupling)
        ratios[n] = (float(e[0]) - minimum) / (e_start - minimum)
        print(f"{coupling}: L-BFGS-B minima {[f'{m:.12f}' for m in minima]}; start {e_start:.6f}; {n} iterations: energy {float(e[0]):.12f}, "
              f"(E - E*) / (E_start - E*) = {ratios[n]:.2e}, change {float(change[0]):.2e}")
    assert max(minima) - min(minima) <= 1e-9 * abs(minimum)          # one minimum
    assert ratios[10000] <= 1e-6
    assert 0.0 <= s.min() and s.max() <= A.CASE_SMAX and 0.0 <= adc.min() and adc.max() <= A.CASE_ADCMAX


def test_the_start_and_the_missing_datum_rule_of_the_restatement():
    _, _, y, w = A.case_data()
    s, u = A.start(y, A.CASE_B, A.CASE_FACTORS, A.CASE_SMAX, A.CASE_ADCMAX, A.CASE_ADC0)
    assert np.array_equal(s, np.clip(T.replicate(y[:, 0], A.CASE_FACTORS), 0, A.CASE_SMAX)) and np.all(u == A.CASE_ADC0 * 1000.0)
    s, u = A.start(y, A.CASE_B, A.CASE_FACTORS, A.CASE_SMAX, A.CASE_ADCMAX, A.CASE_ADC0, x0=(np.full((1, 6, 10), 2.0), np.full((1, 6, 10), -1.0)))
    assert np.all(s == A.CASE_SMAX) and np.all(u == 0.0)
    # a w = 0 datum is never read by the iteration: from one given start, whatever it holds, the same bits
    a = A.case_solve(30)
    x0 = (A.start(y, A.CASE_B, A.CASE_FACTORS, A.CASE_SMAX, A.CASE_ADCMAX, A.CASE_ADC0)[0], np.full((1, 6, 10), A.CASE_ADC0))
    for value in (1e3, float("nan")):
        other = y.copy()
        other[w == 0] = value
        b = A.solve_adc(other, A.CASE_B, A.CASE_FACTORS, "mean", A.CASE_LAM, A.CASE_ALPHA, 30, A.CASE_MU, "joint", A.CASE_SMAX, A.CASE_ADCMAX,
                        A.CASE_ADC0, w=w, x0=x0, return_info=True)
        assert (w == 0).sum() == 1 and all(np.array_equal(p, q) for p, q in zip(a, b)), value


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_ctypes_table_carry_the_symbols():
    text = open(os.path.join(ROOT, "include", "inrhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(inr_[a-z0-9_]+)\s*\(", code))
    build_library()
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(handle, name) and name in _lib.SIGNATURES, name
    assert sorted(k for k in _lib.SIGNATURES if k.startswith(("inr_tvadc_", "inr_adc_signal"))) == sorted(NEW)
    assert "tvadc.hip" in SOURCES and "-ffp-contract=off" in SOURCE_FLAGS["tvadc.hip"]
    for name in ("tv_superres_adc", "adc_signal"):
        assert callable(getattr(baselines, name))
    for name in ("tvadc_solve", "tvadc_workspace_doubles", "adc_signal"):
        assert callable(getattr(ops, name))
    assert reports.SSIM_TV_ADC_HEADER == "Pt_id, b-value, slice, SSIM-tv-adc, SSIM-SR\n"
    src = open(os.path.join(ROOT, "mri-super-resolution_amd", "csrc", "tvadc.hip")).read()
    assert '#include "tv_block.h"' in src and "int tv_shape_check(" not in src and "atomic" not in src.split("#include")[1]
    assert src.count("__syncthreads();   // barrier") == 2


def test_workspace_plan():
    plan = _lib.lib().inr_tvadc_workspace_doubles
    # s | u | sbar | ubar | p_s0 | p_s1 | p_u0 | p_u1 [H][W] and z [C][h][w] of every group, nothing else
    assert plan(1, 3, 6, 10, 3, 2) == 8 * 60 + 3 * 10 and plan(300, 2, 12, 12, 2, 3) == 300 * (8 * 144 + 2 * 24)
    assert plan(1, 16, 1024, 1024, 1, 1) == (8 + 16) << 20
    assert plan(0, 2, 8, 8, 2, 2) == plan(1, 2, 8, 8, 2, 2) > 0
    err = _lib.lib().inr_last_error
    assert plan(-1, 2, 8, 8, 2, 2) == 0 and b"inr_tvadc_workspace_doubles" in err() and b"bad sizes (n_groups" in err()
    assert plan(1, 1, 8, 8, 2, 2) == 0 and b"b-values are 2 .. 16" in err()
    assert plan(1, 17, 8, 8, 2, 2) == 0 and b"b-values are 2 .. 16" in err()
    assert plan(1, 2, 8, 8, 3, 2) == 0 and b"no whole number" in err()
    assert plan(1, 2, 8, 1025, 1, 1) == 0 and b"bad sizes" in err()
    assert ops.tvadc_workspace_doubles(2, 4, 50, 50, (2, 2)) == 2 * (8 * 2500 + 4 * 625)


def test_every_refusal_comes_before_device_work():
    lib = _lib.lib()
    fake = lambda k: ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)      # never dereferenced: every call fails in validation
    err = lib.inr_last_error
    K = lambda *v: (ctypes.c_double * len(v))(*v)
    mean6, nan, inf = K(*([1 / 6] * 6)), float("nan"), float("inf")
    need = lib.inr_tvadc_workspace_doubles(2, 3, 6, 10, 3, 2)
    INV, WS, AL = _lib.INR_E_INVALID, _lib.INR_E_WORKSPACE, _lib.INR_E_ALIGN
    names = ("out", "energy", "change", "y", "weight", "x0", "n", "C", "H", "W", "f0", "f1", "kernel", "b", "mu", "lam", "alpha", "coupling",
             "n_iter", "s_max", "adc_max", "adc0", "ws", "doubles", "stream")
    for call in (lib.inr_tvadc_solve2d, lib.inr_tvadc_solve2d_f32):
        who = call.__name__.encode()
        ok = [fake(0), fake(1), fake(2), fake(3), None, None, 2, 3, 6, 10, 3, 2, mean6, K(0.0, 400.0, 1000.0), K(1.0, 0.1), 0.02, 0.01, 1, 10,
              1.5, 6e-3, 1e-3, fake(4), need, None]

        def bad(code, text, **change):
            args = [change.get(name, value) for name, value in zip(names, ok)]
            assert call(*args) == code, (change, err())
            assert text in err() and who in err(), (change, err())

        bad(INV, b"null pointer (out, y or b)", out=None)
        bad(INV, b"null pointer (out, y or b)", y=None)
        bad(INV, b"null pointer (out, y or b)", b=None)
        bad(INV, b"null pointer (kernel)", kernel=None)
        bad(INV, b"bad sizes (n_groups = -1)", n=-1)
        bad(INV, b"b-values are 2 .. 16 per group (got 1)", C=1)
        bad(INV, b"b-values are 2 .. 16 per group (got 17)", C=17)
        bad(INV, b"block factors are 1 .. 8", f0=0)
        bad(INV, b"bad sizes (HR images", W=1026)
        bad(INV, b"no whole number of 3 x 2 blocks", H=7)
        bad(INV, b"n_iter must be >= 0 (got -1)", n_iter=-1)
        for name, text in (("lam", b"lambda must be finite and >= 0"), ("alpha", b"alpha must be finite and >= 0")):
            for value in (-1e-3, nan, inf):
                bad(INV, text, **{name: value})
        for value in (-1, 2):
            bad(INV, b"coupling is 0 (none) or 1 (joint) (got %d)" % value, coupling=value)
        bad(INV, b"block kernel must be finite", kernel=K(0.5, nan, 0.5, 0, 0, 0))
        bad(INV, b"block kernel must sum to 1", kernel=K(*([0.5] * 6)))
        bad(INV, b"b-values must be finite and >= 0 (entry 1 is", b=K(0.0, -1.0, 1000.0))
        bad(INV, b"b-values must be finite and >= 0 (entry 0 is", b=K(nan, 400.0, 1000.0))
        bad(INV, b"b-values must be finite and >= 0 (entry 2 is", b=K(0.0, 400.0, inf))
        bad(INV, b"the b-values are all equal (700)", b=K(700.0, 700.0, 700.0))
        for value in (0.0, -1.0, nan, inf):
            bad(INV, b"s_max must be finite and > 0", s_max=value)
            bad(INV, b"adc_max must be finite and > 0", adc_max=value)
        bad(INV, b"adc_max must be finite and > 0", adc_max=1e308)               # adc_max b_max overflows
        for value in (-1e-4, 7e-3, nan):
            bad(INV, b"adc0 must be within [0, adc_max]", adc0=value)
        bad(INV, b"map_weights must be finite and within [0, 1] (entry 1 is", mu=K(1.0, 1.5))
        bad(INV, b"map_weights must be finite and within [0, 1] (entry 0 is", mu=K(-0.1, 0.5))
        bad(INV, b"map_weights must be finite and within [0, 1] (entry 0 is", mu=K(nan, 0.5))
        bad(WS, b"workspace too small", doubles=need - 1)
        bad(WS, b"workspace too small", ws=None)
        bad(AL, b"16-byte aligned", ws=ctypes.c_void_p(0x7000_0000_0008))
        # n_groups = 0 succeeds and launches nothing; energy, change and the map weights are optional
        zero = list(ok)
        zero[6] = 0
        assert call(*zero) == 0
        zero[1] = zero[2] = zero[14] = None
        assert call(*zero) == 0
    for call in (lib.inr_adc_signal, lib.inr_adc_signal_f32):
        assert call(None, fake(1), fake(2), K(0.0, 1000.0), 1, 2, 100, None) == INV and b"null pointer" in err()
        assert call(fake(0), fake(1), fake(2), K(0.0, 1000.0), 1, 17, 100, None) == INV and b"b-values are 1 .. 16" in err()
        assert call(fake(0), fake(1), fake(2), K(0.0, nan), 1, 2, 100, None) == INV and b"b-values must be finite" in err()
        assert call(fake(0), fake(1), fake(2), K(0.0, 1000.0), -1, 2, 100, None) == INV and b"bad sizes" in err()
        assert call(fake(0), fake(1), fake(2), K(0.0, 1000.0), 0, 2, 100, None) == 0


def test_python_entry_points_refuse_by_name():
    lr = np.ones((3, 5, 5))
    b = (0.0, 400.0, 1000.0)
    fn = baselines.tv_superres_adc
    with pytest.raises(TypeError, match="tv_superres_adc takes an ndarray or a device tensor.*list"):
        fn([[[1.0, 2.0], [3.0, 4.0]]], b, (1, 1))
    with pytest.raises(ops.InrDeviceError, match="tv_superres_adc.*no CPU fallback"):
        fn(torch.ones(3, 4, 4), b, (2, 2))
    with pytest.raises(ValueError, match="tv_superres_adc needs at least 3-D input"):
        fn(np.ones((4, 4)), b, (2, 2))
    with pytest.raises(ValueError, match="tv_superres_adc: b-values are 2 .. 16 per group \\(got 17\\)"):
        fn(np.ones((17, 4, 4)), np.arange(17.0), (2, 2))
    with pytest.raises(ValueError, match="tv_superres_adc: b-values are 2 .. 16 per group \\(got 1\\)"):
        fn(np.ones((1, 4, 4)), (0.0,), (2, 2))
    with pytest.raises(ValueError, match="tv_superres_adc: b has 2 b-values, expected one per channel \\(3\\)"):
        fn(lr, (0.0, 1000.0), (2, 2))
    for bad_b, text in (((0.0, -5.0, 1000.0), "b-values must be finite and >= 0"), ((0.0, float("nan"), 1000.0), "b-values must be finite and >= 0"),
                        ((0.0, float("inf"), 1000.0), "b-values must be finite and >= 0"), ((500.0, 500.0, 500.0), "the b-values are all equal")):
        with pytest.raises(ValueError, match=f"tv_superres_adc: {text}"):
            fn(lr, bad_b, (2, 2))
    with pytest.raises(ValueError, match="tv_superres_adc: kernel must be 'mean', 'decimate' or an array.*'box'"):
        fn(lr, b, (2, 2), kernel="box")
    with pytest.raises(ValueError, match="tv_superres_adc: factors are 1 .. 8 per axis.*9 x 1"):
        fn(lr, b, (9, 1))
    with pytest.raises(ValueError, match="tv_superres_adc: HR images of 1 .. 1024"):
        fn(np.ones((3, 300, 4)), b, (4, 1))
    with pytest.raises(ValueError, match="tv_superres_adc: coupling must be 'joint' or 'none'.*'tnv'"):
        fn(lr, b, (2, 2), coupling="tnv")
    for kw, text in (({"lam": -1.0}, "lam must be finite and >= 0"), ({"lam": float("nan")}, "lam must be finite"),
                     ({"huber": -0.1}, "huber must be finite and >= 0"), ({"huber": float("inf")}, "huber must be finite"),
                     ({"n_iter": -1}, "n_iter must be an integer >= 0"), ({"n_iter": 2.5}, "n_iter must be an integer"),
                     ({"s_max": 0.0}, "s_max must be finite and > 0"), ({"s_max": float("inf")}, "s_max must be finite and > 0"),
                     ({"adc_max": -1e-3}, "adc_max must be finite and > 0"), ({"adc_max": float("nan")}, "adc_max must be finite and > 0"),
                     ({"adc0": -1e-4}, "adc0 must be within \\[0, adc_max\\]"), ({"adc0": 5e-3}, "adc0 must be within \\[0, adc_max\\]")):
        with pytest.raises(ValueError, match=f"tv_superres_adc: {text}"):
            fn(lr, b, (2, 2), **kw)
    for mu in ((1.0,), (1.0, 0.5, 0.5), (1.0, 1.5), (-0.1, 0.5), (1.0, float("nan"))):
        with pytest.raises(ValueError, match="tv_superres_adc: map_weights are \\(mu_s, mu_d\\), two finite values within \\[0, 1\\]"):
            fn(lr, b, (2, 2), map_weights=mu)
    with pytest.raises(TypeError, match="tv_superres_adc: weight must be given like lr"):
        fn(lr, b, (2, 2), weight=torch.ones(3, 5, 5))
    with pytest.raises(ValueError, match="tv_superres_adc: x0 is a pair \\(s0, adc\\) of maps of shape \\(10, 10\\)"):
        fn(lr, b, (2, 2), x0=np.ones((2, 10, 10)))
    with pytest.raises(ValueError, match="tv_superres_adc: x0 is a pair \\(s0, adc\\) of maps of shape \\(10, 10\\)"):
        fn(lr, b, (2, 2), x0=(np.ones((10, 10)), np.ones((5, 5))))
    with pytest.raises(TypeError, match="tv_superres_adc: x0 must be given like lr"):
        fn(lr, b, (2, 2), x0=(np.ones((10, 10)), torch.ones(10, 10)))
    with pytest.raises(ops.InrDeviceError, match="adc_signal.*no CPU fallback"):
        baselines.adc_signal(torch.ones(4, 4), torch.ones(4, 4), b)
    with pytest.raises(ValueError, match="adc_signal: adc must have the shape and type of s0"):
        baselines.adc_signal(np.ones((4, 4)), np.ones((4, 5)), b)
    with pytest.raises(ValueError, match="adc_signal: b is 1 .. 16 finite b-values"):
        baselines.adc_signal(np.ones((4, 4)), np.ones((4, 4)), (0.0, float("nan")))
    # ops takes device tensors only, and checks the model's host values before anything else of it
    k = [[0.25, 0.25], [0.25, 0.25]]
    with pytest.raises(ops.InrDeviceError, match="y is on cpu"):
        ops.tvadc_solve(torch.ones(1, 2, 4, 4, dtype=torch.float64), (0.0, 1000.0), (2, 2), k, (1.0, 0.1), 0.01, 0.0, "joint", 3, 1.5, 4e-3, 1e-3)
    with pytest.raises(TypeError, match="y must be a torch.Tensor"):
        ops.tvadc_solve(np.ones((1, 2, 4, 4)), (0.0, 1000.0), (2, 2), k, (1.0, 0.1), 0.01, 0.0, "joint", 3, 1.5, 4e-3, 1e-3)
    ok = dict(b=(0.0, 400.0, 1000.0), channels=3, map_weights=(1.0, 0.1), coupling="joint", s_max=1.5, adc_max=4e-3, adc0=1e-3)
    assert ops.tvadc_model("tvadc_solve", **ok) == ([0.0, 400.0, 1000.0], [1.0, 0.1], 1.5, 4e-3, 1e-3)
    for change, text in (({"channels": 1, "b": (0.0,)}, "b-values are 2 .. 16 per group \\(got 1\\)"), ({"channels": 17}, "b-values are 2 .. 16"),
                         ({"b": (0.0, 1000.0)}, "b has 2 b-values, expected one per channel \\(3\\)"),
                         ({"b": (0.0, -1.0, 5.0)}, "b-values must be finite and >= 0"), ({"b": (0.0, float("nan"), 5.0)}, "b-values must be finite"),
                         ({"b": (5.0, 5.0, 5.0)}, "the b-values are all equal"), ({"coupling": 1}, "coupling must be 'joint' or 'none'"),
                         ({"map_weights": (1.0, 2.0)}, "map_weights are \\(mu_s, mu_d\\)"), ({"map_weights": (1.0,)}, "map_weights are"),
                         ({"s_max": float("nan")}, "s_max must be finite and > 0"), ({"adc_max": 0.0}, "adc_max must be finite and > 0"),
                         ({"adc0": 1.0}, "adc0 must be within \\[0, adc_max\\]")):
        with pytest.raises(ValueError, match=f"tvadc_solve: {text}"):
            ops.tvadc_model("tvadc_solve", **{**ok, **change})
    # the defaults are the ones the drivers' flags carry
    args = dwi_script.build_parser().parse_args(["--data", "x.mat"])
    assert args.tv_adc is False and (args.tv_adc_lambda, args.tv_adc_weight, args.tv_adc_iters) == (
        baselines.ADC_DEFAULT_LAMBDA, baselines.ADC_DEFAULT_MAP_WEIGHTS[1], baselines.ADC_DEFAULT_ITERS)
    args = jb_script.build_parser().parse_args(["--data", "x.mat"])
    assert args.with_adc_model is False and (args.tv_adc_lambda, args.tv_adc_weight, args.tv_adc_iters) == (
        baselines.ADC_DEFAULT_LAMBDA, baselines.ADC_DEFAULT_MAP_WEIGHTS[1], baselines.ADC_DEFAULT_ITERS)
    assert baselines.ADC_DEFAULT_MAP_WEIGHTS[0] == 1.0 and baselines.ADC_DEFAULT_COUPLING in ("joint", "none")
    assert (baselines.ADC_DEFAULT_S_MAX, baselines.ADC_DEFAULT_ADC_MAX, baselines.ADC_DEFAULT_ADC0) == (1.5, 4e-3, 1e-3)


def test_the_drivers_refuse_the_adc_model_flags_before_the_input_is_loaded(tmp_path):
    missing = str(tmp_path / "pat03_not_there.mat")        # never opened: every refusal comes first
    run = lambda *flags: dwi_script.main(["--data", missing, "--output_address", str(tmp_path / "res"), "--roi_start", "2", "--roi_end",
                                          "18", *flags])
    with pytest.raises(ValueError, match="--tv_adc is scored beside the per-channel reconstruction: pass --tv_baseline"):
        run("--tv_adc")
    with pytest.raises(ValueError, match="--tv_adc_lambda must be finite and >= 0.*-0.001"):
        run("--tv_baseline", "--tv_adc", "--tv_adc_lambda", "-0.001")
    with pytest.raises(ValueError, match="--tv_adc_lambda must be finite"):
        run("--tv_baseline", "--tv_adc", "--tv_adc_lambda", "nan")
    with pytest.raises(ValueError, match="--tv_adc_weight must be within \\[0, 1\\].*1.5"):
        run("--tv_baseline", "--tv_adc", "--tv_adc_weight", "1.5")
    with pytest.raises(ValueError, match="--tv_adc_iters must be 1 .. 100,000"):
        run("--tv_baseline", "--tv_adc", "--tv_adc_iters", "0")
    # without --tv_adc its values are not looked at: the run gets as far as the missing input
    with pytest.raises((OSError, ValueError), match="not_there"):
        run("--tv_baseline", "--tv_adc_lambda", "-1")
    with pytest.raises((OSError, ValueError), match="not_there"):
        run("--tv_baseline", "--tv_adc")
    # the b-values are refused once the input is known, before the fit (no device is touched: this machine has none)
    args = dwi_script.build_parser().parse_args(["--data", "x.mat", "--tv_baseline", "--tv_adc"])
    with pytest.raises(ValueError, match="--tv_adc fits one decay over the b-values of a slice and needs 2 .. 16 of them; x.mat has 1"):
        dwi_script._check_optional_outputs(args, "x.mat", np.ones((20, 20, 3, 1)), np.zeros(1), None)
    with pytest.raises(ValueError, match="--tv_adc needs 4 distinct, finite b-values >= 0"):
        dwi_script._check_optional_outputs(args, "x.mat", np.ones((20, 20, 3, 4)), np.full(4, 1000.0), None)
    with pytest.raises(ValueError, match="--tv_adc needs 4 distinct, finite b-values >= 0"):
        dwi_script._check_optional_outputs(args, "x.mat", np.ones((20, 20, 3, 4)), np.arange(3.0), None)
    with pytest.raises(ValueError, match="--tv_adc needs 4 distinct, finite b-values >= 0"):
        dwi_script._check_optional_outputs(args, "x.mat", np.ones((20, 20, 3, 4)), np.array([0.0, -1.0, 5.0, 9.0]), None)
    dwi_script._check_optional_outputs(args, "x.mat", np.ones((20, 20, 3, 4)), np.arange(4.0), None)
    # joint_bvalues --with_adc_model
    jb = lambda *flags: jb_script.main(["--data", missing, "--output_address", str(tmp_path / "res"), *flags])
    with pytest.raises(ValueError, match="joint_bvalue_study: tv_adc_lambda must be finite and >= 0"):
        jb("--with_adc_model", "--tv_adc_lambda", "-1")
    with pytest.raises(ValueError, match="joint_bvalue_study: tv_adc_weight must be within \\[0, 1\\]"):
        jb("--with_adc_model", "--tv_adc_weight", "2")
    with pytest.raises(ValueError, match="joint_bvalue_study: tv_adc_iters must be 1 .. 100,000"):
        jb("--with_adc_model", "--tv_adc_iters", "0")
    with pytest.raises((OSError, ValueError), match="not_there"):
        jb("--tv_adc_lambda", "-1", "--synthetic_adc")
    with pytest.raises(ValueError, match="joint_bvalue_study: the S0 / ADC model needs finite b-values >= 0"):
        drivers.check_adc_model((0.0, -150.0))
    assert drivers.check_adc_model() == (baselines.ADC_DEFAULT_LAMBDA, baselines.ADC_DEFAULT_MAP_WEIGHTS[1], baselines.ADC_DEFAULT_ITERS)
