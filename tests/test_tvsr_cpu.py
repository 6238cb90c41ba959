"""CPU: the surface of the TV / Huber super-resolution baseline (header, exports, ctypes table, workspace plan, every refusal of
csrc/tvsr.hip before device work with fake pointers that are never dereferenced, the refusals of the Python entry points and of the
driver's flags) and the float64 restatement the kernels are written from (tests/tvsr_common.py): the adjoint pairs and the minimum of
the Huber energy found by L-BFGS-B, which shares nothing with the iteration."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import tvsr_common as T
from mri_super_resolution_amd import _lib, baselines, matio, ops
from mri_super_resolution_amd.scripts import superresDWI as dwi_script
from mri_super_resolution_amd.scripts import wiretest as wire_script
from mri_super_resolution_amd._build import LIB_PATH, SOURCE_FLAGS, SOURCES, build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("inr_block_apply2d", "inr_block_adjoint2d", "inr_tvsr_workspace_doubles", "inr_tvsr_solve2d", "inr_tvsr_solve2d_f32")


def test_header_library_and_ctypes_table_carry_the_symbols():
    text = open(os.path.join(ROOT, "include", "inrhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(inr_[a-z0-9_]+)\s*\(", code))
    build_library()
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(handle, name) and name in _lib.SIGNATURES, name
    assert sorted(k for k in _lib.SIGNATURES if k.startswith(("inr_tvsr_", "inr_block_"))) == sorted(NEW)
    assert "tvsr.hip" in SOURCES and "-ffp-contract=off" in SOURCE_FLAGS["tvsr.hip"]
    for name in ("INR_TVSR_MAX_FACTOR", "INR_TVSR_MAX_SIDE"):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == getattr(_lib, name)
    assert (_lib.INR_TVSR_MAX_FACTOR, _lib.INR_TVSR_MAX_SIDE) == (8, 1024)
    for name in ("tv_superres", "block_apply", "block_adjoint"):
        assert callable(getattr(baselines, name))
    for name in ("tvsr_solve", "tvsr_workspace_doubles", "block_apply", "block_adjoint"):
        assert callable(getattr(ops, name))


def test_workspace_plan():
    plan = _lib.lib().inr_tvsr_workspace_doubles
    # x | xbar | p0 | p1 of every image, nothing else
    assert plan(1, 6, 10) == 4 * 60 and plan(300, 12, 12) == 300 * 4 * 144 and plan(3, 7, 1024) == 3 * 4 * 7 * 1024
    assert plan(1, 1024, 1024) == 4 << 20
    assert plan(0, 8, 8) == plan(1, 8, 8) > 0
    err = _lib.lib().inr_last_error
    assert plan(-1, 8, 8) == 0 and b"inr_tvsr_workspace_doubles" in err() and b"bad sizes" in err()
    assert plan(1, 0, 8) == 0 and b"bad sizes" in err()
    assert plan(1, 8, 1025) == 0 and b"bad sizes" in err()
    assert ops.tvsr_workspace_doubles(2, 50, 50) == 2 * 4 * 2500


def test_every_refusal_comes_before_device_work():
    lib = _lib.lib()
    fake = lambda k: ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)      # never dereferenced: every call fails in validation
    err = lib.inr_last_error
    K = lambda *v: (ctypes.c_double * len(v))(*v)
    mean6, nan = K(*([1 / 6] * 6)), float("nan")
    need = lib.inr_tvsr_workspace_doubles(2, 6, 10)
    INV, WS, AL = _lib.INR_E_INVALID, _lib.INR_E_WORKSPACE, _lib.INR_E_ALIGN
    for call in (lib.inr_tvsr_solve2d, lib.inr_tvsr_solve2d_f32):
        who = call.__name__.encode()
        # out, energy, change, y, weight, x0, n, H, W, f0, f1, kernel, lambda, alpha, n_iter, workspace, doubles, stream
        ok = [fake(0), fake(1), fake(2), fake(3), None, None, 2, 6, 10, 3, 2, mean6, 0.05, 0.02, 10, fake(4), need, None]

        def bad(code, text, **change):
            names = ("out", "energy", "change", "y", "weight", "x0", "n", "H", "W", "f0", "f1", "kernel", "lam", "alpha", "n_iter", "ws",
                     "doubles", "stream")
            args = [change.get(name, value) for name, value in zip(names, ok)]
            assert call(*args) == code, (change, err())
            assert text in err() and who in err(), (change, err())

        bad(INV, b"null pointer", out=None)
        bad(INV, b"null pointer", y=None)
        bad(INV, b"null pointer (kernel)", kernel=None)
        bad(INV, b"bad sizes (n_images", n=-1)
        bad(INV, b"block factors are 1 .. 8", f0=0)
        bad(INV, b"block factors are 1 .. 8", f1=9)
        bad(INV, b"bad sizes (HR images", H=0)
        bad(INV, b"bad sizes (HR images", W=1026)
        bad(INV, b"no whole number of 3 x 2 blocks", H=7)
        bad(INV, b"no whole number of 3 x 2 blocks", W=11)
        bad(INV, b"n_iter must be >= 0", n_iter=-1)
        for name, text in (("lam", b"lambda must be finite and >= 0"), ("alpha", b"alpha must be finite and >= 0")):
            for value in (-1e-3, nan, float("inf")):
                bad(INV, text, **{name: value})
        bad(INV, b"block kernel must be finite", kernel=K(0.5, nan, 0.5, 0, 0, 0))
        bad(INV, b"block kernel must be finite", kernel=K(float("inf"), float("-inf"), 1, 0, 0, 0))
        bad(INV, b"block kernel must sum to 1", kernel=K(*([0.5] * 6)))
        bad(INV, b"block kernel must sum to 1", kernel=K(-1, 0, 0, 0, 0, 0))
        bad(WS, b"workspace too small", doubles=need - 1)
        bad(WS, b"workspace too small", ws=None)
        bad(AL, b"16-byte aligned", ws=ctypes.c_void_p(0x7000_0000_0008))
        # n_images = 0 succeeds and launches nothing; energy and change are optional
        zero = list(ok)
        zero[6] = 0
        assert call(*zero) == 0
        zero[1] = zero[2] = None
        assert call(*zero) == 0
    for call in (lib.inr_block_apply2d, lib.inr_block_adjoint2d):
        who = call.__name__.encode()
        ok = [fake(0), fake(1), 2, 6, 10, 3, 2, mean6, None]
        sub = lambda i, v: ok[:i] + [v] + ok[i + 1:]
        for args, text in ((sub(0, None), b"null pointer"), (sub(1, None), b"null pointer"), (sub(7, None), b"null pointer (kernel)"),
                           (sub(2, -1), b"bad sizes"), (sub(3, 8), b"no whole number"), (sub(4, 2048), b"bad sizes"),
                           (sub(5, 9), b"block factors"), (sub(7, K(1, 1, 1, 1, 1, 1)), b"sum to 1"),
                           (sub(7, K(nan, 0, 0, 0, 0, 0)), b"finite")):
            assert call(*args) == INV and text in err() and who in err(), (args, err())
        assert call(*sub(2, 0)) == 0


def test_python_entry_points_refuse_by_name():
    lr = np.ones((5, 5))
    for name, fn in (("tv_superres", baselines.tv_superres), ("block_apply", baselines.block_apply), ("block_adjoint", baselines.block_adjoint)):
        with pytest.raises(TypeError, match=f"{name} takes an ndarray or a device tensor.*list"):
            fn([[1.0, 2.0], [3.0, 4.0]], (1, 1))
        with pytest.raises(ops.InrDeviceError, match=f"{name}.*no CPU fallback"):
            fn(torch.ones(4, 4), (2, 2))
        with pytest.raises(ValueError, match=f"{name}: kernel must be 'mean', 'decimate' or an array.*'box'"):
            fn(np.ones((4, 4)), (2, 2), kernel="box")
        with pytest.raises(ValueError, match=f"{name}: factors are 1 .. 8 per axis.*9 x 1"):
            fn(np.ones((9, 4)), (9, 1))
        with pytest.raises(ValueError, match=f"{name}: factors are \\(f0, f1\\)"):
            fn(np.ones((4, 4)), 2)
        with pytest.raises(ValueError, match=f"{name}: the kernel array must be \\[2\\]\\[2\\]"):
            fn(np.ones((4, 4)), (2, 2), kernel=np.ones((2, 3)) / 6)
        with pytest.raises(ValueError, match=f"{name}: the kernel array must be finite and sum to 1"):
            fn(np.ones((4, 4)), (2, 2), kernel=np.ones((2, 2)))
        with pytest.raises(ValueError, match=f"{name} needs at least 2-D"):
            fn(np.ones(4), (2, 2))
    with pytest.raises(ValueError, match="block_apply: the HR image 5 x 5 is no whole number of 2 x 2 blocks"):
        baselines.block_apply(lr, (2, 2))
    with pytest.raises(ValueError, match="tv_superres: HR images of 1 .. 1024"):
        baselines.tv_superres(np.ones((300, 4)), (4, 1))
    with pytest.raises(ValueError, match="block_adjoint: HR images of 1 .. 1024"):
        baselines.block_adjoint(np.ones((4, 600)), (1, 2))
    for kw, text in (({"lam": -1.0}, "lam must be finite and >= 0"), ({"lam": float("nan")}, "lam must be finite"),
                     ({"huber": -0.1}, "huber must be finite and >= 0"), ({"huber": float("inf")}, "huber must be finite"),
                     ({"n_iter": -1}, "n_iter must be an integer >= 0"), ({"n_iter": 2.5}, "n_iter must be an integer")):
        with pytest.raises(ValueError, match=f"tv_superres: {text}"):
            baselines.tv_superres(lr, (2, 2), **kw)
    with pytest.raises(TypeError, match="tv_superres: weight must be given like lr"):
        baselines.tv_superres(lr, (2, 2), weight=torch.ones(5, 5))
    # the defaults are the ones the driver's flags carry
    args = dwi_script.build_parser().parse_args(["--data", "x.mat"])
    assert (args.tv_lambda, args.tv_huber, args.tv_iters) == (baselines.TV_DEFAULT_LAMBDA, baselines.TV_DEFAULT_HUBER,
                                                             baselines.TV_DEFAULT_ITERS)


def test_driver_flags_default_off_and_refuse_before_the_input_is_loaded(tmp_path):
    args = dwi_script.build_parser().parse_args(["--data", "x.mat"])
    assert args.tv_baseline is False and args.tv_lambda >= 0 and args.tv_huber >= 0 and 1 <= args.tv_iters <= 100000
    assert wire_script.build_parser().parse_args(["--data", "x.mat", "--tv_baseline", "--tv_iters", "7"]).tv_iters == 7
    missing = str(tmp_path / "pat03_not_there.mat")        # never opened: every refusal comes first
    run = lambda r1, *flags: dwi_script.main(["--data", missing, "--output_address", str(tmp_path / "res"), "--roi_start", "2",
                                              "--roi_end", str(r1), *flags])
    with pytest.raises(ValueError, match="--tv_baseline.*even ROI side.*15"):
        run(17, "--tv_baseline")
    with pytest.raises(ValueError, match="--tv_lambda must be finite and >= 0.*-0.001"):
        run(18, "--tv_baseline", "--tv_lambda", "-0.001")
    with pytest.raises(ValueError, match="--tv_lambda must be finite"):
        run(18, "--tv_baseline", "--tv_lambda", "nan")
    with pytest.raises(ValueError, match="--tv_huber must be finite and >= 0.*-0.5"):
        run(18, "--tv_baseline", "--tv_huber", "-0.5")
    for n in ("0", "-3", "100001"):
        with pytest.raises(ValueError, match="--tv_iters must be 1 .. 100,000"):
            run(18, "--tv_baseline", "--tv_iters", n)
    with pytest.raises(ValueError, match="--tv_baseline.*even ROI side"):
        run(17, "--tv_baseline", "--model", "wire")
    # without the flag its values are not looked at: the run gets as far as the missing input
    with pytest.raises((OSError, ValueError), match="not_there"):
        run(17, "--tv_iters", "0", "--tv_lambda", "-1")


def test_run_patient_refuses_a_fit_hook_only_if_it_changes_the_lr_data(tmp_path):
    missing = str(tmp_path / "pat03_not_there.mat")
    args = dwi_script.build_parser().parse_args(["--data", missing, "--output_address", str(tmp_path / "res"), "--roi_start", "2",
                                                 "--roi_end", "18", "--tv_baseline"])

    def other_data(*a):
        raise AssertionError("never reached")
    other_data.changes_lr_data = True

    def same_data(*a):
        raise AssertionError("never reached")
    with pytest.raises(ValueError, match="--tv_baseline.*changes the LR data"):
        dwi_script.run_patient(missing, "03", args, fit=other_data)
    with pytest.raises((OSError, ValueError), match="not_there"):       # passes through to the loading of the input
        dwi_script.run_patient(missing, "03", args, fit=same_data)
    args.tv_baseline = False
    with pytest.raises((OSError, ValueError), match="not_there"):
        dwi_script.run_patient(missing, "03", args, fit=other_data)


def test_restated_operators_are_adjoint_pairs():
    rng = np.random.default_rng(3)
    for H, W, f in ((6, 10, (3, 2)), (8, 8, (1, 1)), (16, 24, (8, 8)), (50, 50, (2, 2)), (7, 1024, (7, 1)), (1024, 3, (1, 3))):
        for kernel in ("mean", "decimate", rng.random(f) / 1.0):
            k = T.block_kernel(kernel if isinstance(kernel, str) else kernel / kernel.sum(), f)
            assert abs(k.sum() - 1.0) <= 1e-15
            x, r = rng.standard_normal((2, H, W)), rng.standard_normal((2, H // f[0], W // f[1]))
            a, b = (T.apply_A(x, k) * r).sum(), (x * T.apply_AT(r, k)).sum()
            scale = np.abs(T.apply_A(x, k) * r).sum()
            print(f"{H}x{W} {f}: |<Ax, r> - <x, A^T r>| / sum|.| = {abs(a - b) / scale:.2e}")
            assert abs(a - b) <= 1e-13 * scale
            # A A^T = |k|^2 I
            assert np.abs(T.apply_A(T.apply_AT(r, k), k) - (k * k).sum() * r).max() <= 1e-15 * np.abs(r).max()
        p0, p1 = rng.standard_normal((2, H, W)), rng.standard_normal((2, H, W))
        g0, g1 = T.grad(x)
        c, d = (g0 * p0 + g1 * p1).sum(), -(x * T.div(p0, p1)).sum()
        scale = (np.abs(g0 * p0) + np.abs(g1 * p1)).sum()
        print(f"{H}x{W}: |<grad x, p> + <x, div p>| / sum|.| = {abs(c - d) / max(scale, 1e-300):.2e}")
        assert abs(c - d) <= 1e-13 * max(scale, 1e-300)
    # definitions by hand: a 2 x 3 image
    x = np.array([[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]])
    g0, g1 = T.grad(x)
    assert np.array_equal(g0, [[7, 14, 28], [0, 0, 0]]) and np.array_equal(g1, [[1, 2, 0], [8, 16, 0]])
    p0, p1 = np.array([[1.0, 2, 3], [9, 9, 9]]), np.array([[1.0, 5, 9], [2, 3, 9]])
    assert np.array_equal(T.div(p0, p1), [[1 + 1, 2 + 4, 3 - 5], [-1 + 2, -2 + 1, -3 - 3]])
    assert np.array_equal(T.apply_A(x, T.block_kernel("decimate", (2, 3))), [[1.0]])
    assert np.array_equal(T.apply_A(x[:, :2], T.block_kernel("mean", (1, 2))), [[1.5], [12.0]])
    assert np.array_equal(T.replicate(np.array([[1.0, 2.0]]), (2, 1)), [[1, 2], [1, 2]])
    assert T.huber(0.01, 0.02) == 0.01 ** 2 / 0.04 and T.huber(0.5, 0.02) == 0.49 and T.huber(0.5, 0.0) == 0.5


def test_restated_iteration_reaches_the_lbfgs_minimum_of_the_huber_energy():
    """The issue's case: 6 x 10, factors (3, 2), the mean kernel, weights with a missing datum, lambda 0.05, alpha 0.02."""
    hr, y = T.case_data()
    k = T.block_kernel("mean", T.CASE_FACTORS)
    minimum = T.lbfgs_minimum(y, k, T.CASE_LAM, T.CASE_ALPHA, T.CASE_W, hr.shape)
    gaps = {}
    for n in (100, 300):
        x, e, change = T.solve(y, T.CASE_FACTORS, "mean", T.CASE_LAM, T.CASE_ALPHA, n, T.CASE_W, return_info=True)
        gaps[n] = (e[0] - minimum) / minimum
        print(f"L-BFGS-B minimum {minimum:.12f}; {n} iterations: energy {e[0]:.12f}, relative gap {gaps[n]:.2e}, change {change[0]:.2e}")
    assert abs(minimum - 0.069759743610) <= 1e-11
    assert abs(gaps[300]) <= 1e-9
    assert 0 < gaps[100] <= 1e-5 and gaps[100] > abs(gaps[300])
    # lambda = 0 leaves the replication start where it is: it already satisfies the data
    x = T.solve(y, T.CASE_FACTORS, "mean", 0.0, 0.0, 50)
    assert np.abs(x - T.replicate(y, T.CASE_FACTORS)).max() <= 1e-15
