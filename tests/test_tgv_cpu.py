"""CPU: the second-order TGV solver of csrc/tgv.hip.  The float64 restatement the kernel is written from
(tests/tgv_common.py) against itself -- extended precision, the adjoint pair and the step bound, exact invariances, the TV energy it
cannot exceed, a bracket on the minimum from a smoothed problem that L-BFGS-B solves, the gain over first-order priors on the phantom
-- and the surface: header, exports, ctypes table, workspace plan, every refusal of the C entry points before device work with fake
pointers that are never dereferenced, and the refusals of the Python entry points and the drivers by name.  Every test prints what it
measured before it asserts."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import tgv_common as G
from tests import tvsr_common as T
from mri_super_resolution_amd import _lib, baselines, drivers, ops, reports
from mri_super_resolution_amd.scripts import second_order as so_script
from mri_super_resolution_amd.scripts import superresDWI as dwi_script
from mri_super_resolution_amd._build import LIB_PATH, SOURCE_FLAGS, SOURCES, build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("inr_tgv_workspace_doubles", "inr_tgv_solve2d", "inr_tgv_solve2d_f32")


# ---- the restatement against itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", (0.0, G.CASE_ALPHA), ids=("tv", "huber"))
def test_restated_iteration_in_float64_against_longdouble(alpha):
    """The weighted 6 x 10 (3, 2) case, 300 iterations: what float64 rounding alone moves.  It anchors the GPU bound of 1e-10: a kernel
    that follows the restatement in another valid operation order differs by this order of magnitude, six orders below the bound."""
    _, y = G.case_data()
    args = (y, G.CASE_FACTORS, "mean", G.CASE_LAM, 2.0, alpha, 300)
    x, v, e, c = G.solve(*args, w=G.CASE_W, return_info=True)
    xl, vl, el, cl = G.solve(*args, w=G.CASE_W, return_info=True, dtype=np.longdouble)
    dx, dv = float(np.abs(x - xl).max()), float(np.abs(v - vl).max())
    de, dc = float(np.abs(e - el).max() / el.max()), float(np.abs(c - cl).max())
    print(f"alpha {alpha}, 300 iterations, float64 against longdouble (eps {np.finfo(np.longdouble).eps:.1e}): max|x| diff {dx:.2e}, max|v| diff "
          f"{dv:.2e}, energy relative {de:.2e}, change {dc:.2e}")
    assert xl.dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18
    assert dx <= 1e-13 and dv <= 1e-13 and de <= 1e-13 and dc <= 1e-13


def test_adjoint_pair_and_the_step_bound():
    rng = np.random.default_rng(1)
    worst = 0.0
    for shape in ((16, 16), (5, 9), (1, 7), (7, 1)):
        z = [rng.standard_normal(shape) for _ in range(3)]
        d = [rng.standard_normal(shape) for _ in range(5)]
        Kz, KTd = G.K(*z), G.KT(*d)
        left = sum((a * b).sum() for a, b in zip(Kz[:4], d[:4])) + 2.0 * (Kz[4] * d[4]).sum()       # r01 counts twice
        right = sum((a * b).sum() for a, b in zip(z, KTd))
        scale = np.sqrt(sum((a * a).sum() for a in z) * sum((a * a).sum() for a in d))
        worst = max(worst, abs(left - right) / scale)
        print(f"{shape}: <K z, d> = {left:.12f}, <z, K^T d> = {right:.12f}, |difference| / (|z| |d|) = {abs(left - right) / scale:.2e}")
    assert worst <= 1e-12
    z = [rng.standard_normal((16, 16)) for _ in range(3)]
    for _ in range(500):
        d = G.K(*z)
        d = d[:4] + (d[4],)
        z = G.KT(*d)
        norm = np.sqrt(sum((a * a).sum() for a in z))
        z = [a / norm for a in z]
    print(f"power iteration on K^T K at 16 x 16: {norm:.4f} (bound 12; the 2 x 2 bound of the header comment is 11.37)")
    assert 8.0 < norm <= 12.0
    assert G.STEP * G.STEP * norm <= 1.0


def test_exact_invariances():
    rng = np.random.default_rng(2)
    x, v, e, c = G.solve(np.full((1, 5, 7), 0.7), (2, 2), "mean", 0.01, 2.0, 0.0, 50, return_info=True)
    print(f"constant 0.7, 50 iterations: max|x - 0.7| = {float(np.abs(x - 0.7).max())}, max|v| = {float(np.abs(v).max())}, energy {float(e[0])}, "
          f"change {float(c[0])}")
    assert np.array_equal(x, np.full((1, 10, 14), 0.7)) and not v.any() and float(c[0]) == 0.0
    y = rng.random((2, 5, 6))
    for n_iter in (1, 50):
        x, v, e, c = G.solve(y, (2, 2), "mean", 0.0, 2.0, 0.0, n_iter, return_info=True)
        print(f"lambda = 0, mean (2, 2), {n_iter} iterations: x == replication {np.array_equal(x, T.replicate(y, (2, 2)))}, energy "
              f"{float(e.max()):.1e}")
        assert np.array_equal(x, T.replicate(y, (2, 2))) and not v.any()


@pytest.mark.parametrize("alpha", (0.0, 0.02), ids=("tv", "huber"))
@pytest.mark.parametrize("ratio", (2.0, 0.5))
def test_tgv_energy_is_at_most_the_tv_energy(ratio, alpha):
    """(x_TV, 0) is feasible for the TGV problem, so its minimum is at most the TV minimum: no slack term."""
    k = T.block_kernel("mean", (2, 2))
    y = T.apply_A(np.random.default_rng(12).random((1, 12, 20)), k)
    x_tv = T.solve(y, (2, 2), "mean", 0.05, alpha, 4000)
    zero = np.zeros_like(x_tv)
    e_tv = float(G.energy(x_tv, zero, zero, y, k, 0.05, ratio, alpha)[0])
    for n_iter in (300, 1000):
        _, _, e, _ = G.solve(y, (2, 2), "mean", 0.05, ratio, alpha, n_iter, return_info=True)
        print(f"ratio {ratio}, alpha {alpha}: TGV energy after {n_iter} iterations {float(e[0]):.10f}, E(x_TV, 0) after 4,000 {e_tv:.10f}, "
              f"TGV / TV = {float(e[0]) / e_tv:.5f}")
    assert e_tv == float(T.energy(x_tv, y, k, 0.05, alpha)[0])
    assert float(e[0]) <= e_tv


BRACKET_EPS, BRACKET_ITERS, BRACKET_GAP = 1e-5, 10000, 5e-6


def test_energy_lies_in_the_bracket_of_the_smoothed_problem():
    """With lam0 |Ev|_F replaced by lam0 H_eps(|Ev|_F) the energy is smooth and convex, and t - eps / 2 <= H_eps(t) <= t puts the true
    minimum in [m_eps, m_eps + lam0 H W eps / 2].  eps = 1e-5 makes that 3e-5 wide on the 6 x 10 case (5e-4 of the energy).  Below,
    the interval is widened by the L-BFGS-B residual |gradient|_1 |z* - z|_inf with |z* - z|_inf <= 0.1 (the data are in [0, 1]);
    above, by the convergence gap of 10,000 iterations: the energy falls by 1.5e-6 from 10,000 to 40,000 iterations, which at the
    O(1 / N) rate of the method leaves 2e-6 to the limit, and 5e-6 is taken.  Measured: m_eps = 0.058737871, the energy 0.058759370
    sits at 0.72 of the interval.  One flipped sign in any div term of the v update sends the energy above 600 within 3,000
    iterations, and a flipped sign in div(p) gives 0.61: both far outside."""
    _, y = G.case_data()
    k = T.block_kernel("mean", G.CASE_FACTORS)
    ratio = 2.0
    m, g1 = G.tgv_lbfgs_minimum(y[0], k, G.CASE_LAM, ratio, G.CASE_ALPHA, BRACKET_EPS, G.CASE_W[0], (6, 10))
    low = m - 0.1 * g1
    high = m + ratio * G.CASE_LAM * 60 * BRACKET_EPS / 2 + BRACKET_GAP
    _, _, e, change = G.solve(y, G.CASE_FACTORS, "mean", G.CASE_LAM, ratio, G.CASE_ALPHA, BRACKET_ITERS, w=G.CASE_W, return_info=True)
    e = float(e[0])
    print(f"eps {BRACKET_EPS}: m_eps {m:.12f}, |gradient|_1 {g1:.2e}; bracket [{low:.12f}, {high:.12f}]; energy after {BRACKET_ITERS} iterations "
          f"{e:.12f}, at {(e - m) / (ratio * G.CASE_LAM * 60 * BRACKET_EPS / 2):.3f} of the unwidened interval; change {float(change[0]):.1e}")
    assert g1 <= 1e-4
    assert low <= e <= high


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_the_gain_over_first_order_on_the_phantom(seed):
    hr, lr = G.phantom_data(seed)
    x = G.solve(lr, (2, 2), "mean", 0.01, 4.0, 0.0, 300)
    tv = {(lam, a): G.rmse(T.solve(lr, (2, 2), "mean", lam, a, 300), hr) for lam, a in ((0.005, 0.0), (0.0075, 0.0), (0.01, 0.0), (0.01, 0.03))}
    best, r = min(tv.values()), G.rmse(x, hr)
    print(f"phantom, seed {seed}: TGV (0.01, ratio 4) RMSE {r:.5f}; TV {', '.join(f'{k}: {v:.5f}' for k, v in tv.items())}; ratio to the best "
          f"{r / best:.3f} (bound 0.9); flat-area index: HR {G.flat_share(hr):.3f}, TGV {G.flat_share(x):.3f}, TV 0.0075 "
          f"{G.flat_share(T.solve(lr, (2, 2), 'mean', 0.0075, 0.0, 300)):.3f}")
    assert hr.shape == (48, 48) and lr.shape == (24, 24) and hr.max() == 1.0
    assert r <= 0.9 * best


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_ctypes_table_carry_the_symbols():
    text = open(os.path.join(ROOT, "include", "inrhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(inr_[a-z0-9_]+)\s*\(", code))
    build_library()
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(handle, name) and name in _lib.SIGNATURES, name
    assert sorted(k for k in _lib.SIGNATURES if k.startswith("inr_tgv_")) == sorted(NEW)
    assert "tgv.hip" in SOURCES and "-ffp-contract=off" in SOURCE_FLAGS["tgv.hip"]
    for name in ("tgv_solve", "tgv_workspace_doubles"):
        assert callable(getattr(ops, name))
    assert callable(baselines.tgv_superres) and callable(drivers.second_order_study) and callable(drivers.check_second_order)
    assert reports.SSIM_TV_TGV_HEADER == "Pt_id, b-value, slice, SSIM-tv-tgv, SSIM-SR\n"
    src = open(os.path.join(ROOT, "mri-super-resolution_amd", "csrc", "tgv.hip")).read()
    assert '#include "tv_block.h"' in src and "int tv_shape_check(" not in src and "atomic" not in src.split("#include")[1]
    assert src.count("__syncthreads();   // barrier") == 2
    # the phantom of the driver is the phantom of the tests
    assert np.array_equal(drivers.second_order_phantom(), G.phantom())


def test_the_family_has_one_definition_of_what_it_shares():
    """the Huber function, the floor division, the stride-loop grids, the parameter refusals and the finish kernel
    live once in tv_shared.h, the phases of the three single-workgroup kernels once in tv_block.h, and no unit keeps a copy."""
    csrc = os.path.join(ROOT, "mri-super-resolution_amd", "csrc")
    read = lambda name: open(os.path.join(csrc, name)).read()
    shared, block = read("tv_shared.h"), read("tv_block.h")
    units = {name: read(name) for name in ("tvsr.hip", "tvsr3d.hip", "tvmf.hip", "tvms.hip", "tvop.hip", "tvj.hip", "tgv.hip")}
    for name in ("tvsr3d.hip", "tvms.hip", "tvop.hip"):
        assert '#include "tv_shared.h"' in units[name], name
    for name in ("tvsr.hip", "tvj.hip", "tgv.hip", "tvmf.hip"):          # through tv_block.h, whose checks tvmf.hip calls
        assert '#include "tv_block.h"' in units[name], name
    assert '#include "tv_shared.h"' in block
    for text in ("double tv_huber(", "int tv_floordiv(", "unsigned tv_grid(", "unsigned tv_thread_grid(", "double block_max_f64(",
                 "int tv_params_check(", "int tv_grad_weights_check(", "double tv_grad_weight_sum(", "TvStateView tv_state_view(",
                 " tv_finish_kernel("):
        assert shared.count(text) == 1 and text not in block, text
    for text in ("void tv_start_pixel(", "void tv_primal_block(", "void tv_add_data_term(", "void tv_store_energy_change(",
                 "int tv_shape_check(", "int tv_block_check(", "unsigned tv_pixel_grid("):
        assert block.count(text) == 1 and text not in shared, text
    # the phase helpers hold no barrier: the only ones of tv_block.h are the four of the reduction after the iterations
    phases = block.split("void tv_store_energy_change(")[0]
    assert "__syncthreads" not in re.sub(r"//.*", "", phases) and block.count("__syncthreads();") == 4
    for name, src in units.items():
        code = re.sub(r"//.*", "", src)
        assert not re.search(r"\bdouble\s+\w*huber\w*\s*\(", code), name                     # no Huber function of its own
        assert not re.search(r"\bunsigned\s+\w*grid\w*\s*\(", code), name                    # no *_grid
        assert not re.search(r"\bint\s+\w*floordiv\w*\s*\(", code), name                     # no *_floordiv
        assert not re.search(r"\w*finish_kernel\s*\(\s*double", code), name                  # no *_finish_kernel
        assert not re.search(r"\bdouble\s+\w*block_max\w*\s*\(", code) and "fmax(fmax(red[0]" not in code, name
        assert "n_iter must be" not in src and "lambda must be finite" not in src and "alpha must be finite" not in src, name
        assert not re.search(r"struct\s+\w*View\s*\{\s*double\s*\*\s*state;\s*size_t total;", code), name
    for name in ("tvsr.hip", "tvj.hip", "tgv.hip"):
        # the shared phases are called, the loops and the two barriers of an iteration stay in the unit
        for call in ("tv_start_pixel(", "tv_primal_block(", "tv_add_data_term(", "tv_store_energy_change("):
            assert units[name].count(call) == 1, (name, call)
        assert units[name].count("__syncthreads();   // barrier") == 2, name
    for name in ("tvsr3d.hip", "tvmf.hip", "tvms.hip", "tvop.hip"):
        assert units[name].count("tv_finish<") == 1 and units[name].count("tv_params_check(") == 1, name


def test_workspace_plan():
    plan = _lib.lib().inr_tgv_workspace_doubles
    # x | xbar | v0 | v1 | vbar0 | vbar1 | p0 | p1 | r00 | r11 | r01 of every image, nothing else
    assert plan(1, 6, 10) == 11 * 60 and plan(300, 12, 12) == 300 * 11 * 144 and plan(2, 7, 1024) == 2 * 11 * 7 * 1024
    assert plan(1, 1024, 1024) == 11 << 20 and plan(65536, 1024, 1024) == 11 << 36
    assert plan(0, 8, 8) == plan(1, 8, 8) > 0
    err = _lib.lib().inr_last_error
    assert plan(-1, 8, 8) == 0 and b"inr_tgv_workspace_doubles" in err() and b"bad sizes (n_images" in err()
    assert plan(1, 0, 8) == 0 and b"bad sizes" in err()
    assert plan(1, 8, 1025) == 0 and b"bad sizes" in err()
    assert ops.tgv_workspace_doubles(2, 50, 50) == 2 * 11 * 2500


def test_every_refusal_comes_before_device_work():
    lib = _lib.lib()
    fake = lambda k: ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)      # never dereferenced: every call fails in validation
    err = lib.inr_last_error
    K = lambda *v: (ctypes.c_double * len(v))(*v)
    mean6, nan, inf = K(*([1 / 6] * 6)), float("nan"), float("inf")
    need = lib.inr_tgv_workspace_doubles(2, 6, 10)
    INV, WS, AL = _lib.INR_E_INVALID, _lib.INR_E_WORKSPACE, _lib.INR_E_ALIGN
    names = ("out", "v_out", "energy", "change", "y", "weight", "x0", "n", "H", "W", "f0", "f1", "kernel", "lam", "ratio", "alpha", "n_iter", "ws",
             "doubles", "stream")
    for call in (lib.inr_tgv_solve2d, lib.inr_tgv_solve2d_f32):
        who = call.__name__.encode()
        ok = [fake(0), fake(5), fake(1), fake(2), fake(3), None, None, 2, 6, 10, 3, 2, mean6, 0.05, 2.0, 0.02, 10, fake(4), need, None]

        def bad(code, text, **change):
            args = [change.get(name, value) for name, value in zip(names, ok)]
            assert call(*args) == code, (change, err())
            assert text in err() and who in err(), (change, err())

        bad(INV, b"null pointer", out=None)
        bad(INV, b"null pointer", y=None)
        bad(INV, b"null pointer (kernel)", kernel=None)
        bad(INV, b"bad sizes (n_images = -1)", n=-1)
        bad(INV, b"block factors are 1 .. 8", f0=0)
        bad(INV, b"block factors are 1 .. 8", f1=9)
        bad(INV, b"bad sizes (HR images", H=0)
        bad(INV, b"bad sizes (HR images", W=1026)
        bad(INV, b"no whole number of 3 x 2 blocks", H=7)
        bad(INV, b"no whole number of 3 x 2 blocks", W=11)
        bad(INV, b"n_iter must be >= 0 (got -1)", n_iter=-1)
        for name, text in (("lam", b"lambda must be finite and >= 0"), ("alpha", b"alpha must be finite and >= 0")):
            for value in (-1e-3, nan, inf):
                bad(INV, text, **{name: value})
        for value in (0.0, -1.0, nan, inf):
            bad(INV, b"ratio must be finite and > 0", ratio=value)
        bad(INV, b"ratio must be finite and > 0", ratio=0.0, lam=0.0)            # checked whatever lambda is
        bad(INV, b"block kernel must be finite", kernel=K(0.5, nan, 0.5, 0, 0, 0))
        bad(INV, b"block kernel must sum to 1", kernel=K(*([0.5] * 6)))
        bad(WS, b"workspace too small", doubles=need - 1)
        bad(WS, b"workspace too small", ws=None)
        bad(AL, b"16-byte aligned", ws=ctypes.c_void_p(0x7000_0000_0008))
        # n_images = 0 succeeds and launches nothing; v_out, energy and change are optional
        zero = list(ok)
        zero[7] = 0
        assert call(*zero) == 0
        zero[1] = zero[2] = zero[3] = None
        assert call(*zero) == 0


def test_python_entry_points_refuse_by_name():
    lr = np.ones((3, 5, 5))
    fn = baselines.tgv_superres
    with pytest.raises(TypeError, match="tgv_superres takes an ndarray or a device tensor.*list"):
        fn([[1.0, 2.0], [3.0, 4.0]], (1, 1))
    with pytest.raises(ops.InrDeviceError, match="tgv_superres.*no CPU fallback"):
        fn(torch.ones(2, 4, 4), (2, 2))
    with pytest.raises(ValueError, match="tgv_superres needs at least 2-D input"):
        fn(np.ones(4), (2, 2))
    with pytest.raises(ValueError, match="tgv_superres: kernel must be 'mean', 'decimate' or an array.*'box'"):
        fn(lr, (2, 2), kernel="box")
    with pytest.raises(ValueError, match="tgv_superres: factors are 1 .. 8 per axis.*9 x 1"):
        fn(lr, (9, 1))
    with pytest.raises(ValueError, match="tgv_superres: HR images of 1 .. 1024"):
        fn(np.ones((2, 300, 4)), (4, 1))
    for kw, text in (({"lam": -1.0}, "lam must be finite and >= 0"), ({"lam": float("nan")}, "lam must be finite"),
                     ({"ratio": 0.0}, "ratio must be finite and > 0"), ({"ratio": -2.0}, "ratio must be finite and > 0"),
                     ({"ratio": float("inf")}, "ratio must be finite"), ({"ratio": float("nan")}, "ratio must be finite"),
                     ({"huber": -0.1}, "huber must be finite and >= 0"), ({"huber": float("inf")}, "huber must be finite"),
                     ({"n_iter": -1}, "n_iter must be an integer >= 0"), ({"n_iter": 2.5}, "n_iter must be an integer")):
        with pytest.raises(ValueError, match=f"tgv_superres: {text}"):
            fn(lr, (2, 2), **kw)
    with pytest.raises(TypeError, match="tgv_superres: weight must be given like lr"):
        fn(lr, (2, 2), weight=torch.ones(3, 5, 5))
    with pytest.raises(ValueError, match="tgv_superres: weight must be finite and >= 0"):
        fn(lr, (2, 2), weight=-lr)
    with pytest.raises(ValueError, match="tgv_superres: x0 must have shape \\(3, 10, 10\\)"):
        fn(lr, (2, 2), x0=np.ones((10, 10)))
    # ops.tgv_solve takes device tensors only
    with pytest.raises(ops.InrDeviceError, match="y is on cpu"):
        ops.tgv_solve(torch.ones(1, 4, 4, dtype=torch.float64), (2, 2), [[0.25, 0.25], [0.25, 0.25]], 0.01, 2.0, 0.0, 3)
    with pytest.raises(TypeError, match="y must be a torch.Tensor"):
        ops.tgv_solve(np.ones((1, 4, 4)), (2, 2), [[0.25, 0.25], [0.25, 0.25]], 0.01, 2.0, 0.0, 3)
    # the defaults are the ones the drivers' flags carry
    args = dwi_script.build_parser().parse_args(["--data", "x.mat"])
    assert args.tv_tgv is False and (args.tv_tgv_lambda, args.tv_tgv_ratio) == (baselines.TGV_DEFAULT_LAMBDA, baselines.TGV_DEFAULT_RATIO)
    args = so_script.build_parser().parse_args(["--phantom"])
    assert (args.tv_lambda, args.tv_huber, args.tgv_lambda, args.tgv_ratio, args.tgv_huber, args.iters) == (
        baselines.TV_DEFAULT_LAMBDA, baselines.TV_DEFAULT_HUBER, baselines.TGV_DEFAULT_LAMBDA, baselines.TGV_DEFAULT_RATIO,
        baselines.TGV_DEFAULT_HUBER, baselines.TGV_DEFAULT_ITERS)
    # and they are the sweep's (tools/tgv_sweep.py)
    assert (baselines.TGV_DEFAULT_LAMBDA, baselines.TGV_DEFAULT_RATIO, baselines.TGV_DEFAULT_HUBER, baselines.TGV_DEFAULT_ITERS) == (
        0.005, 0.5, 0.0, 300)


def test_superresDWI_refuses_the_tgv_flags_before_the_input_is_loaded(tmp_path):
    missing = str(tmp_path / "pat03_not_there.mat")        # never opened: every refusal comes first
    run = lambda *flags: dwi_script.main(["--data", missing, "--output_address", str(tmp_path / "res"), "--roi_start", "2", "--roi_end",
                                          "18", *flags])
    with pytest.raises(ValueError, match="--tv_tgv is scored beside the first-order reconstruction: pass --tv_baseline"):
        run("--tv_tgv")
    with pytest.raises(ValueError, match="--tv_tgv_lambda must be finite and >= 0.*-0.001"):
        run("--tv_baseline", "--tv_tgv", "--tv_tgv_lambda", "-0.001")
    with pytest.raises(ValueError, match="--tv_tgv_lambda must be finite"):
        run("--tv_baseline", "--tv_tgv", "--tv_tgv_lambda", "nan")
    for value in ("0", "-1", "inf", "nan"):
        with pytest.raises(ValueError, match="--tv_tgv_ratio must be finite and > 0"):
            run("--tv_baseline", "--tv_tgv", "--tv_tgv_ratio", value)
    with pytest.raises(ValueError, match="--tv_iters must be 1 .. 100,000"):
        run("--tv_baseline", "--tv_tgv", "--tv_iters", "0")
    # without --tv_tgv its values are not looked at: the run gets as far as the missing input
    with pytest.raises((OSError, ValueError), match="not_there"):
        run("--tv_baseline", "--tv_tgv_ratio", "-1")
    with pytest.raises((OSError, ValueError), match="not_there"):
        run("--tv_baseline", "--tv_tgv")


def test_second_order_study_refuses_by_name(tmp_path):
    ok = dict(rows=48, cols=48, factor=2, kernel="mean", noise=0.02, tv_lambda=3e-3, tv_huber=0.0, tgv_lambda=0.01, tgv_ratio=2.0,
              tgv_huber=0.0, iters=300)
    assert drivers.check_second_order(**ok) == (24, 24) and drivers.check_second_order() == (24, 24)
    for change, text in (({"rows": 1}, "the HR image has 2 .. 1024 rows"), ({"cols": 1025}, "the HR image has 2 .. 1024 cols"),
                         ({"factor": 0}, "factor is 1 .. 8"), ({"factor": 5}, "factor is 1 .. 8 and divides the HR sides 48 x 48"),
                         ({"factor": 9}, "factor is 1 .. 8"), ({"kernel": "box"}, "kernel must be 'mean' or 'decimate'"),
                         ({"noise": -0.1}, "noise must be finite and >= 0"), ({"tv_lambda": -1.0}, "tv_lambda must be finite and >= 0"),
                         ({"tgv_lambda": float("nan")}, "tgv_lambda must be finite and >= 0"),
                         ({"tv_huber": float("inf")}, "tv_huber must be finite and >= 0"), ({"tgv_huber": -1.0}, "tgv_huber must be finite"),
                         ({"tgv_ratio": 0.0}, "tgv_ratio must be finite and > 0"), ({"tgv_ratio": float("nan")}, "tgv_ratio must be finite"),
                         ({"iters": 0}, "iters must be 1 .. 100,000"), ({"iters": 100001}, "iters must be 1 .. 100,000")):
        with pytest.raises(ValueError, match=f"second_order_study: {text}"):
            drivers.check_second_order(**{**ok, **change})
    with pytest.raises(ValueError, match="second_order_study: hr is \\[Z, H, W\\]"):
        drivers.second_order_study(np.ones((48, 48)))
    with pytest.raises(ValueError, match="second_order_study: slice_ids are one index >= 0 per slice"):
        drivers.second_order_study(np.ones((2, 8, 8)), slice_ids=[0])
    # the script checks its flags before it opens the input
    missing = str(tmp_path / "pat03_not_there.mat")
    run = lambda *flags: so_script.main(["--output_address", str(tmp_path / "res"), *flags])
    with pytest.raises(ValueError, match="--data FILE ... or --phantom, one of the two"):
        run()
    with pytest.raises(ValueError, match="--data FILE ... or --phantom, one of the two"):
        run("--phantom", "--data", missing)
    with pytest.raises(ValueError, match="second_order_study: factor is 1 .. 8 and divides the HR sides 50 x 50"):
        run("--data", missing, "--factor", "3")
    with pytest.raises(ValueError, match="second_order_study: tgv_ratio must be finite and > 0"):
        run("--phantom", "--tgv_ratio", "0")
    with pytest.raises(ValueError, match="ROI 30:20"):
        run("--data", missing, "--roi_start", "30", "--roi_end", "20")
    with pytest.raises(ValueError, match="--slices are indexes >= 0"):
        run("--phantom", "--slices", "-1")
    with pytest.raises(ValueError, match="the phantom is one slice"):
        run("--phantom", "--slices", "0", "1")
    with pytest.raises((OSError, ValueError), match="not_there"):
        run("--data", missing)
    # the flat-area index is the one of the tests (CPU tensors: plain torch arithmetic)
    img = torch.from_numpy(np.random.default_rng(3).random((2, 9, 7)) * 2e-3)
    assert np.array_equal(drivers.flat_area_index(img).numpy(), [G.flat_share(img[0].numpy()), G.flat_share(img[1].numpy())])
