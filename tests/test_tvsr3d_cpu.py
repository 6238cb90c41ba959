"""CPU: the surface of the 3-D TV / Huber solver (header, exports, ctypes table, workspace plan, every refusal of csrc/tvsr3d.hip
before device work with fake pointers that are never dereferenced, the refusals of the Python entry points and of the through-plane
study's flags) and the float64 restatement the kernels are written from (tests/tvsr3d_common.py): the adjoint pairs, the minimum of
the Huber energy found by L-BFGS-B, which shares nothing with the iteration, and the bits of the 2-D restatement where the slices do
not couple."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import tvsr3d_common as T
from tests import tvsr_common as T2
from mri_super_resolution_amd import _lib, baselines, drivers, ops
from mri_super_resolution_amd.scripts import through_plane as tp_script
from mri_super_resolution_amd._build import LIB_PATH, SOURCE_FLAGS, SOURCES, build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("inr_tvsr3d_block_apply", "inr_tvsr3d_block_adjoint", "inr_tvsr3d_workspace_doubles", "inr_tvsr3d_solve", "inr_tvsr3d_solve_f32")


def test_header_library_and_ctypes_table_carry_the_symbols():
    text = open(os.path.join(ROOT, "include", "inrhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(inr_[a-z0-9_]+)\s*\(", code))
    build_library()
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(handle, name) and name in _lib.SIGNATURES, name
    assert sorted(k for k in _lib.SIGNATURES if k.startswith("inr_tvsr3d_")) == sorted(NEW)
    assert "tvsr3d.hip" in SOURCES and "-ffp-contract=off" in SOURCE_FLAGS["tvsr3d.hip"]
    assert int(re.search(r"#define INR_TVSR3D_MAX_ITER (\d+)", text).group(1)) == _lib.INR_TVSR3D_MAX_ITER == 100000
    for name in ("tv_superres3d", "block_apply3d", "block_adjoint3d", "slice_profile"):
        assert callable(getattr(baselines, name))
    for name in ("tvsr_solve3d", "tvsr3d_workspace_doubles", "block_apply3d", "block_adjoint3d"):
        assert callable(getattr(ops, name))
    assert callable(drivers.through_plane_study)
    # the entry points are defined in the unit that owns the kernels
    unit = open(os.path.join(ROOT, "mri-super-resolution_amd", "csrc", "tvsr3d.hip")).read()
    for name in NEW:
        assert re.search(rf"\b{name}\(", unit), name


def test_workspace_plan():
    plan = _lib.lib().inr_tvsr3d_workspace_doubles
    err = _lib.lib().inr_last_error
    # x | xbar | p0 | p1 | p2 of every volume, then the partials of energy and change: at most 2 x 1,024 (+ padding) per volume
    for n, D, H, W, f in ((1, 4, 6, 6, (2, 3, 2)), (40, 4, 6, 6, (2, 3, 2)), (1, 28, 50, 50, (2, 1, 1)), (2, 5, 7, 1024, (5, 7, 1)),
                          (1, 56, 256, 256, (2, 1, 1)), (1, 1024, 1024, 1024, (8, 8, 8))):
        got = plan(n, D, H, W, *f)
        print(f"{n} x {D}x{H}x{W} by {f}: {got} doubles, state {5 * n * D * H * W}")
        assert 5 * n * D * H * W < got <= 5 * n * D * H * W + n * 2 * 1024 + 4
    assert plan(1, 4, 6, 6, 2, 3, 2) == 5 * 144 + 2 + 2                     # one tile per LR slice: two parts
    assert plan(0, 4, 6, 6, 2, 3, 2) == plan(1, 4, 6, 6, 2, 3, 2) > 0
    sizes = [plan(n, 8, 16, 16, 2, 2, 2) for n in (1, 2, 3, 10, 100)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)         # monotone in n
    assert plan(3, 8, 16, 16, 2, 2, 2) == 3 * plan(1, 8, 16, 16, 2, 2, 2)
    for args, text in (((-1, 8, 8, 8, 1, 1, 1), b"bad sizes"), ((1, 0, 8, 8, 1, 1, 1), b"bad sizes"), ((1, 8, 8, 1025, 1, 1, 1), b"bad sizes"),
                       ((1, 1025, 8, 8, 1, 1, 1), b"bad sizes"), ((1, 8, 8, 8, 0, 1, 1), b"block factors"),
                       ((1, 8, 8, 8, 1, 9, 1), b"block factors"), ((1, 8, 8, 8, 3, 1, 1), b"no whole number")):
        assert plan(*args) == 0 and b"inr_tvsr3d_workspace_doubles" in err() and text in err(), (args, err())
    assert ops.tvsr3d_workspace_doubles(1, 4, 6, 6, (2, 3, 2)) == 724


def test_every_refusal_comes_before_device_work():
    lib = _lib.lib()
    fake = lambda k: ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)      # never dereferenced: every call fails in validation
    err = lib.inr_last_error
    K = lambda *v: (ctypes.c_double * len(v))(*v)
    nan, inf = float("nan"), float("inf")
    need = lib.inr_tvsr3d_workspace_doubles(2, 4, 6, 6, 2, 3, 2)
    INV, WS, AL = _lib.INR_E_INVALID, _lib.INR_E_WORKSPACE, _lib.INR_E_ALIGN
    names = ("out", "energy", "change", "y", "weight", "x0", "n", "D", "H", "W", "f0", "f1", "f2", "k0", "k1", "k2", "g", "lam", "alpha",
             "n_iter", "ws", "doubles", "stream")
    for call in (lib.inr_tvsr3d_solve, lib.inr_tvsr3d_solve_f32):
        who = call.__name__.encode()
        ok = [fake(0), fake(1), fake(2), fake(3), None, None, 2, 4, 6, 6, 2, 3, 2, K(0.25, 0.75), K(*[1 / 3] * 3), K(0.2, 0.8),
              K(0.4, 1, 1), 0.05, 0.02, 10, fake(4), need, None]

        def bad(code, text, **change):
            args = [change.get(name, value) for name, value in zip(names, ok)]
            assert call(*args) == code, (change, err())
            assert text in err() and who in err(), (change, err())

        bad(INV, b"null pointer", out=None)
        bad(INV, b"null pointer", y=None)
        for name in ("k0", "k1", "k2"):
            bad(INV, b"null pointer (kernel factors)", **{name: None})
        bad(INV, b"null pointer (grad_weights)", g=None)
        bad(INV, b"bad sizes (n_volumes", n=-1)
        bad(INV, b"block factors are 1 .. 8", f0=0)
        bad(INV, b"block factors are 1 .. 8", f2=9)
        bad(INV, b"bad sizes (HR volumes", D=0)
        bad(INV, b"bad sizes (HR volumes", W=1026)
        bad(INV, b"no whole number of 2 x 3 x 2 blocks", D=5)
        bad(INV, b"no whole number of 2 x 3 x 2 blocks", H=7)
        bad(INV, b"no whole number of 2 x 3 x 2 blocks", W=7)
        bad(INV, b"n_iter must be 0 .. 100000", n_iter=-1)
        bad(INV, b"n_iter must be 0 .. 100000", n_iter=100001)
        for name, text in (("lam", b"lambda must be finite and >= 0"), ("alpha", b"alpha must be finite and >= 0")):
            for value in (-1e-3, nan, inf):
                bad(INV, text, **{name: value})
        for g in (K(-0.1, 1, 1), K(1, nan, 1), K(1, 1, inf)):
            bad(INV, b"gradient weights must be finite and >= 0", g=g)
        bad(INV, b"kernel factors must be finite (k0[1]", k0=K(0.5, nan))
        bad(INV, b"kernel factors must be finite (k2[0]", k2=K(inf, -inf))
        bad(INV, b"every kernel factor must sum to 1 (k1", k1=K(0.5, 0.5, 0.5))
        bad(INV, b"every kernel factor must sum to 1 (k0", k0=K(-1, 0))
        bad(WS, b"workspace too small", doubles=need - 1)
        bad(WS, b"workspace too small", ws=None)
        bad(AL, b"16-byte aligned", ws=ctypes.c_void_p(0x7000_0000_0008))
        # n_volumes = 0 succeeds and launches nothing; energy and change are optional; n_iter = 100,000 is not refused for its size
        zero = list(ok)
        zero[6] = 0
        assert call(*zero) == 0
        zero[1] = zero[2] = None
        zero[19] = 100000
        assert call(*zero) == 0
    for call in (lib.inr_tvsr3d_block_apply, lib.inr_tvsr3d_block_adjoint):
        who = call.__name__.encode()
        ok = [fake(0), fake(1), 2, 4, 6, 6, 2, 3, 2, K(0.25, 0.75), K(*[1 / 3] * 3), K(0.2, 0.8), None]
        sub = lambda i, v: ok[:i] + [v] + ok[i + 1:]
        for args, text in ((sub(0, None), b"null pointer"), (sub(1, None), b"null pointer"), (sub(10, None), b"null pointer (kernel factors)"),
                           (sub(2, -1), b"bad sizes"), (sub(3, 5), b"no whole number"), (sub(5, 2048), b"bad sizes"),
                           (sub(7, 9), b"block factors"), (sub(11, K(1, 1)), b"sum to 1"), (sub(9, K(nan, 0)), b"finite")):
            assert call(*args) == INV and text in err() and who in err(), (args, err())
        assert call(*sub(2, 0)) == 0


def test_python_entry_points_refuse_by_name():
    v = np.ones((4, 4, 4))
    for name, fn in (("tv_superres3d", baselines.tv_superres3d), ("block_apply3d", baselines.block_apply3d),
                     ("block_adjoint3d", baselines.block_adjoint3d)):
        with pytest.raises(TypeError, match=f"{name} takes an ndarray or a device tensor.*list"):
            fn([[[1.0, 2.0]]], (1, 1, 1))
        with pytest.raises(ops.InrDeviceError, match=f"{name}.*no CPU fallback"):
            fn(torch.ones(4, 4, 4), (2, 2, 2))
        with pytest.raises(ValueError, match=f"{name}: kernel must be 'mean', 'decimate' or a triple.*'box'"):
            fn(v, (2, 2, 2), kernel="box")
        with pytest.raises(ValueError, match=f"{name}: factors are 1 .. 8 per axis.*9 x 1 x 1"):
            fn(np.ones((9, 4, 4)), (9, 1, 1))
        with pytest.raises(ValueError, match=f"{name}: factors are \\(f0, f1, f2\\)"):
            fn(v, (2, 2))
        with pytest.raises(ValueError, match=f"{name}: factors are \\(f0, f1, f2\\)"):
            fn(v, 2)
        with pytest.raises(ValueError, match=f"{name}: the kernel factors must be 1-D arrays of 2, 2 and 2 entries"):
            fn(v, (2, 2, 2), kernel=(np.ones(2) / 2, np.ones(3) / 3, np.ones(2) / 2))
        with pytest.raises(ValueError, match=f"{name}: kernel factor k1 must be finite and sum to 1"):
            fn(v, (2, 2, 2), kernel=(np.ones(2) / 2, np.ones(2), np.ones(2) / 2))
        with pytest.raises(ValueError, match=f"{name} needs at least 3-D"):
            fn(np.ones((4, 4)), (2, 2, 2))
    with pytest.raises(ValueError, match="block_apply3d: the HR volume 4 x 4 x 4 is no whole number of 1 x 3 x 1 blocks"):
        baselines.block_apply3d(v, (1, 3, 1))
    with pytest.raises(ValueError, match="tv_superres3d: HR volumes of 1 .. 1024"):
        baselines.tv_superres3d(np.ones((300, 2, 2)), (4, 1, 1))
    with pytest.raises(ValueError, match="block_adjoint3d: HR volumes of 1 .. 1024"):
        baselines.block_adjoint3d(np.ones((2, 2, 600)), (1, 1, 2))
    for kw, text in (({"lam": -1.0}, "lam must be finite and >= 0"), ({"lam": float("nan")}, "lam must be finite"),
                     ({"huber": -0.1}, "huber must be finite and >= 0"), ({"huber": float("inf")}, "huber must be finite"),
                     ({"n_iter": -1}, "n_iter must be an integer 0 .. 100000"), ({"n_iter": 2.5}, "n_iter must be an integer"),
                     ({"n_iter": 100001}, "n_iter must be an integer 0 .. 100000"),
                     ({"grad_weights": (1.0, 1.0)}, "grad_weights are \\(g0, g1, g2\\)"),
                     ({"grad_weights": (1.0, -1.0, 1.0)}, "grad_weights are \\(g0, g1, g2\\), finite and >= 0"),
                     ({"grad_weights": 1.0}, "grad_weights are")):
        with pytest.raises(ValueError, match=f"tv_superres3d: {text}"):
            baselines.tv_superres3d(v, (2, 2, 2), **kw)
    with pytest.raises(TypeError, match="tv_superres3d: weight must be given like lr"):
        baselines.tv_superres3d(v, (2, 2, 2), weight=torch.ones(4, 4, 4))
    with pytest.raises(ValueError, match="tv_superres3d: x0 must have shape \\(8, 8, 8\\)"):
        baselines.tv_superres3d(v, (2, 2, 2), x0=np.ones((4, 4, 4)))
    with pytest.raises(ValueError, match="tv_superres3d: weight must be finite and >= 0"):
        baselines.tv_superres3d(v, (2, 2, 2), weight=-v)
    assert (baselines.TV3D_DEFAULT_LAMBDA, baselines.TV3D_DEFAULT_HUBER, baselines.TV3D_DEFAULT_ITERS) == (3e-3, 0.1, 300)
    assert baselines.TV3D_DEFAULT_GRAD_WEIGHTS == (1.0, 1.0, 1.0)
    # the 2-D entry points keep their defaults
    assert (baselines.TV_DEFAULT_LAMBDA, baselines.TV_DEFAULT_HUBER, baselines.TV_DEFAULT_ITERS) == (3e-3, 0.3, 300)


def test_slice_profile_sums_symmetry_and_refusals():
    for f in range(1, 9):
        for kind, fwhm in (("mean", None), ("decimate", None), ("gaussian", 0.3), ("gaussian", 1.0), ("gaussian", 2.5)):
            k = baselines.slice_profile(f, kind, fwhm)
            assert k.shape == (f,) and k.dtype == np.float64 and abs(k.sum() - 1.0) <= 1e-15 and (k >= 0).all()
            assert np.array_equal(k, T.slice_profile(f, kind, fwhm))
            if kind != "decimate":
                assert np.abs(k - k[::-1]).max() <= 1e-16                   # symmetric about the thick slice's centre
            if kind == "gaussian" and f > 2:
                assert k[f // 2] == k.max() and k[0] == k.min()
    assert np.array_equal(baselines.slice_profile(4), [0.25] * 4) and np.array_equal(baselines.slice_profile(3, "decimate"), [1, 0, 0])
    # FWHM in thick slices: at f = 2 the samples sit at -1/4 and +1/4 of a thick slice, whatever the width
    assert np.array_equal(baselines.slice_profile(2, "gaussian", 0.5), [0.5, 0.5])
    # a wide Gaussian is the mean; the definition: half the maximum at fwhm / 2 from the centre, samples at (a + 1/2) / f - 1/2
    assert np.abs(baselines.slice_profile(8, "gaussian", 100.0) - 0.125).max() <= 1e-5
    fw = 0.5
    pos = (np.arange(8) + 0.5) / 8 - 0.5
    want = np.exp(-4 * np.log(2) * (pos / fw) ** 2)
    assert np.abs(baselines.slice_profile(8, "gaussian", fw) - want / want.sum()).max() <= 1e-15
    for args, text in (((0,), "f is an integer 1 .. 8"), ((9,), "f is an integer 1 .. 8"), ((2.5,), "f is an integer"),
                       ((2, "box"), "kind must be 'mean', 'decimate' or 'gaussian'"), ((2, "gaussian"), "needs a finite fwhm > 0"),
                       ((2, "gaussian", 0.0), "needs a finite fwhm > 0"), ((2, "gaussian", float("nan")), "needs a finite fwhm"),
                       ((2, "mean", 1.0), "fwhm belongs to kind='gaussian'"), ((4, "gaussian", 1e-3), "too narrow")):
        with pytest.raises(ValueError, match=f"slice_profile: .*{text}"):
            baselines.slice_profile(*args)


def test_study_parser_defaults_and_flag_refusals_before_the_input_is_loaded(tmp_path):
    args = tp_script.build_parser().parse_args(["--data", "x.mat"])
    assert (args.roi_start, args.roi_end, args.factor, args.profile, args.fwhm) == (40, 90, 2, "mean", 1.0)
    assert (args.tv_lambda, args.tv_huber, args.tv_iters, args.tv_gz) == (baselines.TV3D_DEFAULT_LAMBDA, baselines.TV3D_DEFAULT_HUBER,
                                                                         baselines.TV3D_DEFAULT_ITERS, 1.0)
    assert args.with_inr is False and args.footprint == "point" and args.key is None and args.pt_id is None
    missing = str(tmp_path / "pat03_not_there.mat")        # never opened: every refusal comes first
    run = lambda *flags: tp_script.main(["--data", missing, "--output_address", str(tmp_path / "res"), *flags])
    for flags, text in ((("--factor", "1"), "factor is the number of thin slices per thick one, 2 .. 8.*1"),
                        (("--factor", "9"), "factor is the number of thin slices"),
                        (("--profile", "gaussian", "--fwhm", "0"), "gaussian profile needs a finite fwhm > 0"),
                        (("--profile", "gaussian", "--fwhm", "nan"), "gaussian profile needs a finite fwhm"),
                        (("--tv_lambda", "-0.001"), "tv_lambda must be finite and >= 0.*-0.001"),
                        (("--tv_huber", "inf"), "tv_huber must be finite and >= 0"), (("--tv_gz", "-1"), "tv_gz must be finite and >= 0"),
                        (("--tv_iters", "0"), "tv_iters must be 1 .. 100,000"), (("--tv_iters", "100001"), "tv_iters must be 1 .. 100,000"),
                        (("--with_inr", "--factor", "4"), "with_inr.*factor 2 and the mean profile only.*factor 4"),
                        (("--with_inr", "--profile", "gaussian"), "with_inr.*factor 2 and the mean profile only.*'gaussian'"),
                        (("--with_inr", "--number_of_epochs", "0"), "number_of_epochs must be >= 1"),
                        (("--roi_start", "40", "--roi_end", "44"), "ROI 40:44: SSIM needs >= 7 x 7")):
        with pytest.raises(ValueError, match=text):
            run(*flags)
    assert not os.path.exists(str(tmp_path / "res"))
    with pytest.raises(SystemExit):
        run("--profile", "box")
    # flags that are in order get as far as the missing input
    with pytest.raises((OSError, ValueError), match="not_there"):
        run("--profile", "gaussian", "--fwhm", "1.5", "--factor", "4")
    with pytest.raises(ValueError, match="through_plane_study: profile must be 'mean' or 'gaussian'"):
        drivers.through_plane_study(np.ones((8, 8, 4)), profile="box")
    with pytest.raises(ValueError, match="through_plane_study: 9 slices make 2 thick slices of 4; the cubic spline along z needs at least 4"):
        drivers.through_plane_study(np.ones((8, 8, 9)), factor=4)
    with pytest.raises(ValueError, match="through_plane_study: the volume is \\[X, Y, Z, B\\] or \\[X, Y, Z\\]"):
        drivers.through_plane_study(np.ones((8, 8)))


def test_restated_operators_are_adjoint_pairs():
    rng = np.random.default_rng(3)
    g = (0.4, 1.0, 1.0)
    for shape, f in (((4, 6, 10), (2, 3, 2)), ((1, 8, 8), (1, 1, 1)), ((8, 16, 24), (8, 8, 8)), ((3, 5, 7), (3, 5, 7)),
                     ((5, 7, 64), (5, 7, 1))):
        lr_shape = tuple(s // v for s, v in zip(shape, f))
        for kernel in ("mean", "decimate", tuple(k / k.sum() for k in (rng.random(v) + 0.1 for v in f))):
            k = T.block_table(T.block_factors(kernel, f))
            assert abs(k.sum() - 1.0) <= 1e-14
            x, r = rng.standard_normal((2,) + shape), rng.standard_normal((2,) + lr_shape)
            a, b = (T.apply_A(x, k) * r).sum(), (x * T.apply_AT(r, k)).sum()
            scale = np.abs(T.apply_A(x, k) * r).sum()
            print(f"{shape} {f}: |<Ax, r> - <x, A^T r>| / sum|.| = {abs(a - b) / scale:.2e}")
            assert abs(a - b) <= 1e-12 * scale
            # A A^T = |k|^2 I
            assert np.abs(T.apply_A(T.apply_AT(r, k), k) - T.table_sq(k) * r).max() <= 1e-14 * np.abs(r).max()
        p = [rng.standard_normal((2,) + shape) for _ in range(3)]
        t = T.grad(x, g)
        c, d = sum((ti * pi).sum() for ti, pi in zip(t, p)), -(x * T.div(*p, g)).sum()
        scale = sum(np.abs(ti * pi).sum() for ti, pi in zip(t, p))
        print(f"{shape}: |<grad x, p> + <x, div p>| / sum|.| = {abs(c - d) / max(scale, 1e-300):.2e}")
        assert abs(c - d) <= 1e-12 * max(scale, 1e-300)
    # definitions by hand: a 2 x 1 x 2 volume and the table's order of multiplication
    x = np.array([[[1.0, 2.0]], [[4.0, 8.0]]])
    d0, d1, d2 = T.diffs(x)
    assert np.array_equal(d0, [[[3, 6]], [[0, 0]]]) and np.array_equal(d1, np.zeros((2, 1, 2))) and np.array_equal(d2, [[[1, 0]], [[4, 0]]])
    assert np.array_equal(T.div(np.array([[[1.0, 2]], [[9, 9]]]), np.zeros((2, 1, 2)), np.array([[[5.0, 9]], [[7, 9]]]), (0.5, 1, 1)),
                          [[[5 + 0.5, -5 + 1.0]], [[7 - 0.5, -7 - 1.0]]])
    ks = (np.array([0.25, 0.75]), np.array([1.0]), np.array([0.2, 0.8]))
    assert np.array_equal(T.block_table(ks), [[[0.2 * 0.25, 0.8 * 0.25]], [[0.2 * 0.75, 0.8 * 0.75]]])
    assert np.array_equal(T.apply_A(x, T.block_table(T.block_factors("decimate", (2, 1, 2)))), [[[1.0]]])
    assert np.array_equal(T.apply_A(x, T.block_table(T.block_factors("mean", (2, 1, 1)))), [[[2.5, 5.0]]])
    assert T.step((4, 6, 6), (1, 1, 1), 0.1) == (1.0 / np.sqrt(12.0), 0.1) and T.step((1, 6, 6), (5, 1, 1), 0.1)[0] == T2.TAU
    assert T.step((4, 1, 1), (0, 1, 1), 0.1) == (T2.TAU, 0.0) and T.step((4, 6, 6), (0.4, 1, 1), 0.1)[0] == 1.0 / np.sqrt(4.0 * (2.0 + 0.4 * 0.4))


@pytest.mark.parametrize("g", T.CASE_GRAD_WEIGHTS, ids=("g111", "g0.4"))
def test_restated_iteration_reaches_the_lbfgs_minimum_of_the_huber_energy(g):
    """The issue's case: 4 x 6 x 6, factors (2, 3, 2), kernels ([.25, .75], mean, [.2, .8]), weights in [0.5, 1.5) with one zero,
    lambda 0.05, alpha 0.02; relative gap after 1,000 iterations <= 1e-9 (at 300 it is of the order of 1e-7)."""
    hr, y, w = T.case_data()
    assert hr.shape == (1, 4, 6, 6) and (w == 0).sum() == 1 and w[w > 0].min() >= 0.5 and w.max() < 1.5
    k = T.block_table(T.CASE_KERNEL)
    minimum = T.lbfgs_minimum(y, k, T.CASE_LAM, T.CASE_ALPHA, w, hr.shape, g)
    gaps = {}
    for n in (300, 1000):
        x, e, change = T.solve(y, T.CASE_FACTORS, T.CASE_KERNEL, T.CASE_LAM, T.CASE_ALPHA, n, g, w, return_info=True)
        gaps[n] = (e[0] - minimum) / minimum
        print(f"g {g}: L-BFGS-B minimum {minimum:.12f}; {n} iterations: energy {e[0]:.12f}, relative gap {gaps[n]:.2e}, change {change[0]:.2e}")
    assert abs(gaps[1000]) <= 1e-9
    assert gaps[300] > abs(gaps[1000])


def test_restatement_is_the_2d_restatement_where_the_slices_do_not_couple():
    # one slice: D = 1, any g0
    _, y = T2.case_data()
    want, we, wc = T2.solve(y, T2.CASE_FACTORS, "mean", T2.CASE_LAM, T2.CASE_ALPHA, 300, T2.CASE_W, return_info=True)
    got, ge, gc = T.solve(y[:, None], (1,) + T2.CASE_FACTORS, "mean", T2.CASE_LAM, T2.CASE_ALPHA, 300, (0.7, 1.0, 1.0), T2.CASE_W[:, None],
                          return_info=True)
    assert np.array_equal(got[:, 0], want) and np.array_equal(gc, wc) and abs(ge - we) <= 1e-12 * we
    # four pat07 slices at g0 = 0
    v = T2.pat07_roi()[12:16]
    for kernel in ("mean", "decimate"):
        y = T2.apply_A(v, T2.block_kernel(kernel, (2, 2)))
        want, _, wc = T2.solve(y, (2, 2), kernel, 3e-3, 0.3, 100, return_info=True)
        got, _, gc = T.solve(y[None], (1, 2, 2), kernel, 3e-3, 0.3, 100, (0.0, 1.0, 1.0), return_info=True)
        coupled = T.solve(y[None], (1, 2, 2), kernel, 3e-3, 0.3, 100, (1.0, 1.0, 1.0))
        print(f"pat07 slices 12:16 {kernel}: g0 = 0 equal {np.array_equal(got[0], want)}; g0 = 1 differs by {np.abs(coupled[0] - want).max():.2e}")
        assert np.array_equal(got[0], want) and gc[0] == wc.max()
        assert np.abs(coupled[0] - want).max() > 1e-4
