"""No device: the float64 restatement of non-local means and non-local upsampling (tests/nlm_common.py) -- against the definition
evaluated voxel by voxel, its fixed points, the data consistency of the restated solve, that it denoises the cases' data --, the new
symbols, and the refusals of inr_nlm3d / inr_nlm_upsample, of the Python layer and of the drivers' new flags, all before any device
work."""
import ctypes
import itertools
import re

import numpy as np
import pytest
import torch

from tests import nlm_common as N
from mri_super_resolution_amd import _lib, baselines, denoise, ops

NEW_SYMBOLS = ("inr_nlm3d", "inr_nlm3d_f32", "inr_nlm_upsample_workspace_doubles", "inr_nlm_upsample", "inr_nlm_upsample_f32")


def _fake(k):
    return ctypes.c_void_p(0x7000_0000_0000 + (1 << 32) * k)      # never dereferenced: every call here fails in validation


@pytest.mark.parametrize("center", ("max", "one"))
@pytest.mark.parametrize("rician", (False, True))
def test_the_restatement_is_the_definition_voxel_by_voxel(center, rician):
    rng = np.random.default_rng(5)
    shape, search, patch = (3, 5, 6), (1, 2, 2), (1, 1, 1)
    x = 0.5 + 0.2 * rng.random((2,) + shape)
    guide = x.mean(axis=0)
    sigma2 = np.full(shape, 1e-3) if rician else None
    out = N.nlm(x, guide, search, patch, 2e-3, sigma2, center=center)
    worst = 0.0
    for p in itertools.product(*(range(n) for n in shape)):
        worst = max(worst, float(np.abs(out[(slice(None),) + p] - N.nlm_voxel(x, guide, search, patch, 2e-3, p, sigma2, center)).max()))
    print(f"center {center}, rician {rician}: max deviation {worst:.2e}")
    assert worst <= 1e-13        # about 100 terms of O(1) at eps


def test_a_zero_search_radius_returns_the_input_exactly():
    c = N.case("1-small-odd")
    for center in ("max", "one"):
        assert N.nlm(c["x"], c["guide"], (0, 0, 0), (1, 1, 1), N.H2, center=center).tobytes() == c["x"].tobytes()


def test_a_constant_volume_returns_itself():
    x = np.full((1, 4, 6, 5), 0.7)
    for center in ("max", "one"):
        out = N.nlm(x, x[0], (1, 2, 2), (1, 1, 1), N.H2, center=center)
        assert np.abs(out - x).max() <= 4 * N.EPS


def test_voxels_outside_the_mask_or_without_a_positive_strength_pass_through():
    c = N.case("1-small-odd")
    shape = c["x"].shape[1:]
    h2 = np.full(shape, N.H2)
    h2[0, 0, 0], h2[1, 2, 3], h2[2, 2, 2] = 0.0, -1.0, np.nan
    mask = np.ones(shape, np.uint8)
    mask[:, :3] = 0
    out = N.nlm(c["x"], c["guide"], c["search"], c["patch"], h2, mask=mask)
    copied = (mask == 0) | ~(h2 > 0)
    assert np.array_equal(out[0][copied], c["x"][0][copied]) and not np.array_equal(out[0][~copied], c["x"][0][~copied])
    assert np.array_equal(out[0][~copied], N.nlm(c["x"], c["guide"], c["search"], c["patch"], N.H2)[0][~copied])


@pytest.mark.parametrize("kind", ("mean", "decimate"))
def test_the_restated_upsample_satisfies_the_data(kind):
    u = N.UPSAMPLE
    lr, _ = N.upsample_case()
    k = N.named_kernel(kind, u["factors"])
    x, change = N.upsample(lr, u["factors"], k, u["levels"][:1], 1, u["search"], u["patch"])
    res = float(np.abs(N.block_apply(x, u["factors"], N.kernel_table(*k)) - lr).max())
    bound = 4 * (np.prod(u["factors"]) + 2) * N.EPS * float(np.abs(x).max())
    print(f"{kind}: |A x - lr| {res:.2e}, bound {bound:.2e}, change {change}")
    assert res <= bound


def test_the_solve_of_the_gpu_test_is_short_enough_for_its_reference():
    (_, change), d_x, d_change = N.upsample_reference()
    print(f"d_ref of x {d_x:.2e}, of change {d_change:.2e}, change {change}")
    assert d_x <= 1e-12 and np.all(np.diff(change) < 0)


@pytest.mark.parametrize("name", ("2-image", "6-rician-mean-guide"))
def test_the_restatement_denoises_the_data_of_the_cases(name):
    c = N.case(name)
    out, _, _ = N.reference(name)
    before, after = N.rmse(c["x"], c["truth"]), N.rmse(out, c["truth"])
    print(f"{name}: RMSE {before:.4f} -> {after:.4f}")
    assert after < before


@pytest.mark.parametrize("name", N.CASE_IDS)
def test_the_preconditions_of_the_device_comparison_hold(name):
    out, d_ref, info = N.reference(name)
    c = N.case(name)
    print(f"{name}: d_ref {d_ref:.2e}, smallest wmax {info['wmax'].min():.2e}")
    assert info["wmax"].min() >= N.WMAX_FLOOR and 0 < d_ref < 1e-13
    if c["sigma2"] is not None:
        assert (info["m"] - 2.0 * c["sigma2"]).min() >= N.RICIAN_FLOOR


def test_the_new_symbols_are_declared_exported_and_bound():
    from tests.test_abi_cpu import header_symbols
    from mri_super_resolution_amd._build import LIB_PATH
    handle = ctypes.CDLL(LIB_PATH)
    declared = header_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(handle, s), s
    assert (_lib.INR_NLM_MAX_SEARCH, _lib.INR_NLM_MAX_PATCH, _lib.INR_NLM_MAX_CHANNELS, _lib.INR_NLM_MAX_PASSES) == (5, 2, 16, 10000)
    assert baselines.NLM_DEFAULT_LEVELS == (0.125, 0.0625, 0.03125, 0.015625, 0.0078125)


FILTER_GOOD = dict(out=1, x=2, guide=3, h2=2e-3, h2_map=None, sigma2=None, mask=None, G=2, C=3, D=4, H=6, W=5, s=(1, 2, 2), r=(1, 1, 1), center=0)
FILTER_REFUSALS = (
    ("null pointer", dict(out=None)),
    ("null pointer", dict(x=None)),
    ("bad sizes \\(n_groups = -1\\)", dict(G=-1)),
    ("channels must be 1 .. 16 \\(got 0\\)", dict(C=0)),
    ("channels must be 1 .. 16 \\(got 17\\)", dict(C=17)),
    ("a null guide needs channels == 1 \\(got 3\\)", dict(guide=None)),
    ("bad sizes", dict(D=0)),
    ("bad sizes", dict(W=-2)),
    ("fewer than 2\\^31 voxels", dict(D=2048, H=1024, W=1024)),
    ("search radii are 0 .. 5 per axis \\(s1 is 6\\)", dict(s=(1, 6, 2))),
    ("search radii are 0 .. 5 per axis \\(s0 is -1\\)", dict(s=(-1, 2, 2))),
    ("patch radii are 0 .. 2 per axis \\(r2 is 3\\)", dict(r=(1, 1, 3))),
    ("center must be 0 \\(max\\) or 1 \\(one\\) \\(got 2\\)", dict(center=2)),
    ("a scalar h2 must be finite and > 0", dict(h2=0.0)),
    ("a scalar h2 must be finite and > 0", dict(h2=-1.0)),
    ("a scalar h2 must be finite and > 0", dict(h2=float("nan"))),
    ("a scalar h2 must be finite and > 0", dict(h2=float("inf"))),
    ("out must not overlap x", dict(out=2)),
    ("out must not overlap guide", dict(out=3)),
)


@pytest.mark.parametrize("entry", ("inr_nlm3d", "inr_nlm3d_f32"))
def test_every_refusal_of_the_filter_comes_with_its_code_and_message_before_any_device_work(entry):
    lib = _lib.lib()
    fn = getattr(lib, entry)
    ptr = lambda v: None if v is None else _fake(v)

    def call(a):
        """Only ever with arguments that are refused, or with an empty batch: the pointers are fakes."""
        return fn(ptr(a["out"]), ptr(a["x"]), ptr(a["guide"]), a["h2"], ptr(a["h2_map"]), ptr(a["sigma2"]), ptr(a["mask"]), a["G"], a["C"],
                  a["D"], a["H"], a["W"], *a["s"], *a["r"], a["center"], None)

    for text, change in FILTER_REFUSALS:
        a = dict(FILTER_GOOD)
        a.update(change)
        rc = call(a)
        msg = lib.inr_last_error().decode()
        assert rc == _lib.INR_E_INVALID, (change, rc, msg)
        assert re.search(text, msg) and entry in msg, (change, msg)
    assert call(dict(FILTER_GOOD, G=0)) == 0                                  # an empty batch succeeds and launches nothing
    assert call(dict(FILTER_GOOD, G=0, h2=0.0, h2_map=5)) == 0                # with a map the scalar is not looked at


UP_GOOD = dict(out=1, change=2, y=3, x0=None, guide=None, n=2, D=8, H=12, W=14, f=(2, 2, 2), k=((0.5, 0.5),) * 3, levels=(0.125, 0.0625),
               n_iter=2, relax=1.0, s=(2, 2, 2), r=(1, 1, 1))
UP_REFUSALS = (
    ("null pointer", dict(out=None)),
    ("null pointer", dict(y=None)),
    ("bad sizes \\(n_volumes = -1\\)", dict(n=-1)),
    ("block factors are 1 .. 8 per axis \\(got 0 x 2 x 2\\)", dict(f=(0, 2, 2))),
    ("block factors are 1 .. 8 per axis \\(got 2 x 9 x 2\\)", dict(f=(2, 9, 2))),
    ("bad sizes", dict(D=0)),
    ("fewer than 2\\^31 voxels", dict(D=2048, H=1024, W=1024)),
    ("is no whole number of 2 x 2 x 2 blocks", dict(W=13)),
    ("search radii are 0 .. 5 per axis \\(s2 is 6\\)", dict(s=(2, 2, 6))),
    ("patch radii are 0 .. 2 per axis \\(r0 is 3\\)", dict(r=(3, 1, 1))),
    ("kernel factors must be finite \\(k1\\[0\\]", dict(k=((0.5, 0.5), (float("nan"), 0.5), (0.5, 0.5)))),
    ("every kernel factor must sum to 1 \\(k2 sums to", dict(k=((0.5, 0.5), (0.5, 0.5), (0.5, 0.6)))),
    ("levels \\* n_iter must be 0 .. 10000", dict(n_iter=5001)),
    ("levels \\* n_iter must be 0 .. 10000", dict(n_iter=-1)),
    ("every level must be finite and > 0", dict(levels=(0.125, 0.0))),
    ("every level must be finite and > 0", dict(levels=(float("inf"), 0.1))),
    ("relax must lie in \\(0, 1\\] \\(got 0\\)", dict(relax=0.0)),
    ("relax must lie in \\(0, 1\\] \\(got 1.5\\)", dict(relax=1.5)),
    ("relax must lie in \\(0, 1\\] \\(got nan\\)", dict(relax=float("nan"))),
)


@pytest.mark.parametrize("entry", ("inr_nlm_upsample", "inr_nlm_upsample_f32"))
def test_every_refusal_of_the_upsampling_comes_with_its_code_and_message_before_any_device_work(entry):
    lib = _lib.lib()
    fn = getattr(lib, entry)
    ptr = lambda v: None if v is None else _fake(v)
    arr = lambda v: (ctypes.c_double * len(v))(*v)

    def plan_of(a):
        return lib.inr_nlm_upsample_workspace_doubles(a["n"], a["D"], a["H"], a["W"], *a["f"])

    def call(a, ws, ws_doubles):
        return fn(ptr(a["out"]), ptr(a["change"]), ptr(a["y"]), ptr(a["x0"]), ptr(a["guide"]), a["n"], a["D"], a["H"], a["W"], *a["f"],
                  *(arr(k) for k in a["k"]), arr(a["levels"]), len(a["levels"]), a["n_iter"], a["relax"], *a["s"], *a["r"], ws, ws_doubles, None)

    for text, change in UP_REFUSALS:
        a = dict(UP_GOOD)
        a.update(change)
        rc = call(a, _fake(9), max(plan_of(a), plan_of(UP_GOOD)))
        msg = lib.inr_last_error().decode()
        assert rc == _lib.INR_E_INVALID, (change, rc, msg)
        assert re.search(text, msg) and entry in msg, (change, msg)
    plan = plan_of(UP_GOOD)
    assert plan == 2 * (2 * 8 * 12 * 14 + 4 * 6 * 7)
    rc = call(dict(UP_GOOD), _fake(9), plan - 1)
    assert rc == _lib.INR_E_WORKSPACE and "workspace too small" in lib.inr_last_error().decode() and entry in lib.inr_last_error().decode()
    assert call(dict(UP_GOOD), None, plan) == _lib.INR_E_WORKSPACE
    assert call(dict(UP_GOOD), ctypes.c_void_p(0x7000_0000_0008), plan) == _lib.INR_E_ALIGN
    a = dict(UP_GOOD, n=0)
    assert call(a, _fake(9), plan_of(a)) == 0                                 # an empty batch succeeds and launches nothing
    for args in ((-1, 8, 12, 14, 2, 2, 2), (2, 8, 12, 13, 2, 2, 2), (2, 8, 12, 14, 2, 9, 2), (2, 0, 12, 14, 2, 2, 2), (1, 2048, 1024, 1024, 2, 2, 2)):
        assert lib.inr_nlm_upsample_workspace_doubles(*args) == 0, args


def test_the_host_checks_of_ops_refuse_by_name():
    assert ops.nlm_radii("t", 3, 1) == ((3, 3, 3), (1, 1, 1)) and ops.nlm_radii("t", (0, 5, 2), [2, 0, 1]) == ((0, 5, 2), (2, 0, 1))
    for search, patch, text in ((6, 1, "search must be an int or a triple of ints 0 .. 5"), (-1, 1, "search must be"), ((1, 2), 1, "search must be"),
                                (2.5, 1, "search must be"), (True, 1, "search must be"), (2, 3, "patch must be an int or a triple of ints 0 .. 2"),
                                (2, (1, 1, 1.5), "patch must be"), (2, "a", "patch must be")):
        with pytest.raises(ValueError, match=text):
            ops.nlm_radii("t", search, patch)
    with pytest.raises(ValueError, match="center must be 'max' or 'one'"):
        ops.nlm_center("t", "mean")
    for h2 in (0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="h2 must be"):
            ops.nlm_strength("t", h2)
    for c in (0, 17):
        with pytest.raises(ValueError, match="channels must be 1 .. 16"):
            ops.nlm_channels("t", c)
    with pytest.raises(ValueError, match="fewer than 2\\^31 voxels"):
        ops.nlm_volume("t", (2048, 1024, 1024))
    for levels, n_iter, relax, text in (((0.1, 0.0), 2, 1.0, "every level must be finite and > 0"), ((0.1, float("nan")), 2, 1.0, "every level"),
                                        ("ab", 2, 1.0, "levels must be a sequence of numbers"), ((0.1,), -1, 1.0, "n_iter must be"),
                                        ((0.1,), 1.5, 1.0, "n_iter must be"), ((0.1,) * 3, 3334, 1.0, "n_iter must be"),
                                        ((0.1,), 2, 0.0, "relax must lie in \\(0, 1\\]"), ((0.1,), 2, 1.01, "relax must lie")):
        with pytest.raises(ValueError, match=text):
            ops.nlm_schedule("t", levels, n_iter, relax)
    assert ops.nlm_schedule("t", (), 5, 0.5) == ([], 5, 0.5)
    # ops.nlm3d and ops.nlm_upsample: the host values first, then the tensors
    cpu = torch.zeros(1, 1, 4, 6, 5, dtype=torch.float64)
    with pytest.raises(ValueError, match="search must be"):
        ops.nlm3d(cpu, 1e-3, search=6)
    with pytest.raises(ValueError, match="h2 must be finite and > 0"):
        ops.nlm3d(cpu, 0.0)
    with pytest.raises(TypeError, match="float32 or torch.float64"):
        ops.nlm3d(cpu.half(), 1e-3)
    with pytest.raises(ops.InrDeviceError):
        ops.nlm3d(cpu, 1e-3)
    with pytest.raises(ValueError, match="relax must lie"):
        ops.nlm_upsample(cpu[0], (2, 2, 2), N.named_kernel("mean", (2, 2, 2)), (0.1,), relax=2.0)
    with pytest.raises(ValueError, match="kernel factor k0 must be finite and sum to 1"):
        ops.nlm_upsample(cpu[0], (2, 2, 2), ([0.5, 0.6], [0.5, 0.5], [0.5, 0.5]), (0.1,))
    with pytest.raises(ops.InrDeviceError):
        ops.nlm_upsample(cpu[0], (2, 2, 2), N.named_kernel("mean", (2, 2, 2)), (0.1,))


def test_the_refusals_of_denoise_nlm_come_by_name_and_before_the_device():
    x = np.zeros((3, 4, 6, 5))
    for text, kw in (("sigma is required", dict(sigma=None)),
                     ("a scalar sigma must be finite and > 0", dict(sigma=0.0)),
                     ("a scalar sigma must be finite and > 0", dict(sigma=float("nan"))),
                     ("sigma has shape \\(6, 5\\), expected \\(4, 6, 5\\)", dict(sigma=np.ones((6, 5)))),
                     ("beta must be finite and > 0", dict(beta=0.0)),
                     ("search must be an int or a triple", dict(search=6)),
                     ("patch must be an int or a triple", dict(patch=(1, 1))),
                     ("center must be 'max' or 'one'", dict(center="none")),
                     ("guide must be None, 'mean' or an array", dict(guide="median")),
                     ("guide has shape", dict(guide=np.zeros((3, 4, 6, 5)))),
                     ("mask has shape", dict(mask=np.ones((6, 5)))),
                     ("at most 16 channels \\(got 17\\)", dict(data=np.zeros((17, 4, 6, 5)), guide="mean")),
                     ("at least 2 axes", dict(data=np.zeros(5))),
                     ("an image has no first axis", dict(data=np.zeros((6, 5)), search=(1, 2, 2)))):
        kw = dict(kw)
        data = kw.pop("data", x)
        kw.setdefault("sigma", 0.03)
        with pytest.raises(ValueError, match=text):
            denoise.nlm(data, **kw)
    with pytest.raises(TypeError, match="missing 1 required positional argument: 'sigma'"):
        denoise.nlm(x, rician=True)
    with pytest.raises(TypeError, match="ndarray or a device tensor"):
        denoise.nlm([[1.0]], 0.03)
    with pytest.raises(TypeError, match="float16"):
        denoise.nlm(np.zeros((6, 5), np.float16), 0.03)
    with pytest.raises(TypeError, match="float32 or float64"):
        denoise.nlm(torch.zeros(6, 5, dtype=torch.float16), 0.03)
    with pytest.raises(TypeError, match="sigma must be a number, an ndarray or a tensor"):
        denoise.nlm(x, [[0.03]])


def test_the_refusals_of_baselines_nlm_upsample_come_by_name_and_before_the_device():
    lr = np.zeros((4, 6, 7))
    for text, kw in (("factors are \\(f0, f1, f2\\)", dict(factors=(2, 2))),
                     ("factors are 1 .. 8 per axis", dict(factors=(2, 9, 2))),
                     ("kernel must be 'mean', 'decimate' or a triple", dict(kernel="gauss")),
                     ("kernel factor k0 must be finite and sum to 1", dict(kernel=([0.5, 0.4], [0.5, 0.5], [0.5, 0.5]))),
                     ("every level must be finite and > 0", dict(levels=(0.1, -0.1))),
                     ("n_iter must be an integer >= 0", dict(n_iter=-1)),
                     ("len\\(levels\\) \\* n_iter <= 10000", dict(n_iter=2001)),
                     ("search must be", dict(search=6)),
                     ("patch must be", dict(patch=3)),
                     ("relax must lie in \\(0, 1\\]", dict(relax=0.0)),
                     ("needs at least 3-D input", dict(lr=np.zeros((6, 7)))),
                     ("x0 must have shape \\(8, 12, 14\\)", dict(x0=np.zeros((8, 12, 13)))),
                     ("guide must have shape \\(8, 12, 14\\)", dict(guide=np.zeros((4, 6, 7))))):
        kw = dict(kw)
        data = kw.pop("lr", lr)
        kw.setdefault("factors", (2, 2, 2))
        with pytest.raises(ValueError, match=text):
            baselines.nlm_upsample(data, **kw)
    with pytest.raises(TypeError, match="x0 must be given like lr"):
        baselines.nlm_upsample(lr, (2, 2, 2), x0=torch.zeros(8, 12, 14))
    with pytest.raises(TypeError, match="guide must be given like lr"):
        baselines.nlm_upsample(lr, (2, 2, 2), guide=torch.zeros(8, 12, 14))


def test_there_is_no_cpu_fallback():
    with pytest.raises(ops.InrDeviceError):
        denoise.nlm(torch.zeros(4, 6, 5, dtype=torch.float64), 0.03)
    with pytest.raises(ops.InrDeviceError):
        baselines.nlm_upsample(torch.zeros(4, 6, 7, dtype=torch.float64), (2, 2, 2))
    if not torch.cuda.is_available():
        with pytest.raises(ops.InrDeviceError):
            denoise.nlm(np.zeros((4, 6, 5)), 0.03)
        with pytest.raises(ops.InrDeviceError):
            baselines.nlm_upsample(np.zeros((4, 6, 7)), (2, 2, 2))


def test_the_new_driver_flags_are_refused_by_name_before_the_input_is_loaded(tmp_path):
    from mri_super_resolution_amd import drivers
    from mri_super_resolution_amd.scripts import denoise as denoise_script
    from mri_super_resolution_amd.scripts import superresDWI as dwi_script
    from mri_super_resolution_amd.scripts import through_plane as through_plane_script
    missing = str(tmp_path / "pat1_missing.mat")                                 # never opened: every call fails before
    for extra, text in ((["--nlm_search", "6"], "search must be an int or a triple of ints 0 .. 5"), (["--nlm_patch", "3"], "patch must be"),
                        (["--nlm_iters", "-1"], "n_iter must be an integer >= 0"), (["--nlm_iters", "2001"], "len\\(levels\\) \\* n_iter <= 10000")):
        with pytest.raises(ValueError, match=text):
            through_plane_script.main(["--data", missing, "--with_nlm"] + extra)
        with pytest.raises(ValueError, match=text):
            dwi_script.main(["--data", missing, "--nlm_baseline"] + extra)
    with pytest.raises(ValueError, match="nlm_start must be 'replicate' or 'spline'"):
        drivers.check_through_plane(with_nlm=True, nlm_start="zerofill")
    with pytest.raises(ValueError, match="--nlm_baseline solves for 2 x 2 HR pixels per LR pixel and needs an even ROI side"):
        dwi_script.main(["--data", missing, "--nlm_baseline", "--roi_start", "40", "--roi_end", "91"])
    for extra, text in ((["--nlm_search", "6"], "search must be"), (["--nlm_patch", "-1"], "patch must be"), (["--nlm_beta", "0"], "--nlm_beta must be")):
        with pytest.raises(ValueError, match=text):
            denoise_script.main(["--data", missing, "--out", str(tmp_path / "o.mat"), "--method", "nlm"] + extra)
    for argv in (["--nlm_start", "cubic"], ):
        with pytest.raises(SystemExit):
            through_plane_script.build_parser().parse_args(["--data", missing] + argv)
    with pytest.raises(SystemExit):
        denoise_script.build_parser().parse_args(["--data", missing, "--out", "o", "--method", "tv"])
    with pytest.raises(SystemExit):
        dwi_script.build_parser().parse_args(["--data", missing, "--denoise", "tv"])
    # without the flags the values are not looked at, as before
    drivers.check_through_plane(nlm_search=9)
