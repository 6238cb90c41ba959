"""GPU: the S0 / ADC solver of csrc/tvadc.hip against its float64 restatement (tests/tvadc_common.py), against properties that do not
depend on the restatement, against the L-BFGS-B minimum of the stated energy, bit for bit across a batch and between the fp32 and fp64
entries, on the study case, and through ``superresDWI --tv_adc`` and ``scripts/joint_bvalues --with_adc_model``.

Bounds are those of tests/test_gpu_tvsr.py: about ten roundings of 1.1e-16 per pixel and iteration give 1e-12 after 1,000 iterations on
maps of order 1, and 1e-10 absolute on each map (the ADC normalised by the largest b-value, u = adc b_max) leaves two orders of margin.
The nonlinear step is not non-expansive; that the iteration does not amplify rounding is measured instead, by
test_tvadc_cpu.py::test_float64_restatement_agrees_with_extended_precision (<= 1e-13 up to 1,000 iterations).  The device exp may differ
from libm's in the last place: the same order as one rounding.  ``change`` is the difference of two maps within the bound: 2e-10.
``energy`` is a sum of at most C h w + H W non-negative terms of a few roundings each: 1e-12 relative against the restated objective
at the returned maps.  Every test prints what it measured before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

from tests import tvadc_common as A
from tests import tvj_common as J
from tests import tvsr_common as T
from mri_super_resolution_amd import _lib, baselines, drivers, matio, metrics, ops, reports
from mri_super_resolution_amd.scripts import joint_bvalues as jb_script
from mri_super_resolution_amd.scripts import superresDWI as dwi_script

pytestmark = pytest.mark.gpu

SOLVER_BOUND = 1e-10
ENERGY_BOUND = 1e-12
CASE = (A.CASE_B, A.CASE_FACTORS, "mean", A.CASE_LAM, A.CASE_ALPHA)
BOX = (A.CASE_SMAX, A.CASE_ADCMAX, A.CASE_ADC0)


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _compare(name, y, b, f, kernel, lam, alpha, n_iter, mu=A.CASE_MU, coupling="joint", box=BOX, w=None, x0=None):
    s, adc, info = baselines.tv_superres_adc(y, b, f, kernel, lam, alpha, n_iter, mu, coupling, *box, weight=w, x0=x0, return_info=True)
    ws, wadc, _, change = A.solve_adc(y, b, f, kernel, lam, alpha, n_iter, mu, coupling, *box, w=w, x0=x0, return_info=True)
    k = T.block_kernel(kernel, f)
    b_max = float(np.max(b))
    yd = np.where(w == 0, 0.0, y) if w is not None else y
    at_maps = A.energy_adc(s, adc * b_max, np.asarray(b, np.float64) / b_max, yd, k, lam, alpha, w, mu, coupling)
    err_s, err_u = float(np.abs(s - ws).max()), float(np.abs(adc - wadc).max() * b_max)
    e_rel = float(np.abs(info["energy"] - at_maps).max() / np.abs(at_maps).max())
    c_err = float(np.abs(info["change"] - change).max())
    print(f"{name}, {coupling}, {n_iter} iterations: max|s - restated| = {err_s:.3e}, max|u - restated| = {err_u:.3e} (bound "
          f"{SOLVER_BOUND:.0e}), energy against the restated objective at the returned maps {e_rel:.2e} (bound {ENERGY_BOUND:.0e}), "
          f"|change - restated| {c_err:.2e} (change {float(change.max()):.2e})")
    assert s.dtype == adc.dtype == np.float64 and s.shape == ws.shape == adc.shape
    assert err_s <= SOLVER_BOUND and err_u <= SOLVER_BOUND
    assert c_err <= 2 * SOLVER_BOUND            # the difference of two maps that are each within the bound
    assert e_rel <= ENERGY_BOUND
    return s, adc, info


# ---- against the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coupling", ("joint", "none"))
@pytest.mark.parametrize("n_iter", (1, 2, 300))
def test_solver_matches_the_restatement_on_the_small_case(n_iter, coupling):
    _, _, y, w = A.case_data()
    _compare("6x10 (3, 2) mean, beta (0, .4, 1), weighted Huber, mu (1, .1)", y, *CASE, n_iter, A.CASE_MU, coupling, w=w)


def test_solver_matches_the_restatement_at_the_channel_and_parameter_edges():
    rng = np.random.default_rng(16)
    k = T.block_kernel("mean", (3, 2))
    for C in (16, 2):
        b = np.linspace(0.0, 1500.0, C)
        s_true, u_true = 0.2 + 0.8 * rng.random((2, 6, 10)), 0.5 + 2.5 * rng.random((2, 6, 10))
        y = T.apply_A(A.model(s_true, u_true, b / b.max()), k) + 0.02 * rng.standard_normal((2, C, 2, 5))
        for coupling in ("joint", "none"):
            _compare(f"C = {C}, 6x10 (3, 2)", y, b, (3, 2), "mean", 0.02, 0.01, 60, coupling=coupling)
    _, _, y, w = A.case_data()
    _compare("plain TV (Huber 0)", y, A.CASE_B, A.CASE_FACTORS, "mean", A.CASE_LAM, 0.0, 60, w=w)
    # mu_d = 0: the ADC leaves the prior, p_u stays 0
    for coupling in ("joint", "none"):
        _compare("map weights (1, 0)", y, *CASE, 60, (1.0, 0.0), coupling, w=w)
    # a start outside the box is clamped into it
    x0 = (3.0 * rng.random((1, 6, 10)) - 1.0, 0.012 * rng.random((1, 6, 10)) - 3e-3)
    assert x0[0].min() < 0 and x0[0].max() > A.CASE_SMAX and x0[1].min() < 0 and x0[1].max() > A.CASE_ADCMAX
    _compare("x0 outside the box", y, *CASE, 60, w=w, x0=x0)


@pytest.mark.parametrize("H,W,f", ((7, 1024, (7, 1)), (1024, 3, (1, 3)), (9, 250, (3, 2))), ids=("7x1024by7x1", "1024x3by1x3", "9x250by3x2"))
def test_solver_matches_the_restatement_on_long_strides_and_a_one_block_axis(H, W, f):
    """C = 2.  The first two shapes walk the stride loops several times with one axis a single block (their H W and C h w ARE multiples
    of the 1,024 threads); in the third, H W = 2,250 and C h w = 750 are not, so the last pass of each loop is ragged."""
    rng = np.random.default_rng(H)
    b = np.array([0.0, 1000.0])
    k = rng.random(f) + 0.1
    k = k / k.sum()
    s_true, u_true = 0.2 + 0.8 * rng.random((2, H, W)), 0.5 + 2.5 * rng.random((2, H, W))
    y = T.apply_A(A.model(s_true, u_true, b / b.max()), k) + 0.02 * rng.standard_normal((2, 2, H // f[0], W // f[1]))
    w = rng.random(y.shape) * (rng.random(y.shape) > 0.1)
    assert (w == 0).any()
    _compare(f"2 x {H}x{W} {f} random kernel, random weights", y, b, f, k, 0.02, 0.01, 40, box=(1.5, 6e-3, 1e-3), w=w)


# ---- independent of the restatement ---------------------------------------------------------------------------------------------------------
def test_zero_iterations_return_the_start_exactly():
    rng = np.random.default_rng(5)
    _, _, y, w = A.case_data()
    b_max = A.CASE_B.max()
    x0 = (A.CASE_SMAX * rng.random((1, 6, 10)), A.CASE_ADCMAX * rng.random((1, 6, 10)))
    s, adc, info = baselines.tv_superres_adc(y, *CASE, 0, A.CASE_MU, "joint", *BOX, weight=w, x0=x0, return_info=True)
    # the documented start: s as given, the ADC through its normalisation u = adc b_max and back (two correctly rounded operations)
    back = (x0[1] * b_max) / b_max
    print(f"n_iter = 0, x0 given: s == x0 {np.array_equal(s, x0[0])}, adc == (x0 b_max) / b_max {np.array_equal(adc, back)}, max|adc - x0| = "
          f"{np.abs(adc - x0[1]).max():.1e}, change {float(info['change'][0])}")
    assert np.array_equal(s, x0[0]) and np.array_equal(adc, back) and np.abs(adc - x0[1]).max() <= 2 ** -52 * A.CASE_ADCMAX
    assert float(info["change"][0]) == 0.0
    s, adc = baselines.tv_superres_adc(y, *CASE, 0, A.CASE_MU, "joint", *BOX)
    want = np.fmin(np.fmax(T.replicate(y[:, 0], A.CASE_FACTORS), 0.0), A.CASE_SMAX)
    print(f"n_iter = 0, default start: s == clamped replication of b = 0 {np.array_equal(s, want)}; adc == adc0 {np.unique(adc)}")
    assert np.array_equal(s, want) and np.array_equal(adc, np.full(s.shape, (A.CASE_ADC0 * b_max) / b_max))
    # the first channel of smallest b is the one replicated, wherever it stands
    order = [2, 0, 1]
    s2, _ = baselines.tv_superres_adc(y[:, order], A.CASE_B[order], A.CASE_FACTORS, "mean", A.CASE_LAM, A.CASE_ALPHA, 0, A.CASE_MU, "joint", *BOX)
    assert np.array_equal(s2, want)


def test_the_maps_stay_inside_the_box_and_attain_both_bounds():
    rng = np.random.default_rng(6)
    y = 4.0 * rng.random((4, 3, 6, 6)) - 1.5                                 # negative and oversized samples
    s, adc = baselines.tv_superres_adc(y, A.CASE_B, (2, 2), "mean", 1e-3, 0.01, 400, (1.0, 0.1), "joint", 1.5, 4e-3, 1e-3)
    print(f"data in [{y.min():.2f}, {y.max():.2f}]: s in [{s.min()}, {s.max()}], adc in [{adc.min()}, {adc.max()}]")
    assert np.isfinite(s).all() and np.isfinite(adc).all()
    assert s.min() == 0.0 and s.max() == 1.5 and adc.min() == 0.0 and adc.max() == 4e-3


def test_a_missing_datum_is_never_read_and_lambda_zero_stays_finite():
    _, _, y, w = A.case_data()
    start = A.start(y, A.CASE_B, A.CASE_FACTORS, *BOX)
    x0 = (start[0], start[1] / A.CASE_B.max())
    a = baselines.tv_superres_adc(y, *CASE, 30, A.CASE_MU, "joint", *BOX, weight=w, x0=x0, return_info=True)
    for value in (1e3, float("nan")):
        other = y.copy()
        other[w == 0] = value
        c = baselines.tv_superres_adc(other, *CASE, 30, A.CASE_MU, "joint", *BOX, weight=w, x0=x0, return_info=True)
        same = np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and np.array_equal(a[2]["energy"], c[2]["energy"]) and \
            np.array_equal(a[2]["change"], c[2]["change"])
        print(f"the w = 0 datum holds {value}: same bits {same}")
        assert (w == 0).sum() == 1 and np.isfinite(c[0]).all() and np.isfinite(c[1]).all() and np.isfinite(c[2]["energy"]).all() and same
    # lambda = 0: the dual prior phase is skipped, p = 0: the result is the one of any Huber parameter, finite
    s, adc, info = baselines.tv_superres_adc(y, A.CASE_B, A.CASE_FACTORS, "mean", 0.0, 0.0, 50, A.CASE_MU, "joint", *BOX, weight=w, return_info=True)
    s2, adc2, _ = baselines.tv_superres_adc(y, A.CASE_B, A.CASE_FACTORS, "mean", 0.0, 0.3, 50, (0.2, 0.9), "none", *BOX, weight=w, return_info=True)
    ws, wadc, we, _ = A.solve_adc(y, A.CASE_B, A.CASE_FACTORS, "mean", 0.0, 0.0, 50, A.CASE_MU, "joint", *BOX, w=w, return_info=True)
    print(f"lambda = 0, 50 iterations: finite {np.isfinite(s).all() and np.isfinite(adc).all()}, energy {float(info['energy'][0]):.6e} (restated "
          f"{float(we[0]):.6e}), independent of Huber, weights and coupling {np.array_equal(s, s2) and np.array_equal(adc, adc2)}")
    assert np.isfinite(s).all() and np.isfinite(adc).all() and np.isfinite(info["energy"]).all()
    assert np.array_equal(s, s2) and np.array_equal(adc, adc2)
    assert np.abs(s - ws).max() <= SOLVER_BOUND


@pytest.mark.parametrize("coupling", ("joint", "none"))
def test_energy_reaches_the_lbfgs_minimum_which_shares_nothing_with_the_iteration(coupling):
    _, _, y, w = A.case_data()
    minimum, _ = A.case_minimum(coupling)
    e_start = float(baselines.tv_superres_adc(y, *CASE, 0, A.CASE_MU, coupling, *BOX, weight=w, return_info=True)[2]["energy"][0])
    energy = float(baselines.tv_superres_adc(y, *CASE, 10000, A.CASE_MU, coupling, *BOX, weight=w, return_info=True)[2]["energy"][0])
    ratio = (energy - minimum) / (e_start - minimum)
    print(f"{coupling}: L-BFGS-B minimum {minimum:.12f}, energy at the start {e_start:.6f}, after 10,000 iterations {energy:.12f}: "
          f"(E - E*) / (E_start - E*) = {ratio:.2e} (bound 1e-6)")
    assert ratio <= 1e-6


# ---- bit for bit ------------------------------------------------------------------------------------------------------------------------
def test_a_batch_beyond_the_cu_count_equals_its_solitary_solves_bit_for_bit():
    """300 different groups of 2 x 12 x 12 maps from 2 x 6 x 4 data: more workgroups than the 256 CUs, so some are queued."""
    rng = np.random.default_rng(11)
    n, f, b = 300, (2, 3), (0.0, 1000.0)
    y = _dev(rng.random((n, 2, 6, 4)))
    w = _dev(rng.random((n, 2, 6, 4)) * (rng.random((n, 2, 6, 4)) > 0.1))
    args = (b, f, "mean", 0.02, 0.01, 25, (1.0, 0.1), "joint")
    s, adc, info = baselines.tv_superres_adc(y, *args, weight=w, return_info=True)
    torch.cuda.synchronize()
    differ = 0
    for i in range(n):
        s1, adc1, one = baselines.tv_superres_adc(y[i:i + 1], *args, weight=w[i:i + 1], return_info=True)
        differ += int(not (torch.equal(s1[0], s[i]) and torch.equal(adc1[0], adc[i]) and torch.equal(one["energy"][0], info["energy"][i])
                           and torch.equal(one["change"][0], info["change"][i])))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s_side, adc_side, side_info = baselines.tv_superres_adc(y, *args, weight=w, return_info=True)
    side.synchronize()
    distinct = len({s[i].cpu().numpy().tobytes() for i in range(n)})
    print(f"{n} groups of 2 maps 12x12: {differ} differ from their solitary solve; side stream equal "
          f"{torch.equal(s_side, s) and torch.equal(adc_side, adc)}; {distinct} distinct results")
    assert s.shape == adc.shape == (n, 12, 12) and distinct == n
    assert differ == 0
    assert torch.equal(s_side, s) and torch.equal(adc_side, adc) and torch.equal(side_info["energy"], info["energy"])


def test_fp32_is_the_fp64_result_rounded_once_and_types_come_back_as_given():
    rng = np.random.default_rng(9)
    _, _, y, w = A.case_data()
    y32, w32 = _dev(y, torch.float32), _dev(w, torch.float32)
    x32 = (_dev(rng.random((1, 6, 10)), torch.float32), _dev(4e-3 * rng.random((1, 6, 10)), torch.float32))
    for coupling in ("joint", "none"):
        args = (A.CASE_B, A.CASE_FACTORS, "mean", A.CASE_LAM, A.CASE_ALPHA, 100, A.CASE_MU, coupling, *BOX)
        s, adc, info = baselines.tv_superres_adc(y32, *args, weight=w32, x0=x32, return_info=True)
        ws, wadc, winfo = baselines.tv_superres_adc(y32.double(), *args, weight=w32.double(), x0=tuple(m.double() for m in x32), return_info=True)
        same = torch.equal(s, ws.float()) and torch.equal(adc, wadc.float())
        print(f"{coupling}: fp32 out == fp64 out rounded once: {same}")
        assert s.dtype == adc.dtype == torch.float32 and ws.dtype == torch.float64 and s.is_cuda and info["energy"].dtype == torch.float64
        assert same
        assert torch.equal(info["energy"], winfo["energy"]) and torch.equal(info["change"], winfo["change"])
    # leading axes are a batch of groups and keep their shape; ndarrays come back as float64 ndarrays
    stack = _dev(rng.random((2, 3, 4, 4, 6)), torch.float32)
    s, adc, info = baselines.tv_superres_adc(stack, (0.0, 150.0, 1000.0, 1500.0), (2, 1), n_iter=5, return_info=True)
    assert s.shape == adc.shape == (2, 3, 8, 6) and info["energy"].shape == info["change"].shape == (2, 3)
    s, adc = baselines.tv_superres_adc(rng.random((3, 4, 6)), (0.0, 500.0, 1000.0), (2, 2), n_iter=3)
    assert isinstance(s, np.ndarray) and isinstance(adc, np.ndarray) and s.dtype == adc.dtype == np.float64 and s.shape == (8, 12)
    # the model's images of two maps, on the device for tensors: fp64 inside, rounded once
    s64, adc64, bv = _dev(rng.random((2, 5, 7))), _dev(3e-3 * rng.random((2, 5, 7))), np.array([0.0, 150.0, 1500.0])
    images = baselines.adc_signal(s64, adc64, bv)
    want = A.model(s64.cpu().numpy(), adc64.cpu().numpy(), bv)
    err = float(np.abs(images.cpu().numpy() - want).max())
    images32 = baselines.adc_signal(s64.float(), adc64.float(), bv)
    print(f"adc_signal: max|device - numpy| = {err:.1e} (bound 1e-15); fp32 == fp64 of the fp32 maps rounded once "
          f"{torch.equal(images32, baselines.adc_signal(s64.float().double(), adc64.float().double(), bv).float())}")
    assert images.shape == (2, 3, 5, 7) and images.dtype == torch.float64 and images.is_cuda and err <= 1e-15
    assert images32.dtype == torch.float32 and torch.equal(images32, baselines.adc_signal(s64.float().double(), adc64.float().double(), bv).float())
    assert isinstance(baselines.adc_signal(rng.random((5, 7)), rng.random((5, 7)), bv), np.ndarray)


# ---- the study case on the device -----------------------------------------------------------------------------------------------------------
def test_the_study_case_on_the_device():
    hr, _, adc_true = A.study_truth()
    _, y, b = J.study_case(0)
    args = ((2, 2), "mean", baselines.ADC_DEFAULT_LAMBDA, baselines.ADC_DEFAULT_HUBER, baselines.ADC_DEFAULT_ITERS,
            baselines.ADC_DEFAULT_MAP_WEIGHTS, baselines.ADC_DEFAULT_COUPLING)
    s, adc = baselines.tv_superres_adc(y, b, *args)
    ws, wadc = A.solve_adc(y, b, *args)
    err_s, err_u = float(np.abs(s - ws).max()), float(np.abs(adc - wadc).max() * b.max())
    rows = {"tv_superres_adc (the maps)": A.map_scores(s, adc, hr, adc_true),
            "tv_superres (0.024, 0.01)": A.image_scores(baselines.tv_superres(y, (2, 2), "mean", 0.024, 0.01, 300), hr, adc_true),
            "tv_superres_joint (defaults)": A.image_scores(baselines.tv_superres_joint(y, (2, 2), "mean"), hr, adc_true)}
    print(f"study case, seed 0, the defaults {args[2:]}: max|s - restated| = {err_s:.3e}, max|u - restated| = {err_u:.3e} (bound "
          f"{SOLVER_BOUND:.0e})")
    for name, (p0, p_last, rmse) in rows.items():
        print(f"  {name}: b = 0 PSNR {p0:.2f} dB, b = 1500 PSNR {p_last:.2f} dB, ADC RMSE {rmse:.4e}")
    assert err_s <= SOLVER_BOUND and err_u <= SOLVER_BOUND


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------------------
def test_ops_wrapper_checks_before_it_launches(monkeypatch):
    y = torch.rand(2, 3, 3, 5, device="cuda", dtype=torch.float64)
    k = [[0.25, 0.25], [0.25, 0.25]]
    b = (0.0, 500.0, 1000.0)
    tail = (k, (1.0, 0.1), 0.01, 0.01, "joint", 3, 1.5, 4e-3, 1e-3)
    s, adc, energy, change = ops.tvadc_solve(y, b, (2, 2), *tail)
    assert s.shape == adc.shape == (2, 6, 10) and energy.shape == change.shape == (2,)
    need = ops.tvadc_workspace_doubles(2, 3, 6, 10, (2, 2))
    assert need == 2 * (8 * 60 + 3 * 15)
    calls = []
    real = _lib.lib().inr_tvadc_solve2d

    class Spy:
        def __getattr__(self, name):
            if name == "inr_tvadc_solve2d":
                return lambda *a: calls.append(name) or real(*a)
            return getattr(_lib.lib(), name)

    monkeypatch.setattr(ops, "lib", lambda: Spy())
    for text, change_args in (("contiguous", dict(y=y[:, :, :, ::2])), ("weight has shape", dict(weight=y[:1].contiguous())),
                              ("x0 has shape", dict(x0=y)), ("b has 2 b-values, expected one per channel \\(3\\)", dict(b=(0.0, 1000.0))),
                              ("b-values must be finite and >= 0", dict(b=(0.0, -1.0, 1000.0))), ("all equal", dict(b=(5.0, 5.0, 5.0))),
                              ("map_weights are", dict(mu=(1.0, 2.0))), ("coupling must be 'joint' or 'none'", dict(coupling=1)),
                              ("s_max must be finite and > 0", dict(s_max=0.0)), ("adc_max must be finite and > 0", dict(adc_max=float("inf"))),
                              ("adc0 must be within", dict(adc0=5e-3)), ("n_iter must be an integer >= 0", dict(n_iter=-1)),
                              (f"workspace must be a device float64 tensor of at least {need}",
                               dict(workspace=torch.empty(need - 1, device="cuda", dtype=torch.float64)))):
        a = dict(y=y, b=b, mu=(1.0, 0.1), coupling="joint", n_iter=3, s_max=1.5, adc_max=4e-3, adc0=1e-3, weight=None, x0=None, workspace=None)
        a.update(change_args)
        with pytest.raises(ValueError, match=text):
            ops.tvadc_solve(a["y"], a["b"], (2, 2), k, a["mu"], 0.01, 0.01, a["coupling"], a["n_iter"], a["s_max"], a["adc_max"], a["adc0"],
                            a["weight"], a["x0"], a["workspace"])
    with pytest.raises(TypeError, match="float32 or torch.float64"):
        ops.tvadc_solve(y.half(), b, (2, 2), *tail)
    print(f"refusals reached the C entry {len(calls)} times (expected 0)")
    assert calls == []
    ws = torch.empty(need, device="cuda", dtype=torch.float64)
    again = ops.tvadc_solve(y, b, (2, 2), *tail, workspace=ws)
    assert calls == ["inr_tvadc_solve2d"] and torch.equal(again[0], s) and torch.equal(again[1], adc)


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------
TIMINGS = ("t_fit_s", "t_recon_s", "train_voxels_per_s")        # wall-clock: the only values two runs of one command do not share
ADC_KEYS = {"psnr_tv_adc_db", "ssim_tv_adc_mean", "tv_adc_consistency_psnr_db"}


def _four_b_volume(path):
    """The synthetic four-b volume of test_gpu_tvj.py's driver test: maxes per b-value, so the driver rescales the channels."""
    rng = np.random.default_rng(3)
    bvals = np.array([0.0, 150.0, 1000.0, 1500.0])
    gx, gy, gz = np.meshgrid(np.linspace(0, 1, 32), np.linspace(0, 1, 32), np.linspace(0, 1, 2), indexing="ij")
    vol = np.stack([500 * (1.2 + np.sin(3 * gx + gz) * np.cos(2 * gy)) * np.exp(-0.7 * b) for b in range(4)], axis=-1)
    vol *= 1 + 0.02 * rng.standard_normal(vol.shape)
    matio.savemat(path, {"vol": vol, "b": bvals})
    return bvals


def test_superresDWI_tv_adc(tmp_path):
    path = str(tmp_path / "pat068_vol.mat")
    bvals = _four_b_volume(path)
    common = ["--data", path, "--number_of_epochs", "5", "--hidden_dim", "128", "--num_layers", "2", "--mapping_size", "32", "--roi_start",
              "2", "--roi_end", "30", "--seed", "0", "--adc", "--tv_baseline", "--tv_lambda", "2e-3", "--tv_huber", "0.05", "--tv_iters", "80"]
    model = ["--tv_adc", "--tv_adc_lambda", "0.004", "--tv_adc_weight", "0.2", "--tv_adc_iters", "120"]
    out_plain, out = str(tmp_path / "plain"), str(tmp_path / "model")
    res_plain = dwi_script.main(common + ["--output_address", out_plain])[0]
    res = dwi_script.main(common + model + ["--output_address", out])[0]
    d_plain, d = os.path.join(out_plain, "pat068"), os.path.join(out, "pat068")
    # a direct call on the LR stack the driver forms, in the signal's own units
    mean_img, _, _, _, scale = dwi_script.load_input_and_scale(path)
    hs = torch.from_numpy(np.ascontiguousarray(mean_img[2:30, 2:30], dtype=np.float32)).cuda().permute(2, 3, 0, 1).contiguous()
    ls = hs[:, :, ::2, ::2].contiguous()
    sc = torch.as_tensor(scale.astype(np.float32), device="cuda")
    rel = (sc / sc.max())[None, :, None, None]
    s0, adc_map = baselines.tv_superres_adc((ls * rel).contiguous(), bvals.tolist(), (2, 2), "decimate", 0.004, baselines.ADC_DEFAULT_HUBER, 120,
                                            (1.0, 0.2))
    images = (baselines.adc_signal(s0.contiguous(), adc_map.contiguous(), bvals.tolist()) / rel).contiguous()
    adc = matio.loadmat(os.path.join(d, "adc.mat"))
    m = json.load(open(os.path.join(d, "metrics.json")))
    rows = reports.read_csv(os.path.join(d, "ssim_scores.csv"))
    arows = reports.read_csv(os.path.join(d, "ssim_scores_tv_adc.csv"))
    floor = lambda t: t.clamp_min(1e-30)
    want_ssim = metrics.ssim_reference_protocol(floor(hs), floor(images)).cpu().numpy().reshape(-1)
    col = np.array([float(r["SSIM-tv-adc"]) for r in arows])
    want_psnr = float(metrics.psnr(hs, images, 1.0))
    print(f"--tv_adc: psnr_tv_adc_db {m['psnr_tv_adc_db']:.3f} (direct {want_psnr:.3f}), psnr_tv_db {m['psnr_tv_db']:.3f}, ssim_tv_adc_mean "
          f"{m['ssim_tv_adc_mean']:.4f}, tv_adc_consistency_psnr_db {m['tv_adc_consistency_psnr_db']:.2f}, adc_tv_adc median "
          f"{np.median(adc['adc_tv_adc']):.3e} in [{adc['adc_tv_adc'].min():.2e}, {adc['adc_tv_adc'].max():.2e}], s0_tv_adc max {adc['s0_tv_adc'].max():.1f}")
    assert open(os.path.join(d, "ssim_scores_tv_adc.csv")).readline() == reports.SSIM_TV_ADC_HEADER
    assert len(arows) == len(rows) == 8 and set(arows[0]) == {"Pt_id", "b-value", "slice", "SSIM-tv-adc", "SSIM-SR"}
    for key in ("Pt_id", "b-value", "slice", "SSIM-SR"):
        assert [r[key] for r in arows] == [r[key] for r in rows], key
    assert np.array_equal(col, want_ssim) and m["ssim_tv_adc_mean"] == pytest.approx(col.mean())
    assert m["psnr_tv_adc_db"] == want_psnr == res["psnr_tv_adc_db"]
    assert m["tv_adc_consistency_psnr_db"] == float(metrics.psnr(ls, baselines.block_apply(images, (2, 2), "decimate"), 1.0))
    # the solver's own map, not a log-linear fit of its images: non-negative, bounded, no NaN
    assert adc["adc_tv_adc"].shape == adc["s0_tv_adc"].shape == (28, 28, 2)
    assert np.array_equal(adc["adc_tv_adc"], adc_map.permute(1, 2, 0).cpu().numpy())
    assert np.array_equal(adc["s0_tv_adc"], (s0 * float(sc.max())).permute(1, 2, 0).cpu().numpy())
    assert adc["adc_tv_adc"].min() >= 0.0 and adc["adc_tv_adc"].max() <= baselines.ADC_DEFAULT_ADC_MAX
    # without --tv_adc: every file and key is what it was, byte for byte, apart from the wall-clock values
    plain = json.load(open(os.path.join(d_plain, "metrics.json")))
    assert set(m) - set(plain) == ADC_KEYS and not [k for k in list(plain) + list(res_plain) if "tv_adc" in k]
    strip = lambda s: json.dumps({k: v for k, v in s.items() if k not in TIMINGS and k not in ADC_KEYS}, indent=1).encode()
    assert strip(plain) == strip(m)
    assert list(plain) == [k for k in m if k not in ADC_KEYS]
    assert sorted(os.listdir(d)) == sorted(os.listdir(d_plain) + ["ssim_scores_tv_adc.csv"])
    for name in ("recon.npy", "ssim_scores.csv", "ssim_scores_tv.csv"):
        assert open(os.path.join(d_plain, name), "rb").read() == open(os.path.join(d, name), "rb").read(), name
    adc_plain = matio.loadmat(os.path.join(d_plain, "adc.mat"))
    assert set(adc) - set(adc_plain) == {"adc_tv_adc", "s0_tv_adc"}
    for key in adc_plain:
        if not key.startswith("__"):
            assert np.array_equal(adc_plain[key], adc[key], equal_nan=True), key


def test_joint_bvalues_with_the_adc_model_on_pat07(tmp_path, golden):
    vol = golden("pat07_volume.npz")["vol"]
    path = str(tmp_path / "pat07_mean_b0.mat")
    matio.savemat(path, {"data_mean_b0": vol})
    which = [10, 14, 18]
    base = ["--data", path, "--synthetic_adc", "--slices", "10", "14", "18", "--tv_iters", "100", "--tv_lambda", "0.012"]
    out_plain, out = str(tmp_path / "plain"), str(tmp_path / "model")
    jb_script.main(base + ["--output_address", out_plain])
    res = jb_script.main(base + ["--output_address", out, "--with_adc_model", "--tv_adc_iters", "400"])[0]
    d_plain, d = os.path.join(out_plain, "pat07"), os.path.join(out, "pat07")
    m, plain = json.load(open(os.path.join(d, "metrics.json"))), json.load(open(os.path.join(d_plain, "metrics.json")))
    rows, prows = reports.read_csv(os.path.join(d, "joint_bvalues.csv")), reports.read_csv(os.path.join(d_plain, "joint_bvalues.csv"))
    mat, pmat = matio.loadmat(os.path.join(d, "joint_bvalues.mat")), matio.loadmat(os.path.join(d_plain, "joint_bvalues.mat"))
    # a direct call on the data the driver forms
    mean_img = dwi_script.load_input_and_scale(path)[0]
    roi = np.ascontiguousarray(mean_img[40:90, 40:90].transpose(2, 3, 0, 1), dtype=np.float64)[which][:, 0]
    hr = drivers.synthetic_decay(roi / roi.max())
    eta = np.stack([0.02 * np.random.default_rng(z).standard_normal((4, 25, 25)) for z in which])
    y = baselines.block_apply(_dev(hr), (2, 2), "mean") + _dev(eta)
    s0, adc = baselines.tv_superres_adc(y, A.STUDY_B.tolist(), (2, 2), "mean", n_iter=400)
    images = baselines.adc_signal(s0.contiguous(), adc.contiguous(), A.STUDY_B.tolist())
    f32 = lambda t: t.float().contiguous()
    want_psnr = metrics.psnr(f32(_dev(hr)), f32(images), 1.0, per_image=True).cpu().numpy().reshape(-1)
    mask = hr[:, 0] > 0.25 * hr[:, 0].max()
    want_rmse = float(np.sqrt(np.mean((adc.cpu().numpy() - mat["adc_hr"].transpose(2, 0, 1))[mask] ** 2)))
    print("joint_bvalues --with_adc_model on pat07 (synthetic ADC, 400 iterations of the model): " + ", ".join(
        f"{name}: b = 0 {m[f'psnr_{name}_b0_db']:.2f} dB, b = 1500 {m[f'psnr_{name}_b1500_db']:.2f} dB, ADC RMSE {m[f'adc_rmse_{name}']:.3e}"
        for name in m["methods"]) + f"; log-linear fit of the model's images {m['adc_rmse_loglinear_tv_adc']:.3e}")
    assert m["methods"] == list(drivers.JOINT_METHODS) + ["tv_adc"] == list(res["methods"]) and plain["methods"] == list(drivers.JOINT_METHODS)
    assert np.array_equal(np.array([float(r["PSNR-tv_adc"]) for r in rows]), want_psnr)
    assert np.array_equal(mat["adc_tv_adc"], adc.cpu().numpy().transpose(1, 2, 0)) and np.array_equal(mat["s0_tv_adc"], s0.cpu().numpy().transpose(1, 2, 0))
    assert np.array_equal(mat["tv_adc"], images.cpu().numpy().transpose(2, 3, 0, 1))
    assert m["adc_rmse_tv_adc"] == pytest.approx(want_rmse, rel=1e-12) and np.isfinite(m["adc_rmse_loglinear_tv_adc"])
    assert mat["adc_loglinear_tv_adc"].shape == (50, 50, 3)
    # the other rows are bit-equal to a run without the flag
    new_keys = {k for k in m if "tv_adc" in k}
    assert set(m) - set(plain) == new_keys and {k: v for k, v in m.items() if k not in new_keys and k != "methods"} == \
        {k: v for k, v in plain.items() if k != "methods"}
    for r, p in zip(rows, prows):
        assert {k: v for k, v in r.items() if k not in ("SSIM-tv_adc", "PSNR-tv_adc")} == p
    assert len(rows) == len(prows) == 12
    for key in pmat:
        if not key.startswith("__"):
            assert np.array_equal(pmat[key], mat[key], equal_nan=True), key
    assert set(mat) - set(pmat) == {"tv_adc", "adc_tv_adc", "s0_tv_adc", "adc_loglinear_tv_adc"}
