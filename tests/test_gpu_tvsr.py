"""GPU: the TV / Huber super-resolution baseline of csrc/tvsr.hip against its float64 restatement (tests/tvsr_common.py), against
properties that do not depend on the restatement, across a batch, and through ``superresDWI --tv_baseline``.

Bounds are derived, not measured.  A / A^T in fp64 carry the project's 1e-12 of max(max|in|, max|want|).  The solver carries 1e-10
absolute on data in [0, 1] for up to 1,000 iterations: the iteration is non-expansive, about ten roundings of 1.1e-16 per pixel and
iteration give 1e-12, and the bound leaves two orders of margin.  fp32 in and out is the fp64 result of the same (fp32) data rounded
once, bit for bit.  ``energy`` is a sum of at most H W + h w non-negative terms of a few roundings each: 1e-12 relative.  Every
test prints what it measured before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

from tests import tvsr_common as T
from mri_super_resolution_amd import baselines, matio, metrics, ops, reports
from mri_super_resolution_amd.scripts import superresDWI as dwi_script

pytestmark = pytest.mark.gpu

SOLVER_BOUND = 1e-10
OPERATOR_SHAPES = ((6, 10, (3, 2)), (8, 8, (1, 1)), (16, 24, (8, 8)), (50, 50, (2, 2)))


def _kernels(f, rng):
    k = rng.random(f) + 0.1
    return {"mean": "mean", "decimate": "decimate", "random": k / k.sum()}


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


@pytest.mark.parametrize("H,W,f", OPERATOR_SHAPES, ids=[f"{H}x{W}by{f[0]}x{f[1]}" for H, W, f in OPERATOR_SHAPES])
def test_block_operator_and_adjoint_match_the_restatement_and_each_other(H, W, f):
    rng = np.random.default_rng(H * W)
    x, r = rng.standard_normal((3, H, W)), rng.standard_normal((3, H // f[0], W // f[1]))
    for name, kernel in _kernels(f, rng).items():
        k = T.block_kernel(kernel, f)
        got_a, got_t = baselines.block_apply(x, f, kernel), baselines.block_adjoint(r, f, kernel)
        want_a, want_t = T.apply_A(x, k), T.apply_AT(r, k)
        err_a, tol_a = np.abs(got_a - want_a).max(), 1e-12 * max(np.abs(x).max(), np.abs(want_a).max())
        err_t, tol_t = np.abs(got_t - want_t).max(), 1e-12 * max(np.abs(r).max(), np.abs(want_t).max())
        dot_a, dot_t = float((got_a * r).sum()), float((x * got_t).sum())
        scale = float(np.abs(got_a * r).sum())
        print(f"{H}x{W} {f} {name}: |A - want| {err_a:.2e} (bound {tol_a:.2e}), |A^T - want| {err_t:.2e} (bound {tol_t:.2e}), "
              f"|<Ax, r> - <x, A^T r>| / sum|.| {abs(dot_a - dot_t) / scale:.2e}")
        assert got_a.dtype == got_t.dtype == np.float64 and got_a.shape == want_a.shape and got_t.shape == want_t.shape
        assert err_a <= tol_a and err_t <= tol_t
        assert abs(dot_a - dot_t) <= 1e-12 * scale
        # device tensors come back as what they were; fp32 is the fp64 result rounded once
        x32 = _dev(x, torch.float32)
        got32 = baselines.block_apply(x32, f, kernel)
        assert got32.dtype == torch.float32 and torch.equal(got32, baselines.block_apply(x32.double(), f, kernel).float())
        assert baselines.block_adjoint(_dev(r), f, kernel).dtype == torch.float64


def _compare(name, y, f, kernel, lam, alpha, n_iter, w=None, x0=None):
    got, info = baselines.tv_superres(y, f, kernel, lam, alpha, n_iter, weight=w, x0=x0, return_info=True)
    want, energy, change = T.solve(y, f, kernel, lam, alpha, n_iter, w=w, x0=x0, return_info=True)
    err = float(np.abs(got - want).max())
    e_rel = float(np.abs(info["energy"] - energy).max() / np.abs(energy).max())
    c_err = float(np.abs(info["change"] - change).max())
    print(f"{name}, {n_iter} iterations: max|got - restated| = {err:.3e} (bound {SOLVER_BOUND:.0e}), "
          f"energy against the restated run's (not asserted here) {e_rel:.2e}, "
          f"|change - restated| {c_err:.2e} (change {float(change.max()):.2e})")
    assert got.dtype == np.float64 and got.shape == want.shape
    assert err <= SOLVER_BOUND
    assert c_err <= 2 * SOLVER_BOUND            # the difference of two images that are each within the bound
    return got, info


@pytest.mark.parametrize("n_iter", (1, 2, 300))
def test_solver_matches_the_restatement_on_the_weighted_huber_case(n_iter):
    _, y = T.case_data()
    _compare("6x10 (3, 2) mean, weighted Huber", y, T.CASE_FACTORS, "mean", T.CASE_LAM, T.CASE_ALPHA, n_iter, w=T.CASE_W)


@pytest.fixture(scope="module")
def slice14():
    return T.pat07_roi()[14:15]


@pytest.mark.parametrize("kernel", ("mean", "decimate"))
@pytest.mark.parametrize("alpha", (0.0, 0.1), ids=("tv", "huber"))
def test_solver_matches_the_restatement_on_a_pat07_slice(slice14, alpha, kernel):
    y = T.apply_A(slice14, T.block_kernel(kernel, (2, 2)))
    got, _ = _compare(f"pat07 slice 14, 50x50 (2, 2) {kernel}, alpha {alpha}", y, (2, 2), kernel, 1e-3, alpha, 300)
    print(f"    PSNR {T.psnr(slice14, got):.2f} dB, block replication {T.psnr(slice14, T.replicate(y, (2, 2))):.2f} dB")


@pytest.mark.parametrize("H,W,f", ((7, 1024, (7, 1)), (1024, 3, (1, 3))), ids=("7x1024by7x1", "1024x3by1x3"))
def test_solver_matches_the_restatement_on_ragged_strides_and_a_one_block_axis(H, W, f):
    """H W is no multiple of the 1,024 threads and one axis is a single block (7 x 1024) or a single pixel per block (1024 x 3)."""
    rng = np.random.default_rng(H)
    hr = rng.random((2, H, W))
    for name, kernel in _kernels(f, rng).items():
        y = T.apply_A(hr, T.block_kernel(kernel, f))
        w = rng.random(y.shape) * (rng.random(y.shape) > 0.1)
        _compare(f"{H}x{W} {f} {name}", y, f, kernel, 0.02, 0.05, 40, w=w, x0=rng.random(hr.shape))
    _compare(f"{H}x{W} {f} mean, plain TV", T.apply_A(hr, T.block_kernel("mean", f)), f, "mean", 0.02, 0.0, 40)


def test_energy_reaches_the_lbfgs_minimum_which_shares_nothing_with_the_iteration():
    hr, y = T.case_data()
    minimum = T.lbfgs_minimum(y, T.block_kernel("mean", T.CASE_FACTORS), T.CASE_LAM, T.CASE_ALPHA, T.CASE_W, hr.shape)
    _, info = baselines.tv_superres(y, T.CASE_FACTORS, "mean", T.CASE_LAM, T.CASE_ALPHA, 300, weight=T.CASE_W, return_info=True)
    gap = (float(info["energy"][0]) - minimum) / minimum
    print(f"L-BFGS-B minimum {minimum:.12f}, energy after 300 iterations {float(info['energy'][0]):.12f}, relative gap {gap:.2e}")
    assert abs(gap) <= 1e-9


def test_properties_that_do_not_depend_on_the_restatement():
    rng = np.random.default_rng(5)
    hr, y = T.case_data()
    f = T.CASE_FACTORS
    # lambda = 0: the replication start satisfies the data and stays, exactly
    for kernel in ("mean", "decimate"):
        yk = baselines.block_apply(hr, f, kernel)
        for n_iter in (1, 50):
            x, info = baselines.tv_superres(yk, f, kernel, 0.0, 0.0, n_iter, return_info=True)
            res = float(np.abs(baselines.block_apply(x, f, kernel) - yk).max())
            print(f"lambda = 0, {kernel}, {n_iter} iterations: x == x0 {np.array_equal(x, T.replicate(yk, f))}, max|A x - y| = {res:.2e}, "
                  f"energy {float(info['energy'][0]):.2e}, change {float(info['change'][0]):.2e}")
            assert np.array_equal(x, T.replicate(yk, f))
            assert res <= 1e-15
    # n_iter = 0 returns x0: the given one, or the block replication
    x0 = rng.random(hr.shape)
    x, info = baselines.tv_superres(y, f, "mean", 0.05, 0.02, 0, x0=x0, return_info=True)
    assert np.array_equal(x, x0) and float(info["change"][0]) == 0.0
    assert np.array_equal(baselines.tv_superres(y, f, "mean", 0.05, 0.02, 0), T.replicate(y, f))
    # a missing datum (w = 0) is never read: whatever y holds there, the same bits come out
    w = T.CASE_W
    other = y.copy()
    other[w == 0] = 1e3
    a, ia = baselines.tv_superres(y, f, "mean", T.CASE_LAM, T.CASE_ALPHA, 30, weight=w, return_info=True)
    b, ib = baselines.tv_superres(other, f, "mean", T.CASE_LAM, T.CASE_ALPHA, 30, weight=w, x0=T.replicate(y, f), return_info=True)
    assert (w == 0).sum() == 1 and np.array_equal(a, b) and np.array_equal(ia["energy"], ib["energy"])
    # energy is the restated objective at the returned image
    for alpha in (0.0, T.CASE_ALPHA):
        x, info = baselines.tv_superres(y, f, "mean", T.CASE_LAM, alpha, 30, weight=w, return_info=True)
        want = T.energy(x, y, T.block_kernel("mean", f), T.CASE_LAM, alpha, w)
        rel = float(np.abs(info["energy"] - want).max() / np.abs(want).max())
        print(f"alpha {alpha}: energy {float(info['energy'][0]):.12f}, restated at the returned image {float(want[0]):.12f}, relative {rel:.2e}")
        assert rel <= 1e-12
    # (1, 1) is denoising: one datum per pixel
    noisy = np.clip(hr + 0.05 * rng.standard_normal(hr.shape), 0, 1)
    _compare("6x10 (1, 1) denoising", noisy, (1, 1), "mean", 0.05, 0.0, 60)


def test_fp32_is_the_fp64_result_rounded_once_and_types_come_back_as_given(slice14):
    rng = np.random.default_rng(9)
    cases = []
    hr, y = T.case_data()
    cases.append(("6x10 weighted, x0 given", y, T.CASE_FACTORS, "mean", T.CASE_LAM, T.CASE_ALPHA, 100, T.CASE_W, rng.random(hr.shape)))
    cases.append(("pat07 slice 14 decimate", T.apply_A(slice14, T.block_kernel("decimate", (2, 2))), (2, 2), "decimate", 1e-3, 0.0, 100,
                  None, None))
    for name, y, f, kernel, lam, alpha, n_iter, w, x0 in cases:
        y32 = _dev(y, torch.float32)
        w32 = None if w is None else _dev(w, torch.float32)
        x32 = None if x0 is None else _dev(x0, torch.float32)
        up = lambda t: None if t is None else t.double()
        got, info = baselines.tv_superres(y32, f, kernel, lam, alpha, n_iter, weight=w32, x0=x32, return_info=True)
        want, winfo = baselines.tv_superres(y32.double(), f, kernel, lam, alpha, n_iter, weight=up(w32), x0=up(x32), return_info=True)
        same = torch.equal(got, want.float())
        print(f"{name}: fp32 out == fp64 out rounded once: {same}; max|fp32 - fp64| = {float((got.double() - want).abs().max()):.2e}")
        assert got.dtype == torch.float32 and want.dtype == torch.float64 and got.is_cuda and info["energy"].dtype == torch.float64
        assert same
        assert torch.equal(info["energy"], winfo["energy"]) and torch.equal(info["change"], winfo["change"])
    # leading axes are a batch and keep their shape
    stack = _dev(rng.random((2, 3, 4, 6)), torch.float32)
    out, info = baselines.tv_superres(stack, (2, 1), n_iter=5, return_info=True)
    assert out.shape == (2, 3, 8, 6) and info["energy"].shape == info["change"].shape == (2, 3)
    assert isinstance(baselines.tv_superres(rng.random((4, 6)), (2, 2), n_iter=3), np.ndarray)


def test_a_batch_beyond_the_cu_count_equals_its_solitary_solves_bit_for_bit():
    """300 different 12 x 12 images: more workgroups than the 256 CUs, so some are queued behind others."""
    rng = np.random.default_rng(11)
    n, f = 300, (2, 3)
    y = _dev(rng.random((n, 6, 4)))
    w = _dev(rng.random((n, 6, 4)) * (rng.random((n, 6, 4)) > 0.1))
    args = (f, "mean", 0.02, 0.05, 25)
    out, info = baselines.tv_superres(y, *args, weight=w, return_info=True)
    torch.cuda.synchronize()
    differ = 0
    for i in range(n):
        one, one_info = baselines.tv_superres(y[i:i + 1], *args, weight=w[i:i + 1], return_info=True)
        differ += int(not (torch.equal(one[0], out[i]) and torch.equal(one_info["energy"][0], info["energy"][i])
                           and torch.equal(one_info["change"][0], info["change"][i])))
    again, again_info = baselines.tv_superres(y, *args, weight=w, return_info=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side, side_info = baselines.tv_superres(y, *args, weight=w, return_info=True)
    side.synchronize()
    distinct = len({out[i].cpu().numpy().tobytes() for i in range(n)})
    print(f"{n} images of 12x12: {differ} differ from their solitary solve; second run equal {torch.equal(again, out)}; side stream equal "
          f"{torch.equal(on_side, out)}; {distinct} distinct results")
    assert out.shape == (n, 12, 12) and distinct == n
    assert differ == 0
    assert torch.equal(again, out) and torch.equal(again_info["energy"], info["energy"]) and torch.equal(again_info["change"], info["change"])
    assert torch.equal(on_side, out) and torch.equal(side_info["energy"], info["energy"])


def test_ops_wrappers_check_before_they_launch():
    y = torch.rand(2, 3, 5, device="cuda", dtype=torch.float64)
    k = [[0.25, 0.25], [0.25, 0.25]]
    out, energy, change = ops.tvsr_solve(y, (2, 2), k, 0.01, 0.0, 3)
    assert out.shape == (2, 6, 10) and energy.shape == change.shape == (2,)
    assert torch.equal(ops.block_apply(ops.block_adjoint(y, (2, 2), k), (2, 2), k), 0.25 * y)
    with pytest.raises(ValueError, match="contiguous"):
        ops.tvsr_solve(y[:, :, ::2], (2, 2), k, 0.01, 0.0, 3)
    with pytest.raises(TypeError, match="float32 or torch.float64|float64"):
        ops.tvsr_solve(y.half(), (2, 2), k, 0.01, 0.0, 3)
    with pytest.raises(ValueError, match="weight has shape"):
        ops.tvsr_solve(y, (2, 2), k, 0.01, 0.0, 3, weight=y[:1].contiguous())
    with pytest.raises(ValueError, match="sum to 1"):
        ops.tvsr_solve(y, (2, 2), [[1.0, 1.0], [1.0, 1.0]], 0.01, 0.0, 3)
    with pytest.raises(ValueError, match="workspace must be a device float64 tensor of at least 480"):
        ops.tvsr_solve(y, (2, 2), k, 0.01, 0.0, 3, workspace=torch.empty(479, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="n_iter must be an integer >= 0"):
        ops.tvsr_solve(y, (2, 2), k, 0.01, 0.0, -1)


TIMINGS = ("t_fit_s", "t_recon_s", "train_voxels_per_s")        # wall-clock: the only values two runs of one command do not share
TV_KEYS = {"psnr_tv_db", "ssim_tv_mean", "tv_consistency_psnr_db"}


@pytest.fixture(scope="module")
def tv_runs(tmp_path_factory, golden):
    """superresDWI on pat07 as test_superresDWI_entry_point_on_pat07 sets it up: without the flag, with it under both LR models, and
    with --zerofill beside it."""
    tmp = tmp_path_factory.mktemp("tv")
    vol = golden("pat07_volume.npz")["vol"]
    path = str(tmp / "pat07_mean_b0.mat")
    matio.savemat(path, {"data_mean_b0": vol})
    common = ["--data", path, "--number_of_epochs", "20", "--seed", "0", "--roi_start", "40", "--roi_end", "90"]
    runs = {"plain": [], "tv": ["--tv_baseline"], "tv_zerofill": ["--tv_baseline", "--zerofill", "--tv_huber", "0", "--tv_iters", "100"],
            "tv_average": ["--tv_baseline", "--lr_model", "average", "--tv_lambda", "1e-3"]}
    out = {}
    for name, flags in runs.items():
        res = dwi_script.main(common + ["--output_address", str(tmp / name)] + flags)[0]
        out[name] = (os.path.join(str(tmp), name, "pat07"), res)
    return vol, out


def _hr_stack(vol):
    hr = torch.from_numpy(np.ascontiguousarray((vol / vol.max())[40:90, 40:90], dtype=np.float32)).cuda()[..., None]
    return hr.permute(2, 3, 0, 1).contiguous()                      # [Z, B, X, Y] as the driver forms it


@pytest.mark.parametrize("run,kernel,lam,alpha,n_iter", (("tv", "decimate", baselines.TV_DEFAULT_LAMBDA, baselines.TV_DEFAULT_HUBER,
                                                          baselines.TV_DEFAULT_ITERS),
                                                         ("tv_zerofill", "decimate", baselines.TV_DEFAULT_LAMBDA, 0.0, 100),
                                                         ("tv_average", "mean", 1e-3, baselines.TV_DEFAULT_HUBER,
                                                          baselines.TV_DEFAULT_ITERS)), ids=("decimate", "zerofill", "average"))
def test_superresDWI_tv_baseline_on_pat07(tv_runs, run, kernel, lam, alpha, n_iter):
    vol, runs = tv_runs
    d, res = runs[run]
    hs = _hr_stack(vol)
    ls = hs[:, :, ::2, ::2].contiguous() if kernel == "decimate" else hs.reshape(28, 1, 25, 2, 25, 2).mean(dim=(3, 5)).contiguous()
    rows = reports.read_csv(os.path.join(d, "ssim_scores.csv"))
    trows = reports.read_csv(os.path.join(d, "ssim_scores_tv.csv"))
    assert open(os.path.join(d, "ssim_scores_tv.csv")).readline() == "Pt_id, b-value, slice, SSIM-tv, SSIM-SR\n"
    assert len(trows) == len(rows) == 28 and set(trows[0]) == {"Pt_id", "b-value", "slice", "SSIM-tv", "SSIM-SR"}
    for key in ("Pt_id", "b-value", "slice", "SSIM-SR"):
        assert [r[key] for r in trows] == [r[key] for r in rows], key
    if kernel == "mean":       # the driver's block means are footprint.block_means of the float64 ROI, rounded to fp32
        from mri_super_resolution_amd import footprint as footprint_mod
        lr = footprint_mod.block_means((vol.astype(np.float64) / vol.max())[40:90, 40:90][..., None])
        ls = torch.from_numpy(np.ascontiguousarray(lr, dtype=np.float32)).cuda().permute(2, 3, 0, 1).contiguous()
    tv = baselines.tv_superres(ls, (2, 2), kernel, lam, alpha, n_iter)
    m = json.load(open(os.path.join(d, "metrics.json")))
    want_psnr = float(metrics.psnr(hs, tv, 1.0))
    floor = lambda t: t.clamp_min(1e-30)
    want_ssim = np.array([float(v) for v in metrics.ssim_reference_protocol(floor(hs), floor(tv)).cpu().numpy()[:, 0]])
    col = np.array([float(r["SSIM-tv"]) for r in trows])
    print(f"{run}: psnr_tv_db {m['psnr_tv_db']:.3f} (direct {want_psnr:.3f}), psnr_spline_db {m['psnr_spline_db']:.3f}, psnr_db "
          f"{m['psnr_db']:.3f}, ssim_tv_mean {m['ssim_tv_mean']:.4f}, tv_consistency_psnr_db {m['tv_consistency_psnr_db']:.2f}")
    assert m["psnr_tv_db"] == want_psnr == res["psnr_tv_db"]
    assert np.array_equal(col, want_ssim) and m["ssim_tv_mean"] == pytest.approx(col.mean())
    assert np.isfinite(m["tv_consistency_psnr_db"])
    assert m["tv_consistency_psnr_db"] == float(metrics.psnr(ls, baselines.block_apply(tv, (2, 2), kernel), 1.0))
    assert "ssim_scores_zerofill.csv" in os.listdir(d) if run == "tv_zerofill" else "ssim_scores_zerofill.csv" not in os.listdir(d)


def test_superresDWI_without_the_flag_writes_what_it_wrote(tv_runs):
    """The run without --tv_baseline against the run with it, same seed: ssim_scores.csv byte for byte, metrics.json byte for byte once
    the wall-clock values, which no two runs share, and the three new keys are set aside; no TV file and no TV key without the flag."""
    _, runs = tv_runs
    (d_plain, res_plain), (d, res) = runs["plain"], runs["tv"]
    assert open(os.path.join(d_plain, "ssim_scores.csv"), "rb").read() == open(os.path.join(d, "ssim_scores.csv"), "rb").read()
    plain, m = json.load(open(os.path.join(d_plain, "metrics.json"))), json.load(open(os.path.join(d, "metrics.json")))
    assert set(m) - set(plain) == TV_KEYS and not [k for k in list(plain) + list(res_plain) if "tv" in k]
    strip = lambda s: json.dumps({k: v for k, v in s.items() if k not in TIMINGS and k not in TV_KEYS}, indent=1).encode()
    assert strip(plain) == strip(m)
    assert list(plain) == [k for k in m if k not in TV_KEYS]            # the order of the keys too
    assert not [name for name in os.listdir(d_plain) if "tv" in name]
    assert sorted(os.listdir(d)) == sorted(os.listdir(d_plain) + ["ssim_scores_tv.csv"])
    for name in ("recon.npy", "ssim_scores.csv"):
        assert open(os.path.join(d_plain, name), "rb").read() == open(os.path.join(d, name), "rb").read(), name


def test_superresDWI_tv_baseline_adds_its_adc_map_and_goes_with_wire(tmp_path):
    """--tv_baseline --adc on a plain four-b volume: adc_tv is the ADC of the TV reconstruction, on the grid of the HR ROI; the flag
    does not touch the fit, so --model wire takes it too."""
    rng = np.random.default_rng(3)
    bvals = np.array([0.0, 150.0, 1000.0, 1500.0])
    gx, gy, gz = np.meshgrid(np.linspace(0, 1, 32), np.linspace(0, 1, 32), np.linspace(0, 1, 2), indexing="ij")
    vol = np.stack([500 * (1.2 + np.sin(3 * gx + gz) * np.cos(2 * gy)) * np.exp(-0.7 * b) for b in range(4)], axis=-1)
    vol *= 1 + 0.02 * rng.standard_normal(vol.shape)
    path = str(tmp_path / "pat068_vol.mat")
    matio.savemat(path, {"vol": vol, "b": bvals})
    common = ["--data", path, "--number_of_epochs", "5", "--hidden_dim", "128", "--num_layers", "2", "--mapping_size", "32", "--roi_start",
              "2", "--roi_end", "30", "--seed", "0", "--adc", "--tv_baseline", "--tv_lambda", "2e-3", "--tv_huber", "0.05", "--tv_iters",
              "80"]
    for model in ("siren", "wire"):
        out = str(tmp_path / model)
        res = dwi_script.main(common + ["--output_address", out, "--model", model])[0]
        adc = matio.loadmat(os.path.join(out, "pat068", "adc.mat"))
        assert set(adc) >= {"adc_sr", "adc_spline", "adc_hr", "adc_tv", "b"}
        assert adc["adc_tv"].shape == (28, 28, 2) and adc["adc_spline"].shape == (56, 56, 2)
        mean_img, _, _, _, scale = dwi_script.load_input_and_scale(path)
        hs = torch.from_numpy(np.ascontiguousarray(mean_img[2:30, 2:30], dtype=np.float32)).cuda().permute(2, 3, 0, 1).contiguous()
        tv = baselines.tv_superres(hs[:, :, ::2, ::2].contiguous(), (2, 2), "decimate", 2e-3, 0.05, 80)
        stack = (tv.permute(2, 3, 0, 1).contiguous() * torch.as_tensor(scale.astype(np.float32), device="cuda")).contiguous()
        want = metrics.calculate_ADC_device(bvals, stack).cpu().numpy()
        print(f"--model {model}: psnr_tv_db {res['psnr_tv_db']:.2f}, adc_tv median {np.nanmedian(adc['adc_tv']):.3e}")
        assert np.array_equal(adc["adc_tv"], want, equal_nan=True)
        assert res["psnr_tv_db"] == float(metrics.psnr(hs, tv, 1.0)) and os.path.exists(os.path.join(out, "pat068", "ssim_scores_tv.csv"))
