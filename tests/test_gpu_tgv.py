"""GPU: the second-order TGV solver of csrc/tgv.hip against its float64 restatement (tests/tgv_common.py), bit for bit where the
contract gives an exact answer, across a batch, against properties that do not depend on the restatement (the TGV energy is at most
the TV energy; the gain over TV on the phantom), and through ``superresDWI --tv_tgv`` and ``scripts/second_order``.

Bounds are those of tests/test_gpu_tvsr.py, by the same derivation: the iteration is non-expansive, about 25 roundings of 1.1e-16 per
pixel and iteration (10 there) give 3e-12 after 1,000 iterations on data in [0, 1], and 1e-10 absolute on the image and on the field v
leaves more than an order of margin.  ``change`` is the difference of two images within the bound: 2e-10.  ``energy`` is a sum of at
most 2 H W + h w non-negative terms of a few roundings each: 1e-12 relative against the restated objective at the returned (x, v).
Every test prints what it measured before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

from tests import tgv_common as G
from tests import tvsr_common as T
from mri_super_resolution_amd import baselines, drivers, matio, metrics, ops, reports
from mri_super_resolution_amd.scripts import second_order as so_script
from mri_super_resolution_amd.scripts import superresDWI as dwi_script

pytestmark = pytest.mark.gpu

SOLVER_BOUND = 1e-10
ENERGY_BOUND = 1e-12


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _compare(name, y, f, kernel, lam, ratio, alpha, n_iter, w=None, x0=None):
    got, info = baselines.tgv_superres(y, f, kernel, lam, ratio, alpha, n_iter, weight=w, x0=x0, return_info=True)
    want, want_v, _, change = G.solve(y, f, kernel, lam, ratio, alpha, n_iter, w=w, x0=x0, return_info=True)
    v = info["v"]
    at_result = G.energy(got, v[..., 0, :, :], v[..., 1, :, :], np.where(w == 0, 0.0, y) if w is not None else y, T.block_kernel(kernel, f),
                         lam, ratio, alpha, w)
    err, v_err = float(np.abs(got - want).max()), float(np.abs(v - want_v).max())
    e_rel = float(np.abs(info["energy"] - at_result).max() / np.abs(at_result).max()) if np.abs(at_result).max() > 0 else \
        float(np.abs(info["energy"]).max())
    c_err = float(np.abs(info["change"] - change).max())
    print(f"{name}, ratio {ratio}, alpha {alpha}, {n_iter} iterations: max|x - restated| = {err:.3e}, max|v - restated| = {v_err:.3e} (bound "
          f"{SOLVER_BOUND:.0e}), energy against the restated objective at the returned (x, v) {e_rel:.2e} (bound {ENERGY_BOUND:.0e}), "
          f"|change - restated| {c_err:.2e} (change {float(change.max()):.2e}), max|v| {float(np.abs(v).max()):.2e}")
    assert got.dtype == np.float64 and got.shape == want.shape and v.shape == want_v.shape
    assert err <= SOLVER_BOUND and v_err <= SOLVER_BOUND
    assert c_err <= 2 * SOLVER_BOUND            # the difference of two images that are each within the bound
    assert e_rel <= ENERGY_BOUND
    return got, info


# ---- against the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", (0.5, 2.0))
@pytest.mark.parametrize("alpha", (0.0, G.CASE_ALPHA), ids=("tv", "huber"))
@pytest.mark.parametrize("n_iter", (1, 2, 300))
def test_solver_matches_the_restatement_on_the_weighted_case(n_iter, alpha, ratio):
    _, y = G.case_data()
    assert (G.CASE_W == 0).sum() == 1
    _compare("6x10 (3, 2) mean, weighted", y, G.CASE_FACTORS, "mean", G.CASE_LAM, ratio, alpha, n_iter, w=G.CASE_W)


@pytest.mark.parametrize("H,W,f", ((7, 1024, (7, 1)), (1024, 3, (1, 3))), ids=("7x1024by7x1", "1024x3by1x3"))
def test_solver_matches_the_restatement_on_ragged_strides_and_a_one_block_axis(H, W, f):
    """H W and h w are no multiples of the 1,024 threads, and one axis is a single block or a single pixel per block."""
    rng = np.random.default_rng(H)
    hr = rng.random((2, H, W))
    k = rng.random(f) + 0.1
    for name, kernel in (("mean", "mean"), ("random", k / k.sum())):
        y = T.apply_A(hr, T.block_kernel(kernel, f))
        w = rng.random(y.shape) * (rng.random(y.shape) > 0.1)
        assert (w == 0).any()
        _compare(f"2 x {H}x{W} {f} {name}", y, f, kernel, 0.02, 2.0, 0.05, 40, w=w, x0=rng.random(hr.shape))
    _compare(f"2 x {H}x{W} {f} decimate, plain", T.apply_A(hr, T.block_kernel("decimate", f)), f, "decimate", 0.02, 0.5, 0.0, 40)


@pytest.mark.parametrize("h,w,f", ((1, 1, (1, 1)), (1, 20, (1, 2)), (20, 1, (2, 1))), ids=("1x1", "1x40by1x2", "40x1by2x1"))
def test_solver_matches_the_restatement_where_every_difference_is_a_boundary_case(h, w, f):
    rng = np.random.default_rng(40 + h)
    y = rng.random((3, h, w))
    for alpha in (0.0, 0.03):
        _compare(f"{h * f[0]}x{w * f[1]} by {f}", y, f, "mean", 0.05, 2.0, alpha, 1000, x0=rng.random((3, h * f[0], w * f[1])))


# ---- fp32 ---------------------------------------------------------------------------------------------------------------------------------
def test_fp32_is_the_fp64_result_rounded_once_and_types_come_back_as_given():
    rng = np.random.default_rng(9)
    hr, y = G.case_data()
    y32, w32, x32 = _dev(y, torch.float32), _dev(G.CASE_W, torch.float32), _dev(rng.random(hr.shape), torch.float32)
    for alpha in (0.0, G.CASE_ALPHA):
        args = (G.CASE_FACTORS, "mean", G.CASE_LAM, 2.0, alpha, 100)
        got, info = baselines.tgv_superres(y32, *args, weight=w32, x0=x32, return_info=True)
        want, winfo = baselines.tgv_superres(y32.double(), *args, weight=w32.double(), x0=x32.double(), return_info=True)
        same = (torch.equal(got, want.float()), torch.equal(info["v"], winfo["v"].float()))
        print(f"alpha {alpha}: fp32 out, v == fp64 out, v rounded once: {same}; max|fp32 - fp64| = "
              f"{float((got.double() - want).abs().max()):.2e}, max|v| {float(winfo['v'].abs().max()):.2e}")
        assert got.dtype == info["v"].dtype == torch.float32 and want.dtype == winfo["v"].dtype == torch.float64
        assert got.is_cuda and info["energy"].dtype == torch.float64 and float(winfo["v"].abs().max()) > 0
        assert all(same)
        assert torch.equal(info["energy"], winfo["energy"]) and torch.equal(info["change"], winfo["change"])
    # leading axes are a batch and keep their shape
    stack = _dev(rng.random((2, 3, 4, 6)), torch.float32)
    out, info = baselines.tgv_superres(stack, (2, 1), n_iter=5, return_info=True)
    assert out.shape == (2, 3, 8, 6) and info["v"].shape == (2, 3, 2, 8, 6) and info["energy"].shape == info["change"].shape == (2, 3)
    assert isinstance(baselines.tgv_superres(rng.random((3, 4, 6)), (2, 2), n_iter=3), np.ndarray)


# ---- exact properties -------------------------------------------------------------------------------------------------------------------
def test_exact_properties_on_the_device():
    rng = np.random.default_rng(5)
    hr, y = G.case_data()
    w, f = G.CASE_W, G.CASE_FACTORS
    # a constant image is returned exactly, with v = 0 (the 2 x 2 mean of equal values is exact: its weights are a power of two)
    x, info = baselines.tgv_superres(np.full((1, 5, 7), 0.7), (2, 2), "mean", 0.01, 2.0, 0.0, 50, return_info=True)
    print(f"constant 0.7: max|x - 0.7| = {float(np.abs(x - 0.7).max())}, max|v| = {float(np.abs(info['v']).max())}, energy "
          f"{float(info['energy'][0])}, change {float(info['change'][0])}")
    assert np.array_equal(x, np.full((1, 10, 14), 0.7)) and not info["v"].any() and float(info["change"][0]) == 0.0
    # lambda = 0 with the mean kernel at factor 2: the replication start satisfies the data and stays, exactly
    y2 = rng.random((2, 5, 6))
    for n_iter in (1, 50):
        x, info = baselines.tgv_superres(y2, (2, 2), "mean", 0.0, 2.0, 0.0, n_iter, return_info=True)
        print(f"lambda = 0, {n_iter} iterations: x == replication {np.array_equal(x, T.replicate(y2, (2, 2)))}, v == 0 {not info['v'].any()}, "
              f"energy {float(info['energy'].max()):.2e}, change {float(info['change'].max()):.2e}")
        assert np.array_equal(x, T.replicate(y2, (2, 2))) and not info["v"].any()
    # n_iter = 0 returns x0 (the given one, or the block replication), v = 0 and change = 0
    x0 = rng.random(hr.shape)
    x, info = baselines.tgv_superres(y, f, "mean", 0.05, 2.0, 0.02, 0, x0=x0, return_info=True)
    assert np.array_equal(x, x0) and float(info["change"][0]) == 0.0 and not info["v"].any()
    assert np.array_equal(baselines.tgv_superres(y, f, "mean", 0.05, 2.0, 0.02, 0), T.replicate(y, f))
    # a missing datum (w = 0) is never read: whatever y holds there -- 1e3 or NaN --, the same bits come out
    start = T.replicate(y, f)
    a, ia = baselines.tgv_superres(y, f, "mean", G.CASE_LAM, 2.0, G.CASE_ALPHA, 30, weight=w, x0=start, return_info=True)
    for value in (1e3, float("nan")):
        other = y.copy()
        other[w == 0] = value
        b, ib = baselines.tgv_superres(other, f, "mean", G.CASE_LAM, 2.0, G.CASE_ALPHA, 30, weight=w, x0=start, return_info=True)
        same = all(np.array_equal(ia[key], ib[key]) for key in ("energy", "change", "v")) and np.array_equal(a, b)
        print(f"the w = 0 datum holds {value}: same bits {same}")
        assert (w == 0).sum() == 1 and np.isfinite(b).all() and same
    # v_out = null leaves the image bits unchanged
    without = baselines.tgv_superres(y, f, "mean", G.CASE_LAM, 2.0, G.CASE_ALPHA, 30, weight=w, x0=start)
    yd = _dev(y)
    o1, v1, e1, c1 = ops.tgv_solve(yd, f, T.block_kernel("mean", f).tolist(), G.CASE_LAM, 2.0, G.CASE_ALPHA, 30, want_v=False)
    o2, v2, e2, c2 = ops.tgv_solve(yd, f, T.block_kernel("mean", f).tolist(), G.CASE_LAM, 2.0, G.CASE_ALPHA, 30)
    print(f"v_out = null: image bits unchanged {np.array_equal(without, a)}, {torch.equal(o1, o2)}")
    assert np.array_equal(without, a)
    assert v1 is None and v2.shape == (1, 2, 6, 10) and torch.equal(o1, o2) and torch.equal(e1, e2) and torch.equal(c1, c2)


def test_ops_wrapper_checks_before_it_launches():
    y = torch.rand(2, 3, 5, device="cuda", dtype=torch.float64)
    k = [[0.25, 0.25], [0.25, 0.25]]
    out, v, energy, change = ops.tgv_solve(y, (2, 2), k, 0.01, 2.0, 0.0, 3)
    assert out.shape == (2, 6, 10) and v.shape == (2, 2, 6, 10) and energy.shape == change.shape == (2,)
    with pytest.raises(ValueError, match="contiguous"):
        ops.tgv_solve(y[:, :, ::2], (2, 2), k, 0.01, 2.0, 0.0, 3)
    with pytest.raises(TypeError, match="float32 or torch.float64"):
        ops.tgv_solve(y.half(), (2, 2), k, 0.01, 2.0, 0.0, 3)
    with pytest.raises(ValueError, match="weight has shape"):
        ops.tgv_solve(y, (2, 2), k, 0.01, 2.0, 0.0, 3, weight=y[:1].contiguous())
    with pytest.raises(ValueError, match="x0 has shape"):
        ops.tgv_solve(y, (2, 2), k, 0.01, 2.0, 0.0, 3, x0=y)
    with pytest.raises(ValueError, match="sum to 1"):
        ops.tgv_solve(y, (2, 2), [[1.0, 1.0], [1.0, 1.0]], 0.01, 2.0, 0.0, 3)
    with pytest.raises(ValueError, match="ratio must be finite and > 0"):
        ops.tgv_solve(y, (2, 2), k, 0.01, 0.0, 0.0, 3)
    with pytest.raises(ValueError, match="workspace must be a device float64 tensor of at least 1320"):
        ops.tgv_solve(y, (2, 2), k, 0.01, 2.0, 0.0, 3, workspace=torch.empty(1319, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="n_iter must be an integer >= 0"):
        ops.tgv_solve(y, (2, 2), k, 0.01, 2.0, 0.0, -1)
    ws = torch.empty(1320, device="cuda", dtype=torch.float64)
    again = ops.tgv_solve(y, (2, 2), k, 0.01, 2.0, 0.0, 3, workspace=ws)
    assert torch.equal(again[0], out) and torch.equal(again[1], v)


# ---- a batch ------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_beyond_the_cu_count_equals_its_solitary_solves_bit_for_bit():
    """300 different images of 12 x 12: more workgroups than the 256 CUs, so some are queued behind others, and the reduction
    scratch is reused between images."""
    rng = np.random.default_rng(11)
    n, f = 300, (2, 3)
    y = _dev(rng.random((n, 6, 4)))
    w = _dev(rng.random((n, 6, 4)) * (rng.random((n, 6, 4)) > 0.1))
    args = (f, "mean", 0.02, 2.0, 0.05, 25)
    keys = ("energy", "change", "v")
    out, info = baselines.tgv_superres(y, *args, weight=w, return_info=True)
    torch.cuda.synchronize()
    differ = 0
    for i in range(n):
        one, one_info = baselines.tgv_superres(y[i:i + 1], *args, weight=w[i:i + 1], return_info=True)
        differ += int(not (torch.equal(one[0], out[i]) and all(torch.equal(one_info[key][0], info[key][i]) for key in keys)))
    again, again_info = baselines.tgv_superres(y, *args, weight=w, return_info=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side, side_info = baselines.tgv_superres(y, *args, weight=w, return_info=True)
    side.synchronize()
    perm = torch.from_numpy(rng.permutation(n)).cuda()
    moved, moved_info = baselines.tgv_superres(y[perm].contiguous(), *args, weight=w[perm].contiguous(), return_info=True)
    distinct = len({out[i].cpu().numpy().tobytes() for i in range(n)})
    print(f"{n} images of 12x12: {differ} differ from their solitary solve; second run equal {torch.equal(again, out)}; side stream equal "
          f"{torch.equal(on_side, out)}; permuted batch equal {torch.equal(moved, out[perm])}; {distinct} distinct results")
    assert out.shape == (n, 12, 12) and distinct == n
    assert differ == 0
    assert torch.equal(again, out) and all(torch.equal(again_info[key], info[key]) for key in keys)
    assert torch.equal(on_side, out) and all(torch.equal(side_info[key], info[key]) for key in keys)
    assert torch.equal(moved, out[perm]) and all(torch.equal(moved_info[key], info[key][perm]) for key in keys)


# ---- independent of the restatement's iteration ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", (0.0, 0.02), ids=("tv", "huber"))
@pytest.mark.parametrize("ratio", (2.0, 0.5))
def test_tgv_energy_is_at_most_the_tv_energy_on_the_device(ratio, alpha):
    """(x_TV, 0) is feasible for the TGV problem, so its minimum is at most the TV minimum: no slack term."""
    y = T.apply_A(np.random.default_rng(12).random((1, 12, 20)), T.block_kernel("mean", (2, 2)))
    k = T.block_kernel("mean", (2, 2))
    x, info = baselines.tgv_superres(y, (2, 2), "mean", 0.05, ratio, alpha, 1000, return_info=True)
    x_tv, tv_info = baselines.tv_superres(y, (2, 2), "mean", 0.05, alpha, 4000, return_info=True)
    zero = np.zeros_like(x_tv)
    e_tv = float(G.energy(x_tv, zero, zero, y, k, 0.05, ratio, alpha)[0])
    e = float(info["energy"][0])
    print(f"ratio {ratio}, alpha {alpha}: TGV energy after 1,000 iterations {e:.10f}, E(x_TV, 0) after 4,000 {e_tv:.10f} (the TV solver's own "
          f"{float(tv_info['energy'][0]):.10f}), TGV / TV = {e / e_tv:.5f}")
    assert e_tv == pytest.approx(float(tv_info["energy"][0]), rel=1e-12)
    assert e <= e_tv


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_the_gain_over_first_order_on_the_phantom_on_the_device(seed):
    hr, lr = G.phantom_data(seed)
    x = baselines.tgv_superres(lr, (2, 2), "mean", 0.01, 4.0, 0.0, 300)
    tv = {(lam, a): G.rmse(baselines.tv_superres(lr, (2, 2), "mean", lam, a, 300), hr)
          for lam, a in ((0.005, 0.0), (0.0075, 0.0), (0.01, 0.0), (0.01, 0.03))}
    best, r = min(tv.values()), G.rmse(x, hr)
    print(f"phantom, seed {seed}: TGV (0.01, ratio 4) RMSE {r:.5f}; TV {', '.join(f'{k}: {v:.5f}' for k, v in tv.items())}; ratio to the best "
          f"{r / best:.3f} (bound 0.9); flat-area index: HR {G.flat_share(hr):.3f}, TGV {G.flat_share(x):.3f}")
    assert r <= 0.9 * best


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------
TIMINGS = ("t_fit_s", "t_recon_s", "train_voxels_per_s")        # wall-clock: the only values two runs of one command do not share
TGV_KEYS = {"psnr_tv_tgv_db", "ssim_tv_tgv_mean", "tv_tgv_consistency_psnr_db"}


def _four_b_volume(path):
    """The synthetic four-b volume of test_gpu_tvsr.py's --adc test."""
    rng = np.random.default_rng(3)
    bvals = np.array([0.0, 150.0, 1000.0, 1500.0])
    gx, gy, gz = np.meshgrid(np.linspace(0, 1, 32), np.linspace(0, 1, 32), np.linspace(0, 1, 2), indexing="ij")
    vol = np.stack([500 * (1.2 + np.sin(3 * gx + gz) * np.cos(2 * gy)) * np.exp(-0.7 * b) for b in range(4)], axis=-1)
    vol *= 1 + 0.02 * rng.standard_normal(vol.shape)
    matio.savemat(path, {"vol": vol, "b": bvals})
    return bvals


def test_superresDWI_tv_tgv(tmp_path):
    path = str(tmp_path / "pat068_vol.mat")
    bvals = _four_b_volume(path)
    common = ["--data", path, "--number_of_epochs", "5", "--hidden_dim", "128", "--num_layers", "2", "--mapping_size", "32", "--roi_start",
              "2", "--roi_end", "30", "--seed", "0", "--adc", "--tv_baseline", "--tv_lambda", "2e-3", "--tv_huber", "0.05", "--tv_iters", "80"]
    flags = ["--tv_tgv", "--tv_tgv_lambda", "0.004", "--tv_tgv_ratio", "1.5"]
    out_plain, out = str(tmp_path / "plain"), str(tmp_path / "tgv")
    res_plain = dwi_script.main(common + ["--output_address", out_plain])[0]
    res = dwi_script.main(common + flags + ["--output_address", out])[0]
    d_plain, d = os.path.join(out_plain, "pat068"), os.path.join(out, "pat068")
    # a direct call on the LR stack the driver forms
    mean_img, _, _, _, scale = dwi_script.load_input_and_scale(path)
    hs = torch.from_numpy(np.ascontiguousarray(mean_img[2:30, 2:30], dtype=np.float32)).cuda().permute(2, 3, 0, 1).contiguous()
    ls = hs[:, :, ::2, ::2].contiguous()
    tgv = baselines.tgv_superres(ls, (2, 2), "decimate", 0.004, 1.5, 0.05, 80)
    stack = (tgv.permute(2, 3, 0, 1).contiguous() * torch.as_tensor(scale.astype(np.float32), device="cuda")).contiguous()
    want_adc = metrics.calculate_ADC_device(bvals, stack).cpu().numpy()
    adc = matio.loadmat(os.path.join(d, "adc.mat"))
    m = json.load(open(os.path.join(d, "metrics.json")))
    rows = reports.read_csv(os.path.join(d, "ssim_scores.csv"))
    grows = reports.read_csv(os.path.join(d, "ssim_scores_tv_tgv.csv"))
    floor = lambda t: t.clamp_min(1e-30)
    want_ssim = metrics.ssim_reference_protocol(floor(hs), floor(tgv)).cpu().numpy().reshape(-1)
    col = np.array([float(r["SSIM-tv-tgv"]) for r in grows])
    want_psnr = float(metrics.psnr(hs, tgv, 1.0))
    print(f"--tv_tgv: psnr_tv_tgv_db {m['psnr_tv_tgv_db']:.3f} (direct {want_psnr:.3f}), psnr_tv_db {m['psnr_tv_db']:.3f}, "
          f"ssim_tv_tgv_mean {m['ssim_tv_tgv_mean']:.4f}, tv_tgv_consistency_psnr_db {m['tv_tgv_consistency_psnr_db']:.2f}, "
          f"adc_tv_tgv median {np.nanmedian(adc['adc_tv_tgv']):.3e}")
    assert tgv.dtype == torch.float32 and tgv.shape == hs.shape
    assert open(os.path.join(d, "ssim_scores_tv_tgv.csv")).readline() == reports.SSIM_TV_TGV_HEADER
    assert len(grows) == len(rows) == 8 and set(grows[0]) == {"Pt_id", "b-value", "slice", "SSIM-tv-tgv", "SSIM-SR"}
    for key in ("Pt_id", "b-value", "slice", "SSIM-SR"):
        assert [r[key] for r in grows] == [r[key] for r in rows], key
    assert np.array_equal(col, want_ssim) and m["ssim_tv_tgv_mean"] == pytest.approx(col.mean())
    assert m["psnr_tv_tgv_db"] == want_psnr == res["psnr_tv_tgv_db"]
    assert m["tv_tgv_consistency_psnr_db"] == float(metrics.psnr(ls, baselines.block_apply(tgv, (2, 2), "decimate"), 1.0))
    assert adc["adc_tv_tgv"].shape == (28, 28, 2) and np.array_equal(adc["adc_tv_tgv"], want_adc, equal_nan=True)
    # without --tv_tgv: every file and key is what it was, byte for byte, apart from the wall-clock values
    plain = json.load(open(os.path.join(d_plain, "metrics.json")))
    assert set(m) - set(plain) == TGV_KEYS and not [k for k in list(plain) + list(res_plain) if "tgv" in k]
    strip = lambda s: json.dumps({k: v for k, v in s.items() if k not in TIMINGS and k not in TGV_KEYS}, indent=1).encode()
    assert strip(plain) == strip(m)
    assert list(plain) == [k for k in m if k not in TGV_KEYS]
    assert sorted(os.listdir(d)) == sorted(os.listdir(d_plain) + ["ssim_scores_tv_tgv.csv"])
    for name in ("recon.npy", "ssim_scores.csv", "ssim_scores_tv.csv"):
        assert open(os.path.join(d_plain, name), "rb").read() == open(os.path.join(d, name), "rb").read(), name
    adc_plain = matio.loadmat(os.path.join(d_plain, "adc.mat"))
    assert set(adc) - set(adc_plain) == {"adc_tv_tgv"}
    for key in adc_plain:
        if not key.startswith("__"):
            assert np.array_equal(adc_plain[key], adc[key], equal_nan=True), key


def test_second_order_on_the_phantom(tmp_path):
    out = str(tmp_path / "so")
    res = so_script.main(["--phantom", "--output_address", out, "--tv_lambda", "0.0075", "--tgv_lambda", "0.01", "--tgv_ratio", "4", "--iters",
                          "300"])[0]
    d = os.path.join(out, "patphantom")
    assert sorted(os.listdir(d)) == ["metrics.json", "second_order.csv", "second_order.mat"]
    m = json.load(open(os.path.join(d, "metrics.json")))
    rows = reports.read_csv(os.path.join(d, "second_order.csv"))
    # direct calls on the data the driver forms: the phantom of the tests, seed 0
    hr, lr = G.phantom_data(0)
    assert np.array_equal(drivers.second_order_phantom(), hr)
    y = baselines.block_apply(_dev(hr[None]), (2, 2), "mean") + _dev(0.02 * np.random.default_rng(0).standard_normal((1, 24, 24)))
    assert float((y[0].cpu() - torch.from_numpy(lr)).abs().max()) <= 1e-15
    tv = baselines.tv_superres(y, (2, 2), "mean", 0.0075, baselines.TV_DEFAULT_HUBER, 300)
    tgv, info = baselines.tgv_superres(y, (2, 2), "mean", 0.01, 4.0, baselines.TGV_DEFAULT_HUBER, 300, return_info=True)
    f32 = lambda t: t.float().contiguous()
    for name, image in (("tv", tv), ("tgv", tgv)):
        want_ssim = metrics.ssim(f32(_dev(hr[None])), f32(image), 1.0).cpu().numpy().reshape(-1)
        want_psnr = metrics.psnr(f32(_dev(hr[None])), f32(image), 1.0, per_image=True).cpu().numpy().reshape(-1)
        assert np.array_equal(np.array([float(r[f"SSIM-{name}"]) for r in rows]), want_ssim), name
        assert np.array_equal(np.array([float(r[f"PSNR-{name}"]) for r in rows]), want_psnr), name
        assert float(rows[0][f"FLAT-{name}"]) == G.flat_share(image[0].cpu().numpy()) == m[f"flat_{name}_mean"], name
    print("second_order --phantom (300 iterations): " + ", ".join(
        f"{name}: PSNR {m[f'psnr_{name}_db']:.2f} dB, SSIM {m[f'ssim_{name}_mean']:.4f}, flat-area index {m[f'flat_{name}_mean']:.3f}"
        for name in drivers.SECOND_ORDER_METHODS) + f"; HR flat-area index {m['flat_hr_mean']:.3f}")
    assert len(rows) == 1 and rows[0]["slice"] == "0" and rows[0]["Pt_id"] == "phantom"
    assert m["methods"] == list(drivers.SECOND_ORDER_METHODS) == res["methods"]
    assert m["flat_hr_mean"] == G.flat_share(hr) == float(rows[0]["FLAT-hr"])
    mat = matio.loadmat(os.path.join(d, "second_order.mat"))
    assert mat["tgv"].shape == mat["hr"].shape == (48, 48, 1) and mat["lr"].shape == (24, 24, 1) and mat["v"].shape == (48, 48, 1, 2)
    assert np.array_equal(mat["tgv"], tgv.cpu().numpy().transpose(1, 2, 0))
    assert np.array_equal(mat["v"], info["v"].cpu().numpy().transpose(2, 3, 0, 1))
    # the gain of the issue's table, through the driver
    assert m["psnr_tgv_db"] > m["psnr_tv_db"] + 1.0 and m["psnr_tv_db"] > m["psnr_replicate_db"]
