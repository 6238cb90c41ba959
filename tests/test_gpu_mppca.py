"""GPU: the MP-PCA kernel of csrc/mppca.hip against the float64 restatement of its definition (tests/mppca_common.py) on the five
cases of tests/test_mppca_cpu.py, bit for bit across launch shapes, runs and the fp32 / fp64 entries, and through the drivers.

The parity tolerance is measured, not chosen: the restatement is evaluated twice in float64, once with the measurement rows reversed,
and d_ref is the largest deviation between the two results (here 3e-14 .. 3e-13 for ``out`` on data of max|x| about 3, 5e-15 .. 1.4e-14
for ``sigma``).  The kernel must lie within 32 d_ref of the restatement: up to 30 accumulated Jacobi sweeps at rank 64 against LAPACK's
tridiagonal path.  ``rank`` is compared at every voxel whose decision margin (min over p >= 1 of |b - a| / lam_{r-1}) is at least 1e-10;
on these inputs the restatement excludes none (smallest margin 7e-9), and at most 0.2 % may be excluded.  Every test prints what it
measured before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

from tests import mppca_common as P
from tests.guard_common import Guarded
from mri_super_resolution_amd import _lib, denoise, matio, ops
from mri_super_resolution_amd.scripts import denoise as denoise_script
from mri_super_resolution_amd.scripts import superresDWI as dwi_script

pytestmark = pytest.mark.gpu

FACTOR = 32
MARGIN = 1e-10
EXCLUDED_SHARE = 0.002


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a, order="C")).to("cuda", dtype)


def _run(x, window, mask=None, estimator="exp2"):
    out, sigma, rank = ops.mppca_denoise(x, window, mask, estimator)
    torch.cuda.synchronize()
    return out, sigma, rank


def _same(a, b):
    return all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in zip(a, b))


def _parity(index, estimator):
    case = P.cases()[index]
    want_out, want_sigma, want_rank, margin = P.reference(index, P.ESTIMATORS[estimator])
    d_out, d_sigma = P.reference_spread(index, P.ESTIMATORS[estimator])
    out, sigma, rank = (t.cpu().numpy() for t in _run(_dev(case["noisy"]), case["window"], None, estimator))
    decided = margin >= MARGIN
    e_out, e_sigma = float(np.abs(out - want_out).max()), float(np.abs(sigma - want_sigma).max())
    print(f"{P.CASE_IDS[index]} {estimator}: max|out - restated| = {e_out:.3e} (d_ref {d_out:.3e}, bound {FACTOR * d_out:.3e}), max|sigma - restated| = "
          f"{e_sigma:.3e} (d_ref {d_sigma:.3e}, bound {FACTOR * d_sigma:.3e}); rank differs at {int((rank != want_rank)[decided].sum())} of "
          f"{int(decided.sum())} decided voxels, {int((~decided).sum())} excluded (smallest margin {margin.min():.2e}); unconverged "
          f"{int((rank == -2).sum())}; ranks {np.bincount(rank.reshape(-1).clip(min=0)).tolist()}")
    assert out.dtype == sigma.dtype == np.float64 and rank.dtype == np.int32
    assert (rank != -2).all()
    assert (~decided).mean() <= EXCLUDED_SHARE
    assert np.array_equal(rank[decided], want_rank[decided])
    assert e_out <= FACTOR * d_out and e_sigma <= FACTOR * d_sigma


@pytest.mark.parametrize("index", range(len(P.CASES)), ids=P.CASE_IDS)
def test_the_kernel_matches_the_restatement_and_every_voxel_converges(index):
    _parity(index, "exp2")


def test_the_exp1_estimator_matches_the_restatement():
    _parity(1, "exp1")


@pytest.mark.parametrize("index", range(len(P.CASES)), ids=P.CASE_IDS)
def test_the_bits_do_not_depend_on_the_launch_shape_or_the_run(index):
    case = P.cases()[index]
    x = _dev(case["noisy"])
    first = _run(x, case["window"])
    again = _run(x, case["window"])
    capped = {}
    for cap in (1, 3):
        assert _lib.lib().inr_debug_set(32, cap) == 0
        capped[cap] = _run(x, case["window"])
    assert _lib.lib().inr_debug_set(32, 0) == 0
    print(f"{P.CASE_IDS[index]}: second run equal {_same(first, again)}; grid capped at 1 workgroup equal {_same(first, capped[1])}, at 3 "
          f"{_same(first, capped[3])}")
    assert _same(first, again)
    assert _same(first, capped[1]) and _same(first, capped[3])


@pytest.mark.parametrize("index", (0, 3, 4), ids=[P.CASE_IDS[i] for i in (0, 3, 4)])
def test_fp32_is_the_fp64_result_of_the_upcast_input_rounded_once(index):
    case = P.cases()[index]
    x32 = _dev(case["noisy"], torch.float32)
    out, sigma, rank = _run(x32, case["window"])
    wout, wsigma, wrank = _run(x32.double(), case["window"])
    same = torch.equal(out, wout.float()) and torch.equal(sigma, wsigma.float()) and torch.equal(rank, wrank)
    print(f"{P.CASE_IDS[index]}: fp32 entry == fp64 entry on the up-cast input, rounded once: {same}")
    assert out.dtype == sigma.dtype == torch.float32 and rank.dtype == torch.int32 and wout.dtype == torch.float64
    assert same


def test_the_mask_passes_data_through_and_does_not_change_the_voxels_inside():
    case = P.cases()[1]
    x = _dev(case["noisy"])
    rng = np.random.default_rng(4)
    mask = _dev(rng.random(case["shape"]) > 0.4, torch.bool)
    assert 0 < int(mask.sum()) < mask.numel()
    full = _run(x, case["window"])
    out, sigma, rank = _run(x, case["window"], mask)
    as_bytes = _run(x, case["window"], mask.to(torch.uint8) * 7)         # any non-zero byte is inside
    inside = torch.equal(out[:, mask], full[0][:, mask]) and torch.equal(sigma[mask], full[1][mask]) and torch.equal(rank[mask], full[2][mask])
    outside = torch.equal(out[:, ~mask], x[:, ~mask]) and bool((sigma[~mask] == 0).all()) and bool((rank[~mask] == -1).all())
    print(f"{int(mask.sum())} of {mask.numel()} voxels inside: inside equal to the unmasked run {inside}; outside out == x, sigma == 0, "
          f"rank == -1 {outside}; a uint8 mask of 7s equal {_same((out, sigma, rank), as_bytes)}")
    assert inside and outside and _same((out, sigma, rank), as_bytes)


def test_all_three_outputs_are_written_inside_their_guards_and_null_outputs_leave_out_alone():
    lib = _lib.lib()
    for index in (1, 3, 4):                                                  # one case per rank class (16, 32, 64)
        case = P.cases()[index]
        M, (D, H, W), win = case["M"], case["shape"], case["window"]
        for dtype, entry in ((torch.float64, lib.inr_mppca_denoise), (torch.float32, lib.inr_mppca_denoise_f32)):
            x = _dev(case["noisy"], dtype)
            want = _run(x, win)
            out, sigma, rank = Guarded((M, D, H, W), dtype), Guarded((D, H, W), dtype), Guarded((D, H, W), torch.int32)
            rc = entry(out.ptr, sigma.ptr, rank.ptr, x.data_ptr(), None, M, D, H, W, *win, 2, None)
            assert rc == 0, lib.inr_last_error()
            ok = out.intact() and sigma.intact() and rank.intact()
            written = out.written() and sigma.written() and rank.written()
            alone = Guarded((M, D, H, W), dtype)
            assert entry(alone.ptr, None, None, x.data_ptr(), None, M, D, H, W, *win, 2, None) == 0
            print(f"{P.CASE_IDS[index]} {dtype}: guards intact {ok}, every element written {written}, equal to the wrapper "
                  f"{_same((out.view, sigma.view, rank.view), want)}; null sigma / rank: guards intact {alone.intact()}, out equal "
                  f"{torch.equal(alone.view, want[0])}")
            assert ok and written and _same((out.view, sigma.view, rank.view), want)
            assert alone.intact() and alone.written() and torch.equal(alone.view, want[0])


def test_a_volume_of_exactly_the_windows_size_shares_one_window():
    """One window per case is too small a sample to measure a d_ref on, so the bound is reasoned: an eigenvalue of G moves by at most about
    r eps ||G|| under the rounding of either eigensolver, ||G|| <= M N max|x|^2 = 30 x 27 x 11 here, so lam = s / q by 2e-12 and sigma =
    sqrt(mean lam) ~ 0.05 by 2e-11; the projector moves by that over the gap to the noise eigenvalues, of the same order.  1e-10 on
    both, nine orders below the noise."""
    rng = np.random.default_rng(3)
    for M, shape in ((8, (3, 3, 3)), (30, (3, 3, 3)), (16, (1, 5, 5))):
        _, noisy = P.phantom(M, shape, P.SIGMA, rng)
        out, sigma, rank = (t.cpu().numpy() for t in _run(_dev(noisy), shape))
        want_out, want_sigma, want_rank, margin = P.mppca(noisy, shape)
        e_out = float(np.abs(out - want_out).max())
        print(f"M = {M}, volume = window = {shape}: sigma values {np.unique(sigma).size}, rank values {np.unique(rank).size}, max|out - restated| = "
              f"{e_out:.2e}, smallest margin {margin.min():.1e}")
        assert np.unique(sigma).size == 1 and np.unique(rank).size == 1
        assert margin.min() < MARGIN or np.array_equal(rank, want_rank)
        assert e_out <= 1e-10 and np.abs(sigma - want_sigma).max() <= 1e-10


def test_exact_rank_two_data_comes_back_with_rank_at_most_two_and_zero_data_with_rank_zero():
    """Without noise G is numerically rank-deficient: its small eigenvalues are rounding noise, which differs between the two
    eigensolvers, and only the rule s_p <= q eps s_max decides.  The tolerance on ``out`` is that of test_mppca_cpu.py: 32 times the
    upper end of d_ref (4e-14 max|x|)."""
    clean, _ = P.phantom(16, (1, 24, 24), 0.0, None, n_components=2)
    out, sigma, rank = (t.cpu().numpy() for t in _run(_dev(clean), (1, 5, 5)))
    want = P.mppca(clean, (1, 5, 5))
    tol = 32 * 4e-14 * np.abs(clean).max()
    print(f"rank-2 data without noise: ranks {np.bincount(rank.reshape(-1).clip(min=0)).tolist()} (restated "
          f"{np.bincount(want[2].reshape(-1)).tolist()}), max|out - x| = {np.abs(out - clean).max():.2e} (bound {tol:.2e}), largest sigma {sigma.max():.1e}")
    assert rank.max() <= 2 and rank.min() >= 0 and np.array_equal(rank, want[2])
    assert np.abs(out - clean).max() <= tol and sigma.max() == 0.0
    zero = _run(torch.zeros((4, 1, 3, 3), device="cuda", dtype=torch.float64), (1, 3, 3))
    assert bool((zero[2] == 0).all()) and bool((zero[1] == 0).all()) and bool((zero[0] == 0).all())


def test_the_python_layer_keeps_layouts_types_and_the_single_slice():
    case = P.cases()[0]
    noisy = case["noisy"]
    out, info = denoise.mppca(noisy, case["window"], return_info=True)
    want = _run(_dev(noisy), case["window"])
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and np.array_equal(out, want[0].cpu().numpy())
    assert np.array_equal(info["sigma"], want[1].cpu().numpy()) and np.array_equal(info["rank"], want[2].cpu().numpy())
    # [M, H, W] is one slice; the window may name its two in-plane sides
    one, one_info = denoise.mppca(noisy[:, 0], (5, 5), return_info=True)
    assert one.shape == noisy[:, 0].shape and np.array_equal(one, out[:, 0]) and one_info["sigma"].shape == (24, 24)
    # the drivers' layout [X, Y, Z, M]
    last = denoise.mppca(np.ascontiguousarray(np.moveaxis(noisy, 0, -1)), case["window"], measurement_axis=-1)
    assert last.shape == (1, 24, 24, 16) and np.array_equal(np.moveaxis(last, -1, 0), out)
    # device tensors come back as given
    t32 = _dev(noisy, torch.float32)
    got = denoise.mppca(t32, case["window"])
    assert got.dtype == torch.float32 and got.is_cuda and torch.equal(got, _run(t32, case["window"])[0])
    empty = ops.mppca_denoise(torch.empty((16, 0, 24, 24), device="cuda", dtype=torch.float64), (1, 5, 5))
    assert empty[0].shape == (16, 0, 24, 24) and empty[1].shape == (0, 24, 24)
    with pytest.raises(ValueError, match="contiguous"):
        ops.mppca_denoise(_dev(noisy)[:, :, ::2], (1, 5, 5))
    with pytest.raises(TypeError, match="float32 or torch.float64"):
        ops.mppca_denoise(_dev(noisy).half(), (1, 5, 5))


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------
def _master(path):
    """A synthetic master.mat: a 4 x 4 [b][TE] cell of 12 x 12 x 3 volumes, K = 2 acquisitions for b > 0, Gaussian noise of sigma 2."""
    rng = np.random.default_rng(5)
    X = Y = 12
    Z, K = 3, 2
    gx, gy, gz = np.meshgrid(np.linspace(0, 1, X), np.linspace(0, 1, Y), np.linspace(0, 1, Z), indexing="ij")
    tissue = (100 * (1.2 + np.sin(3 * gx) * np.cos(2 * gy)), 60 * (0.5 + gx * gy + 0.3 * gz))
    cell, clean = np.empty((4, 4), dtype=object), np.empty((4, 4), dtype=object)
    for b in range(4):
        for te in range(4):
            sig = tissue[0] * np.exp(-0.4 * b - 0.1 * te) + tissue[1] * np.exp(-1.5 * b - 0.4 * te)
            clean[b, te] = sig if b == 0 else np.repeat(sig[..., None], K, axis=-1)
            cell[b, te] = clean[b, te] + 2.0 * rng.standard_normal(clean[b, te].shape)
    matio.savemat(path, {"hybrid_raw": cell, "b": np.array([0.0, 150.0, 1000.0, 1500.0]), "TE": np.array([0.0, 13.0, 93.0, 143.0])})
    return cell, clean


def test_the_denoise_script_writes_the_clean_cell_the_driver_reads(tmp_path):
    src, dst = str(tmp_path / "pat011_master.mat"), str(tmp_path / "pat011_clean.mat")
    cell, clean = _master(src)
    summary = denoise_script.main(["--data", src, "--out", dst, "--window", "5", "5", "3"])
    saved = matio.loadmat(dst)
    stack = denoise.stack_hybrid(cell)
    want, info = denoise.mppca(stack, (5, 5, 3), return_info=True)
    got = denoise.stack_hybrid(saved["hybrid_raw_clean"])
    truth = denoise.stack_hybrid(clean)
    ratio = P.rmse(got, truth) / P.rmse(stack, truth)
    print(f"scripts/denoise.py: M = {summary['measurements']}, sigma median {summary['sigma_median']:.3f} (noise 2.0), RMSE out / in = {ratio:.3f}, "
          f"ranks {summary['rank_histogram']}, unconverged {summary['unconverged']}")
    assert summary["measurements"] == stack.shape[0] == 28 and summary["unconverged"] == 0
    assert saved["hybrid_raw_clean"].shape == (4, 4) and saved["hybrid_raw_clean"][0, 0].shape == (12, 12, 3)
    assert saved["hybrid_raw_clean"][2, 1].shape == (12, 12, 3, 2)
    assert np.array_equal(got, want) and np.array_equal(saved["sigma"], info["sigma"]) and np.array_equal(saved["rank"], info["rank"])
    assert ratio < 1.0 and 0.8 * 2.0 <= summary["sigma_median"] <= 1.1 * 2.0
    # the file's other variables are kept as they were
    for key in ("b", "TE"):
        assert np.array_equal(saved[key], matio.loadmat(src)[key])
    assert denoise.stack_hybrid(saved["hybrid_raw"]).tobytes() == stack.tobytes()
    # the driver's loader accepts the clean cell like the raw one
    mean_img, acq, bvals, maxes, scale = dwi_script.load_input_and_scale(dst, "hybrid_raw_clean")
    raw_mean = dwi_script.load_input_and_scale(src)[0]
    assert mean_img.shape == raw_mean.shape == (12, 12, 3, 4) and acq.shape[:4] == (12, 12, 3, 4) and maxes.shape == (4, 4)
    assert np.isfinite(mean_img).all() and not np.array_equal(mean_img, raw_mean) and list(bvals) == [0.0, 150.0, 1000.0, 1500.0]
    # ... and the loader's own flag makes the same stack before it normalises
    flag = {"window": (5, 5, 3)}
    flagged = dwi_script.load_input_and_scale(src, None, None, flag)[0]
    assert np.array_equal(flagged, mean_img) and flag["sigma_median"] == summary["sigma_median"]


TIMINGS = ("t_fit_s", "t_recon_s", "train_voxels_per_s")
DENOISE_KEYS = {"denoise", "denoise_window", "denoise_sigma_median"}


def test_superresDWI_without_the_flag_is_what_it_was_and_with_it_records_sigma(tmp_path):
    rng = np.random.default_rng(3)
    gx, gy, gz = np.meshgrid(np.linspace(0, 1, 32), np.linspace(0, 1, 32), np.linspace(0, 1, 2), indexing="ij")
    vol = np.stack([500 * (1.2 + np.sin(3 * gx + gz) * np.cos(2 * gy)) * np.exp(-0.7 * b) for b in range(4)], axis=-1)
    vol = vol + 10.0 * rng.standard_normal(vol.shape)
    path = str(tmp_path / "pat068_vol.mat")
    matio.savemat(path, {"vol": vol, "b": np.array([0.0, 150.0, 1000.0, 1500.0])})
    common = ["--data", path, "--number_of_epochs", "5", "--hidden_dim", "128", "--num_layers", "2", "--mapping_size", "32", "--roi_start", "2",
              "--roi_end", "30", "--seed", "0"]
    runs = {}
    for name, extra in (("plain", []), ("none", ["--denoise", "none"]), ("mppca", ["--denoise", "mppca", "--denoise_window", "3", "3", "1"])):
        out = str(tmp_path / name)
        dwi_script.main(common + extra + ["--output_address", out])
        d = os.path.join(out, "pat068")
        runs[name] = (json.load(open(os.path.join(d, "metrics.json"))), open(os.path.join(d, "recon.npy"), "rb").read(), sorted(os.listdir(d)))
    strip = lambda m: {k: v for k, v in m.items() if k not in TIMINGS}
    plain, none, flagged = runs["plain"], runs["none"], runs["mppca"]
    print(f"--denoise mppca: sigma median {flagged[0]['denoise_sigma_median']:.3f} (noise 10.0), keys added {sorted(set(flagged[0]) - set(plain[0]))}")
    assert strip(plain[0]) == strip(none[0]) and list(plain[0]) == list(none[0]) and plain[1] == none[1] and plain[2] == none[2]
    assert not DENOISE_KEYS & set(plain[0])
    assert set(flagged[0]) - set(plain[0]) == DENOISE_KEYS and flagged[2] == plain[2] and flagged[1] != plain[1]
    assert flagged[0]["denoise"] == "mppca" and flagged[0]["denoise_window"] == [3, 3, 1]
    want = denoise.mppca(vol, (3, 3, 1), return_info=True, measurement_axis=-1)[1]["sigma"]
    assert flagged[0]["denoise_sigma_median"] == float(np.median(want)) and 5.0 < flagged[0]["denoise_sigma_median"] < 12.0
    with pytest.raises(ValueError, match="third window side \\(5\\) is larger than its axis \\(2\\)"):
        dwi_script.main(common + ["--denoise", "mppca", "--output_address", str(tmp_path / "refused")])
