"""GPU: the TV / Huber solver under dense separable operators (csrc/tvop.hip) against the float64 restatement of
tests/tvop_common.py, against an independent minimum, against the block solver, and against itself (equal bits).  A shape is written
(H, W) -> (h, w).  Bounds (derived in tvop_common / DESIGN.md 4p): 1e-10 absolute on x, 2e-10 on change, 1e-12 relative on the
energy at the returned image, fourier_common.bound on the operators alone."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from mri_super_resolution_amd import _lib, baselines, ops
from tests import fourier_common as F
from tests import tvop_common as C
from tests import tvsr_common as T

pytestmark = pytest.mark.gpu


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _pair(kind, shape, lr_shape):
    if kind == "gaussian":
        return C.gaussian_pair(shape, lr_shape)
    if kind == "fourier_center_mirror":
        return C.fourier_pair(shape, lr_shape, "center", "mirror")
    if kind == "fourier_sample_periodic":
        return C.fourier_pair(shape, lr_shape, "sample", "periodic")
    return C.random_pair(shape, lr_shape, seed=shape[0] + lr_shape[1])


OPERATORS = ("gaussian", "fourier_center_mirror", "fourier_sample_periodic", "random")


@functools.lru_cache(maxsize=None)
def _case():
    return C.case_data()


@functools.lru_cache(maxsize=None)
def _case_minimum():
    hr, y, w, pair = _case()
    return C.lbfgs_minimum(y, *pair, C.CASE_LAM, C.CASE_ALPHA, w, C.CASE_SHAPE)


@pytest.mark.parametrize("shape,lr_shape", C.SHAPES)
def test_operators_against_the_restatement_and_each_other(shape, lr_shape):
    rng = np.random.default_rng(3)
    x, r = rng.standard_normal((2,) + shape), rng.standard_normal((2,) + lr_shape)
    for kind in OPERATORS:
        pair = _pair(kind, shape, lr_shape)
        ax, atr = baselines.operator_apply(x, pair), baselines.operator_adjoint(r, pair)
        want_ax, want_atr = C.apply(x, *pair), C.adjoint(r, *pair)
        e_ax, e_atr = np.abs(ax - want_ax).max(), np.abs(atr - want_atr).max()
        dot = abs((ax * r).sum() - (x * atr).sum()) / (np.abs(ax * r).sum() + np.abs(x * atr).sum())
        print(f"{shape} -> {lr_shape} {kind}: apply {e_ax:.2e} (bound {F.bound(x, want_ax):.2e}), adjoint {e_atr:.2e} "
              f"(bound {F.bound(r, want_atr):.2e}), dot test {dot:.2e}")
        assert isinstance(ax, np.ndarray) and ax.shape == (2,) + lr_shape and atr.shape == (2,) + shape
        assert e_ax <= F.bound(x, want_ax) and e_atr <= F.bound(r, want_atr)
        assert dot <= 1e-12
        # fp32 device tensors: the fp64 result rounded once
        x32 = _dev(x, torch.float32)
        got32 = baselines.operator_apply(x32, pair)
        assert got32.dtype == torch.float32 and torch.equal(got32, baselines.operator_apply(x32.double(), pair).float())
        r32 = _dev(r, torch.float32)
        assert torch.equal(baselines.operator_adjoint(r32, pair), baselines.operator_adjoint(r32.double(), pair).float())


@pytest.mark.parametrize("n_iter", [1, 2, 300])
def test_weighted_huber_case_against_the_restatement(n_iter):
    hr, y, w, pair = _case()
    want, want_e, want_ch = C.solve(y, *pair, C.CASE_LAM, C.CASE_ALPHA, n_iter, w=w, return_info=True)
    got, info = baselines.tv_superres_operator(y, pair, C.CASE_LAM, C.CASE_ALPHA, n_iter, weight=w, return_info=True)
    at = C.energy(got, y, *pair, C.CASE_LAM, C.CASE_ALPHA, w)
    e_x, e_ch, e_en = np.abs(got - want).max(), abs(info["change"] - want_ch), abs(info["energy"] - at) / at
    print(f"weighted Huber case, {n_iter} iterations: max|x diff| {e_x:.2e}, change {float(info['change']):.3e} (diff {e_ch:.2e}), energy "
          f"{float(info['energy']):.12e} (rel diff to the restated objective at the result {e_en:.2e}; restated run {want_e:.12e})")
    assert e_x <= C.X_BOUND and e_ch <= C.CHANGE_BOUND and e_en <= C.ENERGY_REL


@pytest.mark.parametrize("shape,lr_shape", C.SHAPES)
def test_ragged_shapes_against_the_restatement(shape, lr_shape):
    rng = np.random.default_rng(5)
    for kind in ("random", "fourier_center_mirror"):
        pair = _pair(kind, shape, lr_shape)
        y = C.apply(rng.random((2,) + shape), *pair) + 0.05 * rng.standard_normal((2,) + lr_shape)
        w = (0.5 + rng.random(y.shape)) * (rng.random(y.shape) > 0.2)
        x0 = rng.random((2,) + shape)
        for alpha in (0.0, 0.05):
            want, _, want_ch = C.solve(y, *pair, 0.05, alpha, 20, w=w, x0=x0, return_info=True)
            got, info = baselines.tv_superres_operator(y, pair, 0.05, alpha, 20, weight=w, x0=x0, return_info=True)
            at = C.energy(got, y, *pair, 0.05, alpha, w)
            e_x, e_ch, e_en = np.abs(got - want).max(), np.abs(info["change"] - want_ch).max(), (np.abs(info["energy"] - at) / at).max()
            print(f"{shape} -> {lr_shape} {kind} alpha {alpha}: max|x diff| {e_x:.2e}, change diff {e_ch:.2e}, energy rel diff {e_en:.2e}")
            assert e_x <= C.X_BOUND and e_ch <= C.CHANGE_BOUND and e_en <= C.ENERGY_REL


@pytest.mark.parametrize("n_iter", (0, 2))
def test_more_partials_than_the_finish_has_threads(n_iter):
    """(1024, 1024) -> (64, 64) is 1 LR tile and 256 HR tiles, 257 energy partials: thread 0 of the finish kernel adds two.  Without
    an iteration the change partials are never written and the change is 0."""
    pair = C.random_pair((1024, 1024), (64, 64), seed=2)
    y = np.random.default_rng(257).random((1, 64, 64))
    want, _, want_ch = C.solve(y, *pair, 0.05, 0.02, n_iter, return_info=True)
    got, info = baselines.tv_superres_operator(y, pair, 0.05, 0.02, n_iter, return_info=True)
    at = C.energy(got, y, *pair, 0.05, 0.02, None)
    e_x, e_ch, e_en = np.abs(got - want).max(), np.abs(info["change"] - want_ch).max(), (np.abs(info["energy"] - at) / at).max()
    print(f"(1024, 1024) -> (64, 64), {n_iter} iterations: max|x diff| {e_x:.2e}, change {info['change'].tolist()} (diff {e_ch:.2e}), "
          f"energy rel diff {e_en:.2e}")
    assert e_x <= C.X_BOUND and e_ch <= C.CHANGE_BOUND and e_en <= C.ENERGY_REL
    assert n_iter > 0 or not info["change"].any()


def test_the_minimum_is_reached():
    hr, y, w, pair = _case()
    low = _case_minimum()
    _, info = baselines.tv_superres_operator(y, pair, C.CASE_LAM, C.CASE_ALPHA, 1000, weight=w, return_info=True)
    gap = (float(info["energy"]) - low) / low
    print(f"weighted Huber case after 1,000 iterations: energy {float(info['energy']):.15e}, L-BFGS-B minimum {low:.15e}, gap {gap:.2e}")
    assert abs(gap) <= 1e-9


def test_against_the_block_solver():
    """6 x 10, factors (3, 2), kernels [1/3, 1/3, 1/3] and [0.2, 0.8], the weights of tvsr_common: two algorithms, one minimiser."""
    k0, k1 = np.full(3, 1.0 / 3.0), np.array([0.2, 0.8])
    k = np.outer(k0, k1)
    hr, _ = T.case_data()
    y = T.apply_A(hr, k)
    pair = (baselines.block_operator(6, 3, k0), baselines.block_operator(10, 2, k1))
    a, a_info = baselines.tv_superres_operator(y, pair, T.CASE_LAM, T.CASE_ALPHA, 1000, weight=T.CASE_W, return_info=True)
    b, b_info = baselines.tv_superres(y, T.CASE_FACTORS, k, T.CASE_LAM, T.CASE_ALPHA, 1000, weight=T.CASE_W, return_info=True)
    e_x = np.abs(a - b).max()
    e_en = abs(float(a_info["energy"][0]) - float(b_info["energy"][0])) / float(b_info["energy"][0])
    print(f"operator solver against the block solver after 1,000 iterations: max|x diff| {e_x:.2e}, energies "
          f"{float(a_info['energy'][0]):.15e} / {float(b_info['energy'][0]):.15e} (rel diff {e_en:.2e})")
    assert e_x <= 1e-10 and e_en <= 1e-12


def test_properties_that_need_no_restatement():
    rng = np.random.default_rng(7)
    shape, lr_shape = (130, 70), (37, 33)
    pair = C.random_pair(shape, lr_shape, 1)
    x0 = rng.random((2,) + shape)
    y = baselines.operator_apply(x0, pair)
    for n_iter in (1, 50):
        out, info = baselines.tv_superres_operator(y, pair, 0.0, 0.0, n_iter, x0=x0, return_info=True)
        print(f"lam = 0, y = A x0, {n_iter} iterations: bits kept {np.array_equal(out, x0)}, change {info['change']}")
        assert np.array_equal(out, x0) and np.all(info["change"] == 0)
    # n_iter = 0: the given start, or else the back-projection
    hr, yc, w, cpair = _case()
    given = rng.random(C.CASE_SHAPE)
    out, info = baselines.tv_superres_operator(yc, cpair, C.CASE_LAM, C.CASE_ALPHA, 0, weight=w, x0=given, return_info=True)
    assert np.array_equal(out, given) and info["change"] == 0
    out, info = baselines.tv_superres_operator(yc, cpair, C.CASE_LAM, C.CASE_ALPHA, 0, weight=w, return_info=True)
    want = C.default_start(yc, *cpair, w)
    e_start = np.abs(out - want).max()
    e_en = abs(info["energy"] - C.energy(out, yc, *cpair, C.CASE_LAM, C.CASE_ALPHA, w)) / info["energy"]
    print(f"n_iter = 0: back-projection max diff {e_start:.2e} (bound {F.bound(yc, want):.2e}), energy rel diff {e_en:.2e}")
    assert e_start <= F.bound(yc, want) and info["change"] == 0 and e_en <= C.ENERGY_REL
    fpair = C.fourier_pair(C.CASE_SHAPE, C.CASE_LR, "center", "mirror")                 # signed operators: the absolute values matter
    out = baselines.tv_superres_operator(yc, fpair, C.CASE_LAM, C.CASE_ALPHA, 0, weight=w)
    assert np.abs(out - C.default_start(yc, *fpair, w)).max() <= F.bound(yc, out)
    # a datum of weight 0 is never read
    assert w[2, 3] == 0
    base = baselines.tv_superres_operator(yc, cpair, C.CASE_LAM, C.CASE_ALPHA, 30, weight=w, return_info=True)
    for poison in (1e3, np.nan):
        yp = yc.copy()
        yp[2, 3] = poison
        out, info = baselines.tv_superres_operator(yp, cpair, C.CASE_LAM, C.CASE_ALPHA, 30, weight=w, return_info=True)
        assert np.array_equal(out, base[0]) and info["energy"] == base[1]["energy"] and info["change"] == base[1]["change"], poison
    # a NaN datum of positive weight: NaNs, no fault
    yp = yc.copy()
    yp[0, 0] = np.nan
    out = baselines.tv_superres_operator(yp, cpair, C.CASE_LAM, C.CASE_ALPHA, 30, weight=w)
    print(f"a NaN datum of positive weight: {int(np.isnan(out).sum())} of {out.size} results are NaN")
    assert np.isnan(out).any()
    torch.cuda.synchronize()


def test_a_batch_a_second_call_a_side_stream_and_a_capped_grid_give_equal_bits():
    rng = np.random.default_rng(11)
    hr, _, _, pair = _case()
    n = 40
    y = _dev(rng.random((n,) + C.CASE_LR))
    w = _dev((0.5 + rng.random((n,) + C.CASE_LR)) * (rng.random((n,) + C.CASE_LR) > 0.1))
    args = (pair, 0.02, 0.05, 25)
    solve = lambda yy, ww: baselines.tv_superres_operator(yy, *args, weight=ww, return_info=True)
    out, info = solve(y, w)
    differ = 0
    for i in range(n):
        one, one_info = solve(y[i:i + 1], w[i:i + 1])
        differ += int(not (torch.equal(one[0], out[i]) and torch.equal(one_info["energy"][0], info["energy"][i])
                           and torch.equal(one_info["change"][0], info["change"][i])))
    again, again_info = solve(y, w)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side, side_info = solve(y, w)
    side.synchronize()
    distinct = len({out[i].cpu().numpy().tobytes() for i in range(n)})
    print(f"{n} images {C.CASE_SHAPE} -> {C.CASE_LR}: {differ} differ from their solitary solve; second run equal {torch.equal(again, out)}; "
          f"side stream equal {torch.equal(on_side, out)}; {distinct} distinct results")
    assert differ == 0 and distinct == n
    for other, other_info in ((again, again_info), (on_side, side_info)):
        assert torch.equal(other, out) and torch.equal(other_info["energy"], info["energy"])
        assert torch.equal(other_info["change"], info["change"])
    # a grid of 3 workgroups on 2 x (130, 70) -> (37, 33): every kernel walks its stride loop
    shape, lr_shape = (130, 70), (37, 33)
    big = C.random_pair(shape, lr_shape, 2)
    yb = _dev(rng.random((2,) + lr_shape))
    free, free_info = baselines.tv_superres_operator(yb, big, 0.02, 0.05, 10, return_info=True)
    assert _lib.lib().inr_debug_set(32, 3) == 0
    try:
        capped, capped_info = baselines.tv_superres_operator(yb, big, 0.02, 0.05, 10, return_info=True)
        ax = baselines.operator_apply(free, big)
    finally:
        assert _lib.lib().inr_debug_set(32, 0) == 0
    print(f"grid capped at 3: equal {torch.equal(capped, free)}")
    assert torch.equal(capped, free) and torch.equal(capped_info["energy"], free_info["energy"])
    assert torch.equal(capped_info["change"], free_info["change"]) and torch.equal(ax, baselines.operator_apply(free, big))


def test_types_shapes_and_refusals():
    rng = np.random.default_rng(13)
    hr, _, _, pair = _case()
    y32 = _dev(rng.random((2, 3) + C.CASE_LR), torch.float32)
    w32 = _dev(0.5 + rng.random((2, 3) + C.CASE_LR), torch.float32)
    out32, info32 = baselines.tv_superres_operator(y32, pair, 0.02, 0.05, 40, weight=w32, return_info=True)
    out64, info64 = baselines.tv_superres_operator(y32.double(), pair, 0.02, 0.05, 40, weight=w32.double(), return_info=True)
    print(f"fp32 against fp64 rounded once: equal {torch.equal(out32, out64.float())}")
    assert out32.dtype == torch.float32 and out32.shape == (2, 3) + C.CASE_SHAPE and torch.equal(out32, out64.float())
    assert info32["energy"].shape == info32["change"].shape == (2, 3) and info32["energy"].dtype == torch.float64
    assert torch.equal(info32["energy"], info64["energy"]) and torch.equal(info32["change"], info64["change"])
    dev_pair = tuple(_dev(r) for r in pair)
    assert torch.equal(baselines.tv_superres_operator(y32, dev_pair, 0.02, 0.05, 40, weight=w32), out32)
    as_np = baselines.tv_superres_operator(rng.random((3,) + C.CASE_LR), pair, n_iter=3)
    assert isinstance(as_np, np.ndarray) and as_np.dtype == np.float64 and as_np.shape == (3,) + C.CASE_SHAPE
    # ops.* checks before it launches
    y = _dev(rng.random((2,) + C.CASE_LR))
    x = _dev(rng.random((2,) + C.CASE_SHAPE))
    need = ops.tvop_workspace_doubles(2, *C.CASE_SHAPE, *C.CASE_LR)
    ws = torch.empty(need, dtype=torch.float64, device="cuda")
    out, energy, change = ops.tvop_solve(y, dev_pair, 0.02, 0.05, 5, workspace=ws)
    assert torch.equal(out, ops.tvop_solve(y, dev_pair, 0.02, 0.05, 5)[0]) and energy.shape == change.shape == (2,)
    assert torch.equal(ops.tvop_apply(x, dev_pair, workspace=ws), ops.tvop_apply(x, dev_pair))
    with pytest.raises(ValueError, match="contiguous"):
        ops.tvop_solve(y.transpose(1, 2), dev_pair, 0.02, 0.05, 5)
    with pytest.raises(ValueError, match="contiguous"):
        ops.tvop_apply(x.transpose(1, 2), dev_pair)
    with pytest.raises(ValueError, match="contiguous"):
        ops.tvop_solve(y, (dev_pair[0].t().contiguous().t(), dev_pair[1]), 0.02, 0.05, 5)
    with pytest.raises(TypeError, match="float64"):
        ops.tvop_solve(y, (dev_pair[0].float(), dev_pair[1]), 0.02, 0.05, 5)
    with pytest.raises(TypeError, match="float64"):
        ops.tvop_apply(x.float(), dev_pair)
    with pytest.raises(TypeError, match="float64"):
        ops.tvop_adjoint(y.float(), dev_pair)
    with pytest.raises(TypeError, match="weight must be"):
        ops.tvop_solve(y, dev_pair, 0.02, 0.05, 5, weight=y.float())
    with pytest.raises(ValueError, match="weight has shape"):
        ops.tvop_solve(y, dev_pair, 0.02, 0.05, 5, weight=y[:1])
    with pytest.raises(ValueError, match="x0 has shape"):
        ops.tvop_solve(y, dev_pair, 0.02, 0.05, 5, x0=y)
    with pytest.raises(ValueError, match="y has shape"):
        ops.tvop_solve(x, dev_pair, 0.02, 0.05, 5)
    with pytest.raises(ValueError, match="lam must be finite and >= 0"):
        ops.tvop_solve(y, dev_pair, -1.0, 0.05, 5)
    with pytest.raises(ValueError, match="n_iter must be an integer 0 .. 100000"):
        ops.tvop_solve(y, dev_pair, 0.02, 0.05, 100001)
    for call in (lambda s: ops.tvop_solve(y, dev_pair, 0.02, 0.05, 5, workspace=s), lambda s: ops.tvop_apply(x, dev_pair, workspace=s),
                 lambda s: ops.tvop_adjoint(y, dev_pair, workspace=s)):
        with pytest.raises(ValueError, match=f"at least {need} elements"):
            call(ws[:need - 1])
        with pytest.raises(ValueError, match="workspace must be"):
            call(ws.float())


# ---- the scored study (scripts/acquisition_model) ---------------------------------------------------------------------------------------
def _synthetic_volume():
    """32 x 32 x 8 with two b-values: smooth blobs and an edge, the second b-value attenuated."""
    rng = np.random.default_rng(21)
    i, j = np.meshgrid(np.arange(32.0), np.arange(32.0), indexing="ij")
    vol = np.empty((32, 32, 8, 2))
    for z in range(8):
        base = np.exp(-((i - 14 - z) ** 2 + (j - 17) ** 2) / 60.0) + 0.5 * (j > 12 + z) + 0.05 * rng.random((32, 32))
        vol[:, :, z, 0], vol[:, :, z, 1] = base, base * np.exp(-0.8 * (1 + 0.3 * (i > 16)))
    return vol


def _run_study(tmp_path, name, volume, flags, b=None):
    from mri_super_resolution_amd import matio
    from mri_super_resolution_amd.scripts import acquisition_model as script
    path = str(tmp_path / name)
    matio.savemat(path, {"data_mean_b0": volume} if b is None else {"data_mean_b0": volume, "b": np.asarray(b, np.float64)})
    out = str(tmp_path / "am")
    summary = script.main(["--data", path, "--output_address", out, *map(str, flags)])[0]
    return summary, os.path.join(out, f"pat{summary['pt_id']}")


def _check_study(d, summary, volume, model, roi, which, b_index, noise, seed, iters, fwhm=None):
    """Every figure of the outputs against direct calls of the four methods on the LR data, and the LR data against the model."""
    from mri_super_resolution_amd import drivers, matio, metrics, reports
    rows = reports.read_csv(os.path.join(d, "acquisition_model.csv"))
    m = json.load(open(os.path.join(d, "metrics.json")))
    mat = matio.loadmat(os.path.join(d, "acquisition_model.mat"))
    R = roi[1] - roi[0]
    vol = np.asarray(volume, np.float64)
    vol = vol if vol.ndim == 4 else vol[..., None]
    vol = vol / vol.reshape(-1, vol.shape[-1]).max(axis=0)
    hr = np.ascontiguousarray(vol[roi[0]:roi[1], roi[0]:roi[1], :, b_index].transpose(2, 0, 1))[list(which)]
    assert np.array_equal(mat["hr"].transpose(2, 0, 1), hr)
    side = mat["lr"].shape[0]
    pair = drivers.acquisition_operators(model, R, side, fwhm)
    assert np.array_equal(mat["R0"], pair[0]) and np.array_equal(mat["R1"], pair[1]) and m["lr_side"] == side
    eta = np.stack([noise * np.random.default_rng(seed * 1000 + z).standard_normal((side, side)) for z in which])
    lr = baselines.operator_apply(hr, pair) + eta
    assert np.array_equal(mat["lr"].transpose(2, 0, 1), lr)
    whole = R % side == 0
    y = _dev(lr)
    direct = {"spline": (baselines.rescale(y.float(), R // side) if whole else baselines.resize(y.float(), (R, R))).double(),
              "zerofill": baselines.fourier_resize(y, (R, R), "center", "mirror")}
    if whole:
        direct["tv_block"] = baselines.tv_superres(y, (R // side, R // side), "mean", m["tv_lambda"], m["tv_huber"], iters)
    direct["tv_operator"] = baselines.tv_superres_operator(y, pair, m["tv_lambda"], m["tv_huber"], iters)
    assert tuple(m["methods"]) == tuple(direct) == tuple(summary["methods"])
    f32 = lambda t: t.float().contiguous()
    ref = _dev(hr)
    for name, img in direct.items():
        assert np.array_equal(mat[name].transpose(2, 0, 1), img.cpu().numpy()), name
        psnr = float(metrics.psnr(f32(ref), f32(img), 1.0, per_image=True).cpu().numpy().mean())      # the mean over the slices on the host
        ssim = metrics.ssim(f32(ref), f32(img), 1.0).cpu().numpy()
        got = np.array([float(r[f"SSIM-{name}"]) for r in rows])
        print(f"{model} {R} -> {side} {name}: PSNR {psnr:.4f} dB (metrics.json {m[f'psnr_{name}_db']:.4f}), SSIM mean {ssim.mean():.4f}, "
              f"max|csv - direct| {np.abs(got - ssim).max():.1e}")
        assert m[f"psnr_{name}_db"] == psnr and np.array_equal(got, ssim) and m[f"ssim_{name}_mean"] == float(ssim.mean())
    ax = baselines.operator_apply(direct["tv_operator"], pair)
    assert m["tv_operator_consistency_psnr_db"] == float(metrics.psnr(f32(y), f32(ax), 1.0, per_image=True).cpu().numpy().mean())
    assert [int(float(r["slice"])) for r in rows] == list(which) and len(rows) == len(which)
    return m, rows, mat


@pytest.mark.parametrize("model", ["kspace", "gaussian", "block"])
def test_the_study_scores_what_direct_calls_give(tmp_path, golden, model):
    volume = _synthetic_volume()
    flags = ["--model", model, "--roi_start", 2, "--roi_end", 30, "--b_index", 1, "--tv_iters", 100, "--seed", 3]
    summary, d = _run_study(tmp_path, "pat21_vol.mat", volume, flags, b=[0, 900])
    m, rows, _ = _check_study(d, summary, volume, model, (2, 30), range(8), 1, 0.02, 3, 100)
    assert m["b_value"] == 900.0 and all(float(r["b-value"]) == 900.0 for r in rows) and m["model"] == model
    pat07 = golden("pat07_volume.npz")["vol"]
    flags = ["--model", model, "--slices", 10, 14, 18, "--tv_iters", 100] + (["--fwhm", 1.0] if model == "gaussian" else [])
    summary, d = _run_study(tmp_path, "pat07_mean_b0.mat", pat07, flags)
    _check_study(d, summary, pat07, model, (40, 90), (10, 14, 18), 0, 0.02, 0, 100, 1.0 if model == "gaussian" else None)


def test_the_study_at_a_ratio_that_is_no_whole_number_has_no_block_row(tmp_path, golden):
    from mri_super_resolution_amd import drivers
    pat07 = golden("pat07_volume.npz")["vol"]
    summary, d = _run_study(tmp_path, "pat07_mean_b0.mat", pat07, ["--model", "kspace", "--lr_side", 20, "--slices", 10, 14, 18, "--tv_iters", 100])
    m, rows, mat = _check_study(d, summary, pat07, "kspace", (40, 90), (10, 14, 18), 0, 0.02, 0, 100)
    assert m["lr_side"] == 20 and mat["lr"].shape == (20, 20, 3) and mat["tv_operator"].shape == (50, 50, 3)
    assert "tv_block" not in mat and not any("tv_block" in k for k in m) and not any("tv_block" in k for k in rows[0])
    assert set(drivers.ACQUISITION_METHODS) - set(m["methods"]) == {"tv_block"}


def test_the_study_without_noise_under_the_block_model_gives_both_solvers_one_answer(tmp_path, golden):
    """--noise 0 --model block: tv_operator and tv_block minimise one objective; after 1,000 iterations they agree to the 1e-10 of the
    6 x 10 case, in one slice.  The two are different algorithms, so the bound holds only where both have CONVERGED in 1,000
    iterations: Chambolle-Pock is linear where the prior is smooth on the scale of the image's gradients, so the run uses lam 0.05 (the
    6 x 10 case's) and the Huber threshold 0.3 of tv_superres's own default.  The two float64 restatements (tvop_common.solve,
    tvsr_common.solve; CPU) then differ by 1.3e-15 on this slice after 1,000 iterations and by 8.5e-14 after 300; at the study's
    defaults (3e-3, 0.03) they are still 5.6e-4 apart after 1,000, which says nothing about either solver."""
    pat07 = golden("pat07_volume.npz")["vol"]
    summary, d = _run_study(tmp_path, "pat07_mean_b0.mat", pat07, ["--model", "block", "--noise", 0, "--slices", 14, "--tv_iters", 1000,
                                                                   "--tv_lambda", 0.05, "--tv_huber", 0.3])
    from mri_super_resolution_amd import matio
    mat = matio.loadmat(os.path.join(d, "acquisition_model.mat"))
    diff = np.abs(mat["tv_operator"] - mat["tv_block"]).max()
    print(f"block model, no noise, 1,000 iterations: max|tv_operator - tv_block| {diff:.2e}; PSNR {summary['psnr_tv_operator_db']:.4f} / "
          f"{summary['psnr_tv_block_db']:.4f} dB")
    assert diff <= 1e-10
