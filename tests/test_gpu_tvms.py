"""GPU: the multi-stack solver of csrc/tvms.hip against its float64 restatement (tests/tvms_common.py), against the sibling kernels it
reduces to (bit for bit where the issue says so), across a batch, streams and grids, and the study driver against the restatement.

Bounds are derived, not measured.  A_s / A_s^T in fp64 carry the project's 1e-12 of max(max|in|, max|want|).  The solver carries
1e-10 of max(1, max|want|): the iteration is non-expansive, and an iteration rounds, per voxel, about 20 times in the
prior's dual update, 12 in the divergence, 4 per gathered datum and, per datum, 3 per tap plus 5 -- at the tap counts used here (at
most 4 taps per stack over 3 stacks at 300 iterations; 16 taps or 8 stacks at fewer) under 100 roundings of 1.1e-16, which over 300
iterations is 3.3e-12 and leaves more than an order of margin.  ``change`` is the difference of two volumes that are each within the
bound: 2e-10.  ``energy`` is a sum of non-negative terms of a few roundings each, added in another order than NumPy's: 1e-12
relative.  Every test prints what it measured before it asserts."""
import numpy as np
import pytest
import torch

from tests import tvmf_common as MF
from tests import tvms_common as M
from tests import tvsr3d_common as T3
from mri_super_resolution_amd import _lib, baselines, drivers

pytestmark = pytest.mark.gpu

SOLVER_BOUND = 1e-10


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _geo(st):
    """The restatement's stack -> (the record of baselines.stack_geometry, its LR shape)."""
    f, taps, o, n = st
    return baselines.stack_geometry(f, taps, o), n


def _operator_cases():
    return [(M.CASE_SHAPE, st) for st in M.case_stacks()] + [M.limit_stack(), M.odd_stack()]


@pytest.mark.parametrize("case", range(5), ids=("overlapping", "gapped", "column_thick", "limits", "odd"))
def test_stack_operator_and_adjoint_match_the_restatement_and_each_other(case):
    shape, st = _operator_cases()[case]
    geo, n = _geo(st)
    rng = np.random.default_rng(case)
    x, r = rng.standard_normal((2,) + shape), rng.standard_normal((2,) + n)
    got_a, got_v = baselines.stack_apply(x, geo, n, return_valid=True)
    got_t = baselines.stack_adjoint(r, geo, shape)
    want_a = np.stack([M.apply(x[i], st) for i in range(2)])
    want_t = np.stack([M.adjoint(r[i], st, shape) for i in range(2)])
    want_v = np.stack([M.valid_mask(st, shape)] * 2)
    err_a, tol_a = np.abs(got_a - want_a).max(), 1e-12 * max(np.abs(x).max(), np.abs(want_a).max())
    err_t, tol_t = np.abs(got_t - want_t).max(), 1e-12 * max(np.abs(r).max(), np.abs(want_t).max())
    dot_a, dot_t, scale = float((got_a * r).sum()), float((x * got_t).sum()), float(np.abs(got_a * r).sum())
    print(f"{shape} {st[0]} L {[len(k) for k in st[1]]} o {st[2]} n {n}: |A - want| {err_a:.2e} (bound {tol_a:.2e}), |A^T - want| {err_t:.2e} "
          f"(bound {tol_t:.2e}), |<Ax, r> - <x, A^T r>| / sum|.| {abs(dot_a - dot_t) / scale:.2e}, valid {int(got_v.sum())} of {got_v.size}")
    assert got_a.dtype == got_t.dtype == np.float64 and got_v.dtype == np.bool_
    assert got_a.shape == (2,) + n and got_t.shape == (2,) + shape
    assert np.array_equal(got_v, want_v) and got_v.any() and (got_a[~got_v] == 0).all()
    assert err_a <= tol_a and err_t <= tol_t
    assert abs(dot_a - dot_t) <= 1e-12 * scale
    # NaN at the invalid data takes no part in the adjoint
    holed = np.where(want_v, r, np.nan)
    assert np.array_equal(baselines.stack_adjoint(holed, geo, shape), got_t)
    # the default LR shape holds the indices from 0 to the last whose footprint is inside
    assert baselines.stack_apply(x, geo).shape == (2,) + M.default_shape(st[0], st[1], st[2], shape)
    # device tensors come back as what they were; fp32 is the fp64 result rounded once
    x32 = _dev(x, torch.float32)
    got32 = baselines.stack_apply(x32, geo, n)
    assert got32.dtype == torch.float32 and torch.equal(got32, baselines.stack_apply(x32.double(), geo, n).float())


def test_a_block_stack_is_the_3d_block_operator_bit_for_bit():
    rng = np.random.default_rng(5)
    x, r = _dev(rng.random((2, 4, 6, 6))), _dev(rng.random((2, 2, 2, 3)))
    geo = baselines.stack_geometry(T3.CASE_FACTORS, T3.CASE_KERNEL)
    a, v = baselines.stack_apply(x, geo, return_valid=True)
    assert a.shape == (2, 2, 2, 3) and bool(v.all())
    assert torch.equal(a, baselines.block_apply3d(x, T3.CASE_FACTORS, T3.CASE_KERNEL))
    assert torch.equal(baselines.stack_adjoint(r, geo, (4, 6, 6)), baselines.block_adjoint3d(r, T3.CASE_FACTORS, T3.CASE_KERNEL))
    for kernel in ("mean", "decimate"):
        geo = baselines.stack_geometry((2, 3, 2), kernel)
        assert torch.equal(baselines.stack_apply(x, geo), baselines.block_apply3d(x, (2, 3, 2), kernel))
        assert torch.equal(baselines.stack_adjoint(r, geo, (4, 6, 6)), baselines.block_adjoint3d(r, (2, 3, 2), kernel))


def _compare(name, ys, stacks, shape, lam, alpha, n_iter, g=(1.0, 1.0, 1.0), w=None, x0=None, bound=SOLVER_BOUND):
    """One volume: the device solve through baselines against the restatement."""
    geos = [_geo(st)[0] for st in stacks]
    got, info = baselines.tv_superres_stacks(ys, geos, shape, lam, alpha, n_iter, g, weight=w, x0=x0, return_info=True)
    want, energy, change, valid = M.solve(ys, stacks, shape, lam, alpha, n_iter, g, w, x0, return_info=True)
    at_got = M.energy(got, ys, stacks, lam, alpha, w, g)
    err, tol = float(np.abs(got - want).max()), bound * max(1.0, float(np.abs(want).max()))
    e_rel = abs(float(info["energy"]) - at_got) / max(abs(at_got), 1e-300)
    c_err = abs(float(info["change"]) - change)
    print(f"{name}, {n_iter} iterations: max|got - restated| = {err:.3e} (bound {tol:.1e}), energy against the restated objective at the "
          f"returned volume {e_rel:.2e} relative, |change - restated| {c_err:.2e} (change {change:.2e}), valid fraction "
          f"{float(info['valid_fraction'])!r}")
    assert got.dtype == np.float64 and got.shape == want.shape == tuple(shape)
    assert err <= tol
    assert c_err <= 2 * bound
    assert e_rel <= 1e-12
    assert float(info["valid_fraction"]) == valid
    return got, info


@pytest.mark.parametrize("n_iter", (1, 2, 300))
@pytest.mark.parametrize("g", M.CASE_GRAD_WEIGHTS, ids=("g111", "g0411"))
def test_solver_matches_the_restatement_on_the_three_stack_case(n_iter, g):
    _, ys, ws = M.case_data()
    for alpha in (0.0, M.CASE_ALPHA):
        _compare(f"7x9x10, three stacks, weights, g {g}, huber {alpha}", ys, M.case_stacks(), M.CASE_SHAPE, M.CASE_LAM, alpha, n_iter, g, ws)


def test_solver_matches_the_restatement_with_and_without_x0_and_weights():
    hr, ys, ws = M.case_data()
    x0 = np.random.default_rng(7).random(M.CASE_SHAPE)
    _compare("7x9x10, three stacks, x0 given", ys, M.case_stacks(), M.CASE_SHAPE, M.CASE_LAM, M.CASE_ALPHA, 50, w=ws, x0=x0)
    _compare("7x9x10, three stacks, no weights", ys, M.case_stacks(), M.CASE_SHAPE, M.CASE_LAM, M.CASE_ALPHA, 50)
    for s, st in enumerate(M.case_stacks()):
        _compare(f"7x9x10, stack {s} alone", [ys[s]], [st], M.CASE_SHAPE, M.CASE_LAM, M.CASE_ALPHA, 50, w=[ws[s]])


def test_more_partials_than_the_finish_has_threads():
    """33 x 64 x 64 under one unit stack is 135,168 voxels and as many data, 264 parts: eight threads of the finish kernel add
    (maximise) two partials of energy, change and the count of valid data.  The bounds of _compare."""
    hr = (33, 64, 64)
    unit = M.stack((1, 1, 1), (M.ONE, M.ONE, M.ONE), (0, 0, 0), hr)
    _compare("33x64x64, one unit stack, 264 parts", [np.random.default_rng(264).random(hr)], [unit], hr, 0.05, 0.02, 3)


def test_one_slice_is_an_image_and_matches_the_multi_frame_solver():
    rng = np.random.default_rng(3)
    hr = rng.random((12, 10))
    shifts, f = np.array([[0.0, 0.0], [1.0, -1.0], [-2.0, 1.0]]), (3, 2)
    frames = MF.apply_frames(hr, MF.block_kernel("mean", f), shifts) + 0.01 * rng.standard_normal((3, 4, 5))
    x0 = MF.replicate(frames[0], f)
    stacks = [M.stack((1,) + f, (M.ONE, np.full(3, 1 / 3), np.full(2, 1 / 2)), (0, int(s[0]), int(s[1])), (1, 4, 5)) for s in shifts]
    got, _ = _compare("1x12x10, three whole-pixel frames", [fr[None] for fr in frames], stacks, (1, 12, 10), 0.05, 0.02, 100, x0=x0[None])
    multi = baselines.tv_superres_multi(frames, f, shifts, "mean", 0.05, 0.02, 100, x0=x0)
    err = float(np.abs(got[0] - multi).max())
    print(f"against tv_superres_multi at whole-pixel shifts: {err:.3e}")
    assert err <= 1e-10


def test_extents_of_one_on_two_axes():
    rng = np.random.default_rng(9)
    shape = (1, 1, 64)
    st = M.stack((1, 1, 4), (M.ONE, M.ONE, [.1, .2, .2, .2, .2, .1]), (0, 0, -1), (1, 1, 17))
    y = M.apply(rng.random(shape), st) + 0.01 * rng.standard_normal(st[3])
    assert 0 < M.valid_mask(st, shape).sum() < 17
    _compare("1x1x64, f 4, L 6", [y], [st], shape, 0.02, 0.01, 200)


def test_eight_stacks():
    rng = np.random.default_rng(10)
    shape = (6, 8, 9)
    hr = rng.random(shape)
    stacks = [M.stack((2, 1, 1), ([.5, .5], M.ONE, M.ONE), (o, 0, 0), hr_shape=shape) for o in (0, 1)]
    stacks += [M.stack((1, 2, 1), (M.ONE, [.25, .5, .25], M.ONE), (0, o, 0), hr_shape=shape) for o in (0, 1, -1)]
    stacks += [M.stack((1, 1, 3), (M.ONE, M.ONE, [.5, .5]), (0, 0, o), hr_shape=shape) for o in (0, 1, 2)]
    ys = [y + 0.01 * rng.standard_normal(y.shape) for y in M.apply_all(hr, stacks)]
    _compare("6x8x9, eight stacks", ys, stacks, shape, 0.02, 0.02, 100)


def test_sixteen_taps_at_spacing_eight():
    shape, st = M.limit_stack()
    rng = np.random.default_rng(12)
    y = M.apply(rng.random(shape), st)
    _compare("3x40x5, f 8, L 16", [y], [st], shape, 0.01, 0.02, 100)


def test_no_iterations_return_x0_or_the_back_projection_exactly():
    _, ys, ws = M.case_data()
    stacks, shape = M.case_stacks(), M.CASE_SHAPE
    geos = [_geo(st)[0] for st in stacks]
    x0 = np.random.default_rng(2).random(shape)
    out, info = baselines.tv_superres_stacks(ys, geos, shape, 0.05, 0.02, 0, x0=x0, return_info=True)
    assert np.array_equal(out, x0) and float(info["change"]) == 0.0
    assert abs(float(info["energy"]) - M.energy(x0, ys, stacks, 0.05, 0.02)) <= 1e-12 * float(info["energy"])
    bp = baselines.tv_superres_stacks(ys, geos, shape, 0.05, 0.02, 0, weight=ws)
    usable = [M.weights(stacks, shape, ws)[s] > 0 for s in range(3)]
    num = sum(baselines.stack_adjoint(np.where(u, y, 0.0), g, shape) for y, u, g in zip(ys, usable, geos))
    den = sum(baselines.stack_adjoint(u.astype(np.float64), g, shape) for u, g in zip(usable, geos))
    want = M.backproject(ys, stacks, shape, ws)
    print(f"back-projection against the restatement: {np.abs(bp - want).max():.2e}; voxels without a usable datum: {int((den == 0).sum())}")
    assert np.abs(bp - want).max() <= 1e-14
    assert np.abs(bp - np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)).max() <= 1e-14
    # one stack: the back-projection launch and the adjoint launch add the same terms in the same order
    valid = M.valid_mask(stacks[0], shape)
    one = baselines.tv_superres_stacks([ys[0]], [geos[0]], shape, 0.05, 0.02, 0)
    d0 = baselines.stack_adjoint(valid.astype(np.float64), geos[0], shape)
    n0 = baselines.stack_adjoint(np.where(valid, ys[0], 0.0), geos[0], shape)
    assert (d0 == 0).any() and np.array_equal(one, np.where(d0 > 0, n0 / np.where(d0 > 0, d0, 1.0), 0.0))


def test_prior_off_and_uncovered_voxels():
    """lam = 0 matches the restatement; in the gapped design with the prior off a voxel that no stack covers keeps x0."""
    _, ys, ws = M.case_data()
    _compare("7x9x10, three stacks, lam = 0", ys, M.case_stacks(), M.CASE_SHAPE, 0.0, 0.02, 100, w=ws)
    st = M.case_stacks()[1]                                                     # rows 1, 2 | 4, 5 | 7, 8 of 9 are covered
    x0 = np.random.default_rng(4).random(M.CASE_SHAPE)
    got, _ = _compare("7x9x10, the gapped stack, lam = 0", [ys[1]], [st], M.CASE_SHAPE, 0.0, 0.0, 100, x0=x0)
    covered = M.adjoint(np.ones(st[3]), st, M.CASE_SHAPE) > 0
    assert (~covered).sum() == 7 * 3 * 10 and np.array_equal(got[~covered], x0[~covered]) and not np.array_equal(got[covered], x0[covered])


def test_dead_stacks_nan_at_invalid_data_and_zero_weights():
    _, ys, ws = M.case_data()
    stacks, shape = M.case_stacks(), M.CASE_SHAPE
    geos = [_geo(st)[0] for st in stacks]
    args = (M.CASE_LAM, M.CASE_ALPHA, 40)
    base, base_info = baselines.tv_superres_stacks(ys, geos, shape, *args, weight=ws, return_info=True)
    # a dead stack -- every footprint outside, all data NaN -- leaves the bits alone, wherever it stands
    for offset in ((0, 40, 0), (1 << 20, 0, 0), (0, 0, -(1 << 20))):
        dead = baselines.stack_geometry((1, 2, 1), "mean", offset)
        nan = np.full((7, 4, 10), np.nan)
        for at in (0, 3):
            yy, gg, ww = list(ys), list(geos), list(ws)
            yy.insert(at, nan), gg.insert(at, dead), ww.insert(at, nan)
            out, info = baselines.tv_superres_stacks(yy, gg, shape, *args, weight=ww, return_info=True)
            assert np.array_equal(out, base), (offset, at)
            # the dead data move the boundaries of the parts: the energy is the same sum in another grouping, the change the same maximum
            assert abs(info["energy"] - base_info["energy"]) <= 1e-12 * base_info["energy"] and info["change"] == base_info["change"]
            total = sum(int(np.prod(st[3])) for st in stacks)
            assert abs(float(info["valid_fraction"]) * (total + nan.size) - float(base_info["valid_fraction"]) * total) < 1e-9
    # NaN at every invalid datum of the live stacks
    holed_y = [np.where(M.valid_mask(st, shape), y, np.nan) for st, y in zip(stacks, ys)]
    holed_w = [np.where(M.valid_mask(st, shape), w, np.nan) for st, w in zip(stacks, ws)]
    assert not all(np.isfinite(y).all() for y in holed_y)
    out = baselines.tv_superres_stacks(holed_y, geos, shape, *args, weight=holed_w)
    assert np.array_equal(out, base)
    # a zero weight equals dropping the datum: its y is not read
    poisoned = [y.copy() for y in ys]
    poisoned[1][3, 1, 4] = np.nan
    assert ws[1][3, 1, 4] == 0.0 and np.array_equal(baselines.tv_superres_stacks(poisoned, geos, shape, *args, weight=ws), base)


def test_fp32_is_the_fp64_result_rounded_once_and_types_come_back_as_given():
    _, ys, ws = M.case_data()
    geos = [_geo(st)[0] for st in M.case_stacks()]
    y32, w32 = [_dev(y, torch.float32) for y in ys], [_dev(w, torch.float32) for w in ws]
    args = (M.CASE_SHAPE, M.CASE_LAM, M.CASE_ALPHA, 60)
    out32, info32 = baselines.tv_superres_stacks(y32, geos, *args, weight=w32, return_info=True)
    out64, info64 = baselines.tv_superres_stacks([y.double() for y in y32], geos, *args, weight=[w.double() for w in w32], return_info=True)
    assert out32.dtype == torch.float32 and out64.dtype == torch.float64 and out32.shape == M.CASE_SHAPE
    assert torch.equal(out32, out64.float())
    assert torch.equal(info32["energy"], info64["energy"]) and torch.equal(info32["change"], info64["change"])
    x0 = torch.rand(M.CASE_SHAPE, device="cuda", dtype=torch.float32)
    assert torch.equal(baselines.tv_superres_stacks(y32, geos, *args, x0=x0),
                       baselines.tv_superres_stacks([y.double() for y in y32], geos, *args, x0=x0.double()).float())
    with pytest.raises(TypeError, match="the stacks must all be"):
        baselines.tv_superres_stacks([ys[0], y32[1], y32[2]], geos, *args)


def test_a_batch_beyond_the_grid_a_second_call_and_a_side_stream_give_equal_bits():
    """40 different volumes of the three-stack case under a grid cap of 7 workgroups (inr_debug_set(32, 7); tests/conftest.py resets
    it), so every kernel walks its stride loop: each volume against its solitary, uncapped solve; the same call again; the same call
    on another stream."""
    rng = np.random.default_rng(11)
    n, stacks, shape = 40, M.case_stacks(), M.CASE_SHAPE
    geos = [_geo(st)[0] for st in stacks]
    ys = [_dev(rng.random((n,) + st[3])) for st in stacks]
    ws = [_dev(rng.random((n,) + st[3]) * (rng.random((n,) + st[3]) > 0.1)) for st in stacks]
    args = (shape, 0.02, 0.05, 25)
    call = lambda y, w: baselines.tv_superres_stacks(y, geos, *args, weight=w, return_info=True)
    solo = [call([y[i:i + 1] for y in ys], [w[i:i + 1] for w in ws]) for i in range(n)]
    free, free_info = call(ys, ws)
    assert _lib.lib().inr_debug_set(32, 7) == 0
    try:
        out, info = call(ys, ws)
        again, again_info = call(ys, ws)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side, side_info = call(ys, ws)
        side.synchronize()
    finally:
        assert _lib.lib().inr_debug_set(32, 0) == 0
    differ = sum(int(not (torch.equal(one[0], out[i]) and torch.equal(one_info["energy"][0], info["energy"][i])
                          and torch.equal(one_info["change"][0], info["change"][i]))) for i, (one, one_info) in enumerate(solo))
    distinct = len({out[i].cpu().numpy().tobytes() for i in range(n)})
    print(f"{n} volumes of 7x9x10 under a grid of 7: {differ} differ from their solitary solve; uncapped equal {torch.equal(free, out)}; "
          f"second run equal {torch.equal(again, out)}; side stream equal {torch.equal(on_side, out)}; {distinct} distinct results")
    assert out.shape == (n,) + shape and distinct == n
    assert differ == 0
    for other, other_info in ((free, free_info), (again, again_info), (on_side, side_info)):
        assert torch.equal(other, out) and torch.equal(other_info["energy"], info["energy"])
        assert torch.equal(other_info["change"], info["change"]) and torch.equal(other_info["valid_fraction"], info["valid_fraction"])


@pytest.mark.parametrize("design", ("shifted", "orthogonal"))
def test_multi_stack_study_keeps_the_orderings_and_scores_what_the_restatement_scores(design):
    """pat07 ROI 40:90, no noise, lam = 3e-3, huber = 0.1, 300 iterations, PSNR over slices 2:-2."""
    ref = M.study_reference(design)
    res = drivers.multi_stack_study(M.pat07_roi(*M.STUDY_ROI), design, 2, 0.0, 0, None, M.STUDY_LAM, M.STUDY_HUBER, M.STUDY_ITERS)
    names = {f"stack{s}": name for s, name in enumerate(res["names"])}
    names.update(mean="mean", joint="joint")
    psnr = res["psnr"]
    for key, name in names.items():
        err = float(np.abs(res["volumes"][name].cpu().numpy() - ref[key][0]).max())
        print(f"{design} {name}: PSNR {psnr[name]:.4f} dB on the device, {ref[key][1]:.4f} dB restated, max|volume - restated| {err:.2e}")
    print({k: round(v, 3) for k, v in psnr.items()})
    for key, name in names.items():
        assert abs(psnr[name] - ref[key][1]) <= 1e-6
        assert np.abs(res["volumes"][name].cpu().numpy() - ref[key][0]).max() <= SOLVER_BOUND
    singles = [psnr[name] for name in res["names"]]
    if design == "shifted":
        assert psnr["joint"] >= singles[0] + 1.0
    else:
        assert psnr["joint"] >= max(singles) + 1.0 and psnr["joint"] >= psnr["mean"] + 1.0
    # a block stack alone is also scored by tv_superres3d
    assert np.isfinite(psnr["axial_tv3d"]) and res["volumes"]["axial_tv3d"].shape == (28, 50, 50)
    assert res["ssim"]["joint"].shape == (28,) and np.isfinite(res["ssim"]["joint"]).all()


def test_multi_stack_script_writes_what_the_driver_gives(tmp_path, golden):
    """scripts/multi_stack on pat07 (ROI 40:72, the overlap and the shifted design, noise 0.02, 30 iterations) against a direct call."""
    import json
    import os

    from mri_super_resolution_amd import matio
    from mri_super_resolution_amd.scripts import multi_stack as script

    path = str(tmp_path / "pat07_mean_b0.mat")
    matio.savemat(path, {"data_mean_b0": golden("pat07_volume.npz")["vol"]})
    vol = script.load_input_and_scale(path)[0]
    zfirst = np.ascontiguousarray(np.moveaxis(vol[40:72, 40:72, :, 0], 2, 0))
    for design, methods in (("overlap", ["axial_overlap"]), ("shifted", ["axial", "axial_tv3d", "axial_shifted", "mean", "joint"])):
        out = str(tmp_path / design)
        m = script.main(["--data", path, "--output_address", out, "--design", design, "--roi_start", "40", "--roi_end", "72", "--noise", "0.02",
                         "--seed", "3", "--tv_iters", "30"])[0]
        d = os.path.join(out, "pat07")
        res = drivers.multi_stack_study(zfirst, design, 2, 0.02, 3, None, None, None, 30)
        lines = open(os.path.join(d, "multi_stack.csv")).read().splitlines()
        assert lines[0] == ", ".join(["Pt_id", "slice"] + [f"SSIM-{name}" for name in methods]) and len(lines) == 1 + 28
        assert json.load(open(os.path.join(d, "metrics.json"))) == json.loads(json.dumps(m))
        assert m["design"] == design and m["hr_shape"] == [28, 32, 32] and m["tv_lambda"] == baselines.TVMS_DEFAULT_LAMBDA
        mat = matio.loadmat(os.path.join(d, "multi_stack.mat"))
        for name in methods:
            assert m[f"psnr_{name}_db"] == res["psnr"][name]
            assert np.array_equal(mat[name], res["volumes"][name].permute(1, 2, 0).cpu().numpy())
            row = [float(line.split(", ")[2 + methods.index(name)]) for line in lines[1:]]
            assert np.array_equal(np.array(row), res["ssim"][name].astype(np.float64))
        assert mat["hr"].shape == (32, 32, 28) and np.array_equal(mat[f"stack_{res['names'][0]}"], res["stacks"][0].cpu().numpy())
        assert set(m["solves"]) == set(res["info"]) and all(0 < v["valid_fraction"] <= 1 for v in m["solves"].values())
