"""GPU: the multi-frame TV / Huber solver of csrc/tvmf.hip against its float64 restatement (tests/tvmf_common.py), against properties
that do not rest on the restatement, across a batch, streams and grids, the shift estimate against planted shifts, and the two
drivers (``scripts/multi_frame``, ``rams_master --tv_multiframe``) against direct calls.

Bounds are derived, not measured.  A_k / A_k^T in fp64 carry the project's 1e-12 of max(max|in|, max|want|).  The solver carries the
1e-10 absolute of tests/test_gpu_tvsr.py on data in [0, 1]: the iteration is non-expansive, an iteration rounds about 10 + 4 K times
per pixel (K <= 8: 42 roundings of 1.1e-16), which over 300 iterations is 1.4e-12 and leaves nearly two orders of margin; ``change`` is
the difference of two images that are each within the bound: 2e-10.  ``energy`` is a sum of non-negative terms of a few roundings each,
added in another order than NumPy's: 1e-12 relative.  Every test prints what it measured before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

from tests import tvmf_common as M
from tests import tvsr_common as T2
from mri_super_resolution_amd import _lib, baselines, ops

pytestmark = pytest.mark.gpu

SOLVER_BOUND = 1e-10
OPERATOR_SHAPES = (((6, 10), (3, 2)), ((8, 8), (1, 1)), ((16, 24), (8, 8)), ((50, 50), (2, 2)))


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _ids(shapes):
    return ["x".join(map(str, s)) + "by" + "x".join(map(str, f)) for s, f in shapes]


def _kernels(f, rng):
    k = rng.random(f) + 0.1
    return {"mean": "mean", "decimate": "decimate", "random": k / k.sum()}


def _operator_shifts(f):
    """Two images of K = 4: zero, fractional, negative, a multiple of f; then mixed and large ones."""
    return np.array([[(0.0, 0.0), (0.25, 0.5), (-1.5, -0.75), (float(f[0]), -2.0 * f[1])],
                     [(0.5, 0.0), (0.0, -0.125), (-float(f[0]), 1.0), (2.75, 1.25)]])


@pytest.mark.parametrize("shape,f", OPERATOR_SHAPES, ids=_ids(OPERATOR_SHAPES))
def test_frame_operator_and_adjoint_match_the_restatement_and_each_other(shape, f):
    rng = np.random.default_rng(int(np.prod(shape)))
    H, W = shape
    h, w = H // f[0], W // f[1]
    shifts = _operator_shifts(f)
    x, r = rng.standard_normal((2, H, W)), rng.standard_normal((2, 4, h, w))
    for name, kernel in _kernels(f, rng).items():
        k = M.block_kernel(kernel, f)
        got_a, got_v = baselines.frame_apply(x, f, shifts, kernel, return_valid=True)
        got_t = baselines.frame_adjoint(r, f, shifts, kernel)
        want_a = np.stack([M.apply_frames(x[i], k, shifts[i]) for i in range(2)])
        want_v = np.stack([[M.valid_mask(k, s, H, W) for s in shifts[i]] for i in range(2)])
        want_t = np.stack([M.adjoint_frames(r[i], k, shifts[i], H, W) for i in range(2)])
        err_a, tol_a = np.abs(got_a - want_a).max(), 1e-12 * max(np.abs(x).max(), np.abs(want_a).max())
        err_t, tol_t = np.abs(got_t - want_t).max(), 1e-12 * max(np.abs(r).max(), np.abs(want_t).max())
        dot_a, dot_t = float((got_a * r).sum()), float((x * got_t).sum())
        scale = float(np.abs(got_a * r).sum())
        print(f"{shape} {f} {name}: |A - want| {err_a:.2e} (bound {tol_a:.2e}), |A^T - want| {err_t:.2e} (bound {tol_t:.2e}), "
              f"|<Ax, r> - <x, A^T r>| / sum|.| {abs(dot_a - dot_t) / max(scale, 1e-300):.2e}, valid {int(got_v.sum())} of {got_v.size}, "
              f"mask equal {np.array_equal(got_v, want_v)}")
        assert got_a.dtype == got_t.dtype == np.float64 and got_v.dtype == np.bool_
        assert got_a.shape == want_a.shape == (2, 4, h, w) and got_t.shape == (2, H, W)
        assert np.array_equal(got_v, want_v) and 0 < got_v.sum() < got_v.size
        assert err_a <= tol_a and err_t <= tol_t
        assert abs(dot_a - dot_t) <= 1e-12 * scale
        # zero shifts: block_apply bit for bit, every datum valid; [K, 2] shifts serve all images
        zero_a, zero_v = baselines.frame_apply(x, f, np.zeros((3, 2)), kernel, return_valid=True)
        block = baselines.block_apply(x, f, kernel)
        assert zero_v.all() and all(np.array_equal(zero_a[:, j], block) for j in range(3))
        assert np.array_equal(baselines.frame_adjoint(r[:, :1], f, np.zeros((1, 2)), kernel), baselines.block_adjoint(r[:, 0], f, kernel))
        # device tensors come back as what they were; fp32 is the fp64 result rounded once
        x32 = _dev(x, torch.float32)
        got32 = baselines.frame_apply(x32, f, _dev(shifts), kernel)
        assert got32.dtype == torch.float32 and torch.equal(got32, baselines.frame_apply(x32.double(), f, shifts, kernel).float())


def _solve_restated(frames, f, shifts, kernel, lam, alpha, n_iter, w=None, x0=None):
    """tvmf_common.solve image by image over a leading axis; shifts [n, K, 2]."""
    outs = [M.solve(frames[i], f, shifts[i], kernel, lam, alpha, n_iter, None if w is None else w[i], None if x0 is None else x0[i],
                    return_info=True) for i in range(len(frames))]
    return tuple(np.array([o[j] for o in outs]) for j in range(4))


def _compare(name, frames, f, shifts, kernel, lam, alpha, n_iter, w=None, x0=None):
    got, info = baselines.tv_superres_multi(frames, f, shifts, kernel, lam, alpha, n_iter, weight=w, x0=x0, return_info=True)
    want, energy, change, valid = _solve_restated(frames, f, shifts, kernel, lam, alpha, n_iter, w, x0)
    k = M.block_kernel(kernel, f)
    at_got = np.array([M.energy(got[i], frames[i], k, shifts[i], lam, alpha, None if w is None else w[i]) for i in range(len(got))])
    err = float(np.abs(got - want).max())
    e_rel = float((np.abs(info["energy"] - at_got) / np.maximum(np.abs(at_got), 1e-300)).max())
    c_err = float(np.abs(info["change"] - change).max())
    print(f"{name}, {n_iter} iterations: max|got - restated| = {err:.3e} (bound {SOLVER_BOUND:.0e}), energy against the restated "
          f"objective at the returned image {e_rel:.2e} relative, |change - restated| {c_err:.2e} (change {float(change.max()):.2e}), "
          f"valid fraction {info['valid_fraction'].tolist()}")
    assert got.dtype == np.float64 and got.shape == want.shape
    assert err <= SOLVER_BOUND
    assert c_err <= 2 * SOLVER_BOUND
    assert e_rel <= 1e-12
    assert np.array_equal(info["valid_fraction"], valid)
    return got, info


@pytest.mark.parametrize("n_iter", (1, 2, 300))
def test_solver_matches_the_restatement_on_the_three_frame_case(n_iter):
    _, frames, w = M.case_data()
    _compare("6x10 (3, 2), 3 frames, frame weights 1 / 0.5 / 2", frames[None], M.CASE_FACTORS, M.CASE_SHIFTS[None], "mean", M.CASE_LAM,
             M.CASE_ALPHA, n_iter, w=w[None])


@pytest.fixture(scope="module")
def pat07():
    return M.pat07_roi()                    # [28, 50, 50] in [0, 1]


@pytest.mark.parametrize("alpha", (0.0, 0.1), ids=("tv", "huber"))
def test_solver_matches_the_restatement_on_a_pat07_slice(pat07, alpha):
    rng = np.random.default_rng(14)
    shifts = rng.uniform(-1.5, 1.5, (8, 2))
    shifts[0] = 0.0
    frames = M.apply_frames(pat07[14], M.block_kernel("mean", (2, 2)), shifts) + 0.02 * rng.standard_normal((8, 25, 25))
    _compare(f"pat07 slice 14, 50x50 (2, 2), 8 frames, huber {alpha}", frames[None], (2, 2), shifts[None], "mean", 0.02, alpha, 300)


RAGGED = (((7, 1024), (7, 1)), ((1024, 3), (1, 3)))


@pytest.mark.parametrize("shape,f", RAGGED, ids=_ids(RAGGED))
def test_solver_matches_the_restatement_on_ragged_shapes(shape, f):
    """No side is a multiple of the workgroup (256 threads) or of a part (1,024 elements); one axis is a single block, the other has
    one pixel per block; 2 images, 3 frames, random kernels, weights with zeros, a given x0."""
    rng = np.random.default_rng(shape[0])
    hr = rng.random((2,) + shape)
    shifts = rng.uniform(-2.0, 2.0, (2, 3, 2))
    shifts[:, 0] = 0.0
    for name, kernel in _kernels(f, rng).items():
        k = M.block_kernel(kernel, f)
        frames = np.stack([M.apply_frames(hr[i], k, shifts[i]) for i in range(2)])
        w = rng.random(frames.shape) * (rng.random(frames.shape) > 0.1)
        _compare(f"{shape} {f} {name}", frames, f, shifts, kernel, 0.02, 0.05, 40, w=w, x0=rng.random(hr.shape))


def test_more_partials_than_the_finish_has_threads():
    """512 x 512 with unit factors and one frame is 512 parts: every thread of the finish kernel adds (maximises) two partials of
    energy, change and the count of valid data.  The bounds of _compare."""
    rng = np.random.default_rng(512)
    _compare("512x512 (1, 1), K = 1, 512 parts", rng.random((1, 1, 512, 512)), (1, 1), np.array([[(0.25, -0.5)]]), "mean", 0.05, 0.02, 3)


def test_one_frame_and_unit_factors_match_the_restatement():
    rng = np.random.default_rng(21)
    hr = rng.random((1, 12, 10))
    k = M.block_kernel("mean", (3, 2))
    one = np.array([[(0.5, -0.25)]])
    _compare("12x10 (3, 2), K = 1", M.apply_frames(hr[0], k, one[0])[None], (3, 2), one, "mean", 0.02, 0.05, 60, x0=rng.random(hr.shape))
    five = rng.uniform(-1.0, 1.0, (1, 5, 2))
    frames = M.apply_frames(hr[0], np.ones((1, 1)), five[0])[None] + 0.02 * rng.standard_normal((1, 5, 12, 10))
    _compare("12x10 (1, 1), 5 fractional frames", frames, (1, 1), five, "mean", 0.05, 0.02, 60)


def test_energy_reaches_the_lbfgs_minimum_which_shares_nothing_with_the_iteration():
    hr, frames, w = M.case_data()
    minimum = M.lbfgs_minimum(frames, M.block_kernel("mean", M.CASE_FACTORS), M.CASE_SHIFTS, M.CASE_LAM, M.CASE_ALPHA, w, hr.shape)
    _, info = baselines.tv_superres_multi(frames, M.CASE_FACTORS, M.CASE_SHIFTS, "mean", M.CASE_LAM, M.CASE_ALPHA, 300, weight=w,
                                          return_info=True)
    gap = (float(info["energy"]) - minimum) / minimum
    print(f"L-BFGS-B minimum {minimum:.12f}, energy after 300 iterations {float(info['energy']):.12f}, relative gap {gap:.2e}")
    assert abs(gap) <= 1e-9


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in ((a[0], b[0]), (a[1]["energy"], b[1]["energy"]), (a[1]["change"], b[1]["change"])))


def test_properties_that_do_not_rest_on_the_restatement():
    rng = np.random.default_rng(5)
    hr, frames, w = M.case_data()
    f = M.CASE_FACTORS
    args = ("mean", M.CASE_LAM, M.CASE_ALPHA)
    # n_iter = 0 returns x0: the given one, or the block replication of frame 0
    x0 = rng.random(hr.shape)
    x, info = baselines.tv_superres_multi(frames, f, M.CASE_SHIFTS, *args, 0, x0=x0, return_info=True)
    assert np.array_equal(x, x0) and float(info["change"]) == 0.0
    x, info = baselines.tv_superres_multi(frames, f, M.CASE_SHIFTS, *args, 0, return_info=True)
    assert np.array_equal(x, M.replicate(frames[0], f)) and float(info["change"]) == 0.0
    # lambda = 0 with one frame at rest: the replication start satisfies the data and stays, exactly (power-of-two factors and data
    # that are multiples of 2^-10, so that every partial sum of the block mean is exact)
    for ff in ((2, 2), (1, 1), (4, 2)):
        y = rng.integers(0, 1025, (8 // ff[0], 12 // ff[1])) / 1024.0
        for n_iter in (1, 50):
            x, info = baselines.tv_superres_multi(y[None], ff, np.zeros((1, 2)), "mean", 0.0, 0.0, n_iter, return_info=True)
            print(f"lambda = 0, one frame at rest, {ff}, {n_iter} iterations: x == x0 {np.array_equal(x, M.replicate(y, ff))}, energy "
                  f"{float(info['energy']):.2e}, change {float(info['change']):.2e}")
            assert np.array_equal(x, M.replicate(y, ff)) and float(info["energy"]) == 0.0 and float(info["change"]) == 0.0
    # a frame that holds no valid datum -- a shift beyond 2^20, a NaN, one simply far outside -- is no frame at all: the bits of x,
    # energy and change are those of the solve without it, whatever its data hold
    base = baselines.tv_superres_multi(frames, f, M.CASE_SHIFTS, *args, 30, weight=w, return_info=True)
    junk = np.full((1,) + frames.shape[1:], np.nan)
    for dead in ((1e9, 0.0), (np.nan, 0.5), (0.0, -np.inf), (40.0, 0.0), (0.0, -40.5), (2.0 ** 20 + 1, 0.0)):
        for data in (junk, rng.random(junk.shape)):
            more = baselines.tv_superres_multi(np.concatenate([frames, data]), f, np.concatenate([M.CASE_SHIFTS, [dead]]), *args, 30,
                                               weight=np.concatenate([w, np.ones_like(junk)]), return_info=True)
            same = _same(base, more)
            print(f"a fourth frame at {dead}, data {'NaN' if data is junk else 'random'}: bits of x, energy, change unchanged {same}; valid "
                  f"fraction {float(more[1]['valid_fraction']):.3f} against {float(base[1]['valid_fraction']):.3f}")
            assert same and float(more[1]["valid_fraction"]) == pytest.approx(0.75 * float(base[1]["valid_fraction"]), rel=1e-15)
    # y = NaN on every invalid datum changes no bit
    valid = np.stack([M.valid_mask(M.block_kernel("mean", f), s, *hr.shape) for s in M.CASE_SHIFTS])
    holes = np.where(valid, frames, np.nan)
    assert 0 < valid.sum() < valid.size and np.isnan(holes).any()
    assert _same(base, baselines.tv_superres_multi(holes, f, M.CASE_SHIFTS, *args, 30, weight=w, return_info=True))
    # and so does the weight there; a weight of 0 hides a valid datum likewise
    w_other = np.where(valid, w, 7.0)
    assert _same(base, baselines.tv_superres_multi(holes, f, M.CASE_SHIFTS, *args, 30, weight=w_other, return_info=True))
    w0 = w.copy()
    w0[0, 1, 2] = 0.0
    other = frames.copy()
    other[0, 1, 2] = 1e3
    a = baselines.tv_superres_multi(frames, f, M.CASE_SHIFTS, *args, 30, weight=w0, x0=x0, return_info=True)
    assert _same(a, baselines.tv_superres_multi(other, f, M.CASE_SHIFTS, *args, 30, weight=w0, x0=x0, return_info=True))
    assert not np.array_equal(a[0], baselines.tv_superres_multi(frames, f, M.CASE_SHIFTS, *args, 30, weight=w, x0=x0))


def test_fp32_is_the_fp64_result_rounded_once_and_types_come_back_as_given():
    rng = np.random.default_rng(9)
    hr, frames, w = M.case_data()
    y32, w32, x32 = _dev(frames, torch.float32), _dev(w, torch.float32), _dev(rng.random(hr.shape), torch.float32)
    shifts = _dev(M.CASE_SHIFTS)
    args = (M.CASE_FACTORS, shifts, "mean", M.CASE_LAM, M.CASE_ALPHA, 100)
    got, info = baselines.tv_superres_multi(y32, *args, weight=w32, x0=x32, return_info=True)
    want, winfo = baselines.tv_superres_multi(y32.double(), *args, weight=w32.double(), x0=x32.double(), return_info=True)
    same = torch.equal(got, want.float())
    print(f"fp32 out == fp64 out rounded once: {same}; max|fp32 - fp64| = {float((got.double() - want).abs().max()):.2e}")
    assert got.dtype == torch.float32 and want.dtype == torch.float64 and got.is_cuda and info["energy"].dtype == torch.float64
    assert same
    assert torch.equal(info["energy"], winfo["energy"]) and torch.equal(info["change"], winfo["change"])
    # leading axes are a batch and keep their shape
    stack = _dev(rng.random((2, 3, 5, 4, 6)), torch.float32)
    each = _dev(rng.uniform(-1, 1, (2, 3, 5, 2)))
    out, info = baselines.tv_superres_multi(stack, (2, 1), each, n_iter=5, return_info=True)
    assert out.shape == (2, 3, 8, 6) and out.dtype == torch.float32
    assert info["energy"].shape == info["change"].shape == info["valid_fraction"].shape == (2, 3)
    shared = baselines.tv_superres_multi(stack, (2, 1), each[0, 0], n_iter=5)
    assert torch.equal(shared[0, 0], out[0, 0]) and not torch.equal(shared[1, 2], out[1, 2])
    assert isinstance(baselines.tv_superres_multi(rng.random((3, 4, 6)), (2, 2), np.zeros((3, 2)), n_iter=3), np.ndarray)
    assert baselines.frame_apply(_dev(rng.random((2, 3, 8, 6))), (2, 1), each).shape == (2, 3, 5, 4, 6)
    assert baselines.frame_adjoint(stack, (2, 1), each).shape == (2, 3, 8, 6)


def test_a_batch_beyond_the_grid_a_second_call_and_a_side_stream_give_equal_bits():
    """300 different 12 x 12 images, factors (2, 3), 3 frames, each with its own shifts and weights, under a grid cap of 7 workgroups
    (inr_debug_set(32, 7); tests/conftest.py resets it), so every kernel walks its stride loop: each image against its solitary,
    uncapped solve; the same call again; the same call on another stream."""
    rng = np.random.default_rng(11)
    n, f = 300, (2, 3)
    y = _dev(rng.random((n, 3, 6, 4)))
    w = _dev(rng.random((n, 3, 6, 4)) * (rng.random((n, 3, 6, 4)) > 0.1))
    shifts = rng.uniform(-2.0, 2.0, (n, 3, 2))
    shifts[:, 0] = 0.0
    shifts = _dev(shifts)
    args = ("mean", 0.02, 0.05, 25)
    solo = [baselines.tv_superres_multi(y[i:i + 1], f, shifts[i:i + 1], *args, weight=w[i:i + 1], return_info=True) for i in range(n)]
    free, free_info = baselines.tv_superres_multi(y, f, shifts, *args, weight=w, return_info=True)
    assert _lib.lib().inr_debug_set(32, 7) == 0
    try:
        out, info = baselines.tv_superres_multi(y, f, shifts, *args, weight=w, return_info=True)
        again, again_info = baselines.tv_superres_multi(y, f, shifts, *args, weight=w, return_info=True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side, side_info = baselines.tv_superres_multi(y, f, shifts, *args, weight=w, return_info=True)
        side.synchronize()
    finally:
        assert _lib.lib().inr_debug_set(32, 0) == 0
    differ = sum(int(not (torch.equal(one[0], out[i]) and torch.equal(one_info["energy"][0], info["energy"][i])
                          and torch.equal(one_info["change"][0], info["change"][i]))) for i, (one, one_info) in enumerate(solo))
    distinct = len({out[i].cpu().numpy().tobytes() for i in range(n)})
    print(f"{n} images of 12x12 under a grid of 7: {differ} differ from their solitary solve; uncapped equal {torch.equal(free, out)}; "
          f"second run equal {torch.equal(again, out)}; side stream equal {torch.equal(on_side, out)}; {distinct} distinct results")
    assert out.shape == (n, 12, 12) and distinct == n
    assert differ == 0
    for other, other_info in ((free, free_info), (again, again_info), (on_side, side_info)):
        assert torch.equal(other, out) and torch.equal(other_info["energy"], info["energy"])
        assert torch.equal(other_info["change"], info["change"])


def test_ops_wrappers_check_before_they_launch():
    y = torch.rand(2, 3, 3, 5, device="cuda", dtype=torch.float64)
    s = torch.zeros(2, 3, 2, device="cuda", dtype=torch.float64)
    k, f = [[0.5], [0.5]], (2, 1)
    out, energy, change, valid = ops.tvmf_solve(y, s, f, k, 0.01, 0.0, 3)
    assert out.shape == (2, 6, 5) and energy.shape == change.shape == valid.shape == (2,) and bool((valid == 1).all())
    need = ops.tvmf_workspace_doubles(2, 3, 6, 5, f)
    assert need >= 2 * (4 * 30 + 3 * 15)
    with pytest.raises(ValueError, match="contiguous"):
        ops.tvmf_solve(y[:, :, :, ::2], s, f, k, 0.01, 0.0, 3)
    with pytest.raises(TypeError, match="float32 or torch.float64"):
        ops.tvmf_solve(y.half(), s, f, k, 0.01, 0.0, 3)
    with pytest.raises(TypeError, match="shifts must be torch.float64"):
        ops.tvmf_solve(y, s.float(), f, k, 0.01, 0.0, 3)
    with pytest.raises(ValueError, match=r"shifts must be a contiguous \[2, 3, 2\]"):
        ops.tvmf_solve(y, s[:, :2].contiguous(), f, k, 0.01, 0.0, 3)
    with pytest.raises(ValueError, match="weight has shape"):
        ops.tvmf_solve(y, s, f, k, 0.01, 0.0, 3, weight=y[:1].contiguous())
    with pytest.raises(ValueError, match="sum to 1"):
        ops.tvmf_solve(y, s, f, [[1.0], [1.0]], 0.01, 0.0, 3)
    with pytest.raises(ValueError, match=f"workspace must be a device float64 tensor of at least {need}"):
        ops.tvmf_solve(y, s, f, k, 0.01, 0.0, 3, workspace=torch.empty(need - 1, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="n_iter must be an integer 0 .. 100000"):
        ops.tvmf_solve(y, s, f, k, 0.01, 0.0, -1)
    with pytest.raises(ValueError, match="frames per image are 1 .. 64"):
        ops.tvmf_solve(torch.rand(1, 65, 2, 2, device="cuda", dtype=torch.float64), torch.zeros(1, 65, 2, device="cuda",
                                                                                               dtype=torch.float64), f, k, 0.01, 0.0, 1)
    assert torch.equal(ops.frame_apply(out, s, f, k)[:, 0], ops.block_apply(out, f, k))


# ---- the shift estimate ------------------------------------------------------------------------------------------------------------------
PLANTED = {4: ((0, 0), (1, -1), (-2, 1), (0.5, 1.5), (-1.5, -0.5), (2, 2)), 2: ((0, 0), (1, -1), (-2, 1), (2, 0), (-1, -2), (2, 2))}


@pytest.fixture(scope="module")
def study_roi():
    return M.pat07_roi(*M.STUDY_ROI)         # [28, 72, 72] in [0, 1]


@pytest.mark.parametrize("upsample", (4, 2))
def test_estimated_shifts_are_within_one_step_of_the_planted_ones(study_roi, upsample):
    """pat07 ROI 30:102, slices 10 / 14 / 18, factors (2, 2), 6 frames, noise 0 and 0.02: every estimate within one step f / upsample
    of the planted shift.  The oracles alone meet the condition (tests/test_tvmf_cpu.py repeats it without a device)."""
    planted = np.array(PLANTED[upsample], np.float64)
    step = 2.0 / upsample
    rng = np.random.default_rng(1)
    for noise in (0.0, 0.02):
        frames = np.stack([M.simulate(study_roi[z], (2, 2), planted) for z in M.STUDY_SLICES])
        frames = frames + noise * rng.standard_normal(frames.shape)
        got = baselines.estimate_shifts(frames, (2, 2), upsample, 4)
        on_device = baselines.estimate_shifts(_dev(frames, torch.float32), (2, 2), upsample, 4)
        err = np.abs(got - planted).max(axis=(1, 2))
        print(f"upsample {upsample}, noise {noise}: max |estimate - planted| per slice {err.tolist()} HR pixels (step {step})")
        assert got.shape == (3, 6, 2) and got.dtype == np.float64 and np.array_equal(got[:, 0], np.zeros((3, 2)))
        assert on_device.is_cuda and on_device.dtype == torch.float64 and on_device.shape == (3, 6, 2)
        assert np.abs(on_device.cpu().numpy() - planted).max() <= step
        assert err.max() <= step
    assert np.array_equal(baselines.estimate_shifts(frames[0], (2, 2), upsample, 4, reference=2)[2], np.zeros(2))


# ---- the study ---------------------------------------------------------------------------------------------------------------------------
def test_multi_frame_study_scores_what_direct_calls_give_and_keeps_the_order_of_the_rows(tmp_path, golden, study_roi):
    """Slices 10 / 14 / 18 of pat07, ROI 30:102, 8 frames, the seed of tvmf_common (checked against both conditions with the
    restatement in tests/test_tvmf_cpu.py), 300 iterations."""
    from mri_super_resolution_amd import matio, metrics, reports
    from mri_super_resolution_amd.scripts import multi_frame as mf_script
    path = str(tmp_path / "pat07_mean_b0.mat")
    matio.savemat(path, {"data_mean_b0": golden("pat07_volume.npz")["vol"]})
    out = str(tmp_path / "mf")
    res = mf_script.main(["--data", path, "--output_address", out, "--slices", *map(str, M.STUDY_SLICES), "--seed", str(M.STUDY_SEED)])[0]
    d = os.path.join(out, "pat07")
    rows = reports.read_csv(os.path.join(d, "multi_frame.csv"))
    m = json.load(open(os.path.join(d, "metrics.json")))
    mat = matio.loadmat(os.path.join(d, "multi_frame.mat"))
    assert [int(r["slice"]) for r in rows] == list(M.STUDY_SLICES) and m == json.loads(json.dumps(res))
    # the frames are the restated simulation of the same draws
    frames = np.ascontiguousarray(mat["frames"].transpose(3, 2, 0, 1))                 # [Z, K, h, w]
    for i, z in enumerate(M.STUDY_SLICES):
        shifts, want = M.study_frames(study_roi[z], M.STUDY_SEED * 1000 + z)
        assert np.array_equal(mat["shifts"][i], shifts) and np.abs(frames[i] - want).max() <= 1e-12
        assert np.abs(mat["hr"][:, :, i] - study_roi[z]).max() == 0.0
    # the five columns are direct calls of the public functions on those frames
    est = baselines.estimate_shifts(frames, (2, 2), 4, 2.5 / 2)
    direct = {"replicate": np.stack([M.replicate(f[0], (2, 2)) for f in frames]), "tv": baselines.tv_superres(frames[:, 0], (2, 2)),
              "ignored": baselines.tv_superres_multi(frames, (2, 2), np.zeros((8, 2))),
              "estimated": baselines.tv_superres_multi(frames, (2, 2), est), "true": baselines.tv_superres_multi(frames, (2, 2), mat["shifts"])}
    hr = np.ascontiguousarray(mat["hr"].transpose(2, 0, 1))
    crop = lambda a: _dev(a[:, 4:-4, 4:-4], torch.float32)
    table = {}
    for name, images in direct.items():
        want = metrics.psnr(crop(hr), crop(images), 1.0, per_image=True).cpu().numpy()
        table[name] = np.array([float(r[f"PSNR-{name}"]) for r in rows])
        print(f"PSNR-{name}: {table[name].round(2).tolist()} dB (direct {want.round(2).tolist()}), restated margin PSNR of the direct image "
              f"{[round(M.margin_psnr(hr[i], images[i]), 2) for i in range(3)]}")
        assert np.array_equal(table[name], want) and np.array_equal(mat[name].transpose(2, 0, 1), images)
        assert m[f"psnr_{name}_db"] == pytest.approx(want.mean(), rel=1e-12)
    assert np.array_equal(mat["estimate"], est) and m["shift_error_max"] == np.abs(est - mat["shifts"]).max()
    gain, loss = table["estimated"] - table["ignored"], table["true"] - table["estimated"]
    print(f"estimated - ignored {gain.round(2).tolist()} dB (>= 1), true - estimated {loss.round(2).tolist()} dB (<= 1); shift error "
          f"{m['shift_error_mean']:.3f} mean, {m['shift_error_max']:.3f} max HR pixels")
    assert (gain >= 1.0).all()
    assert (loss <= 1.0).all()


# ---- rams_master --tv_multiframe -----------------------------------------------------------------------------------------------------------
def test_rams_master_tv_multiframe_flag(tmp_path):
    """`--tv_multiframe` adds DWI_tvmf / ADC_tvmf and three keys to the record, equal to direct calls; without it the record has the
    keys it always had and the written files are those of the flagged run's RAMS path, byte for byte."""
    from oracle import rams_port as R
    from tests import register_common as G
    from mri_super_resolution_amd import matio, rams
    from mri_super_resolution_amd.scripts import rams_master
    dwi, b0 = G.rams_case()
    data_dir = tmp_path / "anon_data"
    data_dir.mkdir()
    matio.savemat(str(data_dir / "pat09_alldata.mat"), {"data": dwi})
    matio.savemat(str(data_dir / "pat09_mean_b0.mat"), {"data_mean_b0": b0})
    spec = [{"pt_id": "18-1681-09", "b": 900, "cancer_loc": [10, 12], "contralateral_loc": [10, 8], "noise": [3, 3],
             "cancer_slice": 1, "acquisitions": [3, 3, 4]}]
    with open(str(tmp_path / "cases.json"), "w") as fh:
        json.dump(spec, fh)
    model = rams.RAMS(3, 32, 3, 9, 8, 12, params=R.init_rams_params(seed=4, perturb_g=True))
    weights = model.save_weights(str(tmp_path / "w.npz"))

    def run(tag, *extra):
        argv = ["--out_folder", str(tmp_path / tag / "exp"), "--out_img_folder", str(tmp_path / tag / "img"), "--exp_name", "mi1",
                "--data_dir", str(data_dir), "--cases", str(tmp_path / "cases.json"), "--weights", weights, "--sample_size", "2",
                "--seed", "3", *extra]
        rec, = rams_master.main(argv)["cases"]
        with open(str(tmp_path / tag / "exp" / "mi1.json")) as fh:
            written, = json.load(fh)["cases"]
        return rec, written

    plain, plain_json = run("plain")
    flagged, flagged_json = run("flag", "--tv_multiframe", "--tv_iters", "100", "--ssim")
    parent_keys = ["patient", "shape", "sample_size", "seconds", "subsets", "out_dir"]
    new_keys = ["cssim_vs_rescaled", "tvmf_shifts", "tvmf_energy", "tvmf_valid_fraction", "cssim_tvmf_vs_rescaled"]
    assert list(plain) == parent_keys == list(plain_json)
    assert list(flagged) == parent_keys + new_keys == list(flagged_json)
    read = lambda rec, name: open(os.path.join(rec["out_dir"], name), "rb").read()
    assert sorted(os.listdir(plain["out_dir"])) == ["ADC_mean.npy", "DWI_mean.npy", "images.mat"]
    assert sorted(os.listdir(flagged["out_dir"])) == ["ADC_mean.npy", "ADC_tvmf.npy", "DWI_mean.npy", "DWI_tvmf.npy", "images.mat"]
    for name in ("DWI_mean.npy", "ADC_mean.npy"):
        assert read(plain, name) == read(flagged, name)
    assert set(matio.loadmat(os.path.join(plain["out_dir"], "images.mat"))) >= {"DWI_mean", "ADC_mean"}
    assert not {"DWI_tvmf", "ADC_tvmf"} & set(matio.loadmat(os.path.join(plain["out_dir"], "images.mat")))
    # the new outputs are direct calls
    seq = dwi[:, :, 1, :].astype(np.float64)
    frames = np.ascontiguousarray(seq.transpose(2, 0, 1)) / seq.max()
    shifts = baselines.estimate_shifts(frames, (3, 3), 4, 8)
    x, info = baselines.tv_superres_multi(frames, (3, 3), shifts, "mean", n_iter=100, return_info=True)
    got = np.load(os.path.join(flagged["out_dir"], "DWI_tvmf.npy"))
    adc = -np.log(x * seq.max() / (baselines.rescale(b0[:, :, 1].astype(np.float64), 3, anti_aliasing=False) + 1e-7) + 1e-7) / 900 * 1e6
    planted = np.zeros((10, 2))
    for t, s in G.RAMS_PLANTED.items():
        planted[t] = s
    print(f"tvmf_shifts / 3 against the planted whole-pixel rolls: max |difference| {np.abs(shifts / 3 - planted).max():.3f} LR pixels; "
          f"energy {flagged['tvmf_energy']:.6f}, valid fraction {flagged['tvmf_valid_fraction']:.3f}, cssim_tvmf_vs_rescaled "
          f"{flagged['cssim_tvmf_vs_rescaled']:.4f}")
    assert got.shape == (60, 60) and np.array_equal(got, x * seq.max())
    assert np.array_equal(np.load(os.path.join(flagged["out_dir"], "ADC_tvmf.npy")), adc)
    assert flagged["tvmf_shifts"] == flagged_json["tvmf_shifts"] == shifts.tolist()
    assert flagged["tvmf_energy"] == float(info["energy"]) and flagged["tvmf_valid_fraction"] == float(info["valid_fraction"])
    assert np.abs(shifts / 3 - planted).max() <= 0.25                       # one step of the estimate, 3 / 4 HR pixel
    mat = matio.loadmat(os.path.join(flagged["out_dir"], "images.mat"))
    assert np.array_equal(mat["DWI_tvmf"], got) and np.array_equal(mat["ADC_tvmf"], adc)
    assert np.isfinite(flagged["cssim_tvmf_vs_rescaled"])
