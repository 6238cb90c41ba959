"""GPU: the 3-D TV / Huber solver of csrc/tvsr3d.hip against its float64 restatement (tests/tvsr3d_common.py), against the 2-D solver
of csrc/tvsr.hip bit for bit where the two must agree, against properties that do not depend on the restatement, across a batch,
streams and grids, and through the through-plane study (``scripts/through_plane``).

Bounds are derived, not measured.  A / A^T in fp64 carry the project's 1e-12 of max(max|in|, max|want|).  The solver carries 1e-10
absolute on data in [0, 1] for up to 1,000 iterations, derived as tests/test_gpu_tvsr.py derives it: the iteration is non-expansive,
about a dozen roundings of 1.1e-16 per voxel and iteration give 1e-12 over 1,000 iterations, and the bound leaves two orders of
margin; ``change`` is the difference of two volumes that are each within the bound: 2e-10.  Against the 2-D solver the comparison is
of bits: with one slice, or with g0 = 0, every slice term of the 3-D iteration is an exact zero (the order contract).
``energy`` is a sum of non-negative terms of a few roundings each, added in another order than the 2-D kernel's: 1e-12 relative.
Every test prints what it measured before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

from tests import tvsr3d_common as T
from tests import tvsr_common as T2
from mri_super_resolution_amd import _lib, baselines, drivers, matio, metrics, ops, reports
from mri_super_resolution_amd.scripts import through_plane as tp_script

pytestmark = pytest.mark.gpu

SOLVER_BOUND = 1e-10
OPERATOR_SHAPES = (((4, 6, 10), (2, 3, 2)), ((1, 8, 8), (1, 1, 1)), ((8, 16, 24), (8, 8, 8)), ((3, 5, 7), (3, 5, 7)))


def _random_factors(f, rng):
    ks = [rng.random(v) + 0.1 for v in f]
    return tuple(k / k.sum() for k in ks)


def _kernels(f, rng):
    return {"mean": "mean", "decimate": "decimate", "random": _random_factors(f, rng)}


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _ids(shapes):
    return ["x".join(map(str, s)) + "by" + "x".join(map(str, f)) for s, f in shapes]


@pytest.mark.parametrize("shape,f", OPERATOR_SHAPES, ids=_ids(OPERATOR_SHAPES))
def test_block_operator_and_adjoint_match_the_restatement_and_each_other(shape, f):
    rng = np.random.default_rng(int(np.prod(shape)))
    lr_shape = tuple(s // v for s, v in zip(shape, f))
    x, r = rng.standard_normal((3,) + shape), rng.standard_normal((3,) + lr_shape)
    for name, kernel in _kernels(f, rng).items():
        k = T.block_table(T.block_factors(kernel, f))
        got_a, got_t = baselines.block_apply3d(x, f, kernel), baselines.block_adjoint3d(r, f, kernel)
        want_a, want_t = T.apply_A(x, k), T.apply_AT(r, k)
        err_a, tol_a = np.abs(got_a - want_a).max(), 1e-12 * max(np.abs(x).max(), np.abs(want_a).max())
        err_t, tol_t = np.abs(got_t - want_t).max(), 1e-12 * max(np.abs(r).max(), np.abs(want_t).max())
        dot_a, dot_t = float((got_a * r).sum()), float((x * got_t).sum())
        scale = float(np.abs(got_a * r).sum())
        print(f"{shape} {f} {name}: |A - want| {err_a:.2e} (bound {tol_a:.2e}), |A^T - want| {err_t:.2e} (bound {tol_t:.2e}), "
              f"|<Ax, r> - <x, A^T r>| / sum|.| {abs(dot_a - dot_t) / scale:.2e}")
        assert got_a.dtype == got_t.dtype == np.float64 and got_a.shape == want_a.shape and got_t.shape == want_t.shape
        assert err_a <= tol_a and err_t <= tol_t
        assert abs(dot_a - dot_t) <= 1e-12 * scale
        # device tensors come back as what they were; fp32 is the fp64 result rounded once
        x32 = _dev(x, torch.float32)
        got32 = baselines.block_apply3d(x32, f, kernel)
        assert got32.dtype == torch.float32 and torch.equal(got32, baselines.block_apply3d(x32.double(), f, kernel).float())
        r32 = _dev(r, torch.float32)
        assert torch.equal(baselines.block_adjoint3d(r32, f, kernel), baselines.block_adjoint3d(r32.double(), f, kernel).float())
        assert baselines.block_adjoint3d(_dev(r), f, kernel).dtype == torch.float64


def _compare(name, y, f, kernel, lam, alpha, n_iter, g=(1.0, 1.0, 1.0), w=None, x0=None):
    got, info = baselines.tv_superres3d(y, f, kernel, lam, alpha, n_iter, g, weight=w, x0=x0, return_info=True)
    want, energy, change = T.solve(y, f, kernel, lam, alpha, n_iter, g, w=w, x0=x0, return_info=True)
    err = float(np.abs(got - want).max())
    e_rel = float(np.abs(info["energy"] - energy).max() / np.abs(energy).max())
    c_err = float(np.abs(info["change"] - change).max())
    print(f"{name}, g {g}, {n_iter} iterations: max|got - restated| = {err:.3e} (bound {SOLVER_BOUND:.0e}), "
          f"energy against the restated run's (not asserted here) {e_rel:.2e}, "
          f"|change - restated| {c_err:.2e} (change {float(change.max()):.2e})")
    assert got.dtype == np.float64 and got.shape == want.shape
    assert err <= SOLVER_BOUND
    assert c_err <= 2 * SOLVER_BOUND
    return got, info


@pytest.mark.parametrize("g", T.CASE_GRAD_WEIGHTS, ids=("g111", "g0.4"))
@pytest.mark.parametrize("n_iter", (1, 2, 300))
def test_solver_matches_the_restatement_on_the_weighted_huber_case(n_iter, g):
    _, y, w = T.case_data()
    _compare("4x6x6 (2, 3, 2) weighted Huber", y, T.CASE_FACTORS, T.CASE_KERNEL, T.CASE_LAM, T.CASE_ALPHA, n_iter, g, w=w)


RAGGED = (((5, 7, 1024), (5, 7, 1)), ((7, 1024, 5), (7, 1, 5)), ((1024, 5, 7), (1, 5, 7)))


@pytest.mark.parametrize("shape,f", RAGGED, ids=_ids(RAGGED))
def test_solver_matches_the_restatement_on_ragged_extents(shape, f):
    """No extent is a multiple of the workgroup tile (64 HR columns, 2,048 voxels, 256 threads); one axis is a single block, one has a
    single voxel per block; random kernels, weights with zeros, a given x0, alpha = 0, and gradient weights (0.4, 1, 1)."""
    rng = np.random.default_rng(shape[0])
    hr = rng.random((2,) + shape)
    for name, kernel in _kernels(f, rng).items():
        y = T.apply_A(hr, T.block_table(T.block_factors(kernel, f)))
        w = rng.random(y.shape) * (rng.random(y.shape) > 0.1)
        _compare(f"{shape} {f} {name}", y, f, kernel, 0.02, 0.05, 20, (0.4, 1.0, 1.0), w=w, x0=rng.random(hr.shape))
    _compare(f"{shape} {f} mean, plain TV", T.apply_A(hr, T.block_table(T.block_factors("mean", f))), f, "mean", 0.02, 0.0, 20)


@pytest.mark.parametrize("n_iter", (0, 3))
def test_more_partials_than_the_finish_has_threads(n_iter):
    """257 x 1 x 1 with unit factors is 257 tiles: thread 0 of the finish kernel adds (maximises) two partials.  The energy against
    the restated objective at the returned volume, within the 1e-12 relative of the other energy checks of this file; without an
    iteration the change partials are never written and the change is 0."""
    y = np.random.default_rng(257).random((2, 257, 1, 1))
    k = (np.ones(1), np.ones(1), np.ones(1))
    got, info = _compare("257x1x1 (1, 1, 1), 257 tiles", y, (1, 1, 1), k, 0.05, 0.02, n_iter)
    at = T.energy(got, y, T.block_table(k), 0.05, 0.02)
    e_rel = float((np.abs(info["energy"] - at) / np.abs(at)).max())
    print(f"energy {info['energy'].tolist()} against the restated objective at the returned volume: {e_rel:.2e} relative")
    assert e_rel <= 1e-12
    assert n_iter > 0 or not info["change"].any()


@pytest.fixture(scope="module")
def pat07():
    return T.pat07_roi()                    # [28, 50, 50] in [0, 1]


def _same_as_2d(name, y2, f2, k12, lam, alpha, n_iter, w2=None, g0=1.0):
    """y2 [n, h, w] as n one-slice volumes through the 3-D solver (k0 = [1]) against the 2-D solver with k1[:, None] * k2[None, :]."""
    k1, k2 = k12
    as3 = lambda a: None if a is None else a[:, None]
    got, info = baselines.tv_superres3d(as3(y2), (1,) + tuple(f2), (np.ones(1), k1, k2), lam, alpha, n_iter, (g0, 1.0, 1.0),
                                        weight=as3(w2), return_info=True)
    want, winfo = baselines.tv_superres(y2, f2, k1[:, None] * k2[None, :], lam, alpha, n_iter, weight=w2, return_info=True)
    e_rel = float(np.abs(info["energy"] - winfo["energy"]).max() / np.abs(winfo["energy"]).max())
    print(f"{name}: x equal {np.array_equal(got[:, 0], want)} (max|diff| {np.abs(got[:, 0] - want).max():.2e}), change equal "
          f"{np.array_equal(info['change'], winfo['change'])}, energy relative {e_rel:.2e}")
    assert np.array_equal(got[:, 0], want)
    assert np.array_equal(info["change"], winfo["change"])
    assert e_rel <= 1e-12


def test_a_one_slice_volume_is_the_2d_solver_bit_for_bit(pat07):
    _, y = T2.case_data()
    mean = lambda f: np.full(f, 1.0 / f)
    _same_as_2d("6x10 weighted Huber", y, T2.CASE_FACTORS, (mean(3), mean(2)), T2.CASE_LAM, T2.CASE_ALPHA, 300, T2.CASE_W, g0=0.7)
    slice14 = pat07[14:15]
    for name, k in (("mean", mean(2)), ("decimate", np.array([1.0, 0.0]))):
        y = T2.apply_A(slice14, k[:, None] * k[None, :])
        _same_as_2d(f"pat07 slice 14 {name}", y, (2, 2), (k, k), 3e-3, 0.3, 300)


def test_uncoupled_slices_are_the_batched_2d_solve_bit_for_bit(pat07):
    """g0 = 0 on pat07 [28, 50, 50], factors (1, 2, 2): the volume is spread over several workgroups, every tile reads its
    neighbours' p and x, and the launches depend on each other through the stream alone -- a misplaced halo, tile edge or ordering
    changes bits."""
    y = T2.apply_A(pat07, T2.block_kernel("mean", (2, 2)))                         # [28, 25, 25]
    args = (3e-3, 0.3, 200)
    got, info = baselines.tv_superres3d(y, (1, 2, 2), "mean", *args, (0.0, 1.0, 1.0), return_info=True)
    want, winfo = baselines.tv_superres(y, (2, 2), "mean", *args, return_info=True)
    coupled = baselines.tv_superres3d(y, (1, 2, 2), "mean", *args, (1.0, 1.0, 1.0))
    print(f"pat07 28x50x50 g0 = 0: equal to the 28 2-D solves {np.array_equal(got, want)} (max|diff| {np.abs(got - want).max():.2e}), "
          f"change {float(info['change']):.3e} against max of the slices' {float(winfo['change'].max()):.3e}; g0 = 1 differs by "
          f"{np.abs(coupled - want).max():.2e}")
    assert got.shape == (28, 50, 50) and np.array_equal(got, want)
    assert float(info["change"]) == float(winfo["change"].max())
    assert abs(float(info["energy"]) - float(winfo["energy"].sum())) <= 1e-12 * float(winfo["energy"].sum())
    assert np.abs(coupled - want).max() > 1e-4             # the coupling is not a no-op


def test_properties_that_do_not_depend_on_the_restatement():
    rng = np.random.default_rng(5)
    hr, y, w = T.case_data()
    f, ks = T.CASE_FACTORS, T.CASE_KERNEL
    # lambda = 0: the replication start satisfies the data and stays, exactly (kernels whose replication is exact: mean, decimate)
    for kernel in ("mean", "decimate"):
        yk = baselines.block_apply3d(hr, f, kernel)
        for n_iter in (1, 50):
            x, info = baselines.tv_superres3d(yk, f, kernel, 0.0, 0.0, n_iter, return_info=True)
            res = float(np.abs(baselines.block_apply3d(x, f, kernel) - yk).max())
            print(f"lambda = 0, {kernel}, {n_iter} iterations: x == x0 {np.array_equal(x, T.replicate(yk, f))}, max|A x - y| = {res:.2e}, "
                  f"energy {float(info['energy'][0]):.2e}, change {float(info['change'][0]):.2e}")
            assert np.array_equal(x, T.replicate(yk, f))
            assert res <= 1e-15
    # zero gradient weights switch the prior off: the same
    x = baselines.tv_superres3d(y, f, "mean", 0.05, 0.02, 5, (0.0, 0.0, 0.0))
    assert np.array_equal(x, baselines.tv_superres3d(y, f, "mean", 0.0, 0.02, 5))
    # n_iter = 0 returns x0: the given one, or the block replication
    x0 = rng.random(hr.shape)
    x, info = baselines.tv_superres3d(y, f, ks, 0.05, 0.02, 0, x0=x0, return_info=True)
    assert np.array_equal(x, x0) and float(info["change"][0]) == 0.0
    assert np.array_equal(baselines.tv_superres3d(y, f, ks, 0.05, 0.02, 0), T.replicate(y, f))
    # a missing datum (w = 0) is never read: whatever y holds there, the same bits come out
    other = y.copy()
    other[w == 0] = 1e3
    a, ia = baselines.tv_superres3d(y, f, ks, T.CASE_LAM, T.CASE_ALPHA, 30, weight=w, return_info=True)
    b, ib = baselines.tv_superres3d(other, f, ks, T.CASE_LAM, T.CASE_ALPHA, 30, weight=w, x0=T.replicate(y, f), return_info=True)
    assert (w == 0).sum() == 1 and np.array_equal(a, b) and np.array_equal(ia["energy"], ib["energy"])
    # energy is the restated objective at the returned volume
    k = T.block_table(ks)
    for alpha, g in ((0.0, (1.0, 1.0, 1.0)), (T.CASE_ALPHA, (0.4, 1.0, 1.0))):
        x, info = baselines.tv_superres3d(y, f, ks, T.CASE_LAM, alpha, 30, g, weight=w, return_info=True)
        want = T.energy(x, y, k, T.CASE_LAM, alpha, w, g)
        rel = float(np.abs(info["energy"] - want).max() / np.abs(want).max())
        print(f"alpha {alpha}, g {g}: energy {float(info['energy'][0]):.12f}, restated at the returned volume {float(want[0]):.12f}, "
              f"relative {rel:.2e}")
        assert rel <= 1e-12


@pytest.mark.parametrize("g", T.CASE_GRAD_WEIGHTS, ids=("g111", "g0.4"))
def test_energy_reaches_the_lbfgs_minimum_which_shares_nothing_with_the_iteration(g):
    hr, y, w = T.case_data()
    minimum = T.lbfgs_minimum(y, T.block_table(T.CASE_KERNEL), T.CASE_LAM, T.CASE_ALPHA, w, hr.shape, g)
    _, info = baselines.tv_superres3d(y, T.CASE_FACTORS, T.CASE_KERNEL, T.CASE_LAM, T.CASE_ALPHA, 1000, g, weight=w, return_info=True)
    gap = (float(info["energy"][0]) - minimum) / minimum
    print(f"g {g}: L-BFGS-B minimum {minimum:.12f}, energy after 1,000 iterations {float(info['energy'][0]):.12f}, relative gap {gap:.2e}")
    assert abs(gap) <= 1e-9


def test_a_batch_a_second_call_and_a_side_stream_give_equal_bits():
    """40 different 4 x 6 x 6 volumes against their solitary solves; the same call again; the same call on another stream."""
    rng = np.random.default_rng(11)
    n, f = 40, T.CASE_FACTORS
    y = _dev(rng.random((n, 2, 2, 3)))
    w = _dev(rng.random((n, 2, 2, 3)) * (rng.random((n, 2, 2, 3)) > 0.1))
    args = (f, T.CASE_KERNEL, 0.02, 0.05, 25, (0.4, 1.0, 1.0))
    out, info = baselines.tv_superres3d(y, *args, weight=w, return_info=True)
    torch.cuda.synchronize()
    differ = 0
    for i in range(n):
        one, one_info = baselines.tv_superres3d(y[i:i + 1], *args, weight=w[i:i + 1], return_info=True)
        differ += int(not (torch.equal(one[0], out[i]) and torch.equal(one_info["energy"][0], info["energy"][i])
                           and torch.equal(one_info["change"][0], info["change"][i])))
    again, again_info = baselines.tv_superres3d(y, *args, weight=w, return_info=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side, side_info = baselines.tv_superres3d(y, *args, weight=w, return_info=True)
    side.synchronize()
    distinct = len({out[i].cpu().numpy().tobytes() for i in range(n)})
    print(f"{n} volumes of 4x6x6: {differ} differ from their solitary solve; second run equal {torch.equal(again, out)}; side stream "
          f"equal {torch.equal(on_side, out)}; {distinct} distinct results")
    assert out.shape == (n, 4, 6, 6) and distinct == n
    assert differ == 0
    assert torch.equal(again, out) and torch.equal(again_info["energy"], info["energy"]) and torch.equal(again_info["change"], info["change"])
    assert torch.equal(on_side, out) and torch.equal(side_info["energy"], info["energy"]) and torch.equal(side_info["change"], info["change"])


def test_a_capped_grid_walks_its_stride_to_the_same_bits():
    """The test-only grid cap (inr_debug_set(32, 3); tests/conftest.py resets it): three workgroups walk the 8 x 32 x 32 volume's tiles
    and voxels in their stride loops and give the bits of the uncapped run, energy and change included."""
    rng = np.random.default_rng(13)
    y = _dev(rng.random((2, 4, 16, 16)))
    args = ((2, 2, 2), "mean", 0.02, 0.05, 30, (0.4, 1.0, 1.0))
    free, free_info = baselines.tv_superres3d(y, *args, return_info=True)
    assert _lib.lib().inr_debug_set(32, 3) == 0
    try:
        capped, capped_info = baselines.tv_superres3d(y, *args, return_info=True)
        apply_capped = baselines.block_apply3d(capped, (2, 2, 2))
    finally:
        assert _lib.lib().inr_debug_set(32, 0) == 0
    print(f"grid cap 3 on 2 x 8x32x32: x equal {torch.equal(capped, free)}, energy equal {torch.equal(capped_info['energy'], free_info['energy'])}, "
          f"change equal {torch.equal(capped_info['change'], free_info['change'])}")
    assert free.shape == (2, 8, 32, 32)
    assert torch.equal(capped, free) and torch.equal(capped_info["energy"], free_info["energy"])
    assert torch.equal(capped_info["change"], free_info["change"])
    assert torch.equal(apply_capped, baselines.block_apply3d(free, (2, 2, 2)))


def test_fp32_is_the_fp64_result_rounded_once_and_types_come_back_as_given():
    rng = np.random.default_rng(9)
    hr, y, w = T.case_data()
    y32, w32, x32 = _dev(y, torch.float32), _dev(w, torch.float32), _dev(rng.random(hr.shape), torch.float32)
    args = (T.CASE_FACTORS, T.CASE_KERNEL, T.CASE_LAM, T.CASE_ALPHA, 100, (0.4, 1.0, 1.0))
    got, info = baselines.tv_superres3d(y32, *args, weight=w32, x0=x32, return_info=True)
    want, winfo = baselines.tv_superres3d(y32.double(), *args, weight=w32.double(), x0=x32.double(), return_info=True)
    same = torch.equal(got, want.float())
    print(f"fp32 out == fp64 out rounded once: {same}; max|fp32 - fp64| = {float((got.double() - want).abs().max()):.2e}")
    assert got.dtype == torch.float32 and want.dtype == torch.float64 and got.is_cuda and info["energy"].dtype == torch.float64
    assert same
    assert torch.equal(info["energy"], winfo["energy"]) and torch.equal(info["change"], winfo["change"])
    # leading axes are a batch and keep their shape
    stack = _dev(rng.random((2, 3, 2, 4, 6)), torch.float32)
    out, info = baselines.tv_superres3d(stack, (2, 2, 1), n_iter=5, return_info=True)
    assert out.shape == (2, 3, 4, 8, 6) and out.dtype == torch.float32 and info["energy"].shape == info["change"].shape == (2, 3)
    assert isinstance(baselines.tv_superres3d(rng.random((2, 4, 6)), (2, 2, 2), n_iter=3), np.ndarray)
    assert baselines.block_apply3d(stack, (1, 2, 3)).shape == (2, 3, 2, 2, 2)


def test_ops_wrappers_check_before_they_launch():
    y = torch.rand(2, 2, 3, 5, device="cuda", dtype=torch.float64)
    k = ([0.5, 0.5], [0.5, 0.5], [1.0])
    f = (2, 2, 1)
    out, energy, change = ops.tvsr_solve3d(y, f, k, 0.01, 0.0, 3)
    assert out.shape == (2, 4, 6, 5) and energy.shape == change.shape == (2,)
    assert torch.equal(ops.block_apply3d(ops.block_adjoint3d(y, f, k), f, k), 0.25 * y)
    need = ops.tvsr3d_workspace_doubles(2, 4, 6, 5, f)
    assert need >= 2 * 5 * 120
    with pytest.raises(ValueError, match="contiguous"):
        ops.tvsr_solve3d(y[:, :, :, ::2], f, k, 0.01, 0.0, 3)
    with pytest.raises(TypeError, match="float32 or torch.float64|float64"):
        ops.tvsr_solve3d(y.half(), f, k, 0.01, 0.0, 3)
    with pytest.raises(ValueError, match="weight has shape"):
        ops.tvsr_solve3d(y, f, k, 0.01, 0.0, 3, weight=y[:1].contiguous())
    with pytest.raises(ValueError, match="sum to 1"):
        ops.tvsr_solve3d(y, f, ([1.0, 1.0], [0.5, 0.5], [1.0]), 0.01, 0.0, 3)
    with pytest.raises(ValueError, match=f"workspace must be a device float64 tensor of at least {need}"):
        ops.tvsr_solve3d(y, f, k, 0.01, 0.0, 3, workspace=torch.empty(need - 1, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="n_iter must be an integer 0 .. 100000"):
        ops.tvsr_solve3d(y, f, k, 0.01, 0.0, -1)
    with pytest.raises(ValueError, match="grad_weights"):
        ops.tvsr_solve3d(y, f, k, 0.01, 0.0, 3, grad_weights=(1.0, -1.0, 1.0))
    with pytest.raises(ValueError, match="contiguous"):
        ops.block_apply3d(out[:, :, :, ::5], f, k)


# ---- the through-plane study ---------------------------------------------------------------------------------------------------------
def _synthetic_volume():
    rng = np.random.default_rng(3)
    gx, gy, gz = np.meshgrid(np.linspace(0, 1, 32), np.linspace(0, 1, 32), np.linspace(0, 1, 8), indexing="ij")
    vol = np.stack([500 * (1.2 + np.sin(3 * gx + 2 * gz) * np.cos(2 * gy + gz)) * np.exp(-0.7 * b) for b in range(2)], axis=-1)
    return vol * (1 + 0.02 * rng.standard_normal(vol.shape)), np.array([0.0, 1000.0])


@pytest.fixture(scope="module")
def study_inputs(tmp_path_factory, golden):
    tmp = tmp_path_factory.mktemp("tp")
    vol, bvals = _synthetic_volume()
    synthetic = str(tmp / "pat068_vol.mat")
    matio.savemat(synthetic, {"vol": vol, "b": bvals})
    pat07 = str(tmp / "pat07_mean_b0.mat")
    matio.savemat(pat07, {"data_mean_b0": golden("pat07_volume.npz")["vol"]})
    return tmp, {"synthetic": (synthetic, ["--roi_start", "2", "--roi_end", "30"], 8, 2),
                 "pat07": (pat07, ["--roi_start", "40", "--roi_end", "90"], 28, 1)}


def _direct(path, roi, factor, profile, fwhm, lam, huber, iters, gz):
    """The four methods called directly on the study's data -> ({method: [Z, B, R, R]}, HR stack, thick stack, kernel)."""
    mean_img = tp_script.load_input_and_scale(path)[0]
    r0, r1 = roi
    hr = torch.from_numpy(np.ascontiguousarray(mean_img[r0:r1, r0:r1], dtype=np.float32)).cuda().permute(3, 2, 0, 1).contiguous()
    kernel = (baselines.slice_profile(factor, profile, fwhm if profile == "gaussian" else None), np.ones(1), np.ones(1))
    thick = baselines.block_apply3d(hr, (factor, 1, 1), kernel)
    Z = hr.shape[1]
    vols = {"replicate": thick.repeat_interleave(factor, dim=1),
            "spline": baselines.resize_z(thick.permute(0, 2, 3, 1).contiguous(), Z).permute(0, 3, 1, 2).float().contiguous(),
            "zerofill": baselines.fourier_resample(thick, Z, axis=1, align="center", boundary="mirror").clamp_min(0),
            "tv3d": baselines.tv_superres3d(thick, (factor, 1, 1), kernel, lam, huber, iters, (gz, 1.0, 1.0))}
    stack = lambda t: t.permute(1, 0, 2, 3).contiguous()
    return {k: stack(v) for k, v in vols.items()}, stack(hr), thick, kernel


STUDY_CASES = (("synthetic", 2, "mean"), ("synthetic", 2, "gaussian"), ("pat07", 2, "mean"), ("pat07", 2, "gaussian"),
               ("pat07", 4, "gaussian"))         # (at factor 2 the two sub-slices sit symmetrically: a Gaussian profile IS the mean)


@pytest.mark.parametrize("case,factor,profile", STUDY_CASES, ids=[f"{c}-{f}-{p}" for c, f, p in STUDY_CASES])
def test_through_plane_study_scores_what_a_direct_call_gives(study_inputs, case, factor, profile):
    tmp, inputs = study_inputs
    path, roi, nz, nb = inputs[case]
    out = str(tmp / f"{case}_{factor}_{profile}")
    res = tp_script.main(["--data", path, "--output_address", out, *roi, "--factor", str(factor), "--profile", profile, "--fwhm", "0.6",
                          "--tv_iters", "100"])[0]
    d = os.path.join(out, "pat068" if case == "synthetic" else "pat07")
    header = open(os.path.join(d, "through_plane.csv")).readline()
    rows = reports.read_csv(os.path.join(d, "through_plane.csv"))
    m = json.load(open(os.path.join(d, "metrics.json")))
    vols, hs, thick, kernel = _direct(path, (int(roi[1]), int(roi[3])), factor, profile, 0.6, baselines.TV3D_DEFAULT_LAMBDA,
                                      baselines.TV3D_DEFAULT_HUBER, 100, 1.0)
    assert header == "Pt_id, b-value, slice, SSIM-replicate, SSIM-spline, SSIM-zerofill, SSIM-tv3d\n"
    assert len(rows) == nz * nb and [int(r["slice"]) for r in rows] == [z for z in range(nz) for _ in range(nb)]
    floor = lambda t: t.clamp_min(1e-30)
    for method, vol in vols.items():
        want = float(metrics.psnr(hs, vol, 1.0))
        col = np.array([float(r[f"SSIM-{method}"]) for r in rows]).reshape(nz, nb)
        want_ssim = metrics.ssim_reference_protocol(floor(hs), floor(vol)).cpu().numpy().astype(np.float64)
        print(f"{case} factor {factor} {profile}: psnr_{method}_db {m[f'psnr_{method}_db']:.3f} (direct {want:.3f}), ssim_{method}_mean "
              f"{m[f'ssim_{method}_mean']:.4f}")
        assert m[f"psnr_{method}_db"] == want == res[f"psnr_{method}_db"]
        assert np.array_equal(col, np.array([[float(v) for v in row] for row in want_ssim]))
        assert m[f"ssim_{method}_mean"] == pytest.approx(col.mean())
    consistency = float(metrics.psnr(thick, baselines.block_apply3d(vols["tv3d"].permute(1, 0, 2, 3).contiguous(), (factor, 1, 1), kernel), 1.0))
    print(f"    tv3d_consistency_psnr_db {m['tv3d_consistency_psnr_db']:.2f} (direct {consistency:.2f})")
    assert np.isfinite(m["tv3d_consistency_psnr_db"]) and m["tv3d_consistency_psnr_db"] == consistency
    assert (m["slice_profile"] == [0.5, 0.5]) == (factor == 2) and abs(sum(m["slice_profile"]) - 1.0) <= 1e-15
    mat = matio.loadmat(os.path.join(d, "through_plane.mat"))
    assert set(mat) >= {"hr", "thick", "replicate", "spline", "zerofill", "tv3d"}
    assert mat["tv3d"].shape == mat["hr"].shape == (int(roi[3]) - int(roi[1]),) * 2 + (nz, nb) and mat["thick"].shape[2] == nz // factor
    assert not [k for k in m if k.endswith("_sr_db")] and "sr" not in mat


def test_through_plane_study_with_inr_adds_its_column_and_leaves_the_rest(study_inputs):
    tmp, inputs = study_inputs
    path, roi, nz, nb = inputs["synthetic"]
    common = ["--data", path, *roi, "--factor", "2", "--profile", "mean", "--tv_iters", "100"]
    plain = tp_script.main(common + ["--output_address", str(tmp / "inr_off")])[0]
    for footprint in ("point", "box"):
        out = str(tmp / f"inr_{footprint}")
        res = tp_script.main(common + ["--output_address", out, "--with_inr", "--footprint", footprint, "--number_of_epochs", "5",
                                       "--seed", "0"])[0]
        d, d0 = os.path.join(out, "pat068"), os.path.join(str(tmp / "inr_off"), "pat068")
        assert open(os.path.join(d, "through_plane.csv")).readline() == \
            "Pt_id, b-value, slice, SSIM-replicate, SSIM-spline, SSIM-zerofill, SSIM-tv3d, SSIM-SR\n"
        rows, rows0 = reports.read_csv(os.path.join(d, "through_plane.csv")), reports.read_csv(os.path.join(d0, "through_plane.csv"))
        assert len(rows) == len(rows0) == nz * nb
        for r, r0 in zip(rows, rows0):
            assert {k: v for k, v in r.items() if k != "SSIM-SR"} == r0 and np.isfinite(float(r["SSIM-SR"]))
        m, m0 = json.load(open(os.path.join(d, "metrics.json"))), json.load(open(os.path.join(d0, "metrics.json")))
        new = set(m) - set(m0)
        print(f"--with_inr --footprint {footprint}: psnr_sr_db {m['psnr_sr_db']:.2f}, ssim_sr_mean {m['ssim_sr_mean']:.4f}, new keys {sorted(new)}")
        assert {"psnr_sr_db", "ssim_sr_mean"} <= new and all("sr" in k or "inr" in k for k in new)
        strip = lambda s: json.dumps({k: v for k, v in s.items() if k in m0 and k != "output"}, indent=1).encode()
        assert strip(m) == strip(m0) and np.isfinite(res["psnr_sr_db"])
        mat = matio.loadmat(os.path.join(d, "through_plane.mat"))
        assert mat["sr"].shape == mat["hr"].shape
    assert "psnr_sr_db" not in plain
