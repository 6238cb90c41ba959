"""The float64 NumPy restatement of the multi-stack reconstruction (tests/tvms_common.py) pinned on its own, without a device:
adjointness, the step bound, the minimum against L-BFGS-B, the reductions to the sibling restatements and the orderings of the study."""
import functools

import numpy as np
import pytest

from tests import tvmf_common as MF
from tests import tvms_common as M
from tests import tvsr3d_common as T3


def all_cases():
    """(hr shape, stack) of every operator case of the issue."""
    out = [(M.CASE_SHAPE, st) for st in M.case_stacks()]
    out.append(M.limit_stack())
    out.append(M.odd_stack())
    return out


@pytest.mark.parametrize("case", range(5))
def test_adjointness(case):
    shape, st = all_cases()[case]
    rng = np.random.default_rng(case)
    x, r = rng.standard_normal(shape), rng.standard_normal(st[3])
    lhs, rhs = (M.apply(x, st) * r).sum(), (x * M.adjoint(r, st, shape)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    valid = M.valid_mask(st, shape)
    assert valid.any() and (M.apply(x, st)[~valid] == 0).all()


def test_validity_of_the_cases():
    """The cases run off the volume where the issue says they do."""
    a, b, c = (M.valid_mask(st, M.CASE_SHAPE) for st in M.case_stacks())
    assert not a[0].any() and not a[3].any() and a[1:3].all()   # the overlapping stack: slice 0 starts at -1, slice 3 ends at 9 > 7
    assert b.all()                                               # the gapped stack lies inside
    assert not c[:, :, 0].any() and not c[:, :, 5].any() and c[:, :, 1:5].all()
    shape, st = M.odd_stack()
    assert M.axis_valid(st, shape)[1].tolist() == [False] * 3 + [True] * 5 + [False] * 2


@pytest.mark.parametrize("case", range(5))
def test_step_bound(case):
    shape, st = all_cases()[case]
    assert M.stack_bound(st) >= M.power_norm_sq(st, shape) * (1.0 - 1e-12)


def test_step_bound_of_a_block_stack_is_the_multi_frame_one():
    """L <= f: c_s = (sum |k|) (max |k|) of the formed table."""
    st = M.block_stack(T3.CASE_FACTORS, T3.CASE_KERNEL, (4, 6, 6))
    k = M.table(st[1])
    assert abs(M.stack_bound(st) - np.abs(k).sum() * np.abs(k).max()) <= 1e-15


@functools.lru_cache(maxsize=None)
def _case_minimum():
    _, ys, ws = M.case_data()
    return M.lbfgs_minimum(ys, M.case_stacks(), M.CASE_LAM, M.CASE_ALPHA, ws, M.CASE_SHAPE)


@pytest.mark.parametrize("n_iter,tol", [(300, 1e-8), (1000, 1e-9)])
def test_energy_reaches_the_lbfgs_minimum(n_iter, tol):
    _, ys, ws = M.case_data()
    _, e, _, _ = M.solve(ys, M.case_stacks(), M.CASE_SHAPE, M.CASE_LAM, M.CASE_ALPHA, n_iter, w=ws, return_info=True)
    print(f"energy {e!r} after {n_iter} iterations, L-BFGS-B {_case_minimum()!r}")
    assert abs(e - _case_minimum()) <= tol


def test_one_block_stack_is_the_3d_block_operator():
    hr, _, _ = T3.case_data()
    st = M.block_stack(T3.CASE_FACTORS, T3.CASE_KERNEL, hr.shape[1:])
    k = T3.block_table(T3.CASE_KERNEL)
    np.testing.assert_allclose(M.apply(hr[0], st), T3.apply_A(hr, k)[0], rtol=0, atol=1e-15)
    r = np.random.default_rng(1).random(st[3])
    np.testing.assert_array_equal(M.adjoint(r, st, hr.shape[1:]), T3.apply_AT(r, k))


def test_one_slice_with_whole_pixel_offsets_is_the_multi_frame_solve():
    hr = np.random.default_rng(3).random((12, 10))
    shifts = np.array([[0.0, 0.0], [1.0, -1.0], [-2.0, 1.0]])
    f = (3, 2)
    k = MF.block_kernel("mean", f)
    frames = MF.apply_frames(hr, k, shifts) + 0.01 * np.random.default_rng(4).standard_normal((3, 4, 5))
    x0 = MF.replicate(frames[0], f)
    want, e, ch, vf = MF.solve(frames, f, shifts, "mean", 0.05, 0.02, 60, x0=x0, return_info=True)
    stacks = [M.stack((1,) + f, (M.ONE, np.full(3, 1 / 3), np.full(2, 1 / 2)), (0, int(s[0]), int(s[1])), (1, 4, 5)) for s in shifts]
    got, e2, ch2, vf2 = M.solve([fr[None] for fr in frames], stacks, (1, 12, 10), 0.05, 0.02, 60, x0=x0[None], return_info=True)
    assert np.abs(got[0] - want).max() <= 1e-12
    assert abs(e - e2) <= 1e-12 * abs(e) and abs(ch - ch2) <= 1e-12 and vf == vf2


def test_study_shifted_beats_the_single_stack():
    ref = M.study_reference("shifted")
    print({name: round(v[1], 3) for name, v in ref.items()})
    assert ref["joint"][1] >= ref["stack0"][1] + 1.0


def test_study_orthogonal_beats_the_best_stack_and_the_mean():
    ref = M.study_reference("orthogonal")
    print({name: round(v[1], 3) for name, v in ref.items()})
    best = max(ref[f"stack{s}"][1] for s in range(3))
    assert ref["joint"][1] >= best + 1.0
    assert ref["joint"][1] >= ref["mean"][1] + 1.0
