"""No device: the refusals of inr_mppca_denoise (all before any device work), the cell <-> stack round trip of denoise.py, and the float64
restatement of the definition (tests/mppca_common.py) on the five cases the GPU tests share -- that it denoises, that its noise level is
the phantom's and that its rank decisions are not ties.

The phantom is three smooth spatial maps times exp(-k t), k = 0.5, 2, 6, plus Gaussian noise of sigma 0.05, the five cases drawn in
order from default_rng(0).  The restatement alone gives on them: RMSE ratio 0.305 .. 0.567, median sigma 0.0485 .. 0.0497, smallest
margin 7.05e-9 (case 1) .. 1.39e-6."""
import ctypes

import numpy as np
import pytest

from tests import mppca_common as P
from mri_super_resolution_amd import _lib, denoise, ops

RMSE_RATIO_BOUND = 0.7
SIGMA_RANGE = (0.9 * P.SIGMA, 1.05 * P.SIGMA)
MARGIN_BOUND = 1e-9


def _fake(k):
    return ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)       # never dereferenced: every call here fails in validation


GOOD = dict(out=1, sigma=2, rank=3, x=4, mask=5, M=16, D=4, H=12, W=12, w0=3, w1=5, w2=5, estimator=2)
REFUSALS = (
    ("null pointer", dict(out=None)),
    ("null pointer", dict(x=None)),
    ("at least 2 measurements", dict(M=1)),
    ("at least 2 measurements", dict(M=0)),
    ("negative size", dict(D=-1)),
    ("negative size", dict(W=-3)),
    ("window sides must be odd and >= 1 \\(side 1 is 4\\)", dict(w1=4)),
    ("window sides must be odd and >= 1 \\(side 0 is 0\\)", dict(w0=0)),
    ("window sides must be odd and >= 1 \\(side 2 is -1\\)", dict(w2=-1)),
    ("window side 0 \\(5\\) is larger than its axis \\(4\\)", dict(w0=5)),
    ("window side 2 \\(13\\) is larger than its axis \\(12\\)", dict(w2=13, w0=1, w1=1)),
    ("at least 2 voxels", dict(w0=1, w1=1, w2=1)),
    ("min\\(M, N\\) = min\\(70, 75\\) exceeds the rank limit 64: shrink the window or split the measurements", dict(M=70)),
    ("max\\(M, N\\) = max\\(16, 1089\\) exceeds 1024", dict(w0=1, w1=33, w2=33, H=40, W=40)),
    ("max\\(M, N\\) = max\\(1025, 25\\) exceeds 1024", dict(M=1025, w0=1)),
    ("estimator must be 1 \\(exp1\\) or 2 \\(exp2\\) \\(got 0\\)", dict(estimator=0)),
    ("estimator must be 1 \\(exp1\\) or 2 \\(exp2\\) \\(got 3\\)", dict(estimator=3)),
)


@pytest.mark.parametrize("entry", ("inr_mppca_denoise", "inr_mppca_denoise_f32"))
def test_every_refusal_comes_with_its_code_and_message_before_any_device_work(entry):
    import re
    lib = _lib.lib()
    fn = getattr(lib, entry)
    for text, change in REFUSALS:
        a = dict(GOOD)
        a.update(change)
        ptr = lambda v: None if v is None else _fake(v)
        rc = fn(ptr(a["out"]), ptr(a["sigma"]), ptr(a["rank"]), ptr(a["x"]), ptr(a["mask"]), a["M"], a["D"], a["H"], a["W"], a["w0"], a["w1"],
                a["w2"], a["estimator"], None)
        msg = lib.inr_last_error().decode()
        assert rc == _lib.INR_E_INVALID, (change, rc, msg)
        assert re.search(text, msg) and entry in msg, (change, msg)
    # an empty volume succeeds and launches nothing (this box has no device), whatever the window
    for D, H, W in ((0, 12, 12), (4, 0, 12), (4, 12, 0)):
        assert fn(_fake(1), None, None, _fake(4), None, 16, D, H, W, 3, 5, 5, 2, None) == 0
    assert _lib.INR_MPPCA_MAX_RANK == 64 and _lib.INR_MPPCA_MAX_LONG == 1024


def test_python_refusals_name_the_axis_and_come_before_the_device():
    x = np.zeros((16, 4, 12, 12))
    for text, kw in (("first window side \\(5\\) is larger than its axis \\(4\\)", dict(window=(5, 5, 5))),
                     ("third window side \\(13\\) is larger than its axis \\(12\\)", dict(window=(1, 1, 13))),
                     ("three odd sides", dict(window=(3, 4, 5))),
                     ("three odd sides", dict(window=(3, 5))),
                     ("estimator must be 'exp1' or 'exp2'", dict(estimator="exp3")),
                     ("measurement_axis must be 0 or -1", dict(measurement_axis=1)),
                     ("mask has shape", dict(window=(3, 5, 5), mask=np.ones((4, 12, 11)))),
                     ("exceeds the rank limit 64: shrink the window or split the measurements", dict(data=np.zeros((70, 4, 12, 12)), window=(3, 5, 5))),
                     ("at least 2 measurements", dict(data=np.zeros((1, 4, 12, 12)), window=(3, 5, 5))),
                     ("data must be \\[M, D, H, W\\]", dict(data=np.zeros((4, 4))))):
        kw = dict(kw)
        data = kw.pop("data", x)
        with pytest.raises(ValueError, match=text):
            denoise.mppca(data, **kw)
    with pytest.raises(TypeError, match="ndarray or a device tensor"):
        denoise.mppca([[1.0]])
    import torch
    with pytest.raises(ops.InrDeviceError):
        denoise.mppca(torch.zeros(16, 4, 12, 12), (3, 5, 5))


def test_stack_and_unstack_of_a_ragged_cell_are_bit_exact():
    rng = np.random.default_rng(7)
    ks = (1, 3, 2, 3)
    cell = np.empty((4, 2), dtype=object)
    for b, k in enumerate(ks):
        for te in range(2):
            if b == 0:
                cell[b, te] = rng.random((6, 5, 3)) if te == 0 else rng.random((6, 5, 3, 1))      # both layouts of b = 0
            else:
                cell[b, te] = rng.random((6, 5, 3, k))
    stack = denoise.stack_hybrid(cell)
    assert stack.shape == (2 * sum(ks), 6, 5, 3) and stack.dtype == np.float64
    # the order is (b, TE, acquisition), every acquisition its own measurement
    assert np.array_equal(stack[0], cell[0, 0]) and np.array_equal(stack[1], cell[0, 1][..., 0])
    assert np.array_equal(stack[2], cell[1, 0][..., 0]) and np.array_equal(stack[5], cell[1, 1][..., 0])
    assert np.array_equal(stack[-1], cell[3, 1][..., 2])
    back = denoise.unstack_hybrid(stack, cell)
    assert isinstance(back, np.ndarray) and back.dtype == object and back.shape == cell.shape
    for idx in np.ndindex(cell.shape):
        assert back[idx].shape == cell[idx].shape and back[idx].tobytes() == cell[idx].tobytes(), idx
    nested = [[cell[b, te] for te in range(2)] for b in range(4)]
    back = denoise.unstack_hybrid(denoise.stack_hybrid(nested), nested)
    assert isinstance(back, list) and all(back[b][te].tobytes() == cell[b, te].tobytes() for b in range(4) for te in range(2))
    f32 = [[cell[b, te].astype(np.float32) for te in range(2)] for b in range(4)]
    assert denoise.stack_hybrid(f32).dtype == np.float32
    with pytest.raises(ValueError, match="measurements of the cell"):
        denoise.unstack_hybrid(stack[:-1], cell)
    with pytest.raises(ValueError, match="the cells before it"):
        denoise.stack_hybrid([[cell[0, 0], rng.random((6, 5, 4))]])


@pytest.mark.parametrize("index", range(len(P.CASES)), ids=P.CASE_IDS)
def test_the_restatement_denoises_finds_the_noise_level_and_decides_no_rank_by_a_tie(index):
    case = P.cases()[index]
    out, sigma, rank, margin = P.reference(index)
    ratio = P.rmse(out, case["clean"]) / P.rmse(case["noisy"], case["clean"])
    med = float(np.median(sigma))
    r = min(case["M"], int(np.prod(case["window"])))
    print(f"{P.CASE_IDS[index]}: RMSE out / in = {ratio:.3f} (bound {RMSE_RATIO_BOUND}), median sigma {med:.4f} (within {SIGMA_RANGE[0]:.4f} .. "
          f"{SIGMA_RANGE[1]:.4f}), smallest margin {margin.min():.2e} (bound {MARGIN_BOUND:.0e}), ranks {np.bincount(rank.reshape(-1)).tolist()}")
    assert out.shape == case["noisy"].shape and sigma.shape == rank.shape == case["shape"]
    assert ratio <= RMSE_RATIO_BOUND
    assert SIGMA_RANGE[0] <= med <= SIGMA_RANGE[1]
    assert margin.min() >= MARGIN_BOUND
    assert rank.min() >= 0 and rank.max() <= r


def test_the_window_is_shifted_inward_and_the_own_column_is_the_centre_only_in_the_interior():
    assert [P.window_start(i, 5, 8) for i in range(8)] == [0, 0, 0, 1, 2, 3, 3, 3]
    assert [P.window_start(i, 3, 3) for i in range(3)] == [0, 0, 0] and P.window_start(0, 1, 1) == 0
    # a volume of exactly the window's size: every voxel shares one window, so sigma and rank are constant
    rng = np.random.default_rng(3)
    _, noisy = P.phantom(8, (3, 3, 3), P.SIGMA, rng)
    _, sigma, rank, _ = P.mppca(noisy, (3, 3, 3))
    assert np.unique(sigma).size == 1 and np.unique(rank).size == 1


def test_exact_rank_two_data_comes_back_with_rank_at_most_two():
    """Two of the phantom's components, no noise, the (16, (1, 24, 24), (1, 5, 5)) geometry: rank <= 2 at every voxel, out == x within the
    parity tolerance.  The loop alone cannot give this: the 14 small eigenvalues of G are rounding noise of either sign (-8e-14 .. 4e-14
    beside 0.14 and 473), for the clamped ones a = b = 0 and `b < a` is false, and from the first positive one on it would need
    (p + 1)(q - r + p + 1) < 16 -- it keeps all 16.  The rule for numerically zero eigenvalues (s_p <= q eps s_max = 2.6e-12 here) cuts
    them: measured rank 2 at all 576 voxels, sigma 0, max|out - x| = 5e-14."""
    clean, _ = P.phantom(16, (1, 24, 24), 0.0, None, n_components=2)
    out, sigma, rank, _ = P.mppca(clean, (1, 5, 5))
    tol = 32 * 4e-14 * np.abs(clean).max()          # the parity tolerance of the GPU test at the upper end of d_ref
    print(f"rank-2 data without noise: ranks {np.bincount(rank.reshape(-1)).tolist()}, max|out - x| = {np.abs(out - clean).max():.2e} (bound "
          f"{tol:.2e}), largest sigma {sigma.max():.2e}")
    assert np.abs(out - clean).max() <= tol
    assert rank.max() <= 2
    assert sigma.max() == 0.0
    # all-zero data: every eigenvalue is numerically zero, nothing is signal
    out, sigma, rank, _ = P.mppca(np.zeros((4, 1, 3, 3)), (1, 3, 3))
    assert (rank == 0).all() and (sigma == 0).all() and (out == 0).all()


def test_scaling_the_data_scales_out_and_sigma_and_leaves_the_rank():
    index = 2
    case = P.cases()[index]
    out, sigma, rank, _ = P.reference(index)
    out_k, sigma_k, rank_k, _ = P.mppca(1000.0 * case["noisy"], case["window"])
    d_out, d_sigma = P.reference_spread(index)
    e_out, e_sigma = float(np.abs(out_k / 1000.0 - out).max()), float(np.abs(sigma_k / 1000.0 - sigma).max())
    print(f"data x 1,000: max|out / 1000 - out| = {e_out:.2e} (32 d_ref = {32 * d_out:.2e}), sigma {e_sigma:.2e} (32 d_ref = {32 * d_sigma:.2e}), "
          f"rank equal {np.array_equal(rank, rank_k)}")
    assert np.array_equal(rank, rank_k)
    assert e_out <= 32 * d_out and e_sigma <= 32 * d_sigma


def test_the_mask_passes_data_through_and_leaves_the_voxels_inside_alone():
    case = P.cases()[2]
    mask = np.zeros(case["shape"], bool)
    mask[1:4, 2:7, 3:9] = True
    out, sigma, rank, _ = P.mppca(case["noisy"], case["window"], mask)
    ref = P.reference(2)
    assert np.array_equal(out[:, mask], ref[0][:, mask]) and np.array_equal(sigma[mask], ref[1][mask]) and np.array_equal(rank[mask], ref[2][mask])
    assert np.array_equal(out[:, ~mask], case["noisy"][:, ~mask]) and (sigma[~mask] == 0).all() and (rank[~mask] == -1).all()
