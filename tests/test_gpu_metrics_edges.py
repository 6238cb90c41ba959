"""-m gpu: the kernels of csrc/metrics.hip at their edges, each against a plain float64 statement of the same operation
(tests/metrics_edges_common.py, the oracle, scipy): second trips of the stride loops, second and ragged blocks of the finish
kernels, the size limits the code states, the refusals, and the per-slice AutoERD kernel on non-finite pixels (whose walk was first
run on the host: tests/test_metrics_edges_cpu.py).  Every test prints what it measured before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

from mri_super_resolution_amd import _lib, baselines, metrics, ops
from mri_super_resolution_amd._lib import InrHipError, check, lib
from oracle import inr_oracle as O
from oracle import rams_port as R
from tests import erd_volume_common as V
from tests import metrics_edges_common as M
from tests import rescale_common as RC

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


# ---- PSNR ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data_range", [1.0, 65535.0])
def test_psnr_sizes_around_one_trip_of_the_grid(data_range):
    worst = 0.0
    for n in M.PSNR_SIZES:
        x, y = M.psnr_pair(n, data_range, seed=n)
        got = metrics.psnr(dev(x), dev(y), data_range=data_range).item()
        want = M.psnr64(x, y, data_range)
        worst = max(worst, abs(got - want))
        print(f"psnr n = {n}, R = {data_range:g}: device {got:.12f} dB, float64 {want:.12f} dB")
        assert abs(got - want) <= M.PSNR_BOUND, n
    print(f"psnr: worst |difference| {worst:.2e} dB (bound {M.PSNR_BOUND:g})")
    x, _ = M.psnr_pair(16385, data_range, seed=1)
    assert metrics.psnr(dev(x), dev(x), data_range=data_range).item() == np.inf == M.psnr64(x, x, data_range)


def test_psnr_65_images_each_with_its_own_noise():
    pairs = [M.psnr_pair(16385, 1.0, seed=200 + k, noise=0.001 * (k + 1)) for k in range(65)]
    x = np.stack([p[0] for p in pairs]).reshape(65, 5, 3277)
    y = np.stack([p[1] for p in pairs]).reshape(65, 5, 3277)
    got = metrics.psnr(dev(x), dev(y), data_range=1.0, per_image=True).cpu().numpy()
    want = np.array([M.psnr64(x[k], y[k], 1.0) for k in range(65)])
    print(f"psnr 65 x 16385: worst |difference| {np.abs(got - want).max():.2e} dB (bound {M.PSNR_BOUND:g}); "
          f"values {want.min():.2f} .. {want.max():.2f} dB")
    assert got.shape == (65,) and np.ptp(want) > 30.0
    assert np.abs(got - want).max() <= M.PSNR_BOUND


# ---- SSIM ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top,data_range", M.SSIM_RANGES)
def test_ssim_shapes_windows_and_ranges(top, data_range):
    worst = 0.0
    for shape, win in M.SSIM_SHAPES:
        x, y = M.ssim_pair(shape, top, seed=win + shape[0])
        got = metrics.ssim(dev(x), dev(y), data_range=data_range, win_size=win).item()
        a, b = O.ssim2d(x, y, data_range, win=win), M.ssim_window_sums(x, y, data_range, win)
        worst = max(worst, abs(got - a), abs(got - b))
        print(f"ssim {shape} win {win} R = {data_range:g}: device {got:.15f}, oracle {a:.15f}, window sums {b:.15f}")
        assert abs(got - a) <= M.SSIM_BOUND and abs(got - b) <= M.SSIM_BOUND, (shape, win)
    print(f"ssim: worst |difference| {worst:.2e} (bound {M.SSIM_BOUND:g})")


def test_ssim_65_images_mask_and_constant_pair():
    pairs = [M.ssim_pair((9, 8), 1.0, seed=100 + k) for k in range(65)]
    x, y = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    got = metrics.ssim(dev(x), dev(y), data_range=1.0, win_size=7).cpu().numpy()
    want = np.array([O.ssim2d(x[k], y[k], 1.0, win=7) for k in range(65)])
    print(f"ssim 65 x 9 x 8: worst |difference| {np.abs(got - want).max():.2e} (bound {M.SSIM_BOUND:g})")
    assert got.shape == (65,) and np.unique(want).size == 65
    assert np.abs(got - want).max() <= M.SSIM_BOUND
    # the mask: a threshold of 0.0 switches it on, as any other does
    x, y = M.ssim_pair((150, 131), 1.0, seed=3)
    x[40:90, 30:80] = 0.0
    plain = metrics.ssim(dev(x), dev(y), data_range=1.0).item()
    for thr in (0.0, 0.05):
        got = metrics.ssim(dev(x), dev(y), data_range=1.0, mask_threshold=thr).item()
        m = x > thr
        a, b = O.ssim2d(x * m, y * m, 1.0), M.ssim_window_sums(x, y, 1.0, 7, mask_threshold=thr)
        print(f"ssim mask > {thr}: device {got:.15f}, oracle {a:.15f}, window sums {b:.15f}; unmasked {plain:.6f}")
        assert abs(got - a) <= M.SSIM_BOUND and abs(got - b) <= M.SSIM_BOUND
        assert abs(got - plain) > 1e-3
    c = np.full((2, 20, 17), 0.37, np.float32)
    c[1] = 2500.0
    assert metrics.ssim(dev(c), dev(c), data_range=4000.0).cpu().numpy().tolist() == [1.0, 1.0]


def test_ssim_refusals():
    x = dev(np.zeros((2, 6, 9), np.float32))
    out = torch.empty(2, dtype=torch.float64, device="cuda")
    ws = ops._ws(lib().inr_metric_workspace_bytes(2), x.device)
    for h, w, win in ((6, 9, 4), (6, 9, 1), (6, 9, 7), (9, 6, 7)):
        rc = lib().inr_ssim2d(out.data_ptr(), x.data_ptr(), x.data_ptr(), 2, h, w, win, 1.0, 0, 0.0, ws.data_ptr(), ws.numel(),
                              ops._stream())
        assert rc == _lib.INR_E_INVALID, (h, w, win)
        with pytest.raises(ValueError):
            metrics.ssim(x.reshape(2, h, w), x.reshape(2, h, w), win_size=win)


# ---- ADC -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_b", M.ADC_NB)
def test_adc_within_one_fp32_ulp_of_the_oracle(n_b):
    worst = 0
    for npix in M.ADC_PIXELS:
        b, data = M.adc_case(n_b, npix, seed=n_b)
        if npix >= 255:
            data[3, n_b - 1] = -5.0                                      # log of a negative number: NaN, where NumPy has it
        got = metrics.calculate_ADC_device(b, dev(data)).cpu().numpy()
        with np.errstate(invalid="ignore"):
            want = O.adc_map(b.astype(np.float64), data).astype(np.float32)
        d = int(M.ulp32_distance(got, want).max())
        worst = max(worst, d)
        print(f"adc n_b = {n_b}, {npix} pixels: largest distance {d} fp32 ULP (bound {M.ADC_ULP})")
        assert got.shape == (npix,) and np.array_equal(np.isnan(got), np.isnan(want))
        assert np.isnan(want).sum() == (1 if npix >= 255 else 0)
        assert d <= M.ADC_ULP
    print(f"adc n_b = {n_b}: worst {worst} fp32 ULP")


def test_adc_clips_and_refusals():
    got = metrics.calculate_ADC_device(M.CLIP_BVALS, dev(M.CLIP_DATA)).cpu().numpy()
    want = O.adc_map(np.asarray(M.CLIP_BVALS), M.CLIP_DATA)
    print(f"adc clips: device {got.tolist()}, oracle {want.tolist()}")
    assert got.tolist() == [3.0, -10.0] == want.tolist()
    for n_b in (33, 1):
        with pytest.raises(InrHipError, match="n_b"):
            metrics.calculate_ADC_device(np.arange(n_b), dev(np.ones((4, n_b), np.float32)))


# ---- shift-tolerant losses and the gradient: the C entry points, any border -----------------------------------------------------------
def _shift_loss(yt, yp, mk, size, border, mode):
    n = yt.shape[0]
    t = [dev(a) for a in (yt, yp, mk)]
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    ws = torch.empty((lib().inr_rams_shift_loss_workspace_bytes(n, border) + 7) // 8, dtype=torch.float64, device="cuda")
    check(lib().inr_rams_shift_loss(out.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, size, border, mode,
                                    ws.data_ptr(), ws.numel() * 8, ops._stream()), "inr_rams_shift_loss")
    return out.cpu().numpy()


def _shift_grad(yt, yp, mk, size, border, upstream):
    n = yt.shape[0]
    t = [dev(a) for a in (yt, yp, mk)]
    up = dev(upstream)
    loss = torch.empty(n, dtype=torch.float64, device="cuda")
    grad = torch.empty_like(t[1])
    ws = torch.empty((lib().inr_rams_shift_loss_grad_workspace_bytes(n, border) + 7) // 8, dtype=torch.float64, device="cuda")
    check(lib().inr_rams_shift_loss_grad(loss.data_ptr(), grad.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                         up.data_ptr(), n, size, border, ws.data_ptr(), ws.numel() * 8, ops._stream()),
          "inr_rams_shift_loss_grad")
    return loss.cpu().numpy(), grad.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("nimg,size,border", M.SHIFT_CASES)
def test_shift_losses_and_gradient_at_every_border(nimg, size, border):
    yt, yp, mk = M.shift_case(nimg, size, border, seed=size)
    with np.errstate(divide="ignore"):
        want_l1, want_ps = R.shift_losses(yt, yp, mk, size, border=border)
    got_l1, got_ps = _shift_loss(yt, yp, mk, size, border, 0), _shift_loss(yt, yp, mk, size, border, 1)
    finite = np.isfinite(want_ps)
    rel = lambda g, w: float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300))) if w.size else 0.0
    print(f"shift losses {nimg} x {size}, border {border}: cL1 rel. error {rel(got_l1[want_l1 > 0], want_l1[want_l1 > 0]):.2e}, "
          f"cPSNR rel. error {rel(got_ps[finite], want_ps[finite]):.2e} (rtol {M.SHIFT_LOSS_RTOL:g})")
    assert np.allclose(got_l1, want_l1, rtol=M.SHIFT_LOSS_RTOL, atol=0)
    assert np.array_equal(got_ps[~finite], want_ps[~finite])            # an exact 0 loss: +inf on both sides
    assert np.allclose(got_ps[finite], want_ps[finite], rtol=M.SHIFT_LOSS_RTOL, atol=0)
    up = np.linspace(0.5, 2.0, nimg).astype(np.float32)
    want_loss, want_grad = M.shift_l1_and_grad(yt, yp, mk, size, border, upstream=up)
    loss, grad = _shift_grad(yt, yp, mk, size, border, up)
    scale = np.abs(want_grad).max()
    print(f"shift gradient: max|difference| {np.abs(grad - want_grad).max():.3e}, max|gradient| {scale:.3e} "
          f"(bound {M.SHIFT_GRAD_REL:g} of it)")
    assert np.allclose(loss, want_loss, rtol=M.SHIFT_LOSS_RTOL, atol=0)
    assert scale > 0 and np.abs(grad - want_grad).max() <= M.SHIFT_GRAD_REL * scale
    if border:
        assert np.count_nonzero(grad[:, :border]) == 0 and np.count_nonzero(grad[:, :, -border:]) == 0


def test_shift_losses_all_zero_mask_on_one_image():
    nimg, size, border = 3, 12, 3
    yt, yp, mk = M.shift_case(nimg, size, border, seed=77)
    mk[1] = 0.0
    with np.errstate(all="ignore"):
        want_l1, want_ps = R.shift_losses(yt, yp, mk, size, border=border)
    for mode, want in ((0, want_l1), (1, want_ps)):
        got = _shift_loss(yt, yp, mk, size, border, mode)
        print(f"zero mask on image 1, mode {mode}: device {got.tolist()}, float64 {want.tolist()}")
        assert np.isnan(got).tolist() == [False, True, False] == np.isnan(want).tolist()
        assert np.allclose(got[[0, 2]], want[[0, 2]], rtol=M.SHIFT_LOSS_RTOL, atol=0)
    loss, _ = _shift_grad(yt, yp, mk, size, border, np.ones(nimg, np.float32))
    assert np.isnan(loss).tolist() == [False, True, False]


# ---- linear up-scale -----------------------------------------------------------------------------------------------------------
def _rescale(img, out_hw):
    x = dev(img)
    n, h, w = x.shape
    out = torch.empty((n,) + tuple(out_hw), dtype=torch.float32, device="cuda")
    check(lib().inr_rescale2d_linear(out.data_ptr(), x.data_ptr(), n, h, w, out_hw[0], out_hw[1], ops._stream()),
          "inr_rescale2d_linear")
    return out.cpu().numpy()


def test_rescale_linear_second_trip_of_the_stride_loop():
    """4098 x 4096 = 16,785,408 outputs: more than the 65,536 x 256 = 16,777,216 threads of the capped grid."""
    img = RC.case_image((2049, 2048), seed=1)
    got = _rescale(img[None], (4098, 4096))[0]
    err = np.abs(got - M.zoom_linear(img, (4098, 4096)))
    print(f"rescale 2049 x 2048 -> 4098 x 4096: max|difference| {err.max():.3e} (bound {RC.BOUND * img.max():.3e}), "
          f"in the second trip {err.reshape(-1)[65536 * 256:].max():.3e}")
    assert err.max() <= RC.BOUND * np.abs(img).max()


def test_rescale_linear_odd_factors_single_rows_and_the_identity():
    for shape, out_hw in (((25, 19), (37, 31)), ((1, 9), (3, 14)), ((9, 1), (14, 3))):
        img = RC.case_image(shape, seed=shape[0])
        err = np.abs(_rescale(img[None], out_hw)[0] - M.zoom_linear(img, out_hw)).max()
        print(f"rescale {shape} -> {out_hw}: max|difference| {err:.3e} (bound {RC.BOUND * img.max():.3e})")
        assert err <= RC.BOUND * np.abs(img).max(), shape
    stack = np.stack([RC.case_image((5, 4), seed=k) for k in range(3)]) * np.array([1.0, -300.0, 6e4])[:, None, None]
    stack = stack.astype(np.float32)
    same = _rescale(stack, (5, 4))
    assert np.array_equal(same.view(np.uint32), stack.view(np.uint32))   # the identity, bit for bit
    for k in range(3):
        assert np.array_equal(M.zoom_linear(stack[k], (5, 4)), stack[k].astype(np.float64))


# ---- through-plane spline ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out", [37, 16385])
def test_resize_z_at_the_largest_line_length(n_out):
    """n_in = 8192: the Thomas factor fills the 64 KiB of dynamic LDS exactly.  scipy's banded solve and the Thomas recurrence
    differ in float64 at this length (e0, measured here on the host), so scipy is held to max(1e-12, 4 e0) and the restatement
    of the kernel's own recurrence to 1e-12."""
    lines = M.spline_lines(5, 8192, seed=8192)
    got = baselines.resize_z(lines, n_out)
    ref, restated = M.scipy_cubic(lines, n_out), M.thomas_cubic(lines, n_out)
    e0 = np.abs(restated - ref).max()
    e_scipy, e_restated = np.abs(got - ref).max(), np.abs(got - restated).max()
    print(f"resize_z n_in = 8192, n_out = {n_out}: e0 = max|restatement - scipy| = {e0:.3e}, max|kernel - scipy| = {e_scipy:.3e}, "
          f"max|kernel - restatement| = {e_restated:.3e}")
    assert got.shape == (5, n_out)
    assert e_scipy <= max(M.SPLINE_BOUND, 4 * e0) and e_restated <= M.SPLINE_BOUND


def test_resize_z_single_output_ragged_second_block_and_refusal():
    for n_in in (4, 5):
        lines = M.spline_lines(3, n_in, seed=n_in)
        got = baselines.resize_z(lines, 1)
        err = np.abs(got - M.scipy_cubic(lines, 1)).max()
        print(f"resize_z n_in = {n_in}, n_out = 1: max|kernel - scipy| = {err:.3e}")
        assert got.shape == (3, 1) and err <= M.SPLINE_BOUND and np.array_equal(got[:, 0], lines[:, 0])
    lines = M.spline_lines(257, 4, seed=257)
    for n_out in (1, 9):
        err = np.abs(baselines.resize_z(lines, n_out) - M.scipy_cubic(lines, n_out)).max()
        print(f"resize_z 257 lines of 4, n_out = {n_out}: max|kernel - scipy| = {err:.3e} (bound {M.SPLINE_BOUND:g})")
        assert err <= M.SPLINE_BOUND
    with pytest.raises(InrHipError, match="8192"):
        baselines.resize_z(np.zeros((2, 8193)), 9)


# ---- per-slice AutoERD on non-finite pixels --------------------------------------------------------------------------------------
def test_auto_erd_non_finite_pixels_keep_every_acquisition():
    """The rule of erd_volume.hip in the per-slice kernel: a pixel with a NaN or an infinity among its acquisitions, or whose
    largest pairwise distance overflows, is not clustered and keeps everything; the other pixels of its wave are unaffected; the
    whole array equals the volume kernel's."""
    from mri_super_resolution_amd import erd
    clean, _ = V.volume_case((70, 12), (4, 4, 4), seed=21)
    x = M.plant_non_finite(clean)
    bad = list(M.BAD_PIXELS)
    good = np.setdiff1d(np.arange(70), bad)
    for rule in (1, 2):
        got = erd.auto_erd(x.reshape(1, 70, 12), rule)[0]
        ref = erd.auto_erd(clean.reshape(1, 70, 12), rule)[0]
        vol = erd.auto_erd_volume(x, rule)
        print(f"auto_erd rule {rule}: bad pixels keep {got[bad].sum(axis=1).tolist()} of 12; rejected elsewhere {int((got[good] == 0).sum())}")
        assert got[bad].all()
        assert np.array_equal(got[good], ref[good]) and (ref[good] == 0).any()
        assert np.array_equal(got, vol)
        assert np.array_equal(got, V.accept_weights(x, rule))
    y = M.plant_overflow(x)                                              # +-1e308: the largest distance overflows
    small = np.array([[[1e308, -1e308], [3.0, 4.0]]])
    for rule in (1, 2):
        got = erd.auto_erd(y.reshape(1, 70, 12), rule)[0]
        vol = erd.auto_erd_volume(y, rule)
        print(f"auto_erd rule {rule}: overflowing pixel keeps {int(got[M.OVERFLOW_PIXEL].sum())} of 12")
        assert got[M.OVERFLOW_PIXEL].all() and np.array_equal(got, vol)
        assert np.array_equal(erd.auto_erd(small, rule), erd.auto_erd_volume(small, rule))
    assert erd.auto_erd(small, 2)[0].tolist() == [[1, 1], [0, 1]]
