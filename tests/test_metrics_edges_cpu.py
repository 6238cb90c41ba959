"""CPU: what tests/test_gpu_metrics_edges.py leans on, checked without a device.

* the float64 restatements of tests/metrics_edges_common.py against the oracle (O.psnr, O.ssim2d, O.adc_map) and scipy on the
  edge inputs the GPU tests use;
* the conditions those tests assume: the planted ADC clips clip, the two spline solvers agree at n_in = 8192, the fractional mask
  separates m (m pred + b) from m (pred + b);
* the per-pixel body of auto_erd_kernel (csrc/auto_erd_pixel.h) compiled for the host into a stand-alone program with
  -fsanitize=address,undefined, run as a child process over the scikit-learn samples of tests/golden/erd.npz and over non-finite
  and overflowing pixels, and compared with oracle/erd_oracle.py.  This is where the walk's termination on such pixels is
  established; the device only sees them afterwards (tests/test_gpu_metrics_edges.py).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import erd_oracle as E
from oracle import inr_oracle as O
from oracle import rams_port as R
from tests import erd_volume_common as V
from tests import metrics_edges_common as M
from tests import rescale_common as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_psnr_restatement_equals_the_oracle():
    for n in M.PSNR_SIZES:
        for data_range in (1.0, 65535.0):
            x, y = M.psnr_pair(n, data_range, seed=n)
            assert M.psnr64(x, y, data_range) == pytest.approx(O.psnr(x, y, data_range), abs=1e-12)
            assert 20.0 < M.psnr64(x, y, data_range) < 60.0
    x, _ = M.psnr_pair(257, 1.0, seed=0)
    assert M.psnr64(x, x, 1.0) == np.inf


def test_ssim_window_sums_equal_the_oracle():
    """The direct window sums and the oracle's uniform_filter form are two float64 orderings of the same numbers: where they agree
    far below the 1e-10 the device is held to, a device mismatch is the device's."""
    worst = 0.0
    for shape, win in M.SSIM_SHAPES:
        for top, data_range in M.SSIM_RANGES:
            x, y = M.ssim_pair(shape, top, seed=win + shape[0])
            a, b = M.ssim_window_sums(x, y, data_range, win), O.ssim2d(x, y, data_range, win=win)
            worst = max(worst, abs(a - b))
            assert 0.0 < a < 1.0
    stack = [M.ssim_pair((9, 8), 1.0, seed=100 + k) for k in range(65)]
    for x, y in stack:
        worst = max(worst, abs(M.ssim_window_sums(x, y, 1.0, 7) - O.ssim2d(x, y, 1.0, win=7)))
    x, y = M.ssim_pair((150, 131), 1.0, seed=3)
    x[40:90, 30:80] = 0.0
    for thr in (0.0, 0.05):
        m = x > thr
        a, b = M.ssim_window_sums(x, y, 1.0, 7, mask_threshold=thr), O.ssim2d(x * m, y * m, 1.0, win=7)
        worst = max(worst, abs(a - b))
        assert abs(a - M.ssim_window_sums(x, y, 1.0, 7)) > 1e-3          # the mask matters on this input, at 0.0 too
    print(f"ssim: window sums vs uniform_filter, worst |difference| {worst:.2e}")
    assert worst <= 1e-12
    c = np.full((20, 17), 0.37, np.float32)
    assert M.ssim_window_sums(c, c, 1.0, 7) == 1.0


def test_adc_inputs_do_what_the_gpu_test_assumes():
    want = O.adc_map(np.asarray(M.CLIP_BVALS), M.CLIP_DATA)
    assert want.tolist() == [3.0, -10.0]
    raw = O.adc_map(np.asarray(M.CLIP_BVALS), M.CLIP_DATA, min_adc=-np.inf, max_adc=np.inf)
    assert raw[0] > 15.0 and raw[1] < -15.0                               # the planted clips really clip, on both sides
    for n_b in M.ADC_NB:
        b, data = M.adc_case(n_b, 257, seed=n_b)
        adc = O.adc_map(b, data)
        assert 0.3 < adc.min() and adc.max() < 2.8                        # of order one and inside the clips
    b, data = M.adc_case(3, 7, seed=1)
    data[2, 1] = -5.0
    with np.errstate(invalid="ignore"):
        assert np.isnan(O.adc_map(b, data)).tolist() == [False, False, True, False, False, False, False]
    assert M.ulp32_distance(np.float32([1.0, np.nan, -0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), np.nan, 0.0])
                            ).tolist() == [1, 0, 0]


def test_fractional_mask_separates_the_two_bias_formulas():
    for nimg, size, border in M.SHIFT_CASES:
        yt, yp, mk = M.shift_case(nimg, size, border, seed=size)
        assert set(np.unique(mk)) <= {0.0, 0.5, 1.0} and (mk == 0.5).any()
        with np.errstate(divide="ignore"):                                # an exact 0 loss has an infinite cPSNR
            right, _ = R.shift_losses(yt, yp, mk, size, border=border)
        wrong = M.shift_losses_bias_outside_mask(yt, yp, mk, size, border)
        assert np.isfinite(right).all()
        assert (np.abs(wrong - right) > 1e-3 * np.abs(right)).any(), (size, border)      # far above rtol = 1e-9
        binary = (mk > 0.25).astype(np.float32)
        with np.errstate(divide="ignore"):
            assert np.allclose(M.shift_losses_bias_outside_mask(yt, yp, binary, size, border),
                               R.shift_losses(yt, yp, binary, size, border=border)[0], rtol=1e-12)
        loss, grad = M.shift_l1_and_grad(yt, yp, mk, size, border)
        assert np.allclose(loss, right, rtol=1e-12)
        assert grad.shape == yp.shape and np.count_nonzero(grad[:, :border]) == 0 and np.abs(grad).max() > 0


def test_zoom_restatement_on_the_edge_shapes():
    for shape, out_hw in (((25, 19), (37, 31)), ((1, 9), (3, 14)), ((9, 1), (14, 3)), ((5, 4), (5, 4))):
        img = RC.case_image(shape, seed=shape[0])
        want = M.zoom_linear(img, out_hw)
        got = RC.restated_resize(img, out_hw, order=1, mode="reflect", anti_aliasing=False, clip=False)
        assert np.abs(got - want).max() <= 1e-14, shape
    img = RC.case_image((5, 4), seed=5)
    assert np.array_equal(M.zoom_linear(img, (5, 4)), img)


def test_thomas_restatement_against_scipy():
    for n_in in (4, 5, 7, 128):
        lines = M.spline_lines(9, n_in, seed=n_in)
        for n_out in (1, 2, 37):
            assert np.abs(M.thomas_cubic(lines, n_out) - M.scipy_cubic(lines, n_out)).max() <= M.SPLINE_BOUND, (n_in, n_out)
    lines = M.spline_lines(5, 8192, seed=8192)
    for n_out in (37, 16385):
        e0 = np.abs(M.thomas_cubic(lines, n_out) - M.scipy_cubic(lines, n_out)).max()
        print(f"spline n_in = 8192, n_out = {n_out}: e0 = max|restatement - scipy| = {e0:.3e}")
        assert e0 < M.SPLINE_E0_LIMIT


# ---- the host program around auto_erd_pixel -------------------------------------------------------------------------------------
def _token(v):
    return "nan" if np.isnan(v) else ("inf" if v == np.inf else ("-inf" if v == -np.inf else float(v).hex()))


def _host_accept(tmp_path, pixels):
    """pixels: [(rule, erd_positive, values)] -> [accept mask as a list of 0 / 1], through the sanitized host program."""
    gxx, clang = shutil.which("g++"), shutil.which("clang++")
    assert gxx or clang, "no host C++ compiler"
    # the sanitizer runtimes linked into the program itself (clang's default): it then starts whatever else the loader brings in
    cxx, static = (gxx, ["-static-libasan", "-static-libubsan"]) if gxx else (clang, [])
    exe = str(tmp_path / "auto_erd_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                            "-I", os.path.join(ROOT, "mri-super-resolution_amd", "csrc"),
                            os.path.join(ROOT, "tools", "auto_erd_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    path = str(tmp_path / "samples.txt")
    with open(path, "w") as fh:
        for rule, positive, values in pixels:
            fh.write(f"{rule} {int(positive)} {len(values)} " + " ".join(_token(v) for v in values) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-2000:]
    lines = run.stdout.split()
    assert len(lines) == len(pixels)
    return [[int(ch) for ch in line] for line in lines]


def test_host_program_equals_the_oracle_on_the_sklearn_samples(tmp_path, golden):
    g = golden("erd.npz")
    samples = [v[:n] for v, n in zip(g["values"], g["lengths"])]
    pixels = [(rule, True, x) for x in samples for rule in (1, 2)] + [(2, False, x) for x in samples[::40]]
    rng = np.random.default_rng(32)
    for n in (17, 25, 31, 32):                                          # beyond the fixtures' n <= 16, up to the limit
        for _ in range(6):
            x = np.round(rng.normal(300.0, 12.0, n))
            x[rng.random(n) < 0.1] += 150.0
            pixels += [(1, True, x), (2, True, x)]
    got = _host_accept(tmp_path, pixels)
    assert len(samples) == 2460
    for (rule, positive, x), keep in zip(pixels, got):
        assert keep == E.accept_mask(x, rule, len(x), positive).tolist(), (rule, positive, x)


def test_host_program_on_non_finite_and_overflowing_pixels(tmp_path):
    """A NaN, an infinity or an overflowing largest distance: the walk is never entered, the pixel keeps everything, and the
    program ends (under the address and undefined-behaviour sanitizers).  Where the largest distance overflows the volume
    kernel's extent walk finds no neighbour (V.extent_two_clusters is None), which is its "keeps everything" too."""
    clean, _ = V.volume_case((70, 12), (4, 4, 4), seed=21)
    x = M.plant_overflow(M.plant_non_finite(clean))
    rng = np.random.default_rng(5)
    big = 1e308
    extra = [np.array([big, -big]), np.array([big, big, -big]), np.array([-big, 3.0, 4.0, big, 5.0]),
             np.array([np.nan, np.nan]), np.array([np.inf, np.inf, np.inf]), np.array([np.inf, -np.inf, 0.0]),
             np.array([1.0, 2.0, np.nan] + [3.0] * 29), np.array([big] + [-big] * 31)]
    for _ in range(40):                                                  # a random mixture of huge and small finite values
        n = int(rng.integers(2, 33))
        v = rng.choice([big, -big, 9e307, -9e307, 1.0, -2.0, 0.0], size=n)
        extra.append(v.astype(np.float64))
    # huge but not overflowing: clustered like any other pixel
    extra += [np.array([8e307, -8e307, 8e307, 7e307]), np.array([8.9e307, -8.9e307])]
    pixels = [(rule, True, row) for row in list(x) + extra for rule in (1, 2)]
    got = _host_accept(tmp_path, pixels)
    n_overflow = n_clustered = 0
    for (rule, _, v), keep in zip(pixels, got):
        with np.errstate(over="ignore", invalid="ignore"):
            overflow = bool(np.isfinite(v).all() and not np.isfinite(v.max() - v.min()))
        if not np.isfinite(v).all() or overflow:
            assert keep == [1] * len(v), (rule, v)
            if overflow:
                assert V.extent_two_clusters(v) is None, v
                n_overflow += 1
        else:
            with np.errstate(over="ignore"):                             # the mean of huge values may overflow, as on the device
                assert keep == E.accept_mask(v, rule, len(v)).tolist(), (rule, v)
            n_clustered += 1
    bad = set(M.BAD_PIXELS) | {M.OVERFLOW_PIXEL}
    assert n_overflow >= 10 and n_clustered >= 2 * (70 - len(bad))
    keep = np.array(got[:140]).reshape(70, 2, 12)
    for rule in (1, 2):                                                  # the other pixels are what they are without the bad ones
        want = V.accept_weights(clean, rule)
        good = np.setdiff1d(np.arange(70), sorted(bad))
        assert np.array_equal(keep[good, rule - 1], want[good])
