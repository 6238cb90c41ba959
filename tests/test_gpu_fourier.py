"""GPU: Fourier (k-space zero-fill / truncation) re-sampling of csrc/fourier.hip -- the operator kernel against the float64 restatement,
the fp64 MFMA apply kernel entry by entry on impulses, values against scipy.signal.resample and the trigonometric polynomial
(tests/fourier_common.py), the properties that define the operation, and the ``--zerofill`` flag of superresDWI.

Bounds are derived, not measured: an operator entry is a sum of at most n/2 + 1 cosines of rounding 2^-53 each, divided by n (1e-13
absolute leaves a few hundred ulp); values in fp64 carry the project's 1e-12 of max(max|in|, max|want|); fp32 in and out is fp64
rounded once, 2e-7 of the same scale (tests/rescale_common.py: BOUND).  Every test prints what it measured before it asserts."""
import json
import os

import numpy as np
import pytest
import scipy.signal
import torch

from tests import fourier_common as F
from tests import rescale_common as R
from mri_super_resolution_amd import _lib, baselines, matio, metrics, ops, reports
from mri_super_resolution_amd.scripts import superresDWI as dwi_script

pytestmark = pytest.mark.gpu

OPERATOR_PAIRS = F.PAIRS + F.GPU_EXTRA_PAIRS


def _modes(n, m):
    return [(a, b) for b in F.BOUNDARIES for a in F.ALIGNS if not (a == "sample" and b == "mirror" and not F.mirror_sample_ok(n, m))]


@pytest.mark.parametrize("n,m", OPERATOR_PAIRS, ids=[f"{n}to{m}" for n, m in OPERATOR_PAIRS])
def test_operator_matches_the_restatement(n, m):
    for align, boundary in _modes(n, m):
        for apodize in F.APODIZE:
            got = baselines.fourier_operator(n, m, align, boundary, apodize)
            want = F.restated_operator(n, m, align, boundary, apodize)
            err = float(np.abs(got - want).max())
            print(f"operator {n}->{m} {align} {boundary} apodize {apodize}: max|got - want| = {err:.3e} (bound 1e-13)")
            assert got.dtype == np.float64 and got.shape == (m, n)
            assert err <= 1e-13


@pytest.mark.parametrize("shape,out_hw", [((17, 19), (33, 38)), ((50, 25), (25, 50))], ids=["17x19to33x38", "50x25to25x50"])
def test_an_impulse_gives_the_outer_product_of_two_operator_columns(shape, out_hw):
    """Pins the row / column mapping of the matrix instruction entry by entry: asymmetric operators, ragged tiles."""
    (h, w), (oh, ow) = shape, out_hw
    a_rows, a_cols = F.restated_operator(h, oh, "center", "mirror"), F.restated_operator(w, ow, "center", "mirror")
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 3, (2 * w) // 3)]
    x = np.zeros((len(spots), h, w))
    for k, (r, c) in enumerate(spots):
        x[k, r, c] = 1.0
    got = baselines.fourier_resize(x, out_hw, "center", "mirror")
    for k, (r, c) in enumerate(spots):
        want = np.outer(a_rows[:, r], a_cols[:, c])
        err = float(np.abs(got[k] - want).max())
        print(f"impulse at ({r}, {c}) of {h} x {w} -> {oh} x {ow}: max|got - outer| = {err:.3e} (bound 1e-13)")
        assert err <= 1e-13


VALUE_SHAPES = [((25, 19), (50, 38)), ((50, 38), (25, 19)), ((26, 26), (51, 52))]


@pytest.fixture(scope="module")
def value_cases():
    """(input [3][4][h][w], out_hw, align, boundary, apodize, oracle) of every defined mode, computed once."""
    cases = []
    for k, (shape, out_hw) in enumerate(VALUE_SHAPES):
        x = np.random.default_rng(10 + k).standard_normal((3, 4) + shape).astype(np.float32).astype(np.float64)    # fp32-representable
        for boundary in F.BOUNDARIES:
            for align in F.ALIGNS:
                if boundary == "mirror" and align == "sample" and \
                        not (F.mirror_sample_ok(shape[0], out_hw[0]) and F.mirror_sample_ok(shape[1], out_hw[1])):
                    continue
                for apodize in (0.0, 1.0):
                    cases.append((x, out_hw, align, boundary, apodize, F.oracle_resize(x, out_hw, align, boundary, apodize)))
    return cases


def test_values_fp64_against_the_oracles(value_cases):
    assert len(value_cases) == 2 * (4 + 4 + 3)
    for x, out_hw, align, boundary, apodize, want in value_cases:
        got = baselines.fourier_resize(x, out_hw, align, boundary, apodize)
        err, tol = float(np.abs(got - want).max()), F.bound(x, want)
        print(f"fp64 {x.shape[-2:]} -> {out_hw} {align} {boundary} apodize {apodize}: max|got - want| = {err:.3e} (bound {tol:.3e})")
        assert got.dtype == np.float64 and got.shape == (3, 4) + tuple(out_hw)
        assert err <= tol
        # a device fp64 tensor takes the same kernels
        dev = baselines.fourier_resize(torch.from_numpy(x).cuda(), out_hw, align, boundary, apodize)
        assert dev.is_cuda and dev.dtype == torch.float64 and np.array_equal(dev.cpu().numpy(), got)


def test_values_where_every_axis_spans_several_tiles():
    """70 x 130 -> 140 x 257: five 64-wide column tiles, three row tiles, nine K stages, all of them ragged."""
    x = np.random.default_rng(20).standard_normal((2, 70, 130))
    for align, boundary in (("sample", "periodic"), ("center", "mirror")):
        want = F.oracle_resize(x, (140, 257), align, boundary)
        got = baselines.fourier_resize(x, (140, 257), align, boundary)
        err, tol = float(np.abs(got - want).max()), F.bound(x, want)
        print(f"fp64 70 x 130 -> 140 x 257 {align} {boundary}: max|got - want| = {err:.3e} (bound {tol:.3e})")
        assert err <= tol
        if align == "sample":            # down again: truncating a zero-filled spectrum gives the line back
            back = baselines.fourier_resize(got, (70, 130), align, boundary)
            print(f"and back: max|back - x| = {np.abs(back - x).max():.3e}")
            assert np.abs(back - x).max() <= F.bound(x, want)


def test_values_fp32_in_and_out(value_cases):
    for x, out_hw, align, boundary, apodize, want in value_cases:
        got = baselines.fourier_resize(torch.from_numpy(x.astype(np.float32)).cuda(), out_hw, align, boundary, apodize)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, 4) + tuple(out_hw)
        err, tol = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max()), F.bound(x, want, R.BOUND)
        print(f"fp32 {x.shape[-2:]} -> {out_hw} {align} {boundary} apodize {apodize}: max|got - want| = {err:.3e} (bound {tol:.3e})")
        assert err <= tol


def test_a_constant_image_stays_constant():
    x = np.full((2, 25, 19), 0.7)
    for out_hw in ((50, 38), (13, 7), (25, 19)):
        for align, boundary in (("sample", "periodic"), ("center", "periodic"), ("center", "mirror")):
            for apodize in (0.0, 0.5):
                got = baselines.fourier_resize(x, out_hw, align, boundary, apodize)
                err = float(np.abs(got - 0.7).max())
                print(f"constant 25 x 19 -> {out_hw} {align} {boundary} apodize {apodize}: max|got - 0.7| = {err:.3e}")
                assert err <= 1e-13
    got = baselines.fourier_resize(x, (50, 38), "sample", "mirror")
    assert np.abs(got - 0.7).max() <= 1e-13
    assert baselines.fourier_rescale(x, 2).shape == (2, 50, 38) and np.array_equal(baselines.fourier_rescale(x, 2), got)


def test_a_band_limited_image_is_restored_from_its_decimation():
    n = 50
    rng = np.random.default_rng(5)
    yy, xx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x = np.zeros((n, n))
    for _ in range(6):                                   # frequencies below n/4 = 12.5: the decimation loses nothing
        fy, fx = rng.integers(0, 12, size=2)
        x += rng.standard_normal() * np.cos(2 * np.pi * (fy * yy + fx * xx) / n + rng.uniform(0, 2 * np.pi))
    got = baselines.fourier_resize(x[::2, ::2], (n, n), "sample", "periodic")
    err = float(np.abs(got - x).max())
    print(f"band-limited 50 x 50 from its 25 x 25 decimation: max|got - x| = {err:.3e} (bound 1e-12 absolute; max|x| = {np.abs(x).max():.3g})")
    assert err <= 1e-12


def test_resample_is_scipy_signal_resample_on_any_axis():
    x = np.random.default_rng(6).standard_normal((6, 9, 10))
    for axis, num in ((0, 15), (-1, 7), (0, 6), (-1, 25)):
        want = scipy.signal.resample(x, num, axis=axis)
        got = baselines.fourier_resample(x, num, axis=axis, boundary="periodic")
        err = float(np.abs(got - want).max())
        print(f"fourier_resample axis {axis} -> {num}: max|got - scipy| = {err:.3e} (bound {F.bound(x, want):.3e})")
        assert got.shape == want.shape and got.dtype == np.float64
        assert err <= F.bound(x, want)
    # the mirrored boundary, the default, on a device tensor: the oracle along axis 0
    want = F.oracle_resample(x, 12, "sample", "mirror")
    got = baselines.fourier_resample(torch.from_numpy(x).cuda(), 12, axis=0)
    assert got.is_cuda and tuple(got.shape) == (12, 9, 10)
    assert np.abs(got.cpu().numpy() - want).max() <= F.bound(x, want)


def test_calls_are_bit_equal_and_a_skipped_axis_passes_its_data_through():
    x64 = torch.from_numpy(np.random.default_rng(7).standard_normal((5, 25, 19))).cuda()
    for x in (x64, x64.float()):
        a, b = baselines.fourier_resize(x, (50, 38)), baselines.fourier_resize(x, (50, 38))
        assert torch.equal(a, b)
        # both axes skipped: the input, bit for bit; one axis skipped: the other axis' result, untouched
        assert torch.equal(baselines.fourier_resize(x, (25, 19)), x)
        rows_only, cols_only = baselines.fourier_resize(x, (50, 19)), baselines.fourier_resize(x, (25, 38))
        for c in (0, 7, 18):             # a column alone (its 1 -> 1 axis passes through) goes through the same launch
            assert torch.equal(rows_only[..., c:c + 1], baselines.fourier_resize(x[..., c:c + 1].contiguous(), (50, 1))), c
        for r in (0, 11, 24):
            assert torch.equal(cols_only[..., r:r + 1, :], baselines.fourier_resize(x[..., r:r + 1, :].contiguous(), (1, 38))), r
        # with a window, or centred, the same shape is an operator and no longer a copy
        assert not torch.equal(baselines.fourier_resize(x, (25, 19), apodize=1.0), x)


def test_no_images_and_the_workspace_check_on_the_device_path():
    lib = _lib.lib()
    empty = baselines.fourier_resize(torch.empty((0, 8, 8), dtype=torch.float64, device="cuda"), (16, 16))
    assert tuple(empty.shape) == (0, 16, 16)
    assert baselines.fourier_resize(np.empty((2, 0, 8, 8)), (4, 4)).shape == (2, 0, 4, 4)
    x = torch.ones((2, 8, 8), dtype=torch.float64, device="cuda")
    out = torch.full((2, 16, 16), -1.0, dtype=torch.float64, device="cuda")
    need = lib.inr_fourier_resample_workspace_doubles(2, 8, 8, 16, 16)
    ws = torch.empty(need, dtype=torch.float64, device="cuda")
    args = (out.data_ptr(), x.data_ptr(), 2, 8, 8, 16, 16, _lib.INR_FOURIER_SAMPLE, _lib.INR_FOURIER_MIRROR, 0.0, ws.data_ptr())
    assert lib.inr_fourier_resample2d(*args, need - 1, ops._stream()) == _lib.INR_E_WORKSPACE
    assert torch.equal(out, torch.full_like(out, -1.0))                # refused before any device work
    assert lib.inr_fourier_resample2d(out.data_ptr(), x.data_ptr(), 0, *args[3:], need, ops._stream()) == 0
    assert torch.equal(out, torch.full_like(out, -1.0))                # n_images = 0 launches nothing
    _lib.check(lib.inr_fourier_resample2d(*args, need, ops._stream()))
    assert float((out - 1.0).abs().max()) <= 1e-13
    with pytest.raises(TypeError, match="fourier_resize: device tensors must be float32 or float64"):
        baselines.fourier_resize(x.half(), (16, 16))


@pytest.fixture(scope="module")
def zerofill_runs(tmp_path_factory, golden):
    """superresDWI on pat07 as test_superresDWI_entry_point_on_pat07 sets it up, with and without --zerofill."""
    tmp = tmp_path_factory.mktemp("zerofill")
    vol = golden("pat07_volume.npz")["vol"]
    path = str(tmp / "pat07_mean_b0.mat")
    matio.savemat(path, {"data_mean_b0": vol})
    common = ["--data", path, "--number_of_epochs", "20", "--seed", "0", "--roi_start", "40", "--roi_end", "90"]
    with_flag = dwi_script.main(common + ["--output_address", str(tmp / "zf"), "--zerofill"])[0]
    without = dwi_script.main(common + ["--output_address", str(tmp / "plain")])[0]
    return vol, os.path.join(str(tmp), "zf", "pat07"), with_flag, os.path.join(str(tmp), "plain", "pat07"), without


def test_superresDWI_zerofill_flag_on_pat07(zerofill_runs):
    vol, d, res, d_plain, res_plain = zerofill_runs
    rows = reports.read_csv(os.path.join(d, "ssim_scores.csv"))
    zrows = reports.read_csv(os.path.join(d, "ssim_scores_zerofill.csv"))
    assert open(os.path.join(d, "ssim_scores_zerofill.csv")).readline() == "Pt_id, b-value, slice, SSIM-zerofill, SSIM-SR\n"
    assert len(zrows) == len(rows) == 28 and set(zrows[0]) == {"Pt_id", "b-value", "slice", "SSIM-zerofill", "SSIM-SR"}
    for key in ("Pt_id", "b-value", "slice", "SSIM-SR"):
        assert [r[key] for r in zrows] == [r[key] for r in rows], key
    # the zero-fill column against a direct call: HR / max as the driver forms it, [Z, B, X, Y]
    hr = torch.from_numpy(np.ascontiguousarray((vol / vol.max())[40:90, 40:90], dtype=np.float32)).cuda()[..., None]
    hs = hr.permute(2, 3, 0, 1).contiguous()
    zf = baselines.fourier_resize(hs[:, :, ::2, ::2].contiguous(), (50, 50), "sample", "mirror", 0.0).clamp_min(0)
    floor = lambda t: t.clamp_min(1e-30)                 # the driver's guard for empty slices; pat07 has none
    want = np.array([float(v) for v in metrics.ssim_reference_protocol(floor(hs), floor(zf)).cpu().numpy()[:, 0]])
    col = np.array([float(r["SSIM-zerofill"]) for r in zrows])
    print(f"SSIM-zerofill: max|csv - direct| = {np.abs(col - want).max():.3e}; mean {col.mean():.4f}")
    assert np.array_equal(col, want)
    m = json.load(open(os.path.join(d, "metrics.json")))
    print(f"psnr_zerofill_db = {m['psnr_zerofill_db']:.2f}, psnr_spline_db = {m['psnr_spline_db']:.2f}")
    assert m["psnr_zerofill_db"] > m["psnr_spline_db"]
    assert m["psnr_zerofill_db"] == pytest.approx(float(metrics.psnr(hs, zf, 1.0))) == pytest.approx(res["psnr_zerofill_db"])
    assert m["ssim_zerofill_mean"] == pytest.approx(col.mean())
    # without the flag: the same ssim_scores.csv byte for byte, no zero-fill key, no zero-fill file
    assert open(os.path.join(d_plain, "ssim_scores.csv"), "rb").read() == open(os.path.join(d, "ssim_scores.csv"), "rb").read()
    plain = json.load(open(os.path.join(d_plain, "metrics.json")))
    assert not [k for k in list(plain) + list(res_plain) if "zerofill" in k]
    assert set(m) - set(plain) == {"psnr_zerofill_db", "ssim_zerofill_mean"}
    assert not [f for f in os.listdir(d_plain) if "zerofill" in f]
    assert sorted(os.listdir(d)) == sorted(os.listdir(d_plain) + ["ssim_scores_zerofill.csv"])


def test_superresDWI_zerofill_adds_its_adc_map(tmp_path):
    """--zerofill --adc on a plain four-b volume: adc_zerofill is the ADC of the x4 zero-fill of the LR ROI, on adc_spline's grid."""
    rng = np.random.default_rng(3)
    bvals = np.array([0.0, 150.0, 1000.0, 1500.0])
    gx, gy, gz = np.meshgrid(np.linspace(0, 1, 32), np.linspace(0, 1, 32), np.linspace(0, 1, 2), indexing="ij")
    vol = np.stack([500 * (1.2 + np.sin(3 * gx + gz) * np.cos(2 * gy)) * np.exp(-0.7 * b) for b in range(4)], axis=-1)
    vol *= 1 + 0.02 * rng.standard_normal(vol.shape)
    path = str(tmp_path / "pat068_vol.mat")
    matio.savemat(path, {"vol": vol, "b": bvals})
    out = str(tmp_path / "res")
    dwi_script.main(["--data", path, "--output_address", out, "--number_of_epochs", "5", "--hidden_dim", "128", "--num_layers", "2",
                     "--mapping_size", "32", "--roi_start", "2", "--roi_end", "30", "--seed", "0", "--adc", "--zerofill",
                     "--zerofill_apodize", "0.25"])
    adc = matio.loadmat(os.path.join(out, "pat068", "adc.mat"))
    assert set(adc) >= {"adc_sr", "adc_spline", "adc_hr", "adc_zerofill", "b"}
    assert adc["adc_zerofill"].shape == adc["adc_spline"].shape == (56, 56, 2)
    mean_img, _, _, _, scale = dwi_script.load_input_and_scale(path)
    hs = torch.from_numpy(np.ascontiguousarray(mean_img[2:30, 2:30], dtype=np.float32)).cuda().permute(2, 3, 0, 1).contiguous()
    zf = baselines.fourier_resize(hs[:, :, ::2, ::2].contiguous(), (56, 56), "sample", "mirror", 0.25).clamp_min(0)
    stack = (zf.permute(2, 3, 0, 1).contiguous() * torch.as_tensor(scale.astype(np.float32), device="cuda")).contiguous()
    want = metrics.calculate_ADC_device(bvals, stack).cpu().numpy()
    assert np.array_equal(adc["adc_zerofill"], want, equal_nan=True)
    # the signal falls as exp(-0.7 k) over the b indices k, whatever the interpolation
    want_adc = 0.7 * np.polyfit(bvals / 1000, np.arange(4.0), 1)[0]
    print(f"median adc_zerofill = {np.nanmedian(adc['adc_zerofill']):.4f}, adc_spline = {np.nanmedian(adc['adc_spline']):.4f}, want {want_adc:.4f}")
    assert abs(float(np.nanmedian(adc["adc_zerofill"])) - want_adc) < 0.02
