"""-m gpu: the through-plane spline (baselines.resize_z = inr_resize_z_cubic) against scipy's interp1d(kind='cubic') and the
reference fixture, and the two optional superresDWI products built on the same fit: the coronal volumes
(--transverse_length) and the ADC maps (--adc)."""
import json
import os

import numpy as np
import pytest
import torch
from scipy.interpolate import interp1d

import mri_super_resolution_amd as inr
from mri_super_resolution_amd import baselines, matio, ops
from mri_super_resolution_amd._lib import InrHipError
from mri_super_resolution_amd.scripts import superresDWI as dwi_script

pytestmark = pytest.mark.gpu


def scipy_resize(arr, n_out):
    return interp1d(np.linspace(0, 1, arr.shape[-1]), arr, kind="cubic", axis=-1)(np.linspace(0, 1, n_out))


def test_resize_z_matches_the_reference_fixture(golden):
    h = golden("helpers.npz")
    got = baselines.resize_z(h["resize_in"], 9)
    assert got.dtype == np.float64 and got.shape == h["resize_out"].shape
    assert np.abs(got - h["resize_out"]).max() <= 1e-12


@pytest.mark.parametrize("n_in", [4, 5, 7, 24, 28, 34, 128])
def test_resize_z_matches_scipy(n_in):
    rng = np.random.default_rng(n_in)
    vol = rng.random((6, 5, n_in))                     # arr[X, Y, Z] as resize_array takes it
    lines = rng.random((300, n_in))                    # [lines, Z]: more than one 256-thread block
    for n_out in (1, 2, 9, 100, 257):
        got = baselines.resize_z(vol, n_out)
        assert got.shape == (6, 5, n_out) and got.dtype == np.float64
        assert np.abs(got - scipy_resize(vol, n_out)).max() <= 1e-12, n_out
        assert np.abs(baselines.resize_z(lines, n_out) - scipy_resize(lines, n_out)).max() <= 1e-12, n_out
        if n_out == 1:
            assert np.array_equal(got[..., 0], vol[..., 0])
    # a device tensor in, a float64 device tensor out, same values
    t = baselines.resize_z(torch.from_numpy(vol).cuda(), 100)
    assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (6, 5, 100)
    assert np.abs(t.cpu().numpy() - scipy_resize(vol, 100)).max() <= 1e-12


def test_resize_z_refusals():
    with pytest.raises(InrHipError, match="at least 4 samples"):
        baselines.resize_z(np.zeros((4, 3)), 9)
    with pytest.raises(ValueError):
        baselines.resize_z(np.zeros((4, 8)), 9, kind="linear")


# ---- the driver ---------------------------------------------------------------------------------------------------------
X = Y = 32
R0, R1 = 2, 30
R = R1 - R0
BVALS = np.array([0.0, 150.0, 1000.0, 1500.0])
NET = ["--number_of_epochs", "60", "--pertubation_epochs", "4", "--hidden_dim", "128", "--num_layers", "2", "--mapping_size",
       "32", "--roi_start", str(R0), "--roi_end", str(R1), "--seed", "0"]


def _hybrid_raw(tmp_path, Z):
    """The synthetic master.mat of test_superresDWI_hybrid_raw_input_runs_the_perturbnet_schedule, with Z slices and a signal
    that also varies along z."""
    rng = np.random.default_rng(2)
    nacq = (1, 2, 2, 2)
    gx, gy, gz = np.meshgrid(np.linspace(0, 1, X), np.linspace(0, 1, Y), np.linspace(0, 1, Z), indexing="ij")
    base = 100 * (1.2 + np.sin(3 * gx) * np.cos(2 * gy)) * (1 + 0.3 * np.sin(2.5 * gz))
    cell = np.empty((4, 4), dtype=object)
    for b in range(4):
        for te in range(4):
            shape = (X, Y, Z) if b == 0 else (X, Y, Z, nacq[b])
            sig = base * np.exp(-0.4 * b) * (1 - 0.1 * te)
            cell[b, te] = (sig if b == 0 else sig[..., None] * np.ones(nacq[b])) * (1 + 0.02 * rng.standard_normal(shape))
    path = str(tmp_path / "pat066_master.mat")
    matio.savemat(path, {"hybrid_raw": cell, "b": BVALS})
    return path


def _families(counts):
    return {k for k, v in counts.items() if v}


def test_superresDWI_coronal_and_adc_outputs(tmp_path):
    Z = 6
    path = _hybrid_raw(tmp_path, Z)
    out_on, out_off = str(tmp_path / "on"), str(tmp_path / "off")
    res = dwi_script.main(["--data", path, "--pt_id", "66", "--output_address", out_on, *NET, "--transverse_length", str(Z),
                           "--adc"])[0]
    d = os.path.join(out_on, "pat66")
    rec = matio.loadmat(os.path.join(d, "recon.mat"))
    cor = matio.loadmat(os.path.join(d, "coronal.mat"))
    recon, maxes = rec["recon"], rec["maxes"]
    assert recon.shape == (2 * R, 2 * R, Z, 4)
    assert cor["coronal_sr"].shape == (2 * R, 2 * R, Z) and cor["coronal_spline"].shape == (R, R, Z)
    assert int(np.asarray(cor["transverse_length"]).reshape(-1)[0]) == Z
    assert np.array_equal(np.load(os.path.join(d, "coronal.npy")), cor["coronal_sr"])
    assert res["t_coronal_s"] > 0 and json.load(open(os.path.join(d, "metrics.json")))["t_coronal_s"] == res["t_coronal_s"]

    # T == Z: the coronal grid's points are the in-plane test grid's points at b index 0 (linspace(-1, 1, 1) == [-1]).  Whether
    # the two reconstructions run the same kernel families is read from the launch counters on a network of the same shape.
    # For this network they do not: the 75,264-row test grid runs hp_pkc + hp_tile, the 18,816-row coronal grid hp_narrow, so
    # the 2e-6 bound is what holds (the two happen to agree bit for bit as well, but nothing promises that across families).
    net = inr.Siren(in_features=64, out_features=1, hidden_features=128, hidden_layers=2).cuda()
    Bt = torch.randn(32, 4, device="cuda") * 0.5
    fam = []
    for shape, clamp in (((2 * R, 2 * R, Z, 4), 0.0), ((2 * R, 2 * R, Z, 1), None)):
        ops.launch_counts_reset()
        inr.reconstruct(net, shape, Bt, clamp_min=clamp)
        torch.cuda.synchronize()
        fam.append(_families(ops.launch_counts()))
    sr0 = np.maximum(cor["coronal_sr"], 0)
    assert np.abs(sr0 - recon[..., 0]).max() <= 2e-6
    if fam[0] == fam[1]:          # same kernels, rows are independent: the same bits
        assert np.array_equal(sr0, recon[..., 0]), fam

    mean_img, _, _, maxes_in, scale = dwi_script.load_input_and_scale(path)
    assert np.array_equal(maxes_in, maxes) and np.array_equal(scale, maxes[:, 1])
    want_spline = inr.resize_array(mean_img[R0:R1, R0:R1, :, 0], Z)             # the host function (scipy)
    assert np.abs(cor["coronal_spline"] - want_spline).max() <= 1e-12
    # with T == Z the spline reproduces the slices it interpolates
    assert np.abs(cor["coronal_spline"] - mean_img[R0:R1, R0:R1, :, 0]).max() <= 1e-12

    # ADC maps: host calculate_ADC of the same fp32 stacks, each b-image times maxes[b, 1]
    adc = matio.loadmat(os.path.join(d, "adc.mat"))
    s32 = maxes[:, 1].astype(np.float32)
    hr = np.ascontiguousarray(mean_img[R0:R1, R0:R1].transpose(2, 3, 0, 1))    # [Z, B, R, R], as the driver stacks it
    to_xyzb = lambda a: np.ascontiguousarray(a.astype(np.float32).transpose(2, 3, 0, 1))
    stacks = {"adc_sr": recon.astype(np.float32), "adc_spline": to_xyzb(baselines.rescale(hr[:, :, ::2, ::2], 4)),
              "adc_hr": to_xyzb(baselines.rescale(hr, 2))}
    for k, st in stacks.items():
        want = inr.calculate_ADC(BVALS, (st * s32).astype(np.float32))
        assert adc[k].shape == (2 * R, 2 * R, Z), k
        assert np.allclose(adc[k], want, rtol=2e-6, atol=2e-6), (k, np.abs(adc[k] - want).max())
    assert np.array_equal(np.asarray(adc["b"]).reshape(-1), BVALS)
    assert adc["adc_hr"].std() > 0 and np.isfinite(adc["adc_sr"]).all()

    # without the flags: no new files, recon.mat with today's keys, and the same fit and volumes bit for bit
    dwi_script.main(["--data", path, "--pt_id", "66", "--output_address", out_off, *NET])
    d0 = os.path.join(out_off, "pat66")
    assert sorted(os.listdir(d0)) == ["metrics.json", "recon.mat", "recon.npy", "ssim_scores.csv"]
    rec0 = matio.loadmat(os.path.join(d0, "recon.mat"))
    assert sorted(rec0) == sorted(rec) == ["SR_recon", "b", "maxes", "recon"]
    assert "t_coronal_s" not in json.load(open(os.path.join(d0, "metrics.json")))
    for k in rec0:
        assert np.array_equal(rec0[k], rec[k]), k


def test_superresDWI_transverse_length_100_on_a_plain_volume(tmp_path):
    """The reference's T = 100 on a plain [X, Y, Z, B] volume; --adc there rescales by the per-b maxima the volume was divided
    by."""
    Z = 5
    rng = np.random.default_rng(3)
    gx, gy, gz = np.meshgrid(np.linspace(0, 1, X), np.linspace(0, 1, Y), np.linspace(0, 1, Z), indexing="ij")
    vol = np.stack([500 * (1.2 + np.sin(3 * gx + gz) * np.cos(2 * gy)) * np.exp(-0.7 * b) for b in range(4)], axis=-1)
    vol *= 1 + 0.02 * rng.standard_normal(vol.shape)
    path = str(tmp_path / "pat067_vol.mat")
    matio.savemat(path, {"vol": vol, "b": BVALS})
    out = str(tmp_path / "res")
    dwi_script.main(["--data", path, "--output_address", out, *NET, "--transverse_length", "100", "--adc"])
    d = os.path.join(out, "pat067")
    cor = matio.loadmat(os.path.join(d, "coronal.mat"))
    assert cor["coronal_sr"].shape == (2 * R, 2 * R, 100) and cor["coronal_spline"].shape == (R, R, 100)
    assert np.isfinite(cor["coronal_sr"]).all() and np.isfinite(cor["coronal_spline"]).all()
    mean_img = dwi_script.load_input(path)[0]
    assert np.abs(cor["coronal_spline"] - inr.resize_array(mean_img[R0:R1, R0:R1, :, 0], 100)).max() <= 1e-12
    adc = matio.loadmat(os.path.join(d, "adc.mat"))
    rec = matio.loadmat(os.path.join(d, "recon.mat"))
    s32 = vol.reshape(-1, 4).max(axis=0).astype(np.float32)
    want = inr.calculate_ADC(BVALS, (rec["recon"].astype(np.float32) * s32).astype(np.float32))
    assert np.allclose(adc["adc_sr"], want, rtol=2e-6, atol=2e-6)
    # the signal falls as exp(-0.7 k) over the b indices k: the HR ROI's ADC is 0.7 times the slope of k against b / 1000
    want_hr = 0.7 * np.polyfit(BVALS / 1000, np.arange(4.0), 1)[0]
    assert abs(float(np.median(adc["adc_hr"])) - want_hr) < 0.02
