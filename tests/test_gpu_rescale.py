"""GPU: the skimage-style resize of csrc/rescale.hip (anti-aliased down-scaling, cubic, 'edge'), ``bicubic`` of the multi-image tree
and the low-resolution study against the scipy composition skimage 0.20 makes (tests/rescale_common.py).

The bound, max|got - want| <= 2e-7 max|in|, is the project's bound for the linear up-scale and is derived, not measured: fp64
arithmetic rounded once to fp32 errs by <= 6e-8 of the value.  Every test prints what it measured before it asserts."""
import csv
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

from tests import rescale_common as R
from mri_super_resolution_amd import _lib, baselines, ops

pytestmark = pytest.mark.gpu


def _report(what, got, want, scale):
    err = float(np.abs(np.asarray(got, dtype=np.float64) - want).max())
    print(f"{what}: max|got - want| = {err:.3e}, bound {R.BOUND * scale:.3e} (max|in| = {scale:.4g})")
    return err


@pytest.mark.parametrize("shape,scale,order,mode,aa", R.CASES, ids=R.CASE_IDS)
def test_resize_matches_the_scipy_composition(shape, scale, order, mode, aa):
    img = R.case_image(shape)
    out_hw = R.out_shape(shape, scale)
    want = R.scipy_resize(img, out_hw, order, mode, aa)
    got = baselines.rescale2d(img, scale, order=order, mode=mode, anti_aliasing=aa)
    assert got.dtype == np.float64 and got.shape == out_hw
    err = _report(f"rescale2d {shape} x{scale} order {order} {mode}", got, want, np.abs(img).max())
    assert err <= R.BOUND * np.abs(img).max()
    # resize to the same shape is the same call; anti_aliasing=None is on exactly when an axis shrinks
    same = baselines.resize(img, out_hw, order=order, mode=mode, anti_aliasing=None if aa == (scale < 1) else aa)
    assert np.array_equal(same, got)


@pytest.mark.parametrize("mode", ["reflect", "edge"])
def test_a_device_batch_is_resized_image_by_image(mode):
    x = torch.from_numpy(np.random.default_rng(2).random((3, 4, 10, 12)).astype(np.float32)).cuda()
    got = baselines.rescale2d(x, 0.5, mode=mode, anti_aliasing=True)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, 4, 5, 6)
    img = x[1, 2].cpu().numpy().astype(np.float64)
    want = R.scipy_resize(img, (5, 6), 1, mode, True)
    assert _report(f"batch image [1, 2] {mode}", got[1, 2].cpu().numpy(), want, np.abs(img).max()) <= R.BOUND * np.abs(img).max()
    # the cubic clips the batch as ONE group: every image to the range of all of them
    cubic = baselines.resize(x, (30, 36), order=3, mode=mode).cpu().numpy()
    lo, hi = float(x.min()), float(x.max())
    want = R.scipy_resize(img, (30, 36), 3, mode, False, clip_range=(lo, hi))
    assert _report(f"cubic batch image [1, 2] {mode}", cubic[1, 2], want, hi) <= R.BOUND * hi
    assert cubic.min() >= lo and cubic.max() <= hi


@pytest.fixture(scope="module")
def bicubic_case():
    X = np.random.default_rng(1).random((2, 16, 16, 9))
    free = np.stack([ndi.zoom(item, (3, 3, 1), order=3, mode="nearest", grid_mode=True) for item in X])   # skimage: channel factor 1
    return X, free


def test_bicubic_equals_the_clipped_scipy_result(bicubic_case):
    from mri_super_resolution_amd.compat.utils import preprocessing
    X, free = bicubic_case
    lo, hi = X.min(axis=(1, 2, 3), keepdims=True), X.max(axis=(1, 2, 3), keepdims=True)
    outside = float(np.mean((free < lo) | (free > hi)))
    print(f"unclipped cubic: {100 * outside:.2f} % of the pixels outside [min, max], values {free.min():.3f} .. {free.max():.3f}")
    assert outside >= 0.01                       # else the clip would pass untested
    want = np.clip(free, lo, hi)
    got = preprocessing.bicubic(X, scale=3)
    assert got.dtype == np.float64 and got.shape == (2, 48, 48, 9)
    assert _report("bicubic", got, want, np.abs(X).max()) <= R.BOUND * np.abs(X).max()
    # the clip is per item: an item scaled down is clipped to its own, narrower range; a single item takes the 3-D form
    Y = X.copy()
    Y[1] *= 0.25
    got2 = preprocessing.bicubic(Y)
    assert np.array_equal(got2[0], got[0]) and got2[1].max() <= Y[1].astype(np.float32).max() < got2[0].max()   # (fp32 on entry)
    assert np.array_equal(preprocessing.bicubic(X[0]), got[:1])
    with pytest.raises(ValueError, match="bicubic: X must be"):
        preprocessing.bicubic(X[0, 0])


def test_calls_are_bit_equal_and_rescale_is_what_it_was():
    x = torch.from_numpy(np.random.default_rng(3).random((5, 25, 19)).astype(np.float32)).cuda()
    for kw in ({"order": 1, "anti_aliasing": True}, {"order": 3, "mode": "edge", "anti_aliasing": True}):
        a, b = baselines.rescale2d(x, 0.5, **kw), baselines.rescale2d(x, 0.5, **kw)
        assert torch.equal(a, b)
    # baselines.rescale stays on inr_rescale2d_linear, bit for bit
    direct = torch.empty((5, 50, 38), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().inr_rescale2d_linear(direct.data_ptr(), x.data_ptr(), 5, 25, 19, 50, 38, ops._stream()))
    assert torch.equal(baselines.rescale(x, 2), direct)


def test_no_cpu_fallback_and_the_workspace_is_checked_on_the_device_path():
    with pytest.raises(ops.InrDeviceError):
        baselines.resize(torch.ones(8, 8), (4, 4))
    x = torch.ones((1, 8, 8), dtype=torch.float32, device="cuda")
    out = torch.empty((1, 4, 4), dtype=torch.float32, device="cuda")
    need = _lib.lib().inr_rescale2d_workspace_doubles(1, 8, 8, 3, 1)
    ws = torch.empty(need, dtype=torch.float64, device="cuda")
    rc = _lib.lib().inr_rescale2d(out.data_ptr(), x.data_ptr(), 1, 8, 8, 4, 4, 3, 1, 1, 1, ws.data_ptr(), need - 1, ops._stream())
    assert rc == _lib.INR_E_WORKSPACE
    _lib.check(_lib.lib().inr_rescale2d(out.data_ptr(), x.data_ptr(), 1, 8, 8, 4, 4, 3, 1, 1, 1, ws.data_ptr(), need, ops._stream()))
    assert torch.equal(out, torch.ones_like(out))                     # a constant image stays that constant, to the bit


def _synthetic_volume(seed=0, side=32, slices=2, K=4):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:side, 0:side]
    body = 0.2 + 0.6 * np.exp(-((yy - side / 2) ** 2 + (xx - side / 2) ** 2) / (side * side / 14.0))
    b0 = np.repeat((1.5 * body)[:, :, None], slices, axis=2)
    b3 = body[:, :, None, None] * (1 + 0.05 * rng.standard_normal((side, side, slices, K)))
    b3[side - 6:] = 0.01 * np.abs(rng.standard_normal((6, side, slices, K)))          # background: the low-signal branch
    return b0, b3


def test_low_res_study_on_a_synthetic_case():
    from mri_super_resolution_amd import drivers, erd_inr
    b0, b3 = _synthetic_volume()
    case = SimpleNamespace(pt_id="18-1681-07", b=(0, 300, 600, 900), cancer_loc=(15, 15), contralateral_loc=(15, 20), noise=(29, 16),
                           cancer_slice=1, b0=b0, b3=b3)
    torch.manual_seed(0)
    maps, label, info = drivers.low_res_study(case, 0, seed=5, hidden_features=64, max_steps=40)
    base, b0s = b3[:, :, 0, :].mean(-1), b0[:, :, 0]
    low = R.scipy_resize(base, (16, 16), 1, "reflect", True)
    b0_low = R.scipy_resize(b0s, (16, 16), 1, "reflect", True)
    assert np.array_equal(maps["base"], base)
    for name, got, want, scale in (("low", maps["low"], low, base.max()),
                                   ("interpolated", maps["interpolated"], R.scipy_resize(low, (32, 32), 1, "reflect", False), base.max()),
                                   ("b0_low", info["b0_low"], b0_low, b0s.max()),
                                   ("b0_up", info["b0_up"], R.scipy_resize(b0_low, (32, 32), 1, "reflect", False), b0s.max())):
        assert got.shape == want.shape
        assert _report(name, got, want, scale) <= R.BOUND * scale
    b = case.b[3]
    assert np.array_equal(maps["adc_low"], erd_inr.calc_adc(maps["low"], info["b0_low"], b))
    assert np.array_equal(maps["adc_interpolated"], erd_inr.calc_adc(maps["interpolated"], info["b0_up"], b))
    assert np.array_equal(maps["adc_gold"], erd_inr.calc_adc(base, b0s, b))
    assert maps["SR"].shape == (32, 32) and np.isfinite(maps["SR"]).all()
    assert np.array_equal(maps["adc_superres"], erd_inr.calc_adc(maps["SR"], info["b0_up"], b))
    assert sorted(maps) == sorted(["low", "interpolated", "SR", "base", "adc_low", "adc_interpolated", "adc_superres", "adc_gold"])
    assert label["pt"] == case.pt_id and label["image"] == "0"
    assert sorted(label[k] for k in "1234") == sorted(drivers.QUAL_PANELS)
    assert info["pretrain"]["steps"] <= 40 * 17 and np.isfinite(info["finetune_loss"])
    # the panel order is seeded: the same (seed, patient, slice) draws the same order
    assert label == drivers.low_res_study(case, 0, seed=5, hidden_features=64, max_steps=8, finetune_steps=1)[1]


def test_script_writes_labels_and_one_mat_per_slice(tmp_path):
    from mri_super_resolution_amd import matio
    from mri_super_resolution_amd.scripts import prepare_qual_images as S
    b0, b3 = _synthetic_volume(seed=1)
    d = tmp_path / "07" / "no_aver"
    d.mkdir(parents=True)
    matio.savemat(str(d / "bigImage.mat"), {"b0": b0, "b1": b3, "b2": b3, "b3": b3})
    cases = tmp_path / "cases.json"
    cases.write_text('[{"pt_id": "18-1681-07", "erc": 0, "cancer_loc": [15, 15], "contralateral_loc": [15, 20], '
                     '"noise": [29, 16], "cancer_slice": 1}]')
    out_dir = tmp_path / "qual"
    summary = S.main(["--data_dir", str(tmp_path), "--cases", str(cases), "--out_dir", str(out_dir), "--max_steps", "40"])
    rows = list(csv.reader(open(out_dir / "labels.csv")))
    assert rows[0] == ["file", "pt", "image", "1", "2", "3", "4"] and len(rows) == 3 == len(summary) + 1
    assert [r[0] for r in rows[1:]] == ["291", "292"] and sorted(r[2] for r in rows[1:]) == ["0", "1"]
    for r in rows[1:]:
        assert r[1] == "18-1681-07" and sorted(r[3:]) == sorted(["low", "interpolated", "SR", "base"])
        mat = matio.loadmat(str(out_dir / f"{r[0]}.mat"))
        npy = np.load(out_dir / f"{r[0]}.npy", allow_pickle=True).item()
        for key, shape in (("low", (16, 16)), ("interpolated", (32, 32)), ("SR", (32, 32)), ("base", (32, 32)), ("adc_low", (16, 16)),
                           ("adc_interpolated", (32, 32)), ("adc_superres", (32, 32)), ("adc_gold", (32, 32))):
            assert mat[key].shape == shape and np.array_equal(mat[key], npy[key])
    # --slices cancer: the one slice of the case table
    only = S.main(["--data_dir", str(tmp_path), "--cases", str(cases), "--out_dir", str(tmp_path / "q2"), "--max_steps", "8",
                   "--slices", "cancer"])
    assert [s["image"] for s in only] == ["1"] and os.path.exists(tmp_path / "q2" / "291.mat")
