"""-m gpu: the shift-tolerant SSIM kernels (csrc/cssim.hip) against the float64 restatement of utils/loss.py:131-177
(tests/cssim_common.py; TensorFlow absent -- the restatement is pinned to analytic cases in test_cssim_cpu.py), the gradient
against torch autograd on it, and the Python / script surface."""
import json
import os

import numpy as np
import pytest
import torch

from mri_super_resolution_amd import matio, rams
from oracle import rams_port as R
from tests import cssim_common as S

pytestmark = pytest.mark.gpu

RTOL = 1e-9          # what cL1 and cPSNR are held to: fp64 accumulations of fp32 inputs


def _check_values(y_true, y_pred, mask, size):
    for clear_only in (False, True):
        want_table = S.cssim_table(y_true, y_pred, mask, size, clear_only)
        want = want_table.reshape(len(y_true), -1).max(axis=1)
        got, table = rams.ssim_per_image(y_true, y_pred, mask, size_image=size, clear_only=clear_only, return_table=True)
        got, table = got.cpu().numpy(), table.cpu().numpy()
        print(f"size {size} clear_only {clear_only}: max rel err per image {np.abs(got / want - 1).max():.3e}, "
              f"table {np.abs(table / want_table - 1).max():.3e}")
        assert got.dtype == np.float64 and np.allclose(got, want, rtol=RTOL, atol=0)
        assert np.allclose(table, want_table, rtol=RTOL, atol=0)
        again, table2 = rams.ssim_per_image(y_true, y_pred, mask, size_image=size, clear_only=clear_only, return_table=True)
        assert np.array_equal(again.cpu().numpy(), got) and np.array_equal(table2.cpu().numpy(), table)     # bit-equal


@pytest.mark.parametrize("size,soft_mask", [(40, False), (60, False), (60, True)])
def test_values_and_shift_table_match_the_float64_restatement(size, soft_mask):
    y_true, y_pred, mask = S.planted_case(7 + size, 3, size, soft_mask=soft_mask)
    assert 0.10 < 1.0 - (mask > 0).mean() < 0.20
    _check_values(y_true, y_pred, mask, size)
    # the prediction is the label rolled by (1, -2), so pred[u, v] = label[u - 1, v + 2] and the label window that lines up with
    # the crop starts at (border - 1, border + 2) = (2, 5): that shift is the best one, far ahead of the others (the label is
    # white noise, so every other shift compares unrelated pixels)
    table = S.cssim_table(y_true, y_pred, mask, size).reshape(3, 49)
    ranked = np.sort(table, axis=1)
    assert (table.argmax(axis=1) == 7 * 2 + 5).all() and (ranked[:, -1] - ranked[:, -2] > 0.1).all()
    if not soft_mask:
        # 3 % gain and noise of 30 against constants built on 65535; with a soft mask x = P M^2 + b M is no scaled copy of
        # y = L M, so no such figure holds there
        assert (ranked[:, -1] > 0.99).all()


def test_values_at_the_production_size():
    y_true, y_pred, mask = S.planted_case(21, 2, 384)
    _check_values(y_true, y_pred, mask, 384)


@pytest.mark.parametrize("clear_only", [False, True])
def test_gradient_matches_autograd_on_the_restatement(clear_only):
    B, size = 3, 40
    y_true, y_pred, mask = S.planted_case(11, B, size, roll=(-1, 2), gain=1.02, offset=-90.0, noise=40.0, masked=0.2,
                                          soft_mask=clear_only)
    up = np.array([1.0, 0.5, 2.0], np.float32)
    # precondition, on the restatement: the arg-max over the shifts is unambiguous
    ranked = np.sort(S.cssim_table(y_true, y_pred, mask, size, clear_only).reshape(B, 49), axis=1)
    assert (ranked[:, -1] - ranked[:, -2] > 1e-6).all()

    yp = torch.from_numpy(y_pred).double().requires_grad_(True)
    want_loss = S.cssim_loss_torch(torch.from_numpy(y_true), yp, torch.from_numpy(mask), size, clear_only)
    (want_loss * torch.from_numpy(up).double()).sum().backward()
    w = yp.grad.numpy()

    loss, grad = rams.ssim_loss_and_grad(y_true, y_pred, mask, HR_SIZE=size, upstream=up, clear_only=clear_only)
    g = grad.cpu().numpy().astype(np.float64)
    print(f"clear_only {clear_only}: loss rel err {np.abs(loss.cpu().numpy() / want_loss.detach().numpy() - 1).max():.3e}, "
          f"grad max err / max {np.abs(g - w).max() / np.abs(w).max():.3e}")
    assert np.allclose(loss.cpu().numpy(), want_loss.detach().numpy(), rtol=RTOL, atol=0)
    assert np.abs(w).max() > 0 and np.abs(g - w).max() <= 1e-6 * np.abs(w).max()
    frame = np.ones((size, size), bool)
    frame[3:-3, 3:-3] = False
    assert np.count_nonzero(g[:, frame]) == 0 and np.count_nonzero(w[:, frame]) == 0     # nothing on the border frame
    # without upstream: the gradient of sum_b loss[b]; upstream scales linearly
    loss1, grad1 = rams.ssim_loss_and_grad(y_true, y_pred, mask, HR_SIZE=size, clear_only=clear_only)
    g1 = grad1.cpu().numpy().astype(np.float64)
    assert torch.equal(loss1, loss)
    yp.grad = None
    S.cssim_loss_torch(torch.from_numpy(y_true), yp, torch.from_numpy(mask), size, clear_only).sum().backward()
    w1 = yp.grad.numpy()
    assert np.abs(g1 - w1).max() <= 1e-6 * np.abs(w1).max()
    for b in range(B):
        assert np.allclose(g1[b] * float(up[b]), g[b], rtol=1e-6, atol=1e-9 * np.abs(g[b]).max())
    # the loss is the forward entry point's value
    per = rams.ssim_per_image(y_true, y_pred, mask, size_image=size, clear_only=clear_only)
    assert torch.equal(1.0 - per, loss)
    again = rams.ssim_loss_and_grad(y_true, y_pred, mask, HR_SIZE=size, upstream=up, clear_only=clear_only)
    assert torch.equal(again[0], loss) and torch.equal(again[1], grad)


def test_ssim_is_the_batch_mean_and_accepts_channel_last_inputs():
    y_true, y_pred, mask = S.planted_case(13, 3, 40)
    per = rams.ssim_per_image(y_true, y_pred, mask, size_image=40)
    got = rams.ssim(y_true[..., None], y_pred[..., None], mask[..., None], size_image=40)
    assert got.dtype == torch.float64 and got.item() == per.mean().item()
    assert rams.ssim(y_true, y_pred, mask, size_image=40, clear_only=True).item() == \
        rams.ssim_per_image(y_true, y_pred, mask, size_image=40, clear_only=True).mean().item()
    with pytest.raises(ValueError):
        rams.ssim(y_true, y_pred, mask, size_image=48)


def test_trainer_test_step_returns_the_pair_by_default_and_the_triple_on_request():
    rng = np.random.default_rng(5)
    side = 16
    x = (rng.random((2, side, side, 9)) * 20000 + 2000).astype(np.float32)
    hr = (rng.random((2, 3 * side, 3 * side)) * 20000 + 2000).astype(np.float32)
    mask = (rng.random((2, 3 * side, 3 * side)) > 0.1).astype(np.float32)
    params = R.init_rams_params(seed=6, perturb_g=True, N=1)
    tr = rams.RamsTrainer(rams.RAMS(3, 32, 3, 9, 8, 1, params=params))
    pair = tr.test_step(x, hr, mask)
    triple = tr.test_step(x, hr, mask, with_ssim=True)
    assert len(pair) == 2 and len(triple) == 3
    assert torch.equal(pair[0], triple[0]) and torch.equal(pair[1], triple[1])
    sr = tr.sync_model().forward(x)
    assert triple[2].item() == rams.ssim(hr, sr, mask, size_image=3 * side).item()
    want = S.cssim_per_image(hr, sr.cpu().numpy().reshape(2, 3 * side, 3 * side), mask, 3 * side).mean()
    assert triple[2].item() == pytest.approx(want, rel=RTOL)


def test_rams_master_ssim_flag(tmp_path):
    """`--ssim` adds `cssim_vs_rescaled` to the case record, the JSON file and nothing else; without it the record has the keys
    it always had and the written images are the same bytes."""
    from mri_super_resolution_amd import baselines
    from mri_super_resolution_amd.scripts import rams_master
    rng = np.random.default_rng(8)
    n = 20
    gx, gy = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n), indexing="ij")
    base = 60.0 + 50.0 * np.sin(5 * gx) * np.cos(4 * gy)
    Z, T = 2, 10
    dwi = np.stack([np.stack([base * (1 + 0.1 * z) * (1 + 0.04 * rng.standard_normal(base.shape)) for _ in range(T)], axis=-1)
                    for z in range(Z)], axis=2).clip(1, 250).astype(np.float32)
    b0 = np.stack([2.5 * base * (1 + 0.1 * z) for z in range(Z)], axis=2).astype(np.float32)
    data_dir = tmp_path / "anon_data"
    data_dir.mkdir()
    matio.savemat(str(data_dir / "pat09_alldata.mat"), {"data": dwi})
    matio.savemat(str(data_dir / "pat09_mean_b0.mat"), {"data_mean_b0": b0})
    spec = [{"pt_id": "18-1681-09", "b": 900, "cancer_loc": [10, 12], "contralateral_loc": [10, 8], "noise": [3, 3],
             "cancer_slice": 1, "acquisitions": [3, 3, 4]}]
    with open(str(tmp_path / "cases.json"), "w") as fh:
        json.dump(spec, fh)
    weights = rams.RAMS(3, 32, 3, 9, 8, 12, params=R.init_rams_params(seed=4, perturb_g=True)).save_weights(str(tmp_path / "w.npz"))

    def run(tag, *extra):
        argv = ["--out_folder", str(tmp_path / tag / "exp"), "--out_img_folder", str(tmp_path / tag / "img"), "--exp_name", "mi1",
                "--data_dir", str(data_dir), "--cases", str(tmp_path / "cases.json"), "--weights", weights, "--sample_size", "2",
                "--seed", "3", *extra]
        rec, = rams_master.main(argv)["cases"]
        with open(str(tmp_path / tag / "exp" / "mi1.json")) as fh:
            written, = json.load(fh)["cases"]
        return rec, written

    plain, plain_json = run("plain")
    flagged, flagged_json = run("flag", "--ssim")
    parent_keys = ["patient", "shape", "sample_size", "seconds", "subsets", "out_dir"]
    assert list(plain) == parent_keys == list(plain_json)
    assert list(flagged) == parent_keys + ["cssim_vs_rescaled"] == list(flagged_json)
    for k in ("patient", "shape", "sample_size", "subsets"):
        assert plain[k] == flagged[k] == plain_json[k]
    for name in ("DWI_mean.npy", "ADC_mean.npy", "images.mat"):
        with open(os.path.join(plain["out_dir"], name), "rb") as a, open(os.path.join(flagged["out_dir"], name), "rb") as b:
            assert a.read() == b.read(), name
    # the figure itself: cSSIM of the mean prediction against the rescaled acquisition mean, all pixels clear
    mean = np.load(os.path.join(flagged["out_dir"], "DWI_mean.npy"))
    lor = dwi[:, :, 1, :].astype("uint16") * 256
    ref = baselines.rescale(lor.astype(np.float64).mean(axis=-1), 3, anti_aliasing=False)
    want = S.cssim_per_image(ref.astype(np.float32)[None], mean.astype(np.float32)[None], np.ones((1, 60, 60)), 60)[0]
    assert flagged["cssim_vs_rescaled"] == flagged_json["cssim_vs_rescaled"] == pytest.approx(want, rel=RTOL)
    assert -1.0 <= flagged["cssim_vs_rescaled"] <= 1.0
