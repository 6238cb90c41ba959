"""-m gpu: the registration kernels (csrc/register.hip) against the float64 definition and scipy.ndimage.shift
(tests/register_common.py), the preparation chain against its NumPy restatement, and ``rams_master --register``."""
import json
import os

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

from mri_super_resolution_amd import matio, ops, rams, registration
from oracle import rams_port as R
from tests import register_common as G

pytestmark = pytest.mark.gpu


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


# ---- the correlation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,planted", G.CASES, ids=G.CASE_IDS)
def test_maps_and_shifts_match_the_definition(shape, planted):
    """One call of two sets of three images.  Per image max|C - oracle| <= max(100 y, 4 N 2^-53 kappa) over EVERY entry (y: the
    float64 FFT-against-direct difference of that image, N = H W), and the shift equals the oracle's exactly.
    Measured on an MI355X (max|C - oracle| / bound): see DESIGN.md 4i."""
    planes, masks, ref_index, want_shift = G.make_sets(shape, planted)
    args = (_dev(planes), _dev(masks), _dev(ref_index, torch.int32), G.window(shape), G.OVERLAP)
    shifts, peak, n_max, cmap = registration._xcorr(*args, want_map=True)
    shifts2, peak2, n_max2, cmap2 = registration._xcorr(*args, want_map=True)
    assert torch.equal(shifts, shifts2) and torch.equal(peak, peak2) and torch.equal(n_max, n_max2) and torch.equal(cmap, cmap2)
    shifts, peak, n_max, cmap = (t.cpu().numpy() for t in (shifts, peak, n_max, cmap))
    assert cmap.shape == (2, 3, 2 * shape[0] - 1, 2 * shape[1] - 1) and cmap.dtype == np.float64
    worst = 0.0
    for s in range(2):
        for t in range(3):
            st = G.case_stats(planes[s, ref_index[s]], planes[s, t], masks[s, t])
            # conditions on the inputs (tests/test_register_cpu.py holds the table's four to the same ones)
            assert st["count"] == 1 and st["peak"] - st["second"] >= 0.05 and st["kappa"] <= 100 and not st["near_tol"]
            bound = G.map_bound(st, shape[0] * shape[1])
            err = np.abs(cmap[s, t] - st["C"]).max()
            worst = max(worst, err / bound)
            print(f"{shape} set {s} image {t}: shift {shifts[s, t]} max|C - oracle| {err:.3e} bound {bound:.3e} "
                  f"(y {st['fft_diff']:.2e}, kappa {st['kappa']:.1f})")
            assert err <= bound
            assert tuple(shifts[s, t]) == tuple(st["shift"]) == tuple(want_shift[s, t])
            assert peak[s, t] == cmap[s, t].max() and n_max[s, t] == 1
    print(f"{shape}: worst max|C - oracle| / bound {worst:.3f}")


def test_a_window_restricts_the_displacements_and_takes_its_own_maxima():
    ref, x, m = G.make_case(*G.CASES[2])                                     # 33 x 31, planted (5, 6): outside the window in x
    st = G.case_stats(ref, x, m, max_shift=5)
    assert st["count"] == 1 and not st["near_tol"]
    got = registration.masked_xcorr(ref, x, m, max_shift=5)
    bound = G.map_bound(st, ref.size)
    print(f"window 5: max|C - oracle| {np.abs(got - st['C']).max():.3e} bound {bound:.3e}")
    assert got.shape == (11, 11) and np.abs(got - st["C"]).max() <= bound
    s = registration.masked_register_translation(ref, x, m, max_shift=5)
    assert s.dtype == np.float64 and tuple(s) == tuple(st["shift"])
    # a window wider than the image is the full search
    assert np.array_equal(registration.masked_xcorr(ref, x, m, max_shift=99), registration.masked_xcorr(ref, x, m))
    # device tensors in, device tensors out
    s_dev = registration.masked_register_translation(_dev(ref), _dev(x), _dev(m), max_shift=5)
    assert s_dev.is_cuda and s_dev.dtype == torch.float64 and tuple(s_dev.cpu().numpy()) == tuple(s)


def test_an_all_zero_mask_gives_a_zero_map_and_the_centre():
    ref, x, m = G.make_case(*G.CASES[0])
    zero = np.zeros_like(m)
    C = registration.masked_xcorr(ref, x, zero)
    assert C.shape == (47, 39) and not C.any()
    assert tuple(registration.masked_register_translation(ref, x, zero)) == (0.0, 0.0)
    shifts, peak, n_max, _ = registration._xcorr(_dev(np.array([[ref, x]])), _dev(np.zeros((1, 2) + ref.shape)),
                                                 torch.zeros(1, dtype=torch.int32, device="cuda"), G.window(ref.shape), G.OVERLAP)
    assert not shifts.cpu().numpy().any() and not peak.cpu().numpy().any() and n_max.cpu().tolist() == [[47 * 39, 47 * 39]]


# ---- the shift -----------------------------------------------------------------------------------------------------------------------
SHIFTS = [(1.3, -2.6), (-0.5, 0.5), (2, -3), (0, 0), (40.25, -3)]           # the last one is larger than every image below
CVAL = 0.25


@pytest.mark.parametrize("mode", ["reflect", "constant"])
@pytest.mark.parametrize("shape", [(9, 11), (24, 20), (33, 31)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shift_matches_scipy(shape, mode):
    img = G.f32(1.0 + np.random.default_rng(shape[0]).random(shape))
    stack = np.stack([img] * len(SHIFTS))
    got_all = registration.shift(stack, np.asarray(SHIFTS), mode=mode, cval=CVAL)          # one call, a shift per image
    for k, s in enumerate(SHIFTS):
        want = ndi.shift(img, s, mode=mode, cval=CVAL)
        got = registration.shift(img, s, mode=mode, cval=CVAL)
        err = np.abs(got - want).max()
        print(f"{shape} {mode} shift {s}: max|got - want| {err:.3e} bound {G.SHIFT_BOUND * np.abs(img).max():.3e}")
        assert got.dtype == np.float64 and got.shape == shape
        assert err <= G.SHIFT_BOUND * np.abs(img).max()
        if mode == "constant":
            assert np.array_equal(got == CVAL, want == CVAL)                 # cval exactly, and where scipy has it
            if k == 4:
                assert (got == CVAL).all()
            if shape == (9, 11) and k == 0:
                assert (got[:2] == CVAL).all() and (got[:, 8:] == CVAL).all() and not (got[2:, :8] == CVAL).any()
        assert np.array_equal(got_all[k], got)                               # per-image shifts: bit-equal to the calls one by one
    t = registration.shift(_dev(img), (1.3, -2.6), mode=mode, cval=CVAL)
    assert t.is_cuda and t.dtype == torch.float32
    assert np.array_equal(t.cpu().numpy().astype(np.float64), registration.shift(img, (1.3, -2.6), mode=mode, cval=CVAL))
    dev_shifts = registration.shift(_dev(stack), _dev(np.asarray(SHIFTS), torch.float64), mode=mode, cval=CVAL)
    assert np.array_equal(dev_shifts.cpu().numpy().astype(np.float64), got_all)


# ---- register_imgset / register_dataset ------------------------------------------------------------------------------------------------
def test_register_imgset_is_the_oracle_followed_by_scipy_shift():
    imgs, masks, planted = G.make_imgset()
    want, want_m, want_s, best = G.scipy_register_imgset(imgs, masks)
    assert best == 3 and np.array_equal(want_s, planted - planted[best])
    reg, reg_m, shifts = registration.register_imgset(imgs, masks, return_shifts=True)
    assert reg.dtype == reg_m.dtype == shifts.dtype == np.float64 and reg.shape == imgs.shape and shifts.shape == (5, 2)
    assert np.array_equal(shifts, want_s)
    err, err_m = np.abs(reg - want).max(), np.abs(reg_m - want_m).max()
    print(f"register_imgset: images max|got - want| {err:.3e} (bound {G.SHIFT_BOUND * np.abs(imgs).max():.3e}), masks {err_m:.3e} "
          f"(bound {G.SHIFT_BOUND:.1e})")
    assert err <= G.SHIFT_BOUND * np.abs(imgs).max() and err_m <= G.SHIFT_BOUND
    rows, cols = np.arange(24)[:, None], np.arange(20)[None, :]
    for t, (sy, sx) in enumerate(want_s):                                    # what the 'constant' shift pushed in is exactly 0
        pushed = (rows - sy < 0) | (rows - sy > 23) | (cols - sx < 0) | (cols - sx > 19)
        assert pushed.any() == bool(sy or sx) and not reg_m[..., t][pushed].any() and not want_m[..., t][pushed].any()
    # the reference image is itself, shifted by (0, 0)
    assert np.array_equal(reg[..., best], registration.shift(imgs[..., best], (0, 0), mode="reflect"))
    assert np.abs(reg[..., best] - imgs[..., best]).max() <= G.SHIFT_BOUND * np.abs(imgs).max()
    # registration did its job: every image now lies on the reference far better than before
    inner = (slice(4, -4), slice(4, -4))
    for t in range(5):
        if t != best:
            assert np.abs(reg[..., t] - imgs[..., best])[inner].max() < 0.25 * np.abs(imgs[..., t] - imgs[..., best])[inner].max()
    again = registration.register_imgset(imgs, masks, return_shifts=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, (reg, reg_m, shifts)))
    pair = registration.register_imgset(imgs, masks)
    assert len(pair) == 2 and np.array_equal(pair[0], reg)
    # device tensors: fp32 device tensors out, the same bits
    d_reg, d_m, d_s = registration.register_imgset(_dev(imgs), _dev(masks), return_shifts=True)
    assert d_reg.is_cuda and d_reg.dtype == torch.float32 and d_s.dtype == torch.float64
    assert np.array_equal(d_reg.cpu().numpy().astype(np.float64), reg) and np.array_equal(d_m.cpu().numpy().astype(np.float64), reg_m)
    # a window that holds the planted shifts gives the same registration
    assert np.array_equal(registration.register_imgset(imgs, masks, max_shift=4, return_shifts=True)[2], want_s)


def test_register_dataset_groups_sets_by_shape():
    a, ma, _ = G.make_imgset(seed=4)
    b, mb, _ = G.make_imgset(seed=5)
    c, mc, _ = G.make_imgset(shape=(17, 23), shifts=((0, 0), (2, 1), (-1, -2)), seed=6)
    X_reg, M_reg, shifts = registration.register_dataset([a, c, b], [ma, mc, mb], return_shifts=True)
    assert [x.shape for x in X_reg] == [a.shape, c.shape, b.shape]
    for k, (x, m) in enumerate([(a, ma), (c, mc), (b, mb)]):
        one = registration.register_imgset(x, m, return_shifts=True)
        assert np.array_equal(X_reg[k], one[0]) and np.array_equal(M_reg[k], one[1]) and np.array_equal(shifts[k], one[2])
    assert np.array_equal(shifts[1], G.scipy_register_imgset(c, mc)[2])
    assert len(registration.register_dataset([a], [ma])) == 2


# ---- the preparation chain ---------------------------------------------------------------------------------------------------------------
def test_preparation_chain_equals_the_numpy_restatement():
    rng = np.random.default_rng(12)
    X = [rng.integers(0, 16000, (16, 16, 11)).astype(np.uint16) for _ in range(2)]
    masks = []
    for i in range(2):
        m = np.ones((16, 16, 11), dtype=bool)
        for t, cleared in enumerate((0, 60, 5, 45, 10, 70, 15, 30, 20, 50, 25)):   # distinct clearances, four below the threshold
            flat = np.ones(256, dtype=bool)
            flat[:cleared + i] = False
            m[..., t] = flat.reshape(16, 16)
        masks.append(m)
    clear = registration.clearances(masks)
    for i in range(2):
        want = np.mean(masks[i], axis=(0, 1))
        assert len(set(want)) == 11 and np.array_equal(clear[i], want)       # 0 / 1 sums are exact in any order
    y = rng.random((2, 48, 48, 1))
    ym = (rng.random((2, 48, 48, 1)) > 0.1)

    def chain(select, gen_sub, augment):
        np.random.seed(21)
        sel, removed = select(X, masks, T=9, thr=0.85)
        sub = gen_sub(sel, 8, 4)
        y_sub, m_sub = gen_sub(y, 24, 12), gen_sub(ym.astype(np.float64), 24, 12)
        return (sel, removed, sub) + tuple(augment(sub, y_sub, m_sub, 3))

    got = chain(registration.select_T_images, lambda a, d, s: registration.gen_sub(a, d, s, verbose=False), registration.augment_dataset)
    want = chain(G.select_restated, G.gen_sub_restated, G.augment_restated)
    assert got[1] == want[1] == []
    assert got[0].shape == (2, 16, 16, 9) and got[0].dtype == np.uint16 and (np.mean(masks[0], axis=(0, 1)) <= 0.85).sum() == 4
    assert got[2].shape == (18, 8, 8, 9) and got[3].shape == (54, 8, 8, 9) and got[4].shape == got[5].shape == (54, 24, 24, 1)
    for g, w in zip(got, want):
        if not isinstance(g, list):
            assert g.shape == w.shape and np.array_equal(g, w)
    assert got[3].dtype == got[4].dtype == np.float64
    # one item: sub_images and augment_imgset
    assert np.array_equal(registration.sub_images(got[0][1].astype(np.float64), 8, 4, 3), want[2][9:])
    np.random.seed(3)
    Xa, ya, ma = registration.augment_imgset(want[2][0], y[0], ym[0], 4)
    np.random.seed(3)
    perms = [np.arange(9)] + [np.random.permutation(9) for _ in range(3)]
    assert np.array_equal(Xa, np.stack([want[2][0][..., p] for p in perms])) and ya.shape == (4, 48, 48, 1) and ma.dtype == bool
    # a set with no clear image is removed, or keeps its best image T times
    dark = [X[0], X[1]], [masks[0], np.zeros_like(masks[1])]
    sel, removed = registration.select_T_images(*dark, T=9)
    assert removed == [1] and sel.shape == (1, 16, 16, 9)
    dark[1][1][:2, :, 6] = True
    sel, removed = registration.select_T_images(*dark, T=9, remove_bad=False)
    assert removed == [] and np.array_equal(sel[1], np.repeat(X[1][..., 6:7], 9, axis=-1))
    # device tensors stay on the device
    t = registration.gen_sub(_dev(got[0].astype(np.float32)), 8, 4, verbose=False)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), want[2])


# ---- rams_master --register --------------------------------------------------------------------------------------------------------------
def test_rams_master_register_flag(tmp_path):
    """`--register` lays the slice's acquisitions on acquisition 0 and adds `shifts` [T, 2] to the record and the JSON file; without
    it the record has the keys it always had and the written images are what the unregistered pipeline gives, byte for byte."""
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
    flagged, flagged_json = run("flag", "--register")
    parent_keys = ["patient", "shape", "sample_size", "seconds", "subsets", "out_dir"]
    assert list(plain) == parent_keys == list(plain_json)
    assert list(flagged) == parent_keys + ["shifts"] == list(flagged_json)
    for k in ("patient", "shape", "sample_size", "subsets"):
        assert plain[k] == flagged[k] == plain_json[k]
    planted = np.zeros((10, 2))
    for t, s in G.RAMS_PLANTED.items():
        planted[t] = s
    assert flagged["shifts"] == flagged_json["shifts"] == planted.tolist()
    # without the flag: master.py:38-57 restated on the recorded subsets
    lor = dwi[:, :, 1, :][None].astype("uint16") * 256
    batch = np.concatenate([lor[..., inx] for inx in plain["subsets"]], axis=0)
    mean = rams.predict_tensor(model, batch)[:, :, :, 0].double().sum(dim=0).cpu().numpy() / 2
    assert np.array_equal(np.load(os.path.join(plain["out_dir"], "DWI_mean.npy")), mean)
    assert sorted(os.listdir(plain["out_dir"])) == sorted(os.listdir(flagged["out_dir"])) == ["ADC_mean.npy", "DWI_mean.npy", "images.mat"]
    # with it the network sees the registered acquisitions
    seq = dwi[:, :, 1, :].astype(np.float64)
    reg = np.clip(registration.register_imgset(seq, np.ones(seq.shape), max_shift=8)[0], 0, None)
    lor = reg[None].astype("uint16") * 256
    batch = np.concatenate([lor[..., inx] for inx in flagged["subsets"]], axis=0)
    mean_reg = rams.predict_tensor(model, batch)[:, :, :, 0].double().sum(dim=0).cpu().numpy() / 2
    assert np.array_equal(np.load(os.path.join(flagged["out_dir"], "DWI_mean.npy")), mean_reg) and not np.array_equal(mean_reg, mean)
    # a narrower window than the planted shifts is passed through
    assert run("narrow", "--register", "--register_max_shift", "1")[0]["shifts"] != planted.tolist()


def test_a_cpu_tensor_is_refused():
    img = torch.ones((8, 8))
    with pytest.raises(ops.InrDeviceError):
        registration.shift(img, (1, 1))
    with pytest.raises(ops.InrDeviceError):
        registration.masked_register_translation(img, img, img)
    with pytest.raises(ops.InrDeviceError):
        registration.register_imgset(torch.ones((8, 8, 3)), torch.ones((8, 8, 3)))
    with pytest.raises(ops.InrDeviceError):
        registration.gen_sub(torch.ones((1, 8, 8, 3)), 4, 4, verbose=False)
