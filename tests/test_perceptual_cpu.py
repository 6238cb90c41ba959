"""CPU-only checks of the reader study's scores (csrc/perceptual.hip, perceptual.py, scripts/perceptual_similarity.py): the float64
restatement of the definitions (tests/perceptual_common.py) reproduces the recorded fixture and the cross-check values of figure 291;
the entry points are declared, exported and bound; every argument error is refused before any device work (fake device pointers
that are never dereferenced); and the script's host logic -- crop geometry, labels by position, --qual_dir parsing, the CSV columns
and the t-test -- runs with a stub scorer."""
import csv
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import stats

from mri_super_resolution_amd import _lib, matio
from mri_super_resolution_amd.scripts import perceptual_similarity as script
from tests import perceptual_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("inr_perceptual_workspace_doubles", "inr_ssim2d_gauss", "inr_msssim2d", "inr_filter3x3", "inr_image_mse", "inr_hf_gain")

# A throwaway float64 restatement of the definitions, run once on a CPU (NOT MATLAB output): figure 291, data_range 255 on the
# crops and 1 after the high-pass
FIGURE_291 = {"ssim_raw_interpolated": 0.9157286614, "ssim_raw_SR": 0.9230577327, "mse_raw_interpolated": 58.28272834,
              "mse_raw_SR": 152.41419519, "ms_ssim_raw_interpolated": 0.9079416152, "ms_ssim_raw_SR": 0.9256254172,
              "ssim_hpf_interpolated": 0.5096563796, "ssim_hpf_SR": 0.5680081442, "ms_ssim_hpf_interpolated": 0.7183957555,
              "ms_ssim_hpf_SR": 0.7731505390, "hf_gain": 0.0099716975}


def _fake(k, off=0):
    return ctypes.c_void_p(0x7000_0000_0000 + 4096 * k + off)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crops():
    return np.load(pc.GOLDEN)


def test_fixture_holds_the_crops_their_labels_and_the_scores(crops):
    assert os.path.getsize(pc.GOLDEN) < 1000000
    figures = crops["figures"].tolist()
    assert figures[0] == 291
    for fig in figures:
        for name in script.PANEL_NAMES:
            assert crops[f"{fig}/{name}"].shape == (401, 401) and crops[f"{fig}/{name}"].dtype == np.uint8
        row = crops[f"{fig}/label_row"].tolist()
        assert row[1] == str(fig) and sorted(row[4:8]) == sorted(script.PANEL_NAMES)


def test_restatement_reproduces_the_fixture_and_the_cross_check_values(crops):
    for fig in crops["figures"].tolist():
        got = pc.reader_study_scores(crops[f"{fig}/interpolated"], crops[f"{fig}/SR"], crops[f"{fig}/base"], 255.0, 1.0)
        assert len(got) == 13
        for key, val in got.items():
            assert val == pytest.approx(float(crops[f"{fig}/score/{key}"]), rel=1e-13, abs=0), (fig, key)
        if fig == 291:
            for key, val in FIGURE_291.items():
                assert got[key] == pytest.approx(val, abs=1e-8, rel=0), key


def test_restatement_edge_rules():
    g = pc.gauss_window(1.5)
    assert len(g) == 11 and g.sum() == pytest.approx(1.0, abs=1e-15) and np.array_equal(g, g[::-1])
    assert len(pc.gauss_window(0.8)) == 7 and len(pc.gauss_window(2.3)) == 15
    a = np.arange(15, dtype=np.float64).reshape(3, 5)
    d = pc.down2(a)
    assert d.shape == (2, 3)
    assert d[0, 0] == (0 + 1 + 5 + 6) / 4 and d[0, 2] == (4 + 4 + 9 + 9) / 4 and d[1, 2] == 14.0 and d[1, 0] == (10 + 11) / 2
    k = pc.unsharp_kernel()
    assert k.sum() == pytest.approx(1.0, abs=1e-15) and k[1, 1] == pytest.approx(5.2 / 1.2)
    one = pc.filter3x3(np.ones((2, 3), dtype=np.float32), k)
    assert one[0, 0] == pytest.approx(k[1:, 1:].sum()) and one[0, 1] == pytest.approx(k[1:, :].sum())      # zero padding
    x = np.random.default_rng(0).random((9, 12))
    s, cs, m = pc.ssim_gauss(x, x)
    assert s == 1.0 and cs == 1.0 and m.shape == x.shape
    v, per = pc.ms_ssim(x, 1.0 - x, weights=(0.5, 0.5))
    assert per[0] < 0 and np.isnan(v)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inrhip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name) and hasattr(_lib.lib(), name), name
    assert "INR_PERCEPTUAL_MAX_RADIUS 7" in text and "INR_PERCEPTUAL_MAX_SCALES 8" in text
    from mri_super_resolution_amd import _build
    assert "perceptual.hip" in _build.SOURCES


def test_module_exports():
    from mri_super_resolution_amd import perceptual
    assert sorted(perceptual.__all__) == sorted(["ssim_gauss", "ms_ssim", "hpf", "filter3x3", "unsharp_kernel", "mse", "hf_gain",
                                                 "reader_study_scores"])
    for name in perceptual.__all__:
        assert callable(getattr(perceptual, name)), name
    assert np.array_equal(perceptual.unsharp_kernel(), pc.unsharp_kernel())
    assert perceptual.MS_SSIM_WEIGHTS == pc.MS_SSIM_WEIGHTS


def test_workspace_doubles_planner_is_pinned():
    ws = _lib.lib().inr_perceptual_workspace_doubles
    # recorded values: regions of 256 bytes -- 128 partials of the flat reductions per image, 2 per tile (32 x 16) and image,
    # 8 per-scale means per image, then two pairs of fp64 levels (23 x 26 and 12 x 13 per image for 45 x 52)
    assert [ws(*a) for a in ((1, 1, 1, 1), (3, 1, 1, 1), (3, 45, 52, 1), (3, 45, 52, 3), (4, 401, 401, 5))] == \
        [192, 448, 480, 5088, 408192]
    assert ws(3, 45, 52, 3) * 8 == 3072 + 512 + 256 + 2 * 14592 + 2 * 3840
    assert ws(3, 1, 1, 1) <= ws(3, 45, 52, 1) <= ws(3, 45, 52, 2) <= ws(3, 45, 52, 3) == ws(3, 45, 52, 8)
    assert ws(4, 401, 401, 5) >= 2 * 4 * (201 * 201 + 101 * 101)
    assert ws(4, 401, 401, 5) % 32 == 0
    for bad in ((0, 4, 4, 1), (-1, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (1, 4, 4, 9), (65536, 4, 4, 1)):
        assert ws(*bad) == 0, bad


def test_ssim_gauss_refusals_come_before_device_work():
    lib = _lib.lib()
    need = lib.inr_perceptual_workspace_doubles(3, 45, 52, 1)

    def call(ssim=_fake(1), cs=None, smap=None, x=_fake(4), y=_fake(5), n=3, h=45, w=52, sigma=1.5, rng=1.0, ws=_fake(6), wb=need):
        return lib.inr_ssim2d_gauss(ssim, cs, smap, x, y, n, h, w, sigma, rng, ws, wb, None)

    for kw in ({"ssim": None}, {"x": None}, {"y": None}):
        assert call(**kw) == _lib.INR_E_INVALID, kw
        assert b"null pointer" in lib.inr_last_error()
    for kw in ({"n": 0}, {"n": -2}, {"h": 0}, {"w": 0}, {"h": -1}, {"sigma": 0.0}, {"sigma": -1.0}, {"sigma": float("nan")},
               {"sigma": 2.4}, {"sigma": 50.0}, {"rng": 0.0}):
        assert call(**kw) == _lib.INR_E_INVALID, kw
        assert lib.inr_last_error().startswith(b"inr_ssim2d_gauss:")
    assert call(sigma=2.4) == _lib.INR_E_INVALID and b"<= 7" in lib.inr_last_error()        # ceil(7.2) = 8 taps per side
    assert call(ws=None) == _lib.INR_E_WORKSPACE
    assert call(wb=need - 1) == _lib.INR_E_WORKSPACE and b"workspace too small" in lib.inr_last_error()
    assert call(wb=0) == _lib.INR_E_WORKSPACE
    for kw in ({"ssim": _fake(1, 8)}, {"cs": _fake(2, 8)}, {"smap": _fake(3, 4)}, {"x": _fake(4, 4)}, {"y": _fake(5, 12)},
               {"ws": _fake(6, 8)}):
        assert call(**kw) == _lib.INR_E_ALIGN, kw
        assert b"16-byte aligned" in lib.inr_last_error()


def test_msssim_refusals_come_before_device_work():
    lib = _lib.lib()
    need = lib.inr_perceptual_workspace_doubles(2, 45, 52, 3)
    wts = (ctypes.c_double * 3)(0.2, 0.3, 0.5)

    def call(out=_fake(1), per=None, x=_fake(4), y=_fake(5), n=2, h=45, w=52, weights=wts, s=3, sigma=1.5, rng=1.0, ws=_fake(6),
             wb=need):
        return lib.inr_msssim2d(out, per, x, y, n, h, w, weights, s, sigma, rng, ws, wb, None)

    for kw in ({"out": None}, {"x": None}, {"y": None}, {"weights": None}):
        assert call(**kw) == _lib.INR_E_INVALID, kw
        assert b"null pointer" in lib.inr_last_error()
    for kw in ({"n": 0}, {"h": 0}, {"w": 0}, {"s": 0}, {"s": 9}, {"s": -1}, {"sigma": 2.5}, {"sigma": 0.0}, {"rng": -1.0}):
        assert call(**kw) == _lib.INR_E_INVALID, kw
    assert call(s=9) == _lib.INR_E_INVALID and b"n_scales" in lib.inr_last_error()
    assert call(ws=None) == _lib.INR_E_WORKSPACE
    assert call(wb=lib.inr_perceptual_workspace_doubles(2, 45, 52, 1)) == _lib.INR_E_WORKSPACE     # sized for one scale only
    assert b"workspace too small" in lib.inr_last_error()
    for kw in ({"out": _fake(1, 8)}, {"per": _fake(2, 8)}, {"x": _fake(4, 4)}, {"y": _fake(5, 4)}, {"ws": _fake(6, 4)}):
        assert call(**kw) == _lib.INR_E_ALIGN, kw


def test_filter_and_pair_score_refusals_come_before_device_work():
    lib = _lib.lib()
    k9 = (ctypes.c_double * 9)(*pc.unsharp_kernel().reshape(-1))
    filt = lambda out=_fake(1), inp=_fake(2), n=3, h=45, w=52, k=k9: lib.inr_filter3x3(out, inp, n, h, w, k, None)      # noqa: E731
    for kw in ({"out": None}, {"inp": None}, {"k": None}):
        assert filt(**kw) == _lib.INR_E_INVALID and b"null pointer" in lib.inr_last_error(), kw
    for kw in ({"n": 0}, {"h": 0}, {"w": 0}, {"w": -3}):
        assert filt(**kw) == _lib.INR_E_INVALID, kw
    for kw in ({"out": _fake(1, 4)}, {"inp": _fake(2, 8)}):
        assert filt(**kw) == _lib.INR_E_ALIGN, kw
    need = lib.inr_perceptual_workspace_doubles(3, 1, 1, 1)
    for entry, who in ((lib.inr_image_mse, b"inr_image_mse"), (lib.inr_hf_gain, b"inr_hf_gain")):
        call = lambda out=_fake(1), x=_fake(2), y=_fake(3), n=3, per=2340, ws=_fake(4), wb=need: entry(out, x, y, n, per, ws, wb, None)  # noqa: E731
        for kw in ({"out": None}, {"x": None}, {"y": None}):
            assert call(**kw) == _lib.INR_E_INVALID and b"null pointer" in lib.inr_last_error(), kw
        for kw in ({"n": 0}, {"n": -1}, {"per": 0}, {"per": -5}):
            assert call(**kw) == _lib.INR_E_INVALID and lib.inr_last_error().startswith(who), kw
        assert call(ws=None) == _lib.INR_E_WORKSPACE
        assert call(wb=need - 1) == _lib.INR_E_WORKSPACE and b"workspace too small" in lib.inr_last_error()
        for kw in ({"out": _fake(1, 8)}, {"x": _fake(2, 4)}, {"y": _fake(3, 4)}, {"ws": _fake(4, 8)}):
            assert call(**kw) == _lib.INR_E_ALIGN, kw


# ---- the script's host logic -----------------------------------------------------------------------------------------------------------
def _stub(inter, sr, base, data_range, hpf_data_range):
    """a scorer that needs no device: every score a simple function of its inputs, recognisable afterwards"""
    n = inter.shape[0]
    flat = lambda a: a.reshape(n, -1).astype(np.float64)        # noqa: E731
    out = {}
    for j, index in enumerate(script.INDICES):
        for filt, rng in (("raw", data_range), ("hpf", hpf_data_range)):
            out[f"{index}_{filt}_interpolated"] = (flat(inter).mean(1) + j) / rng
            out[f"{index}_{filt}_SR"] = (flat(sr).mean(1) * (1.5 + 0.1 * np.arange(n)) + j) / rng
    out["hf_gain"] = flat(base).mean(1)
    return out


def _pattern(h, w):
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return ((r * 7 + c * 13) % 251).astype(np.uint8)


def test_rgb2gray_is_the_rounded_weighted_sum():
    rgb = np.array([[[255, 255, 255, 9], [0, 0, 0, 9], [10, 200, 30, 9], [1, 1, 1, 9], [3, 0, 1, 9]]], dtype=np.uint8)
    assert script.rgb2gray_uint8(rgb).tolist() == [[255, 0, 124, 1, 1]]      # .2989*10 + .587*200 + .114*30 = 123.809; 1.0107
    assert script.rgb2gray_uint8(rgb).dtype == np.uint8


def test_png_route_crops_by_the_m_files_geometry_and_names_panels_by_position(tmp_path):
    from PIL import Image
    gray = _pattern(3000, 6000)
    rgba = np.stack([gray, gray, gray, np.full_like(gray, 255)], axis=-1)       # gray = round(0.9999 v) = v
    Image.fromarray(rgba).save(tmp_path / "7.png", compress_level=1)
    with open(tmp_path / "labels.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["", "file", "pt", "image", "1", "2", "4", "3"])
        w.writerow(["0", "6", "p", "1", "low", "interpolated", "SR", "base"])       # row 2: not selected
        w.writerow(["1", "7", "pt-07", "12", "SR", "base", "low", "interpolated"])
    slices = script.load_png_dir(str(tmp_path), rows="3:3")
    assert len(slices) == 1
    s = slices[0]
    assert (s["file"], s["pt"], s["image"], s["data_range"], s["hpf_data_range"]) == ("7", "pt-07", "12", 255.0, 1.0)
    # 1-based inclusive rows 381:1390, then 300:700 -> 0-based rows 679 .. 1079; columns start + 299 .. start + 699 (start 1-based)
    for name, start in zip(("SR", "base", "low", "interpolated"), (751, 1964, 4390, 3177)):
        crop = s["panels"][name]
        assert crop.shape == (401, 401) and crop.dtype == np.uint8
        assert np.array_equal(crop, gray[679:1080, start - 1 + 299:start - 1 + 700]), name
    assert script.PANEL_WIDTH == 1011
    with pytest.raises(ValueError, match="at least"):
        script.crop_panels(gray[:1000], ["low", "interpolated", "SR", "base"])
    # the whole script on this route, with the stub: MATLAB's class rule reaches the scorer
    seen = []
    script.main(["--png_dir", str(tmp_path), "--rows", "3:3", "--out_dir", str(tmp_path / "out")],
                scorer=lambda i, s_, b, r, hr: (seen.append((i.shape, i.dtype, r, hr)), _stub(i, s_, b, r, hr))[1])
    assert seen == [((1, 401, 401), np.dtype(np.float32), 255.0, 1.0)]
    with pytest.raises(ValueError, match="class rule"):
        script.main(["--png_dir", str(tmp_path), "--data_range", "1"], scorer=_stub)


def test_rows_selection():
    rows = [["h"]] + [[str(i)] for i in range(2, 80)]
    assert [r[0] for r in script.select_rows(rows, "2:66")] == [str(i) for i in range(2, 67)]
    assert script.select_rows(rows, None) == rows[1:]
    assert script.select_rows(rows[:4], "2:66") == rows[1:4]
    with pytest.raises(ValueError):
        script.select_rows(rows, "1:3")


def _qual_dir(tmp_path, n=3):
    rng = np.random.default_rng(5)
    with open(tmp_path / "labels.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["file", "pt", "image", "1", "2", "3", "4"])
        for k in range(n):
            maps = {name: rng.random((12, 10)) * (k + 1) for name in ("low", "interpolated", "SR", "base", "adc_gold")}
            matio.savemat(str(tmp_path / f"{291 + k}.mat"), maps)
            w.writerow([str(291 + k), f"pt{k}", str(k + 4), "SR", "low", "base", "interpolated"])
            yield maps


def test_qual_dir_route_takes_panels_by_name_and_writes_both_csvs(tmp_path):
    maps = list(_qual_dir(tmp_path))
    slices = script.load_qual_dir(str(tmp_path))
    assert [s["file"] for s in slices] == ["291", "292", "293"] and [s["image"] for s in slices] == ["4", "5", "6"]
    for s, m in zip(slices, maps):
        for name in script.PANEL_NAMES:
            assert np.array_equal(s["panels"][name], m[name]) and s["panels"][name].dtype == np.float64
        assert s["data_range"] == s["hpf_data_range"] == m["base"].max()
    assert all(s["data_range"] == 2.0 for s in script.load_qual_dir(str(tmp_path), data_range=2.0))
    assert [s["file"] for s in script.load_qual_dir(str(tmp_path), rows="3:4")] == ["292", "293"]

    out = tmp_path / "out"
    _, scores = script.main(["--qual_dir", str(tmp_path), "--data_range", "2", "--out_dir", str(out)], scorer=_stub)
    table = list(csv.reader(open(out / "scores.csv")))
    assert table[0] == ["file", "pt", "image", "index", "filter", "interpolated", "SR"]
    assert len(table) == 1 + 3 * 7
    assert [r[3:5] for r in table[1:8]] == [["ssim", "raw"], ["ssim", "hpf"], ["mse", "raw"], ["mse", "hpf"], ["ms_ssim", "raw"],
                                            ["ms_ssim", "hpf"], ["hf_gain", "hpf"]]
    assert table[1][:3] == ["291", "pt0", "4"] and table[8][:3] == ["292", "pt1", "5"]
    assert float(table[1][5]) == pytest.approx(maps[0]["interpolated"].mean() / 2.0, rel=1e-6)
    assert table[7][5] == "" and float(table[7][6]) == pytest.approx(maps[0]["base"].mean(), rel=1e-6)
    assert "FSIM" not in " ".join(table[0])

    summary = list(csv.reader(open(out / "summary.csv")))
    assert summary[0] == ["index", "filter", "n", "mean_interpolated", "mean_SR", "std_interpolated", "std_SR", "p"]
    assert len(summary) == 1 + 6
    for row in summary[1:]:
        a = np.array([sc[f"{row[0]}_{row[1]}_interpolated"] for sc in scores])
        b = np.array([sc[f"{row[0]}_{row[1]}_SR"] for sc in scores])
        assert int(row[2]) == 3
        assert float(row[3]) == a.mean() and float(row[4]) == b.mean()
        assert float(row[5]) == np.std(a, ddof=1) and float(row[6]) == np.std(b, ddof=1)
        assert float(row[7]) == stats.ttest_rel(a, b).pvalue and 0.0 < float(row[7]) < 1.0


def test_qual_dir_default_ranges_split_the_batch_per_slice(tmp_path):
    list(_qual_dir(tmp_path, n=2))
    seen = []
    script.main(["--qual_dir", str(tmp_path), "--out_dir", str(tmp_path / "o")],
                scorer=lambda i, s_, b, r, hr: (seen.append((i.shape[0], r, hr)), _stub(i, s_, b, r, hr))[1])
    assert len(seen) == 2 and all(n == 1 and r == hr for n, r, hr in seen) and seen[0][1] != seen[1][1]


def test_one_slice_gives_no_t_test(tmp_path):
    rows = script.summary_rows([{f"{i}_{f}_{p}": 0.5 for i in script.INDICES for f in script.FILTERS for p in ("interpolated", "SR")}])
    assert all(r[2] == 1 and r[7] == "nan" and r[5] == "nan" for r in rows)


def test_parser_needs_exactly_one_source():
    with pytest.raises(SystemExit):
        script.build_parser().parse_args([])
    with pytest.raises(SystemExit):
        script.build_parser().parse_args(["--qual_dir", "a", "--png_dir", "b"])
