"""CPU: the registration and data-preparation surface (compat import line, header, exports, ctypes table, the refusals that must arrive
before any device work), the float64 oracle of tests/register_common.py against the FFT form of the same definition, and the host
logic of select_T_images / gen_sub / augment_* against the reference's expressions restated in NumPy."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi

from tests import register_common as G
from mri_super_resolution_amd import _lib, registration
from mri_super_resolution_amd._build import LIB_PATH, SOURCES, build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = os.path.join(ROOT, "mri-super-resolution_amd", "compat")
NEW = ("inr_image_means", "inr_masked_xcorr_workspace_doubles", "inr_masked_xcorr", "inr_shift2d_workspace_doubles", "inr_shift2d")
NAMES = ("register_dataset", "register_imgset", "select_T_images", "gen_sub", "augment_dataset", "sub_images", "augment_imgset",
         "masked_register_translation", "shift")


def test_compat_import_line_resolves_to_the_package_functions():
    code = ("from utils.preprocessing import register_dataset, register_imgset, select_T_images, gen_sub, augment_dataset\n"
            "import utils.preprocessing as P\nfrom mri_super_resolution_amd import registration as R\n"
            f"print(all(getattr(P, n) is getattr(R, n) for n in {NAMES!r}), callable(P.bicubic))\n"
            "try:\n    P.load_dataset('d', 'train', 'NIR')\nexcept NotImplementedError as e:\n    print('cv2' in str(e))\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd="/tmp",
                         env=dict(os.environ, PYTHONPATH=COMPAT))
    assert out.returncode == 0 and out.stdout.split() == ["True", "True", "True"], out.stdout + out.stderr[-3000:]


def test_header_library_and_ctypes_table_carry_the_symbols():
    text = open(os.path.join(ROOT, "include", "inrhip.h")).read()
    assert "preprocessing.py:138-161" in text and "OVER THE WINDOW" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(inr_[a-z0-9_]+)\s*\(", code))
    build_library()
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(handle, name) and name in _lib.SIGNATURES, name
    assert "register.hip" in SOURCES
    assert int(re.search(r"#define INR_SHIFT_REFLECT (\d+)", text).group(1)) == registration._SHIFT_MODES["reflect"]
    assert int(re.search(r"#define INR_SHIFT_CONSTANT (\d+)", text).group(1)) == registration._SHIFT_MODES["constant"]
    assert int(re.search(r"#define INR_XCORR_MAX_SIDE (\d+)", text).group(1)) == registration._XCORR_MAX_SIDE


def test_workspace_plans_and_host_side_argument_checks():
    lib = _lib.lib()
    fake = lambda k: ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)      # never dereferenced: every call fails in validation
    plan = lib.inr_masked_xcorr_workspace_doubles
    assert plan(2, 3, 24, 20, 23, 19) == 2 * 3 * 6 * 47 * 39             # six sums per displacement and image
    assert plan(2, 3, 24, 20, 5, 5) == 2 * 3 * 6 * 11 * 11
    assert plan(2, 3, 24, 20, 24, 19) == 0 and b"window" in lib.inr_last_error()
    assert plan(2, 3, 24, 20, -1, 0) == 0 and b"window" in lib.inr_last_error()
    assert plan(0, 3, 24, 20, 1, 1) == 0 and b"bad sizes" in lib.inr_last_error()
    assert plan(1, 3, 4097, 20, 1, 1) == 0 and b"at most 4096" in lib.inr_last_error()
    assert plan(6554, 10, 8, 8, 1, 1) == 0 and b"65535 images" in lib.inr_last_error()
    need = plan(2, 3, 24, 20, 23, 19)
    ok = (fake(0), fake(1), fake(2), None, fake(3), fake(4), fake(5), 2, 3, 24, 20, 23, 19, 0.3)
    call = lib.inr_masked_xcorr
    assert call(None, *ok[1:], fake(6), need, None) == _lib.INR_E_INVALID and b"null pointer" in lib.inr_last_error()
    assert call(*ok[:6], None, *ok[7:], fake(6), need, None) == _lib.INR_E_INVALID and b"null pointer" in lib.inr_last_error()
    assert call(*ok[:11], 24, *ok[12:], fake(6), need, None) == _lib.INR_E_INVALID and b"window" in lib.inr_last_error()
    assert call(*ok[:13], 1.5, fake(6), need, None) == _lib.INR_E_INVALID and b"overlap_ratio" in lib.inr_last_error()
    assert call(*ok, fake(6), need - 1, None) == _lib.INR_E_WORKSPACE and b"workspace too small" in lib.inr_last_error()
    assert call(*ok, None, need, None) == _lib.INR_E_WORKSPACE
    assert call(*ok, ctypes.c_void_p(0x7000_0000_0008), need, None) == _lib.INR_E_ALIGN

    plan = lib.inr_shift2d_workspace_doubles
    assert plan(3, 9, 11, 0) == plan(3, 9, 11, 1) == 3 * 9 * 11 and plan(0, 9, 11, 0) == 99
    assert plan(3, 9, 11, 2) == 0 and b"mode must be" in lib.inr_last_error()
    assert plan(3, 0, 11, 0) == 0 and b"bad sizes" in lib.inr_last_error()
    assert plan(3, _lib.INR_RESCALE_MAX_LINE + 1, 11, 0) == 0 and b"lines of at most" in lib.inr_last_error()
    call = lib.inr_shift2d
    ok = (fake(0), fake(1), fake(2), 3, 9, 11, 1, 0.0)
    assert call(*ok[:2], None, *ok[3:], fake(3), 297, None) == _lib.INR_E_INVALID and b"null pointer" in lib.inr_last_error()
    assert call(*ok[:6], 5, 0.0, fake(3), 297, None) == _lib.INR_E_INVALID and b"mode must be" in lib.inr_last_error()
    assert call(*ok[:7], float("nan"), fake(3), 297, None) == _lib.INR_E_INVALID and b"cval" in lib.inr_last_error()
    assert call(*ok, fake(3), 296, None) == _lib.INR_E_WORKSPACE and b"workspace too small" in lib.inr_last_error()
    assert call(*ok, None, 297, None) == _lib.INR_E_WORKSPACE
    assert call(*ok, ctypes.c_void_p(0x7000_0000_0008), 297, None) == _lib.INR_E_ALIGN
    assert lib.inr_image_means(None, None, fake(0), 1, 1, 4, 4, None) == _lib.INR_E_INVALID and b"null pointer" in lib.inr_last_error()
    assert lib.inr_image_means(fake(0), None, fake(1), 1, 0, 4, 4, None) == _lib.INR_E_INVALID and b"bad sizes" in lib.inr_last_error()


def test_every_refusal_arrives_by_name_before_device_work():
    img, m = np.ones((8, 8)), np.ones((8, 8))
    with pytest.raises(ValueError, match="shift: only order 3"):
        registration.shift(img, (1, 1), order=1)
    with pytest.raises(ValueError, match="shift: mode must be 'reflect' or 'constant'.*'wrap'"):
        registration.shift(img, (1, 1), mode="wrap")
    with pytest.raises(ValueError, match="shift: shift must be"):
        registration.shift(img, (1, 1, 1))
    with pytest.raises(ValueError, match="shift: shift must be"):
        registration.shift(np.ones((3, 8, 8)), np.zeros((2, 2)))
    for fn in (registration.masked_register_translation, registration.masked_xcorr):
        with pytest.raises(ValueError, match=f"{fn.__name__}: target_mask is not supported"):
            fn(img, img, m, target_mask=m)
        with pytest.raises(ValueError, match=f"{fn.__name__}: src_image .* and src_mask .* differ in shape"):
            fn(img, img, np.ones((8, 7)))
        with pytest.raises(ValueError, match=f"{fn.__name__}: src_image .* and target_image .* differ in shape"):
            fn(img, np.ones((7, 8)), m)
        with pytest.raises(ValueError, match=f"{fn.__name__}: max_shift"):
            fn(img, img, m, max_shift=-1)
        with pytest.raises(ValueError, match=f"{fn.__name__}: overlap_ratio"):
            fn(img, img, m, overlap_ratio=1.5)
    with pytest.raises(ValueError, match="register_imgset: imgset .* and mask .* differ in shape"):
        registration.register_imgset(np.ones((8, 8, 3)), np.ones((8, 8, 4)))
    with pytest.raises(ValueError, match="register_imgset: imgset must have 3 axes"):
        registration.register_imgset(img, m)
    with pytest.raises(ValueError, match="register_dataset: set 1: imgset .* and mask .* differ"):
        registration.register_dataset([np.ones((8, 8, 3))] * 2, [np.ones((8, 8, 3)), np.ones((8, 6, 3))])
    sets, masks = [np.ones((8, 8, 3))], [np.ones((8, 8, 3))]
    for T in (0, -1, 2.5):
        with pytest.raises(ValueError, match="select_T_images: T must be a positive integer"):
            registration.select_T_images(sets, masks, T=T)
    for thr in (-0.1, 1.5):
        with pytest.raises(ValueError, match="select_T_images: thr"):
            registration.select_T_images(sets, masks, thr=thr)
    with pytest.raises(ValueError, match="select_T_images: set 0: imgset .* and mask .* differ"):
        registration.select_T_images(sets, [np.ones((8, 8, 2))])
    with pytest.raises(ValueError, match="d, s and n should be integer values"):
        registration.gen_sub(np.ones((2, 16, 16, 9)), 8, 3, verbose=False)             # (16 - 8) / 3 + 1 is no integer
    with pytest.raises(ValueError, match="Wrong array shape"):
        registration.gen_sub(np.ones((16, 16, 9)), 8, 4, verbose=False)
    with pytest.raises(ValueError, match="augment_dataset: n_augment"):
        registration.augment_dataset(np.ones((1, 4, 4, 3)), np.ones((1, 12, 12, 1)), np.ones((1, 12, 12, 1)), n_augment=0)


@pytest.mark.parametrize("shape,planted", G.CASES, ids=G.CASE_IDS)
def test_the_oracle_stands(shape, planted):
    """The direct float64 form against the FFT form of the same six correlations, and the conditions on the INPUTS under which a
    device map can be compared entry by entry (an input that fails one is to be changed, not the bound)."""
    ref, x, m = G.make_case(shape, planted)
    assert np.array_equal(ref, ref.astype(np.float32)) and np.array_equal(x, x.astype(np.float32))
    assert 0 < (m == 0).sum() < m.size / 4
    st = G.case_stats(ref, x, m)
    print(f"{shape}: shift {st['shift']} peak {st['peak']:.4f} second {st['second']:.4f} kappa {st['kappa']:.1f} "
          f"fft-direct {st['fft_diff']:.2e} bound {G.map_bound(st, shape[0] * shape[1]):.2e}")
    assert st["C"].shape == (2 * shape[0] - 1, 2 * shape[1] - 1)
    assert st["fft_diff"] <= 1e-10
    assert tuple(st["shift"]) == planted
    assert st["count"] == 1
    assert st["peak"] - st["second"] >= 0.05
    assert st["kappa"] <= 100
    assert not st["near_tol"]
    # the oracle is the definition: a displacement evaluated pair by pair
    H, W = shape
    for dy, dx in [planted, (0, 0), (3, -2), (-2, 1)]:                       # small enough for the overlap rule to keep them
        r0, r1, c0, c1 = max(0, dy), min(H, H + dy), max(0, dx), min(W, W + dx)
        k = (m[r0:r1, c0:c1] != 0) & (m[r0 - dy:r1 - dy, c0 - dx:c1 - dx] != 0)
        a, b = ref[r0:r1, c0:c1][k], x[r0 - dy:r1 - dy, c0 - dx:c1 - dx][k]
        n = k.sum()
        num = (a * b).sum() - a.sum() * b.sum() / n
        den = np.sqrt(max((a * a).sum() - a.sum() ** 2 / n, 0) * max((b * b).sum() - b.sum() ** 2 / n, 0))
        assert abs(st["C"][dy + H - 1, dx + W - 1] - np.clip(num / den, -1, 1)) <= 1e-12


def test_the_oracle_window_all_zero_mask_and_scipy_shift_facts():
    ref, x, m = G.make_case(*G.CASES[2])
    # a window restricts the displacements; max den and max n are then the window's
    C5 = G.direct_xcorr(ref, x, m, max_shift=5)
    assert C5.shape == (11, 11)
    full = G.direct_xcorr(ref, x, m)
    assert np.abs(C5 - full[32 - 5:32 + 6, 30 - 5:30 + 6]).max() <= 1e-15      # here the full map's maxima lie inside the window
    # no pixel set: every entry 0, every entry a maximum, the mean position the centre
    C0 = G.direct_xcorr(ref, x, np.zeros_like(m))
    s, peak, count = G.shift_of(C0)
    assert not C0.any() and tuple(s) == (0.0, 0.0) and peak == 0.0 and count == C0.size
    # scipy 1.15: the 'constant' prefilter is the 'mirror' one, bit for bit; what leaves [0, n - 1] on any axis is cval exactly
    line = np.random.default_rng(0).random(9)
    assert np.array_equal(ndi.spline_filter1d(line, 3, mode="constant"), ndi.spline_filter1d(line, 3, mode="mirror"))
    out = ndi.shift(np.random.default_rng(1).random((9, 11)) + 1, (1.3, -2.6), mode="constant", cval=0)
    assert list(np.flatnonzero((out == 0).all(axis=1))) == [0, 1] and list(np.flatnonzero((out == 0).all(axis=0))) == [8, 9, 10]


def test_select_indexes_against_the_restated_reference():
    rng = np.random.default_rng(3)
    for trial in range(20):
        clear = rng.permutation(np.linspace(0.5, 0.99, 14))[:rng.integers(1, 14)]        # distinct: argsort ties are unspecified
        for T, thr, remove_bad in [(9, 0.85, True), (9, 0.85, False), (4, 0.6, True), (12, 0.995, False), (3, 0.995, True)]:
            np.random.seed(trial)
            want = G.select_indexes(clear, T, thr, remove_bad)
            np.random.seed(trial)
            got = registration.select_indexes(clear, T, thr, remove_bad)
            assert got == want
            if want is not None:
                assert len(want) == T
                kept = [i for i in want if clear[i] > thr]
                first = kept[:min(T, (clear > thr).sum())]
                assert list(clear[first]) == sorted(clear[first], reverse=True)
    # the reference's own expressions on one hand-made set: three clear images, T = 5 -> two np.random.choice draws from the three
    clear = np.array([0.9, 0.5, 0.95, 0.86])
    np.random.seed(7)
    order = list(np.argsort(clear[clear > 0.85])[::-1])
    draws = [np.random.choice(order) for _ in range(2)]
    np.random.seed(7)
    assert registration.select_indexes(clear, 5, 0.85, True) == [int(np.flatnonzero(clear > 0.85)[j]) for j in order + draws]
    assert registration.select_indexes(np.array([0.2, 0.4, 0.3]), 3, 0.85, True) is None
    assert registration.select_indexes(np.array([0.2, 0.4, 0.3]), 3, 0.85, False) == [1, 1, 1]


def test_patch_count_and_augment_permutations():
    assert registration.patch_count(16, 8, 4) == 3 and registration.patch_count(128, 32, 32) == 4
    for d_o, d, s in [(16, 8, 3), (16, 5, 4), (16, 17, 1), (16, 0, 4), (16, 8, 0)]:
        with pytest.raises(ValueError, match="d, s and n should be integer values"):
            registration.patch_count(d_o, d, s)
    np.random.seed(11)
    want = [np.arange(9)] + [np.random.permutation(9) for _ in range(6)]
    np.random.seed(11)
    got = registration.augment_permutations(9, 7)
    assert got.shape == (7, 9) and all(np.array_equal(a, b) for a, b in zip(got, want))
    # restated gen_sub / augment on the host: order item, row, column; the original first, then the permuted copies
    arr = np.arange(2 * 16 * 16 * 3, dtype=np.float64).reshape(2, 16, 16, 3)
    sub = G.gen_sub_restated(arr, 8, 4)
    assert sub.shape == (18, 8, 8, 3) and np.array_equal(sub[9 + 3 * 1 + 2], arr[1, 4:12, 8:16])
    np.random.seed(5)
    Xa, ya, ma = G.augment_restated(arr, np.arange(2)[:, None], np.arange(2)[:, None], 3)
    assert Xa.shape == (6, 16, 16, 3) and np.array_equal(Xa[3], arr[1]) and list(ya[:, 0]) == [0, 0, 0, 1, 1, 1]
