"""CPU: the Fourier re-sampling surface (header, exports, ctypes table, workspace plan, host-side argument checks, the refusals of the
Python entry points) and the float64 restatement the kernels of csrc/fourier.hip are written from (tests/fourier_common.py) against
scipy.signal.resample and a direct evaluation of the trigonometric polynomial."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import fourier_common as F
from mri_super_resolution_amd import _lib, baselines, matio, ops
from mri_super_resolution_amd.scripts import superresDWI as dwi_script
from mri_super_resolution_amd._build import LIB_PATH, SOURCES, build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("inr_fourier_operator", "inr_fourier_resample_workspace_doubles", "inr_fourier_resample2d", "inr_fourier_resample2d_f32")


def _check(n, m, align, boundary, apodize):
    x = F.lines(n)
    A = F.restated_operator(n, m, align, boundary, apodize)
    want = F.oracle_resample(x, m, align, boundary, apodize)
    got = A @ x
    err, tol, rows = np.abs(got - want).max(), F.bound(x, want), np.abs(A.sum(axis=1) - 1.0).max()
    print(f"{n}->{m} {align} {boundary} apodize {apodize}: |restated - oracle| {err:.2e} (bound {tol:.2e}), |row sums - 1| {rows:.2e}")
    assert A.shape == (m, n) and got.shape == want.shape
    assert err <= tol
    assert rows <= 1e-13


@pytest.mark.parametrize("apodize", F.APODIZE)
@pytest.mark.parametrize("align", F.ALIGNS)
@pytest.mark.parametrize("n,m", F.PAIRS, ids=[f"{n}to{m}" for n, m in F.PAIRS])
def test_restatement_matches_the_oracles_periodic(n, m, align, apodize):
    _check(n, m, align, "periodic", apodize)


@pytest.mark.parametrize("apodize", F.APODIZE)
@pytest.mark.parametrize("n,m,align", [(n, m, "sample") for n, m in F.MIRROR_SAMPLE_PAIRS] + [(n, m, "center") for n, m in F.PAIRS],
                         ids=[f"{n}to{m}-sample" for n, m in F.MIRROR_SAMPLE_PAIRS] + [f"{n}to{m}-center" for n, m in F.PAIRS])
def test_restatement_matches_the_oracles_mirror(n, m, align, apodize):
    _check(n, m, align, "mirror", apodize)


def test_the_oracles_are_what_they_are_listed_as():
    """The trigonometric polynomial is scipy.signal.resample where both are defined, so the apodised and centred cases are checked
    against a continuation of the same function; and the listed pairs cover what they are listed for."""
    for n, m in F.PAIRS:
        x = F.lines(n)
        assert np.abs(F.trig_resample(x, m) - F.oracle_resample(x, m, "sample", "periodic")).max() <= F.bound(x, x)
    assert [F.mirror_sample_ok(n, m) for n, m in F.MIRROR_SAMPLE_PAIRS] == [True] * 4
    assert not F.mirror_sample_ok(25, 30) and not F.mirror_sample_ok(26, 51) and not F.mirror_sample_ok(1, 4)
    # the Hann window removes the band's last bin, no window keeps it
    assert F.tukey(4, 8, 1.0) == pytest.approx(0.0, abs=1e-16) and F.tukey(4, 8, 0.0) == 1.0 and F.tukey(2, 8, 0.5) == 1.0
    # the window against values worked out by hand.  L = 8, so r = k/4.  Hann (alpha = 1): w = (1 + cos(pi r))/2 = (1 + cos(pi/4))/2,
    # 1/2, (1 - cos(pi/4))/2 at k = 1, 2, 3.  alpha = 1/2: flat up to r = 1/2, then (1 + cos(2 pi (r - 1/2)))/2 = 1/2 at k = 3, 0 at k = 4.
    # L = 5 (odd: r = k/2.5), alpha = 0.4: flat up to r = 0.6, so w(1) = 1 and w(2) = (1 + cos(pi (0.8 - 0.6)/0.4))/2 = 1/2.
    hand = {(0, 8, 1.0): 1.0, (1, 8, 1.0): (2 + 2 ** 0.5) / 4, (2, 8, 1.0): 0.5, (3, 8, 1.0): (2 - 2 ** 0.5) / 4,
            (1, 8, 0.5): 1.0, (3, 8, 0.5): 0.5, (4, 8, 0.5): 0.0, (1, 5, 0.4): 1.0, (2, 5, 0.4): 0.5}
    for (k, L, alpha), want in hand.items():
        assert F.tukey(k, L, alpha) == pytest.approx(want, abs=1e-15), (k, L, alpha)
    # the bin at k = L/2: the input's own Nyquist bin once, two bins folded onto the output's Nyquist twice
    assert F.nyquist_weight(8, 16) == 1.0 and F.nyquist_weight(8, 8) == 1.0 and F.nyquist_weight(16, 8) == 2.0
    # an identity axis: the restated operator is the unit matrix to rounding
    assert np.abs(F.restated_operator(7, 7, "sample", "periodic") - np.eye(7)).max() <= 1e-15


def test_header_library_and_ctypes_table_carry_the_symbols():
    text = open(os.path.join(ROOT, "include", "inrhip.h")).read()
    assert "scipy.signal.resample" in text and "v_mfma_f64_16x16x4_f64" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(inr_[a-z0-9_]+)\s*\(", code))
    build_library()
    handle = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(handle, name) and name in _lib.SIGNATURES, name
    assert sorted(k for k in _lib.SIGNATURES if k.startswith("inr_fourier_") and k != "inr_fourier_map") == sorted(NEW)
    assert "fourier.hip" in SOURCES
    for name in ("INR_FOURIER_SAMPLE", "INR_FOURIER_CENTER", "INR_FOURIER_PERIODIC", "INR_FOURIER_MIRROR", "INR_FOURIER_MAX_LINE"):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == getattr(_lib, name)
    assert _lib.INR_FOURIER_MAX_LINE == 1024


def test_workspace_plan_and_host_side_argument_checks():
    lib = _lib.lib()
    fake = lambda k: ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)      # never dereferenced: every call fails in validation
    plan = lib.inr_fourier_resample_workspace_doubles
    # the two operators [OH][H] and [OW][W] and the plane between the passes [n][H][OW], every region rounded up to 256 bytes
    up = lambda n: (n + 31) // 32 * 32
    assert plan(12, 25, 19, 50, 38) == up(50 * 25) + up(38 * 19) + up(12 * 25 * 38) == 1280 + 736 + 11424
    assert plan(3, 128, 128, 64, 64) == up(64 * 128) + up(64 * 128) + up(3 * 128 * 64) == 8192 + 8192 + 24576
    assert plan(0, 8, 8, 16, 16) == plan(1, 8, 8, 16, 16) > 0
    assert plan(1, 0, 8, 8, 8) == 0 and b"bad sizes" in lib.inr_last_error()
    assert plan(-1, 8, 8, 8, 8) == 0 and b"bad sizes" in lib.inr_last_error()
    assert plan(1, 8, 8, 8, _lib.INR_FOURIER_MAX_LINE + 1) == 0 and b"lines of at most 1024" in lib.inr_last_error()
    assert plan(1, _lib.INR_FOURIER_MAX_LINE, 8, 8, _lib.INR_FOURIER_MAX_LINE) > 0

    S, C, P, M = _lib.INR_FOURIER_SAMPLE, _lib.INR_FOURIER_CENTER, _lib.INR_FOURIER_PERIODIC, _lib.INR_FOURIER_MIRROR
    need = plan(2, 25, 19, 50, 38)
    for call in (lib.inr_fourier_resample2d, lib.inr_fourier_resample2d_f32):
        who = call.__name__.encode()
        err = lambda: lib.inr_last_error()
        ok = (fake(0), fake(1), 2, 25, 19, 50, 38, S, M, 0.0)
        assert call(None, *ok[1:], fake(2), need, None) == _lib.INR_E_INVALID and b"null pointer" in err() and who in err()
        assert call(ok[0], None, *ok[2:], fake(2), need, None) == _lib.INR_E_INVALID and b"null pointer" in err()
        assert call(*ok[:3], 0, *ok[4:], fake(2), need, None) == _lib.INR_E_INVALID and b"bad sizes" in err()
        assert call(*ok[:6], 0, *ok[7:], fake(2), need, None) == _lib.INR_E_INVALID and b"bad sizes" in err()
        assert call(*ok[:2], -1, *ok[3:], fake(2), need, None) == _lib.INR_E_INVALID and b"bad sizes" in err()
        assert call(*ok[:5], 1025, *ok[6:], fake(2), need, None) == _lib.INR_E_INVALID and b"lines of at most 1024" in err()
        assert call(*ok[:9], 1.5, fake(2), need, None) == _lib.INR_E_INVALID and b"apodize must be in [0, 1]" in err()
        assert call(*ok[:9], -0.1, fake(2), need, None) == _lib.INR_E_INVALID and b"apodize" in err()
        assert call(*ok[:9], float("nan"), fake(2), need, None) == _lib.INR_E_INVALID and b"apodize" in err()
        assert call(*ok[:7], 2, *ok[8:], fake(2), need, None) == _lib.INR_E_INVALID and b"align must be" in err()
        assert call(*ok[:8], 2, ok[9], fake(2), need, None) == _lib.INR_E_INVALID and b"boundary must be" in err()
        # the mirror rule of align 'sample': (2n - 2) m divisible by n, per axis; 'center' and the periodic boundary take the pair
        odd = (fake(0), fake(1), 0, 25, 19, 30, 38)
        assert call(*odd, S, M, 0.0, fake(2), need, None) == _lib.INR_E_INVALID and b"divisible by n (got 25 -> 30)" in err()
        assert call(*odd[:3], 19, 25, 38, 30, S, M, 0.0, fake(2), need, None) == _lib.INR_E_INVALID and b"(got 25 -> 30)" in err()
        assert call(*odd[:3], 1, 19, 4, 38, S, M, 0.0, fake(2), need, None) == _lib.INR_E_INVALID and b"n >= 2" in err()
        assert call(*odd, C, M, 0.0, fake(2), need, None) == 0 and call(*odd, S, P, 0.0, fake(2), need, None) == 0      # n_images = 0
        assert call(*odd[:3], 1, 19, 1, 38, S, M, 0.5, fake(2), need, None) == 0                    # a 1 -> 1 axis passes through
        # one double too few, no workspace, a misaligned one: refused before any device work
        assert call(*ok, fake(2), need - 1, None) == _lib.INR_E_WORKSPACE and b"workspace too small" in err()
        assert call(*ok, None, need, None) == _lib.INR_E_WORKSPACE
        assert call(*ok, ctypes.c_void_p(0x7000_0000_0008), need, None) == _lib.INR_E_ALIGN and b"16-byte aligned" in err()
        # n_images = 0 succeeds and launches nothing
        assert call(fake(0), fake(1), 0, *ok[3:], fake(2), need, None) == 0

    op = lib.inr_fourier_operator
    assert op(None, 8, 16, S, M, 0.0, None) == _lib.INR_E_INVALID and b"null pointer" in lib.inr_last_error()
    assert op(fake(0), 0, 16, S, M, 0.0, None) == _lib.INR_E_INVALID and b"bad sizes" in lib.inr_last_error()
    assert op(fake(0), 8, 1025, S, M, 0.0, None) == _lib.INR_E_INVALID and b"lines of at most" in lib.inr_last_error()
    assert op(fake(0), 8, 16, 3, M, 0.0, None) == _lib.INR_E_INVALID and b"align must be" in lib.inr_last_error()
    assert op(fake(0), 8, 16, S, -1, 0.0, None) == _lib.INR_E_INVALID and b"boundary must be" in lib.inr_last_error()
    assert op(fake(0), 8, 16, S, M, 2.0, None) == _lib.INR_E_INVALID and b"apodize" in lib.inr_last_error()
    assert op(fake(0), 25, 30, S, M, 0.0, None) == _lib.INR_E_INVALID and b"divisible by n" in lib.inr_last_error()
    assert op(fake(0), 1, 1, S, M, 0.0, None) == _lib.INR_E_INVALID and b"n >= 2" in lib.inr_last_error()      # no mirrored line of one sample


def test_python_entry_points_refuse_by_name():
    img = np.ones((25, 25))
    calls = {"fourier_resize": lambda **kw: baselines.fourier_resize(img, (50, 50), **kw),
             "fourier_rescale": lambda **kw: baselines.fourier_rescale(img, 2, **kw),
             "fourier_resample": lambda **kw: baselines.fourier_resample(img, 50, **kw),
             "fourier_operator": lambda **kw: baselines.fourier_operator(25, 50, **kw)}
    for name, fn in calls.items():
        with pytest.raises(ValueError, match=f"{name}: align must be 'sample' or 'center'.*'corner'"):
            fn(align="corner")
        with pytest.raises(ValueError, match=f"{name}: boundary must be 'periodic' or 'mirror'.*'edge'"):
            fn(boundary="edge")
        with pytest.raises(ValueError, match=f"{name}: apodize must be in \\[0, 1\\].*1.5"):
            fn(apodize=1.5)
    for name, fn in {"fourier_resize": lambda: baselines.fourier_resize(img, (30, 50)),
                     "fourier_rescale": lambda: baselines.fourier_rescale(img, 1.2),
                     "fourier_resample": lambda: baselines.fourier_resample(img, 30, axis=0),
                     "fourier_operator": lambda: baselines.fourier_operator(25, 30)}.items():
        with pytest.raises(ValueError, match=f"{name}: boundary='mirror' with align='sample' needs.*25 -> 30"):
            fn()
    with pytest.raises(ValueError, match="fourier_resize: lines of at most 1024"):
        baselines.fourier_resize(img, (2048, 50))
    with pytest.raises(ValueError, match="fourier_resize: output_shape"):
        baselines.fourier_resize(img, (50,))
    with pytest.raises(ops.InrDeviceError, match="fourier_resize.*no CPU fallback"):
        baselines.fourier_resize(torch.ones(25, 25), (50, 50))
    with pytest.raises(ops.InrDeviceError, match="fourier_resample"):
        baselines.fourier_resample(torch.ones(25), 50)
    with pytest.raises(TypeError, match="fourier_resize takes an ndarray or a device tensor"):
        baselines.fourier_resize([[1.0, 2.0], [3.0, 4.0]], (4, 4))
    with pytest.raises(TypeError, match="fourier_rescale takes an ndarray or a device tensor.*list"):
        baselines.fourier_rescale([[1.0, 2.0], [3.0, 4.0]], 2)
    with pytest.raises(TypeError, match="fourier_resample takes an ndarray or a device tensor.*list"):
        baselines.fourier_resample([1.0, 2.0, 3.0, 4.0], 8)
    with pytest.raises(TypeError, match="fourier_resample takes an ndarray or a device tensor.*float"):
        baselines.fourier_resample(3.0, 8)
    # the baselines beside it keep their contracts
    with pytest.raises(ValueError, match="only kind='cubic'"):
        baselines.resize_z(np.ones((4, 4, 8)), 16, kind="fourier")
    with pytest.raises(ValueError, match="only up-scaling"):
        baselines.rescale(img, 0.5)


def test_driver_flag_defaults_off_and_refuses_what_it_cannot_serve(tmp_path):
    """Refused while checking the input, before any device work."""
    args = dwi_script.build_parser().parse_args(["--data", "x.mat"])
    assert args.zerofill is False and args.zerofill_apodize == 0.0
    path = str(tmp_path / "pat03_vol.mat")
    matio.savemat(path, {"vol": np.random.default_rng(0).random((20, 20, 2)) + 0.5})
    run = lambda r1, *flags: dwi_script.main(["--data", path, "--output_address", str(tmp_path / "res"), "--number_of_epochs", "1",
                                              "--hidden_dim", "16", "--num_layers", "1", "--mapping_size", "8", "--roi_start", "2",
                                              "--roi_end", str(r1), *flags])
    with pytest.raises(ValueError, match="--zerofill.*even ROI side.*15"):
        run(17, "--zerofill")
    with pytest.raises(ValueError, match="--zerofill_apodize must be in \\[0, 1\\]"):
        run(18, "--zerofill", "--zerofill_apodize", "1.5")
