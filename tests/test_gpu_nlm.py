"""inr_nlm3d / inr_nlm_upsample (csrc/nlm.hip) on the device against the float64 restatement of tests/nlm_common.py: the
output within 32 d_ref, d_ref the deviation between the restatement's two summation orders, under the preconditions that keep the
definition continuous; the bits across runs, streams, grid caps, batch positions, the fp32 twin and the equivalent ways to state one
problem; pass-through and NaN voxels; what the entry points write; the upsampling against the restated solve and against its public
pieces alternated by hand; the Python layer and the drivers.  Every test prints what it measured before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

from tests import nlm_common as N
from tests.guard_common import POISON, Guarded, same_bits
from mri_super_resolution_amd import _lib, baselines, denoise, matio, ops
from mri_super_resolution_amd.scripts import denoise as denoise_script
from mri_super_resolution_amd.scripts import superresDWI as dwi_script
from mri_super_resolution_amd.scripts import through_plane as through_plane_script

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=torch.float64):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(DEV).to(dtype)


def _inputs(name, member=0, dtype=torch.float64):
    """(x [1, C, D, H, W], kwargs of ops.nlm3d) of a case on the device."""
    c = N.case(name, member)
    h2 = c["h2"] if np.isscalar(c["h2"]) else _dev(c["h2"][None], dtype)
    return _dev(c["x"][None], dtype), dict(h2=h2, search=c["search"], patch=c["patch"], guide=_dev(c["guide"][None], dtype),
                                           sigma2=_dev(None if c["sigma2"] is None else c["sigma2"][None], dtype))


def _parity(what, got, name, center="max", member=0):
    ref, d_ref, info = N.reference(name, center, member)
    c = N.case(name, member)
    if center == "max":
        assert info["wmax"].min() >= N.WMAX_FLOOR
    if c["sigma2"] is not None:
        assert (info["m"] - 2.0 * c["sigma2"]).min() >= N.RICIAN_FLOOR
    err = float(np.abs(got - ref).max())
    print(f"{what} {name} center {center}: max |out - ref| {err:.2e}, d_ref {d_ref:.2e}, bound {N.BOUND_FACTOR * d_ref:.2e}, smallest wmax "
          f"{info['wmax'].min():.2e}")
    assert err <= N.BOUND_FACTOR * d_ref


@pytest.mark.parametrize("name", N.CASE_IDS)
def test_the_filter_matches_the_restatement(name):
    x, kw = _inputs(name)
    _parity("nlm3d", ops.nlm3d(x, **kw)[0].cpu().numpy(), name)


def test_both_centre_weights_match_the_restatement():
    x, kw = _inputs("1-small-odd")
    for center in ("max", "one"):
        _parity("nlm3d", ops.nlm3d(x, center=center, **kw)[0].cpu().numpy(), "1-small-odd", center)


def test_a_batch_of_three_volumes_matches_the_restatement_volume_by_volume():
    name = "3-tiles"
    xs = [_inputs(name, m) for m in range(3)]
    x = torch.cat([v[0] for v in xs])
    out = ops.nlm3d(x, xs[0][1]["h2"], xs[0][1]["search"], xs[0][1]["patch"], torch.cat([v[1]["guide"] for v in xs]))
    for m in range(3):
        _parity(f"batch member {m}", out[m].cpu().numpy(), name, member=m)


@pytest.mark.parametrize("name", ("1-small-odd", "3-tiles", "6-rician-mean-guide"))
def test_the_bits_do_not_depend_on_the_run_the_stream_the_grid_or_the_place_in_the_batch(name):
    x, kw = _inputs(name)
    first = ops.nlm3d(x, **kw)
    verdict = {"again": same_bits(first, ops.nlm3d(x, **kw))}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        streamed = ops.nlm3d(x, **kw)
    side.synchronize()
    verdict["side stream"] = same_bits(first, streamed)
    for cap in (1, 3):
        assert _lib.lib().inr_debug_set(32, cap) == 0
        verdict[f"grid cap {cap}"] = same_bits(first, ops.nlm3d(x, **kw))
    assert _lib.lib().inr_debug_set(32, 0) == 0
    other, okw = _inputs(name, 1)
    batch = {k: (torch.cat([okw[k], 0.5 * okw[k], kw[k]]) if isinstance(kw[k], torch.Tensor) else kw[k]) for k in kw}
    inside = ops.nlm3d(torch.cat([other, 0.5 * other, x]), **batch)
    verdict["alone against position 2 of a batch of 3"] = same_bits(first[0], inside[2])
    print(f"{name}: equal bits {verdict}")
    assert all(verdict.values()), verdict


@pytest.mark.parametrize("name", ("1-small-odd", "6-rician-mean-guide"))
def test_the_fp32_entry_is_the_fp64_entry_on_the_same_values_rounded_once(name):
    x, kw = _inputs(name, dtype=torch.float32)
    up = {k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    got, want = ops.nlm3d(x, **kw), ops.nlm3d(x.double(), **up).float()
    print(f"{name}: fp32 entry equals the rounded fp64 entry: {same_bits(got, want)}")
    assert got.dtype == torch.float32 and same_bits(got, want)


def test_equivalent_statements_of_one_problem_give_the_same_bits():
    x, kw = _inputs("1-small-odd")
    null_guide = ops.nlm3d(x, kw["h2"], kw["search"], kw["patch"], None)
    verdict = {"guide = x against a null guide": same_bits(ops.nlm3d(x, **kw), null_guide)}
    x2, kw2 = _inputs("2-image")
    flat = ops.nlm3d(x2, **kw2)
    full = ops.nlm3d(x2, kw2["h2"], (3, 3, 3), (1, 1, 1), kw2["guide"])
    verdict["an image under (3, 3, 3) / (1, 1, 1) against (0, 3, 3) / (0, 1, 1)"] = same_bits(flat, full)
    verdict["search 0 returns the input"] = same_bits(ops.nlm3d(x, kw["h2"], 0, kw["patch"], kw["guide"]), x)
    print(f"equal bits {verdict}")
    assert all(verdict.values()), verdict


def test_masked_voxels_and_voxels_without_a_positive_strength_are_copied():
    x, kw = _inputs("3-tiles")
    shape = tuple(x.shape[2:])
    plain = ops.nlm3d(x, **kw)
    mask = torch.ones((1,) + shape, dtype=torch.uint8, device=DEV)
    mask[:, :, :5] = 0
    mask[:, 4:] = 0
    masked = ops.nlm3d(x, mask=mask, **kw)
    inside = mask[0] != 0
    verdict = {"x outside the mask": same_bits(masked[0, 0][~inside], x[0, 0][~inside]),
               "the unmasked run inside it": same_bits(masked[0, 0][inside], plain[0, 0][inside]),
               "a bool mask": same_bits(ops.nlm3d(x, mask=mask.bool(), **kw), masked)}
    h2 = torch.full((1,) + shape, N.H2, dtype=torch.float64, device=DEV)
    h2[0, 0, 0, 0], h2[0, 3, 7, 9], h2[0, 8, 18, 20], h2[0, 4, 8, 8] = 0.0, -1.0, float("nan"), float("-inf")
    kwm = dict(kw, h2=h2)
    mapped = ops.nlm3d(x, **kwm)
    off = ~(h2[0] > 0)
    verdict["x where h2 is zero, negative or NaN"] = int(off.sum()) == 4 and same_bits(mapped[0, 0][off], x[0, 0][off])
    verdict["the scalar run elsewhere"] = same_bits(mapped[0, 0][~off], plain[0, 0][~off])
    print(f"equal bits {verdict}")
    assert all(verdict.values()), verdict


def test_nans_in_the_input_stay_where_the_definition_puts_them():
    c = N.case("1-small-odd")
    x = np.array(c["x"])
    for p in ((0, 0, 0), (2, 5, 6), (4, 10, 12), (1, 3, 11), (3, 8, 2)):
        x[(0,) + p] = np.nan
    ref = N.nlm(x, x[0], c["search"], c["patch"], N.H2)
    expected = np.isnan(ref)
    xd = _dev(x[None])
    got = ops.nlm3d(xd, N.H2, c["search"], c["patch"], None)            # the call returns 0: ops.nlm3d raises otherwise
    torch.cuda.synchronize()
    got = got[0].cpu().numpy()
    nan = np.isnan(got)
    clean = ~expected
    err = float(np.abs(got - ref)[clean].max()) if clean.any() else 0.0
    _, d_ref, _ = N.reference("1-small-odd")
    print(f"NaN voxels: {int(nan.sum())} in the output, {int(expected.sum())} by the definition, {int((nan & ~expected).sum())} outside them, "
          f"{int(clean.sum())} clean voxels with max |out - ref| {err:.2e} (bound {N.BOUND_FACTOR * d_ref:.2e})")
    assert not (nan & ~expected).any()
    assert err <= N.BOUND_FACTOR * d_ref


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32))
def test_the_filter_writes_all_of_out_and_nothing_else(dtype):
    x, kw = _inputs("6-rician-mean-guide", dtype=dtype)
    want = ops.nlm3d(x, **kw)
    out = Guarded(tuple(x.shape), dtype)
    s, r = kw["search"], kw["patch"]
    entry = "inr_nlm3d" if dtype == torch.float64 else "inr_nlm3d_f32"
    rc = getattr(_lib.lib(), entry)(out.ptr, x.data_ptr(), kw["guide"].data_ptr(), 0.0, kw["h2"].data_ptr(), kw["sigma2"].data_ptr(), None,
                                    *x.shape, *s, *r, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.lib().inr_last_error()
    print(f"{entry}: guards intact {out.intact()}, written {out.written()}, equals the wrapper {same_bits(out.view, want)}")
    assert out.intact() and out.written() and same_bits(out.view, want)


# ---- the upsampling ---------------------------------------------------------------------------------------------------------------------
def _up_call(entry, out, change, y, x0, guide, f, k, levels, n_iter, relax, s, r, ws_ptr, ws_doubles):
    arr = lambda v: ops._doubles(float(t) for t in v)
    n, d, h, w = y.shape
    return getattr(_lib.lib(), entry)(out, change, y.data_ptr(), ops._ptr(x0), ops._ptr(guide), n, d * f[0], h * f[1], w * f[2], *f,
                                      *(arr(t) for t in k), arr(levels), len(levels), n_iter, relax, *s, *r, ws_ptr, ws_doubles,
                                      torch.cuda.current_stream().cuda_stream)


def _by_hand(lr, factors, kernel, levels, n_iter, search, patch, relax=1.0, guide=None):
    """The solve from the public pieces: ops.nlm3d, then the correction built from block_apply3d; change restated in the kernel's order."""
    x = lr.repeat_interleave(factors[0], 1).repeat_interleave(factors[1], 2).repeat_interleave(factors[2], 3)
    change = []
    for h in levels:
        for _ in range(n_iter):
            xp = ops.nlm3d(x[:, None], h * h, search, patch, None if guide is None else guide, center="one")[:, 0]
            res = ops.block_apply3d(xp, factors, kernel) - lr
            rep = res.repeat_interleave(factors[0], 1).repeat_interleave(factors[1], 2).repeat_interleave(factors[2], 3)
            new = xp - relax * rep
            change.append([N.change_in_kernel_order(a, b, factors) for a, b in zip(new.cpu().numpy(), x.cpu().numpy())])
            x = new
    return x, np.array(change)


def test_the_upsampling_matches_the_restated_solve():
    u = N.UPSAMPLE
    lr, _ = N.upsample_case()
    (ref, ref_change), d_x, d_change = N.upsample_reference()
    assert d_x <= 1e-12
    out, info = baselines.nlm_upsample(lr, u["factors"], "mean", u["levels"], u["n_iter"], u["search"], u["patch"], return_info=True)
    err, cerr = float(np.abs(out - ref).max()), float(np.abs(info["change"] - ref_change).max())
    res = float(np.abs(N.block_apply(out, u["factors"], N.kernel_table(*N.named_kernel("mean", u["factors"]))) - lr).max())
    bound_res = 4 * (np.prod(u["factors"]) + 2) * N.EPS * float(np.abs(out).max())
    print(f"upsample: max |x - ref| {err:.2e} (d_ref {d_x:.2e}, bound {N.BOUND_FACTOR * d_x:.2e}); change {info['change']}, max deviation "
          f"{cerr:.2e} (d_ref {d_change:.2e}, bound {N.BOUND_FACTOR * max(d_change, N.EPS * ref_change.max()):.2e}); |A x - lr| {res:.2e} "
          f"(bound {bound_res:.2e})")
    assert out.dtype == np.float64 and info["change"].shape == (4,)
    assert err <= N.BOUND_FACTOR * d_x
    assert cerr <= N.BOUND_FACTOR * max(d_change, N.EPS * ref_change.max())     # a mean of 2,688 terms: at least its own eps
    assert res <= bound_res


@pytest.mark.parametrize("fixed_guide", (False, True))
def test_the_upsampling_is_its_public_pieces_alternated_by_hand_bit_for_bit(fixed_guide):
    u = N.UPSAMPLE
    lr_np, truth = N.upsample_case()
    lr = torch.cat([_dev(lr_np[None]), _dev(0.5 * lr_np[None] + 0.1)])
    k = [t.tolist() for t in N.named_kernel("mean", u["factors"])]
    guide = torch.cat([_dev(truth[None]), _dev(truth[None] ** 2)]) if fixed_guide else None
    want, want_change = _by_hand(lr, u["factors"], k, u["levels"], u["n_iter"], u["search"], u["patch"], guide=guide)
    got, change = ops.nlm_upsample(lr, u["factors"], k, u["levels"], u["n_iter"], u["search"], u["patch"], guide=guide)
    verdict = {"x": same_bits(got, want), "change": change.cpu().numpy().tobytes() == want_change.tobytes()}
    print(f"fixed guide {fixed_guide}: equal bits {verdict}; change {change.cpu().numpy().tolist()}")
    assert all(verdict.values()), verdict


@pytest.mark.parametrize("factors", ((2, 1, 1), (1, 2, 2)))
@pytest.mark.parametrize("kind", ("gaussian", "decimate"))
def test_the_mean_correction_restores_the_data_under_other_operators(factors, kind):
    rng = np.random.default_rng(11)
    hr = (8, 12, 14)
    truth = N.phantom(hr)
    if kind == "gaussian":
        k = [baselines.slice_profile(factors[0], "gaussian", fwhm=1.0).tolist()] + [np.full(f, 1.0 / f).tolist() for f in factors[1:]]
    else:
        k = [t.tolist() for t in N.named_kernel("decimate", factors)]
    ks = N.kernel_table(*k)
    lr = N.block_apply(truth, factors, ks) + 0.01 * rng.standard_normal(tuple(s // f for s, f in zip(hr, factors)))
    A = lambda v: N.block_apply(v, factors, ks)
    full, _ = ops.nlm_upsample(_dev(lr[None]), factors, k, (0.0625,), 1, 2, 1)
    full = full[0].cpu().numpy()
    bound = 4 * (np.prod(factors) + 2) * N.EPS * float(np.abs(full).max())
    res = float(np.abs(A(full) - lr).max())
    # relax = 0.5 from the same start: the filtered x' is the same, so the residual of the result is half that of x'
    half, _ = ops.nlm_upsample(_dev(lr[None]), factors, k, (0.0625,), 1, 2, 1, relax=0.5)
    half = half[0].cpu().numpy()
    xp = ops.nlm3d(_dev(N.replicate(lr, factors)[None, None]), 0.0625 ** 2, 2, 1, center="one")[0, 0].cpu().numpy()
    dev = float(np.abs((A(half) - lr) - 0.5 * (A(xp) - lr)).max())
    print(f"factors {factors} {kind}: |A x - lr| {res:.2e} at relax 1, |r(relax 0.5) - r(x') / 2| {dev:.2e}, bound {bound:.2e}, |r(x')| "
          f"{np.abs(A(xp) - lr).max():.2e}")
    assert res <= bound and dev <= bound


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32))
def test_the_upsampling_writes_out_and_change_and_stays_inside_its_workspace(dtype):
    u = N.UPSAMPLE
    lr_np, _ = N.upsample_case()
    y = torch.cat([_dev(lr_np[None], dtype), _dev(0.5 * lr_np[None], dtype)])
    f, s, r = u["factors"], u["search"], u["patch"]
    k = [t.tolist() for t in N.named_kernel("mean", f)]
    hr = tuple(a * b for a, b in zip(u["lr_shape"], f))
    entry = "inr_nlm_upsample" if dtype == torch.float64 else "inr_nlm_upsample_f32"
    need = ops.nlm_upsample_workspace_doubles(2, *hr, f)
    want, want_change = ops.nlm_upsample(y, f, k, u["levels"], u["n_iter"], s, r)
    results = []
    for fill in (0x00, POISON):
        ws, out, change = Guarded(need * 8, torch.uint8, fill), Guarded((2,) + hr, dtype), Guarded((4, 2), torch.float64)
        rc = _up_call(entry, out.ptr, change.ptr, y, None, None, f, k, u["levels"], u["n_iter"], 1.0, s, r, ws.ptr, need)
        assert rc == 0, _lib.lib().inr_last_error()
        assert ws.intact() and out.intact() and change.intact() and out.written() and change.written()
        results.append((out, change))
    lone = Guarded((2,) + hr, dtype)
    ws = Guarded(need * 8, torch.uint8, POISON)
    assert _up_call(entry, lone.ptr, None, y, None, None, f, k, u["levels"], u["n_iter"], 1.0, s, r, ws.ptr, need) == 0
    verdict = {"the workspace's earlier contents do not matter": same_bits(results[0][0].view, results[1][0].view)
               and same_bits(results[0][1].view, results[1][1].view),
               "the wrapper": same_bits(results[0][0].view, want) and same_bits(results[0][1].view, want_change),
               "a null change leaves out alone": lone.intact() and ws.intact() and same_bits(lone.view, want)}
    print(f"{entry}: workspace of {need} doubles; equal bits {verdict}")
    assert all(verdict.values()), verdict
    # no passes: out is the start, rounded once; nothing is written to change
    none = Guarded((2,) + hr, dtype)
    assert _up_call(entry, none.ptr, None, y, None, None, f, k, (), 3, 1.0, s, r, ws.ptr, need) == 0
    rep = y.repeat_interleave(f[0], 1).repeat_interleave(f[1], 2).repeat_interleave(f[2], 3)
    assert none.intact() and same_bits(none.view, rep)


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
def test_denoise_nlm_serves_every_layout_and_type():
    c = N.case("6-rician-mean-guide")
    x, sigma = np.array(c["x"]), np.array(c["sigma"])
    s, r = c["search"], c["patch"]
    # guide = 'mean', a sigma map, Rician: the case itself
    out = denoise.nlm(x, sigma, beta=1.0 / 3.0, search=s, patch=r, guide="mean", rician=True)
    ref, d_ref, _ = N.reference("6-rician-mean-guide")
    err = float(np.abs(out - ref).max())
    print(f"guide='mean': ndarray in -> {out.dtype} {out.shape}, max |out - ref| {err:.2e} (bound {2 * N.BOUND_FACTOR * d_ref:.2e})")
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == x.shape
    assert err <= 2 * N.BOUND_FACTOR * d_ref         # h2 = 2 beta sigma^2 and the mean are formed on the device: one rounding each more
    xd = _dev(x)
    verdict = {}
    for dtype in (torch.float64, torch.float32):
        t = denoise.nlm(xd.to(dtype), sigma, beta=1.0 / 3.0, search=s, patch=r, guide="mean", rician=True)
        verdict[f"{dtype} tensor comes back as given"] = t.dtype == dtype and t.is_cuda and t.shape == xd.shape
    verdict["the fp64 tensor equals the ndarray"] = np.array_equal(denoise.nlm(xd, sigma, 1.0 / 3.0, s, r, "mean", True).cpu().numpy(), out)
    # no guide: each volume guides itself, leading axes are a batch
    own = denoise.nlm(xd.reshape(3, 1, 4, 14, 15), 0.03, search=s, patch=r)
    each = torch.stack([ops.nlm3d(xd[i][None, None], 2 * 0.03 ** 2, s, r)[0] for i in range(3)])
    verdict["leading axes are a batch"] = own.shape == (3, 1, 4, 14, 15) and same_bits(own, each)
    # an array guide shared by all, and a mask
    g = xd.mean(dim=0)
    mask = np.ones((4, 14, 15), np.uint8)
    mask[:, :4] = 0
    shared = denoise.nlm(xd, 0.03, search=s, patch=r, guide=g, mask=mask)
    direct = ops.nlm3d(xd[None], 2 * 0.03 ** 2, s, r, g[None], mask=_dev(mask[None], torch.uint8))[0]
    verdict["an array guide and a mask"] = same_bits(shared, direct)
    # an image is D = 1
    img = xd[0, 2]
    flat = denoise.nlm(img, 0.03, search=3, patch=1)
    verdict["an image is D = 1"] = flat.shape == img.shape and same_bits(flat, ops.nlm3d(img[None, None, None], 2 * 0.03 ** 2, (0, 3, 3), (0, 1, 1))[0, 0, 0])
    print(f"layouts and types: {verdict}")
    assert all(verdict.values()), verdict


def test_baselines_nlm_upsample_serves_every_layout_and_type():
    u = N.UPSAMPLE
    lr, truth = N.upsample_case()
    args = (u["factors"], "mean", u["levels"], u["n_iter"], u["search"], u["patch"])
    out, info = baselines.nlm_upsample(lr, *args, return_info=True)
    stack = np.stack([lr, 0.5 * lr + 0.1]).reshape(2, 1, *lr.shape)
    both, binfo = baselines.nlm_upsample(stack, *args, return_info=True)
    verdict = {"leading axes are a batch": both.shape == (2, 1) + truth.shape and np.array_equal(both[0, 0], out)
               and binfo["change"].shape == (4, 2, 1) and np.array_equal(binfo["change"][:, 0, 0], info["change"])}
    for dtype in (torch.float64, torch.float32):
        t = baselines.nlm_upsample(_dev(lr, dtype), *args)
        verdict[f"{dtype} tensor comes back as given"] = t.dtype == dtype and t.is_cuda and tuple(t.shape) == truth.shape
    verdict["the fp64 tensor equals the ndarray"] = np.array_equal(baselines.nlm_upsample(_dev(lr), *args).cpu().numpy(), out)
    start = N.replicate(lr, u["factors"])
    verdict["x0 = the replication is the default start"] = np.array_equal(baselines.nlm_upsample(lr, *args, x0=start), out)
    guided = baselines.nlm_upsample(lr, *args, guide=truth)
    verdict["a guide changes the result and keeps the data"] = not np.array_equal(guided, out) and float(
        np.abs(N.block_apply(guided, u["factors"], N.kernel_table(*N.named_kernel("mean", u["factors"]))) - lr).max()) <= 40 * N.EPS
    print(f"layouts and types: {verdict}; RMSE against the phantom: replication {N.rmse(start, truth):.4f}, nlm {N.rmse(out, truth):.4f}, "
          f"guided by the truth {N.rmse(guided, truth):.4f}")
    assert all(verdict.values()), verdict


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------
TIMINGS = ("t_fit_s", "t_recon_s", "train_voxels_per_s", "output")


def _files(d):
    return {name: open(os.path.join(d, name), "rb").read() for name in sorted(os.listdir(d))}


def test_through_plane_gains_the_nlm_method_and_nothing_else_changes(tmp_path):
    rng = np.random.default_rng(4)
    vol = np.stack([N.phantom((24, 24, 8)) * s for s in (1.0, 0.6)], axis=-1) * 800.0 + 4.0 * rng.standard_normal((24, 24, 8, 2))
    path = str(tmp_path / "pat31_vol.mat")
    matio.savemat(path, {"vol": np.abs(vol), "b": np.array([0.0, 1000.0])})
    common = ["--data", path, "--roi_start", "2", "--roi_end", "22", "--tv_iters", "20"]
    runs = {}
    for name, extra in (("plain", []), ("defaults", ["--nlm_start", "replicate", "--nlm_iters", "2", "--nlm_search", "2", "--nlm_patch", "1"]),
                        ("nlm", ["--with_nlm"]), ("spline", ["--with_nlm", "--nlm_start", "spline", "--nlm_iters", "1"])):
        out = str(tmp_path / name)
        through_plane_script.main(common + extra + ["--output_address", out])
        runs[name] = _files(os.path.join(out, "pat31"))
    plain, nlm = runs["plain"], runs["nlm"]
    mp, mn, ms = (json.loads(runs[k]["metrics.json"]) for k in ("plain", "nlm", "spline"))
    added = set(mn) - set(mp)
    print(f"through_plane --with_nlm: keys added {sorted(added)}; PSNR replicate {mn['psnr_replicate_db']:.2f}, spline {mn['psnr_spline_db']:.2f}, "
          f"tv3d {mn['psnr_tv3d_db']:.2f}, nlm {mn['psnr_nlm_db']:.2f} (from the spline, 1 pass per level: {ms['psnr_nlm_db']:.2f}); consistency "
          f"{mn['nlm_consistency_psnr_db']:.1f} dB")
    assert runs["defaults"] == plain                                            # every file, byte for byte
    assert sorted(nlm) == sorted(plain)
    assert added == {"psnr_nlm_db", "ssim_nlm_mean", "nlm_consistency_psnr_db", "nlm_start", "nlm_iters", "nlm_search", "nlm_patch"}
    assert {k: v for k, v in mn.items() if k not in added} == mp
    rows_p, rows_n = (runs[k]["through_plane.csv"].decode().splitlines() for k in ("plain", "nlm"))
    assert rows_n[0] == rows_p[0] + ", SSIM-nlm" and all(a.rsplit(", ", 1)[0] == b for a, b in zip(rows_n, rows_p))
    mat_p, mat_n = matio.loadmat(str(tmp_path / "plain" / "pat31" / "through_plane.mat")), matio.loadmat(str(tmp_path / "nlm" / "pat31" / "through_plane.mat"))
    keys = lambda m: {k for k in m if not k.startswith("__")}
    assert keys(mat_n) - keys(mat_p) == {"nlm"} and all(np.array_equal(mat_p[k], mat_n[k]) for k in keys(mat_p))
    assert mn["nlm_consistency_psnr_db"] > 100 and mn["psnr_nlm_db"] > mn["psnr_replicate_db"]      # fp32 data: A nlm = thick to rounding
    assert ms["nlm_start"] == "spline" and ms["nlm_iters"] == 1 and ms["psnr_nlm_db"] != mn["psnr_nlm_db"]


def test_the_denoise_script_with_method_nlm_filters_the_raw_stack_under_the_mppca_noise_map(tmp_path):
    from tests.test_gpu_mppca import _master
    src = str(tmp_path / "pat011_master.mat")
    cell, clean_cell = _master(src)
    stack, truth = denoise.stack_hybrid(cell), denoise.stack_hybrid(clean_cell)
    _, info = denoise.mppca(stack, (5, 5, 3), return_info=True)
    base = ["--data", src, "--window", "5", "5", "3"]
    plain = denoise_script.main(base + ["--out", str(tmp_path / "plain.mat")])
    default = denoise_script.main(base + ["--out", str(tmp_path / "default.mat"), "--method", "mppca", "--nlm_beta", "1.0", "--nlm_search", "3",
                                          "--nlm_patch", "1"])
    flagged = denoise_script.main(base + ["--out", str(tmp_path / "nlm.mat"), "--method", "nlm"])
    tuned = denoise_script.main(base + ["--out", str(tmp_path / "tuned.mat"), "--method", "nlm", "--nlm_beta", "0.5", "--nlm_search", "2",
                                        "--nlm_rician"])
    saved = {k: matio.loadmat(str(tmp_path / f"{k}.mat")) for k in ("plain", "nlm", "tuned")}
    got = denoise.stack_hybrid(saved["nlm"]["hybrid_raw_clean"])
    before, after, mppca_after = N.rmse(stack, truth), N.rmse(got, truth), N.rmse(denoise.stack_hybrid(saved["plain"]["hybrid_raw_clean"]), truth)
    print(f"scripts/denoise.py --method nlm: keys added {sorted(set(flagged) - set(plain))}; RMSE against the clean cell {before:.3f} -> "
          f"{after:.3f} (MP-PCA: {mppca_after:.3f}), sigma median {flagged['sigma_median']:.3f} (noise 2.0)")
    assert open(tmp_path / "plain.mat", "rb").read() == open(tmp_path / "default.mat", "rb").read()
    assert {k: v for k, v in plain.items() if k != "output"} == {k: v for k, v in default.items() if k != "output"}
    assert set(flagged) - set(plain) == {"method", "nlm_beta", "nlm_search", "nlm_patch", "nlm_rician"}
    assert {k: v for k, v in flagged.items() if k in plain and k != "output"} == {k: v for k, v in plain.items() if k != "output"}
    assert got.tobytes() == denoise.nlm_stack(stack, info["sigma"]).tobytes()
    assert denoise.stack_hybrid(saved["tuned"]["hybrid_raw_clean"]).tobytes() == denoise.nlm_stack(stack, info["sigma"], 0.5, 2, 1, True).tobytes()
    for key in ("sigma", "rank", "b", "TE", "hybrid_raw"):
        a, b = saved["plain"][key], saved["nlm"][key]
        assert (denoise.stack_hybrid(a).tobytes() == denoise.stack_hybrid(b).tobytes()) if key == "hybrid_raw" else a.tobytes() == b.tobytes()
    assert after < before
    # a plain volume [X, Y, Z, B] is filtered along its last axis
    vol = np.abs(np.moveaxis(stack[:6], 0, -1)).copy()
    path = str(tmp_path / "pat012_vol.mat")
    matio.savemat(path, {"hybrid_raw": vol})
    denoise_script.main(["--data", path, "--out", str(tmp_path / "vol.mat"), "--window", "3", "3", "1", "--method", "nlm"])
    sig = denoise.mppca(vol, (3, 3, 1), return_info=True, measurement_axis=-1)[1]["sigma"]
    want = np.moveaxis(denoise.nlm_stack(np.ascontiguousarray(np.moveaxis(vol, -1, 0)), sig), 0, -1)
    assert np.array_equal(matio.loadmat(str(tmp_path / "vol.mat"))["hybrid_raw_clean"], want)


def test_superresDWI_gains_the_nlm_baseline_and_the_nlm_denoiser_and_is_what_it_was_without_them(tmp_path):
    rng = np.random.default_rng(3)
    gx, gy, gz = np.meshgrid(np.linspace(0, 1, 32), np.linspace(0, 1, 32), np.linspace(0, 1, 2), indexing="ij")
    vol = np.stack([500 * (1.2 + np.sin(3 * gx + gz) * np.cos(2 * gy) + (gx > 0.4)) * np.exp(-0.7 * b) for b in range(4)], axis=-1)
    vol = vol + 10.0 * rng.standard_normal(vol.shape)
    path = str(tmp_path / "pat068_vol.mat")
    matio.savemat(path, {"vol": vol, "b": np.array([0.0, 150.0, 1000.0, 1500.0])})
    common = ["--data", path, "--number_of_epochs", "5", "--hidden_dim", "128", "--num_layers", "2", "--mapping_size", "32", "--roi_start", "2",
              "--roi_end", "30", "--seed", "0", "--adc"]
    runs = {}
    for name, extra in (("plain", []), ("defaults", ["--denoise", "none", "--nlm_iters", "2", "--nlm_search", "2", "--nlm_patch", "1"]),
                        ("baseline", ["--nlm_baseline", "--nlm_iters", "1"]), ("denoised", ["--denoise", "nlm", "--denoise_window", "3", "3", "1"])):
        out = str(tmp_path / name)
        dwi_script.main(common + extra + ["--output_address", out])
        runs[name] = _files(os.path.join(out, "pat068"))
    metrics_of = lambda k: {a: b for a, b in json.loads(runs[k]["metrics.json"]).items() if a not in TIMINGS}
    plain, base, den = metrics_of("plain"), metrics_of("baseline"), metrics_of("denoised")
    added = set(base) - set(plain)
    print(f"--nlm_baseline: keys added {sorted(added)}, files added {sorted(set(runs['baseline']) - set(runs['plain']))}; PSNR spline "
          f"{base['psnr_spline_db']:.2f}, nlm {base['psnr_nlm_db']:.2f}, consistency {base['nlm_consistency_psnr_db']:.1f} dB; --denoise nlm: "
          f"keys added {sorted(set(den) - set(plain))}, sigma median {den['denoise_sigma_median']:.2f} (noise 10)")
    same_files = [k for k in runs["plain"] if k != "metrics.json"]
    assert metrics_of("defaults") == plain and all(runs["defaults"][k] == runs["plain"][k] for k in same_files)
    assert added == {"psnr_nlm_db", "ssim_nlm_mean", "nlm_consistency_psnr_db"} and {k: v for k, v in base.items() if k not in added} == plain
    assert set(runs["baseline"]) - set(runs["plain"]) == {"ssim_scores_nlm.csv"} and not set(runs["plain"]) - set(runs["baseline"])
    assert all(runs["baseline"][k] == runs["plain"][k] for k in same_files if k != "adc.mat")
    adc_p, adc_b = (matio.loadmat(str(tmp_path / k / "pat068" / "adc.mat")) for k in ("plain", "baseline"))
    keys = lambda m: {k for k in m if not k.startswith("__")}
    assert keys(adc_b) - keys(adc_p) == {"adc_nlm"} and all(np.array_equal(adc_p[k], adc_b[k], equal_nan=True) for k in keys(adc_p))
    assert adc_b["adc_nlm"].shape == (28, 28, 2) and base["nlm_consistency_psnr_db"] > 100             # the grid of the HR ROI
    assert runs["baseline"]["ssim_scores_nlm.csv"].decode().splitlines()[0] == "Pt_id, b-value, slice, SSIM-nlm, SSIM-SR"
    assert set(den) - set(plain) == {"denoise", "denoise_window", "denoise_sigma_median"} and den["denoise"] == "nlm"
    assert runs["denoised"]["recon.npy"] != runs["plain"]["recon.npy"]
    # the loader: the raw volume filtered under MP-PCA's noise map, then normalised
    dn = {"window": (3, 3, 1), "method": "nlm"}
    got = dwi_script.load_input_and_scale(path, None, None, dn, None)[0]
    sig = denoise.mppca(vol, (3, 3, 1), return_info=True, measurement_axis=-1)[1]["sigma"]
    want = np.moveaxis(denoise.nlm_stack(np.ascontiguousarray(np.moveaxis(vol, -1, 0)), sig), 0, -1)
    assert np.array_equal(got, want / want.reshape(-1, 4).max(axis=0)) and dn["sigma_median"] == float(np.median(sig))
