"""Every workspace-taking entry point added since tests/test_gpu_workspace_guard.py, held to its plan and to its outputs.

One case per entry point, the protocol of tests/guard_common.py: the C ABI is called directly with a guarded workspace of EXACTLY the
planner's size -- once zeroed, once filled with 0xFF -- and with every output in a guarded buffer of its own that is filled with 0xFF.
Asserted: the return code, every guard, every output element written (finite; integers and bytes off the pre-fill), the two calls
equal bit for bit, and both equal bit for bit to what the public wrapper returns for the same inputs.  Entry points with nullable
arguments get one more call with them null that asserts the guards and the written elements only.  No tolerance appears: every
comparison is bit equality or a byte pattern.  The shapes are the smallest at which a view or a store can still go wrong: a batch of 2
or 3, sides that are no multiple of a workgroup or a tile and, where the workspace holds per-workgroup partials, the smallest shape
of the unit's own "more partials than the finish has threads" test.  Only allocated memory is read and written."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.guard_common import DEV, POISON, guard_case
from mri_super_resolution_amd import _lib, baselines, metrics, ops, perceptual, rams, registration, wire

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
LAM, ALPHA, ITERS = 0.05, 0.02, 3


def stream():
    return torch.cuda.current_stream().cuda_stream


def rnd(*shape, seed, dtype=F64, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=F64) * (hi - lo) + lo).to(DEV, dtype)


def dbl(values):
    values = [float(v) for v in values]
    return (C.c_double * len(values))(*values)


def ptr(t):
    return 0 if t is None else t.data_ptr()


def gp(out, name):
    """The pointer of the guarded output `name`, null where the case passes none."""
    return out[name].ptr if name in out else 0


def case(entry, need, unit, outputs, call, reference):
    return guard_case(entry, int(need) * unit, outputs, call, reference, last_error=_lib.lib().inr_last_error)


def nulls(entry, need, unit, outputs, call):
    return guard_case(entry + " (nullable arguments null)", int(need) * unit, outputs, call, None, fills=(POISON,),
                      last_error=_lib.lib().inr_last_error)


def dtype_of(entry):
    """The twins are named in full in every parametrisation, so a search of this file finds each export."""
    return F32 if entry.endswith("_f32") else F64


def block_kernel(f0, f1, seed=3):
    k = np.random.default_rng(seed).random((f0, f1)) + 0.1
    return (k / k.sum()).tolist()


def flat(kernel):
    return dbl([v for row in kernel for v in row])


# ---- the eight TV / Huber / TGV solver units and the dense-operator unit -----------------------------------------------------------------
@pytest.mark.parametrize("entry", ["inr_tvsr_solve2d", "inr_tvsr_solve2d_f32"])
def test_tvsr_solve2d(entry):
    lib, dtype = _lib.lib(), dtype_of(entry)
    n, H, W, f0, f1 = 3, 6, 10, 3, 2
    k = block_kernel(f0, f1)
    y, w, x0 = rnd(n, H // f0, W // f1, seed=1, dtype=dtype), rnd(n, H // f0, W // f1, seed=2, dtype=dtype), rnd(n, H, W, seed=3, dtype=dtype)
    w[1, 0, 2] = 0
    need = lib.inr_tvsr_workspace_doubles(n, H, W)

    def call(weight, start):
        return lambda ws, o: getattr(lib, entry)(o["out"].ptr, gp(o, "energy"), gp(o, "change"), y.data_ptr(), ptr(weight), ptr(start), n, H, W,
                                                 f0, f1, flat(k), LAM, ALPHA, ITERS, ws.ptr, need, stream())
    outs = {"out": ((n, H, W), dtype), "energy": ((n,), F64), "change": ((n,), F64)}
    ref = ops.tvsr_solve(y, (f0, f1), k, LAM, ALPHA, ITERS, w, x0)
    case(entry, need, 8, outs, call(w, x0), dict(zip(outs, ref)))
    nulls(entry, need, 8, {"out": outs["out"]}, call(None, None))


@pytest.mark.parametrize("entry", ["inr_tgv_solve2d", "inr_tgv_solve2d_f32"])
def test_tgv_solve2d(entry):
    lib, dtype = _lib.lib(), dtype_of(entry)
    n, H, W, f0, f1, ratio = 3, 6, 10, 3, 2, 2.0
    k = block_kernel(f0, f1)
    y, w, x0 = rnd(n, H // f0, W // f1, seed=1, dtype=dtype), rnd(n, H // f0, W // f1, seed=2, dtype=dtype), rnd(n, H, W, seed=3, dtype=dtype)
    w[2, 1, 0] = 0
    need = lib.inr_tgv_workspace_doubles(n, H, W)

    def call(weight, start):
        return lambda ws, o: getattr(lib, entry)(o["out"].ptr, gp(o, "v_out"), gp(o, "energy"), gp(o, "change"), y.data_ptr(), ptr(weight),
                                                 ptr(start), n, H, W, f0, f1, flat(k), LAM, ratio, ALPHA, ITERS, ws.ptr, need, stream())
    outs = {"out": ((n, H, W), dtype), "v_out": ((n, 2, H, W), dtype), "energy": ((n,), F64), "change": ((n,), F64)}
    ref = ops.tgv_solve(y, (f0, f1), k, LAM, ratio, ALPHA, ITERS, w, x0)
    case(entry, need, 8, outs, call(w, x0), dict(zip(outs, ref)))
    nulls(entry, need, 8, {"out": outs["out"]}, call(None, None))


@pytest.mark.parametrize("entry", ["inr_tvj_solve2d", "inr_tvj_solve2d_f32"])
@pytest.mark.parametrize("coupling", ["joint", "none"])
def test_tvj_solve2d(coupling, entry):
    lib, dtype = _lib.lib(), dtype_of(entry)
    n, ch, H, W, f0, f1 = 2, 3, 6, 10, 3, 2
    k, mu = block_kernel(f0, f1), (1.0, 0.5, 0.25)
    y, w = rnd(n, ch, H // f0, W // f1, seed=1, dtype=dtype), rnd(n, ch, H // f0, W // f1, seed=2, dtype=dtype)
    x0 = rnd(n, ch, H, W, seed=3, dtype=dtype)
    w[1, 2, 0, 3] = 0
    need = lib.inr_tvj_workspace_doubles(n, ch, H, W)

    def call(weight, start, weights):
        return lambda ws, o: getattr(lib, entry)(o["out"].ptr, gp(o, "energy"), gp(o, "change"), y.data_ptr(), ptr(weight), ptr(start), n, ch, H,
                                                 W, f0, f1, flat(k), weights, LAM, ALPHA, ops._TVJ_COUPLING[coupling], ITERS, ws.ptr, need,
                                                 stream())
    outs = {"out": ((n, ch, H, W), dtype), "energy": ((n,), F64), "change": ((n,), F64)}
    ref = ops.tvj_solve(y, (f0, f1), k, mu, LAM, ALPHA, coupling, ITERS, w, x0)
    case(f"{entry} ({coupling})", need, 8, outs, call(w, x0, dbl(mu)), dict(zip(outs, ref)))
    nulls(f"{entry} ({coupling})", need, 8, {"out": outs["out"]}, call(None, None, None))


@pytest.mark.parametrize("entry", ["inr_tvadc_solve2d", "inr_tvadc_solve2d_f32"])
@pytest.mark.parametrize("coupling", ["joint", "none"])
def test_tvadc_solve2d(coupling, entry):
    lib, dtype = _lib.lib(), dtype_of(entry)
    n, H, W, f0, f1 = 2, 6, 10, 3, 2
    b, mu, s_max, adc_max, adc0 = (0.0, 500.0, 1000.0), (1.0, 0.5), 2.0, 0.005, 0.001
    k = block_kernel(f0, f1)
    h, w_ = H // f0, W // f1
    s_true, d_true = rnd(n, 1, h, w_, seed=1, lo=0.3, hi=1.0), rnd(n, 1, h, w_, seed=2, lo=0.0005, hi=0.003)
    y = (s_true * torch.exp(-torch.tensor(b, device=DEV, dtype=F64).view(1, 3, 1, 1) * d_true)).to(dtype).contiguous()
    w = rnd(n, 3, h, w_, seed=3, dtype=dtype)
    w[0, 1, 1, 4] = 0
    x0 = torch.stack((rnd(n, H, W, seed=4), rnd(n, H, W, seed=5, hi=0.003)), 1).to(dtype).contiguous()
    need = lib.inr_tvadc_workspace_doubles(n, 3, H, W, f0, f1)

    def call(weight, start, weights):
        return lambda ws, o: getattr(lib, entry)(o["out"].ptr, gp(o, "energy"), gp(o, "change"), y.data_ptr(), ptr(weight), ptr(start), n, 3, H, W,
                                                 f0, f1, flat(k), dbl(b), weights, LAM, ALPHA, ops._TVJ_COUPLING[coupling], ITERS, s_max, adc_max,
                                                 adc0, ws.ptr, need, stream())
    outs = {"out": ((n, 2, H, W), dtype), "energy": ((n,), F64), "change": ((n,), F64)}
    s0, adc, energy, change = ops.tvadc_solve(y, b, (f0, f1), k, mu, LAM, ALPHA, coupling, ITERS, s_max, adc_max, adc0, w, x0)
    case(f"{entry} ({coupling})", need, 8, outs, call(w, x0, dbl(mu)), {"out": torch.stack((s0, adc), 1), "energy": energy, "change": change})
    nulls(f"{entry} ({coupling})", need, 8, {"out": outs["out"]}, call(None, None, None))


@pytest.mark.parametrize("entry", ["inr_tvsr3d_solve", "inr_tvsr3d_solve_f32"])
@pytest.mark.parametrize("shape", [(2, (4, 6, 5), (2, 3, 1)), (1, (257, 1, 1), (1, 1, 1))], ids=["2x4x6x5", "257_tiles"])
def test_tvsr3d_solve(shape, entry):
    """257 x 1 x 1 with unit factors is 257 tiles: more partials of energy and change than the finish kernel has threads."""
    lib, dtype = _lib.lib(), dtype_of(entry)
    n, (D, H, W), f = shape
    lr = (n, D // f[0], H // f[1], W // f[2])
    rng = np.random.default_rng(7)
    ks = [(lambda v: (v / v.sum()).tolist())(rng.random(fa) + 0.1) for fa in f]
    g = (0.5, 1.0, 1.0)
    y, w, x0 = rnd(*lr, seed=1, dtype=dtype), rnd(*lr, seed=2, dtype=dtype), rnd(n, D, H, W, seed=3, dtype=dtype)
    w.view(-1)[1] = 0
    need = lib.inr_tvsr3d_workspace_doubles(n, D, H, W, *f)

    def call(weight, start):
        return lambda ws, o: getattr(lib, entry)(o["out"].ptr, gp(o, "energy"), gp(o, "change"), y.data_ptr(), ptr(weight), ptr(start), n, D, H, W,
                                                 *f, *[dbl(k) for k in ks], dbl(g), LAM, ALPHA, ITERS, ws.ptr, need, stream())
    outs = {"out": ((n, D, H, W), dtype), "energy": ((n,), F64), "change": ((n,), F64)}
    ref = ops.tvsr_solve3d(y, f, ks, LAM, ALPHA, ITERS, g, w, x0)
    case(entry, need, 8, outs, call(w, x0), dict(zip(outs, ref)))
    nulls(entry, need, 8, {"out": outs["out"]}, call(None, None))


@pytest.mark.parametrize("entry", ["inr_tvmf_solve2d", "inr_tvmf_solve2d_f32"])
@pytest.mark.parametrize("shape", [(2, 3, (6, 10), (3, 2)), (1, 1, (512, 512), (1, 1))], ids=["2x3x6x10", "512_parts"])
def test_tvmf_solve2d(shape, entry):
    """512 x 512 with unit factors and one frame is 512 parts: every thread of the finish kernel adds two partials."""
    lib, dtype = _lib.lib(), dtype_of(entry)
    n, K, (H, W), (f0, f1) = shape
    k = block_kernel(f0, f1)
    shifts = rnd(n, K, 2, seed=4, lo=-1.5, hi=1.5)
    if K > 1:
        shifts[0, 0] = 0.0
        shifts[1, 2, 1] = float("nan")
    y, w = rnd(n, K, H // f0, W // f1, seed=1, dtype=dtype), rnd(n, K, H // f0, W // f1, seed=2, dtype=dtype)
    x0 = rnd(n, H, W, seed=3, dtype=dtype)
    w.view(-1)[5] = 0
    need = lib.inr_tvmf_workspace_doubles(n, K, H, W, f0, f1)

    def call(weight, start):
        return lambda ws, o: getattr(lib, entry)(o["out"].ptr, gp(o, "energy"), gp(o, "change"), gp(o, "valid_fraction"), y.data_ptr(),
                                                 shifts.data_ptr(), ptr(weight), ptr(start), n, K, H, W, f0, f1, flat(k), LAM, ALPHA, ITERS,
                                                 ws.ptr, need, stream())
    outs = {"out": ((n, H, W), dtype), "energy": ((n,), F64), "change": ((n,), F64), "valid_fraction": ((n,), F64)}
    ref = ops.tvmf_solve(y, shifts, (f0, f1), k, LAM, ALPHA, ITERS, w, x0)
    case(entry, need, 8, outs, call(w, x0), dict(zip(outs, ref)))
    nulls(entry, need, 8, {"out": outs["out"]}, call(None, None))


def _two_stacks():
    """A 5 x 6 x 7 volume under two stacks of different spacing and tap count: the first starts one slice before the volume (its first
    slice is invalid), the second runs past the last row and column."""
    a = ((2, 1, 1), ([0.5, 0.5], [1.0], [1.0]), (-1, 0, 0), (3, 6, 7))
    b = ((1, 2, 3), ([1.0], [0.25, 0.5, 0.25], [0.5, 0.5]), (0, 0, 1), (5, 3, 3))
    return 2, (5, 6, 7), [a, b]


def _unit_stack():
    hr = (33, 64, 64)
    return 1, hr, [((1, 1, 1), ([1.0], [1.0], [1.0]), (0, 0, 0), hr)]


@pytest.mark.parametrize("entry", ["inr_tvms_solve", "inr_tvms_solve_f32"])
@pytest.mark.parametrize("setup", [_two_stacks, _unit_stack], ids=["two_stacks", "264_parts"])
def test_tvms_solve(setup, entry):
    """33 x 64 x 64 under one unit stack is 264 parts: eight threads of the finish kernel add two partials."""
    lib, dtype = _lib.lib(), dtype_of(entry)
    n, (D, H, W), stacks = setup()
    geo = (C.c_int * (12 * len(stacks)))(*[v for f, ks, o, ext in stacks for v in (*f, *[len(k) for k in ks], *o, *ext)])
    taps = dbl([v for _, ks, _, _ in stacks for k in ks for v in k])
    M = sum(e[0] * e[1] * e[2] for _, _, _, e in stacks)
    g = (0.5, 1.0, 1.0)
    y, w, x0 = rnd(n, M, seed=1, dtype=dtype), rnd(n, M, seed=2, dtype=dtype), rnd(n, D, H, W, seed=3, dtype=dtype)
    w[0, M - 1] = 0
    need = lib.inr_tvms_workspace_doubles(n, D, H, W, len(stacks), geo)

    def call(weight, start):
        return lambda ws, o: getattr(lib, entry)(o["out"].ptr, gp(o, "energy"), gp(o, "change"), gp(o, "valid_fraction"), y.data_ptr(),
                                                 ptr(weight), ptr(start), n, D, H, W, len(stacks), geo, taps, dbl(g), LAM, ALPHA, ITERS, ws.ptr,
                                                 need, stream())
    outs = {"out": ((n, D, H, W), dtype), "energy": ((n,), F64), "change": ((n,), F64), "valid_fraction": ((n,), F64)}
    ref = ops.tvms_solve(y, stacks, (D, H, W), LAM, ALPHA, ITERS, g, w, x0)
    case(entry, need, 8, outs, call(w, x0), dict(zip(outs, ref)))
    nulls(entry, need, 8, {"out": outs["out"]}, call(None, None))


def _operators(H, W, h, w):
    r0, r1 = rnd(h, H, seed=8, lo=0.05), rnd(w, W, seed=9, lo=0.05)
    return (r0 / r0.sum(1, keepdim=True)).contiguous(), (r1 / r1.sum(1, keepdim=True)).contiguous()


TVOP_SHAPES = pytest.mark.parametrize("shape", [(2, 7, 9, 3, 4), (1, 1024, 1024, 64, 64)], ids=["2x7x9", "257_partials"])


@pytest.mark.parametrize("entry", ["inr_tvop_solve2d", "inr_tvop_solve2d_f32"])
@TVOP_SHAPES
def test_tvop_solve2d(shape, entry):
    """(1024, 1024) -> (64, 64) is 1 LR tile and 256 HR tiles, 257 energy partials: thread 0 of the finish kernel adds two."""
    lib, dtype = _lib.lib(), dtype_of(entry)
    n, H, W, h, w_ = shape
    r0, r1 = _operators(H, W, h, w_)
    y, w, x0 = rnd(n, h, w_, seed=1, dtype=dtype), rnd(n, h, w_, seed=2, dtype=dtype), rnd(n, H, W, seed=3, dtype=dtype)
    w.view(-1)[3] = 0
    need = lib.inr_tvop_workspace_doubles(n, H, W, h, w_)

    def call(weight, start):
        return lambda ws, o: getattr(lib, entry)(o["out"].ptr, gp(o, "energy"), gp(o, "change"), y.data_ptr(), ptr(weight), ptr(start),
                                                 r0.data_ptr(), r1.data_ptr(), n, H, W, h, w_, LAM, ALPHA, ITERS, ws.ptr, need, stream())
    outs = {"out": ((n, H, W), dtype), "energy": ((n,), F64), "change": ((n,), F64)}
    ref = ops.tvop_solve(y, (r0, r1), LAM, ALPHA, ITERS, w, x0)
    case(entry, need, 8, outs, call(w, x0), dict(zip(outs, ref)))
    nulls(entry, need, 8, {"out": outs["out"]}, call(None, None))


@TVOP_SHAPES
def test_tvop_apply_and_adjoint(shape):
    lib = _lib.lib()
    n, H, W, h, w_ = shape
    r0, r1 = _operators(H, W, h, w_)
    x, r = rnd(n, H, W, seed=1), rnd(n, h, w_, seed=2)
    need = lib.inr_tvop_workspace_doubles(n, H, W, h, w_)
    case("inr_tvop_apply", need, 8, {"out": ((n, h, w_), F64)},
         lambda ws, o: lib.inr_tvop_apply(o["out"].ptr, x.data_ptr(), r0.data_ptr(), r1.data_ptr(), n, H, W, h, w_, ws.ptr, need, stream()),
         {"out": ops.tvop_apply(x, (r0, r1))})
    case("inr_tvop_adjoint", need, 8, {"out": ((n, H, W), F64)},
         lambda ws, o: lib.inr_tvop_adjoint(o["out"].ptr, r.data_ptr(), r0.data_ptr(), r1.data_ptr(), n, H, W, h, w_, ws.ptr, need, stream()),
         {"out": ops.tvop_adjoint(r, (r0, r1))})


# ---- skimage-style resize, masked registration and shift, the through-plane cubic, Fourier re-sampling -----------------------------------
@pytest.mark.parametrize("clip_group", [1, 2])
@pytest.mark.parametrize("mode", ["reflect", "edge"])
@pytest.mark.parametrize("order", [1, 3])
def test_rescale2d(order, mode, clip_group):
    lib = _lib.lib()
    n, H, W, OH, OW = 2, 7, 5, 4, 3
    x = rnd(n, H, W, seed=1, dtype=F32)
    need = lib.inr_rescale2d_workspace_doubles(n, H, W, order, baselines._MODES[mode])
    ref = baselines._resize("resize", x, (OH, OW), order, mode, True, True, group_axes=clip_group - 1)
    case(f"inr_rescale2d (order {order}, {mode}, clip_group {clip_group})", need, 8, {"out": ((n, OH, OW), F32)},
         lambda ws, o: lib.inr_rescale2d(o["out"].ptr, x.data_ptr(), n, H, W, OH, OW, order, baselines._MODES[mode], 1, clip_group, ws.ptr, need,
                                         stream()), {"out": ref})


@pytest.mark.parametrize("window", [None, (2, 3)], ids=["full_search", "window_2x3"])
def test_masked_xcorr(window):
    lib = _lib.lib()
    S, T, H, W = 2, 3, 9, 11
    my, mx = window or (H - 1, W - 1)
    planes, masks = rnd(S, T, H, W, seed=1, dtype=F32), (rnd(S, T, H, W, seed=2) > 0.2).to(F32)
    ref_index = torch.tensor([1, 2], dtype=torch.int32, device=DEV)
    need = lib.inr_masked_xcorr_workspace_doubles(S, T, H, W, my, mx)

    def call(ws, o):
        return lib.inr_masked_xcorr(o["shifts"].ptr, o["peak"].ptr, o["n_max"].ptr, gp(o, "map"), planes.data_ptr(), masks.data_ptr(),
                                    ref_index.data_ptr(), S, T, H, W, my, mx, 0.3, ws.ptr, need, stream())
    outs = {"shifts": ((S, T, 2), F64), "peak": ((S, T), F64), "n_max": ((S, T), torch.int32), "map": ((S, T, 2 * my + 1, 2 * mx + 1), F64)}
    ref = registration._xcorr(planes, masks, ref_index, (my, mx), 0.3, want_map=True)
    case("inr_masked_xcorr", need, 8, outs, call, dict(zip(outs, ref)))
    nulls("inr_masked_xcorr", need, 8, {k: v for k, v in outs.items() if k != "map"}, call)


@pytest.mark.parametrize("mode", ["reflect", "constant"])
def test_shift2d(mode):
    lib = _lib.lib()
    n, H, W = 2, 9, 11
    x = rnd(n, H, W, seed=1, dtype=F32)
    shifts = torch.tensor([[1.25, -2.5], [-0.75, 3.0]], dtype=F64, device=DEV)
    need = lib.inr_shift2d_workspace_doubles(n, H, W, registration._SHIFT_MODES[mode])
    case(f"inr_shift2d ({mode})", need, 8, {"out": ((n, H, W), F32)},
         lambda ws, o: lib.inr_shift2d(o["out"].ptr, x.data_ptr(), shifts.data_ptr(), n, H, W, registration._SHIFT_MODES[mode], 0.5, ws.ptr, need,
                                       stream()), {"out": registration._shift_planes(x, shifts, mode, 0.5)})


def test_resize_z_cubic():
    lib = _lib.lib()
    lines, n_in, n_out = 257, 7, 20
    x = rnd(lines, n_in, seed=1)
    need = lib.inr_resize_z_cubic_workspace_bytes(lines, n_in)
    case("inr_resize_z_cubic", need, 1, {"out": ((lines, n_out), F64)},
         lambda ws, o: lib.inr_resize_z_cubic(o["out"].ptr, x.data_ptr(), lines, n_in, n_out, ws.ptr, need, stream()),
         {"out": baselines.resize_z(x, n_out)})


@pytest.mark.parametrize("entry", ["inr_fourier_resample2d", "inr_fourier_resample2d_f32"])
@pytest.mark.parametrize("shape", [((17, 19), (33, 38), "center", "mirror", 0.25), ((50, 25), (25, 50), "sample", "periodic", 0.0)],
                         ids=["17x19_to_33x38", "50x25_to_25x50"])
def test_fourier_resample2d(shape, entry):
    lib, dtype = _lib.lib(), dtype_of(entry)
    (H, W), (OH, OW), align, boundary, apodize = shape
    n = 2
    x = rnd(n, H, W, seed=1, dtype=dtype)
    need = lib.inr_fourier_resample_workspace_doubles(n, H, W, OH, OW)
    case(entry, need, 8, {"out": ((n, OH, OW), dtype)},
         lambda ws, o: getattr(lib, entry)(o["out"].ptr, x.data_ptr(), n, H, W, OH, OW, baselines._FOURIER_ALIGN[align],
                                           baselines._FOURIER_BOUNDARY[boundary], apodize, ws.ptr, need, stream()),
         {"out": baselines.fourier_resize(x, (OH, OW), align, boundary, apodize)})


# ---- the reader-study scores and the end-of-fit metrics ------------------------------------------------------------------------------------
def _score_pair(n=2, H=45, W=52):
    x = rnd(n, H, W, seed=1, dtype=F32)
    return x, (x + 0.05 * rnd(n, H, W, seed=2, dtype=F32)).contiguous()


def test_ssim2d_gauss():
    lib = _lib.lib()
    x, y = _score_pair()
    n, H, W = x.shape
    need = lib.inr_perceptual_workspace_doubles(n, H, W, 1)

    def call(ws, o):
        return lib.inr_ssim2d_gauss(o["ssim"].ptr, gp(o, "mean_cs"), gp(o, "map"), x.data_ptr(), y.data_ptr(), n, H, W, 1.5, 1.0, ws.ptr, need,
                                    stream())
    outs = {"ssim": ((n,), F64), "mean_cs": ((n,), F64), "map": ((n, H, W), F32)}
    ref = perceptual.ssim_gauss(x, y, 1.5, 1.0, return_cs=True, return_map=True)
    case("inr_ssim2d_gauss", need, 8, outs, call, dict(zip(outs, ref)))
    nulls("inr_ssim2d_gauss", need, 8, {"ssim": outs["ssim"]}, call)


def test_msssim2d():
    lib = _lib.lib()
    x, y = _score_pair()
    n, H, W = x.shape
    weights = (0.3, 0.3, 0.4)
    need = lib.inr_perceptual_workspace_doubles(n, H, W, len(weights))

    def call(ws, o):
        return lib.inr_msssim2d(o["out"].ptr, gp(o, "per_scale"), x.data_ptr(), y.data_ptr(), n, H, W, dbl(weights), len(weights), 1.5, 1.0,
                                ws.ptr, need, stream())
    outs = {"out": ((n,), F64), "per_scale": ((n, len(weights)), F64)}
    ref = perceptual.ms_ssim(x, y, weights, 1.5, 1.0, return_per_scale=True)
    case("inr_msssim2d", need, 8, outs, call, dict(zip(outs, ref)))
    nulls("inr_msssim2d", need, 8, {"out": outs["out"]}, call)


@pytest.mark.parametrize("name", ["inr_image_mse", "inr_hf_gain"])
def test_pair_scores(name):
    lib = _lib.lib()
    x, y = _score_pair()
    n, H, W = x.shape
    need = lib.inr_perceptual_workspace_doubles(n, 1, 1, 1)
    case(name, need, 8, {"out": ((n,), F64)},
         lambda ws, o: getattr(lib, name)(o["out"].ptr, x.data_ptr(), y.data_ptr(), n, H * W, ws.ptr, need, stream()),
         {"out": (perceptual.mse if name == "inr_image_mse" else perceptual.hf_gain)(x, y)})


def test_psnr_and_ssim2d():
    lib = _lib.lib()
    x, y = _score_pair(3, 13, 17)
    n, H, W = x.shape
    need = lib.inr_metric_workspace_bytes(n)
    case("inr_psnr", need, 1, {"out": ((n,), F64)},
         lambda ws, o: lib.inr_psnr(o["out"].ptr, x.data_ptr(), y.data_ptr(), n, H * W, 1.0, ws.ptr, need, stream()),
         {"out": metrics.psnr(x, y, 1.0, per_image=True)})
    for thr in (None, 0.3):
        case(f"inr_ssim2d (mask threshold {thr})", need, 1, {"out": ((n,), F64)},
             lambda ws, o: lib.inr_ssim2d(o["out"].ptr, x.data_ptr(), y.data_ptr(), n, H, W, 7, 1.0, int(thr is not None), thr or 0.0, ws.ptr,
                                          need, stream()),
             {"out": metrics.ssim(x, y, 1.0, 7, thr)})


# ---- the shift-tolerant losses, the stand-alone 3-D convolution gradients, the footprint loss, WIRE re-sampling -----------------------------
def _loss_images(B=2, size=24):
    yt, yp = rnd(B, size, size, seed=1, dtype=F32, lo=500, hi=60000), rnd(B, size, size, seed=2, dtype=F32, lo=500, hi=60000)
    return yt, yp, (rnd(B, size, size, seed=3) > 0.1).to(F32)


@pytest.mark.parametrize("mode", [0, 1], ids=["cL1", "cPSNR"])
def test_rams_shift_loss(mode):
    lib = _lib.lib()
    yt, yp, mk = _loss_images()
    B, size, border = yt.shape[0], yt.shape[1], 3
    need = lib.inr_rams_shift_loss_workspace_bytes(B, border)
    case(f"inr_rams_shift_loss (mode {mode})", need, 1, {"out": ((B,), F64)},
         lambda ws, o: lib.inr_rams_shift_loss(o["out"].ptr, yt.data_ptr(), yp.data_ptr(), mk.data_ptr(), B, size, border, mode, ws.ptr, need,
                                               stream()), {"out": rams._shift_loss(yt, yp, mk, size, mode)})


def test_rams_shift_loss_grad():
    lib = _lib.lib()
    yt, yp, mk = _loss_images()
    B, size, border = yt.shape[0], yt.shape[1], 3
    up = torch.tensor([0.5, 2.0], dtype=F32, device=DEV)
    need = lib.inr_rams_shift_loss_grad_workspace_bytes(B, border)

    def call(upstream):
        return lambda ws, o: lib.inr_rams_shift_loss_grad(o["loss"].ptr, o["grad"].ptr, yt.data_ptr(), yp.data_ptr(), mk.data_ptr(), ptr(upstream),
                                                          B, size, border, ws.ptr, need, stream())
    outs = {"loss": ((B,), F64), "grad": ((B, size, size), F32)}
    case("inr_rams_shift_loss_grad", need, 1, outs, call(up), dict(zip(outs, rams.l1_loss_and_grad(yt, yp, mk, size, upstream=up))))
    nulls("inr_rams_shift_loss_grad", need, 1, outs, call(None))


def test_rams_conv3d_gradients():
    lib = _lib.lib()
    B, D1, D2, D3 = 2, 10, 9, 5
    x, dy = rnd(B, D1, D2, D3, 32, seed=1, dtype=F32, lo=-1), rnd(B, D1, D2, D3, 32, seed=2, dtype=F32, lo=-1)
    w = rnd(27, 32, 32, seed=3, dtype=F32, lo=-0.1, hi=0.1)
    need = lib.inr_rams_conv3d_dgrad_workspace_bytes()
    case("inr_rams_conv3d_dgrad", need, 1, {"dx": ((B, D1, D2, D3, 32), F32)},
         lambda ws, o: lib.inr_rams_conv3d_dgrad(o["dx"].ptr, dy.data_ptr(), w.data_ptr(), B, D1, D2, D3, ws.ptr, need, stream()),
         {"dx": rams.conv3d_dgrad(dy, w)})
    need = lib.inr_rams_conv3d_wgrad_workspace_bytes(B, D1, D2, D3, 1)

    def call(ws, o):
        return lib.inr_rams_conv3d_wgrad(o["gw"].ptr, gp(o, "gb"), x.data_ptr(), dy.data_ptr(), B, D1, D2, D3, 1, ws.ptr, need, stream())
    outs = {"gw": ((27, 32, 32), F32), "gb": ((32,), F32)}
    case("inr_rams_conv3d_wgrad", need, 1, outs, call, dict(zip(outs, rams.conv3d_wgrad(x, dy, 1))))
    nulls("inr_rams_conv3d_wgrad", need, 1, {"gw": outs["gw"]}, call)


def test_footprint_loss_grad():
    lib = _lib.lib()
    n, K = 255, 5
    y, t, wt = rnd(n * K, seed=1, dtype=F32), rnd(n, seed=2, dtype=F32), rnd(n, seed=3, dtype=F32)
    fw = torch.tensor([0.1, 0.2, 0.4, 0.2, 0.1], dtype=F32, device=DEV)
    need = lib.inr_footprint_loss_workspace_floats(n)

    def call(weight):
        return lambda ws, o: lib.inr_footprint_loss_grad(o["gy"].ptr, o["loss"].ptr, gp(o, "pred"), y.data_ptr(), t.data_ptr(), ptr(weight),
                                                         fw.data_ptr(), n, K, 0, ws.ptr, need, stream())
    outs = {"gy": ((n * K,), F32), "loss": ((1,), F32), "pred": ((n,), F32)}
    case("inr_footprint_loss_grad", need, 4, outs, call(wt), dict(zip(outs, ops.footprint_loss_grad(y, t, wt, fw, 0, want_pred=True))))
    nulls("inr_footprint_loss_grad", need, 4, {k: outs[k] for k in ("gy", "loss")}, call(None))


def test_wire_reconstruct():
    lib = _lib.lib()
    shape, m, chunk = (9, 7, 5), 16, 128
    torch.manual_seed(11)
    model = wire.Wire(2 * m, 32, 1, 1).to(DEV)
    B = rnd(m, len(shape), seed=1, dtype=F32, lo=-2, hi=2)
    desc = model.desc()
    params = model._flat(desc)
    need = lib.inr_wire_reconstruct_workspace_bytes(C.byref(desc), chunk)
    total = int(np.prod(shape))

    def call(mapping, use_clamp):
        return lambda ws, o: lib.inr_wire_reconstruct(C.byref(desc), params.data_ptr(), _lib.shape_array(shape), len(shape), ptr(mapping), m,
                                                      o["y"].ptr, use_clamp, 0.0, chunk, ws.ptr, need, stream())
    case("inr_wire_reconstruct", need, 1, {"y": ((total,), F32)}, call(B, 1), {"y": wire.reconstruct(model, shape, B, 0.0, chunk)})


# ---- the four layer-level entry points, at the ragged shapes tests/test_workspace_plans_cpu.py pins -----------------------------------------
N_ROWS = 3601


def sym(*shape, seed, scale=1.0):
    return rnd(*shape, seed=seed, dtype=F32, lo=-scale, hi=scale)


def test_mse_loss_grad():
    lib = _lib.lib()
    y, t, w = sym(N_ROWS, 1, seed=1), sym(N_ROWS, 1, seed=2), rnd(N_ROWS, 1, seed=3, dtype=F32)
    need = lib.inr_mse_workspace_bytes(N_ROWS)

    def call(weight):
        return lambda ws, o: lib.inr_mse_loss_grad(o["gy"].ptr, o["loss"].ptr, y.data_ptr(), t.data_ptr(), ptr(weight), N_ROWS, ws.ptr, need,
                                                   stream())
    outs = {"gy": ((N_ROWS, 1), F32), "loss": ((1,), F32)}
    loss, gy = ops.mse_loss_grad(y, t, w)
    case("inr_mse_loss_grad", need, 1, outs, call(w), {"gy": gy, "loss": loss})
    nulls("inr_mse_loss_grad", need, 1, outs, call(None))


@pytest.mark.parametrize("hidden,out_f", [(64, 1), (48, 3)])
def test_linear_head_backward(hidden, out_f):
    lib = _lib.lib()
    n = N_ROWS
    gy, a, dact, W = sym(n, out_f, seed=1), sym(n, hidden, seed=2), sym(n, hidden, seed=3), sym(out_f, hidden, seed=4, scale=0.2)
    need = lib.inr_head_backward_workspace_bytes(n, hidden, out_f)

    def call(slope):
        return lambda ws, o: lib.inr_linear_head_backward(o["dz_last"].ptr, o["gW"].ptr, o["gb"].ptr, gp(o, "gb_last"), gy.data_ptr(),
                                                          a.data_ptr(), ptr(slope), W.data_ptr(), n, hidden, out_f, ws.ptr, need, stream())
    outs = {"dz_last": ((n, hidden), F32), "gW": ((out_f, hidden), F32), "gb": ((out_f,), F32), "gb_last": ((hidden,), F32)}
    ref = ops.linear_head_backward(gy, a, dact, W, True, True, True)
    case(f"inr_linear_head_backward ({hidden} -> {out_f})", need, 1, outs, call(dact), dict(zip(outs, ref)))
    nulls(f"inr_linear_head_backward ({hidden} -> {out_f})", need, 1, {k: v for k, v in outs.items() if k != "gb_last"}, call(None))


def test_sine_layer_backward_input():
    lib = _lib.lib()
    n, fin, fout = N_ROWS, 64, 64
    dz, W, dact = sym(n, fout, seed=1), sym(fout, fin, seed=2, scale=0.2), sym(n, fin, seed=3)
    need = lib.inr_sine_layer_backward_input_workspace_bytes(n, fin)

    def call(slope):
        return lambda ws, o: lib.inr_sine_layer_backward_input(o["dz_prev"].ptr, gp(o, "gb_prev"), dz.data_ptr(), W.data_ptr(), ptr(slope), n, fin,
                                                               fout, ws.ptr, need, stream())
    outs = {"dz_prev": ((n, fin), F32), "gb_prev": ((fin,), F32)}
    case("inr_sine_layer_backward_input", need, 1, outs, call(dact), dict(zip(outs, ops.sine_layer_backward_input(dz, W, dact, need_bias=True))))
    nulls("inr_sine_layer_backward_input", need, 1, {"dz_prev": outs["dz_prev"]}, call(None))


def test_linear_param_grad():
    lib = _lib.lib()
    n, fin, fout = N_ROWS, 2, 64
    dz, x = sym(n, fout, seed=1), sym(n, fin, seed=2)
    need = lib.inr_linear_param_grad_workspace_bytes(n, fin, fout)

    def call(ws, o):
        return lib.inr_linear_param_grad(o["gW"].ptr, gp(o, "gb"), dz.data_ptr(), x.data_ptr(), n, fin, fout, ws.ptr, need, stream())
    outs = {"gW": ((fout, fin), F32), "gb": ((fout,), F32)}
    case("inr_linear_param_grad", need, 1, outs, call, dict(zip(outs, ops.linear_param_grad(dz, x, True))))
    nulls("inr_linear_param_grad", need, 1, {"gW": outs["gW"]}, call)
