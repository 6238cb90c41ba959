"""The second trip of the batch loops and of the capped pixel grids of the block-operator units.

The single-workgroup solvers (csrc/tvsr.hip, tvj.hip, tgv.hip, tvadc.hip) launch min(n, 65,536) workgroups and walk the batch with
stride gridDim.x; the one-thread-per-pixel launches sized by tv_pixel_grid (inr_block_apply2d, inr_block_adjoint2d, inr_adc_signal)
stop at 65,536 x 256 threads and walk the pixels the same way.  No other test has a batch above 300 or 16,777,216 pixels, so only
these cases take the second trip: a new state offset, the start written behind the previous image's last barrier, the block kernel
and the b-values staged once, the reduction's LDS reused.  There is no debug key and no test-only cap: the images are tiny instead.

Everything is guarded as in tests/test_gpu_workspace_guard_units.py and every comparison is bit equality.  The inputs behind the cap
repeat the inputs one period earlier, so the outputs must repeat too; the head is anchored to solitary solves (the solvers) or to the
same expression in torch float64 (the block operator under the 'decimate' and the mean kernel, both exact in any order of summation
because the unit is compiled with -ffp-contract=off)."""
import ctypes as C

import pytest
import torch

from tests.guard_common import DEV, POISON, Guarded, guard_case, same_bits
from mri_super_resolution_amd import _lib, ops

pytestmark = pytest.mark.gpu
F64 = torch.float64
CAP = 1 << 16                   # TV_MAX_GRID of csrc/tv_block.h
PERIOD = CAP * 256              # the threads of a capped pixel grid
EXTRA = 5
H, W, F0, F1 = 2, 3, 2, 1
KERNEL = [[0.75], [0.25]]
LAM, ALPHA, ITERS = 0.05, 0.02, 3


def stream():
    return torch.cuda.current_stream().cuda_stream


def dbl(values):
    values = [float(v) for v in values]
    return (C.c_double * len(values))(*values)


def batch(*shape, seed, lo=0.0, hi=1.0):
    """[CAP + EXTRA, *shape] random doubles whose last EXTRA items repeat the first EXTRA."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    head = torch.rand(CAP, *shape, generator=g, dtype=F64, device=DEV) * (hi - lo) + lo
    return torch.cat((head, head[:EXTRA])).contiguous()


def second_trip(entry, need, outputs, call, solitary):
    """The guarded protocol on the batch of CAP + EXTRA, then: item CAP + i repeats item i, and items 0 .. EXTRA - 1 equal their
    solitary solves (`solitary(i)`: name -> tensor, through the public wrapper with a batch of 1)."""
    got = guard_case(entry, int(need) * 8, outputs, call, None, last_error=_lib.lib().inr_last_error)
    for name, t in got.items():
        assert same_bits(t[CAP:], t[:EXTRA]), f"{entry}: `{name}` of the items behind the grid differs from the items one grid earlier"
    for i in range(EXTRA):
        for name, want in solitary(i).items():
            assert same_bits(got[name][i:i + 1], want.reshape(got[name][i:i + 1].shape)), f"{entry}: `{name}` of item {i} differs from its solitary solve"


def test_tvsr_batch_beyond_the_grid():
    lib, n = _lib.lib(), CAP + EXTRA
    y, w = batch(H // F0, W // F1, seed=1), batch(H // F0, W // F1, seed=2)
    need = lib.inr_tvsr_workspace_doubles(n, H, W)
    outs = {"out": ((n, H, W), F64), "energy": ((n,), F64), "change": ((n,), F64)}
    second_trip("inr_tvsr_solve2d", need, outs,
                lambda ws, o: lib.inr_tvsr_solve2d(o["out"].ptr, o["energy"].ptr, o["change"].ptr, y.data_ptr(), w.data_ptr(), 0, n, H, W, F0, F1,
                                                   dbl(sum(KERNEL, [])), LAM, ALPHA, ITERS, ws.ptr, need, stream()),
                lambda i: dict(zip(outs, ops.tvsr_solve(y[i:i + 1], (F0, F1), KERNEL, LAM, ALPHA, ITERS, w[i:i + 1]))))


def test_tgv_batch_beyond_the_grid():
    lib, n, ratio = _lib.lib(), CAP + EXTRA, 2.0
    y, w = batch(H // F0, W // F1, seed=1), batch(H // F0, W // F1, seed=2)
    need = lib.inr_tgv_workspace_doubles(n, H, W)
    outs = {"out": ((n, H, W), F64), "v_out": ((n, 2, H, W), F64), "energy": ((n,), F64), "change": ((n,), F64)}
    second_trip("inr_tgv_solve2d", need, outs,
                lambda ws, o: lib.inr_tgv_solve2d(o["out"].ptr, o["v_out"].ptr, o["energy"].ptr, o["change"].ptr, y.data_ptr(), w.data_ptr(), 0, n,
                                                  H, W, F0, F1, dbl(sum(KERNEL, [])), LAM, ratio, ALPHA, ITERS, ws.ptr, need, stream()),
                lambda i: dict(zip(outs, ops.tgv_solve(y[i:i + 1], (F0, F1), KERNEL, LAM, ratio, ALPHA, ITERS, w[i:i + 1]))))


def test_tvj_batch_beyond_the_grid():
    lib, n, ch, mu = _lib.lib(), CAP + EXTRA, 3, (1.0, 0.5, 0.25)
    y, w = batch(ch, H // F0, W // F1, seed=1), batch(ch, H // F0, W // F1, seed=2)
    need = lib.inr_tvj_workspace_doubles(n, ch, H, W)
    outs = {"out": ((n, ch, H, W), F64), "energy": ((n,), F64), "change": ((n,), F64)}
    second_trip("inr_tvj_solve2d", need, outs,
                lambda ws, o: lib.inr_tvj_solve2d(o["out"].ptr, o["energy"].ptr, o["change"].ptr, y.data_ptr(), w.data_ptr(), 0, n, ch, H, W, F0,
                                                  F1, dbl(sum(KERNEL, [])), dbl(mu), LAM, ALPHA, 1, ITERS, ws.ptr, need, stream()),
                lambda i: dict(zip(outs, ops.tvj_solve(y[i:i + 1], (F0, F1), KERNEL, mu, LAM, ALPHA, "joint", ITERS, w[i:i + 1]))))


def test_tvadc_batch_beyond_the_grid():
    lib, n = _lib.lib(), CAP + EXTRA
    b, mu, s_max, adc_max, adc0 = (0.0, 500.0, 1000.0), (1.0, 0.5), 2.0, 0.005, 0.001
    s, d = batch(1, H // F0, W // F1, seed=1, lo=0.3), batch(1, H // F0, W // F1, seed=2, lo=0.0005, hi=0.003)
    y = (s * torch.exp(-torch.tensor(b, dtype=F64, device=DEV).view(1, 3, 1, 1) * d)).contiguous()
    w = batch(3, H // F0, W // F1, seed=3)
    need = lib.inr_tvadc_workspace_doubles(n, 3, H, W, F0, F1)
    outs = {"out": ((n, 2, H, W), F64), "energy": ((n,), F64), "change": ((n,), F64)}

    def solitary(i):
        s0, adc, energy, change = ops.tvadc_solve(y[i:i + 1], b, (F0, F1), KERNEL, mu, LAM, ALPHA, "joint", ITERS, s_max, adc_max, adc0, w[i:i + 1])
        return {"out": torch.stack((s0, adc), 1), "energy": energy, "change": change}
    second_trip("inr_tvadc_solve2d", need, outs,
                lambda ws, o: lib.inr_tvadc_solve2d(o["out"].ptr, o["energy"].ptr, o["change"].ptr, y.data_ptr(), w.data_ptr(), 0, n, 3, H, W, F0,
                                                    F1, dbl(sum(KERNEL, [])), dbl(b), dbl(mu), LAM, ALPHA, 1, ITERS, s_max, adc_max, adc0, ws.ptr,
                                                    need, stream()), solitary)


# ---- the one-thread-per-pixel launches: PERIOD + some threads' worth of work ------------------------------------------------------------------
BH, BW = 128, 64                # HR images of 128 x 64 by (2, 1): 4,096 LR pixels and 8,192 HR pixels each
KERNELS = {"decimate": (1.0, 0.0), "mean": (0.5, 0.5)}


def guarded_output(entry, shape, call):
    out = Guarded(shape, F64, POISON)
    rc = call(out)
    assert rc == 0, (entry, rc, _lib.lib().inr_last_error())
    assert out.intact(), f"{entry}: the call wrote outside its output {out.shape}"
    assert out.written(), f"{entry}: output elements are unwritten or not finite"
    print(f"{entry}: output {out.shape} pre-filled with {POISON:#04x}, {out.view.numel() - PERIOD} elements behind the capped grid")
    return out.view


@pytest.mark.parametrize("kernel", KERNELS)
def test_block_apply_beyond_the_pixel_grid(kernel):
    """4,097 HR images: 16,777,216 + 4,096 LR pixels, one per thread.  Image 4,096 repeats image 0."""
    lib, k = _lib.lib(), KERNELS[kernel]
    n = PERIOD // (BH // 2 * BW) + 1
    g = torch.Generator(device=DEV).manual_seed(1)
    head = torch.rand(n - 1, BH, BW, generator=g, dtype=F64, device=DEV)
    x = torch.cat((head, head[:1])).contiguous()
    got = guarded_output("inr_block_apply2d", (n, BH // 2, BW),
                         lambda o: lib.inr_block_apply2d(o.ptr, x.data_ptr(), n, BH, BW, 2, 1, dbl(k), stream()))
    flat = got.view(-1)
    assert same_bits(flat[PERIOD:], flat[:flat.numel() - PERIOD]), "the pixels behind the capped grid differ from those one period earlier"
    want = (0.0 + k[0] * x[:, 0::2, :]) + k[1] * x[:, 1::2, :]
    assert same_bits(got, want), f"inr_block_apply2d differs from the torch float64 expression under the '{kernel}' kernel"


@pytest.mark.parametrize("kernel", KERNELS)
def test_block_adjoint_beyond_the_pixel_grid(kernel):
    """4,097 LR images: 2 x 16,777,216 + 8,192 HR pixels, one per thread.  The LR images repeat with the period of the grid, 2,048."""
    lib, k = _lib.lib(), KERNELS[kernel]
    per = PERIOD // (BH * BW)
    n = 2 * per + 1
    g = torch.Generator(device=DEV).manual_seed(2)
    head = torch.rand(per, BH // 2, BW, generator=g, dtype=F64, device=DEV)
    r = torch.cat((head, head, head[:1])).contiguous()
    got = guarded_output("inr_block_adjoint2d", (n, BH, BW),
                         lambda o: lib.inr_block_adjoint2d(o.ptr, r.data_ptr(), n, BH, BW, 2, 1, dbl(k), stream()))
    flat = got.view(-1)
    assert same_bits(flat[PERIOD:], flat[:flat.numel() - PERIOD]), "the pixels behind the capped grid differ from those one period earlier"
    want = torch.stack((k[0] * r, k[1] * r), 2).reshape(n, BH, BW)
    assert same_bits(got, want), f"inr_block_adjoint2d differs from the torch float64 expression under the '{kernel}' kernel"


def test_adc_signal_beyond_the_pixel_grid():
    """One pair of maps of 16,777,216 + 1,000 pixels and two b-values; the last 1,000 pixels repeat the first.  The b = 0 channel is
    s0 exp(-0) = s0 exactly."""
    lib, extra, b = _lib.lib(), 1000, (0.0, 800.0)
    P = PERIOD + extra
    g = torch.Generator(device=DEV).manual_seed(3)
    s_head = torch.rand(PERIOD, generator=g, dtype=F64, device=DEV)
    d_head = torch.rand(PERIOD, generator=g, dtype=F64, device=DEV) * 0.003
    s0, adc = torch.cat((s_head, s_head[:extra])).contiguous(), torch.cat((d_head, d_head[:extra])).contiguous()
    got = guarded_output("inr_adc_signal", (1, len(b), P),
                         lambda o: lib.inr_adc_signal(o.ptr, s0.data_ptr(), adc.data_ptr(), dbl(b), 1, len(b), P, stream()))
    assert same_bits(got[:, :, PERIOD:], got[:, :, :extra]), "the pixels behind the capped grid differ from those one period earlier"
    assert same_bits(got[0, 0], s0), "the b = 0 channel is not s0"
    assert same_bits(got, ops.adc_signal(s0.view(1, 1, P), adc.view(1, 1, P), b).view(1, len(b), P))
