"""The host plumbing every fitter shares (flat.py), on CPU tensors: no library, no device."""
import gc
import weakref

import pytest
import torch
from torch import nn

from mri_super_resolution_amd.flat import AdamState, FlatParams, Workspace, WorkspacePool

CPU = torch.device("cpu")
# tensors [3, 2], [3], [1, 3], [1]: every one padded to 4 floats, and back to back
LAYOUTS = {"padded": (20, [0, 8, 12, 16]), "unpadded": (13, [0, 6, 9, 12])}


def _params(seed=0):
    torch.manual_seed(seed)
    a, b = nn.Linear(2, 3), nn.Linear(3, 1)
    return [a.weight, a.bias, b.weight, b.bias]


def _padding(total, offsets, params):
    used = torch.zeros(total, dtype=torch.bool)
    for off, p in zip(offsets, params):
        used[off:off + p.numel()] = True
    return ~used


@pytest.fixture(params=sorted(LAYOUTS))
def layout(request):
    return LAYOUTS[request.param]


def test_adopt_keeps_values_shares_storage_and_zeroes_padding(layout):
    total, offsets = layout
    params = _params()
    before = [p.detach().clone() for p in params]
    fp = FlatParams(total, offsets)
    flat = fp.adopt(params)
    assert flat is fp.flat and flat.shape == (total,) and flat.dtype == torch.float32
    for p, old, off in zip(params, before, offsets):
        assert torch.equal(p.detach().view(torch.int32), old.view(torch.int32))
        assert p.data_ptr() == flat.data_ptr() + 4 * off
    pad = _padding(total, offsets, params)
    assert int(pad.sum()) == total - 13
    assert torch.equal(flat[pad].view(torch.int32), torch.zeros(int(pad.sum()), dtype=torch.int32))
    # a write through flat is seen by the parameter, and the reverse
    flat[offsets[1] + 2] = 7.5
    assert float(params[1].detach()[2]) == 7.5
    with torch.no_grad():
        params[2][0, 1] = -3.25
    assert float(flat[offsets[2] + 1]) == -3.25


def test_owns_and_ensure(layout):
    total, offsets = layout
    params = _params()
    fp = FlatParams(total, offsets)
    assert not fp.owns(params)                       # nothing adopted yet
    first = fp.adopt(params)
    assert fp.owns(params)
    assert fp.ensure(params) is False and fp.flat is first

    params[2].data = params[2].data.clone() + 1.0    # what a reload or a move does: new storage
    want = [p.detach().clone() for p in params]
    assert not fp.owns(params)
    assert fp.ensure(params) is True
    assert fp.flat is not first and fp.owns(params)
    for p, w, off in zip(params, want, offsets):
        assert torch.equal(p.detach(), w)
        assert torch.equal(fp.flat[off:off + w.numel()], w.reshape(-1))
    second = fp.flat
    assert fp.ensure(params) is False and fp.flat is second


def test_owns_is_false_on_another_device_type(layout):
    total, offsets = layout
    params = _params()
    fp = FlatParams(total, offsets)
    fp.adopt(params)
    meta = [nn.Parameter(torch.empty_like(p, device="meta")) for p in params]
    assert meta[0].device.type != params[0].device.type
    assert not fp.owns(meta)


def test_split_views_cover_exactly_the_non_padding_floats(layout):
    total, offsets = layout
    params = _params()
    fp = FlatParams(total, offsets)
    fp.adopt(params)
    v = torch.zeros(total)
    parts = fp.split(v)
    assert [tuple(t.shape) for t in parts] == [(3, 2), (3,), (1, 3), (1,)]
    for t, off in zip(parts, offsets):
        assert t.data_ptr() == v.data_ptr() + 4 * off
        t.fill_(1.0)                                  # through the view, into v
    assert torch.equal(v == 0, _padding(total, offsets, params))


def test_pack_copies_and_repoints_nothing(layout):
    total, offsets = layout
    params, twin = _params(3), _params(3)
    ptrs = [p.data_ptr() for p in params]
    packed = FlatParams(total, offsets).pack(params)
    assert [p.data_ptr() for p in params] == ptrs
    assert all(p.data_ptr() != packed.data_ptr() + 4 * off for p, off in zip(params, offsets))
    assert torch.equal(packed.view(torch.int32), FlatParams(total, offsets).adopt(twin).view(torch.int32))


def test_a_layout_refuses_another_number_of_tensors():
    with pytest.raises(ValueError):
        FlatParams(20, [0, 8, 12]).adopt(_params())


def test_adam_state_reset_and_survival_of_a_readoption(layout):
    total, offsets = layout
    params = _params()
    fp = FlatParams(total, offsets)
    adam = AdamState(fp.adopt(params))
    for t in (adam.grads, adam.m, adam.v):
        assert t.shape == (total,) and t.dtype == torch.float32 and not t.any()
    assert adam.step_count == 0
    kept = (adam.grads, adam.m, adam.v)
    for k, t in enumerate(kept):
        t.fill_(k + 1.0)
    adam.step_count = 9
    params[0].data = params[0].data.clone()
    assert fp.ensure(params) is True                 # the re-adoption does not touch the optimizer
    assert all(a is b for a, b in zip((adam.grads, adam.m, adam.v), kept))
    assert [float(t[0]) for t in kept] == [1.0, 2.0, 3.0] and adam.step_count == 9
    adam.reset()
    assert adam.step_count == 0
    for t in (adam.grads, adam.m, adam.v):
        assert t.shape == (total,) and not t.any()


def test_pool_reuses_allocates_and_keeps_the_larger_buffer():
    pool = WorkspacePool()
    a, fresh = pool.take(100, CPU)
    assert fresh and a.dtype == torch.uint8 and a.numel() >= 100
    pool.give_back(a)
    b, fresh = pool.take(50, CPU)
    assert b is a and not fresh
    pool.give_back(b)
    c, fresh = pool.take(200, CPU)
    assert fresh and c is not a and c.numel() >= 200
    # `a` went out with the take above and was dropped for the larger one: the pool is empty, and keeps the larger of two
    pool.give_back(c)
    pool.give_back(a)
    d, fresh = pool.take(150, CPU)
    assert d is c and not fresh
    # a free buffer on another device is not handed out
    pool.give_back(d)
    e, fresh = pool.take(10, torch.device("meta"))
    assert fresh and e.device.type == "meta"


def test_holder_grows_only_and_drops_the_old_buffer_first():
    holder = Workspace()
    a = holder.grow(100, CPU)
    assert a.dtype == torch.uint8 and a.numel() == 100
    assert holder.grow(40, CPU) is a and holder.grow(100, CPU) is a
    old = weakref.ref(a)
    del a
    b = holder.grow(101, CPU)
    gc.collect()
    assert b.numel() == 101 and old() is None and holder.grow(1, CPU) is b
    holder.release()
    assert holder.buf is None
    assert holder.grow(8, CPU).numel() == 8
