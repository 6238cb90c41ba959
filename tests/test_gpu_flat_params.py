"""Re-adoption of the flat parameter buffer (flat.py) under every fitter: a model that is moved to the host and back gets
new parameter storage, and the next call has to re-flatten it -- with the optimizer state kept.  A twin that is never moved
runs the same kernels on the same bytes (fixed-order reductions), so every comparison here is exact."""
import os
import sys

import pytest
import torch

import mri_super_resolution_amd as inr
from mri_super_resolution_amd import erd_inr, ops, pia_net
from mri_super_resolution_amd import inr as inr_mod

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pia_net_common as PC  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = ("small_multi", "small_step", "small_batch")
PRESPLIT = ("hp_pkd", "hp_pkc", "hp_tile", "hp_rc", "hp_narrow", "hp_fused_fwd", "hp_row")
EXACT = ("h3", "f32_pipe16", "f32_pipe", "f32_generic")


def _twins(make, seed=5):
    out = []
    for _ in range(2):
        torch.manual_seed(seed)
        out.append(make().cuda())
    return out


def _move(model):
    """To the host and back: same values, new storage for every parameter."""
    before = [p.data_ptr() for p in model.parameters()]
    model.cpu()
    model.cuda()
    assert all(p.is_cuda and p.data_ptr() != old for p, old in zip(model.parameters(), before))


def _rows(n, fin, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, fin, generator=g) * 2 - 1).cuda(), torch.rand(n, generator=g).cuda()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


@pytest.mark.parametrize("fin,hidden,path,others", [(2, 64, SMALL, PRESPLIT + EXACT), (32, 128, PRESPLIT, SMALL + EXACT)],
                         ids=["persistent", "presplit"])
def test_siren_fitter_readopts_and_keeps_its_adam_state(fin, hidden, path, others):
    A, B = _twins(lambda: inr.Siren(fin, hidden, 1, 1))
    fa, fb = inr.SirenFitter(A, lr=1e-3), inr.SirenFitter(B, lr=1e-3)
    x, t = _rows(256, fin)
    ops.launch_counts_reset()
    la, lb = [fa.step(x, t, 3)], [fb.step(x, t, 3)]
    c = ops.launch_counts()
    assert sum(c[k] for k in path) > 0 and sum(c[k] for k in others) == 0, c
    m, v, grads, old_flat = fa.m, fa.v, fa.grads, fa.flat
    _move(A)
    la.append(fa.step(x, t, 3))
    lb.append(fb.step(x, t, 3))
    assert _same_bits(torch.cat(la), torch.cat(lb))
    for pa, pb in zip(A.layer_parameters(), B.layer_parameters()):
        assert _same_bits(pa, pb)
    assert _same_bits(fa.flat, fb.flat) and _same_bits(fa.m, fb.m) and _same_bits(fa.v, fb.v)
    assert fa.m is m and fa.v is v and fa.grads is grads and fa.step_count == 6 == fb.step_count
    assert fa.flat is not old_flat
    for p, off in zip(A.layer_parameters(), [o for pair in fa.offsets for o in pair]):
        assert p.data_ptr() == fa.flat.data_ptr() + 4 * off       # views into the new flat buffer again


def test_autograd_state_rebuilds_after_a_move():
    """``_TrainState``: after the move the flat buffer and the operand image are rebuilt, not trusted -- the gradients on the
    same input tensor are those of a freshly built model holding the same weights."""
    assert inr_mod.HP_AUTOGRAD
    torch.manual_seed(3)
    A = inr.Siren(32, 128, 1, 1).cuda()
    x, t = _rows(256, 32)

    def grads_of(model):
        for p in model.parameters():
            p.grad = None
        ops.launch_counts_reset()
        loss = ((model(x) - t.unsqueeze(1)) ** 2).mean()
        loss.backward()
        c = ops.launch_counts()
        assert sum(c[k] for k in PRESPLIT) > 0 and sum(c[k] for k in SMALL + EXACT) == 0, c
        return loss.detach().clone(), [p.grad.detach().clone() for p in model.layer_parameters()]

    grads_of(A)
    state = A.__dict__["_hp_state"]
    old_flat = state.flat
    assert state._last is not None
    _move(A)
    loss_a, ga = grads_of(A)
    assert A.__dict__["_hp_state"] is state and state.flat is not old_flat and state.params.owns(A.layer_parameters())
    fresh = inr.Siren(32, 128, 1, 1)
    fresh.load_state_dict({k: w.detach().cpu() for k, w in A.state_dict().items()})
    loss_f, gf = grads_of(fresh.cuda())
    assert _same_bits(loss_a, loss_f)
    for a, b in zip(ga, gf):
        assert _same_bits(a, b)


def test_erd_fitter_readopts_and_the_model_reads_its_live_buffer():
    A, B = _twins(lambda: erd_inr.ErdSiren(2, 64, 0, 1))
    fa, fb = erd_inr.ErdFitter(A), erd_inr.ErdFitter(B)
    x, _ = _rows(256, 2)
    g = torch.Generator().manual_seed(2)
    targets, weights = torch.rand(3, 256, generator=g).cuda(), (0.5 + torch.rand(3, 256, generator=g)).cuda()
    kw = dict(steps=2, lr_perturb=3e-4, lr_net=1e-4, new_optimizers=False)
    la, lb = [fa.finetune(x, targets, weights, **kw)], [fb.finetune(x, targets, weights, **kw)]
    m, v = fa.m, fa.v
    _move(A)
    assert not fa.owns(A)
    la.append(fa.finetune(x, targets, weights, **kw))
    lb.append(fb.finetune(x, targets, weights, **kw))
    assert _same_bits(torch.cat(la), torch.cat(lb))
    for pa, pb in zip(A.kernel_parameters(), B.kernel_parameters()):
        assert _same_bits(pa, pb)
    assert fa.owns(A) and A._flat() is fa.flat and _same_bits(fa.flat, fb.flat)
    assert fa.m is m and fa.v is v and fa.step_count == 4 == fb.step_count
    assert _same_bits(A(x, 1, 1.0 / 128.0), B(x, 1, 1.0 / 128.0))


def test_pia_fitter_readopts_and_keeps_counting():
    A, B = _twins(lambda: pia_net.PIA(hidden_dims=list(PC.SMALL_HIDDEN)), seed=0)
    fa, fb = pia_net.PiaFitter(A, lr=1e-3), pia_net.PiaFitter(B, lr=1e-3)
    x = (torch.rand(64, 16, generator=torch.Generator().manual_seed(4)) * 1000).cuda()
    la, lb = [fa.step(x), fa.step(x)], [fb.step(x), fb.step(x)]
    m, v, old_flat = fa.m, fa.v, fa.state.flat
    _move(A)
    la += [fa.step(x), fa.step(x)]
    lb += [fb.step(x), fb.step(x)]
    assert _same_bits(torch.cat(la), torch.cat(lb))
    for pa, pb in zip(A.parameters(), B.parameters()):
        assert _same_bits(pa, pb)
    assert fa.state.flat is not old_flat and _same_bits(fa.state.flat, fb.state.flat)
    assert fa.m is m and fa.v is v and fa.steps_done == 4 == fb.steps_done
