"""Workspace planners and their entry points, without a GPU.

(a) Every ``inr_*_workspace_bytes`` export is pinned at a regular and a ragged shape.  The numbers were recorded from the library
    as it stood BEFORE the planners became the null-base call of each unit's workspace view (csrc/common.h: WsCarver): callers
    have allocated by them so far, and a view that sizes a workspace differently is a bug.  The two RAMS planners were upper
    estimates with slack; they are pinned twice -- the earlier value as a bound that must never be exceeded, and the exact
    carve.
(b) Every entry point that takes ``workspace, workspace_bytes`` refuses one byte less than its planner asks for with
    INR_E_WORKSPACE before any device work: the calls below pass pointers that are never dereferenced and run on a machine
    with no HIP device.  (For ``inr_rams_train_grads`` this is what shows that the check precedes the launches.)
"""
import ctypes as C

import pytest

from mri_super_resolution_amd import _lib

S = lambda *a: C.byref(_lib.SirenDesc(*a, 30.0, 30.0))
WIRE = lambda i, h, l: C.byref(_lib.WireDesc(i, h, l, 1, 10.0, 10.0, 10.0, 10.0))
RAMS = lambda scale, n: C.byref(_lib.RamsDesc(scale, 32, 3, 9, 8, n, 7433.6436, 2353.0723))


def PIA(hidden):
    d = _lib.PiaDesc()
    d.n_signals, d.n_hidden, d.predictor_depth, d.n_b, d.n_te, d.leaky_slope = 16, len(hidden), 1, 4, 4, 0.01
    for i, h in enumerate(hidden):
        d.hidden[i] = h
    for i in range(4):
        d.b_values[i] = 500.0 * i
        d.te_values[i] = 60.0 + 20.0 * i
    for c in range(3):
        d.D_mean[c], d.D_delta[c], d.T2_mean[c], d.T2_delta[c] = 1.5, 1.0, 100.0, 50.0
    return C.byref(d)


# planner, arguments (a tuple starting with a descriptor tag is resolved by DESC), value before the views
PINNED = [
    ("inr_mse_workspace_bytes", (4096,), 16),
    ("inr_mse_workspace_bytes", (3601,), 16),
    ("inr_head_backward_workspace_bytes", (4096, 512, 1), 262144),
    ("inr_head_backward_workspace_bytes", (3601, 64, 1), 28928),
    ("inr_head_backward_workspace_bytes", (3601, 48, 3), 65088),
    ("inr_sine_layer_backward_input_workspace_bytes", (4096, 512), 262144),
    ("inr_sine_layer_backward_input_workspace_bytes", (3601, 64), 28928),
    ("inr_linear_param_grad_workspace_bytes", (4096, 256, 512), 8388608),
    ("inr_linear_param_grad_workspace_bytes", (3601, 2, 64), 28928),
    ("inr_metric_workspace_bytes", (1,), 512),
    ("inr_metric_workspace_bytes", (7,), 3584),
    ("inr_resize_z_cubic_workspace_bytes", (4096, 20), 655360),
    ("inr_resize_z_cubic_workspace_bytes", (3601, 7), 201656),
    ("inr_rams_shift_loss_workspace_bytes", (4, 3), 1568),
    ("inr_rams_shift_loss_workspace_bytes", (7, 2), 1400),
    ("inr_rams_shift_loss_grad_workspace_bytes", (4, 3), 1592),
    ("inr_rams_shift_loss_grad_workspace_bytes", (7, 2), 1436),
    ("inr_rams_shift_ssim_workspace_bytes", (2, 24, 3), 18816),
    ("inr_rams_shift_ssim_workspace_bytes", (7, 96, 3), 2120272),
    ("inr_rams_shift_ssim_workspace_bytes", (3, 37, 2), 90480),
    ("inr_rams_shift_ssim_grad_workspace_bytes", (2, 24, 3), 27112),
    ("inr_rams_shift_ssim_grad_workspace_bytes", (7, 96, 3), 3650112),
    ("inr_rams_shift_ssim_grad_workspace_bytes", (3, 37, 2), 154864),
    ("inr_rams_conv3d_dgrad_workspace_bytes", (), 110848),
    ("inr_rams_conv3d_wgrad_workspace_bytes", (1, 10, 10, 9, 1), 116929024),
    ("inr_rams_conv3d_wgrad_workspace_bytes", (3, 13, 11, 7, 0), 116929024),
    ("inr_wire_layer_workspace_bytes", (4096, 32, 32), 541184),
    ("inr_wire_layer_workspace_bytes", (3601, 3, 64), 494848),
    ("inr_wire_layer_workspace_bytes", (100, 512, 256), 2306048),
    ("inr_wire_layer_workspace_bytes", (3601, 40, 128), 1054976),
    ("inr_siren_fit_workspace_bytes", (("siren", (64, 128, 1, 1)), 4096), 11581952),
    ("inr_siren_forward_workspace_bytes", (("siren", (64, 128, 1, 1)), 4096), 5443840),
    ("inr_siren_reconstruct_workspace_bytes", (("siren", (64, 128, 1, 1)), 4096), 6492416),
    ("inr_siren_fit_workspace_bytes", (("siren", (64, 128, 1, 1)), 3601), 10301440),
    ("inr_siren_forward_workspace_bytes", (("siren", (64, 128, 1, 1)), 3601), 4810240),
    ("inr_siren_reconstruct_workspace_bytes", (("siren", (64, 128, 1, 1)), 3601), 5732096),
    ("inr_siren_fit_workspace_bytes", (("siren", (2, 32, 1, 1)), 4096), 3230464),
    ("inr_siren_forward_workspace_bytes", (("siren", (2, 32, 1, 1)), 4096), 1094400),
    ("inr_siren_reconstruct_workspace_bytes", (("siren", (2, 32, 1, 1)), 4096), 1127168),
    ("inr_siren_fit_workspace_bytes", (("siren", (2, 32, 1, 1)), 3601), 2856704),
    ("inr_siren_forward_workspace_bytes", (("siren", (2, 32, 1, 1)), 3601), 964096),
    ("inr_siren_reconstruct_workspace_bytes", (("siren", (2, 32, 1, 1)), 3601), 993024),
    ("inr_siren_fit_workspace_bytes", (("siren", (3, 48, 2, 3)), 4096), 5056000),
    ("inr_siren_forward_workspace_bytes", (("siren", (3, 48, 2, 3)), 4096), 1664512),
    ("inr_siren_reconstruct_workspace_bytes", (("siren", (3, 48, 2, 3)), 4096), 1713664),
    ("inr_siren_fit_workspace_bytes", (("siren", (3, 48, 2, 3)), 3601), 4459264),
    ("inr_siren_forward_workspace_bytes", (("siren", (3, 48, 2, 3)), 3601), 1468672),
    ("inr_siren_reconstruct_workspace_bytes", (("siren", (3, 48, 2, 3)), 3601), 1511936),
    ("inr_erd_workspace_bytes", (("siren", (2, 64, 1, 1)), 4096), 8754192),
    ("inr_erd_workspace_bytes", (("siren", (2, 64, 1, 1)), 3601), 7748592),
    ("inr_erd_workspace_bytes", (("siren", (3, 128, 4, 1)), 4096), 63968272),
    ("inr_erd_workspace_bytes", (("siren", (3, 128, 4, 1)), 3601), 56731120),
    ("inr_siren_jet_workspace_bytes", (("siren", (2, 32, 1, 1)), 2, 0, 4096, 1), 4194304),
    ("inr_siren_jet_workspace_bytes", (("siren", (2, 32, 1, 1)), 2, 0, 3601, 1), 3687424),
    ("inr_siren_jet_workspace_bytes", (("siren", (64, 128, 2, 1)), 3, 32, 4096, 0), 16777216),
    ("inr_siren_jet_workspace_bytes", (("siren", (64, 128, 2, 1)), 3, 32, 3601, 0), 14749696),
    ("inr_siren_jet_workspace_bytes", (("siren", (40, 96, 2, 1)), 2, 20, 4096, 1), 12582912),
    ("inr_siren_jet_workspace_bytes", (("siren", (40, 96, 2, 1)), 2, 20, 3601, 1), 11062272),
    ("inr_wire_workspace_bytes", (("wire", (32, 32, 1)), 4096, 0), 2663424),
    ("inr_wire_workspace_bytes", (("wire", (32, 32, 1)), 4096, 1), 6991104),
    ("inr_wire_workspace_bytes", (("wire", (32, 32, 1)), 4096, 2), 6898688),
    ("inr_wire_reconstruct_workspace_bytes", (("wire", (32, 32, 1)), 4096), 3187712),
    ("inr_wire_workspace_bytes", (("wire", (32, 32, 1)), 3601, 0), 2346752),
    ("inr_wire_workspace_bytes", (("wire", (32, 32, 1)), 3601, 1), 6163968),
    ("inr_wire_workspace_bytes", (("wire", (32, 32, 1)), 3601, 2), 6075136),
    ("inr_wire_reconstruct_workspace_bytes", (("wire", (32, 32, 1)), 3601), 2807808),
    ("inr_wire_workspace_bytes", (("wire", (2, 64, 0)), 4096, 0), 4736000),
    ("inr_wire_workspace_bytes", (("wire", (2, 64, 0)), 4096, 1), 6902528),
    ("inr_wire_workspace_bytes", (("wire", (2, 64, 0)), 4096, 2), 6834176),
    ("inr_wire_reconstruct_workspace_bytes", (("wire", (2, 64, 0)), 4096), 4768768),
    ("inr_wire_workspace_bytes", (("wire", (2, 64, 0)), 3601, 0), 4165888),
    ("inr_wire_workspace_bytes", (("wire", (2, 64, 0)), 3601, 1), 6075392),
    ("inr_wire_workspace_bytes", (("wire", (2, 64, 0)), 3601, 2), 6010624),
    ("inr_wire_reconstruct_workspace_bytes", (("wire", (2, 64, 0)), 3601), 4194816),
    ("inr_wire_workspace_bytes", (("wire", (40, 256, 3)), 4096, 0), 24264704),
    ("inr_wire_workspace_bytes", (("wire", (40, 256, 3)), 4096, 1), 118682368),
    ("inr_wire_workspace_bytes", (("wire", (40, 256, 3)), 4096, 2), 114524160),
    ("inr_wire_reconstruct_workspace_bytes", (("wire", (40, 256, 3)), 4096), 24920064),
    ("inr_wire_workspace_bytes", (("wire", (40, 256, 3)), 3601, 0), 22110464),
    ("inr_wire_workspace_bytes", (("wire", (40, 256, 3)), 3601, 1), 106386944),
    ("inr_wire_workspace_bytes", (("wire", (40, 256, 3)), 3601, 2), 102232320),
    ("inr_wire_reconstruct_workspace_bytes", (("wire", (40, 256, 3)), 3601), 22686720),
    ("inr_pia_workspace_bytes", (("pia", ((256,),)), 4096, 0), 20971520),
    ("inr_pia_workspace_bytes", (("pia", ((256,),)), 4096, 1), 82585856),
    ("inr_pia_workspace_bytes", (("pia", ((256,),)), 3601, 0), 18437120),
    ("inr_pia_workspace_bytes", (("pia", ((256,),)), 3601, 1), 51500032),
    ("inr_pia_workspace_bytes", (("pia", ((32, 64, 128, 256, 512),)), 4096, 0), 41943040),
    ("inr_pia_workspace_bytes", (("pia", ((32, 64, 128, 256, 512),)), 4096, 1), 182488320),
    ("inr_pia_workspace_bytes", (("pia", ((32, 64, 128, 256, 512),)), 3601, 0), 36874240),
    ("inr_pia_workspace_bytes", (("pia", ((32, 64, 128, 256, 512),)), 3601, 1), 118431744),
    ("inr_pia_workspace_bytes", (("pia", ((48, 512),)), 4096, 0), 41943040),
    ("inr_pia_workspace_bytes", (("pia", ((48, 512),)), 4096, 1), 137092352),
    ("inr_pia_workspace_bytes", (("pia", ((48, 512),)), 3601, 0), 36874240),
    ("inr_pia_workspace_bytes", (("pia", ((48, 512),)), 3601, 1), 99661824),
]
DESC = {"siren": S, "wire": WIRE, "rams": RAMS, "pia": PIA}

# RAMS forward / training planners at (scale, n_rfab, B, H = W): (the earlier estimate, the exact carve)
RAMS_PINNED = [
    (3, 1, 1, 8, (3056192, 3022636), (130986356, 126643456)),
    (3, 1, 3, 8, (4751040, 4714892), (138570420, 132913920)),
    (3, 1, 2, 13, (5626160, 5589868), (142738052, 136540672)),
    (3, 1, 33, 16, (80370240, 80257196), (484953972, 425006848)),
    (3, 12, 1, 8, (5759552, 5725996), (144919044, 140579840)),
    (3, 12, 3, 8, (7454400, 7418252), (160115460, 154459136)),
    (3, 12, 2, 13, (8329520, 8293228), (169980916, 163782656)),
    (3, 12, 33, 16, (83073600, 82960556), (901698564, 841710080)),
    (2, 2, 1, 8, (3299392, 3265836), (132241956, 127900672)),
    (2, 2, 3, 8, (4989120, 4952972), (140502692, 134850048)),
    (2, 2, 2, 13, (5858400, 5822108), (145170788, 138980608)),
    (2, 2, 33, 16, (80278080, 80165036), (521822756, 462040832)),
]


def _resolve(args):
    if args and isinstance(args[0], tuple):
        kind, spec = args[0]
        return (DESC[kind](*spec),) + tuple(args[1:])
    return args


@pytest.mark.parametrize("name,args,want", PINNED, ids=[f"{n}{a}".replace(" ", "") for n, a, _ in PINNED])
def test_planner_values_are_the_recorded_ones(name, args, want):
    assert getattr(_lib.lib(), name)(*_resolve(args)) == want


def test_every_planner_is_pinned():
    planners = {n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")}
    pinned = {n for n, _, _ in PINNED} | {"inr_rams_workspace_bytes", "inr_rams_train_workspace_bytes"}
    # fit / forward / reconstruct of the two networks of tests/test_abi_cpu.py are pinned there as well
    assert planners == pinned, planners ^ pinned


@pytest.mark.parametrize("scale,n_rfab,B,H,fwd,train", RAMS_PINNED)
def test_rams_planners_are_exact_and_never_above_the_earlier_estimate(scale, n_rfab, B, H, fwd, train):
    lib = _lib.lib()
    got = (lib.inr_rams_workspace_bytes(RAMS(scale, n_rfab), B, H, H), lib.inr_rams_train_workspace_bytes(RAMS(scale, n_rfab), B, H, H))
    assert got == (fwd[1], train[1])
    assert fwd[1] <= fwd[0] and train[1] <= train[0]


fake = lambda k: C.c_void_p(0x7000_0000_0000 + 4096 * k)      # never dereferenced: the calls fail in validation
P = [fake(k) for k in range(16)]
ADAM = (1e-4, 0.9, 0.999, 1e-8)


def _ptr_array(*ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _too_small_cases():
    """(id, planner bytes, call(workspace_bytes) -> status) for every entry point with a workspace."""
    lib = _lib.lib()
    sd, n = _lib.SirenDesc(64, 128, 1, 1, 30.0, 30.0), 300
    sdp = C.byref(sd)
    fit_b, fwd_b = lib.inr_siren_fit_workspace_bytes(sdp, n), lib.inr_siren_forward_workspace_bytes(sdp, n)
    tiny = C.byref(_lib.SirenDesc(2, 64, 2, 1, 30.0, 30.0))      # a small-path network: its fused step carves the same bytes
    tiny_b = lib.inr_siren_fit_workspace_bytes(tiny, 130)
    shape2 = _lib.shape_array((9, 7))
    yield "mse", lib.inr_mse_workspace_bytes(3601), lambda b: lib.inr_mse_loss_grad(P[0], P[1], P[2], P[3], None, 3601, P[4], b, None)
    yield "head_backward", lib.inr_head_backward_workspace_bytes(3601, 64, 1), lambda b: lib.inr_linear_head_backward(
        P[0], P[1], P[2], P[3], P[4], P[5], P[6], P[7], 3601, 64, 1, P[8], b, None)
    yield "input_grad", lib.inr_sine_layer_backward_input_workspace_bytes(3601, 64), lambda b: lib.inr_sine_layer_backward_input(
        P[0], P[1], P[2], P[3], P[4], 3601, 64, 64, P[5], b, None)
    yield "param_grad", lib.inr_linear_param_grad_workspace_bytes(3601, 2, 64), lambda b: lib.inr_linear_param_grad(
        P[0], P[1], P[2], P[3], 3601, 2, 64, P[4], b, None)
    yield "siren_forward", fwd_b, lambda b: lib.inr_siren_forward(sdp, P[0], P[1], n, P[2], 0, 0.0, P[3], b, None)
    yield "siren_reconstruct", lib.inr_siren_reconstruct_workspace_bytes(C.byref(_lib.SirenDesc(2, 64, 2, 1, 30.0, 30.0)), 32), \
        lambda b: lib.inr_siren_reconstruct(tiny, P[0], shape2, 2, None, 0, P[1], 0, 0.0, 32, P[2], b, None)
    yield "siren_fit", fit_b, lambda b: lib.inr_siren_fit(sdp, P[0], P[1], P[2], P[3], P[4], P[5], None, n, 1, 2, *ADAM, None, P[6], b, None)
    yield "siren_fit_small", tiny_b, lambda b: lib.inr_siren_fit(tiny, P[0], P[1], P[2], P[3], P[4], P[5], None, 130, 1, 2, *ADAM, None,
                                                                 P[6], b, None)
    yield "siren_fit_cycle", fit_b, lambda b: lib.inr_siren_fit_cycle(sdp, P[0], P[1], P[2], P[3], P[4], P[5], None, 2, 0, n, 1, 2, *ADAM,
                                                                      None, P[6], b, None)
    one = (C.c_int * 2)(1, 1)
    zero = (C.c_int * 2)(0, 0)
    yield "siren_fit_cycle_batch", tiny_b, lambda b: lib.inr_siren_fit_cycle_batch(
        tiny, 2, _ptr_array(P[0], P[1]), _ptr_array(P[2], P[3]), _ptr_array(P[4], P[5]), _ptr_array(P[6], P[7]), P[8],
        _ptr_array(P[9], P[10]), None, one, zero, 130, 1, 2, *ADAM, None, _ptr_array(P[11], P[12]), b, None)
    yield "siren_loss_grad", fit_b, lambda b: lib.inr_siren_loss_grad(sdp, P[0], P[1], P[2], P[3], None, n, 0, P[4], P[5], b, None)
    yield "siren_loss_grad_ex", fit_b, lambda b: lib.inr_siren_loss_grad_ex(sdp, P[0], P[1], P[2], P[3], None, n, 0, P[4], P[5], b, 0, None)
    yield "siren_forward_train", fit_b, lambda b: lib.inr_siren_forward_train(sdp, P[0], P[1], P[2], n, P[3], b, 0, None)
    yield "siren_backward_train", fit_b, lambda b: lib.inr_siren_backward_train(sdp, P[0], P[1], P[2], n, P[3], b, None)
    yield "psnr", lib.inr_metric_workspace_bytes(7), lambda b: lib.inr_psnr(P[0], P[1], P[2], 7, 100, 1.0, P[3], b, None)
    yield "ssim2d", lib.inr_metric_workspace_bytes(7), lambda b: lib.inr_ssim2d(P[0], P[1], P[2], 7, 24, 24, 7, 1.0, 0, 0.0, P[3], b, None)
    yield "resize_z", lib.inr_resize_z_cubic_workspace_bytes(3601, 7), lambda b: lib.inr_resize_z_cubic(P[0], P[1], 3601, 7, 21, P[2], b, None)
    yield "shift_loss", lib.inr_rams_shift_loss_workspace_bytes(7, 2), lambda b: lib.inr_rams_shift_loss(
        P[0], P[1], P[2], P[3], 7, 24, 2, 0, P[4], b, None)
    yield "shift_loss_grad", lib.inr_rams_shift_loss_grad_workspace_bytes(7, 2), lambda b: lib.inr_rams_shift_loss_grad(
        P[0], P[1], P[2], P[3], P[4], None, 7, 24, 2, P[5], b, None)
    yield "shift_ssim", lib.inr_rams_shift_ssim_workspace_bytes(2, 24, 3), lambda b: lib.inr_rams_shift_ssim(
        P[0], P[1], P[2], P[3], 2, 24, 3, 0, P[4], b, None)
    yield "shift_ssim_grad", lib.inr_rams_shift_ssim_grad_workspace_bytes(2, 24, 3), lambda b: lib.inr_rams_shift_ssim_grad(
        P[0], P[1], P[2], P[3], P[4], None, 2, 24, 3, 0, P[5], b, None)
    yield "conv3d_dgrad", lib.inr_rams_conv3d_dgrad_workspace_bytes(), lambda b: lib.inr_rams_conv3d_dgrad(
        P[0], P[1], P[2], 1, 10, 10, 9, P[3], b, None)
    yield "conv3d_wgrad", lib.inr_rams_conv3d_wgrad_workspace_bytes(1, 10, 10, 9, 1), lambda b: lib.inr_rams_conv3d_wgrad(
        P[0], P[1], P[2], P[3], 1, 10, 10, 9, 1, P[4], b, None)
    rd = RAMS(3, 1)
    yield "rams_forward", lib.inr_rams_workspace_bytes(rd, 3, 8, 8), lambda b: lib.inr_rams_forward(rd, P[0], P[1], P[2], 3, 8, 8, 0, P[3], b, None)
    rt_b = lib.inr_rams_train_workspace_bytes(rd, 1, 8, 8)
    yield "rams_train_grads", rt_b, lambda b: lib.inr_rams_train_grads(rd, P[0], P[1], P[2], P[3], P[4], P[5], None, 1, 8, 8, P[6], b, None)
    yield "rams_train_step", rt_b, lambda b: lib.inr_rams_train_step(rd, P[0], P[1], P[2], P[3], P[4], P[5], P[6], P[7], 1, 8, 8, 1, *ADAM,
                                                                    P[8], b, None)
    pd = PIA((256,))
    pf, pt = lib.inr_pia_workspace_bytes(pd, 70, 0), lib.inr_pia_workspace_bytes(pd, 70, 1)
    yield "pia_forward", pf, lambda b: lib.inr_pia_forward(pd, P[0], P[1], 70, P[2], P[3], P[4], P[5], 70, P[6], b, None)
    yield "pia_forward_train", pt, lambda b: lib.inr_pia_forward_train(pd, P[0], P[1], 70, P[2], P[3], P[4], P[5], P[6], b, None)
    yield "pia_backward_train", pt, lambda b: lib.inr_pia_backward_train(pd, P[0], P[1], P[2], P[3], P[4], P[5], P[6], 70, P[7], b, None)
    yield "pia_fit_step", pt, lambda b: lib.inr_pia_fit_step(pd, P[0], P[1], P[2], P[3], P[4], P[5], 70, 1, *ADAM, P[6], P[7], b, None)
    ed = S(2, 64, 1, 1)
    eb = lib.inr_erd_workspace_bytes(ed, 70)
    yield "erd_loss_grad", eb, lambda b: lib.inr_erd_loss_grad(ed, P[0], P[1], P[2], P[3], None, 70, 0, 0.1, 1, 0, P[4], P[5], b, None)
    yield "erd_pretrain", eb, lambda b: lib.inr_erd_pretrain(ed, P[0], P[1], P[2], P[3], P[4], P[5], 70, 1, 2, *ADAM, 0.5, P[6], P[7], b, None)
    yield "erd_finetune", eb, lambda b: lib.inr_erd_finetune(ed, P[0], P[1], P[2], P[3], P[4], P[5], None, 2, 70, 0.1, 1, 2, 1e-4, *ADAM,
                                                             None, P[6], b, None)
    jd = S(2, 32, 1, 1)
    jb = lib.inr_siren_jet_workspace_bytes(jd, 2, 0, 32, 1)
    yield "siren_jet", jb, lambda b: lib.inr_siren_jet(jd, P[0], P[1], 50, 2, 2, None, 0, P[2], P[3], P[4], 32, P[5], b, None)
    yield "siren_jet_grid", jb, lambda b: lib.inr_siren_jet_grid(jd, P[0], shape2, 2, 2, None, 0, P[1], P[2], P[3], 32, P[4], b, None)
    wd = WIRE(32, 32, 1)
    wb = [lib.inr_wire_workspace_bytes(wd, 100, mode) for mode in (0, 1, 2)]
    yield "wire_layer_forward", lib.inr_wire_layer_workspace_bytes(100, 3, 32), lambda b: lib.inr_wire_layer_forward(
        P[0], P[1], P[2], P[3], P[4], P[5], 100, 3, 32, 1, 10.0, 10.0, P[6], b, None)
    yield "wire_forward", wb[0], lambda b: lib.inr_wire_forward(wd, P[0], P[1], 100, P[2], P[3], b, None)
    w2 = WIRE(2, 32, 1)
    yield "wire_reconstruct", lib.inr_wire_reconstruct_workspace_bytes(w2, 32), lambda b: lib.inr_wire_reconstruct(
        w2, P[0], shape2, 2, None, 0, P[1], 0, 0.0, 32, P[2], b, None)
    yield "wire_loss_grad", wb[1], lambda b: lib.inr_wire_loss_grad(wd, P[0], P[1], P[2], P[3], None, 100, P[4], P[5], b, None)
    yield "wire_fit", wb[1], lambda b: lib.inr_wire_fit(wd, P[0], P[1], P[2], P[3], P[4], P[5], None, 100, 1, 2, *ADAM, None, P[6], b, None)
    yield "wire_forward_stash", wb[2], lambda b: lib.inr_wire_forward_stash(wd, P[0], P[1], 100, P[2], P[3], b, None)
    yield "wire_input_grad", wb[2], lambda b: lib.inr_wire_input_grad(wd, P[0], P[1], 100, P[2], P[3], b, None)


def test_every_entry_point_with_a_workspace_is_in_the_table():
    with_ws = {n for n, (_, argtypes) in _lib.SIGNATURES.items()
               if any(a is C.c_void_p and b is C.c_size_t for a, b in zip(argtypes, argtypes[1:])) or n == "inr_siren_fit_cycle_batch"}
    covered = {"inr_mse_loss_grad", "inr_linear_head_backward", "inr_sine_layer_backward_input", "inr_linear_param_grad",
               "inr_siren_forward", "inr_siren_reconstruct", "inr_siren_fit", "inr_siren_fit_cycle", "inr_siren_fit_cycle_batch",
               "inr_siren_loss_grad", "inr_siren_loss_grad_ex", "inr_siren_forward_train", "inr_siren_backward_train", "inr_psnr",
               "inr_ssim2d", "inr_resize_z_cubic", "inr_rams_shift_loss", "inr_rams_shift_loss_grad", "inr_rams_shift_ssim",
               "inr_rams_shift_ssim_grad", "inr_rams_conv3d_dgrad", "inr_rams_conv3d_wgrad", "inr_rams_forward",
               "inr_rams_train_grads", "inr_rams_train_step", "inr_pia_forward", "inr_pia_forward_train", "inr_pia_backward_train",
               "inr_pia_fit_step", "inr_erd_loss_grad", "inr_erd_pretrain", "inr_erd_finetune", "inr_siren_jet",
               "inr_siren_jet_grid", "inr_wire_layer_forward", "inr_wire_forward", "inr_wire_reconstruct", "inr_wire_loss_grad",
               "inr_wire_fit", "inr_wire_forward_stash", "inr_wire_input_grad"}
    assert with_ws == covered, with_ws ^ covered


_CASE_IDS = ["mse", "head_backward", "input_grad", "param_grad", "siren_forward", "siren_reconstruct", "siren_fit", "siren_fit_small",
             "siren_fit_cycle", "siren_fit_cycle_batch", "siren_loss_grad", "siren_loss_grad_ex", "siren_forward_train",
             "siren_backward_train", "psnr", "ssim2d", "resize_z", "shift_loss", "shift_loss_grad", "shift_ssim", "shift_ssim_grad",
             "conv3d_dgrad", "conv3d_wgrad", "rams_forward", "rams_train_grads", "rams_train_step", "pia_forward", "pia_forward_train",
             "pia_backward_train", "pia_fit_step", "erd_loss_grad", "erd_pretrain", "erd_finetune", "siren_jet", "siren_jet_grid",
             "wire_layer_forward", "wire_forward", "wire_reconstruct", "wire_loss_grad", "wire_fit", "wire_forward_stash",
             "wire_input_grad"]


@pytest.mark.parametrize("case", _CASE_IDS)
def test_one_byte_too_few_is_refused_before_device_work(case):
    lib = _lib.lib()
    table = {k: (need, call) for k, need, call in _too_small_cases()}
    assert sorted(table) == sorted(_CASE_IDS)
    need, call = table[case]
    assert need > 0, lib.inr_last_error()
    rc = call(need - 1)
    if case == "siren_backward_train":
        # the one entry point whose size check cannot be reached without a GPU: it first asks for the pending
        # inr_siren_forward_train on this workspace (a host-side stamp that only a forward that ran can leave), and refuses
        # with INR_E_INVALID -- earlier still, and as much "before device work"
        assert rc == _lib.INR_E_INVALID and b"pending on this workspace" in lib.inr_last_error(), (rc, lib.inr_last_error())
        return
    assert rc == _lib.INR_E_WORKSPACE, (rc, lib.inr_last_error())
    assert b"workspace" in lib.inr_last_error()
