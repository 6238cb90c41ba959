"""CPU-side checks of the PIA autoencoder port: construction, parameter layout, the synthetic generator, the float64
restatement the GPU tests rely on, the drop-in module and the refusal to run without a HIP device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import mri_super_resolution_amd as inr
from mri_super_resolution_amd import _lib, pia_net

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pia_net_common as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_init_is_bit_identical_to_reference_and_state_dict_matches(golden):
    g = golden("pia_net.npz")
    torch.manual_seed(0)
    m = pia_net.PIA()
    names = [str(n) for n in g["param_names"]]
    assert names == C.PARAM_NAMES and len(names) == 22
    assert list(m.state_dict().keys()) == names
    assert [n for n, _ in m.named_parameters()] == names
    shapes = [tuple(int(s) for s in str(t).split(",")) for t in g["param_shapes"]]
    assert [tuple(p.shape) for p in m.parameters()] == shapes == [tuple(s) for s in C.PARAM_SHAPES]
    for n, p in m.named_parameters():
        assert C.sha(p.detach().cpu().numpy()) == str(g[f"init_sha/{n}"]), n
    assert sum(p.numel() for p in m.parameters()) == C.PARAM_COUNT


def test_get_batch_follows_the_reference_draws(golden):
    """Same seed, same batch.  The vectorised expression evaluates the reference's float64 formula in the reference's order;
    numpy's array `exp` may differ from its scalar `exp` by a few float64 ulp (1e-16 relative), which the float32 results
    show as at most one float32 ulp: 6e-8 relative, i.e. 6.1e-5 absolute at the signals' scale of 1000 -- the bounds below
    are two such ulps."""
    g = golden("pia_net.npz")
    np.random.seed(1)
    out = pia_net.get_batch(512, 0.02)
    assert [t.dtype for t in out] == [torch.float32] * 5 and [tuple(t.shape) for t in out] == [(512, 16), (512, 3), (512, 3),
                                                                                                 (512, 3), (512, 16)]
    x = out[0].numpy()
    print("get_batch max |x - ref| =", np.abs(x - g["batch/x"]).max())
    assert np.allclose(x, g["batch/x"], rtol=1.2e-7, atol=1.3e-4)
    for k, t in zip(("D", "T2", "v", "clean"), out[1:]):
        assert np.allclose(C.sample(t.numpy()), g[f"batch/{k}"], rtol=1.2e-7, atol=1.3e-4 if k == "clean" else 0), k


def _default_desc():
    torch.manual_seed(0)
    return pia_net._as_desc(pia_net.PIA())


def test_param_layout_and_descriptor_validation():
    lib = _lib.lib()
    d = _default_desc()
    assert lib.inr_pia_param_count(ctypes.byref(d)) == C.PARAM_COUNT
    total, offs = pia_net.pia_param_layout(d)
    sizes = [int(np.prod(s)) for s in C.PARAM_SHAPES]
    assert total == C.PARAM_COUNT and offs == [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
    small = (ctypes.c_int64 * 4)()
    assert lib.inr_pia_param_offsets(ctypes.byref(d), small, 4) == _lib.INR_E_INVALID
    assert lib.inr_pia_workspace_bytes(ctypes.byref(d), 512, 1) > 512 * (992 + 3 * 512) * 4
    assert lib.inr_pia_workspace_bytes(ctypes.byref(d), 512, 0) >= 512 * 5 * 512 * 4
    # bad descriptors are refused before any device work
    for field, value in (("n_signals", 0), ("n_hidden", 0), ("n_hidden", 9), ("predictor_depth", 0), ("n_b", 3)):
        bad = _default_desc()
        setattr(bad, field, value)
        assert lib.inr_pia_param_count(ctypes.byref(bad)) == -1 and b"bad pia descriptor" in lib.inr_last_error(), field
    fake = lambda k: ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)      # never dereferenced: the calls fail in validation
    deep = _default_desc()
    deep.predictor_depth = 2
    assert lib.inr_pia_param_count(ctypes.byref(deep)) == C.PARAM_COUNT + 3 * (512 * 512 + 512)
    assert lib.inr_pia_workspace_bytes(ctypes.byref(deep), 512, 1) == 0
    rc = lib.inr_pia_forward(ctypes.byref(deep), fake(1), fake(2), 8, fake(3), fake(4), fake(5), fake(6), 8, fake(7), 1 << 30, None)
    assert rc == _lib.INR_E_INVALID and b"predictor_depth" in lib.inr_last_error()
    odd = _default_desc()
    odd.hidden[1] = 72
    assert lib.inr_pia_fit_step(ctypes.byref(odd), fake(1), fake(2), fake(3), fake(4), fake(5), None, 8, 1, 1e-3, 0.9, 0.999, 1e-8,
                                fake(6), fake(7), 1 << 30, None) == _lib.INR_E_INVALID
    assert lib.inr_pia_forward(ctypes.byref(d), None, fake(2), 8, fake(3), fake(4), fake(5), fake(6), 8, fake(7), 1 << 30, None) == \
        _lib.INR_E_INVALID
    assert lib.inr_pia_forward(ctypes.byref(d), fake(1), fake(2), 8, fake(3), fake(4), fake(5), fake(6), 8, fake(7), 16, None) == \
        _lib.INR_E_WORKSPACE
    assert lib.inr_pids_slice(None, None, None, None, None, None, 4, None) == _lib.INR_E_INVALID
    n = ctypes.c_int64(-1)
    assert lib.inr_launch_counts_reset() == 0
    for fam in range(_lib.INR_PIA_LF_COUNT):
        assert lib.inr_pia_launch_count(fam, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.inr_pia_launch_count(_lib.INR_PIA_LF_COUNT, ctypes.byref(n)) == _lib.INR_E_INVALID


def test_float64_restatement_reproduces_the_reference_float64_run(golden):
    g = golden("pia_net.npz")
    torch.manual_seed(0)
    m = pia_net.PIA().cpu()
    params = [p.detach().cpu() for p in m.parameters()]
    x = torch.from_numpy(g["batch/x"])
    pids = C.pids_map()
    assert np.array_equal(C.sample(pids), g["pids"]) and C.sha(pids) == str(g["pids/sha"])
    loss, grads, outs = C.loss_and_grads64(params, x, pids)
    for k, t in zip(("signal", "D", "T2", "v"), outs):
        dev = C.rel_dev(C.sample(t.numpy()), g[f"f64/{k}"])
        print(f"restatement f64/{k}: {dev:.2e}")
        assert dev <= 1e-12, (k, dev)
    assert abs(loss.item() - float(g["f64/loss"])) <= 1e-12 * abs(float(g["f64/loss"]))
    for n, gr in zip(C.PARAM_NAMES, grads):
        dev = C.rel_dev(C.sample(gr.numpy()), g[f"f64/grad/{n}"])
        assert dev <= 1e-12, (n, dev)


def test_compat_module_exports_the_class_and_its_helpers():
    sys.path.insert(0, os.path.join(ROOT, "mri-super-resolution_amd", "compat"))
    try:
        from PIA import PIA, ADC_slice, detect_PIDS_slice, get_batch, hybrid_fit  # noqa: F401
    finally:
        sys.path.pop(0)
    assert PIA is pia_net.PIA and get_batch is pia_net.get_batch
    from mri_super_resolution_amd import pia
    assert pia.PIA is PIA and pia.PiaFitter is pia_net.PiaFitter and hybrid_fit is pia.hybrid_fit


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the refusal path is exercised on the CPU runner")
    m = pia_net.PIA()
    with pytest.raises(inr.InrDeviceError):
        m(torch.zeros(4, 16))
    with pytest.raises(inr.InrDeviceError):
        m.encode(torch.zeros(4, 16))
    with pytest.raises(inr.InrDeviceError):
        pia_net.PiaFitter(m)
    with pytest.raises(inr.InrDeviceError):
        pia_net.detect_PIDS_slice(np.array(C.B_VALUES), np.ones((2, 2, 4, 4)))
    with pytest.raises(inr.InrDeviceError):
        pia_net.ADC_slice(np.array(C.B_VALUES), np.ones((2, 2, 4)))


def test_supervised_loss_value_on_host_tensors(golden):
    """`loss_function(tissue_available=True)` is tensor arithmetic on whatever device its inputs live on: on the reference's
    float32 outputs (regenerated by the restatement to float32 precision) it evaluates, in float64, to the fixture's value
    to the precision those inputs carry."""
    g = golden("pia_net.npz")
    assert str(g["supervised_dtype"]) == "torch.float64"
    torch.manual_seed(0)
    m = pia_net.PIA().cpu()
    np.random.seed(1)
    x, D, T2, v, _ = pia_net.get_batch(512, 0.02)
    signal, D64, T264, v64 = C.forward64([p.detach() for p in m.parameters()], torch.from_numpy(g["batch/x"]))
    with torch.no_grad():
        val = m.loss_function([signal.float(), D64, T264.float(), v64.float()], [torch.from_numpy(g["batch/x"]), D, T2, v], None,
                              tissue_available=True)
    assert val.dtype == torch.float64
    assert abs(val.item() - float(g["supervised_loss"])) <= 1e-5 * float(g["supervised_loss"])


def test_superres_hybrid_parser_defaults_to_curve_fit():
    from mri_super_resolution_amd.scripts import superresHybrid
    args = superresHybrid.build_parser().parse_args(["--data", "m.mat"])
    assert args.estimator == "curve_fit" and args.pia_steps > 0 and args.pia_batch > 0 and args.pia_noise > 0
    assert superresHybrid.build_parser().parse_args(["--data", "m.mat", "--estimator", "pia"]).estimator == "pia"
    with pytest.raises(SystemExit):
        superresHybrid.build_parser().parse_args(["--data", "m.mat", "--estimator", "other"])
