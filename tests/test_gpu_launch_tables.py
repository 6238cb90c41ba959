"""-m gpu: the SIREN, ERD, PIA and jet launch families share one table (csrc/api.hip, bases in csrc/common.h) and are read
through three entry points.  One small run of each of the three newer families must count in its own families and in no other's:
an offset that made two families share a slot would show here."""
import ctypes

import pytest
import torch

import erd_common
import jet_common as jc
import pia_net_common
from mri_super_resolution_amd import _lib, erd_inr, ops, pia_net

pytestmark = pytest.mark.gpu

ERD_IDS = {"erd_step": _lib.INR_LF_ERD_STEP, "erd_reduce": _lib.INR_LF_ERD_REDUCE, "erd_forward": _lib.INR_LF_ERD_FORWARD,
           "erd_soft": _lib.INR_LF_ERD_SOFT}


def _all_counts():
    out = {"siren": ops.launch_counts(), "pia": ops.pia_launch_counts(), "jet": ops.jet_launch_counts(), "erd": {}}
    for name, fam in ERD_IDS.items():
        n = ctypes.c_int64(-1)
        assert _lib.lib().inr_launch_count(fam, ctypes.byref(n)) == 0
        out["erd"][name] = int(n.value)
    return out


def _assert_only(counts, table, hit):
    for name in hit:
        assert counts[table][name] > 0, (table, name, counts)
    for t, fams in counts.items():
        for name, n in fams.items():
            if t != table or name not in hit:
                assert n == 0, (t, name, counts)


def test_launch_tables_do_not_alias(golden):
    # the smallest derivative evaluation of test_gpu_jet.py
    name = min(jc.CASES, key=lambda k: (jc.CASES[k]["hidden"], jc.CASES[k]["hidden_layers"], k))
    desc, flat, x, B = jc.on_device(jc.make_case(**jc.CASES[name]))
    ops.launch_counts_reset()
    ops.siren_jet(desc, flat, x=x, B=B, chunk_rows=jc.CHUNK)
    _assert_only(_all_counts(), "jet", ("jet_input", "jet_layer", "jet_head"))

    # the 512-row fused step of test_gpu_pia_net.py
    torch.manual_seed(0)
    fitter = pia_net.PiaFitter(pia_net.PIA().cuda(), lr=0.0)
    xb = torch.from_numpy(golden("pia_net.npz")["batch/x"]).cuda()
    pids = torch.from_numpy(pia_net_common.pids_map()).cuda()
    ops.launch_counts_reset()
    fitter.step(xb, pids)
    _assert_only(_all_counts(), "pia", ("pia_fwd", "pia_dx", "pia_dw", "pia_head"))

    # one pre-training step of the smallest network of test_gpu_erd_inr.py
    model, xe, targets, _ = erd_common.make_case(erd_inr.ErdSiren, 64, 1)
    f = erd_inr.ErdFitter(model.cuda())
    status = f.new_status(torch.device("cuda"))
    ops.launch_counts_reset()
    f.pretrain_steps(xe.cuda(), targets[0].cuda(), 1, 3e-4, -1.0, status)
    torch.cuda.synchronize()
    _assert_only(_all_counts(), "erd", ("erd_step", "erd_reduce"))
