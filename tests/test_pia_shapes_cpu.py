"""CPU-side checks of the PIA shape-class table (tests/pia_shapes_common.py): the table reaches every class, the restated host
rules agree with the lines of csrc/pia.hip they cite, the generalised float64 restatement reproduces the reference's float64
run on every case of tests/golden/pia_net_shapes.npz, and tests/golden/pia_net.npz is the file it was."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

from mri_super_resolution_amd import pia_net

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pia_net_common as C  # noqa: E402
import pia_shapes_common as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIA_NET_SHA256 = "950e0af5c2f3aff3d7b6cdafff200279b8d24be481e91a373d6d48d5be109b0c"


def test_the_table_reaches_every_class():
    reached = {c.name: S.classes_of(c) for c in S.CASES}
    union = set().union(*reached.values())
    for k in S.ALL_CLASSES:
        print(f"{k}: {[n for n, r in reached.items() if k in r]}")
    assert union - set(S.ALL_CLASSES) == set(), "a class outside the list"
    assert [k for k in S.ALL_CLASSES if k not in union] == []
    # forward-only cases alone must not be what covers a training class, nor the functional cases a GEMM class
    train = set().union(*(reached[c.name] for c in S.TRAIN_CASES))
    assert [k for k in S.CORE_CLASSES if k not in train] == []


def test_every_row_class_of_the_table_is_needed():
    """Dropping the cases of one row class from the table loses a class: each row class below is the only source of one."""
    reached = {c: S.classes_of(c) for c in S.CASES}
    for rows in ({1}, {63}, {65, 129}, {513}, {8269, 16461}, {16461}, {130}, {32773}):
        rest = set().union(*(r for c, r in reached.items() if c.rows not in rows))
        lost = [k for k in S.ALL_CLASSES if k not in rest]
        print(f"without the cases at {sorted(rows)} rows: lost {lost}")
        assert lost, rows
    for shape in "ABD":                  # and so are these shapes (C repeats B's classes under the 512-wide row kernel)
        rest = set().union(*(r for c, r in reached.items() if c.shape != shape))
        assert [k for k in S.ALL_CLASSES if k not in rest], shape


def test_the_table_holds_the_planned_cases():
    got = {(c.shape, c.rows, c.kind, c.table, c.functional) for c in S.CASES}
    want = {(s, r, "train", "4x4", "") for s in "BC" for r in (1, 17, 63, 65, 129)}
    want |= {("D", r, "train", "4x4", "") for r in (1, 65, 513)} | {("A", r, "train", "4x4", "") for r in (513, 4096, 8269, 16461)}
    want |= {("B", 8269, "train", "4x4", ""), ("A", 130, "train", "2x8", ""), ("A", 130, "train", "8x2", "")}
    want |= {("A", 32773, "forward", "4x4", "")} | {(s, r, "forward", "4x4", "") for s in ("W512", "W256") for r in (1, 65)}
    want |= {(s, 129, "functional", "4x4", f) for s in "AB" for f in S.FUNCTIONALS}
    assert got == want and len(S.CASES) == len(want)
    assert len({c.name for c in S.CASES}) == len(S.CASES)
    assert len({c.seed for c in S.CASES if not c.functional}) == len(S.CASES) - len(S.FUNCTIONAL_CASES)
    assert len({c.seed for c in S.FUNCTIONAL_CASES}) == 2          # the five functionals of a shape share batch and weights
    for b, te in S.TABLES.values():
        assert len(b) * len(te) == 16
    assert S.SHAPES["A"] == C.HIDDEN and S.UNFILTERED.name == "train_C_65"


def test_the_restated_rules_cite_the_lines_they_restate():
    lines = open(os.path.join(ROOT, "mri-super-resolution_amd", "csrc", "pia.hip")).read().split("\n")
    common = open(os.path.join(ROOT, "mri-super-resolution_amd", "csrc", "common.h")).read().split("\n")
    at = lambda n: lines[n - 1]
    assert "constexpr int PIA_BK = 16;" in at(30)
    assert "chunk = (p.K + p.splits - 1) / p.splits;" in at(61) and "PIA_BK - 1) / PIA_BK * PIA_BK" in at(62)
    assert "if (kbeg > kend) kbeg = kend;" in at(65)
    assert "a four-float read is checked on its FIRST element only" in at(77)
    assert "n < p.N && k < kend" in at(102) and "if (n >= p.N) continue;" in at(162)
    assert "inline bool pia_big(" in at(198) and "M >= 128 && N >= 128" in at(199) and ">= 256" in at(199)
    assert "int pia_dw_splits(" in at(204) and "out_f >= 128 && in_f >= 128 && n >= 4096" in at(205)
    assert "(512 + tiles - 1) / tiles" in at(208) and "(n + 63) / 64" in at(209) and "s > 128" in at(211)
    assert "const long long per = (p.n + nwaves - 1) / nwaves;" in at(256)
    assert "pia_head_waves(long long n)" in at(500) and "w > 1024" in at(502) and "(w + 3) / 4 * 4" in at(503)
    assert "#define PIA_FWD_ROWS_PER_WAVE 16" in at(508) and "pia_head_waves_fwd(long long n)" in at(510)
    assert "if (H == 512)" in at(586)
    assert "s.H >= 128 && n >= 4096" in at(644) and "s.out[l] >= 128 && s.in[l] >= 128 && n >= 4096" in at(673)
    assert "pia_big(g.M, g.N, 1)" in at(609) and "pia_big(g.M, g.N, 3)" in at(622) and "pia_big(g.M, g.N, 1)" in at(658)
    assert "job.seg[k].nslabs = (int)w.waves;" in at(712)
    assert "constexpr int FIN_GROUP = 32;" in common[195] and "constexpr int FIN_TALL = 4 * FIN_GROUP;" in common[196]
    src = open(os.path.join(ROOT, "mri-super-resolution_amd", "pia_net.py")).read()
    assert f"chunk_rows: int = {S.FWD_CHUNK}" in src


def test_the_rules_at_the_boundary_row_counts():
    """The smallest row counts at which each big-tile class exists, the empty splits, and the boundary of the two-stage reduction."""
    first_big = lambda N, z: next(n for n in range(1, 40000) if S.pia_big(n, N, z))
    assert [first_big(N, 1) for N in (512, 256, 128)] == [8065, 16257, 32641]
    assert first_big(512, 3) == 2689 and first_big(256, 3) == 5377 and not any(S.pia_big(n, 64, 3) for n in (4096, 32768, 10 ** 6))
    assert S.pia_dw_splits(8269, 32, 16, 1) == (128, "cap")
    ranges = S.dw_split_ranges(8269, 128)
    assert ranges[103] == (8240, 8269) and all(r == (8269, 8269) for r in ranges[104:]) and len(ranges) == 128
    assert S.pia_dw_splits(4173, 32, 16, 1) == (66, "rows") and not any(b == e for b, e in S.dw_split_ranges(4173, 66))
    assert sum(b == e for b, e in S.dw_split_ranges(8192 + 17, 128)) > 0
    assert sum(e - b for b, e in ranges) == 8269
    assert S.pia_head_waves(512) == 128 and S.fin_stages(128) == (1, 1, 128)
    assert S.pia_head_waves(513) == 132 and S.fin_stages(132) == (2, 5, 4)
    assert S.pia_head_waves(1) == 4 and S.head_idle_waves(1, 4) == 3
    assert S.pia_head_waves(4096) == S.pia_head_waves(10 ** 6) == 1024 and S.fin_stages(1024) == (2, 32, 32)
    assert S.pia_head_waves_fwd(5) == 4 and S.pia_head_waves_fwd(32768) == 2048
    assert S.pia_dw_splits(1, 512, 512, 3) == (1, "rows") and S.pia_dw_splits(513, 512, 512, 3) == (3, "tiles")
    assert S.pia_dw_splits(8269, 256, 144, 1)[0] == 128 and S.dw_big(8269, 256, 144) and not S.dw_big(4095, 256, 144)
    assert S.launch_counts(S.BY_NAME["train_D_513"], fused=True) == {"pia_fwd": 9, "pia_dx": 8, "pia_dw": 9, "pia_head": 1}
    assert S.pool_rows(8269) == 8269 + 1024 and S.pool_rows(16461) == 16461 + 16461 // 8


def test_pia_net_fixture_is_unchanged():
    with open(os.path.join(ROOT, "tests", "golden", "pia_net.npz"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == PIA_NET_SHA256


def test_pids_slice_inputs_hold_the_edges():
    for n in S.PIDS_PIXELS:
        s = S.pids_slice_input(n)
        assert s.shape == (1, n, 4, 4) and s.dtype == np.float64 and np.isfinite(s).all()
        assert np.array_equal(s, S.pids_slice_input(n))
    s = S.pids_slice_input(257)[0]
    assert (s == 0).any() and (s < 0).any() and (s[:, 1, 2] == s[:, 1, 1]).any() and (s[:, 3, 1] == s[:, 2, 1]).any()
    assert (s[:, :, 0] < 0).any(axis=1).sum() >= 30            # NaN logarithms on the ADC line
    assert (S.pids_slice_input(1)[0] == 0).any()


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_restatement_reproduces_the_reference_float64_run_on_every_case(golden, case):
    """The generalised restatement (tables, depth, widths, functionals) against the reference class's own float64 run, 1e-12."""
    g = golden("pia_net_shapes.npz")
    assert [str(n) for n in g["case_names"]] == [c.name for c in S.CASES]
    b_values, te_values = case.tables
    torch.manual_seed(0)
    m = pia_net.PIA(hidden_dims=list(case.hidden), b_values=list(b_values), TE_values=list(te_values)).cpu()
    host = [p.detach().cpu().clone() for p in m.parameters()]
    pre = case.name
    assert S.params_sha([p.numpy() for p in host]) == str(g[f"{pre}/init_sha"])
    x, pids, flagged = S.case_inputs(case, host, pia_net.get_batch)
    assert C.sha(x.numpy()) == str(g[f"{pre}/x_sha"]), "the seeded input batch is not the generator's"
    if flagged is not None:
        assert flagged == int(g[f"{pre}/flagged"]) and not C.kink_rows(host, x, b_values=b_values, te_values=te_values).any()
    if case.kind == "forward":
        outs = C.forward64(host, x, b_values=b_values, te_values=te_values)
    else:
        f = S.functional64(case.functional, S.functional_weights(case.rows, case.seed)) if case.kind == "functional" else None
        loss, grads, outs = C.loss_and_grads64(host, x, pids, b_values=b_values, te_values=te_values, functional=f)
        want = float(g[f"{pre}/f64/loss"])
        assert abs(loss.item() - want) <= 1e-12 * abs(want), (loss.item(), want)
        flat, l1 = S.flat_grad_sample([gr.numpy() for gr in grads])
        dev = C.rel_dev(flat, g[f"{pre}/f64/grad_flat"])
        dev_l1 = float(np.max(np.abs(l1 - g[f"{pre}/f64/grad_l1"]) / np.maximum(g[f"{pre}/f64/grad_l1"], 1e-300)))
        print(f"{pre}: gradients {dev:.2e}, L1 norms {dev_l1:.2e}")
        assert dev <= 1e-12 and dev_l1 <= 1e-12, (dev, dev_l1)
        reached = ~np.isnan(g[f"{pre}/ref_err_grad"])
        assert np.array_equal(l1 > 0, reached)
    for k, t in zip(("signal", "D", "T2", "v"), outs):
        dev = C.rel_dev(C.sample(t.numpy()), g[f"{pre}/f64/{k}"])
        print(f"{pre}: f64/{k} {dev:.2e}")
        assert dev <= 1e-12, (k, dev)
