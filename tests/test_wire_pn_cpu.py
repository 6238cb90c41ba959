"""CPU checks of the WIRE network's input gradient and PerturbNet phase (wiretest.ipynb cell 10): the float64 restatement
(tests/wire_pn_common.py) against the fixture made from the reference's own layer, PN and input_mapping
(tools/make_wire_pn_golden.py), every refusal of the two new entry points that has to come before any device work (fake
device pointers that are never dereferenced), the epoch schedule of ``drivers.fit_wire_with_perturbnet`` with the fitter and
the networks mocked, and ``scripts/wiretest.py``'s defaults and refusals.

Restatement against fixture, measured: every tensor within 1.1e-15 of its maximum (bound 1e-12, float64 round-off, as for the
sibling restatement of tests/wire_common.py)."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import wire_common as C
import wire_pn_common as PNC
from mri_super_resolution_amd import _lib, drivers, matio
from mri_super_resolution_amd.scripts import superresDWI as dwi_script
from mri_super_resolution_amd.scripts import wiretest as wt_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = 1e-12        # of each tensor's maximum
L = 1                # the fixture's hidden layers


def _fake(k):
    return ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)


def _desc(in_f=16, hidden=32, layers=1, out=1):
    return _lib.WireDesc(in_f, hidden, layers, out, 1.2, 1.2, 1.2, 1.2)


def _gap(got, want):
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


def test_fixture_holds_data_only_and_is_small():
    g = PNC.golden()
    assert os.path.getsize(PNC.GOLDEN) < 200_000
    assert g["x"].shape == (333, 16) and g["x"].dtype == np.float32 and g["coords"].shape == (333, 3) and g["B"].shape == (8, 3)
    assert g["acq"].shape == (2, 3, 3, 37) and g["mean"].shape == (3, 3, 37) and g["dx"].shape == (333, 16) and g["gy"].shape == (333,)
    assert g["sched_pn_losses"].shape == (4,) and g["sched_inr_losses"].shape == (2,) and float(g["eps"]) == 1 / 128.
    assert g["pn/perturb_linear.weight"].shape == (32, 17) and g["pn/perturb_linear2.weight"].shape == (3, 32)
    for k in g.files:
        assert g[k].dtype.kind in "fU", k                                            # numbers and the list of names: no objects
    # the reference's own float32 against its float64: the tiers of test_gpu_wire_pn.py stand at least 20 x above it
    for k in ("y", "dx", "step_loss", "step_g"):
        assert 20 * float(g["noise/" + k]) <= 1e-5, k
    for k in ("sched_pn_losses", "sched_inr_losses", "sched_m"):
        assert 20 * float(g["noise/" + k]) <= 1e-4, k


def test_restatement_agrees_with_the_reference():
    g = PNC.golden()
    P, Q = C.golden_leaves(g), PNC.pn_leaves(g)
    x, B, eps = g["x"].astype(np.float64), g["B"], float(g["eps"])
    gaps = {}
    y, dx = PNC.input_grad64(P, x, g["gy"], L)
    gaps["y"], gaps["dx"] = _gap(y, g["y"]), _gap(dx, g["dx"])
    assert np.allclose(PNC.fourier64(g["coords"].astype(np.float64), B), x, atol=1e-6)          # x is input_mapping(coords, B)
    acq = g["acq"].astype(np.float64).reshape(2, -1)
    loss, G = PNC.pn_step64(P, Q, x, B, 1, eps, acq[1], L)
    gaps["step_loss"] = abs(loss - float(g["step_loss"])) / float(g["step_loss"])
    for k in PNC.PN_KEYS:
        assert G[k].shape == g["step_g/" + k].shape, k
        gaps["step_g/" + k] = _gap(G[k], g["step_g/" + k])
    inr_losses, pn_losses, m = PNC.schedule64(P, Q, x, B, eps, g["mean"].astype(np.float64).reshape(-1), acq, L, 4, 4)
    gaps["sched_pn_losses"], gaps["sched_inr_losses"] = _gap(pn_losses, g["sched_pn_losses"]), _gap(inr_losses, g["sched_inr_losses"])
    for k in PNC.PN_KEYS:
        gaps["sched_m/" + k] = _gap(m[k], g["sched_m/" + k])
    for k, v in gaps.items():
        print(f"[wire pn restatement] {k:40s} {v:.3e}")
    assert max(gaps.values()) <= TIGHT, gaps
    assert np.abs(g["dx"]).max() > 1e-3 and np.abs(g["sched_m/perturb_linear.weight"]).max() > 0      # there is a gradient to pin
    assert np.abs(Q["perturb_linear.weight"] - g["pn/perturb_linear.weight"]).max() > 1e-7           # the schedule moved the PerturbNet


def test_input_grad64_is_the_derivative_of_forward64():
    """The restatement against central differences of its own forward (raw coordinates, two hidden layers)."""
    rng = np.random.default_rng(0)
    from mri_super_resolution_amd.wire import Wire
    model, x, _, _ = C.make_case(Wire, 7, 3, 32, 2, seed=3, raw=True)
    P, x = C.leaves64(model), x.numpy().astype(np.float64)
    gy = rng.standard_normal(7)
    _, dx = PNC.input_grad64(P, x, gy, 2)
    h = 1e-6
    for r, c in ((0, 0), (3, 2), (6, 1)):
        e = np.zeros_like(x)
        e[r, c] = h
        fd = (gy @ C.forward64(P, x + e, 2) - gy @ C.forward64(P, x - e, 2)) / (2 * h)
        assert abs(fd - dx[r, c]) <= 1e-7 * max(1.0, abs(dx[r, c])), (r, c, fd, dx[r, c])


def test_new_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inrhip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("inr_wire_forward_stash", "inr_wire_input_grad"):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name) and hasattr(_lib.lib(), name), name


def test_workspace_modes():
    lib, d = _lib.lib(), ctypes.byref(_desc())
    inf, train, grad = (lib.inr_wire_workspace_bytes(d, 100, mode) for mode in (0, 1, 2))
    assert 0 < inf < grad and grad != train                  # the stash of every layer, no parameter-gradient slabs
    assert lib.inr_wire_workspace_bytes(d, 0, 2) == 0 and lib.inr_wire_workspace_bytes(d, 65535 * 2048 + 1, 2) == 0
    assert lib.inr_wire_workspace_bytes(d, 65535 * 2048, 2) > 0
    raw = ctypes.byref(_desc(in_f=3))                         # the transposed layer-0 image is [in][2H]: it grows with in_features
    assert lib.inr_wire_workspace_bytes(raw, 100, 2) < grad


def test_argument_errors_are_refused_before_device_work():
    lib, desc = _lib.lib(), _desc()
    d = ctypes.byref(desc)
    n = 100
    need = lib.inr_wire_workspace_bytes(d, n, 2)
    E, W, A = _lib.INR_E_INVALID, _lib.INR_E_WORKSPACE, _lib.INR_E_ALIGN
    odd = ctypes.c_void_p(0x7000_0000_0004)
    limit = 65535 * 2048
    for fn, who in ((lib.inr_wire_forward_stash, b"inr_wire_forward_stash"), (lib.inr_wire_input_grad, b"inr_wire_input_grad")):
        call = lambda p=_fake(1), a=_fake(2), rows=n, b=_fake(3), w=_fake(4), wb=need, dd=d: fn(dd, p, a, rows, b, w, wb, None)      # noqa: E731
        assert call(dd=None) == E and call(p=None) == E and call(a=None) == E and call(b=None) == E
        assert b"null" in lib.inr_last_error() and who in lib.inr_last_error()
        assert call(rows=0) == E and call(rows=-1) == E and call(rows=limit + 1, wb=1 << 62) == E
        assert b"bad row count" in lib.inr_last_error()
        assert call(w=None) == W and call(wb=need - 1) == W and call(wb=lib.inr_wire_workspace_bytes(d, n, 0)) == W
        assert b"workspace too small" in lib.inr_last_error()
        assert call(p=odd) == A and call(w=odd) == A
        for bad in (_desc(out=2), _desc(hidden=48), _desc(hidden=512), _desc(in_f=1025), _desc(in_f=0), _desc(layers=9)):
            assert call(dd=ctypes.byref(bad)) == E


class _FakePN(torch.nn.Module):
    def __init__(self, log, dimension):
        super().__init__()
        self.log, self.dimension = log, dimension
        self.a = torch.nn.Parameter(torch.ones(3))
        self.b = torch.nn.Parameter(torch.ones(1))

    def forward(self, coords, sample=0, eps=0):
        self.log.append(("pn", sample, eps))
        return (self.a.sum() + self.b) * torch.ones(coords.shape[0], self.dimension)


class _FakeFitter:
    def __init__(self, log):
        self.log = log

    def step(self, model_input, target, n_steps=1, weight=None):
        self.log.append(("inr", int(n_steps)))
        return torch.full((int(n_steps),), float(len(self.log)))


SCHEDULES = {   # cell 10 by hand: the head in ONE call, odd tail epochs one INR step, even tail epochs a PerturbNet step per acquisition
    (6, 4): [("inr", 2), "pn", ("inr", 1), "pn", ("inr", 1)],
    (5, 3): [("inr", 2), "pn", ("inr", 1), "pn"],
    (4, 0): [("inr", 4)],
    (3, 5): ["pn", ("inr", 1), "pn"],
}


@pytest.mark.parametrize("epochs,pert", sorted(SCHEDULES))
def test_fit_wire_with_perturbnet_follows_cell_10(monkeypatch, epochs, pert):
    K, n, log, adam = 3, 5, [], []
    want = []
    for item in SCHEDULES[(epochs, pert)]:
        want += [("pn", s, 1 / 128.) for s in range(K)] if item == "pn" else [item]
    # (the hand-written table against the loop's condition stated on its own)
    per_epoch = []
    for item in SCHEDULES[(epochs, pert)]:
        per_epoch += ["pn"] if item == "pn" else ["inr"] * item[1]
    assert per_epoch == PNC.epoch_branches(epochs, pert)

    class FakeSet:
        def __init__(self, images):
            self.shape = tuple(images[0].shape)
            self.pixels = torch.stack([torch.as_tensor(i, dtype=torch.float32).reshape(-1, 1) for i in images])

        def __len__(self):
            return len(self.pixels)

    monkeypatch.setattr(drivers, "ImageFitting_set", FakeSet)
    monkeypatch.setattr(drivers, "input_mapping", lambda x, B: x)
    monkeypatch.setattr(drivers.ops, "adam_step", lambda p, g, m, v, step, lr: adam.append((tuple(p.shape), int(step), lr)))
    mean = SimpleNamespace(coords=[torch.zeros(n, 2)], pixels=[torch.zeros(n, 1)])
    pn = _FakePN(log, 2)
    inr_calls = []

    def INR(x):
        inr_calls.append(x.requires_grad)
        return x.sum(-1, keepdim=True)

    losses = drivers.fit_wire_with_perturbnet(INR, None, mean, [np.full((n, 1), float(k)) for k in range(K)], epochs, pert,
                                              perturb_net=pn, fitter=_FakeFitter(log))
    assert log == want
    n_pn = sum(1 for e in want if e[0] == "pn")
    assert len(losses) == sum(e[1] for e in want if e[0] == "inr") == epochs - n_pn // K
    f = drivers.fit_wire_with_perturbnet
    assert f.last_pn is pn and f.last_pn_steps == n_pn == len(f.last_pn_losses) and len(f.last_pn_state) == 2
    assert inr_calls == [True] * n_pn                         # the network saw an input that carries the PerturbNet's graph
    assert adam == [(shape, s, 1e-6) for s in range(1, n_pn + 1) for shape in ((3,), (1,))]      # Adam(lr=1e-6), PerturbNet only
    assert all(m.shape == p.shape and v.shape == p.shape for p, (m, v) in zip(pn.parameters(), f.last_pn_state))


def test_wiretest_parser_has_the_notebook_defaults():
    a = wt_script.build_parser().parse_args(["--data", "x.mat"])
    assert (a.mapping_size, a.scale, a.hidden_dim, a.num_layers, a.PN_dim, a.roi_start, a.roi_end) == (256, 0.5, 256, 3, 128, 45, 75)
    assert (a.number_of_epochs, a.pertubation_epochs, a.learning_rate, a.wire_omega, a.wire_scale) == (2500, 3, 5e-5, 1.2, 1.2)
    assert a.model == "wire" and wt_script.check_model(a) is None
    b = dwi_script.build_parser().parse_args(["--data", "x.mat"])          # superresDWI keeps its own
    assert (b.mapping_size, b.hidden_dim, b.roi_start, b.roi_end, b.pertubation_epochs, b.learning_rate, b.model) == \
        (128, 512, 40, 90, 10, 1e-4, "siren")
    assert set(vars(a)) == set(vars(b))                                    # the same flags


def _hybrid_raw():
    raw = np.empty((4, 2), dtype=object)
    for b in range(4):
        for te in range(2):
            raw[b, te] = np.ones((20, 20, 3, 1 if b == 0 else 2))
    return {"hybrid_raw": raw, "b": np.array([0.0, 150.0, 1000.0, 1500.0])}


def test_wiretest_refuses_what_wire_does_not_serve_before_any_device_call(tmp_path, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(drivers, "acquisition_products", no_device)
    monkeypatch.setattr(dwi_script.inr, "ImageFitting_set", no_device)
    vol = {"vol": np.random.default_rng(0).random((20, 20, 6, 4)) + 0.5, "b": np.array([0.0, 150.0, 1000.0, 1500.0])}
    plain = str(tmp_path / "pat03_vol.mat")
    matio.savemat(plain, vol)
    base = ["--output_address", str(tmp_path / "res"), "--number_of_epochs", "4", "--hidden_dim", "64", "--num_layers", "1",
            "--mapping_size", "8", "--roi_start", "2", "--roi_end", "18"]
    with pytest.raises(ValueError, match="no derivative maps of a WIRE network"):
        wt_script.main(["--data", plain, "--derivative_maps", *base])
    with pytest.raises(ValueError, match="hidden_dim // 2"):
        wt_script.main(["--data", plain, *base, "--hidden_dim", "96"])
    with pytest.raises(ValueError, match="hidden_dim // 2"):
        wt_script.main(["--data", plain, *base, "--mapping_size", "513"])
    with pytest.raises(ValueError, match="num_layers"):
        wt_script.main(["--data", plain, *base, "--num_layers", "9"])
    with pytest.raises(ValueError, match="WIRE network only"):
        wt_script.main(["--data", plain, *base, "--model", "siren"])
    with pytest.raises(ValueError, match="pertubation_epochs"):
        wt_script.main(["--data", plain, *base, "--pertubation_epochs", "-1"])
    monkeypatch.setattr(matio, "loadmat", lambda path: _hybrid_raw())
    with pytest.raises(AssertionError, match="device work"):                      # single acquisitions ARE served here
        wt_script.main(["--data", "pat09_master.mat", *base])
    with pytest.raises(ValueError, match="PerturbNet phase.*wiretest"):           # superresDWI keeps refusing, and says where to go
        dwi_script.main(["--data", "pat09_master.mat", *base, "--model", "wire"])
