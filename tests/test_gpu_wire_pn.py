"""-m gpu: the WIRE network's gradient with respect to its input (csrc/wire.hip: inr_wire_forward_stash / inr_wire_input_grad)
and the PerturbNet phase of wiretest.ipynb cell 10 built on it, against the fixture made from the reference's own layer, PN and
input_mapping (tests/golden/wire_pn.npz) and, on other shapes, against the float64 restatement that fixture pins
(tests/wire_pn_common.py).

Bounds are the project's tiers as relative L2 per tensor: 1e-5 for y, dx, the PerturbNet step's loss and its gradients, 1e-4 for
the short schedule's losses and the PerturbNet's first-moment state.  The reference's own float32 against its float64 on the
fixture (``noise/*``, tools/make_wire_pn_golden.py) is <= 3.2e-7 for the first group and <= 5.4e-7 for the second, so every
tier stands at least 20 x above arithmetic noise (test_wire_pn_cpu.py asserts that of the fixture).  Every test prints its
measured figures before it asserts."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import wire_common as C
import wire_pn_common as PNC
import mri_super_resolution_amd as inr
from mri_super_resolution_amd import _lib, drivers, matio, ops
from mri_super_resolution_amd.scripts import wiretest as wt_script
from mri_super_resolution_amd.wire import ComplexGaborLayer2D, Wire, WireFitter

pytestmark = pytest.mark.gpu

T1 = 1e-5        # y, dx, one PerturbNet step
T3 = 1e-4        # the schedule


def _host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _fixture_model(g):
    model = Wire(16, 32, 1, 1, first_omega_0=C.OMEGA, hidden_omega_0=C.OMEGA, scale=C.SCALE)
    sd = {}
    for k, v in model.state_dict().items():
        w = torch.from_numpy(g["w/" + k])
        sd[k] = torch.view_as_complex(w.contiguous()) if v.is_complex() else w
    model.load_state_dict(sd)
    return model.cuda()


def _fixture_pn(g):
    pn = inr.PN(16, 32, 3)
    pn.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("pn/")})
    return pn.cuda()


def _c_input_grad(model, x, gy):
    """(y [n], dx [n, in]) through the two C entry points themselves."""
    lib = _lib.lib()
    desc = model.desc()
    flat = model._flat(desc)
    n = x.shape[0]
    need = lib.inr_wire_workspace_bytes(ctypes.byref(desc), n, 2)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    y = torch.empty(n, dtype=torch.float32, device=x.device)
    dx = torch.full_like(x, float("nan"))
    _lib.check(lib.inr_wire_forward_stash(ctypes.byref(desc), flat.data_ptr(), x.data_ptr(), n, y.data_ptr(), ws.data_ptr(), need,
                                          ops._stream()), "inr_wire_forward_stash")
    _lib.check(lib.inr_wire_input_grad(ctypes.byref(desc), flat.data_ptr(), gy.data_ptr(), n, dx.data_ptr(), ws.data_ptr(), need,
                                       ops._stream()), "inr_wire_input_grad")
    return y, dx


def _check_input_grad(model, x, gy, L, want_y, want_dx, tag):
    y, dx = _c_input_grad(model, x, gy)
    assert dx.shape == x.shape and bool(torch.isfinite(dx).all())          # unpadded, every entry written
    e_y, e_dx = C.rel_l2(_host(y), want_y), C.rel_l2(_host(dx), want_dx)
    print(f"[wire pn {tag}] y rel-L2 {e_y:.3e}  dx rel-L2 {e_dx:.3e}  max|dx| {np.abs(want_dx).max():.3e}")
    assert e_y <= T1 and e_dx <= T1
    return y, dx


def test_input_gradient_matches_the_reference_fixture():
    g = PNC.golden()
    _check_input_grad(_fixture_model(g), torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["gy"]).cuda(), 1, g["y"], g["dx"],
                      "fixture")


CASES = [  # (n, in_features, hidden, hidden layers, raw coordinates)
    (357, 3, 64, 2, True),           # raw coordinates: fewer columns than half a tile
    (130, 96, 128, 0, False),        # no complex layer; a ragged second column tile
    (5, 40, 32, 1, False),           # fewer rows than a tile; in_features not a multiple of the K block
    (2049, 16, 32, 1, False),        # one row past the parameter-gradient slab size, which plays no part here
]


@pytest.mark.parametrize("n,in_f,hidden,layers,raw", CASES)
def test_input_gradient_matches_the_restatement(n, in_f, hidden, layers, raw):
    model, x, _, _ = C.make_case(Wire, n, in_f, hidden, layers, seed=n + hidden, raw=raw)
    gy = torch.randn(n, generator=torch.Generator().manual_seed(n))
    want_y, want_dx = PNC.input_grad64(C.leaves64(model), x.numpy(), gy.numpy(), layers)
    _check_input_grad(model.cuda(), x.cuda(), gy.cuda(), layers, want_y, want_dx, f"n={n} in={in_f} H={hidden} L={layers}")


def test_bits_are_reproducible_and_rows_are_independent():
    g = PNC.golden()
    model = _fixture_model(g)
    x, gy = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["gy"]).cuda()
    y, dx = _c_input_grad(model, x, gy)
    y2, dx2 = _c_input_grad(model, x, gy)
    assert torch.equal(y, y2) and torch.equal(dx, dx2)                                      # two runs
    ya, dxa = _c_input_grad(model, x[:100].contiguous(), gy[:100].contiguous())
    assert torch.equal(ya, y[:100]) and torch.equal(dxa, dx[:100])                          # neither n nor the tile a row sits in
    yb, dxb = _c_input_grad(model, x[37:170].contiguous(), gy[37:170].contiguous())
    assert torch.equal(yb, y[37:170]) and torch.equal(dxb, dx[37:170])                      # nor the row's position
    plain = model(x)
    assert not plain.requires_grad and plain.shape == (333, 1)
    with_grad = model(x.clone().requires_grad_(True))
    assert with_grad.requires_grad and torch.equal(with_grad.detach(), plain) and torch.equal(plain[:, 0], y)
    with torch.no_grad():
        assert not model(x.clone().requires_grad_(True)).requires_grad


def test_autograd_equals_the_c_call_and_runs_one_backward():
    g = PNC.golden()
    model = _fixture_model(g)
    x, gy = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["gy"]).cuda()
    _, dx = _c_input_grad(model, x, gy)
    xg = x.clone().requires_grad_(True)
    out = model(xg)
    (got,) = torch.autograd.grad((out[:, 0] * gy).sum(), xg, retain_graph=True)
    assert torch.equal(got, dx)
    assert all(p.grad is None for p in model.parameters())                                  # the input's gradient only
    with pytest.raises(RuntimeError, match="ONE backward per forward"):
        torch.autograd.grad((out[:, 0] * gy).sum(), xg)
    xg3 = x.reshape(9, 37, 16).clone().requires_grad_(True)                                 # leading axes are kept
    out3 = model(xg3)
    assert out3.shape == (9, 37, 1)
    (out3[..., 0] * gy.reshape(9, 37)).sum().backward()
    assert torch.equal(xg3.grad.reshape(333, 16), dx)
    fitter = WireFitter(model)                                                               # the fitter's live flat buffer serves too
    xg = x.clone().requires_grad_(True)
    (got,) = torch.autograd.grad((model(xg)[:, 0] * gy).sum(), xg)
    assert fitter.owns(model) and torch.equal(got, dx)
    with pytest.raises(RuntimeError, match="WireFitter"):                                   # the single layer keeps refusing
        model.net[0](x.clone().requires_grad_(True))
    assert isinstance(model.net[0], ComplexGaborLayer2D)


def test_one_perturbnet_step_matches_the_reference_fixture():
    g = PNC.golden()
    model, pn = _fixture_model(g), _fixture_pn(g)
    x, B = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["B"]).cuda()
    target = torch.from_numpy(g["acq"][1]).reshape(-1, 1).cuda()
    out = model(inr.input_mapping(pn(x, 1, float(g["eps"])), B))
    loss = ((out - target) ** 2).mean()
    loss.backward()
    e_loss = abs(float(loss.detach()) - float(g["step_loss"])) / float(g["step_loss"])
    errs = {k: C.rel_l2(_host(p.grad), g["step_g/" + k]) for k, p in pn.named_parameters()}
    print(f"[wire pn step] loss rel {e_loss:.3e}  " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert set(errs) == set(PNC.PN_KEYS)
    assert e_loss <= T1 and max(errs.values()) <= T1, errs
    assert all(p.grad is None for p in model.parameters())


def test_short_schedule_matches_the_reference_fixture():
    """Cell 10 with number_of_epochs = pertubation_epochs = 4 and K = 2: PerturbNet losses and its Adam first moments (the
    parameters themselves barely move at lr 1e-6 and would pass whatever the gradients were)."""
    g = PNC.golden()
    model, pn = _fixture_model(g), _fixture_pn(g)
    B = torch.from_numpy(g["B"]).cuda()
    mean = inr.ImageFitting_set([g["mean"]])
    assert np.array_equal(mean.coords[0].cpu().numpy(), g["coords"])
    f = drivers.fit_wire_with_perturbnet
    inr_losses = f(model, B, mean, [g["acq"][k] for k in range(2)], 4, 4, lr=5e-5, perturb_lr=1e-6, eps=float(g["eps"]),
                   perturb_net=pn)
    assert f.last_pn is pn and f.last_pn_steps == 4 and len(inr_losses) == 2
    e_pn, e_inr = C.rel_l2(f.last_pn_losses, g["sched_pn_losses"]), C.rel_l2(inr_losses, g["sched_inr_losses"])
    errs = {k: C.rel_l2(_host(m), g["sched_m/" + k]) for (k, _), (m, _) in zip(pn.named_parameters(), f.last_pn_state)}
    print(f"[wire pn schedule] PerturbNet losses rel-L2 {e_pn:.3e}  INR losses rel-L2 {e_inr:.3e}  m: "
          + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert e_pn <= T3 and e_inr <= T3 and max(errs.values()) <= T3, errs
    for k, p in pn.named_parameters():
        assert not np.array_equal(_host(p), g["pn/" + k].astype(np.float64)), k             # every tensor was updated


def _master(tmp_path):
    """A synthetic master.mat in the reference's layout: 20 x 20 x 4 voxels, a 4 x 4 [b][TE] cell, 2 x 2 x 1 = 4 products."""
    rng = np.random.default_rng(2)
    X = Y = 20
    Z, nacq = 4, (1, 2, 2, 1)
    gx, gy = np.meshgrid(np.linspace(0, 1, X), np.linspace(0, 1, Y), indexing="ij")
    base = 100 * (1.2 + np.sin(3 * gx) * np.cos(2 * gy))
    cell = np.empty((4, 4), dtype=object)
    for b in range(4):
        for te in range(4):
            shape = (X, Y, Z) if b == 0 else (X, Y, Z, nacq[b])
            sig = base[..., None] * np.exp(-0.4 * b) * (1 - 0.1 * te) * np.ones(Z)
            cell[b, te] = (sig if b == 0 else sig[..., None] * np.ones(nacq[b])) * (1 + 0.02 * rng.standard_normal(shape))
    path = str(tmp_path / "pat065_master.mat")
    matio.savemat(path, {"hybrid_raw": cell, "b": np.array([0.0, 150.0, 1000.0, 1500.0])})
    return path, Z


FLAGS = ["--number_of_epochs", "6", "--pertubation_epochs", "4", "--mapping_size", "8", "--hidden_dim", "64", "--num_layers", "1",
         "--roi_start", "2", "--roi_end", "18", "--seed", "0"]


def test_wiretest_runs_the_perturbnet_phase_on_a_master_mat(tmp_path):
    path, Z = _master(tmp_path)
    out = str(tmp_path / "res")
    res = wt_script.main(["--data", path, "--pt_id", "65", "--output_address", out, *FLAGS])[0]
    d = os.path.join(out, "pat65")
    assert sorted(os.listdir(d)) == ["metrics.json", "recon.mat", "recon.npy", "ssim_scores.csv"]
    saved = json.load(open(os.path.join(d, "metrics.json")))
    assert saved == json.loads(json.dumps(res)) and saved["pn_steps"] == 8 and saved["steps"] == 6
    assert np.isfinite(saved["pn_final_loss"]) and np.isfinite(saved["final_loss"]) and saved["n_coords"] == 8 * 8 * Z * 4
    rec = matio.loadmat(os.path.join(d, "recon.mat"))
    assert rec["recon"].shape == (32, 32, Z, 4) and rec["SR_recon"].shape == (16, 16, Z, 4) and rec["maxes"].shape == (4, 4)
    assert np.all(np.isfinite(rec["recon"])) and rec["recon"].min() >= 0.0
    assert np.array_equal(np.load(os.path.join(d, "recon.npy")), rec["recon"])
    f = drivers.fit_wire_with_perturbnet
    assert f.last_pn_steps == 8 and len(f.last_pn_losses) == 8 and len(f.last_pn_state) == 4
    for (k, p), (m, v) in zip(f.last_pn.named_parameters(), f.last_pn_state):
        assert float(m.abs().max()) > 0 and bool(torch.isfinite(m).all()), k                # the gradient reached the PerturbNet


def test_wiretest_fits_a_plain_volume_without_the_phase(tmp_path):
    rng = np.random.default_rng(3)
    path = str(tmp_path / "pat07_vol.mat")
    matio.savemat(path, {"vol": rng.random((20, 20, 4, 4)) + 0.5, "b": np.array([0.0, 150.0, 1000.0, 1500.0])})
    out = str(tmp_path / "res")
    res = wt_script.main(["--data", path, "--output_address", out, *FLAGS])[0]
    d = os.path.join(out, "pat07")
    assert sorted(os.listdir(d)) == ["metrics.json", "recon.mat", "recon.npy", "ssim_scores.csv"]
    assert res["pn_steps"] == 0 and res["pn_final_loss"] is None and res["steps"] == 6 and np.isfinite(res["final_loss"])
    assert "maxes" not in matio.loadmat(os.path.join(d, "recon.mat"))
