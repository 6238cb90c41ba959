#!/usr/bin/env python3
"""Generate tests/golden/pia_net.npz by running the REAL reference `PIA` class on the CPU.

    python tools/gen_golden_pia_net.py --reference <checkout>/implicit-neural-representations
    python tools/gen_golden_pia_net.py --reference <checkout>/implicit-neural-representations --shapes    # pia_net_shapes.npz

Imports `PIA` from the reference checkout at generation time and writes data only: SHA-256 of the seeded initial weights,
a `get_batch` batch, forward / loss / gradients in float32 and from a float64 deep copy, the deviation of the former from
the latter (`ref_err/*`, the yardstick of the GPU tests), a 20-step Adam trajectory, the same quantities for one non-default shape (`small/*`), the supervised loss value, and
`detect_PIDS_slice` / `ADC_slice` on a seeded slice.  Sampling rule of oracle/gen_golden.py: tensors of <= 512 elements
whole, larger ones every 97th element plus the SHA-256 of the whole (`<name>/sha`); the input batch `batch/x` is stored
whole (32 KiB) because the float64 restatement is pinned on it to 1e-12.
"""
import argparse
import copy
import os
import sys
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pia_net_common as C  # noqa: E402


REF_ERR_TIER = 1e-5      # the project's gradient tier: a training case whose reference run misses it is no yardstick


def shapes(R):
    """tests/golden/pia_net_shapes.npz: the yardstick of tests/pia_shapes_common.CASES.

    Per case: SHA-256 of the seeded initial weights and of the input batch, the reference class's float32-versus-float64-deepcopy
    deviation per output and per gradient tensor (`ref_err_out`, `ref_err_grad`), and float64 values to which
    tests/test_pia_shapes_cpu.py pins the restatement at 1e-12: the outputs by the every-97th rule, the gradients as every 997th
    element of the tensors laid end to end plus each tensor's L1 norm (the every-97th rule on every gradient tensor of every
    case would come to 1.7 MB).  Inputs are not stored: they are `pia_net.get_batch` under the case's NumPy seed -- the
    project's own generator, which tests/test_pia_net_cpu.py holds to the reference's draws, so that generator and tests build
    the same bits -- filtered by `kink_rows`.  A training case whose reference run deviates more than REF_ERR_TIER on any
    tensor stops the generator: choose another seed or a deeper shape of the same class in the table, never a wider bound.
    Also `detect_PIDS_slice` on the seeded one-row slices of `pids_slice_input`."""
    import pia_shapes_common as S
    from mri_super_resolution_amd import pia_net

    out = {"case_names": np.array([c.name for c in S.CASES])}
    for case in S.CASES:
        b_values, te_values = case.tables
        torch.manual_seed(0)
        m = R.PIA(hidden_dims=list(case.hidden), b_values=list(b_values), TE_values=list(te_values))
        m64 = copy.deepcopy(m).double()
        host = [p.detach().clone() for p in m.parameters()]
        pre = case.name
        out[f"{pre}/init_sha"] = np.array(S.params_sha([p.numpy() for p in host]))
        x, pids, flagged = S.case_inputs(case, host, pia_net.get_batch)
        out[f"{pre}/x_sha"] = np.array(C.sha(x.numpy()))
        if flagged is not None:
            out[f"{pre}/flagged"] = np.array(flagged)
            assert flagged <= S.MAX_FLAGGED * S.pool_rows(case.rows), (pre, flagged)
        o32, o64 = m(x), m64(x.double())
        idx = (("signal", 0), ("D", 2), ("T2", 3), ("v", 4))
        out[f"{pre}/ref_err_out"] = np.array([C.rel_dev(o32[i].detach().numpy(), o64[i].detach().numpy()) for _, i in idx])
        for k, i in idx:
            out[f"{pre}/f64/{k}"] = C.sample(o64[i].detach().numpy().astype(np.float64))
        line = f"{pre}: flagged {flagged}, ref_err out {out[pre + '/ref_err_out'].max():.2e}"
        if case.kind != "forward":
            if case.kind == "train":
                l32 = m.loss_function(o32[0], x, pids)
                l64 = m64.loss_function(o64[0], x.double(), pids.double())
            else:
                w = S.functional_weights(case.rows, case.seed)
                named32 = {k: o32[i] for k, i in idx}
                named64 = {k: o64[i] for k, i in idx}
                l32 = sum((w[k] * named32[k]).sum() for k in S.functional_terms(case.functional))
                l64 = sum((w[k].double() * named64[k]).sum() for k in S.functional_terms(case.functional))
            l32.backward()
            l64.backward()
            out[f"{pre}/f64/loss"] = np.array(l64.item())
            g32 = [np.zeros(tuple(p.shape), np.float32) if p.grad is None else p.grad.numpy() for p in m.parameters()]
            g64 = [np.zeros(tuple(p.shape), np.float64) if p.grad is None else p.grad.numpy() for p in m64.parameters()]
            # a tensor the functional does not reach has a zero gradient on both sides: no deviation, and NaN marks it
            err = np.array([C.rel_dev(a, b) if np.abs(b).max() > 0 else np.nan for a, b in zip(g32, g64)])
            out[f"{pre}/ref_err_grad"] = err
            out[f"{pre}/f64/grad_flat"], out[f"{pre}/f64/grad_l1"] = S.flat_grad_sample(g64)
            line += f", ref_err grad {np.nanmin(err):.2e} .. {np.nanmax(err):.2e} (median {np.nanmedian(err):.2e})"
            if case.kind == "train":
                assert np.nanmax(err) <= REF_ERR_TIER and out[f"{pre}/ref_err_out"].max() <= REF_ERR_TIER, \
                    f"{pre}: the reference's own float32 run is {np.nanmax(err):.2e} off its float64 copy -- not a yardstick"
        print(line, flush=True)
    bv = np.array(C.B_VALUES, dtype=np.float64)
    for n in S.PIDS_PIXELS:
        res = R.detect_PIDS_slice(bv, S.pids_slice_input(n))
        for k, a in zip(("adc1", "adc2", "b_decay", "te_decay"), res):
            out[f"pids_slice/{n}/{k}"] = a.astype(np.uint8)
        print(f"pids_slice/{n}: sums", [float(a.sum()) for a in res])
    path = os.path.join(ROOT, "tests", "golden", "pia_net_shapes.npz")
    np.savez_compressed(path, **out)
    print("pia_net_shapes.npz", os.path.getsize(path), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory of the reference checkout that holds PIA.py")
    ap.add_argument("--shapes", action="store_true", help="write tests/golden/pia_net_shapes.npz (the shape-class table) instead")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import PIA as R  # noqa: E402  (the reference module itself)
    if args.shapes:
        sys.path.insert(0, ROOT)
        return shapes(R)

    out = {}

    def store(name, a):
        a = np.asarray(a)
        out[name] = C.sample(a)
        if a.size > 512:
            out[name + "/sha"] = np.array(C.sha(a))

    torch.manual_seed(0)
    m = R.PIA()
    names = [n for n, _ in m.named_parameters()]
    out["param_names"] = np.array(names)
    out["param_shapes"] = np.array([",".join(str(s) for s in p.shape) for p in m.parameters()])
    for n, p in m.named_parameters():
        out[f"init_sha/{n}"] = np.array(C.sha(p.detach().numpy()))

    np.random.seed(1)
    batch = R.get_batch(512, 0.02)
    for k, t in zip(("x", "D", "T2", "v", "clean"), batch):
        if k == "x":
            out["batch/x"] = t.numpy()
        else:
            store(f"batch/{k}", t.numpy())
    x = batch[0]
    pids = torch.from_numpy(C.pids_map())
    store("pids", pids.numpy())

    # float32 run
    signal, _, D, T2, v = m(x)
    loss = m.loss_function(signal, x, pids)
    m.zero_grad()
    loss.backward()
    f32 = {"signal": signal, "D": D, "T2": T2, "v": v}
    for k, t in f32.items():
        store(f"f32/{k}", t.detach().numpy())
        out[f"dtype/{k}"] = np.array(str(t.dtype))
    out["f32/loss"] = np.array(loss.item())
    g32 = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    for n, g in g32.items():
        store(f"f32/grad/{n}", g.numpy())
    with torch.no_grad():
        sup = m.loss_function([signal, D, T2, v], [x, batch[1], batch[2], batch[3]], None, tissue_available=True)
    out["supervised_loss"] = np.array(sup.item())
    out["supervised_dtype"] = np.array(str(sup.dtype))

    # float64 deep copy
    m64 = copy.deepcopy(m).double()
    m64.zero_grad()
    s64, _, D64, T264, v64 = m64(x.double())
    loss64 = m64.loss_function(s64, x.double(), pids.double())
    loss64.backward()
    for k, t in {"signal": s64, "D": D64, "T2": T264, "v": v64}.items():
        store(f"f64/{k}", t.detach().numpy().astype(np.float64))
        out[f"ref_err/{k}"] = np.array(C.rel_dev(f32[k].detach().numpy(), t.detach().numpy()))
    out["f64/loss"] = np.array(loss64.item())
    for n, p in m64.named_parameters():
        store(f"f64/grad/{n}", p.grad.numpy())
        out[f"ref_err/grad/{n}"] = np.array(C.rel_dev(g32[n].numpy(), p.grad.numpy()))

    # a non-default shape (four encoder layers, 256-wide heads) on the first rows of the same batch: the yardstick for the
    # kernels' other code paths (narrow head kernel, another layer count)
    torch.manual_seed(0)
    ms = R.PIA(hidden_dims=list(C.SMALL_HIDDEN))
    ms64 = copy.deepcopy(ms).double()
    xs, ps = x[:C.SMALL_ROWS], pids[:C.SMALL_ROWS]
    out["small/param_names"] = np.array([n for n, _ in ms.named_parameters()])
    for n, p in ms.named_parameters():
        out[f"small/init_sha/{n}"] = np.array(C.sha(p.detach().numpy()))
    o32, o64 = ms(xs), ms64(xs.double())
    l32s, l64s = ms.loss_function(o32[0], xs, ps), ms64.loss_function(o64[0], xs.double(), ps.double())
    l32s.backward()
    l64s.backward()
    out["small/f64/loss"] = np.array(l64s.item())
    for k, i in (("signal", 0), ("D", 2), ("T2", 3), ("v", 4)):
        store(f"small/f64/{k}", o64[i].detach().numpy().astype(np.float64))
        out[f"small/ref_err/{k}"] = np.array(C.rel_dev(o32[i].detach().numpy(), o64[i].detach().numpy()))
    for (n, p32), p64 in zip(ms.named_parameters(), ms64.parameters()):
        store(f"small/f64/grad/{n}", p64.grad.numpy())
        out[f"small/ref_err/grad/{n}"] = np.array(C.rel_dev(p32.grad.numpy(), p64.grad.numpy()))

    # 20 Adam steps, float32 and float64, fresh seeded batches
    def trajectory(model, dt):
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        losses = []
        for it in range(20):
            np.random.seed(100 + it)
            xb = R.get_batch(512, 0.02)[0].to(dt)
            sig = model(xb)[0]
            ls = model.loss_function(sig, xb, pids.to(dt))
            opt.zero_grad()
            ls.backward()
            opt.step()
            losses.append(ls.item())
        return np.array(losses)

    l32 = trajectory(m, torch.float32)
    l64 = trajectory(m64, torch.float64)
    out["traj/losses"] = l32
    out["traj/losses_f64"] = l64
    out["traj/ref_err"] = np.array(float(np.max(np.abs(l32 - l64) / np.abs(l64))))
    for n, p in m.named_parameters():
        store(f"traj/final/{n}", p.detach().numpy())
    out["traj/final_ref_err"] = np.array(max(C.rel_dev(p.detach().numpy(), q.detach().numpy())
                                             for p, q in zip(m.parameters(), m64.parameters())))

    # detect_PIDS_slice / ADC_slice
    S = C.pids_slice_input()
    bv = np.array(C.B_VALUES, dtype=np.float64)
    a1, a2, bd, td = R.detect_PIDS_slice(bv, S)
    out["pids_slice/S"] = S
    out["pids_slice/adc1"], out["pids_slice/adc2"], out["pids_slice/b_decay"], out["pids_slice/te_decay"] = a1, a2, bd, td
    out["pids_slice/adc_slice"] = R.ADC_slice(bv, S[:, :, :, 0])

    path = os.path.join(ROOT, "tests", "golden", "pia_net.npz")
    np.savez_compressed(path, **out)
    print("pia_net.npz", os.path.getsize(path), "bytes")
    for k in ("signal", "D", "T2", "v"):
        print(f"ref_err/{k} = {float(out['ref_err/' + k]):.3e}")
    ge = [float(out[f"ref_err/grad/{n}"]) for n in names]
    print(f"ref_err/grad: {min(ge):.3e} .. {max(ge):.3e}")
    print("small shape ref_err:", {k: f"{float(out[k]):.2e}" for k in out if k.startswith("small/ref_err/")})
    print(f"traj/ref_err = {float(out['traj/ref_err']):.3e}, final params {float(out['traj/final_ref_err']):.3e}")
    print("losses", l32[:3], "...", l32[-1], "supervised", float(out["supervised_loss"]), out["supervised_dtype"])
    print("pids sums", a1.sum(), a2.sum(), bd.sum(), td.sum())


if __name__ == "__main__":
    main()
