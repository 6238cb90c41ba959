#!/usr/bin/env python3
"""Generate tests/golden/pia_net.npz by running the REAL reference `PIA` class on the CPU.

    python tools/gen_golden_pia_net.py --reference <checkout>/implicit-neural-representations

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory of the reference checkout that holds PIA.py")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import PIA as R  # noqa: E402  (the reference module itself)

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
