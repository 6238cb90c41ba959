"""GPU box: the time of one Chambolle-Pock iteration of the 3-D TV / Huber solver:
    python tools/tv3d_time.py [--out profiles/tv3d_time.txt]
Volumes of 28 x 100 x 100 and 56 x 256 x 256, fp64, seeded random data in [0, 1], 300 iterations after a warm-up solve, device events
around the solve (workspace allocated before): milliseconds per iteration as (t(300 iterations) - t(0 iterations)) / 300, median of 5.
Two yardsticks.  ONE, the bytes the iteration has to move: 13 doubles per HR voxel -- the dual kernel reads xbar and
reads and writes p0, p1, p2 (7), the primal kernel reads p0, p1, p2 and x and writes x and xbar (6); neighbours' values and the
primal kernel's second read of x are counted as cache hits, y and w (per LR voxel) are left out -- over the time: achieved bytes/s.
TWO, the 2-D solver on the same slices as a batch (baselines.tv_superres: one workgroup per slice, all iterations in one launch),
which solves the SAME problem as the 3-D solver with factors (1, 2, 2) and g0 = 0, bit for bit: the ratio of the two times.
The through-plane problem itself -- factors (2, 1, 1), weights (1, 1, 1) -- is timed beside them.
Every configuration runs in a child process of its own under its own time limit; after a child that fails nothing more is started."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = {"28x100x100": ((28, 100, 100), 120), "56x256x256": ((56, 256, 256), 240)}      # HR shape, time limit in seconds
N_ITER, REPEATS = 300, 5


def measure(name):
    import numpy as np
    import torch

    from mri_super_resolution_amd import ops

    (D, H, W), _ = CONFIGS[name]
    gen = torch.Generator(device="cuda").manual_seed(0)
    mean = lambda f: [1.0 / f] * f
    lam, alpha = 3e-3, 0.1

    def timed(fn):
        fn(N_ITER)                                                               # warm-up: code objects, allocator
        out = []
        for n_iter in (0, N_ITER):
            windows = []
            for _ in range(REPEATS):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                fn(n_iter)
                end.record()
                end.synchronize()
                windows.append(start.elapsed_time(end))
            out.append(float(np.median(windows)))
        return out

    voxels = D * H * W
    lines = []
    y_tp = torch.rand((1, D // 2, H, W), generator=gen, device="cuda", dtype=torch.float64)
    y_ip = torch.rand((1, D, H // 2, W // 2), generator=gen, device="cuda", dtype=torch.float64)
    cases = (("3-D through-plane, factors (2, 1, 1), g (1, 1, 1)", y_tp, (2, 1, 1), (1.0, 1.0, 1.0)),
             ("3-D in-plane, factors (1, 2, 2), g (0, 1, 1)", y_ip, (1, 2, 2), (0.0, 1.0, 1.0)))
    times = {}
    for label, y, f, g in cases:
        ws = torch.empty(ops.tvsr3d_workspace_doubles(1, D, H, W, f), dtype=torch.float64, device="cuda")
        k = tuple(mean(v) for v in f)
        t0, t1 = timed(lambda n: ops.tvsr_solve3d(y, f, k, lam, alpha, n, g, workspace=ws))
        per = (t1 - t0) / N_ITER
        times[label] = per
        lines.append(f"{name} {label}: {t1:.3f} ms for {N_ITER} iterations, {t0:.3f} ms for 0 -> {per * 1e3:.2f} us per iteration; "
                     f"13 doubles per voxel = {13 * 8 * voxels / 1e6:.1f} MB per iteration -> {13 * 8 * voxels / (per * 1e-3) / 1e12:.3f} TB/s; "
                     f"state {5 * 8 * voxels / 1e6:.1f} MB")
    y2 = y_ip[0].contiguous()
    ws2 = torch.empty(ops.tvsr_workspace_doubles(D, H, W), dtype=torch.float64, device="cuda")
    k2 = [mean(2), mean(2)]
    k2 = [[a * b for b in k2[1]] for a in k2[0]]
    t0, t1 = timed(lambda n: ops.tvsr_solve(y2, (2, 2), k2, lam, alpha, n, workspace=ws2))
    per2 = (t1 - t0) / N_ITER
    same = torch.equal(ops.tvsr_solve(y2, (2, 2), k2, lam, alpha, 20, workspace=ws2)[0],
                       ops.tvsr_solve3d(y_ip, (1, 2, 2), (mean(1), mean(2), mean(2)), lam, alpha, 20, (0.0, 1.0, 1.0))[0][0])
    label = "3-D in-plane, factors (1, 2, 2), g (0, 1, 1)"
    lines.append(f"{name} 2-D solver, {D} slices of {H} x {W} as a batch ({D} workgroups), factors (2, 2): {t1:.3f} ms for {N_ITER} "
                 f"iterations, {t0:.3f} ms for 0 -> {per2 * 1e3:.2f} us per iteration; the 3-D solver on the same problem (equal bits: "
                 f"{same}) takes {times[label] / per2:.3f} of that")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tv3d_time.txt"))
    ap.add_argument("--config", default=None, help="(internal) measure one configuration and print its lines")
    args = ap.parse_args()
    if args.config:
        print("\n".join(measure(args.config)), flush=True)
        return 0
    lines = []
    for name, (_, limit) in CONFIGS.items():
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{name}: not measured (no result within {limit} s); nothing further started")
            break
        if res.returncode != 0:
            lines.append(f"{name}: not measured (exit status {res.returncode}); nothing further started\n{res.stderr[-2000:]}")
            break
        lines += [l for l in res.stdout.splitlines() if l.startswith(name)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text, end="")
    return 0 if all("not measured" not in l for l in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
