"""GPU box: the time of one Chambolle-Pock iteration of the multi-frame TV / Huber solver:
    python tools/tvmf_time.py [--out profiles/tvmf_time.txt]
One image of 384 x 384 from 9 frames at x3 (the shapes of rams_master), and a batch of 28 images of 100 x 100 from 8 frames at x2 (a
volume's slices), fp64, seeded random data in [0, 1] and shifts in +- 1.5 HR pixels; device events around whole solves (workspace
allocated before) after a warm-up solve: microseconds per iteration as (t(2,200 iterations) - t(200 iterations)) / 2,000 -- init, final
and the host's set-up cancel --, median of 7 with the range.  Beside it baselines.tv_superres of ONE frame on the same HR sizes, the
same way (one workgroup per image, all iterations in one launch), and the bytes the multi-frame iteration has to move: per HR pixel
the dual kernel reads xbar and reads and writes p0, p1 (5 doubles), the primal kernel reads p0, p1, x and writes x, xbar (5); per
LR datum the dual kernel reads y and reads and writes q (3), and the primal kernel reads every q once (1); neighbours' values and the
table are counted as cache hits.  Every configuration runs in a child process of its own under its own time limit; after a child
that fails nothing more is started."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = {"1x384x384_9frames_x3": ((1, 384, 3, 9), 240), "28x100x100_8frames_x2": ((28, 100, 2, 8), 240)}    # (n, side, f, K), limit
LO, HI, REPEATS = 200, 2200, 7


def measure(name):
    import numpy as np
    import torch

    from mri_super_resolution_amd import ops

    (n, side, f, K), _ = CONFIGS[name]
    rng = np.random.default_rng(0)
    y = torch.from_numpy(rng.random((n, K, side // f, side // f))).cuda()
    s = rng.uniform(-1.5, 1.5, (n, K, 2))
    s[:, 0] = 0.0
    s = torch.from_numpy(s).cuda()
    y0 = y[:, 0].contiguous()
    k = [[1.0 / (f * f)] * f] * f
    ws = torch.empty(ops.tvmf_workspace_doubles(n, K, side, side, (f, f)), dtype=torch.float64, device="cuda")
    ws1 = torch.empty(ops.tvsr_workspace_doubles(n, side, side), dtype=torch.float64, device="cuda")

    def per_iteration(fn):
        fn(LO), fn(HI)                                                           # warm-up: code objects, allocator
        windows = {LO: [], HI: []}
        for _ in range(REPEATS):
            for n_iter in (LO, HI):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                start.record()
                fn(n_iter)
                end.record()
                end.synchronize()
                windows[n_iter].append(start.elapsed_time(end))
        per = (np.array(windows[HI]) - np.median(windows[LO])) / (HI - LO) * 1e3
        return float(np.median(per)), float(per.min()), float(per.max()), float(np.median(windows[HI]))

    multi = per_iteration(lambda it: ops.tvmf_solve(y, s, (f, f), k, 0.02, 0.1, it, workspace=ws))
    single = per_iteration(lambda it: ops.tvsr_solve(y0, (f, f), k, 3e-3, 0.3, it, workspace=ws1))
    moved = 8 * n * (10 * side * side + 4 * K * (side // f) ** 2)
    return [f"{name} tv_superres_multi: {multi[0]:.2f} us per iteration (range {multi[1]:.2f} .. {multi[2]:.2f} over {REPEATS}; "
            f"{multi[3]:.1f} ms for {HI} iterations); {moved / 1e6:.2f} MB per iteration -> {moved / (multi[0] * 1e-6) / 1e12:.3f} TB/s",
            f"{name} tv_superres of frame 0 on the same HR size: {single[0]:.2f} us per iteration (range {single[1]:.2f} .. "
            f"{single[2]:.2f}; {single[3]:.1f} ms for {HI} iterations); the multi-frame iteration takes {multi[0] / single[0]:.2f} of that"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tvmf_time.txt"))
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
