"""GPU box: the time of one Chambolle-Pock iteration of the TV / Huber solver under dense separable operators:
    python tools/tvop_time.py [--out profiles/tvop_time.txt]
28 images of (50, 50) -> (25, 25) -- the driver's ROI at x2 -- and one of (384, 384) -> (128, 128), Gaussian operators of FWHM 1.2 LR
pixels (baselines.psf_operator), fp64, seeded random data in [0, 1]; device events around whole solves (workspace allocated before)
after a warm-up solve: microseconds per iteration as (t(2,200 iterations) - t(200 iterations)) / 2,000 -- the step, init, the
back-projection, final and the host's set-up cancel --, median of 7 with the range.  Beside it ops.tvsr_solve (baselines.tv_superres:
one workgroup per image, a closed-form data step) on the same HR sizes with the block mean, the same way: it solves another problem
with other machinery, so it stands beside the new figures and is no like-for-like comparison.  And what the algorithm has to do per
iteration and image: four contractions, 2 h W (H + w) multiply-adds = 4 h W (H + w) flops; per HR pixel the dual kernel reads xbar and
reads and writes p0, p1 (5 doubles), launch 2 reads xbar (1), launch 5 reads p0, p1, x and writes x, xbar (5); per element of the plane
[h][W] one write and one read in either direction (4); per datum launch 3 reads y and reads and writes q (3) and launch 4 reads q (1);
the operators, neighbours' values and an operand's re-reads by other tiles are counted as cache hits.  Every configuration runs in a
child process of its own under its own time limit; after a child that fails nothing more is started."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
#          name: ((n, H, h, block factor of the comparison), time limit of the child in seconds)
CONFIGS = {"28x50x50_to_25x25": ((28, 50, 25, 2), 240), "1x384x384_to_128x128": ((1, 384, 128, 3), 240)}
LO, HI, REPEATS = 200, 2200, 7


def measure(name):
    import numpy as np
    import torch

    from mri_super_resolution_amd import baselines, ops

    (n, H, h, f), _ = CONFIGS[name]
    rng = np.random.default_rng(0)
    op = torch.from_numpy(baselines.psf_operator(H, h, 1.2)).cuda()
    pair = (op, op.clone())
    y = torch.from_numpy(rng.random((n, h, h))).cuda()
    y0 = torch.from_numpy(rng.random((n, H // f, H // f))).cuda()
    k = [[1.0 / (f * f)] * f] * f
    ws = torch.empty(ops.tvop_workspace_doubles(n, H, H, h, h), dtype=torch.float64, device="cuda")
    ws1 = torch.empty(ops.tvsr_workspace_doubles(n, H, H), dtype=torch.float64, device="cuda")

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

    new = per_iteration(lambda it: ops.tvop_solve(y, pair, 3e-3, 0.03, it, workspace=ws))
    block = per_iteration(lambda it: ops.tvsr_solve(y0, (f, f), k, 3e-3, 0.3, it, workspace=ws1))
    flops = n * 4 * h * H * (H + h)
    moved = 8 * n * (11 * H * H + 4 * h * H + 4 * h * h)
    return [f"{name} tv_superres_operator: {new[0]:.2f} us per iteration (range {new[1]:.2f} .. {new[2]:.2f} over {REPEATS}; {new[3]:.1f} ms "
            f"for {HI} iterations), five launches: {new[0] / 5:.2f} us per launch; the algorithm does {flops / 1e6:.2f} MFLOP and moves "
            f"{moved / 1e6:.2f} MB per iteration -> {flops / (new[0] * 1e-6) / 1e12:.3f} TFLOP/s, {moved / (new[0] * 1e-6) / 1e12:.3f} TB/s",
            f"{name} tv_superres (block mean x{f}) on the same HR size: {block[0]:.2f} us per iteration (range {block[1]:.2f} .. {block[2]:.2f}; "
            f"{block[3]:.1f} ms for {HI} iterations); the operator iteration takes {new[0] / block[0]:.2f} of that"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tvop_time.txt"))
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
