"""GPU box: the time of one Chambolle-Pock iteration of the multi-stack TV / Huber solver:
    python tools/tvms_time.py [--out profiles/tvms_time.txt]
One volume of 56 x 256 x 256 from the orthogonal three-stack design at x2 (axial, coronal, sagittal, the mean profile) and one of
28 x 100 x 100 from the shifted two-stack design at x2 (two axial stacks, the second displaced by one thin slice), fp64, seeded random
data in [0, 1]; device events around whole solves (workspace allocated before) after a warm-up solve: microseconds per iteration as
(t(2,200 iterations) - t(200 iterations)) / 2,000 -- init, back-projection, final and the host's set-up cancel --, median of 7 with
the range.  Beside it baselines.tv_superres3d on ONE block stack (the axial one) of the same HR size, the same way: it solves a
smaller problem with a closed-form data step, so it stands beside the new figures and is no like-for-like comparison.  And the bytes
the multi-stack iteration has to move: per HR voxel the dual kernel reads xbar and reads and writes p0, p1, p2 (7 doubles), the primal
kernel reads p0, p1, p2, x and writes x, xbar (6); per datum the dual kernel reads y and reads and writes q (3), and the primal
kernel reads every q once (1); neighbours' values, re-read footprints and the table are counted as cache hits.  Every configuration
runs in a child process of its own under its own time limit; after a child that fails nothing more is started."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = {"56x256x256_orthogonal_x2": (((56, 256, 256), "orthogonal"), 300), "28x100x100_shifted_x2": (((28, 100, 100), "shifted"), 240)}
LO, HI, REPEATS = 200, 2200, 7


def measure(name):
    import numpy as np
    import torch

    from mri_super_resolution_amd import baselines, drivers, ops

    (shape, design), _ = CONFIGS[name]
    _, geos = drivers.multi_stack_designs(design, 2)
    rng = np.random.default_rng(0)
    table = [(g.factors, g.kernels, g.offsets, baselines.default_lr_shape(g, shape)) for g in geos]
    M = sum(int(np.prod(t[3])) for t in table)
    y = torch.from_numpy(rng.random((1, M))).cuda()
    y0 = torch.from_numpy(rng.random((1, shape[0] // 2, shape[1], shape[2]))).cuda()
    k = [[0.5, 0.5], [1.0], [1.0]]
    ws = torch.empty(ops.tvms_workspace_doubles(1, *shape, table), dtype=torch.float64, device="cuda")
    ws1 = torch.empty(ops.tvsr3d_workspace_doubles(1, *shape, (2, 1, 1)), dtype=torch.float64, device="cuda")

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

    multi = per_iteration(lambda it: ops.tvms_solve(y, table, shape, 0.01, 0.03, it, workspace=ws))
    single = per_iteration(lambda it: ops.tvsr_solve3d(y0, (2, 1, 1), k, 3e-3, 0.1, it, workspace=ws1))
    moved = 8 * (13 * int(np.prod(shape)) + 4 * M)
    return [f"{name} tv_superres_stacks, {len(table)} stacks, {M} data: {multi[0]:.2f} us per iteration (range {multi[1]:.2f} .. "
            f"{multi[2]:.2f} over {REPEATS}; {multi[3]:.1f} ms for {HI} iterations); the algorithm moves {moved / 1e6:.2f} MB per iteration "
            f"-> {moved / (multi[0] * 1e-6) / 1e12:.3f} TB/s",
            f"{name} tv_superres3d of one axial block stack on the same HR size: {single[0]:.2f} us per iteration (range {single[1]:.2f} .. "
            f"{single[2]:.2f}; {single[3]:.1f} ms for {HI} iterations); the multi-stack iteration takes {multi[0] / single[0]:.2f} of that"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tvms_time.txt"))
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
