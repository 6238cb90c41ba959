"""GPU box: the time of one Chambolle-Pock iteration of the channel-coupled TV / Huber solver, and the study case in fp32:
    python tools/tvj_time.py [--out profiles/tvj_time.txt]
28 groups of 4 channels at (50, 50) <- (25, 25) -- the driver's ROI at x2, four b-values -- and one group of 4 channels at (384, 384) <-
(192, 192), the block mean, fp64, seeded random data in [0, 1]; device events around whole solves (workspace allocated before) after
a warm-up solve: microseconds per iteration as (t(2,000 iterations) - t(1,000 iterations)) / 1,000 -- the start, the objective and the
host's set-up cancel --, median of 7 with the range.  Beside each figure ops.tvsr_solve (baselines.tv_superres) on the same 112 (or 4)
images, measured the same way in the same run with the two solvers alternating: the per-image kernel the repository already had, so it
is the baseline and not the code under test.  The coupled solve runs a quarter as many workgroups with four times the work each.  And
what the algorithm moves per iteration and HR pixel of a channel: the dual phase reads xbar and reads and writes p0, p1 (5 doubles; the
coupled rescale of the pixel's own p, 4 more, hits the L1), the primal phase reads p0, p1, x and writes x, xbar, with v passing
through xbar (7); neighbours' values are counted as cache hits.  Then the study case (tests/tvj_common.py, seeds 0 .. 2, fp32 in and
out) at the defaults and at lambda 0.024 / Huber 0.03, coupled and per channel.  Every configuration runs in a child process of its
own under its own time limit; after a child that fails nothing more is started."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
#          name: ((groups, channels, HR side, block factor), time limit of the child in seconds)
CONFIGS = {"28x4x50x50": ((28, 4, 50, 2), 240), "1x4x384x384": ((1, 4, 384, 2), 240), "study": (None, 240)}
LO, HI, REPEATS = 1000, 2000, 7


def measure(name):
    import numpy as np
    import torch

    from mri_super_resolution_amd import ops

    (n, C, H, f), _ = CONFIGS[name]
    rng = np.random.default_rng(0)
    y = torch.from_numpy(rng.random((n, C, H // f, H // f))).cuda()
    y1 = y.reshape(n * C, H // f, H // f).contiguous()
    k = [[1.0 / (f * f)] * f] * f
    ws = torch.empty(ops.tvj_workspace_doubles(n, C, H, H), dtype=torch.float64, device="cuda")
    ws1 = torch.empty(ops.tvsr_workspace_doubles(n * C, H, H), dtype=torch.float64, device="cuda")
    solvers = {"joint": lambda it: ops.tvj_solve(y, (f, f), k, None, 0.024, 0.03, "joint", it, workspace=ws),
               "none": lambda it: ops.tvj_solve(y, (f, f), k, None, 0.024, 0.03, "none", it, workspace=ws),
               "tv_superres": lambda it: ops.tvsr_solve(y1, (f, f), k, 0.024, 0.03, it, workspace=ws1)}
    windows = {key: {LO: [], HI: []} for key in solvers}
    for fn in solvers.values():
        fn(LO), fn(HI)                                                             # warm-up: code objects, allocator
    for _ in range(REPEATS):                                                       # the solvers alternate inside every repeat
        for key, fn in solvers.items():
            for n_iter in (LO, HI):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                start.record()
                fn(n_iter)
                end.record()
                end.synchronize()
                windows[key][n_iter].append(start.elapsed_time(end))
    per = {}
    for key, w in windows.items():
        p = (np.array(w[HI]) - np.median(w[LO])) / (HI - LO) * 1e3
        per[key] = (float(np.median(p)), float(p.min()), float(p.max()), float(np.median(w[HI])))
    moved = 8 * n * C * H * H * 12
    base = per["tv_superres"]
    lines = []
    for key, label in (("joint", "tv_superres_joint, coupled"), ("none", "tv_superres_joint, coupling none")):
        t = per[key]
        lines.append(f"{name} {label}: {t[0]:.2f} us per iteration (range {t[1]:.2f} .. {t[2]:.2f} over {REPEATS}; {t[3]:.1f} ms for {HI} "
                     f"iterations), {n} workgroup(s); the algorithm moves {moved / 1e6:.2f} MB per iteration -> "
                     f"{moved / (t[0] * 1e-6) / 1e12:.3f} TB/s; {t[0] / base[0]:.2f} of tv_superres on the same {n * C} images")
    lines.append(f"{name} tv_superres (the baseline, {n * C} workgroup(s)): {base[0]:.2f} us per iteration (range {base[1]:.2f} .. {base[2]:.2f}; "
                 f"{base[3]:.1f} ms for {HI} iterations)")
    return lines


def study(name):
    import numpy as np
    import torch

    from mri_super_resolution_amd import baselines
    from tests import tvj_common as J

    lines = []
    for lam, huber in ((baselines.TVJ_DEFAULT_LAMBDA, baselines.TVJ_DEFAULT_HUBER), (J.STUDY_LAM, J.STUDY_HUBER)):
        rows = {"joint": [], "none": []}
        for seed in (0, 1, 2):
            hr, y, b = J.study_case(seed)
            y32 = torch.from_numpy(y).cuda().float().contiguous()
            for coupling in rows:
                x = baselines.tv_superres_joint(y32, (2, 2), "mean", lam, huber, J.STUDY_ITERS, None, coupling)
                assert x.dtype == torch.float32
                rows[coupling].append(J.study_scores(x.double().cpu().numpy(), hr, b))
        for coupling, r in rows.items():
            m = np.mean(r, axis=0)
            lines.append(f"{name} fp32 lambda {lam:g} huber {huber:g} {coupling}: b = 1500 PSNR {m[0]:.2f} dB, all channels {m[1]:.2f} dB, ADC RMSE "
                         f"{m[2]:.4e} (mean of seeds 0 .. 2; seed 0: {r[0][0]:.2f} dB, {r[0][1]:.2f} dB, {r[0][2]:.4e})")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tvj_time.txt"))
    ap.add_argument("--config", default=None, help="(internal) measure one configuration and print its lines")
    args = ap.parse_args()
    if args.config:
        print("\n".join((study if args.config == "study" else measure)(args.config)), flush=True)
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
