"""GPU box: the time of one iteration of the S0 / ADC solver, and the study case in fp32:
    python tools/tvadc_time.py [--out profiles/tvadc_time.txt]
28 groups of 4 b-values at (50, 50) <- (25, 25) -- the driver's ROI at x2 -- and one group of 4 b-values at (384, 384) <- (192, 192), the
block mean, fp64, seeded data that follow the model (s in [0.2, 1], ADC in [0.5, 2.5]e-3, b = 0 / 150 / 1000 / 1500, noise 0.02); device
events around whole solves (workspace allocated before) after a warm-up solve: microseconds per iteration as (t(1,000 iterations) -
t(500 iterations)) / 500 -- the start, the objective and the host's set-up cancel --, median of 7 with the range.  Beside each figure
ops.tvj_solve (baselines.tv_superres_joint, coupled) on the same data, measured the same way in the same run with the two solvers
alternating: the kernel the repository already had, so it is the baseline and not the code under test.  Both run one workgroup per
group.  The new solver holds 8 planes and C / (f0 f1) data duals per pixel instead of 4 C planes and calls the fp64 exp 2 C times per
pixel and iteration.  Then the study case (tests/tvadc_common.py, seeds 0 .. 2, fp32 in and out): the maps at the defaults and at 10,000
iterations beside tv_superres at its best ADC pair (0.024, 0.01) and tv_superres_joint at its defaults.  Every configuration runs in a
child process of its own under its own time limit; after a child that fails nothing more is started."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
#          name: ((groups, channels, HR side, block factor), time limit of the child in seconds)
CONFIGS = {"28x4x50x50": ((28, 4, 50, 2), 240), "1x4x384x384": ((1, 4, 384, 2), 240), "study": (None, 240)}
LO, HI, REPEATS = 500, 1000, 7
B = (0.0, 150.0, 1000.0, 1500.0)


def measure(name):
    import numpy as np
    import torch

    from mri_super_resolution_amd import baselines, ops
    from tests import tvadc_common as A
    from tests import tvsr_common as T

    (n, C, H, f), _ = CONFIGS[name]
    rng = np.random.default_rng(0)
    s, d = 0.2 + 0.8 * rng.random((n, H, H)), 0.5e-3 + 2e-3 * rng.random((n, H, H))
    y = T.apply_A(A.model(s, d, np.asarray(B)), T.block_kernel("mean", (f, f))) + 0.02 * rng.standard_normal((n, C, H // f, H // f))
    y = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    k = [[1.0 / (f * f)] * f] * f
    ws = torch.empty(ops.tvadc_workspace_doubles(n, C, H, H, (f, f)), dtype=torch.float64, device="cuda")
    wsj = torch.empty(ops.tvj_workspace_doubles(n, C, H, H), dtype=torch.float64, device="cuda")
    model = (baselines.ADC_DEFAULT_MAP_WEIGHTS, baselines.ADC_DEFAULT_LAMBDA, baselines.ADC_DEFAULT_HUBER, baselines.ADC_DEFAULT_COUPLING)
    box = (baselines.ADC_DEFAULT_S_MAX, baselines.ADC_DEFAULT_ADC_MAX, baselines.ADC_DEFAULT_ADC0)
    solvers = {"tv_superres_adc": lambda it: ops.tvadc_solve(y, B, (f, f), k, *model, it, *box, workspace=ws),
               "tv_superres_joint": lambda it: ops.tvj_solve(y, (f, f), k, None, baselines.TVJ_DEFAULT_LAMBDA, baselines.TVJ_DEFAULT_HUBER, "joint", it,
                                                             workspace=wsj)}
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
    t, base = per["tv_superres_adc"], per["tv_superres_joint"]
    exps = 2 * C * n * H * H
    return [f"{name} tv_superres_adc: {t[0]:.2f} us per iteration (range {t[1]:.2f} .. {t[2]:.2f} over {REPEATS}; {t[3]:.1f} ms for {HI} "
            f"iterations), {n} workgroup(s); {exps / 1e6:.3f} M fp64 exp per iteration -> {exps / (t[0] * 1e-6) / 1e9:.2f} G exp/s; "
            f"{t[0] / base[0]:.2f} of tv_superres_joint on the same data",
            f"{name} tv_superres_joint (the baseline, {n} workgroup(s)): {base[0]:.2f} us per iteration (range {base[1]:.2f} .. {base[2]:.2f}; "
            f"{base[3]:.1f} ms for {HI} iterations)"]


def study(name):
    import numpy as np
    import torch

    from mri_super_resolution_amd import baselines
    from tests import tvadc_common as A
    from tests import tvj_common as J

    hr, _, adc_true = A.study_truth()
    rows = {}
    for seed in (0, 1, 2):
        y32 = torch.from_numpy(J.study_case(seed)[1]).cuda().float().contiguous()
        host = lambda t: t.double().cpu().numpy()
        for n_iter in (baselines.ADC_DEFAULT_ITERS, 10000):
            s0, adc = baselines.tv_superres_adc(y32, A.STUDY_B.tolist(), (2, 2), "mean", n_iter=n_iter)
            assert s0.dtype == adc.dtype == torch.float32
            rows.setdefault(f"tv_superres_adc, the defaults, {n_iter} iterations (the maps)", []).append(A.map_scores(host(s0), host(adc), hr, adc_true))
            if n_iter == baselines.ADC_DEFAULT_ITERS:
                images = host(baselines.adc_signal(s0.contiguous(), adc.contiguous(), A.STUDY_B.tolist()))
                rows.setdefault("tv_superres_adc, the defaults (log-linear fit of its images)", []).append(A.image_scores(images, hr, adc_true))
        rows.setdefault("tv_superres lambda 0.024 huber 0.01, 300 iterations", []).append(
            A.image_scores(host(baselines.tv_superres(y32, (2, 2), "mean", 0.024, 0.01, 300)), hr, adc_true))
        rows.setdefault("tv_superres_joint, its defaults", []).append(A.image_scores(host(baselines.tv_superres_joint(y32, (2, 2), "mean")), hr, adc_true))
        rows.setdefault("tv_superres_joint lambda 0.024 huber 0.03 (its balanced pair)", []).append(
            A.image_scores(host(baselines.tv_superres_joint(y32, (2, 2), "mean", 0.024, 0.03)), hr, adc_true))
    lines = []
    for label, r in rows.items():
        m = np.mean(r, axis=0)
        lines.append(f"{name} fp32 {label}: b = 0 PSNR {m[0]:.2f} dB, b = 1500 PSNR {m[1]:.2f} dB, ADC RMSE {m[2]:.4e} (mean of seeds 0 .. 2; seed 0: "
                     f"{r[0][0]:.2f} dB, {r[0][1]:.2f} dB, {r[0][2]:.4e})")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tvadc_time.txt"))
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
