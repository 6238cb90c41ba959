#!/usr/bin/env python3
"""Headline benchmark: voxels/sec of the INR fit on a synthetic 128^3 volume (x4 up-scaling config).

One "step" = one full-batch fit step (forward + MSE + backward + Adam) over the N = 64*64*128 = 524,288
LR coordinates of the volume (LR = vol[::2, ::2, :]); Siren(256,512,3,1), Fourier
features 128 x sigma 0.5, Adam 1e-4 -- the loop of superresDWI.py:132-138.  Inputs (feature matrix,
targets, weights) are resident in HBM before the timed region.  `value` = coordinate-steps per second
summed over all ranks (each rank fits its own volume: weak scaling, no data-path collective; the
only collective is the final all_gather of metric records over RCCL).

A plain run sets up, warms up, times `--steps` steps and prints the headline line; `--dump-outputs DIR` writes what the timed
steps computed (losses, final parameters) as .npy files.  Everything below is measured with `--full` only.

Extra objects on the JSON line: `roofline` (the GEMM kernels, HIP-event timed inside the timed region on the stream they
run on; `traffic` from the tracked rocprofv3 PMC summary, null when that summary was taken from other kernel sources),
`fp32_mfma` (the same steps on the exact-fp32 f32-input MFMA kernels: the figure that owes nothing to the fp16 split),
`full_fit` (a complete 2,500-step fit + dense x4 re-sampling: voxels/s PER INR FIT, end to end), `recon` (warmed, averaged),
`cpu_baseline` (the torch-CPU port of the reference loop on a bounded row sample, thread count swept) and the real-data /
other-config legs (`quality`, `cfg2_real_volume`, `cfg5_te_fits`, `rams`, `hybrid_fit`).
"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: fp32 MFMA dense peak (32x32x2 and 16x16x4 alike)
PEAK_F16_MFMA_TFLOPS = 2500.0     # MI355X_MICROARCH.md: dense fp16/bf16 MFMA peak (the 2:1-sparsity figure is not used)
PEAK_HBM_GBPS = 8000.0            # MI355X_MICROARCH.md: HBM3E peak (about 6.3 TB/s is what streaming kernels reach)
IN_F, HIDDEN, LAYERS, OUT_F = 256, 512, 3, 1
SIDE = 128


def flops_per_coord():
    fwd = 2 * IN_F * HIDDEN + LAYERS * 2 * HIDDEN * HIDDEN          # sine-layer GEMMs (head is a row-dot)
    dw = fwd                                                         # param-grad GEMMs, same shapes
    dx = LAYERS * 2 * HIDDEN * HIDDEN                                # input-grad GEMMs (none for layer 0)
    return fwd, dx, dw


def source_hash():
    """sha256 over the kernel sources: ties a tracked PMC summary to the code it was measured on (the GPU box has no .git)."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "mri-super-resolution_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".inc", ".h")):
            with open(os.path.join(d, f), "rb") as fh:
                h.update(f.encode() + b"\0" + fh.read())
    with open(os.path.join(ROOT, "mri-super-resolution_amd", "_build.py"), "rb") as fh:      # the compiler flags are part of the code
        h.update(b"_build.py\0" + fh.read())
    return h.hexdigest()[:16]


def synthetic_volume(side, seed=0):
    """np.random.default_rng(seed).random((side,)*3) as fp32."""
    return np.random.default_rng(seed).random((side, side, side)).astype(np.float32)


def dump_outputs(out_dir, losses, net):
    """What a caller of the timed path receives, as float32 .npy files: `losses.npy` (the per-step losses `SirenFitter.step`
    returned for the timed steps) and `param.<name>.npy` for every parameter of the network after the last of them (~3.7 MB)."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"losses": losses}
    arrays.update((f"param.{name}", p) for name, p in net.named_parameters())
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), t.detach().float().cpu().numpy())


def cpu_baseline(n_sweep, steps, warmup, B_np, vol, thread_counts):
    """Torch-CPU port of the reference loop (oracle/torch_port: nn.Linear -> *30 -> sin, autograd, torch.optim.Adam) on the SAME
    workload: all 524,288 LR rows, `warmup` + `steps` full-batch steps at the best thread count, which a one-step sweep over
    `thread_counts` on the first `n_sweep` rows picks.  BASELINE.md section 3 asks for 5 + >= 20 steps; at ~10 s per step on
    the host that is four minutes of a run the driver wants back within a few, so the step counts are bounded (a rate metric:
    the per-step time does not depend on how many steps are timed) and the deviation is stated in `sample`."""
    from oracle import torch_port as P
    lr = vol[::2, ::2, :]
    grid = P.port_mgrid(lr.shape)
    x = P.port_input_mapping(grid, torch.from_numpy(B_np))
    t = torch.from_numpy(np.ascontiguousarray(lr).reshape(-1, 1))
    n_all = x.shape[0]
    sweep = []
    for nt in thread_counts:
        torch.set_num_threads(nt)
        torch.manual_seed(0)
        net = P.PortSiren(IN_F, HIDDEN, LAYERS, OUT_F)
        opt = torch.optim.Adam(lr=1e-4, params=list(net.parameters()))
        P.port_fit(net, x[:n_sweep], t[:n_sweep], 1, optimizer=opt)
        t0 = time.perf_counter()
        P.port_fit(net, x[:n_sweep], t[:n_sweep], 2, optimizer=opt)
        sweep.append({"threads": nt, "rows": n_sweep, "voxels_per_s": n_sweep * 2 / (time.perf_counter() - t0)})
    best_nt = max(sweep, key=lambda r: r["voxels_per_s"])["threads"]
    torch.set_num_threads(best_nt)
    torch.manual_seed(0)
    net = P.PortSiren(IN_F, HIDDEN, LAYERS, OUT_F)
    opt = torch.optim.Adam(lr=1e-4, params=list(net.parameters()))
    P.port_fit(net, x, t, warmup, optimizer=opt)
    t0 = time.perf_counter()
    P.port_fit(net, x, t, steps, optimizer=opt)
    dt = time.perf_counter() - t0
    return {"value": n_all * steps / dt, "unit": "voxels/s", "cores": best_nt, "kind": "port",
            "sample": f"all {n_all} LR rows of the synthetic 128^3 fit, {steps} timed full-batch steps after {warmup} warm-up at "
                      f"{best_nt} threads (BASELINE.md section 3 asks for 5 + 20: bounded here to keep the run within minutes -- the "
                      f"5 + 20 form, run once on the GPU box's host, is profiles/r04_cpu_baseline.json: 73.4 k voxels/s at 32 threads; "
                      f"thread count picked by a 2-step sweep on {n_sweep} rows), torch {torch.__version__} CPU "
                      f"({os.cpu_count()} logical CPUs visible)",
            "seconds": dt, "ms_per_step": dt / steps * 1e3, "thread_sweep": sweep}


def sample_power(out):
    """One `rocm-smi` reading (shader clock, package power) taken from a timer thread while the long fit runs: the fused steps
    are power-limited, so the clock the GPU actually holds belongs next to the throughput."""
    import re
    import subprocess
    try:
        txt = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level:.*?\((\d+)Mhz\)", txt)
        w = re.search(r"Power \(W\):\s*([0-9.]+)", txt)
        if m:
            out["sclk_mhz"] = int(m.group(1))
        if w:
            out["package_watts"] = float(w.group(1))
    except Exception as e:  # noqa: BLE001 -- telemetry is optional
        out["error"] = str(e)[:100]


NOMINAL_SCLK_MHZ = 2400.0         # the clock the dense MFMA peaks of MI355X_MICROARCH.md are quoted at


def add_clock_adjusted(roofline, sclk_mhz, source, watts=None):
    """The MFMA fractions of the bench line beside the peak the HELD shader clock allows (peak x sclk / 2.4 GHz): the fused steps sit
    at the 1,400 W package cap, where the chip holds ~1.6 GHz, so "0.37 of nominal" is ~0.55 of what the cap leaves.  HBM bandwidth does
    not scale with the shader clock: the HBM fraction stays as it is."""
    scale = sclk_mhz / NOMINAL_SCLK_MHZ
    peak = PEAK_F16_MFMA_TFLOPS * scale
    k = roofline.get("mfma_of_this_kernel", {})
    m = roofline.get("mfma", {})
    roofline["clock_adjusted"] = {
        "sclk_mhz": sclk_mhz, "nominal_sclk_mhz": NOMINAL_SCLK_MHZ, "package_watts": watts, "source": source,
        "fp16_mfma_peak_at_held_clock_tflops": peak,
        "dominant_kernel_frac_executed": (k.get("executed_tflops") / peak) if k.get("executed_tflops") else None,
        "whole_step_frac_executed": (m.get("executed_tflops") / peak) if m.get("executed_tflops") else None,
        "hbm": "clock-independent: roofline.frac stands"}


def cfg1_quality(inr, steps=2500, max_seeds=60):
    """Config 1 on the committed real slice: fit the 64x64 LR of pat07 slice 11, PSNR of the x2 recon vs HR, for every seed the
    REAL reference was run at (tests/golden/cfg1_ref_psnr.npz, oracle/gen_golden_t4.py; seed s drives the Fourier matrix and the
    weights as in superresDWI.py).  Full-batch Adam at this loss level spikes now and then (the reference's own numbers move by
    +-0.2 dB between seeds and thread counts), so the comparable figure is the difference of the MEANS over seeds with its
    standard error: `delta_db` +- `se_db` (north_star: within 0.05 dB)."""
    path = os.path.join(ROOT, "tests", "golden", "pat07_slice11.npz")
    ref_path = os.path.join(ROOT, "tests", "golden", "cfg1_ref_psnr.npz")
    if not (os.path.exists(path) and os.path.exists(ref_path)):
        return None
    from mri_super_resolution_amd import drivers
    hr = np.load(path)["hr"]
    ref = np.load(ref_path)
    seeds = [int(v) for v in ref["seeds"]][:max_seeds]
    ref_db = np.asarray(ref["psnr_db"], np.float64)[:len(seeds)]
    psnrs, dts, finals = [], [], []
    for seed in seeds:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = drivers.fit_volume(hr, steps=steps, seed=seed, return_recon=False)
        torch.cuda.synchronize()
        dts.append(time.perf_counter() - t0)
        psnrs.append(float(res["psnr_db"]))
        finals.append(float(res["final_loss"]))
    ours = np.asarray(psnrs, np.float64)
    se = float(np.sqrt(ours.var(ddof=1) / len(ours) + ref_db.var(ddof=1) / len(ref_db)))
    # spike-robust forms: full-batch Adam at a ~5e-7 loss level spikes, and a fit that ends ON a spike is several dB down for ~50
    # steps -- the reference's own seed 14 ends at 30.98 dB.  5 %-trimmed means (what tests/test_gpu_cfg4.py holds to 0.05 dB +
    # 2 se) and medians are what a single such seed does not move.
    k = max(1, len(ours) // 20)
    trim = lambda a: np.sort(a)[k:len(a) - k]                                                          # noqa: E731
    to, tr = trim(ours), trim(ref_db)
    se_trim = float(np.sqrt(to.var(ddof=1) / len(to) + tr.var(ddof=1) / len(tr)))
    low = lambda a: [int(i) for i in np.nonzero(a < np.median(a) - 1.0)[0]]                             # noqa: E731
    return {"config": f"pat07 slice 11, 64x64 LR -> 128x128, {steps} steps, {len(seeds)} seeds (those of the reference runs)",
            "psnr_db_mean": float(ours.mean()), "psnr_db_sigma": float(ours.std(ddof=1)),
            "reference_cpu_psnr_db_mean": float(ref_db.mean()), "reference_cpu_psnr_db_sigma": float(ref_db.std(ddof=1)),
            "delta_db": float(ours.mean() - ref_db.mean()), "se_db": se, "n_seeds": len(seeds),
            "delta_db_trimmed": float(to.mean() - tr.mean()), "se_db_trimmed": se_trim,
            "delta_db_median": float(np.median(ours) - np.median(ref_db)),
            "seeds_ending_on_a_spike": {"ours": low(ours), "reference": low(ref_db),
                                        "rule": "PSNR more than 1 dB under the median of its own series"},
            "psnr_db_trimmed_mean": float(np.sort(ours)[1:-1].mean()),
            "reference_cpu_psnr_db_trimmed_mean": float(np.sort(ref_db)[1:-1].mean()),
            "psnr_db_per_seed": [round(v, 3) for v in psnrs], "reference_cpu_psnr_db_per_seed": [round(float(v), 3) for v in ref_db],
            "note": "delta = mean(ours) - mean(reference), se = two-sample standard error; a fit caught on an Adam spike at step "
                    "2,500 is several dB down for ~50 steps (profiles/r05_t4_paths.json: sixty seeds on both arithmetic paths, per-seed traces and spike "
                    "statistics -- the paths are statistically indistinguishable, each has one such seed)",
            "final_loss_seed0": finals[0], "fit_recon_eval_seconds_seed0": dts[0],
            "train_voxels_per_s": res["n_coords"] * steps / res["t_fit"]}


def cfg2_leg(steps=2500):
    """Config 2: the whole pat07 mean-b0 volume (128x128x28, committed fixture): LR 64x64x28 (N = 114,688), full
    2,500-step fit, x4 re-sampling to 256x256x28, PSNR / mean per-slice SSIM of the HR-grid reconstruction."""
    path = os.path.join(ROOT, "tests", "golden", "pat07_volume.npz")
    if not os.path.exists(path):
        return None
    from mri_super_resolution_amd import drivers
    vol = np.load(path)["vol"]
    res = drivers.fit_volume(vol, steps=steps, seed=0, return_recon=False)
    return {"config": "pat07_mean_b0 (128,128,28): LR 64x64x28 -> x4 grid 256x256x28, 2500 steps, seed 0",
            "n_coords": res["n_coords"], "t_fit_s": res["t_fit"], "t_recon_s": res["t_recon"],
            "train_voxels_per_s": res["train_voxels_per_s"], "recon_voxels_per_s": res["recon_voxels_per_s"],
            "e2e_voxels_per_s": res["e2e_voxels_per_s"], "psnr_db": res.get("psnr_db"), "ssim_mean": res.get("ssim_mean"),
            "final_loss": res["final_loss"]}


def cfg4_leg(steps=2500):
    """Config 4 on ONE GPU: all 11 patients' mean-b0 volumes (committed fixtures, z = 24 / 28 / 34) fitted one after the
    other through `drivers.run_volumes` (2,500 steps + x4 re-sampling + PSNR / SSIM each): the single-GPU time the 8-GPU
    plan (dist.plan_fits: three 34-slice volumes row-sharded over 3 + 3 + 2 ranks, the rest one per rank) divides."""
    p7 = os.path.join(ROOT, "tests", "golden", "pat07_volume.npz")
    rest = os.path.join(ROOT, "tests", "golden", "patients_mean_b0.npz")
    if not (os.path.exists(p7) and os.path.exists(rest)):
        return None
    from mri_super_resolution_amd import dist as inr_dist
    from mri_super_resolution_amd import drivers
    z = np.load(rest)
    names = sorted(list(z.keys()) + ["pat07"])
    vols = [np.load(p7)["vol"] if n == "pat07" else z[n] for n in names]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    recs = drivers.run_volumes(vols, steps=steps, seed=0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    costs = [float(64 * 64 * v.shape[2]) * steps for v in vols]
    plan8 = drivers.plan_volumes(vols, steps, 8)
    return {"config": f"11 patients (z = {sorted(set(v.shape[2] for v in vols))}), LR 64x64xz -> x4, {steps} steps each, one GPU",
            "seconds_total": dt, "coordinate_steps_per_s": sum(costs) / sum(r["t_fit"] for r in recs),
            "psnr_db": {n: round(r["psnr_db"], 3) for n, r in zip(names, recs)},
            "ssim_mean": {n: round(r["ssim_mean"], 4) for n, r in zip(names, recs)},
            "psnr_db_mean": float(np.mean([r["psnr_db"] for r in recs])),
            "modelled_speedup_8_gpus": dt / plan8["makespan"],
            "modelled_8_gpu_plan": {"gangs": [[j, r] for j, r in plan8["gangs"]], "whole": plan8["whole"],
                                    "makespan_s": plan8["makespan"], "per_rank_s": plan8["loads"], "one_rank_s_model": plan8["one_rank"]},
            "modelled_note": "makespan from dist.StepTimeModel: per-fit and per-shard step times MEASURED on one GPU "
                             "(profiles/r05_step_time_table.json), the per-step all-reduce of a row-sharded fit MODELLED (RCCL has "
                             "not run: no multi-GPU node); divided into THIS run's measured one-GPU seconds"}


def eleven_patients_leg(steps):
    """north_star's multi-GPU figure ("the 11-patient batch"): the eleven committed patNN_mean_b0 volumes through
    `drivers.run_volumes` over ALL ranks of this job -- the plan of dist.plan_fits (row-sharded gangs first, each with one
    gradient all-reduce per step over RCCL, then whole volumes, LPT), one all_gather of metric records at the end.  Called by
    every rank; returns the record on every rank (rank 0 prints it).  Speed-up over one GPU = the `seconds` of the N = 1 run's
    `cfg4_eleven_patients` leg / these `seconds` (the driver has both lines)."""
    p7 = os.path.join(ROOT, "tests", "golden", "pat07_volume.npz")
    rest = os.path.join(ROOT, "tests", "golden", "patients_mean_b0.npz")
    if not (os.path.exists(p7) and os.path.exists(rest)):
        return None
    from mri_super_resolution_amd import dist as inr_dist
    from mri_super_resolution_amd import drivers
    z = np.load(rest)
    names = sorted(list(z.keys()) + ["pat07"])
    vols = [np.load(p7)["vol"] if n == "pat07" else z[n] for n in names]
    world = dist.get_world_size() if dist.is_initialized() else 1
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    stats = {}
    recs = drivers.run_volumes(vols, steps=steps, seed=0, stats=stats)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    per_rank = inr_dist.gather_records({"busy_s": stats["busy_s"], "seconds": dt})
    plan = stats["plan"]
    units = sum(float(r["n_coords"]) * steps for r in recs)
    seconds = max(r["seconds"] for r in per_rank)
    return {"config": f"11 patients (z = {sorted(set(v.shape[2] for v in vols))}), LR 64x64xz -> x4, {steps} steps each, "
                      f"{world} rank(s): fit + re-sampling + PSNR / SSIM per volume",
            "steps": steps, "seconds": seconds, "coordinate_steps_per_s": units / seconds,
            "plan": {"gangs": [[int(j), list(r)] for j, r in plan["gangs"]], "whole": [list(w) for w in plan["whole"]],
                     "modelled_makespan_s": plan["makespan"], "modelled_one_rank_s": plan["one_rank"], "unit": plan["unit"]},
            "per_rank_busy_s": [r["busy_s"] for r in per_rank],
            "psnr_db_mean": float(np.mean([r["psnr_db"] for r in recs])),
            "final_loss_max": float(max(r["final_loss"] for r in recs))}


def rams_leg(reps=3):
    """Config 3 (multi-image CNN): RAMS(3,32,3,9,8,12) forward on synthetic (B,128,128,9) uint16-range stacks: B = 25 = the
    25 random 9-acquisition subsets of one case (multi-image-super-resolution/master.py:43-52) as one batched call, and
    B = 1, the reference's own call shape; and one `train_step` (utils/training.py:193-209) at the reference's training shape,
    batch 32 of 32x32x9 patches.  The 32 -> 32 convolutions -- forward, data gradient and weight gradient -- run on the fp16 matrix
    cores with hi/lo-split operands staged in LDS."""
    from mri_super_resolution_amd import rams
    model = rams.RAMS(seed=0)
    out = {"config": "RAMS(3,32,3,9,8,12) predict_tensor, (B,128,128,9) -> (384,384), random weights", "flop_per_stack": 265.0e9,
           "peak_tflops_fp32_mfma": PEAK_F32_MFMA_TFLOPS, "peak_tflops_fp32_equivalent_split_fp16": PEAK_F16_MFMA_TFLOPS / 3.0}
    for batch in (25, 1):
        x = torch.from_numpy((np.random.default_rng(0).random((batch, 128, 128, 9)) * 60000).astype(np.float32)).cuda()
        rams.predict_tensor(model, x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            rams.predict_tensor(model, x)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        out[f"batch{batch}"] = {"ms_per_stack": dt / batch * 1e3, "stacks_per_s": batch / dt,
                                "output_voxels_per_s": batch * 384 * 384 / dt, "tflops": 265.0e9 * batch / dt / 1e12}
    # training step: ~3 forward-equivalents (forward, data gradient, weight gradient) of 32 patches of 32 x 32 x 9
    B, P = 32, 32
    rng = np.random.default_rng(1)
    tr = rams.RamsTrainer(model)
    lr = (rng.random((B, P, P, 9)) * 20000).astype(np.float32)
    hr = (rng.random((B, 3 * P, 3 * P, 1)) * 20000).astype(np.float32)
    mask = np.ones((B, 3 * P, 3 * P, 1), np.float32)
    for _ in range(2):                                     # (the first call sizes the trainer's workspace)
        tr.train_step(lr, hr, mask)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(2 * reps):
        tr.train_step(lr, hr, mask)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / (2 * reps)
    out["train_step"] = {"batch": B, "patch": P, "ms_per_step": dt * 1e3,
                         "tflops": 3 * 265.0e9 * (P * P) / (128 * 128) * B / dt / 1e12}
    return out


def compat_loop_leg(x, target, steps=20, warmup=3):
    """The reference's loop UNMODIFIED (superresDWI.py:132-138: `INR(x)` -> `((out - gt)**2).mean()` -> `zero_grad()` ->
    `loss.backward()` -> `torch.optim.Adam.step()`) on the 128^3 workload: what a user who only swaps the import line gets.
    `Siren.forward` under autograd runs the fused fit's kernels (inr_siren_forward_train / inr_siren_backward_train); the loss and
    Adam are torch's own ATen kernels.  `layer_by_layer_ms_per_step`: the same loop with `inr.HP_AUTOGRAD = False` (one autograd
    Function over the stand-alone exact-fp32 layer entry points: what this loop ran on through round 3)."""
    import mri_super_resolution_amd as inr
    from mri_super_resolution_amd import inr as inr_mod

    def run(hp, k):
        inr_mod.HP_AUTOGRAD = hp
        try:
            torch.manual_seed(0)
            INR = inr.Siren(IN_F, HIDDEN, LAYERS, OUT_F).cuda()
            inr_optim = torch.optim.Adam(lr=1e-4, params=INR.parameters())
            loss = None
            for ctr in range(warmup + k):
                if ctr == warmup:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                model_output = INR(x)
                loss = ((model_output - target) ** 2).mean()
                inr_optim.zero_grad()
                loss.backward()
                inr_optim.step()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / k
            final = float(loss.detach())
            del INR, inr_optim, model_output, loss
            torch.cuda.empty_cache()
            return dt, final
        finally:
            inr_mod.HP_AUTOGRAD = True

    dt, final = run(True, steps)
    dt_old, _ = run(False, max(5, steps // 2))
    n = x.shape[0]
    return {"config": "superresDWI.py:132-138 verbatim through compat/SRDWI's Siren: torch autograd + torch.optim.Adam around "
                      "inr_siren_forward_train / inr_siren_backward_train, synthetic 128^3 workload",
            "ms_per_step": dt * 1e3, "voxels_per_s": n / dt, "steps": steps, "final_loss": final,
            "layer_by_layer_ms_per_step": dt_old * 1e3}


def small_net_leg(steps=2000, side=60, n_acq=4):
    """The master.py regime (a-11): Siren(2,64,6,1) on a 60x60 slice, weighted loss, the acquisition changing every step:
    microseconds per optimizer step through one inr_siren_fit_cycle call (persistent kernel, 64 steps per launch)."""
    import mri_super_resolution_amd as inr
    torch.manual_seed(0)
    net = inr.Siren(2, 64, 6, 1).cuda()
    coords = inr.ImageFitting_set([np.zeros((side, side), np.float32)]).coords[0]
    tg = torch.rand(n_acq, side * side, device="cuda") * 2 - 1
    wt = torch.rand(n_acq, side * side, device="cuda")
    f = inr.SirenFitter(net, lr=3e-4)
    f.step_cycle(coords, tg, 64, wt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f.step_cycle(coords, tg, steps, wt)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {"config": f"Siren(2,64,6,1), N = {side * side} rows, {n_acq} acquisitions cycling, weighted MSE, Adam 3e-4",
            "us_per_optimizer_step": dt * 1e6, "train_voxels_per_s": side * side / dt, "steps": steps}


def small_fits_leg(n_fits=12, side=128, steps=300):
    """Many slice-sized fits on one GPU (config-1 shape: 128 x 128 slice -> 4,096 training rows): `drivers.run_volumes` one at a time
    and four side by side on streams of their own (every fit bit-identical to its solitary run); fit + x2 re-sampling, no metrics."""
    from mri_super_resolution_amd import drivers
    rng = np.random.default_rng(3)
    vols = [rng.random((side, side)).astype(np.float32) + 0.05 for _ in range(n_fits)]
    drivers.run_volumes(vols[:2], steps=10, evaluate=False)
    out = {"config": f"{n_fits} fits of a {side} x {side} slice ({side * side // 4} rows each), {steps} steps + re-sampling", "fits": n_fits}
    for k in (1, 4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        recs = drivers.run_volumes(vols, steps=steps, concurrent=k, evaluate=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[f"concurrent_{k}"] = {"seconds": dt, "coordinate_steps_per_s": sum(r["n_coords"] for r in recs) * steps / dt}
    out["speedup"] = out["concurrent_1"]["seconds"] / out["concurrent_4"]["seconds"]
    return out


def cfg5_leg(steps=4):
    """Config 5 (superresHybrid.py:79-125 on a synthetic 256^3 hybrid volume): FOUR echo-time fits, each LR 128x128x256 =
    4,194,304 rows, Siren(256,512,3,1), targets stored in fp16 (as BASELINE config 5 says) and widened on the device per
    fit; a few fused steps per fit (a full fit is 2,500).  On one GPU the four fits run back to back; on N GPUs
    `dist.plan_fits` puts one per rank (or row-shards them over rank pairs)."""
    from mri_super_resolution_amd import drivers, inr, ops
    shape = (128, 128, 256)
    n = shape[0] * shape[1] * shape[2]
    x = ops.grid_fourier_map(shape, torch.from_numpy(drivers.fourier_matrix(3, seed=0)).cuda())
    targets16 = torch.rand(4, n, device="cuda").half()                  # the four TE volumes, 2 bytes per voxel
    per_fit = []
    for te in range(4):
        torch.manual_seed(te)
        net = inr.Siren(256, 512, 3, 1).cuda()
        fitter = inr.SirenFitter(net, lr=1e-4)
        target = targets16[te].float()
        fitter.step(x, target, n_steps=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fitter.step(x, target, n_steps=steps)
        torch.cuda.synchronize()
        per_fit.append((time.perf_counter() - t0) / steps)
        fitter.release_workspace()
    dt = float(np.mean(per_fit))
    return {"config": "synthetic 256^3 x 4 TE, LR 128x128x256 (N=4194304 rows per fit), fp16-stored targets, "
                      "Siren(256,512,3,1), fused steps, four fits back to back on one GPU",
            "ms_per_step": dt * 1e3, "ms_per_step_each_te": [v * 1e3 for v in per_fit], "train_voxels_per_s": n / dt,
            "gemm_tflops_equiv": n * 5242880 / dt / 1e12, "target_bytes_per_voxel": 2}


def hybrid_fit_leg(n=120 * 120 * 4):
    """(f)-1: three-compartment fit of four 120x120 slices worth of voxels (PIA.hybrid_fit, superresHybrid.py:140),
    2 % noise; next to scipy's curve_fit on 32 of the same voxels on one host core."""
    from mri_super_resolution_amd import pia
    from scipy.optimize import curve_fit
    sig_np = pia.phantom_signals(n, 0.02, seed=5)
    sig = torch.from_numpy(sig_np).cuda()
    pia.hybrid_fit_device(sig[:6400])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = pia.hybrid_fit_device(sig)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    b16, te16 = pia.acquisition_table()
    t0 = time.perf_counter()
    for y in sig_np[:32]:
        try:
            curve_fit(pia.three_compartment_fit, np.vstack([b16, te16]), y, p0=list(pia.P0), bounds=(list(pia.LB), list(pia.UB)),
                      method="trf", maxfev=5000)
        except RuntimeError:
            pass
    dt_cpu = (time.perf_counter() - t0) / 32
    return {"config": f"{n} voxels x 16 signals, 2% noise, fp64 TRF, maxfev 5000", "seconds": dt,
            "voxel_fits_per_s": n / dt, "mean_nfev": float(out["nfev"].double().mean()),
            "scipy_voxel_fits_per_s_1core": 1.0 / dt_cpu}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip recon/quality legs (profiling runs)")
    ap.add_argument("--cpu-sample", type=int, default=65536, help="LR rows of the CPU baseline's thread-count sweep")
    ap.add_argument("--cpu-steps", type=int, default=3, help="timed full-workload steps of the CPU baseline")
    ap.add_argument("--cpu-warmup", type=int, default=1)
    ap.add_argument("--eleven-steps", type=int, default=2500, help="steps per fit of the 11-patient leg at --gpus N > 1")
    ap.add_argument("--no-eleven", action="store_true", help="skip the 11-patient leg at --gpus N > 1")
    ap.add_argument("--no-full-fit", action="store_true", help="skip the complete 2,500-step fit (about half a minute)")
    ap.add_argument("--no-cfg4", action="store_true", help="skip the 11-patient leg (about a minute)")
    ap.add_argument("--fp32-mfma", action="store_true",
                    help="A/B: run the GEMMs on the f32-input MFMA kernels instead of the split-fp16 ones")
    ap.add_argument("--full", action="store_true",
                    help="also every secondary figure: roofline (per-class HIP events inside the timed steps), exact-fp32 leg, "
                         "recon / full fit / real-data and other-config legs, CPU baseline, 11-patient leg at --gpus N > 1 "
                         "(the --no-* / --cpu-* / --eleven-* options act within it); a plain run times the headline steps only")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what they computed as DIR/<name>.npy (float32): the per-step losses the "
                         "fit call returned and the network's parameters after its last step (rank 0's fit)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: start the N ranks as a CHILD job (one process per GPU under
        # torch.distributed.run) and relay rank 0's JSON line.  Nothing in this process has touched the GPU yet (no HIP call, no
        # torch.cuda.is_available()), and the child is started, never exec'ed into.
        import socket
        import subprocess
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")).returncode)
    if args.gpus > 1 and world == 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE=1")
    assert torch.cuda.is_available(), "bench.py needs a HIP device"
    device_index = local_rank % torch.cuda.device_count()   # (a rehearsal may put several ranks on one card)
    torch.cuda.set_device(device_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("INR_BENCH_BACKEND", "nccl")   # "gloo" only to rehearse the N > 1 path on one GPU
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device_index))
        else:
            dist.init_process_group(backend)

    import mri_super_resolution_amd as inr
    from mri_super_resolution_amd import dist as inr_dist
    from mri_super_resolution_amd import ops
    from mri_super_resolution_amd._lib import lib as inr_lib
    from mri_super_resolution_amd import drivers
    inr_lib().inr_debug_set(3, 0 if args.fp32_mfma else 1)
    for kv in filter(None, os.environ.get("INR_DEBUG_KEYS", "").split(",")):   # e.g. "5=0,6=0": A/B of tuning switches
        k, v = kv.split("=")
        inr_lib().inr_debug_set(int(k), int(v))

    # ---- workload: one synthetic 128^3 volume per rank (seeded by rank), resident in HBM -------------
    vol = synthetic_volume(SIDE, seed=rank)
    lr = np.ascontiguousarray(vol[::2, ::2, :])
    n_lr = lr.size
    B_np = drivers.fourier_matrix(3, seed=0)
    B = torch.from_numpy(B_np).cuda()
    torch.manual_seed(0)
    net = inr.Siren(IN_F, HIDDEN, LAYERS, OUT_F).cuda()
    x = ops.grid_fourier_map(lr.shape, B)                           # [N, 256] feature matrix, built once per fit
    target = torch.from_numpy(lr.reshape(-1, 1)).cuda()
    fitter = inr.SirenFitter(net, lr=1e-4)

    fitter.step(x, target, n_steps=args.warmup)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    if args.full:
        ops.prof_reset()
        ops.prof_enable(True)
    t0 = time.perf_counter()
    losses = fitter.step(x, target, n_steps=args.steps)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.full:
        ops.prof_enable(False)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, losses, net)

    # ---- final metric gather (the only collective on the path) --------------------------------------
    record = {"rank": rank, "n": n_lr, "steps": args.steps, "seconds": dt, "final_loss": float(losses[-1])}
    records = inr_dist.gather_records(record)
    dt_max = max(r["seconds"] for r in records)
    total_units = sum(r["n"] * r["steps"] for r in records)

    eleven = None
    if world > 1 and args.full and not args.no_eleven:
        fitter.release_workspace()
        try:
            eleven = eleven_patients_leg(args.eleven_steps)   # every rank takes part (gangs, all-reduce, gather)
        except Exception as e:  # noqa: BLE001 -- the weak-scaling figure above is measured: report the leg's failure, keep the line
            eleven = {"error": f"{type(e).__name__}: {e}"[:400]}

    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    out = {"metric": "voxels/sec per INR fit (128^3, x4 upscale): train coordinate-steps/s",
           "value": total_units / dt_max, "unit": "voxels/s", "n_gpus": world, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": dt_max / args.steps * 1e3, "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None,
           "dtype": "f32" if args.fp32_mfma else "f32 as 3 x f16 MFMA products (hi/lo split operands, f32 accumulate)",
           "data": "synthetic",
           "config": {"workload": "synthetic 128^3 volume, LR 64x64x128 (N=524288 coords) -> x4 grid 256x256x128; "
                                  "Siren(256,512,3,1) + 128 Fourier features, Adam 1e-4, full-batch MSE",
                      "per_gpu_rows": n_lr, "parallelism": f"{world} independent fits (one volume per GPU)"},
           "kernel_source_hash": source_hash()}
    if not args.full:
        print(json.dumps(out))
        if world > 1:
            dist.destroy_process_group()
        return

    fwd_f, dx_f, dw_f = flops_per_coord()
    classes = {}
    tot_ms, tot_flop, tot_launch = 0.0, 0.0, 0
    for kc, (name, fl) in enumerate((("gemm_forward", fwd_f), ("gemm_input_grad", dx_f), ("gemm_param_grad", dw_f))):
        launches, ms = ops.prof_read(kc)
        flop = fl * n_lr * args.steps
        classes[name] = {"launches": launches, "avg_ms": ms / max(launches, 1), "tflops": flop / (ms * 1e-3) / 1e12}
        tot_ms += ms
        tot_flop += flop
        tot_launch += launches
    other_launches, other_ms = ops.prof_read(3)
    # HBM traffic of the GEMM kernels per launch: PMC counters cannot be read from inside this process, so the tracked
    # rocprofv3 summary of this same command is used (profiles/r02_pmc_hbm.json: FETCH_SIZE x2 per the gfx950 correction +
    # WRITE_SIZE, separate --pmc passes, written by tools/save_profiles.py together with the hash of the kernel sources it
    # was measured on).  A summary taken from other sources is stale: traffic is then null.
    traffic, traffic_by_class, traffic_src, src_hash = None, None, None, source_hash()
    pmc_path = os.path.join(ROOT, "profiles", "r03_fp32mfma_pmc_hbm.json" if args.fp32_mfma else "r05_pmc_hbm.json")
    if os.path.exists(pmc_path):
        with open(pmc_path) as fh:
            pm = json.load(fh)
        recorded = pm.get("source_hash")
        traffic_src = f"{os.path.relpath(pmc_path, ROOT)} (kernel sources {recorded}, git {pm.get('git_head')}; these sources: {src_hash})"
        if recorded == src_hash:
            traffic = pm.get("gemm_avg_hbm_bytes_per_launch")
            traffic_by_class = pm.get("hbm_bytes_per_launch_by_class")
        else:
            traffic_src += " -- STALE, traffic withheld"
    # algorithmic HBM bytes of the 11 GEMM launches of one step, in units of one [N,512] 4-byte matrix (fp32 or HL32):
    # forward 0.5+2 (layer 0) + 3*(1+2); input-grad 3*(1+1+1); param-grad 1.5 (layer 0) + 3*2  = 28 matrices; on the
    # pre-split path the last sine layer stashes z only (its output feeds nothing but the head step): 27
    z_head = not args.fp32_mfma and "16=0" not in os.environ.get("INR_DEBUG_KEYS", "")
    algo_matrices = 27.0 if z_head else 28.0
    algo_bytes = algo_matrices * n_lr * HIDDEN * 4 / 11.0
    achieved = tot_flop / (tot_ms * 1e-3) / 1e12
    avg_ms = tot_ms / max(tot_launch, 1)
    common = {"traffic": traffic, "traffic_unit": "bytes per launch (HBM, PMC)", "traffic_source": traffic_src,
              "algorithmic_bytes_per_launch": algo_bytes, "algorithmic_matrices_per_step": algo_matrices, "launches": tot_launch, "avg_launch_ms": avg_ms,
              "gemm_ms_per_step": tot_ms / args.steps, "other_kernels_ms_per_step": other_ms / args.steps,
              "per_class": classes}
    # achieved = N * steps * 5,245,952 FLOP / t against the peak of the operand type used
    algo_tflops_step = n_lr * 5245952.0 / (dt_max / args.steps) / 1e12
    if args.fp32_mfma:
        roofline = {"bound": "mfma", "kernel": "gemm_f32_pipe16_kernel (v_mfma_f32_16x16x4_f32)", "achieved": achieved,
                    "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": achieved / PEAK_F32_MFMA_TFLOPS, **common,
                    "mfma": {"algorithmic_tflops": algo_tflops_step, "executed_tflops": algo_tflops_step,
                             "peak": PEAK_F32_MFMA_TFLOPS, "frac": algo_tflops_step / PEAK_F32_MFMA_TFLOPS}}
    else:
        # pre-split fp16 GEMMs: three fp16 MFMA products per fp32 product.  The DOMINANT kernel is the input-grad launch
        # (gemm_hp_pkd_kernel<HPE_MUL, 16>, three per step): it reads dz and the stashed factor and writes dz_prev -- three
        # [N, 512] 4-byte matrices -- so its algorithmic bytes are 3 N 512 4; at three MFMAs per product it sits on the ridge of
        # the machine (HBM roof 3.22 GB / 8 TB/s = 0.40 ms, MFMA roof 3 x 275 GFLOP / 2.5 PFLOP/s = 0.33 ms): HBM binds.
        dx = classes["gemm_input_grad"]
        dx_bytes = 3.0 * n_lr * HIDDEN * 4
        dx_gbps = dx_bytes / (dx["avg_ms"] * 1e-3) / 1e9
        dx_flop = 2.0 * n_lr * HIDDEN * HIDDEN
        gbps = algo_bytes / (avg_ms * 1e-3) / 1e9
        mfma_peak = PEAK_F16_MFMA_TFLOPS / 3.0
        roofline = {"bound": "hbm",
                    "kernel": "gemm_hp_pkd_kernel<HPE_MUL, 16> (input-grad: persistent, HL32 operands by LDS-DMA, 3 x "
                              "v_mfma_f32_16x16x32_f16 per fp32 product, epilogue deferred under the next tile's K-loop)",
                    "achieved": dx_gbps, "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": dx_gbps / PEAK_HBM_GBPS,
                    "algorithmic_bytes_per_launch": dx_bytes, "avg_launch_ms": dx["avg_ms"], "launches": dx["launches"],
                    "traffic": (traffic_by_class or {}).get("gemm_input_grad"), "traffic_unit": "bytes per launch (HBM, PMC)",
                    "traffic_source": traffic_src,
                    "mfma_of_this_kernel": {"algorithmic_tflops": dx_flop / (dx["avg_ms"] * 1e-3) / 1e12,
                                            "executed_tflops": 3.0 * dx_flop / (dx["avg_ms"] * 1e-3) / 1e12,
                                            "peak": PEAK_F16_MFMA_TFLOPS,
                                            "frac_executed": 3.0 * dx_flop / (dx["avg_ms"] * 1e-3) / 1e12 / PEAK_F16_MFMA_TFLOPS},
                    # the whole step against SURVEY.md 8(d)'s formula (every kernel's time in the denominator)
                    "mfma": {"algorithmic_tflops": algo_tflops_step, "executed_tflops": 3.0 * algo_tflops_step,
                             "peak": PEAK_F16_MFMA_TFLOPS, "frac": algo_tflops_step / PEAK_F16_MFMA_TFLOPS,
                             "frac_executed": 3.0 * algo_tflops_step / PEAK_F16_MFMA_TFLOPS,
                             "note": "SURVEY 8(d): N x steps x 5,245,952 FLOP / step time against the dense fp16 MFMA peak (the "
                                     "operand type used); executed = x3 products per fp32 product"},
                    "all_gemm_launches": {"achieved_gbps": gbps, "frac_hbm": gbps / PEAK_HBM_GBPS, **common,
                                          "tflops_fp32_equivalent": achieved, "frac_of_fp16_peak_over_3": achieved / mfma_peak},
                    "vs_fp32_mfma_peak": achieved / PEAK_F32_MFMA_TFLOPS,
                    "power_note": "peaks are the nominal 2.4 GHz figures; during these steps the package sits at its 1,400 W cap and "
                                  "the shader clock at 1.63 GHz (84 rocm-smi samples over 36 s: profiles/r04_ablate_power.txt; the "
                                  "dominant kernel's K-loop alone, on random operands, holds the package at the cap as well: "
                                  "profiles/r05_kloop_rowown_probe_shared_a.txt); clock-adjusted fractions: roofline.clock_adjusted"}
    ops.prof_reset()

    out["roofline"] = roofline
    if eleven is not None:
        out["eleven_patients"] = eleven

    if world == 1 and not args.fp32_mfma:
        # the same steps on the f32-input MFMA kernels (exact fp32 products: nothing here depends on the fp16 split)
        inr_lib().inr_debug_set(3, 0)
        torch.manual_seed(0)
        net32 = inr.Siren(IN_F, HIDDEN, LAYERS, OUT_F).cuda()
        f32 = inr.SirenFitter(net32, lr=1e-4)
        f32.step(x, target, n_steps=2)
        torch.cuda.synchronize()
        k32 = max(5, min(args.steps, 20))
        t0 = time.perf_counter()
        f32.step(x, target, n_steps=k32)
        torch.cuda.synchronize()
        dt32 = (time.perf_counter() - t0) / k32
        f32.release_workspace()
        inr_lib().inr_debug_set(3, 1)
        tf32 = n_lr * sum(flops_per_coord()) / dt32 / 1e12
        out["fp32_mfma"] = {"ms_per_step": dt32 * 1e3, "value": n_lr / dt32, "unit": "voxels/s", "steps": k32,
                            "kernel": "gemm_f32_pipe16_kernel (v_mfma_f32_16x16x4_f32, exact fp32)",
                            "gemm_tflops_incl_other_kernels": tf32, "peak_tflops": PEAK_F32_MFMA_TFLOPS,
                            "frac": tf32 / PEAK_F32_MFMA_TFLOPS}
        del net32, f32

    if not args.no_extras and world == 1:   # single-GPU run only: the N > 1 runs measure scaling of the fit itself
        grid3 = (2 * SIDE, 2 * SIDE, SIDE)
        rec = inr.reconstruct(net, grid3, B)                       # warm call: workspace allocation, code load
        torch.cuda.synchronize()
        reps = 3
        t0 = time.perf_counter()
        for _ in range(reps):
            rec = inr.reconstruct(net, grid3, B)
        torch.cuda.synchronize()
        t_rec = (time.perf_counter() - t0) / reps
        out["recon"] = {"grid": list(grid3), "voxels_per_s": rec.numel() / t_rec, "seconds": t_rec, "reps_after_warmup": reps,
                        "tflops": rec.numel() * (fwd_f + 2 * HIDDEN) / t_rec / 1e12}
        n_test = rec.numel()
        del rec
        fitter.release_workspace()
        if not args.no_full_fit:
            # what "per INR fit" means end to end: a complete 2,500-step fit of this volume + the dense x4 re-sampling
            torch.manual_seed(0)
            net_full = inr.Siren(IN_F, HIDDEN, LAYERS, OUT_F).cuda()
            torch.cuda.synchronize()
            telemetry = {}
            sampler = threading.Timer(6.0, sample_power, args=(telemetry,))   # the steps are enqueued at once: the GPU is ~6 s in
            sampler.start()
            t0 = time.perf_counter()
            _, full_losses = inr.fit_siren(net_full, x, target, 2500, lr=1e-4)
            torch.cuda.synchronize()
            t_fit = time.perf_counter() - t0
            sampler.join()
            t0 = time.perf_counter()
            rec = inr.reconstruct(net_full, grid3, B)
            torch.cuda.synchronize()
            t_inf = time.perf_counter() - t0
            out["full_fit"] = {"steps": 2500, "t_fit_s": t_fit, "t_recon_s": t_inf,
                               "train_voxels_per_s": n_lr * 2500 / t_fit, "recon_voxels_per_s": n_test / t_inf,
                               "e2e_voxels_per_s": n_test / (t_fit + t_inf), "final_loss": float(full_losses[-1]),
                               "power_during_fit": telemetry or None}
            del rec, net_full
            held = (telemetry or {}).get("sclk_mhz")
            if held and "mfma" in roofline and not args.fp32_mfma:
                add_clock_adjusted(roofline, float(held), "rocm-smi, 6 s into this run's 2,500-step fit (the same kernels, the package at its cap)",
                                   telemetry.get("package_watts"))
        out["compat_loop"] = compat_loop_leg(x, target, steps=max(5, min(args.steps, 20)))
        out["compat_loop"]["vs_fused_step"] = out["compat_loop"]["ms_per_step"] / out["ms_per_step"]
        out["quality"] = cfg1_quality(inr)
        out["rams"] = rams_leg()
        out["small_net"] = small_net_leg()
        out["small_fits_side_by_side"] = small_fits_leg()
        out["cfg2_real_volume"] = cfg2_leg()
        if not args.no_cfg4:
            out["cfg4_eleven_patients"] = cfg4_leg()
        out["cfg5_te_fits"] = cfg5_leg()
        out["hybrid_fit"] = hybrid_fit_leg()
    if world == 1 and not args.fp32_mfma and "clock_adjusted" not in roofline:
        add_clock_adjusted(roofline, 1630.0, "profiles/r04_ablate_power.txt (84 rocm-smi samples over 36 s of these steps; not sampled in this run)",
                           1400.0)
    if not args.no_cpu_baseline and world == 1:
        ncpu = os.cpu_count() or 1
        # (profiles/r04_cpu_baseline.json: 5 + 20 steps with a sweep over 32 .. 256 threads on the 2 x 64-core host -- 32 threads win)
        sweep = sorted({max(1, ncpu // 8), max(1, ncpu // 4)}) if ncpu >= 16 else [ncpu]
        out["cpu_baseline"] = cpu_baseline(args.cpu_sample, args.cpu_steps, args.cpu_warmup, B_np, vol, sweep)
        out["speedup_vs_cpu_baseline"] = out["value"] / world / out["cpu_baseline"]["value"]
    print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
