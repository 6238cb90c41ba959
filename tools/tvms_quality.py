"""The quality table of the multi-stack study, on tests/golden/pat07_volume.npz, ROI 40:90, thickness 2:
    python tools/tvms_quality.py --restated [--out profiles/tvms_quality_restated.txt]     (CPU: tests/tvms_common.py in float64)
    python tools/tvms_quality.py            [--out profiles/tvms_quality_device.txt]       (GPU box: drivers.multi_stack_study)
Per design (shifted, orthogonal, overlap) and noise (0 at lambda 3e-3, huber 0.1 -- the noiseless setting of the issue's study; 0.02
at the defaults of baselines.tv_superres_stacks), seed 0, 300 iterations: PSNR over the thin slices 2 .. 25 (data range 1) of every
stack alone, the voxel-wise mean of the single-stack solves and the joint solve; the device run adds the mean SSIM by the reference
protocol and tv_superres3d on the block stacks.  The two modes draw the same noise (one generator, the stacks in order); their
outputs, the restated one first, make up profiles/tvms_quality.txt."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DESIGNS = ("shifted", "orthogonal", "overlap")
SETTINGS = ((0.0, 3e-3, 0.1), (0.02, None, None))                     # (noise, lambda, huber); None: the defaults
ITERS, SEED = 300, 0


def restated(defaults):
    from tests import tvms_common as M
    vol = M.pat07_roi(*M.STUDY_ROI)
    lines = []
    for design in DESIGNS:
        stacks = M.design_stacks(design, vol.shape)
        for noise, lam, huber in SETTINGS:
            lam, huber = (defaults[0] if lam is None else lam), (defaults[1] if huber is None else huber)
            ys = M.study_data(vol, stacks, noise, SEED)
            singles = [M.solve([y], [st], vol.shape, lam, huber, ITERS) for y, st in zip(ys, stacks)]
            scores = [f"stack{s} {M.trim_psnr(vol, x):.3f}" for s, x in enumerate(singles)]
            if len(stacks) > 1:
                scores.append(f"mean {M.trim_psnr(vol, sum(singles) / len(singles)):.3f}")
                scores.append(f"joint {M.trim_psnr(vol, M.solve(ys, stacks, vol.shape, lam, huber, ITERS)):.3f}")
            lines.append(f"restated {design} noise {noise:g} lambda {lam:g} huber {huber:g}: PSNR dB " + ", ".join(scores))
            print(lines[-1], flush=True)
    return lines


def device(defaults):
    from tests import tvms_common as M
    from mri_super_resolution_amd import drivers
    vol = M.pat07_roi(*M.STUDY_ROI)
    lines = []
    for design in DESIGNS:
        for noise, lam, huber in SETTINGS:
            lam, huber = (defaults[0] if lam is None else lam), (defaults[1] if huber is None else huber)
            res = drivers.multi_stack_study(vol, design, 2, noise, SEED, None, lam, huber, ITERS)
            scores = [f"{m} {res['psnr'][m]:.3f} / {float(res['ssim'][m][res['valid']].mean()):.4f}" for m in res["psnr"]]
            lines.append(f"device {design} noise {noise:g} lambda {lam:g} huber {huber:g}: PSNR dB / mean SSIM " + ", ".join(scores))
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--restated", action="store_true", help="the float64 NumPy restatement on the CPU instead of the device")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mri_super_resolution_amd import baselines
    defaults = (baselines.TVMS_DEFAULT_LAMBDA, baselines.TVMS_DEFAULT_HUBER)
    lines = restated(defaults) if args.restated else device(defaults)
    out = args.out or os.path.join(ROOT, "profiles", f"tvms_quality_{'restated' if args.restated else 'device'}.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
