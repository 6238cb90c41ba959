"""GPU box: the time of MP-PCA denoising on whole stacks:
    python tools/mppca_time.py [--out profiles/mppca_time.txt]
A [16, 20, 128, 128] and a [40, 20, 128, 128] stack (the phantom of tests/mppca_common.py, noise 0.05, seed 0) with the window (5, 5, 5),
through the fp64 and the fp32 entry: device events around the call (outputs allocated by the wrapper inside the window, as a caller pays
for them), a stream synchronisation before the first event and on the second, 3 warm-up calls, then the median of 10 with the range.
M = 16 runs the rank class 16 (r = 16, q = 125), M = 40 the class 64 (r = 40, q = 125).  Beside each stack the float64 restatement
(tests/mppca_common.py: numpy, LAPACK eigh per voxel) on this box's CPU, timed on a 1/64 sub-volume [M, 5, 32, 32] and scaled by 64.
Nothing here has a target: the figures are stated as found."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STACKS = ((16, (20, 128, 128)), (40, (20, 128, 128)))
WINDOW = (5, 5, 5)
WARMUP, REPEATS = 3, 10


def main():
    import numpy as np
    import torch

    from mri_super_resolution_amd import ops
    from tests import mppca_common as P

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mppca_time.txt"))
    args = ap.parse_args()
    lines = []
    for M, shape in STACKS:
        rng = np.random.default_rng(0)
        clean, noisy = P.phantom(M, shape, P.SIGMA, rng)
        voxels = int(np.prod(shape))
        for dtype in (torch.float64, torch.float32):
            x = torch.from_numpy(noisy).to("cuda", dtype)
            for _ in range(WARMUP):
                ops.mppca_denoise(x, WINDOW)
            times = []
            for _ in range(REPEATS):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                start.record()
                out, sigma, rank = ops.mppca_denoise(x, WINDOW)
                end.record()
                end.synchronize()
                times.append(start.elapsed_time(end))
            t = float(np.median(times))
            ratio = P.rmse(out.double().cpu().numpy(), clean) / P.rmse(noisy, clean)
            lines.append(f"[{M}, {', '.join(map(str, shape))}] window {WINDOW} {str(dtype).split('.')[-1]}: {t:.2f} ms (range {min(times):.2f} .. "
                         f"{max(times):.2f} over {REPEATS} after {WARMUP} warm-ups), {t * 1e3 / voxels:.3f} us per voxel, {voxels / t / 1e3:.2f} M voxels/s; "
                         f"median sigma {float(sigma.median()):.4f}, RMSE out / in {ratio:.3f}, unconverged {int((rank == -2).sum())}")
        sub = np.ascontiguousarray(noisy[:, :5, :32, :32])
        t0 = time.perf_counter()
        P.mppca(sub, WINDOW)
        cpu = time.perf_counter() - t0
        lines.append(f"[{M}, {', '.join(map(str, shape))}] window {WINDOW} float64 restatement on the CPU (numpy, eigh per voxel): {cpu:.2f} s for the "
                     f"1/64 sub-volume [{M}, 5, 32, 32] -> {64 * cpu:.0f} s scaled to the stack")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
