"""GPU box: the time of Gibbs-ringing removal on whole stacks:
    python tools/degibbs_time.py [--out profiles/degibbs_time.txt]
A [16, 20, 128, 128] and a [40, 20, 128, 128] stack (320 and 800 images of 128 x 128: the truncated phantom of tests/degibbs_common.py
scaled per image, noise 0.02, seed 0), nshifts 20, window (1, 3), through ``denoise.degibbs`` on device tensors, fp64 and fp32: device
events around the call (outputs and the workspace allocated by the wrapper inside the window, as a caller pays for them), a stream
synchronisation before the first event and on the second, 3 warm-up calls, then the median of 10 with the range; beside it the rate
against the arithmetic of the method (80 circulant products of the 64 / 54 halo tiles and the 12 DFT products of the split, 0.45 GFLOP
per image).  Beside each stack the float64 restatement (tests/degibbs_common.py, the np.fft path) on this box's CPU, timed on 1/16 of
the images and scaled by 16.  Nothing here has a target: the figures are stated as found."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STACKS = ((16, 20, 128, 128), (40, 20, 128, 128))
WARMUP, REPEATS = 3, 10


def flop_per_image(H, W, nshifts=20, own=54):
    tiles = lambda n: -(-n // own)
    lines = 2 * nshifts * 2 * 64 * (tiles(W) * H * W + tiles(H) * W * H)          # both passes: 64 computed columns per tile, K = n
    split = 2 * (H * 2 * W * W + 2 * (2 * H) * (2 * H) * W + H * W * 2 * W)
    return lines + split


def main():
    import numpy as np
    import torch

    from mri_super_resolution_amd import denoise
    from tests import degibbs_common as G

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "degibbs_time.txt"))
    args = ap.parse_args()
    lines = []
    for shape in STACKS:
        rng = np.random.default_rng(0)
        n = shape[0] * shape[1]
        base = G.trunc(G.phantom(128, 128), 128, 128)
        stack = ((1 + 0.5 * rng.random((n, 1, 1))) * base + 0.02 * rng.standard_normal((n, 128, 128))).reshape(shape)
        gflop = n * flop_per_image(128, 128) / 1e9
        for dtype in (torch.float64, torch.float32):
            x = torch.from_numpy(stack).to("cuda", dtype)
            for _ in range(WARMUP):
                denoise.degibbs(x)
            times = []
            for _ in range(REPEATS):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                start.record()
                out = denoise.degibbs(x)
                end.record()
                end.synchronize()
                times.append(start.elapsed_time(end))
            t = float(np.median(times))
            lines.append(f"{list(shape)} nshifts 20 window (1, 3) {str(dtype).split('.')[-1]}: {t:.2f} ms (range {min(times):.2f} .. {max(times):.2f} "
                         f"over {REPEATS} after {WARMUP} warm-ups), {t * 1e3 / n:.1f} us per image, {gflop:.0f} GFLOP fp64 -> {gflop / t:.1f} TFLOP/s")
        sub = stack.reshape(n, 128, 128)[:n // 16]
        t0 = time.perf_counter()
        ref = G.degibbs2d(sub)[0]
        cpu = time.perf_counter() - t0
        dev = denoise.degibbs(sub)
        lines.append(f"{list(shape)} float64 restatement on the CPU (numpy, np.fft path): {cpu:.2f} s for 1/16 of the images -> {16 * cpu:.0f} s scaled "
                     f"to the stack; max |device - restatement| on them {np.abs(dev - ref).max():.2e}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
