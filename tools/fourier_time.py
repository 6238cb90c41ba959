#!/usr/bin/env python3
"""Time Fourier re-sampling (baselines.fourier_resize, csrc/fourier.hip) on batches of 1,000 images.

    python tools/fourier_time.py [output file]      # prints and writes profiles/fourier_time.txt (or the file named)

25 x 25 -> 50 x 50 (the driver's ROI), 128 x 128 -> 256 x 256 (zero-fill of whole slices) and 128 x 128 -> 64 x 64 (k-space
truncation), fp64 and fp32 device tensors, align 'sample', mirrored boundary, no window.  Per shape: the time per batch from device
events around a window of calls after warm-up (workspace allocation, both operator launches and both apply launches are in),
the median of 5 windows, and the rate the two GEMMs' 2 (n h w ow + n oh h ow) floating-point operations give over that time -- a
whole-call rate, not a kernel's share of peak.  Not gated; the figures are what a run recorded."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mri_super_resolution_amd import baselines  # noqa: E402

N_IMAGES = 1000
SHAPES = (((25, 25), (50, 50)), ((128, 128), (256, 256)), ((128, 128), (64, 64)))


def batch_ms(fn, warmup=3, calls=20, windows=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / calls)
    return statistics.median(times), min(times), max(times)


def main(argv):
    out = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "fourier_time.txt")
    lines = [f"device {torch.cuda.get_device_name(0)}; fourier_resize of {N_IMAGES} images, align 'sample', boundary 'mirror', no window; "
             "device events around 20 calls after 3 warm-ups, median (min .. max) of 5 windows"]
    for (h, w), (oh, ow) in SHAPES:
        flop = 2.0 * N_IMAGES * (h * w * ow + oh * h * ow)
        for dtype in (torch.float64, torch.float32):
            x = torch.rand((N_IMAGES, h, w), dtype=dtype, device="cuda")
            med, lo, hi = batch_ms(lambda: baselines.fourier_resize(x, (oh, ow)))
            lines.append(f"{h} x {w} -> {oh} x {ow} {str(dtype).split('.')[-1]}: {med:8.3f} ms per batch ({lo:.3f} .. {hi:.3f}); "
                         f"{flop / med / 1e9:7.2f} TFLOP/s fp64 over the whole call")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv)
