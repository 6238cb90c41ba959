#!/usr/bin/env python3
"""Time the registration kernels (registration.register_dataset, csrc/register.hip) on PROBA-V-sized sets, beside the CPU route the
reference takes for the shift (scipy.ndimage.shift, one core) -- the masked correlation has no CPU counterpart here (scikit-image
is not installed).

    python tools/register_time.py [output file]      # prints and writes profiles/register_time.txt (or the file named)

Sets of 128 x 128 x 19 images (smoothed noise, planted integer shifts, two masked blocks per image), full search (|d| <= 127) and a
window of 8; medians of host-timed synchronised calls on device tensors.  Not gated; the figures are what a run recorded."""
import os
import statistics
import sys
import time

import numpy as np
import scipy.ndimage as ndi
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mri_super_resolution_amd import registration  # noqa: E402


def median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def make_sets(n_sets, side=128, T=19, seed=0):
    rng = np.random.default_rng(seed)
    X, M, planted = [], [], []
    for _ in range(n_sets):
        big = 4.0 + ndi.gaussian_filter(rng.standard_normal((side + 16, side + 16)), 1.5, mode="wrap") * 4
        s = rng.integers(-4, 5, (T, 2))
        imgs = np.stack([big[8 + a:8 + a + side, 8 + b:8 + b + side] + 0.02 * rng.standard_normal((side, side)) for a, b in s], axis=-1)
        m = np.ones((side, side, T))
        for t in range(T):
            for _ in range(2):
                r, c = rng.integers(0, side - 24, 2)
                m[r:r + 8 + t, c:c + 16, t] = 0
        X.append(imgs.astype(np.float32))
        M.append(m.astype(np.float32))
        planted.append(s)
    return X, M, planted


def main(argv):
    out = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "register_time.txt")
    lines = [f"device {torch.cuda.get_device_name(0)}; sets of 128 x 128 x 19, fp32 device tensors in and out; medians of 5 synchronised "
             "calls after 2 warm-ups, host timer"]
    for n_sets in (1, 8):
        X, M, planted = make_sets(n_sets)
        Xd, Md = [torch.from_numpy(x).cuda() for x in X], [torch.from_numpy(m).cuda() for m in M]
        for max_shift in (None, 8):
            ms = median_ms(lambda: registration.register_dataset(Xd, Md, max_shift=max_shift), 2, 5)
            _, _, shifts = registration.register_dataset(Xd, Md, max_shift=max_shift, return_shifts=True)
            best = [int(np.argmax(m.mean(axis=(0, 1)))) for m in M]
            ok = all(np.array_equal(shifts[i].cpu().numpy(), planted[i] - planted[i][best[i]]) for i in range(n_sets))
            lines.append(f"{n_sets} set(s), max_shift {max_shift}: register_dataset {ms:9.2f} ms  ({ms / n_sets:8.2f} ms per set); "
                         f"planted shifts found: {ok}")
    x, m = X[0].astype(np.float64), M[0].astype(np.float64)
    t0 = time.perf_counter()
    for t in range(x.shape[-1]):
        ndi.shift(x[..., t], (1.0, -2.0), mode="reflect")
        ndi.shift(m[..., t], (1.0, -2.0), mode="constant", cval=0)
    lines.append(f"scipy.ndimage.shift of one set's 19 images and 19 masks on one CPU core: {(time.perf_counter() - t0) * 1e3:.2f} ms")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv)
