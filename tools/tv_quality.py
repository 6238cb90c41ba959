"""GPU box: the TV / Huber model-based baseline beside the rows of tools/footprint_quality.py:
    python tools/tv_quality.py
tests/golden/pat07_volume.npz, ROI 40:90, all slices, fp32 on the device as the driver holds them; LR = 2 x 2 block means (the table of
4k) and LR = every second pixel (the driver's default); block replication, the interpolation baseline of each model, and
baselines.tv_superres at the driver's defaults and at the two settings of the CPU prototype.  Then one timing of the default solve:
device events around windows of 200 calls after 3 warm-up calls, median of 5 windows; there is no predecessor to compare with."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mri_super_resolution_amd import baselines, metrics  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vol = np.load(os.path.join(ROOT, "tests", "golden", "pat07_volume.npz"))["vol"][40:90, 40:90].astype(np.float32)
vol = vol / vol.max()
hr = torch.from_numpy(vol).cuda().permute(2, 0, 1).contiguous()                      # [Z, X, Y]
ok = hr.amax(dim=(-2, -1)) > 0


def score(name, img):
    ssim = metrics.ssim_reference_protocol(hr[ok].contiguous(), img[ok].contiguous().clamp_min(1e-30))
    print(f"{name}: psnr_db {float(metrics.psnr(hr, img, 1.0)):.3f} ssim_mean {float(ssim.mean()):.4f}", flush=True)


D = (baselines.TV_DEFAULT_LAMBDA, baselines.TV_DEFAULT_HUBER, baselines.TV_DEFAULT_ITERS)
SETTINGS = (("defaults", *D), ("plain TV", 1e-3, 0.0, 1000), ("Huber", 1e-3, 0.1, 500))
for kernel, lr in (("mean", hr.reshape(hr.shape[0], 25, 2, 25, 2).mean(dim=(2, 4)).contiguous()), ("decimate", hr[:, ::2, ::2].contiguous())):
    print(f"LR model: {kernel}", flush=True)
    score("  block replication", lr.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1))
    if kernel == "mean":
        score("  rescale of the block means", baselines.rescale(lr, 2))
    else:
        score("  rescale of every second pixel", baselines.rescale(lr, 2))
        score("  zero-fill (fourier_resize, sample, mirror)", baselines.fourier_resize(lr, (50, 50), "sample", "mirror", 0.0).clamp_min(0))
    for name, lam, alpha, n_iter in SETTINGS:
        tv, info = baselines.tv_superres(lr, (2, 2), kernel, lam, alpha, n_iter, return_info=True)
        consistency = float(metrics.psnr(lr, baselines.block_apply(tv, (2, 2), kernel), 1.0))
        score(f"  tv_superres {name} (lambda {lam:g}, huber {alpha:g}, {n_iter} iterations; consistency {consistency:.2f} dB, "
              f"max change {float(info['change'].max()):.2e})", tv)
    for _ in range(3):
        baselines.tv_superres(lr, (2, 2), kernel, *D)
    windows = []
    for _ in range(5):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(200):
            baselines.tv_superres(lr, (2, 2), kernel, *D)
        end.record()
        end.synchronize()
        windows.append(start.elapsed_time(end) / 200)
    print(f"  time of one default solve, {lr.shape[0]} images of 50 x 50 in one launch ({D[2]} iterations; includes the wrapper's "
          f"allocations): median {np.median(windows):.3f} ms (windows {', '.join(f'{w:.3f}' for w in windows)})", flush=True)
