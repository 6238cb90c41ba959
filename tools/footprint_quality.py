"""GPU box: what the footprint forward model does to the quality of a fit of block-mean data:
    python tools/footprint_quality.py
tests/golden/pat07_volume.npz, ROI 40:90, all slices; fit_volume(lr_model="average") with footprint None and "box", seeds 0-2, the
default network and steps; beside them the spline baseline (baselines.rescale of the block means, x2) under the same scores."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mri_super_resolution_amd import baselines, drivers, metrics  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vol = np.load(os.path.join(ROOT, "tests", "golden", "pat07_volume.npz"))["vol"][40:90, 40:90].astype(np.float32)
vol = vol / vol.max()
hr = torch.from_numpy(vol).cuda().permute(2, 0, 1).contiguous()                      # [Z, X, Y]
lr = hr.reshape(hr.shape[0], 25, 2, 25, 2).mean(dim=(2, 4)).contiguous()
sp = baselines.rescale(lr, 2)
ok = hr.amax(dim=(-2, -1)) > 0
ssim = metrics.ssim_reference_protocol(hr[ok].contiguous(), sp[ok].contiguous().clamp_min(1e-30))
print(f"rescale baseline: psnr_db {float(metrics.psnr(hr, sp, 1.0)):.3f} ssim_mean {float(ssim.mean()):.4f}", flush=True)
for footprint in (None, "box"):
    rows = []
    for seed in (0, 1, 2):
        r = drivers.fit_volume(vol, seed=seed, lr_model="average", footprint=footprint, return_recon=False)
        rows.append((r["psnr_db"], r["ssim_mean"], r["lr_consistency_psnr_db"]))
        print(f"footprint {footprint} seed {seed}: psnr_db {r['psnr_db']:.3f} ssim_mean {r['ssim_mean']:.4f} lr_consistency_psnr_db "
              f"{r['lr_consistency_psnr_db']:.3f} final_loss {r['final_loss']:.3e} t_fit {r['t_fit']:.2f} s status {r['status']}", flush=True)
    a = np.array(rows)
    print(f"footprint {footprint}: mean psnr_db {a[:, 0].mean():.3f} (min {a[:, 0].min():.3f}, max {a[:, 0].max():.3f}), ssim_mean "
          f"{a[:, 1].mean():.4f} (min {a[:, 1].min():.4f}, max {a[:, 1].max():.4f}), lr_consistency_psnr_db {a[:, 2].mean():.3f}", flush=True)
