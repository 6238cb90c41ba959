"""GPU box: what Gibbs-ringing removal does to the acquisition-model study:
    python tools/degibbs_study.py [--out profiles/degibbs_study.txt]
tests/golden/pat07_volume.npz divided by its maximum, ROI 40:90, slices 10 / 14 / 18, LR slices by k-space truncation x2 (25 x 25),
noise 0.02 and 0, seed 0, the committed TV defaults: ``drivers.acquisition_model_study(..., with_degibbs=True)``, mean PSNR (dB) and
SSIM of the three slices per method, and the mean |shift| the LR slices were given.  The figures are stated as found."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SLICES = (10, 14, 18)


def main():
    import numpy as np

    from mri_super_resolution_amd import denoise, drivers

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "degibbs_study.txt"))
    args = ap.parse_args()
    vol = np.load(os.path.join(ROOT, "tests", "golden", "pat07_volume.npz"))["vol"].astype(np.float64)
    vol = vol / vol.max()
    slices = np.ascontiguousarray(vol[40:90, 40:90].transpose(2, 0, 1))[list(SLICES)]
    lines = []
    for model in ("kspace", "gaussian"):
        for noise in (0.02, 0.0):
            res = drivers.acquisition_model_study(slices, model, 2, None, None, noise, 0, slice_ids=list(SLICES), with_degibbs=True)
            shift = denoise.degibbs(res["lr"], return_info=True)[1]["shift"]
            row = ", ".join(f"{name} {res['psnr'][name].mean():.2f} / {res['ssim'][name].mean():.3f}" for name in res["methods"])
            lines.append(f"pat07 ROI 40:90 slices {SLICES} x2 model {model} noise {noise}: {row}; mean |shift| {float(shift.abs().mean()):.3f} px")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
