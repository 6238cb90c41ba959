"""CPU: the sweep behind the defaults of baselines.tv_superres_operator / scripts/acquisition_model:
    python tools/tvop_sweep.py
The float64 restatement (tests/tvop_common.py) on tests/golden/pat07_volume.npz, ROI 40:90 divided by its maximum, slices 10 / 14 / 18,
x2 (50 -> 25): the LR slices made by k-space truncation (fourier_common.restated_operator, 'center' / 'mirror') and by a Gaussian PSF of
FWHM 1.2 LR pixels (tvop_common.psf_operator), without noise and with noise 0.02 (slice z draws from default_rng(1000 seed + z), seed
0, as the study does); 500 iterations from the default start with the operator that made the data; PSNR over the whole ROI per
(lambda, alpha), then the iteration count at the pair chosen for noise 0.02.  The method of tools/tv_sweep.py: a coarse grid, then past
its edge where the best sits on it.  No other column -- not the spline, not zero-filling, not the block solver -- is ever looked at."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import fourier_common as F  # noqa: E402
from tests import tvop_common as C  # noqa: E402

GRID = [(lam, alpha) for lam in (3e-4, 1e-3, 3e-3, 1e-2, 3e-2) for alpha in (0.0, 0.01, 0.03, 0.1, 0.3)]
ITERS = (100, 300, 500, 1000, 3000)
SLICES, SEED = (10, 14, 18), 0

hr = C.pat07_roi(40, 90)[list(SLICES)]
fourier = F.restated_operator(50, 25, "center", "mirror", 0.0)
gauss = C.psf_operator(50, 25, 1.2)
MODELS = {"kspace": (fourier, fourier), "gaussian": (gauss, gauss)}


def data(model, noise):
    eta = np.stack([noise * np.random.default_rng(SEED * 1000 + z).standard_normal((25, 25)) for z in SLICES])
    return C.apply(hr, *MODELS[model]) + eta


def score(model, y, lam, alpha, n_iter):
    x = C.solve(y, *MODELS[model], lam, alpha, n_iter)
    return [C.psnr(a, b) for a, b in zip(hr, x)]


table = {}
for model in MODELS:
    for noise in (0.0, 0.02):
        y = data(model, noise)
        best = None
        for lam, alpha in GRID:
            s = score(model, y, lam, alpha, 500)
            table[(model, noise, lam, alpha)] = float(np.mean(s))
            print(f"{model} noise {noise:g} lambda {lam:g} alpha {alpha:g}: " + " ".join(f"{v:.3f}" for v in s) + f"  mean {np.mean(s):.3f}", flush=True)
            if best is None or np.mean(s) > best[0]:
                best = (float(np.mean(s)), lam, alpha)
        print(f"{model} noise {noise:g}: best of the grid lambda {best[1]:g} alpha {best[2]:g}, mean {best[0]:.3f} dB", flush=True)
# one pair for both models at noise 0.02: the largest of the smaller mean of the two
both = max(GRID, key=lambda g: min(table[("kspace", 0.02) + g], table[("gaussian", 0.02) + g]))
print(f"noise 0.02, both models: lambda {both[0]:g} alpha {both[1]:g} (kspace {table[('kspace', 0.02) + both]:.3f}, gaussian "
      f"{table[('gaussian', 0.02) + both]:.3f} dB)", flush=True)
for model in MODELS:
    y = data(model, 0.02)
    for n in ITERS:
        s = score(model, y, both[0], both[1], n)
        print(f"{model} noise 0.02 lambda {both[0]:g} alpha {both[1]:g} iterations {n}: " + " ".join(f"{v:.3f}" for v in s) + f"  mean {np.mean(s):.3f}",
              flush=True)
