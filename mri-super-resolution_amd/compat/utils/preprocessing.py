"""``utils/preprocessing.py`` of the reference, the part a model comparison needs: ``bicubic`` (preprocessing.py:271-294), the
multi-image tree's own interpolation baseline.  The rest of that file prepares the PROBA-V data set and is not provided."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _bootstrap  # noqa: F401,E402
from mri_super_resolution_amd import baselines  # noqa: E402


def bicubic(X, scale=3):
    """``rescale(lr, scale, order=3, mode='edge', anti_aliasing=False, multichannel=True, preserve_range=True)`` of every item of
    ``X`` [B, H, W, T] (or one item [H, W, T]) on the device: float64 [B, scale H, scale W, T], each item clipped to the range of
    its own T channels, as skimage clips one call."""
    X = np.asarray(X)
    if X.ndim == 3:
        X = X[None]
    if X.ndim != 4:
        raise ValueError(f"bicubic: X must be [B, H, W, T] or [H, W, T] (got {X.ndim} axes)")
    out_hw = (X.shape[1] * scale, X.shape[2] * scale)
    planes = np.ascontiguousarray(np.moveaxis(X, -1, 1))                                   # [B, T, H, W]
    up = baselines._resize("bicubic", planes, out_hw, 3, "edge", False, True, group_axes=1)
    return np.ascontiguousarray(np.moveaxis(up, 1, -1))
