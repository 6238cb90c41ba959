"""``utils/preprocessing.py`` of the reference on the device path: ``bicubic`` (preprocessing.py:271-294), the multi-image tree's own
interpolation baseline, and the preparation of the PROBA-V data set -- ``register_dataset`` / ``register_imgset`` (:115-161, with
``masked_register_translation`` and ``shift``, which they call), ``select_T_images`` (:165-216), ``sub_images`` / ``gen_sub``
(:218-269) and ``augment_dataset`` / ``augment_imgset`` (:62-111), all from ``mri_super_resolution_amd.registration``.
``register_imgset`` returns the REGISTERED images: the vendored copy returns its input (:161) and never imports
``masked_register_translation`` (:15 is commented out), see that module.  ``load_dataset`` (:19-58) is a name that raises."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _bootstrap  # noqa: F401,E402
from mri_super_resolution_amd import baselines  # noqa: E402
from mri_super_resolution_amd.registration import (augment_dataset, augment_imgset, gen_sub, masked_register_translation,  # noqa: E402,F401
                                                   register_dataset, register_imgset, select_T_images, shift, sub_images)


def load_dataset(base_dir, part, band):
    """preprocessing.py:19-58 reads the PROBA-V PNG trees through ``cv2``: neither OpenCV nor the data set is part of this build.
    The name exists so that ``from utils.preprocessing import load_dataset`` resolves; calling it says why nothing is read."""
    raise NotImplementedError("load_dataset: reading the PROBA-V PNG trees (cv2.imread) is outside this build's scope; load "
                              f"'{base_dir}/{part}/{band}' into [H, W, T] arrays yourself and pass them to register_dataset")


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
