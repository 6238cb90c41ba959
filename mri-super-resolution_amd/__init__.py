"""mri-super-resolution_amd -- MI355X (gfx950) implementation of the INR / SIREN super-resolution
fit path of MRIRC/MRI-super-resolution.

The directory name carries a hyphen (it is the project name), so import it through the alias package
``mri_super_resolution_amd`` at the repo root, or put ``mri-super-resolution_amd/compat`` on
``sys.path`` to get drop-in ``SRDWI`` / ``INRmodel`` / ``nn_mri`` modules for the reference's drivers.

Layout:  csrc/ (HIP kernels + C ABI, built into libinrhip.so) . _lib.py (ctypes binding) . ops.py
(tensor wrappers) . flat.py (flat parameter buffer, workspaces and Adam state of every fitter) . inr.py (reference module surface + fused fit / reconstruct) . metrics.py . baselines.py (spline
rescale) . drivers.py (the reference's driver loops) . dist.py (fit partitioning over GPUs, metric gather) . matio.py
(.mat level 5) . reports.py (CSV schemas) . contrast.py (case / calculate_contrast) . wire.py (the complex-Gabor WIRE network and
its fitter) . footprint.py (the voxel-footprint forward model of a SIREN fit) . registration.py (masked registration and the multi-image data preparation) . scripts/ (superresDWI, master).
"""
from ._lib import InrHipError, InrHipUnavailable  # noqa: F401
from .ops import InrDeviceError  # noqa: F401
from .inr import (Derivatives, ImageFitting_set, PN, ShardedSirenFitter, SineLayer, Siren, SirenFitter, calculate_ADC,  # noqa: F401
                  calculate_combinations, derivatives, divergence, fit_cycle_batch, fit_siren, flat_parameters, get_mgrid,
                  gradient, input_mapping, laplace, reconstruct, resize_array)
from .footprint import Footprint, FootprintSirenFitter, footprint_forward, footprint_inputs  # noqa: F401

__all__ = ["Derivatives", "derivatives", "divergence", "gradient", "laplace", "ImageFitting_set", "PN", "ShardedSirenFitter", "SineLayer", "Siren", "SirenFitter", "calculate_ADC",
           "calculate_combinations", "fit_cycle_batch", "fit_siren", "flat_parameters", "get_mgrid", "input_mapping",
           "reconstruct", "resize_array", "InrHipError", "InrHipUnavailable", "InrDeviceError", "Footprint", "FootprintSirenFitter",
           "footprint_forward", "footprint_inputs"]
