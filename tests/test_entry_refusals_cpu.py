"""What the C entry points of the metric, re-sampling, perceptual, AutoERD, hybrid-fit, RAMS and small layer-op families answer to
a bad call: the status and the full inr_last_error() text, and what their workspace planners return at a small fixed shape and at
an out-of-range one.  Every call is refused in validation, before any device work, so the file needs no GPU; pointers are fake
addresses that are never dereferenced (ODD: low bits set, for the alignment rows).  The expected strings and values are literals,
recorded from the library as it was before the entry points moved into the units that own their kernels: the Python layer and its
callers match on them."""
import ctypes as C

import pytest

from mri_super_resolution_amd import _lib
from mri_super_resolution_amd._lib import RamsDesc, shape_array

P = lambda k: 0x7000_0000_0000 + 4096 * k      # never dereferenced
ODD = lambda k: P(k) + 8                        # not 16-byte aligned
SHAPE = shape_array((4, 4))
RAMS = C.byref(RamsDesc(3, 32, 3, 9, 8, 2, 0.0, 1.0))
RAMS_BAD = C.byref(RamsDesc(3, 16, 3, 9, 8, 2, 0.0, 1.0))      # 16 filters
RAMS_CH8 = C.byref(RamsDesc(3, 32, 3, 8, 8, 2, 0.0, 1.0))      # a temporal depth of 4 before the head
K9 = (C.c_double * 9)()
W5 = (C.c_double * 5)(0.2, 0.2, 0.2, 0.2, 0.2)
GROUPS = (C.c_int * 2)(3, 3)
GROUPS_SHORT = (C.c_int * 2)(3, 2)
OFFS = (C.c_int64 * 512)()
BIG = 1 << 40

# (entry point, arguments, status, inr_last_error())
REFUSALS = [
    # ---- kernels.hip
    ("inr_mgrid", (None, None, 2, 0, 4, None), -1, "inr_mgrid: null pointer"),
    ("inr_mgrid", (P(1), SHAPE, 2, -1, 4, None), -1, "inr_mgrid: negative row range"),
    ("inr_fourier_map", (P(1), None, P(3), 4, 2, 8, None), -1, "inr_fourier_map: null pointer"),
    ("inr_fourier_map", (P(1), P(2), P(3), -1, 2, 8, None), -1, "inr_fourier_map: bad sizes n=-1 d=2 m=8"),
    ("inr_grid_fourier_map", (P(1), SHAPE, 2, 0, 4, None, 8, None), -1, "inr_grid_fourier_map: null pointer"),
    ("inr_grid_fourier_map", (P(1), SHAPE, 2, 0, 4, P(2), 0, None), -1, "inr_grid_fourier_map: bad sizes"),
    ("inr_linear_head_forward", (P(1), P(2), None, None, 4, 8, 1, 0, 0.0, None), -1, "inr_linear_head_forward: null pointer"),
    ("inr_linear_head_forward", (P(1), P(2), P(3), None, 4, 0, 1, 0, 0.0, None), -1, "inr_linear_head_forward: bad sizes"),
    ("inr_linear_tanh_head_forward", (None, None, P(2), P(3), None, 4, 8, 1, 1.0, None), -1, "inr_linear_tanh_head_forward: null pointer"),
    ("inr_linear_tanh_head_forward", (P(1), None, P(2), P(3), None, -1, 8, 1, 1.0, None), -1, "inr_linear_tanh_head_forward: bad sizes"),
    ("inr_mse_loss_grad", (P(1), None, P(3), P(4), None, 16, P(5), 1 << 20, None), -1, "inr_mse_loss_grad: null pointer"),
    ("inr_mse_loss_grad", (P(1), P(2), P(3), P(4), None, 0, P(5), 1 << 20, None), -1, "inr_mse_loss_grad: count must be >= 1"),
    ("inr_mse_loss_grad", (P(1), P(2), P(3), P(4), None, 5000, None, 1 << 20, None), -2, "inr_mse_loss_grad: workspace too small"),
    ("inr_mse_loss_grad", (P(1), P(2), P(3), P(4), None, 5000, P(5), 8, None), -2, "inr_mse_loss_grad: workspace too small"),
    ("inr_adam_step", (None, None, None, None, 4, 1, 1e-4, 0.9, 0.999, 1e-8, None), -1, "inr_adam_step: null pointer"),
    ("inr_adam_step", (P(1), P(2), P(3), P(4), 4, 0, 1e-4, 0.9, 0.999, 1e-8, None), -1, "inr_adam_step: count >= 0 and step >= 1 required"),
    ("inr_adam_step", (P(1), P(2), P(3), P(4), -1, 1, 1e-4, 0.9, 0.999, 1e-8, None), -1, "inr_adam_step: count >= 0 and step >= 1 required"),
    ("inr_mul", (P(1), P(2), None, 4, None), -1, "inr_mul: bad arguments"),
    ("inr_mul", (P(1), P(2), P(3), -4, None), -1, "inr_mul: bad arguments"),
    ("inr_acquisition_products", (P(1), P(2), P(3), P(4), None, 8, 2, 2, 2, None), -1, "inr_acquisition_products: null pointer"),
    ("inr_acquisition_products", (P(1), P(2), P(3), P(4), P(5), 8, 0, 2, 2, None), -1, "inr_acquisition_products: bad sizes"),
    ("inr_acquisition_products", (P(1), P(2), P(3), P(4), P(5), 8, 4096, 4096, 1, None), -1, "inr_acquisition_products: bad sizes"),
    ("inr_sincos_probe", (P(1), None, P(3), 4, None), -1, "inr_sincos_probe: bad arguments"),
    ("inr_sincos_probe", (P(1), P(2), P(3), -1, None), -1, "inr_sincos_probe: bad arguments"),
    # ---- gemm_f32.hip
    ("inr_sine_layer_forward", (None, None, P(2), P(3), None, 4, 8, 8, 30.0, None), -1, "inr_sine_layer_forward: null pointer"),
    ("inr_sine_layer_forward", (P(1), None, P(2), P(3), None, -1, 8, 0, 30.0, None), -1, "inr_sine_layer_forward: bad sizes n=-1 in=8 out=0"),
    ("inr_sine_layer_forward", (P(1), None, P(2), P(3), None, 1 << 31, 8, 8, 30.0, None), -1, "inr_sine_layer_forward: bad sizes n=2147483648 in=8 out=8"),
    ("inr_tanh_layer_forward", (P(1), None, None, P(3), None, 4, 8, 8, 1.0, None), -1, "inr_tanh_layer_forward: null pointer"),
    ("inr_tanh_layer_forward", (P(1), None, P(2), P(3), None, 4, 0, 8, 1.0, None), -1, "inr_tanh_layer_forward: bad sizes"),
    # ---- metrics.hip
    ("inr_psnr", (None, P(2), P(3), 2, 100, 1.0, P(4), 1 << 20, None), -1, "inr_psnr: null pointer"),
    ("inr_psnr", (P(1), P(2), P(3), 0, 100, 1.0, P(4), 1 << 20, None), -1, "inr_psnr: bad sizes"),
    ("inr_psnr", (P(1), P(2), P(3), 2, 100, 0.0, P(4), 1 << 20, None), -1, "inr_psnr: bad sizes"),
    ("inr_psnr", (P(1), P(2), P(3), 2, 100, 1.0, None, 1 << 20, None), -2, "inr_psnr: workspace too small"),
    ("inr_psnr", (P(1), P(2), P(3), 2, 100, 1.0, P(4), 1023, None), -2, "inr_psnr: workspace too small"),
    ("inr_ssim2d", (P(1), None, P(3), 2, 32, 32, 7, 1.0, 0, 0.0, P(4), 1 << 20, None), -1, "inr_ssim2d: null pointer"),
    ("inr_ssim2d", (P(1), P(2), P(3), 2, 32, 30, 6, 1.0, 0, 0.0, P(4), 1 << 20, None), -1, "inr_ssim2d: need odd win >= 3 and images at least win x win (got 32x30, win 6)"),
    ("inr_ssim2d", (P(1), P(2), P(3), 2, 5, 32, 7, 1.0, 0, 0.0, P(4), 1 << 20, None), -1, "inr_ssim2d: need odd win >= 3 and images at least win x win (got 5x32, win 7)"),
    ("inr_ssim2d", (P(1), P(2), P(3), 2, 32, 32, 7, 1.0, 0, 0.0, P(4), 1023, None), -2, "inr_ssim2d: workspace too small"),
    ("inr_rams_shift_loss", (P(1), P(2), P(3), None, 2, 32, 3, 0, P(4), 1 << 20, None), -1, "inr_rams_shift_loss: null pointer"),
    ("inr_rams_shift_loss", (P(1), P(2), P(3), P(4), 2, 6, 3, 0, P(5), 1 << 20, None), -1, "inr_rams_shift_loss: bad arguments (size=6 border=3 mode=0)"),
    ("inr_rams_shift_loss", (P(1), P(2), P(3), P(4), 2, 32, 3, 2, P(5), 1 << 20, None), -1, "inr_rams_shift_loss: bad arguments (size=32 border=3 mode=2)"),
    ("inr_rams_shift_loss", (P(1), P(2), P(3), P(4), 2, 32, 3, 0, P(5), 783, None), -2, "inr_rams_shift_loss: workspace too small"),
    ("inr_rams_shift_loss", (P(1), P(2), P(3), P(4), 2, 32, 3, 0, None, 1 << 20, None), -2, "inr_rams_shift_loss: workspace too small"),
    ("inr_rams_shift_loss_grad", (None, P(2), P(3), P(4), P(5), None, 2, 32, 3, P(6), 1 << 20, None), -1, "inr_rams_shift_loss_grad: null pointer"),
    ("inr_rams_shift_loss_grad", (P(1), P(2), P(3), P(4), P(5), None, 2, 32, 17, P(6), 1 << 20, None), -1, "inr_rams_shift_loss_grad: bad arguments (size=32 border=17)"),
    ("inr_rams_shift_loss_grad", (P(1), P(2), P(3), P(4), P(5), None, 2, 32, 3, P(6), 799, None), -2, "inr_rams_shift_loss_grad: workspace too small"),
    ("inr_rams_shift_loss_grad", (P(1), P(2), P(3), P(4), P(5), None, 2, 32, 3, P(6) + 4, 1 << 20, None), -3, "inr_rams_shift_loss_grad: workspace must be 8-byte aligned"),
    ("inr_adc_map", (P(1), None, P(3), 16, 4, None), -1, "inr_adc_map: null pointer"),
    ("inr_adc_map", (P(1), P(2), P(3), 16, 1, None), -1, "inr_adc_map: need 2 <= n_b <= 32"),
    ("inr_adc_map", (P(1), P(2), P(3), 16, 33, None), -1, "inr_adc_map: need 2 <= n_b <= 32"),
    ("inr_rescale2d_linear", (None, P(2), 2, 8, 8, 16, 16, None), -1, "inr_rescale2d_linear: null pointer"),
    ("inr_rescale2d_linear", (P(1), P(2), 2, 8, 0, 16, 16, None), -1, "inr_rescale2d_linear: bad sizes"),
    ("inr_rescale2d_linear", (P(1), P(2), 2, 65536, 65536, 16, 16, None), -1, "inr_rescale2d_linear: image too large"),
    ("inr_resize_z_cubic", (P(1), None, 10, 8, 16, P(3), 1 << 20, None), -1, "inr_resize_z_cubic: null pointer"),
    ("inr_resize_z_cubic", (P(1), P(2), 0, 8, 16, P(3), 1 << 20, None), -1, "inr_resize_z_cubic: bad sizes (n_lines=0, n_in=8, n_out=16)"),
    ("inr_resize_z_cubic", (P(1), P(2), 10, 3, 16, P(3), 1 << 20, None), -1, "inr_resize_z_cubic: a not-a-knot cubic spline needs at least 4 samples per line (got 3)"),
    ("inr_resize_z_cubic", (P(1), P(2), 10, 8, 16, P(3), 639, None), -2, "inr_resize_z_cubic: workspace too small"),
    ("inr_resize_z_cubic", (P(1), P(2), 10, 8, 16, None, 1 << 20, None), -2, "inr_resize_z_cubic: workspace too small"),
    ("inr_resize_z_cubic", (P(1), P(2), 10, 9000, 16, P(3), 1 << 20, None), -1, "inr_resize_z_cubic: 4 to 8192 samples per line (got 9000)"),
    ("inr_auto_erd", (None, P(2), None, 16, 6, 1, None), -1, "inr_auto_erd: null pointer"),
    ("inr_auto_erd", (P(1), P(2), None, -1, 6, 1, None), -1, "inr_auto_erd: bad pixel count"),
    ("inr_auto_erd", (P(1), P(2), None, 16, 1, 1, None), -1, "inr_auto_erd: 2 <= acquisitions <= 32 (got 1)"),
    ("inr_auto_erd", (P(1), P(2), None, 16, 6, 3, None), -1, "inr_auto_erd: rule must be 1 (majority voting) or 2 (intensity-cognisant)"),
    # ---- cssim.hip
    ("inr_rams_shift_ssim", (P(1), None, P(3), P(4), 2, 64, 3, 0, P(5), BIG, None), -1, "inr_rams_shift_ssim: null pointer"),
    ("inr_rams_shift_ssim", (P(1), P(2), P(3), P(4), 2, 16, 3, 0, P(5), BIG, None), -1, "inr_rams_shift_ssim: bad arguments (n_images=2 size=16 border=3; size - 2*border >= 11)"),
    ("inr_rams_shift_ssim", (P(1), P(2), P(3), P(4), 0, 64, 3, 0, P(5), BIG, None), -1, "inr_rams_shift_ssim: bad arguments (n_images=0 size=64 border=3; size - 2*border >= 11)"),
    ("inr_rams_shift_ssim", (P(1), P(2), P(3), P(4), 2, 64, 3, 0, P(5), 1000, None), -2, "inr_rams_shift_ssim: workspace too small"),
    ("inr_rams_shift_ssim", (P(1), P(2), P(3), P(4), 2, 64, 3, 0, None, BIG, None), -2, "inr_rams_shift_ssim: workspace too small"),
    ("inr_rams_shift_ssim", (P(1), P(2), P(3), P(4), 2, 64, 3, 0, P(5) + 4, BIG, None), -3, "inr_rams_shift_ssim: workspace must be 8-byte aligned"),
    ("inr_rams_shift_ssim_grad", (P(1), P(2), P(3), P(4), None, None, 2, 64, 3, 0, P(6), BIG, None), -1, "inr_rams_shift_ssim_grad: null pointer"),
    ("inr_rams_shift_ssim_grad", (P(1), P(2), P(3), P(4), P(5), None, 2, 9000, 3, 0, P(6), BIG, None), -1, "inr_rams_shift_ssim_grad: bad arguments (n_images=2 size=9000 border=3; size - 2*border >= 11)"),
    ("inr_rams_shift_ssim_grad", (P(1), P(2), P(3), P(4), P(5), None, 2, 64, 3, 0, P(6), 1000, None), -2, "inr_rams_shift_ssim_grad: workspace too small"),
    ("inr_rams_shift_ssim_grad", (P(1), P(2), P(3), P(4), P(5), None, 2, 64, 3, 0, P(6) + 4, BIG, None), -3, "inr_rams_shift_ssim_grad: workspace must be 8-byte aligned"),
    # ---- rescale.hip
    ("inr_rescale2d", (P(1), None, 2, 32, 48, 16, 24, 3, 1, 1, 0, P(3), BIG, None), -1, "inr_rescale2d: null pointer"),
    ("inr_rescale2d", (P(1), P(2), 2, 32, 48, 16, 24, 2, 1, 1, 0, P(3), BIG, None), -1, "inr_rescale2d: order must be 1 or 3 (got 2)"),
    ("inr_rescale2d", (P(1), P(2), 2, 32, 48, 16, 24, 3, 2, 1, 0, P(3), BIG, None), -1, "inr_rescale2d: mode must be INR_RESCALE_REFLECT or INR_RESCALE_EDGE (got 2)"),
    ("inr_rescale2d", (P(1), P(2), 2, 32, 5000, 16, 24, 3, 1, 1, 0, P(3), BIG, None), -1, "inr_rescale2d: lines of at most 4096 samples (got 32 x 5000 -> 16 x 24)"),
    ("inr_rescale2d", (P(1), P(2), 3, 32, 48, 16, 24, 3, 1, 1, 2, P(3), BIG, None), -1, "inr_rescale2d: clip_group (2) must be 0 or divide n_images (3)"),
    ("inr_rescale2d", (P(1), P(2), 2, 4000, 48, 10, 24, 3, 1, 1, 0, P(3), BIG, None), -1, "inr_rescale2d: anti-aliasing radius beyond 64 taps (4000 x 48 -> 10 x 24)"),
    ("inr_rescale2d", (P(1), P(2), 2, 32, 48, 16, 24, 3, 1, 1, 0, None, BIG, None), -2, "inr_rescale2d: workspace too small (0 doubles, 11168 needed)"),
    ("inr_rescale2d", (P(1), P(2), 2, 32, 48, 16, 24, 3, 1, 1, 0, P(3), 100, None), -2, "inr_rescale2d: workspace too small (100 doubles, 11168 needed)"),
    ("inr_rescale2d", (P(1), P(2), 2, 32, 48, 16, 24, 3, 1, 1, 0, P(3), -1, None), -2, "inr_rescale2d: workspace too small (-1 doubles, 11168 needed)"),
    ("inr_rescale2d", (P(1), P(2), 2, 32, 48, 16, 24, 3, 1, 1, 0, ODD(3), BIG, None), -3, "inr_rescale2d: workspace must be 16-byte aligned"),
    # ---- fourier.hip
    ("inr_fourier_operator", (None, 8, 16, 0, 0, 0.0, None), -1, "inr_fourier_operator: null pointer"),
    ("inr_fourier_operator", (P(1), 8, 16, 2, 0, 0.0, None), -1, "inr_fourier_operator: align must be INR_FOURIER_SAMPLE or INR_FOURIER_CENTER (got 2)"),
    ("inr_fourier_operator", (P(1), 8, 16, 0, 2, 0.0, None), -1, "inr_fourier_operator: boundary must be INR_FOURIER_PERIODIC or INR_FOURIER_MIRROR (got 2)"),
    ("inr_fourier_operator", (P(1), 8, 16, 0, 0, 1.5, None), -1, "inr_fourier_operator: apodize must be in [0, 1] (got 1.5)"),
    ("inr_fourier_operator", (P(1), 0, 16, 0, 0, 0.0, None), -1, "inr_fourier_operator: bad sizes (a line of 0 samples to 16)"),
    ("inr_fourier_operator", (P(1), 8, 2000, 0, 0, 0.0, None), -1, "inr_fourier_operator: lines of at most 1024 samples (got 8 -> 2000)"),
    ("inr_fourier_operator", (P(1), 8, 15, 0, 1, 0.0, None), -1, "inr_fourier_operator: the mirror boundary with align 'sample' needs n >= 2 and (2n - 2) m divisible by n (got 8 -> 15)"),
    ("inr_fourier_resample2d", (P(1), None, 2, 8, 12, 16, 24, 0, 0, 0.0, P(3), BIG, None), -1, "inr_fourier_resample2d: null pointer"),
    ("inr_fourier_resample2d", (P(1), P(2), 2, 8, 12, 16, 24, 3, 0, 0.0, P(3), BIG, None), -1, "inr_fourier_resample2d: align must be INR_FOURIER_SAMPLE or INR_FOURIER_CENTER (got 3)"),
    ("inr_fourier_resample2d", (P(1), P(2), -1, 8, 12, 16, 24, 0, 0, 0.0, P(3), BIG, None), -1, "inr_fourier_resample2d: bad sizes (n_images = -1)"),
    ("inr_fourier_resample2d", (P(1), P(2), 2, 8, 12, 16, 1025, 0, 0, 0.0, P(3), BIG, None), -1, "inr_fourier_resample2d: lines of at most 1024 samples (got 12 -> 1025)"),
    ("inr_fourier_resample2d", (P(1), P(2), 2, 8, 12, 16, 24, 0, 0, 0.0, None, BIG, None), -2, "inr_fourier_resample2d: workspace too small (0 doubles, 800 needed)"),
    ("inr_fourier_resample2d", (P(1), P(2), 2, 8, 12, 16, 24, 0, 0, 0.0, P(3), 100, None), -2, "inr_fourier_resample2d: workspace too small (100 doubles, 800 needed)"),
    ("inr_fourier_resample2d", (P(1), P(2), 2, 8, 12, 16, 24, 0, 0, 0.0, ODD(3), BIG, None), -3, "inr_fourier_resample2d: workspace must be 16-byte aligned"),
    ("inr_fourier_resample2d_f32", (None, P(2), 2, 8, 12, 16, 24, 0, 0, 0.0, P(3), BIG, None), -1, "inr_fourier_resample2d_f32: null pointer"),
    ("inr_fourier_resample2d_f32", (P(1), P(2), 2, 8, 12, 16, 25, 0, 1, 0.0, P(3), BIG, None), -1, "inr_fourier_resample2d_f32: the mirror boundary with align 'sample' needs n >= 2 and (2n - 2) m divisible by n (got 12 -> 25)"),
    ("inr_fourier_resample2d_f32", (P(1), P(2), 2, 8, 12, 16, 24, 1, 1, 0.0, P(3), 100, None), -2, "inr_fourier_resample2d_f32: workspace too small (100 doubles, 800 needed)"),
    ("inr_fourier_resample2d_f32", (P(1), P(2), 2, 8, 12, 16, 24, 1, 1, 0.0, ODD(3), BIG, None), -3, "inr_fourier_resample2d_f32: workspace must be 16-byte aligned"),
    # ---- perceptual.hip
    ("inr_ssim2d_gauss", (P(1), None, None, None, P(3), 2, 40, 50, 1.5, 1.0, P(4), BIG, None), -1, "inr_ssim2d_gauss: null pointer"),
    ("inr_ssim2d_gauss", (P(1), None, None, P(2), P(3), 0, 40, 50, 1.5, 1.0, P(4), BIG, None), -1, "inr_ssim2d_gauss: 1 <= n_images <= 65535 (got 0)"),
    ("inr_ssim2d_gauss", (P(1), None, None, P(2), P(3), 2, 40, 50, 3.0, 1.0, P(4), BIG, None), -1, "inr_ssim2d_gauss: sigma must be positive with a window radius ceil(3 sigma) <= 7 (got 3)"),
    ("inr_ssim2d_gauss", (P(1), None, None, P(2), P(3), 2, 40, 50, 1.5, 0.0, P(4), BIG, None), -1, "inr_ssim2d_gauss: data_range must be positive (got 0)"),
    ("inr_ssim2d_gauss", (P(1), None, None, P(2), P(3), 2, 40, 50, 1.5, 1.0, None, BIG, None), -2, "inr_ssim2d_gauss: workspace too small (0 doubles, 320 needed)"),
    ("inr_ssim2d_gauss", (P(1), None, None, P(2), P(3), 2, 40, 50, 1.5, 1.0, P(4), 100, None), -2, "inr_ssim2d_gauss: workspace too small (100 doubles, 320 needed)"),
    ("inr_ssim2d_gauss", (P(1), None, None, P(2), P(3), 2, 40, 50, 1.5, 1.0, ODD(4), BIG, None), -3, "inr_ssim2d_gauss: workspace must be 16-byte aligned"),
    ("inr_ssim2d_gauss", (P(1), None, None, ODD(2), P(3), 2, 40, 50, 1.5, 1.0, P(4), BIG, None), -3, "inr_ssim2d_gauss: pointers must be 16-byte aligned"),
    ("inr_msssim2d", (P(1), None, P(2), P(3), 2, 40, 50, None, 5, 1.5, 1.0, P(4), BIG, None), -1, "inr_msssim2d: null pointer"),
    ("inr_msssim2d", (P(1), None, P(2), P(3), 2, 40, 50, W5, 9, 1.5, 1.0, P(4), BIG, None), -1, "inr_msssim2d: 1 <= n_scales <= 8 (got 9)"),
    ("inr_msssim2d", (P(1), None, P(2), P(3), 2, 40, 50, W5, 5, 1.5, 1.0, P(4), 100, None), -2, "inr_msssim2d: workspace too small (100 doubles, 2944 needed)"),
    ("inr_msssim2d", (P(1), None, P(2), P(3), 2, 40, 50, W5, 5, 1.5, 1.0, ODD(4), BIG, None), -3, "inr_msssim2d: workspace must be 16-byte aligned"),
    ("inr_msssim2d", (ODD(1), None, P(2), P(3), 2, 40, 50, W5, 5, 1.5, 1.0, P(4), BIG, None), -3, "inr_msssim2d: pointers must be 16-byte aligned"),
    ("inr_filter3x3", (P(1), P(2), 2, 40, 50, None, None), -1, "inr_filter3x3: null pointer"),
    ("inr_filter3x3", (P(1), P(2), 2, 0, 50, K9, None), -1, "inr_filter3x3: bad sizes (0 x 50)"),
    ("inr_filter3x3", (P(1), P(2), 2, 65536, 65536, K9, None), -1, "inr_filter3x3: image too large (65536 x 65536)"),
    ("inr_filter3x3", (P(1), ODD(2), 2, 40, 50, K9, None), -3, "inr_filter3x3: pointers must be 16-byte aligned"),
    ("inr_image_mse", (P(1), P(2), None, 2, 100, P(3), BIG, None), -1, "inr_image_mse: null pointer"),
    ("inr_image_mse", (P(1), P(2), P(3), 2, 0, P(4), BIG, None), -1, "inr_image_mse: bad sizes (n_images=2, per_image=0)"),
    ("inr_image_mse", (P(1), P(2), P(3), 2, 100, None, BIG, None), -2, "inr_image_mse: workspace too small (0 doubles, 320 needed)"),
    ("inr_image_mse", (P(1), P(2), P(3), 2, 100, P(4), 100, None), -2, "inr_image_mse: workspace too small (100 doubles, 320 needed)"),
    ("inr_image_mse", (P(1), P(2), P(3), 2, 100, ODD(4), BIG, None), -3, "inr_image_mse: workspace must be 16-byte aligned"),
    ("inr_image_mse", (P(1), ODD(2), P(3), 2, 100, P(4), BIG, None), -3, "inr_image_mse: pointers must be 16-byte aligned"),
    ("inr_hf_gain", (None, P(2), P(3), 2, 100, P(4), BIG, None), -1, "inr_hf_gain: null pointer"),
    ("inr_hf_gain", (P(1), P(2), P(3), 70000, 100, P(4), BIG, None), -1, "inr_hf_gain: bad sizes (n_images=70000, per_image=100)"),
    ("inr_hf_gain", (P(1), P(2), P(3), 2, 100, P(4), 100, None), -2, "inr_hf_gain: workspace too small (100 doubles, 320 needed)"),
    ("inr_hf_gain", (P(1), P(2), P(3), 2, 100, ODD(4), BIG, None), -3, "inr_hf_gain: workspace must be 16-byte aligned"),
    # ---- erd_volume.hip
    ("inr_auto_erd_volume", (P(1), None, None, None, None, None, None, None, None, None, 16, 6, GROUPS, 2, 1000.0, 1, None), -1, "inr_auto_erd_volume: null pointer (values)"),
    ("inr_auto_erd_volume", (P(1), None, None, None, None, P(2), P(3), None, None, None, 16, 6, GROUPS, 2, 1000.0, 1, None), -1, "inr_auto_erd_volume: null pointer (b0, which the ADC outputs need)"),
    ("inr_auto_erd_volume", (P(1), None, None, None, None, None, P(3), None, None, None, -1, 6, GROUPS, 2, 1000.0, 1, None), -1, "inr_auto_erd_volume: bad pixel count"),
    ("inr_auto_erd_volume", (P(1), None, None, None, None, None, P(3), None, None, None, 16, 1, GROUPS, 2, 1000.0, 1, None), -1, "inr_auto_erd_volume: 2 <= acquisitions <= 32 (got 1)"),
    ("inr_auto_erd_volume", (P(1), None, None, None, None, None, P(3), None, None, None, 16, 6, GROUPS, 2, 1000.0, 3, None), -1, "inr_auto_erd_volume: rule must be 0 (no clustering), 1 (majority voting) or 2 (intensity-cognisant)"),
    ("inr_auto_erd_volume", (P(1), None, None, None, None, None, P(3), None, None, None, 16, 6, GROUPS, 0, 1000.0, 1, None), -1, "inr_auto_erd_volume: 1 <= groups <= 8 (got 0)"),
    ("inr_auto_erd_volume", (P(1), None, None, None, None, None, P(3), None, None, None, 16, 6, None, 2, 1000.0, 1, None), -1, "inr_auto_erd_volume: null pointer (group_sizes)"),
    ("inr_auto_erd_volume", (P(1), None, None, None, None, None, P(3), None, None, None, 16, 6, GROUPS_SHORT, 2, 1000.0, 1, None), -1, "inr_auto_erd_volume: the group sizes sum to 5, not to the 6 acquisitions"),
    ("inr_auto_erd_volume", (P(1), None, None, None, None, None, P(3), None, None, None, 16, 6, GROUPS, 2, 0.0, 1, None), -1, "inr_auto_erd_volume: b must not be 0"),
    ("inr_auto_erd_volume", (P(1), None, None, None, None, None, P(3), None, None, P(4), 16, 6, GROUPS, 2, 1000.0, 1, None), -1, "inr_auto_erd_volume: accept_in supplies the weights of rule 0; rules 1 and 2 compute them"),
    # ---- hybrid_fit.hip
    ("inr_hybrid_fit", (P(1), P(2), P(3), P(4), None, 8, None), -1, "inr_hybrid_fit: null pointer"),
    ("inr_hybrid_fit", (P(1), P(2), P(3), P(4), P(5), -1, None), -1, "inr_hybrid_fit: bad voxel count -1"),
    ("inr_hybrid_fit", (P(1), P(2), P(3), P(4), P(5), (1 << 33) + 1, None), -1, "inr_hybrid_fit: bad voxel count 8589934593"),
    # ---- rams.hip
    ("inr_rams_forward", (None, P(1), P(2), P(3), 1, 16, 16, 0, P(4), BIG, None), -1, "rams descriptor is null"),
    ("inr_rams_forward", (RAMS_BAD, P(1), P(2), P(3), 1, 16, 16, 0, P(4), BIG, None), -1, "rams kernels need filters == 32 and kernel_size == 3 (got 16, 3)"),
    ("inr_rams_forward", (RAMS_CH8, P(1), P(2), P(3), 1, 16, 16, 0, P(4), BIG, None), -1, "rams: channels must leave a temporal depth of 3 before the head (channels=8)"),
    ("inr_rams_forward", (RAMS, P(1), None, P(3), 1, 16, 16, 0, P(4), BIG, None), -1, "inr_rams_forward: null pointer"),
    ("inr_rams_forward", (RAMS, P(1), P(2), P(3), 0, 16, 16, 0, P(4), BIG, None), -1, "inr_rams_forward: bad sizes (B=0 H=16 W=16)"),
    ("inr_rams_forward", (RAMS, P(1), P(2), P(3), 1, 2000, 2000, 0, P(4), BIG, None), -1, "inr_rams_forward: one image's activations must stay below 2 GiB"),
    ("inr_rams_forward", (RAMS, P(1), P(2), P(3), 1, 16, 16, 0, P(4), 1000, None), -2, "inr_rams_forward: workspace too small"),
    ("inr_rams_forward", (RAMS, P(1), P(2), P(3), 1, 16, 16, 0, None, BIG, None), -2, "inr_rams_forward: workspace too small"),
    ("inr_rams_forward", (RAMS, P(1), P(2), P(3), 1, 16, 16, 0, ODD(4), BIG, None), -3, "inr_rams_forward: params/workspace alignment"),
    ("inr_rams_conv3d_forward", (P(1), P(2), P(3), None, 1, 8, 8, 8, 1, 0, None), -1, "inr_rams_conv3d_forward: null pointer"),
    ("inr_rams_conv3d_forward", (P(1), P(2), P(3), P(4), 1, 8, 8, 8, 2, 0, None), -1, "conv3d: bad shape (B=1 D=8x8x8 pad=2)"),
    ("inr_rams_conv3d_forward", (P(1), P(2), P(3), P(4), 1, 2, 8, 8, 0, 0, None), -1, "conv3d: volume smaller than the kernel"),
    ("inr_rams_conv3d_forward", (P(1), P(2), P(3), P(4), 65535, 512, 512, 512, 1, 0, None), -1, "conv3d: volume too large"),
    ("inr_rams_conv3d_forward", (P(1), P(2), P(3), P(4), 1, 512, 512, 512, 1, 0, None), -1, "conv3d: one image must stay below 2 GiB"),
    ("inr_rams_conv3d_forward", (P(1), ODD(2), P(3), P(4), 1, 8, 8, 8, 1, 0, None), -3, "inr_rams_conv3d_forward: x / w must be 16-byte aligned"),
    ("inr_rams_conv3d_dgrad", (P(1), None, P(3), 1, 8, 8, 8, P(4), BIG, None), -1, "inr_rams_conv3d_dgrad: null pointer"),
    ("inr_rams_conv3d_dgrad", (P(1), P(2), P(3), 0, 8, 8, 8, P(4), BIG, None), -1, "conv3d: bad shape (B=0 D=8x8x8 pad=1)"),
    ("inr_rams_conv3d_dgrad", (P(1), P(2), P(3), 1, 8, 8, 8, P(4), 1000, None), -2, "inr_rams_conv3d_dgrad: workspace too small"),
    ("inr_rams_conv3d_dgrad", (P(1), P(2), P(3), 1, 8, 8, 8, None, BIG, None), -2, "inr_rams_conv3d_dgrad: workspace too small"),
    ("inr_rams_conv3d_dgrad", (P(1), P(2), P(3), 1, 8, 8, 8, ODD(4), BIG, None), -3, "inr_rams_conv3d_dgrad: dy / workspace must be 16-byte aligned"),
    ("inr_rams_conv3d_wgrad", (P(1), None, None, P(3), 1, 8, 8, 8, 1, P(4), BIG, None), -1, "inr_rams_conv3d_wgrad: null pointer"),
    ("inr_rams_conv3d_wgrad", (P(1), None, P(2), P(3), 1, 8, 8, 0, 1, P(4), BIG, None), -1, "conv3d: bad shape (B=1 D=8x8x0 pad=1)"),
    ("inr_rams_conv3d_wgrad", (P(1), None, P(2), P(3), 1, 8, 8, 8, 1, P(4), 1000, None), -2, "inr_rams_conv3d_wgrad: workspace too small"),
    ("inr_rams_conv3d_wgrad", (P(1), None, ODD(2), P(3), 1, 8, 8, 8, 1, P(4), BIG, None), -3, "inr_rams_conv3d_wgrad: x / dy must be 16-byte aligned"),
    ("inr_rams_train_param_offsets", (None, OFFS, 512), -1, "inr_rams_train_param_offsets: null pointer"),
    ("inr_rams_train_param_offsets", (RAMS, None, 512), -1, "inr_rams_train_param_offsets: null pointer"),
    ("inr_rams_train_param_offsets", (RAMS, OFFS, 2), -1, "rams: 31 layers, room for 2"),
    ("inr_rams_train_grads", (None, P(1), P(2), P(3), P(4), P(5), P(6), None, 1, 16, 16, P(7), BIG, None), -1, "rams descriptor is null"),
    ("inr_rams_train_grads", (RAMS_CH8, P(1), P(2), P(3), P(4), P(5), P(6), None, 1, 16, 16, P(7), BIG, None), -1, "rams train: supported configuration is filters 32, kernel 3, channels 9"),
    ("inr_rams_train_grads", (RAMS, P(1), P(2), P(3), P(4), P(5), P(6), None, 1, 16, 12, P(7), BIG, None), -1, "rams train: batch >= 1 and square low-resolution patches (the loss of utils/loss.py works on squares)"),
    ("inr_rams_train_grads", (RAMS, P(1), P(2), P(3), P(4), None, P(6), None, 1, 16, 16, P(7), BIG, None), -1, "inr_rams_train_grads: null pointer"),
    ("inr_rams_train_grads", (RAMS, P(1), P(2), P(3), P(4), P(5), P(6), None, 1, 16, 16, P(7), 1000, None), -2, "inr_rams_train_grads: workspace too small"),
    ("inr_rams_train_grads", (RAMS, P(1), P(2), P(3), P(4), P(5), P(6), None, 1, 16, 16, None, BIG, None), -2, "inr_rams_train_grads: workspace too small"),
    ("inr_rams_train_grads", (RAMS, P(1), P(2), P(3), P(4), P(5), P(6), None, 1, 16, 16, ODD(7), BIG, None), -3, "inr_rams_train_grads: params / grads / workspace must be 16-byte aligned"),
    ("inr_rams_train_step", (RAMS, P(1), P(2), None, P(4), P(5), P(6), P(7), P(8), 1, 16, 16, 1, 1e-4, 0.9, 0.999, 1e-7, P(9), BIG, None), -1, "inr_rams_train_step: Adam state missing or step < 1"),
    ("inr_rams_train_step", (RAMS, P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8), 1, 16, 16, 0, 1e-4, 0.9, 0.999, 1e-7, P(9), BIG, None), -1, "inr_rams_train_step: Adam state missing or step < 1"),
    ("inr_rams_train_step", (RAMS, P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8), 1, 16, 16, 1, 1e-4, 0.9, 0.999, 1e-7, P(9), 1000, None), -2, "inr_rams_train_grads: workspace too small"),
    # ---- register.hip (not moved: its two workspace refusals share the helper of the fp64 image families)
    ("inr_masked_xcorr", (P(1), P(2), P(3), None, P(4), P(5), P(6), 2, 3, 32, 32, 4, 4, 0.3, None, BIG, None), -2, "inr_masked_xcorr: workspace too small (0 doubles, 2916 needed)"),
    ("inr_masked_xcorr", (P(1), P(2), P(3), None, P(4), P(5), P(6), 2, 3, 32, 32, 4, 4, 0.3, P(7), 100, None), -2, "inr_masked_xcorr: workspace too small (100 doubles, 2916 needed)"),
    ("inr_masked_xcorr", (P(1), P(2), P(3), None, P(4), P(5), P(6), 2, 3, 32, 32, 4, 4, 0.3, P(7), -1, None), -2, "inr_masked_xcorr: workspace too small (-1 doubles, 2916 needed)"),
    ("inr_masked_xcorr", (P(1), P(2), P(3), None, P(4), P(5), P(6), 2, 3, 32, 32, 4, 4, 0.3, ODD(7), BIG, None), -3, "inr_masked_xcorr: workspace must be 16-byte aligned"),
    ("inr_shift2d", (P(1), P(2), P(3), 2, 32, 32, 0, 0.0, None, BIG, None), -2, "inr_shift2d: workspace too small (0 doubles, 2048 needed)"),
    ("inr_shift2d", (P(1), P(2), P(3), 2, 32, 32, 0, 0.0, P(4), 100, None), -2, "inr_shift2d: workspace too small (100 doubles, 2048 needed)"),
    ("inr_shift2d", (P(1), P(2), P(3), 2, 32, 32, 0, 0.0, P(4), -1, None), -2, "inr_shift2d: workspace too small (-1 doubles, 2048 needed)"),
    ("inr_shift2d", (P(1), P(2), P(3), 2, 32, 32, 0, 0.0, ODD(4), BIG, None), -3, "inr_shift2d: workspace must be 16-byte aligned"),
]

# (planner, arguments, value): a small fixed shape, then where there is one an out-of-range shape that the planner answers with 0
# (a count answers with INR_E_INVALID)
PLANNERS = [
    ("inr_mse_workspace_bytes", (5000,), 20),
    ("inr_mse_workspace_bytes", (0,), 4),
    ("inr_metric_workspace_bytes", (3,), 1536),
    ("inr_metric_workspace_bytes", (0,), 512),
    ("inr_rams_shift_loss_workspace_bytes", (2, 3), 784),
    ("inr_rams_shift_loss_workspace_bytes", (0, -1), 8),
    ("inr_rams_shift_loss_grad_workspace_bytes", (2, 3), 800),
    ("inr_rams_shift_loss_grad_workspace_bytes", (0, -1), 20),
    ("inr_resize_z_cubic_workspace_bytes", (10, 8), 640),
    ("inr_resize_z_cubic_workspace_bytes", (0, 0), 8),
    ("inr_rams_shift_ssim_workspace_bytes", (2, 64, 3), 240336),
    ("inr_rams_shift_ssim_workspace_bytes", (2, 64, 17), 0),
    ("inr_rams_shift_ssim_workspace_bytes", (2, 16, 3), 0),
    ("inr_rams_shift_ssim_grad_workspace_bytes", (2, 64, 3), 404888),
    ("inr_rams_shift_ssim_grad_workspace_bytes", (2, 9000, 3), 0),
    ("inr_rescale2d_workspace_doubles", (2, 32, 48, 3, 1), 11168),
    ("inr_rescale2d_workspace_doubles", (2, 32, 48, 1, 0), 6176),
    ("inr_rescale2d_workspace_doubles", (2, 32, 48, 2, 0), 0),
    ("inr_rescale2d_workspace_doubles", (2, 32, 5000, 3, 1), 0),
    ("inr_fourier_resample_workspace_doubles", (2, 8, 12, 16, 24), 800),
    ("inr_fourier_resample_workspace_doubles", (2, 8, 12, 16, 1025), 0),
    ("inr_fourier_resample_workspace_doubles", (-1, 8, 12, 16, 24), 0),
    ("inr_perceptual_workspace_doubles", (2, 40, 50, 5), 2944),
    ("inr_perceptual_workspace_doubles", (2, 1, 1, 1), 320),
    ("inr_perceptual_workspace_doubles", (2, 40, 50, 0), 0),
    ("inr_perceptual_workspace_doubles", (0, 40, 50, 5), 0),
    ("inr_rams_param_count", (RAMS,), 419828),
    ("inr_rams_param_count", (None,), -1),
    ("inr_rams_param_count", (RAMS_BAD,), -1),
    ("inr_rams_workspace_bytes", (RAMS, 1, 16, 16), 4787884),
    ("inr_rams_workspace_bytes", (RAMS, 0, 16, 16), 0),
    ("inr_rams_workspace_bytes", (RAMS_BAD, 1, 16, 16), 0),
    ("inr_rams_conv3d_dgrad_workspace_bytes", (), 110848),
    ("inr_rams_conv3d_wgrad_workspace_bytes", (1, 8, 8, 8, 1), 116929024),
    ("inr_rams_conv3d_wgrad_workspace_bytes", (1, 1, 1, 1, 0), 116929024),
    ("inr_rams_train_param_count", (RAMS,), 400660),
    ("inr_rams_train_param_count", (None,), -1),
    ("inr_rams_train_workspace_bytes", (RAMS, 1, 16, 16), 134683904),
    ("inr_rams_train_workspace_bytes", (RAMS, 1, 2, 16), 0),
    ("inr_rams_train_workspace_bytes", (None, 1, 16, 16), 0),
    ("inr_masked_xcorr_workspace_doubles", (2, 3, 32, 32, 4, 4), 2916),
    ("inr_masked_xcorr_workspace_doubles", (2, 3, 32, 32, 32, 4), 0),
    ("inr_shift2d_workspace_doubles", (2, 32, 32, 0), 2048),
    ("inr_shift2d_workspace_doubles", (2, 32, 32, 5), 0),
]


@pytest.mark.parametrize("row", range(len(REFUSALS)), ids=lambda i: f"{REFUSALS[i][0]}-{i}")
def test_a_bad_call_is_refused_with_its_status_and_message(row):
    name, args, status, message = REFUSALS[row]
    lib = _lib.lib()
    assert getattr(lib, name)(*args) == status
    assert lib.inr_last_error().decode() == message


@pytest.mark.parametrize("row", range(len(PLANNERS)), ids=lambda i: f"{PLANNERS[i][0]}-{i}")
def test_a_planner_keeps_its_value(row):
    name, args, value = PLANNERS[row]
    assert getattr(_lib.lib(), name)(*args) == value


def test_every_row_names_a_bound_entry_point_and_a_refusal_status():
    for name, _, status, _ in REFUSALS:
        assert name in _lib.SIGNATURES and status in (_lib.INR_E_INVALID, _lib.INR_E_WORKSPACE, _lib.INR_E_ALIGN), name
    assert all(name in _lib.SIGNATURES for name, _, _ in PLANNERS)
