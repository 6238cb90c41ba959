"""ctypes binding of libinrhip.so (include/inrhip.h).  No compute happens here.

The library is REQUIRED: there is no CPU or PyTorch fallback for the kernels.  ``lib()`` raises
``InrHipUnavailable`` if the shared object has not been built.
"""
from __future__ import annotations

import ctypes as C
import os

from ._build import LIB_PATH

c_f32p = C.c_void_p      # raw device pointers travel as integers (tensor.data_ptr())
c_i64p = C.POINTER(C.c_int64)
c_stream = C.c_void_p
c_ptr_array = C.POINTER(C.c_void_p)   # host array of device pointers (nullable where the header says so)


INR_E_INVALID, INR_E_WORKSPACE, INR_E_ALIGN, INR_E_TIMEOUT = -1, -2, -3, -4     # include/inrhip.h
INR_LF_COUNT = 14
INR_PIA_LF_COUNT = 4
INR_JET_LF_INPUT, INR_JET_LF_LAYER, INR_JET_LF_HEAD, INR_JET_LF_COUNT = 0, 1, 2, 3
INR_LF_ERD_STEP, INR_LF_ERD_REDUCE, INR_LF_ERD_FORWARD, INR_LF_ERD_SOFT = 32, 33, 34, 35
INR_ERD_RUNNING, INR_ERD_CONVERGED, INR_ERD_COLLAPSED = 0, 1, 2
INR_RESCALE_REFLECT, INR_RESCALE_EDGE, INR_RESCALE_MAX_RADIUS, INR_RESCALE_MAX_LINE = 0, 1, 64, 4096
INR_FOURIER_SAMPLE, INR_FOURIER_CENTER, INR_FOURIER_PERIODIC, INR_FOURIER_MIRROR, INR_FOURIER_MAX_LINE = 0, 1, 0, 1, 1024
INR_TVSR_MAX_FACTOR, INR_TVSR_MAX_SIDE, INR_TVSR3D_MAX_ITER, INR_TVMF_MAX_FRAMES = 8, 1024, 100000, 64
INR_TVMS_MAX_STACKS, INR_TVMS_MAX_TAPS = 8, 16
INR_TVJ_MAX_CHANNELS = 16
INR_MPPCA_MAX_RANK, INR_MPPCA_MAX_LONG = 64, 1024
INR_DEGIBBS_MAX_LINE, INR_DEGIBBS_MAX_SHIFTS, INR_DEGIBBS_MAX_WINDOW, INR_DEGIBBS_CHUNK_DOUBLES = 1024, 64, 8, 1 << 21
INR_NLM_MAX_SEARCH, INR_NLM_MAX_PATCH, INR_NLM_MAX_CHANNELS, INR_NLM_MAX_PASSES, INR_NLM_CENTER_MAX, INR_NLM_CENTER_ONE = 5, 2, 16, 10000, 0, 1


class InrHipError(RuntimeError):
    """A libinrhip.so entry point returned a non-zero status."""


class InrHipUnavailable(RuntimeError):
    """libinrhip.so is missing (not built) -- the HIP path cannot run and nothing replaces it."""


class SirenDesc(C.Structure):
    _fields_ = [("in_features", C.c_int), ("hidden_features", C.c_int), ("hidden_layers", C.c_int),
                ("out_features", C.c_int), ("first_omega", C.c_float), ("hidden_omega", C.c_float)]


class RamsDesc(C.Structure):
    _fields_ = [("scale", C.c_int), ("filters", C.c_int), ("kernel_size", C.c_int), ("channels", C.c_int),
                ("r", C.c_int), ("n_rfab", C.c_int), ("mean", C.c_float), ("std", C.c_float)]


class PiaDesc(C.Structure):
    _fields_ = [("n_signals", C.c_int), ("n_hidden", C.c_int), ("hidden", C.c_int * 8), ("predictor_depth", C.c_int),
                ("n_b", C.c_int), ("n_te", C.c_int), ("leaky_slope", C.c_float), ("b_values", C.c_double * 8),
                ("te_values", C.c_double * 8), ("D_mean", C.c_double * 3), ("D_delta", C.c_double * 3),
                ("T2_mean", C.c_double * 3), ("T2_delta", C.c_double * 3)]


class WireDesc(C.Structure):
    _fields_ = [("in_features", C.c_int), ("hidden_features", C.c_int), ("hidden_layers", C.c_int),
                ("out_features", C.c_int), ("first_omega", C.c_float), ("hidden_omega", C.c_float),
                ("first_scale", C.c_float), ("hidden_scale", C.c_float)]


class DeviceCaps(C.Structure):
    _fields_ = [("abi_version", C.c_int), ("device", C.c_int), ("compute_units", C.c_int),
                ("wavefront_size", C.c_int), ("lds_bytes_per_cu", C.c_int), ("clock_khz", C.c_int),
                ("hbm_bytes", C.c_int64), ("arch", C.c_char * 32)]


# name -> (restype, argtypes); must list EVERY symbol declared in include/inrhip.h
SIGNATURES = {
    "inr_version": (C.c_int, []),
    "inr_build_flags": (C.c_int, []),
    "inr_last_error": (C.c_char_p, []),
    "inr_device_caps": (C.c_int, [C.c_int, C.POINTER(DeviceCaps)]),
    "inr_mgrid": (C.c_int, [c_f32p, c_i64p, C.c_int, C.c_int64, C.c_int64, c_stream]),
    "inr_fourier_map": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int, C.c_int, c_stream]),
    "inr_grid_fourier_map": (C.c_int, [c_f32p, c_i64p, C.c_int, C.c_int64, C.c_int64, c_f32p, C.c_int, c_stream]),
    "inr_sine_layer_forward": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int, C.c_int,
                                         C.c_float, c_stream]),
    "inr_tanh_layer_forward": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int, C.c_int,
                                         C.c_float, c_stream]),
    "inr_linear_tanh_head_forward": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int, C.c_int,
                                               C.c_float, c_stream]),
    "inr_mul": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int64, c_stream]),
    "inr_linear_head_forward": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                          C.c_float, c_stream]),
    "inr_mse_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "inr_mse_loss_grad": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_void_p, C.c_size_t,
                                    c_stream]),
    "inr_head_backward_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "inr_linear_head_backward": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64,
                                           C.c_int, C.c_int, C.c_void_p, C.c_size_t, c_stream]),
    "inr_sine_layer_backward_input_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "inr_sine_layer_backward_input": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int, C.c_int,
                                                C.c_void_p, C.c_size_t, c_stream]),
    "inr_linear_param_grad_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "inr_linear_param_grad": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                        C.c_size_t, c_stream]),
    "inr_adam_step": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int64, C.c_double, C.c_double,
                                C.c_double, C.c_double, c_stream]),
    "inr_siren_param_count": (C.c_int64, [C.POINTER(SirenDesc)]),
    "inr_siren_param_offsets": (C.c_int, [C.POINTER(SirenDesc), c_i64p]),
    "inr_siren_forward_workspace_bytes": (C.c_size_t, [C.POINTER(SirenDesc), C.c_int64]),
    "inr_siren_forward": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_f32p, C.c_int64, c_f32p, C.c_int, C.c_float,
                                    C.c_void_p, C.c_size_t, c_stream]),
    "inr_siren_reconstruct_workspace_bytes": (C.c_size_t, [C.POINTER(SirenDesc), C.c_int64]),
    "inr_siren_reconstruct": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_i64p, C.c_int, c_f32p, C.c_int, c_f32p,
                                        C.c_int, C.c_float, C.c_int64, C.c_void_p, C.c_size_t, c_stream]),
    "inr_siren_fit_workspace_bytes": (C.c_size_t, [C.POINTER(SirenDesc), C.c_int64]),
    "inr_siren_fit": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "inr_siren_fit_cycle": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int,
                                      C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double,
                                      C.c_double, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "inr_siren_fit_cycle_batch": (C.c_int, [C.POINTER(SirenDesc), C.c_int, c_ptr_array, c_ptr_array, c_ptr_array, c_ptr_array,
                                            c_f32p, c_ptr_array, c_ptr_array, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int64,
                                            C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, c_ptr_array,
                                            c_ptr_array, C.c_size_t, c_stream]),
    "inr_metric_workspace_bytes": (C.c_size_t, [C.c_int]),
    "inr_psnr": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int64, C.c_double, C.c_void_p, C.c_size_t, c_stream]),
    "inr_ssim2d": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                             C.c_float, C.c_void_p, C.c_size_t, c_stream]),
    "inr_rams_train_param_count": (C.c_int64, [C.POINTER(RamsDesc)]),
    "inr_rams_train_param_offsets": (C.c_int, [C.POINTER(RamsDesc), c_i64p, C.c_int]),
    "inr_rams_train_workspace_bytes": (C.c_size_t, [C.POINTER(RamsDesc), C.c_int, C.c_int, C.c_int]),
    "inr_rams_train_grads": (C.c_int, [C.POINTER(RamsDesc), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_int,
                                       C.c_int, C.c_int, C.c_void_p, C.c_size_t, c_stream]),
    "inr_rams_train_step": (C.c_int, [C.POINTER(RamsDesc), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p,
                                      C.c_int, C.c_int, C.c_int, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double,
                                      C.c_void_p, C.c_size_t, c_stream]),
    "inr_acquisition_products": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                           c_stream]),
    "inr_rescale2d_linear": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_stream]),
    "inr_rescale2d_workspace_doubles": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "inr_rescale2d": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_void_p, C.c_int64, c_stream]),
    "inr_image_means": (C.c_int, [C.c_void_p, C.c_void_p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_stream]),
    "inr_masked_xcorr_workspace_doubles": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "inr_masked_xcorr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int64, c_stream]),
    "inr_shift2d_workspace_doubles": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "inr_shift2d": (C.c_int, [c_f32p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int64,
                              c_stream]),
    "inr_adc_map": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int, c_stream]),
    "inr_resize_z_cubic_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "inr_resize_z_cubic": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_size_t, c_stream]),
    "inr_fourier_operator": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, c_stream]),
    "inr_fourier_resample_workspace_doubles": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "inr_fourier_resample2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_double, C.c_void_p, C.c_int64, c_stream]),
    "inr_fourier_resample2d_f32": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_double, C.c_void_p, C.c_int64, c_stream]),
    "inr_perceptual_workspace_doubles": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "inr_ssim2d_gauss": (C.c_int, [C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                   C.c_void_p, C.c_int64, c_stream]),
    "inr_msssim2d": (C.c_int, [C.c_void_p, C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int,
                               C.c_double, C.c_double, C.c_void_p, C.c_int64, c_stream]),
    "inr_filter3x3": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), c_stream]),
    "inr_image_mse": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, c_stream]),
    "inr_hf_gain": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, c_stream]),
    "inr_rams_param_count": (C.c_int64, [C.POINTER(RamsDesc)]),
    "inr_rams_workspace_bytes": (C.c_size_t, [C.POINTER(RamsDesc), C.c_int, C.c_int, C.c_int]),
    "inr_rams_forward": (C.c_int, [C.POINTER(RamsDesc), c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_size_t, c_stream]),
    "inr_siren_loss_grad": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int64,
                                      c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "inr_siren_loss_grad_ex": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int64,
                                         c_f32p, C.c_void_p, C.c_size_t, C.c_int, c_stream]),
    "inr_siren_hp_eligible": (C.c_int, [C.POINTER(SirenDesc)]),
    "inr_siren_forward_train": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_f32p, c_f32p, C.c_int64, C.c_void_p, C.c_size_t, C.c_int,
                                          c_stream]),
    "inr_siren_backward_train": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_f32p, c_f32p, C.c_int64, C.c_void_p, C.c_size_t,
                                           c_stream]),
    "inr_block_apply2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), c_stream]),
    "inr_block_adjoint2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), c_stream]),
    "inr_tvsr_workspace_doubles": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "inr_tvsr_solve2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int64,
                                   c_stream]),
    "inr_tvsr_solve2d_f32": (C.c_int, [c_f32p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.POINTER(C.c_double), C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int64,
                                       c_stream]),
    "inr_tvsr3d_block_apply": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.POINTER(C.c_double)] * 3 + [c_stream]),
    "inr_tvsr3d_block_adjoint": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.POINTER(C.c_double)] * 3 + [c_stream]),
    "inr_tvsr3d_workspace_doubles": (C.c_int64, [C.c_int] * 7),
    "inr_tvsr3d_solve": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 7 + [C.POINTER(C.c_double)] * 4 + [C.c_double, C.c_double, C.c_int,
                                                                                                 C.c_void_p, C.c_int64, c_stream]),
    "inr_tvsr3d_solve_f32": (C.c_int, [c_f32p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_f32p] + [C.c_int] * 7 +
                             [C.POINTER(C.c_double)] * 4 + [C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int64, c_stream]),
    "inr_frame_apply2d": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 6 + [C.POINTER(C.c_double), c_stream]),
    "inr_frame_adjoint2d": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.POINTER(C.c_double), c_stream]),
    "inr_tvmf_workspace_doubles": (C.c_int64, [C.c_int] * 6),
    "inr_tvmf_solve2d": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 6 + [C.POINTER(C.c_double), C.c_double, C.c_double, C.c_int, C.c_void_p,
                                                                     C.c_int64, c_stream]),
    "inr_tvmf_solve2d_f32": (C.c_int, [c_f32p, C.c_void_p, C.c_void_p, C.c_void_p, c_f32p, C.c_void_p, c_f32p, c_f32p] + [C.c_int] * 6 +
                             [C.POINTER(C.c_double), C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int64, c_stream]),
    "inr_tvms_apply": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 5 + [C.POINTER(C.c_int), C.POINTER(C.c_double), c_stream]),
    "inr_tvms_adjoint": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 5 + [C.POINTER(C.c_int), C.POINTER(C.c_double), c_stream]),
    "inr_tvms_workspace_doubles": (C.c_int64, [C.c_int] * 5 + [C.POINTER(C.c_int)]),
    "inr_tvms_solve": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 5 + [C.POINTER(C.c_int)] + [C.POINTER(C.c_double)] * 2 +
                       [C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int64, c_stream]),
    "inr_tvms_solve_f32": (C.c_int, [c_f32p, C.c_void_p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_f32p] + [C.c_int] * 5 +
                           [C.POINTER(C.c_int)] + [C.POINTER(C.c_double)] * 2 +
                           [C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int64, c_stream]),
    "inr_tvop_workspace_doubles": (C.c_int64, [C.c_int] * 5),
    "inr_tvop_apply": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p, C.c_int64, c_stream]),
    "inr_tvop_adjoint": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p, C.c_int64, c_stream]),
    "inr_tvop_solve2d": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 5 + [C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int64, c_stream]),
    "inr_tvop_solve2d_f32": (C.c_int, [c_f32p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_void_p] + [C.c_int] * 5 +
                             [C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int64, c_stream]),
    "inr_tvj_workspace_doubles": (C.c_int64, [C.c_int] * 4),
    "inr_tvj_solve2d": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 6 + [C.POINTER(C.c_double)] * 2 + [C.c_double, C.c_double, C.c_int, C.c_int,
                                                                                                C.c_void_p, C.c_int64, c_stream]),
    "inr_tvj_solve2d_f32": (C.c_int, [c_f32p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_f32p] + [C.c_int] * 6 +
                            [C.POINTER(C.c_double)] * 2 + [C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int64, c_stream]),
    "inr_tvadc_workspace_doubles": (C.c_int64, [C.c_int] * 6),
    "inr_tvadc_solve2d": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 6 + [C.POINTER(C.c_double)] * 3 +
                          [C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int64, c_stream]),
    "inr_tvadc_solve2d_f32": (C.c_int, [c_f32p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_f32p] + [C.c_int] * 6 +
                              [C.POINTER(C.c_double)] * 3 + [C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double,
                                                             C.c_double, C.c_void_p, C.c_int64, c_stream]),
    "inr_adc_signal": (C.c_int, [C.c_void_p] * 3 + [C.POINTER(C.c_double), C.c_int64, C.c_int, C.c_int64, c_stream]),
    "inr_adc_signal_f32": (C.c_int, [c_f32p] * 3 + [C.POINTER(C.c_double), C.c_int64, C.c_int, C.c_int64, c_stream]),
    "inr_mppca_denoise": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 8 + [c_stream]),
    "inr_mppca_denoise_f32": (C.c_int, [c_f32p] * 2 + [C.c_void_p, c_f32p, C.c_void_p] + [C.c_int] * 8 + [c_stream]),
    "inr_degibbs_lines_workspace_doubles": (C.c_int64, [C.c_longlong, C.c_int, C.c_int]),
    "inr_degibbs2d_workspace_doubles": (C.c_int64, [C.c_int] * 4),
    "inr_degibbs_lines": (C.c_int, [C.c_void_p] * 3 + [C.c_longlong] + [C.c_int] * 4 + [C.c_void_p, C.c_int64, c_stream]),
    "inr_degibbs_lines_f32": (C.c_int, [c_f32p, C.c_void_p, c_f32p, C.c_longlong] + [C.c_int] * 4 + [C.c_void_p, C.c_int64, c_stream]),
    "inr_degibbs2d": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p, C.c_int64, c_stream]),
    "inr_degibbs2d_f32": (C.c_int, [c_f32p, C.c_void_p, c_f32p] + [C.c_int] * 6 + [C.c_void_p, C.c_int64, c_stream]),
    "inr_nlm3d": (C.c_int, [C.c_void_p] * 3 + [C.c_double] + [C.c_void_p] * 3 + [C.c_int] * 12 + [c_stream]),
    "inr_nlm3d_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_double, c_f32p, c_f32p, C.c_void_p] + [C.c_int] * 12 + [c_stream]),
    "inr_nlm_upsample_workspace_doubles": (C.c_int64, [C.c_int] * 7),
    "inr_nlm_upsample": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 7 + [C.POINTER(C.c_double)] * 4 + [C.c_int, C.c_int, C.c_double] +
                         [C.c_int] * 6 + [C.c_void_p, C.c_int64, c_stream]),
    "inr_nlm_upsample_f32": (C.c_int, [c_f32p, C.c_void_p, c_f32p, c_f32p, c_f32p] + [C.c_int] * 7 + [C.POINTER(C.c_double)] * 4 +
                             [C.c_int, C.c_int, C.c_double] + [C.c_int] * 6 + [C.c_void_p, C.c_int64, c_stream]),
    "inr_tgv_workspace_doubles": (C.c_int64, [C.c_int] * 3),
    "inr_tgv_solve2d": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 5 + [C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, C.c_int,
                                                                    C.c_void_p, C.c_int64, c_stream]),
    "inr_tgv_solve2d_f32": (C.c_int, [c_f32p, c_f32p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_f32p] + [C.c_int] * 5 +
                            [C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int64, c_stream]),
    "inr_footprint_expand": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int, C.c_int, c_stream]),
    "inr_footprint_reduce": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int, c_stream]),
    "inr_footprint_loss_workspace_floats": (C.c_int64, [C.c_int64]),
    "inr_footprint_loss_grad": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int, C.c_int64,
                                          C.c_void_p, C.c_int64, c_stream]),
    "inr_siren_fit_footprint_workspace_floats": (C.c_int64, [C.POINTER(SirenDesc), C.c_int64, C.c_int]),
    "inr_siren_fit_footprint": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                          C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                          c_f32p, C.c_void_p, C.c_int64, c_stream]),
    "inr_rams_shift_loss_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "inr_rams_shift_loss": (C.c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_size_t, c_stream]),
    "inr_rams_conv3d_forward": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          c_stream]),
    "inr_rams_conv3d_dgrad_workspace_bytes": (C.c_size_t, []),
    "inr_rams_conv3d_dgrad": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                        c_stream]),
    "inr_rams_conv3d_wgrad_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "inr_rams_conv3d_wgrad": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_size_t, c_stream]),
    "inr_rams_shift_loss_grad_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "inr_rams_shift_loss_grad": (C.c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_size_t, c_stream]),
    "inr_rams_shift_ssim_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "inr_rams_shift_ssim": (C.c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_size_t, c_stream]),
    "inr_rams_shift_ssim_grad_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "inr_rams_shift_ssim_grad": (C.c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_size_t, c_stream]),
    "inr_hybrid_fit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, c_stream]),
    "inr_pia_param_count": (C.c_int64, [C.POINTER(PiaDesc)]),
    "inr_pia_param_offsets": (C.c_int, [C.POINTER(PiaDesc), c_i64p, C.c_int]),
    "inr_pia_workspace_bytes": (C.c_size_t, [C.POINTER(PiaDesc), C.c_int64, C.c_int]),
    "inr_pia_forward": (C.c_int, [C.POINTER(PiaDesc), c_f32p, c_f32p, C.c_int64, c_f32p, C.c_void_p, c_f32p, c_f32p, C.c_int64,
                                  C.c_void_p, C.c_size_t, c_stream]),
    "inr_pia_forward_train": (C.c_int, [C.POINTER(PiaDesc), c_f32p, c_f32p, C.c_int64, c_f32p, C.c_void_p, c_f32p, c_f32p,
                                        C.c_void_p, C.c_size_t, c_stream]),
    "inr_pia_backward_train": (C.c_int, [C.POINTER(PiaDesc), c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, C.c_int64,
                                         C.c_void_p, C.c_size_t, c_stream]),
    "inr_pia_fit_step": (C.c_int, [C.POINTER(PiaDesc), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int64,
                                   C.c_double, C.c_double, C.c_double, C.c_double, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "inr_pia_launch_count": (C.c_int, [C.c_int, c_i64p]),
    "inr_pids_slice": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_void_p, C.c_int64, c_stream]),
    "inr_auto_erd": (C.c_int, [c_f32p, C.c_void_p, c_f32p, C.c_int64, C.c_int, C.c_int, c_stream]),
    "inr_auto_erd_volume": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_double, C.c_int, c_stream]),
    "inr_erd_param_count": (C.c_int64, [C.POINTER(SirenDesc)]),
    "inr_erd_param_offsets": (C.c_int, [C.POINTER(SirenDesc), c_i64p, C.c_int]),
    "inr_erd_workspace_bytes": (C.c_size_t, [C.POINTER(SirenDesc), C.c_int64]),
    "inr_erd_forward": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_f32p, C.c_int64, c_f32p, C.c_int, C.c_float, C.c_int,
                                  C.c_int64, c_stream]),
    "inr_erd_loss_grad": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int, C.c_float,
                                    C.c_int, C.c_int, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "inr_erd_adam_step": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_double, C.c_double,
                                    C.c_double, C.c_double, C.c_double, c_stream]),
    "inr_erd_pretrain": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int64,
                                   C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_float, C.c_void_p, C.c_void_p,
                                   C.c_size_t, c_stream]),
    "inr_erd_finetune": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int,
                                   C.c_int64, C.c_float, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                   C.c_double, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "inr_soft_erd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_double,
                               C.c_double, C.c_double, C.c_void_p, c_stream]),
    "inr_siren_jet_workspace_bytes": (C.c_size_t, [C.POINTER(SirenDesc), C.c_int, C.c_int, C.c_int64, C.c_int]),
    "inr_siren_jet": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_f32p, C.c_int64, C.c_int, C.c_int, c_f32p, C.c_int, c_f32p, c_f32p,
                                c_f32p, C.c_int64, C.c_void_p, C.c_size_t, c_stream]),
    "inr_siren_jet_grid": (C.c_int, [C.POINTER(SirenDesc), c_f32p, c_i64p, C.c_int, C.c_int, c_f32p, C.c_int, c_f32p, c_f32p, c_f32p,
                                     C.c_int64, C.c_void_p, C.c_size_t, c_stream]),
    "inr_jet_launch_count": (C.c_int, [C.c_int, c_i64p]),
    "inr_wire_param_count": (C.c_int64, [C.POINTER(WireDesc)]),
    "inr_wire_param_offsets": (C.c_int, [C.POINTER(WireDesc), c_i64p, C.c_int]),
    "inr_wire_workspace_bytes": (C.c_size_t, [C.POINTER(WireDesc), C.c_int64, C.c_int]),
    "inr_wire_layer_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "inr_wire_layer_forward": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                         C.c_float, C.c_float, C.c_void_p, C.c_size_t, c_stream]),
    "inr_wire_forward": (C.c_int, [C.POINTER(WireDesc), c_f32p, c_f32p, C.c_int64, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "inr_wire_reconstruct_workspace_bytes": (C.c_size_t, [C.POINTER(WireDesc), C.c_int64]),
    "inr_wire_reconstruct": (C.c_int, [C.POINTER(WireDesc), c_f32p, c_i64p, C.c_int, c_f32p, C.c_int, c_f32p, C.c_int, C.c_float,
                                       C.c_int64, C.c_void_p, C.c_size_t, c_stream]),
    "inr_wire_loss_grad": (C.c_int, [C.POINTER(WireDesc), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, c_f32p, C.c_void_p,
                                     C.c_size_t, c_stream]),
    "inr_wire_fit": (C.c_int, [C.POINTER(WireDesc), c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_int64,
                               C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "inr_wire_forward_stash": (C.c_int, [C.POINTER(WireDesc), c_f32p, c_f32p, C.c_int64, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "inr_wire_input_grad": (C.c_int, [C.POINTER(WireDesc), c_f32p, c_f32p, C.c_int64, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "inr_wire_derivatives_workspace_floats": (C.c_int64, [C.POINTER(WireDesc), C.c_int, C.c_int, C.c_int64, C.c_int]),
    "inr_wire_derivatives": (C.c_int, [C.POINTER(WireDesc), c_f32p, c_f32p, C.c_int64, C.c_int, C.c_int, c_f32p, C.c_int, c_f32p,
                                       c_f32p, c_f32p, C.c_int64, C.c_void_p, C.c_int64, c_stream]),
    "inr_wire_derivatives_grid": (C.c_int, [C.POINTER(WireDesc), c_f32p, c_i64p, C.c_int, C.c_int, c_f32p, C.c_int, c_f32p, c_f32p,
                                            c_f32p, C.c_int64, C.c_void_p, C.c_int64, c_stream]),
    "inr_prof_enable": (C.c_int, [C.c_int]),
    "inr_prof_reset": (C.c_int, []),
    "inr_prof_read": (C.c_int, [C.c_int, c_i64p, C.POINTER(C.c_double)]),
    "inr_debug_set": (C.c_int, [C.c_int, C.c_int]),
    "inr_debug_get": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "inr_debug_reset": (C.c_int, []),
    "inr_launch_count": (C.c_int, [C.c_int, c_i64p]),
    "inr_launch_counts_reset": (C.c_int, []),
    "inr_debug_set_ptr": (C.c_int, [C.c_int, C.c_void_p]),
    "inr_sincos_probe": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int64, c_stream]),
}

_LIB = None


def lib():
    """The loaded library with argtypes set.  Raises InrHipUnavailable when it is not built."""
    global _LIB
    if _LIB is None:
        path = os.environ.get("INR_LIB") or LIB_PATH       # INR_LIB: an explicitly selected (diagnostic) build
        if not os.path.exists(path):
            raise InrHipUnavailable(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no fallback path.")
        handle = C.CDLL(path)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        if handle.inr_version() != 1:
            raise InrHipUnavailable(f"libinrhip.so ABI version {handle.inr_version()} != 1: rebuild")
        if handle.inr_build_flags() != 0 and not os.environ.get("INR_LIB"):
            raise InrHipUnavailable(
                f"{path} is a DIAGNOSTIC build (inr_build_flags() = {handle.inr_build_flags()}: time stamps / ablated "
                "kernels); rebuild the product library (`python mri-super-resolution_amd/_build.py --force`) or select the "
                "diagnostic one explicitly with INR_LIB=<path>")
        _LIB = handle
    return _LIB


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().inr_last_error().decode("utf-8", "replace")
        raise InrHipError(f"{what or 'libinrhip'} failed with status {rc}: {msg}")


def shape_array(shape):
    arr = (C.c_int64 * len(shape))(*[int(s) for s in shape])
    return arr
