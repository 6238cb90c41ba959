// Everything that crosses a translation unit of libinrhip.so: host launchers, planners and the diagnostic switches behind
// inr_debug_set, grouped by the file that defines them.  Every .hip file includes this header -- the defining one too, so that
// a declaration that has drifted from its definition fails to compile in the file that is wrong.  Default arguments live here
// and nowhere else.  (set_error, count_launch, launch_finalize and the profiler hooks are in common.h, beside their types.)
#pragma once
#include <vector>

#include "common.h"

namespace inr {

// ---- api.hip: the flat SIREN parameter layout (inr_siren_param_offsets) --------------------------------------------------------------
struct Layout {
    int n_sine;                      // 1 + hidden_layers
    std::vector<long long> w_off, b_off;  // per layer, head last (long long: what siren_small.hip and FinalizeSeg take)
    std::vector<int> fan_in, fan_out;
    long long total;
};
Layout make_layout(const inr_siren_desc_t* d);
inline float layer_omega(const inr_siren_desc_t* d, int l) { return l == 0 ? d->first_omega : d->hidden_omega; }

// ---- gemm_f32.hip: fp32 MFMA and split-fp16 (gemm_h3.inc) GEMMs -------------------------------------------------------------------
int gemm_build_flags();   // inr_build_flags: this unit's diagnostic macros | hp_build_flags()
int gemm_sine_forward(float* act, float* dact, const float* x, const float* W, const float* b, int64_t n,
                      int in_f, int out_f, float omega, hipStream_t stream, const H3Args* h3 = nullptr);
int gemm_tanh_forward(float* act, float* dact, const float* x, const float* W, const float* b, int64_t n, int in_f,
                      int out_f, float scale, hipStream_t stream);
int input_grad_colsum_rows(int64_t n);
int gemm_input_grad(float* dz_prev, const float* dz, const float* W, const float* mul, int64_t n, int in_f,
                    int out_f, float* colsum_slab, int* slab_rows, hipStream_t stream, const H3Args* h3 = nullptr);
int param_grad_splits(int64_t n, int in_f, int out_f);
int gemm_param_grad_slabs(float* slabs, int splits, const float* dz, const float* x, int64_t n, int in_f,
                          int out_f, hipStream_t stream, const H3Args* h3 = nullptr);
size_t h3_planes_bytes(long long weights);
int h3_tensor_amax(unsigned* out, const float* x, long long n, hipStream_t stream, unsigned floor_bits = 0);
int h3_weight_split(const float* const* W, const int* out_f, const int* in_f, int layers, _Float16* planes,
                    unsigned* amax, unsigned* zero_slots, int n_zero, hipStream_t stream);
extern tune_int g_force_generic;   // key 0
extern tune_int g_mfma16;          // key 1
extern tune_int g_h3;              // key 3
extern tune_int g_h3_wide;         // key 6
extern char* g_h3_scratch;         // inr_debug_set_ptr(1, .)
extern unsigned long long* g_stamps;          // inr_debug_set_ptr(0, .): diagnostic builds only (every unit with stamped kernels reads it)

// ---- gemm_hp.hip: the pre-split (HL32) GEMM family, gemm_hp*.inc ---------------------------------------------------------------------
int hp_build_flags();
bool hp_head_ok(int hidden);
size_t hp_prep_part_bytes();
int hp_weight_prep(const float* const* W, const int* out_f, const int* in_f, int layers, char* planes, HpSlots slots,
                   unsigned* part, float* head_bound, const float* head_W, const float* head_b, int hidden, const unsigned* tmax,
                   const unsigned* wtmax, float inv_count, float omega, hipStream_t stream, const float* const* bias = nullptr,
                   const float* layer_omega = nullptr, float* act_bound = nullptr, const unsigned* x_amax = nullptr);
int hp_convert(char* out, const float* x, long long rows, int cols, HpScale sc, hipStream_t stream);
int hp_unconvert(float* out, const char* x, long long rows, int cols, HpScale sc, hipStream_t stream);
bool hp_z_stash_ok(int in_f);
int hp_sine_forward(char* act_hl, float* dact, const char* x_hl, const char* W_hl, const float* bias, int64_t n, int in_f,
                    int out_f, float omega, HpScale sa, HpScale sb, int reverse_m, hipStream_t stream, bool z_only = false,
                    HpScale so = HpScale{});
bool hp_row_head_ok(int64_t n, int hidden, int in_f);
int hp_row_head_rows(int64_t n);
int hp_sine_forward_head(char* dz_hl, const char* x_hl, const char* W_hl, const float* bias, int64_t n, int in_f, int out_f, float omega,
                         HpScale sa, HpScale sb, HpScale dz_so, const float* head_w, const float* head_b, const float* target,
                         const float* weight, int64_t count_total, float* slab_b, float* slab_w, float* part_loss, float* part_g,
                         unsigned* amax_out, hipStream_t stream);
int hp_input_grad_max_rows(int64_t n);
int hp_input_grad(char* dzprev_hl, const char* dz_hl, const char* WT_hl, const float* mul, int64_t n, int in_f, int out_f,
                  float* colsum_slab, int* colsum_rows, unsigned* amax_out, HpScale sa, HpScale sb, HpScale so,
                  hipStream_t stream);
bool hp_grid_fourier_ok(int m, int dim);
int hp_grid_fourier_hl(char* x_hl, unsigned* x_amax, const int64_t* shape, int dim, int64_t row_begin, int64_t n_rows, const float* B,
                       int m, hipStream_t stream);
bool hp_fused_forward_ok(int in_f, int hidden, int n_sine);
int hp_fused_forward(float* y, const char* x_hl, const unsigned* x_amax, int64_t n, int in_f, int hidden, int n_sine,
                     const char* const* W_hl, const float* const* bias, const unsigned* const* w_amax, float first_omega,
                     float hidden_omega, const float* head_W, const float* head_b, int use_clamp, float clamp_min,
                     hipStream_t stream);
int hp_param_grad_splits(int64_t n, int in_f, int out_f);
int hp_param_grad_slabs(float* slabs, int splits, const char* dz_hl, const char* x_hl, int64_t n, int in_f, int out_f,
                        HpScale sa, HpScale sb, hipStream_t stream);
int hp_param_grad_multi_max();
int hp_param_grad_multi(const HpParamGradJob* jobs, int njobs, int64_t n, hipStream_t stream);
int hp_head_forward(float* y, const char* a_hl, const float* W, const float* bias, int64_t n, int hidden, int use_clamp,
                    float clamp_min, hipStream_t stream, bool from_z = false, float omega = 0.f, HpScale sa = HpScale{});
int hp_head_bound_ext(float* head_bound, const unsigned* gmax, const float* head_W, int hidden, float omega, hipStream_t stream);
int64_t hp_head_blocks(int64_t n);
int hp_head_step(char* dz_hl, float* slab_b, float* slab_w, float* part_loss, float* part_g, const char* a_hl,
                 const float* dact, const float* W, const float* bias, const float* t, const float* wgt, int64_t n, int hidden,
                 int64_t count_total, unsigned* amax_out, HpScale so, hipStream_t stream, bool from_z = false,
                 float omega = 0.f, const float* g_ext = nullptr, HpScale sa = HpScale{});
extern tune_int g_stamp_class, g_stamp_nth;       // keys 8, 9: which hp launch receives g_stamps
extern tune_int g_hp_persistent, g_hp_stagger;   // keys 10, 11
extern tune_int g_hp_zhead;                       // key 16
extern tune_int g_hp_narrow;                      // key 18
extern tune_int g_hp_fused_fwd;                   // key 19
extern tune_int g_hp_head_min_rows;               // key 21
extern tune_int g_hp_head_rows;                   // key 23
extern tune_int g_hp_row, g_hp_row_min_tiles;     // keys 27, 28: the row-owning 128 x 512 kernel
extern tune_int g_hp_narrow_max_tiles;            // key 29
extern tune_int g_hp_row_head, g_hp_row_head_min_tiles;   // keys 30, 31: the head step fused into the last sine layer
extern tune_int g_hp_grid_cap;                    // key 32: test-only cap on the persistent grids

// ---- kernels.hip ----------------------------------------------------------------------------------------------------------------------
int launch_mgrid(float* out, const int64_t* shape, int dim, int64_t row_begin, int64_t n_rows, hipStream_t st);
int launch_fourier(float* out, const float* x, const int64_t* shape, int dim, int64_t row_begin, int64_t n_rows,
                   const float* B, int m, hipStream_t st);
int launch_head_forward(float* y, const float* a, const float* W, const float* b, int64_t n, int hidden,
                        int out_f, int use_clamp, float clamp_min, hipStream_t st, float* dy = nullptr);
int mse_blocks(int64_t count);
int launch_mse(float* gy, float* loss, const float* y, const float* t, const float* w, int64_t count,
               float* partial, hipStream_t st, int64_t count_total = 0);
int launch_head_dz(float* dz, const float* gy, const float* W, const float* dact, int64_t n, int hidden,
                   int out_f, hipStream_t st);
int64_t colsum_ws_floats(int64_t n, int C, int G);
int launch_colsum(float* out, const float* X, const float* g, int64_t n, int C, int G, float* slab,
                  hipStream_t st);
int64_t reduce_tmp_floats(int64_t nslabs, int64_t len);
int launch_reduce_slabs(float* out, const float* slab, int nslabs, int64_t len, float* tmp, hipStream_t st);
int launch_reduce_slabs_pitched(float* out, const float* slab, int nslabs, int64_t len, int64_t pitch, float* tmp, hipStream_t st);
bool head_fused_ok(int hidden, int out_f, const void* a, const void* b, const void* c, const void* d);
int64_t head_fused_blocks(int64_t n);
int launch_head_bwd_fused(float* dz, float* slab_b, float* slab_w, const float* gy, const float* W, const float* a,
                          const float* dact, int64_t n, int hidden, hipStream_t st, unsigned* amax_out = nullptr);
bool head_step_fused_ok(int hidden, int out_f, const void* a, const void* b, const void* c, const void* d);
int launch_head_step_fused(float* dz, float* slab_b, float* slab_w, float* part_loss, float* part_g, const float* a,
                           const float* dact, const float* W, const float* bias, const float* t, const float* wgt,
                           int64_t n, int hidden, int64_t count_total, hipStream_t st, unsigned* amax_out);
int launch_finish_sum(float* out, const float* partial, int nparts, float scale, hipStream_t st);
int launch_adam(float* p, const float* g, float* m, float* v, int64_t count, int64_t step, double lr, double b1,
                double b2, double eps, hipStream_t st);
int launch_acquisition_products(float* out, const float* r0, const float* r1, const float* r2, const float* r3, int64_t nvox,
                                int n1, int n2, int n3, hipStream_t st);
int launch_mul(float* out, const float* a, const float* b, int64_t count, hipStream_t st);
int launch_sincos_probe(float* s, float* c, const float* x, int64_t n, hipStream_t st);
extern tune_int g_reduce_onepass;   // key 25

// ---- metrics.hip ------------------------------------------------------------------------------------------------------------------------
int metric_workspace_doubles(int nimg);
int launch_psnr(double* out, const float* x, const float* y, int nimg, int64_t per_image, double data_range,
                double* ws, hipStream_t st);
int launch_ssim(double* out, const float* x, const float* y, int nimg, int H, int W, int win, double data_range,
                int use_mask, float mask_thr, double* ws, hipStream_t st);
int launch_shift_loss(double* out, const float* y_true, const float* y_pred, const float* mask, int nimg, int size,
                      int border, int mode, double* ws, hipStream_t st);
int launch_shift_loss_grad(double* loss, float* grad, const float* y_true, const float* y_pred, const float* mask,
                           const float* upstream, int nimg, int size, int border, double* ws, hipStream_t st);
int launch_rescale_linear(float* out, const float* in, int nimg, int H, int W, int OH, int OW, hipStream_t st);
size_t resize_z_workspace_doubles(int64_t n_lines, int n_in);
int launch_resize_z_cubic(double* out, const double* in, int64_t n_lines, int n_in, int n_out, double* ws, hipStream_t st);
int launch_adc(float* out, const float* data, const float* bvals, int64_t npix, int nb, hipStream_t st);
int launch_auto_erd(float* accept, const double* values, const float* erd_map, int64_t npix, int n, int rule, hipStream_t st);

// ---- erd_volume.hip: whole-volume AutoERD on cluster extents, the per-group means and their ADC maps (david.py:44-91) -----------------
int erd_volume_check(int n, const int* group_sizes, int n_groups, double b, int rule);   // host only: no device is touched
int launch_erd_volume(double* accept, double* direction_mean, double* accepted_mean, double* direction_adc, double* accepted_adc,
                      double* adc, const double* values, const double* b0, const double* erd_map, const double* accept_in, int64_t npix,
                      int n, const int* group_sizes, int n_groups, double b, int rule, hipStream_t st);

// ---- rescale.hip: skimage resize for 2-D images (anti-aliasing Gaussian, orders 1 and 3, modes 'reflect' and 'edge') -------------------
constexpr int RESCALE_MAX_RADIUS = INR_RESCALE_MAX_RADIUS;   // Gaussian taps per side that the kernel arguments carry
constexpr int RESCALE_MAX_LINE = INR_RESCALE_MAX_LINE;       // one padded line, staged in LDS as doubles, fits 64 KiB
struct RescaleView { double *filtered, *coef, *minmax; size_t total; };
RescaleView rescale_view(int nimg, int H, int W, int order, int mode, void* base);
int rescale_check(const char* who, int nimg, int H, int W, int OH, int OW, int order, int mode, int anti_aliasing, int clip_group);
int launch_rescale2d(float* out, const float* in, int nimg, int H, int W, int OH, int OW, int order, int mode, int anti_aliasing,
                     int clip_group, const RescaleView& v, hipStream_t st);

// ---- fourier.hip: Fourier (k-space zero-fill / truncation) re-sampling, one dense operator per axis applied as an fp64 MFMA GEMM -----------
constexpr int FOURIER_MAX_LINE = INR_FOURIER_MAX_LINE;
struct FourierView { double *op_rows, *op_cols, *mid; size_t total; };
FourierView fourier_view(int nimg, int H, int W, int OH, int OW, void* base);
int fourier_sizes_check(const char* who, int nimg, int H, int W, int OH, int OW);   // what the planner can judge
int fourier_operator_check(const char* who, int n, int m, int align, int boundary, double apodize);
int fourier_check(const char* who, int nimg, int H, int W, int OH, int OW, int align, int boundary, double apodize);
int launch_fourier_operator(double* op, int n, int m, int align, int boundary, double apodize, hipStream_t st);
int launch_fourier_resample2d(double* out, const double* in, int nimg, int H, int W, int OH, int OW, int align, int boundary,
                              double apodize, const FourierView& v, hipStream_t st);
int launch_fourier_resample2d(float* out, const float* in, int nimg, int H, int W, int OH, int OW, int align, int boundary,
                              double apodize, const FourierView& v, hipStream_t st);

// (register.hip -- masked cross-correlation, image means, the spline shift -- defines public entry points only; the spline prefilter and
// sampler it shares with rescale.hip are device code, in spline.h.)

// ---- perceptual.hip: the reader study's scores (Gaussian SSIM, MS-SSIM, 3 x 3 high-pass, MSE, high-frequency gain) ------------------------
constexpr int PERCEPTUAL_MAX_RADIUS = INR_PERCEPTUAL_MAX_RADIUS;   // window taps per side: what the tile's halo in LDS holds
constexpr int PERCEPTUAL_MAX_SCALES = INR_PERCEPTUAL_MAX_SCALES;
struct PerceptualView { double *reduce, *partial, *vals, *lx[2], *ly[2]; size_t total; };
PerceptualView perceptual_view(int nimg, int H, int W, int n_scales, void* base);
int perceptual_check(const char* who, int nimg, int H, int W, double sigma, double data_range, int n_scales);
int launch_ssim_gauss(double* ssim, double* mean_cs, float* map, const float* x, const float* y, int nimg, int H, int W, double sigma,
                      double data_range, const PerceptualView& v, hipStream_t st);
int launch_msssim(double* out, double* per_scale, const float* x, const float* y, int nimg, int H, int W, const double* weights,
                  int n_scales, double sigma, double data_range, const PerceptualView& v, hipStream_t st);
int launch_filter3x3(float* out, const float* in, int nimg, int H, int W, const double* k9, hipStream_t st);
int launch_pair_score(double* out, const float* x, const float* y, int nimg, int64_t per_image, int mode, const PerceptualView& v,
                      hipStream_t st);

// ---- cssim.hip: the shift-tolerant SSIM of the RAMS tree (utils/loss.py:131-177) and its gradient ---------------------------------------
int cssim_min_crop();   // the cropped window must hold one 11 x 11 filter window
size_t cssim_workspace_doubles(int nimg, int size, int border, bool grad);
int launch_cssim(double* out, const float* y_true, const float* y_pred, const float* mask, int nimg, int size, int border,
                 int clear_only, double* ws, hipStream_t st);
int launch_cssim_grad(double* loss, float* grad, const float* y_true, const float* y_pred, const float* mask,
                      const float* upstream, int nimg, int size, int border, int clear_only, double* ws, hipStream_t st);

// ---- hybrid_fit.hip -----------------------------------------------------------------------------------------------------------------------
int launch_hybrid_fit(double* params, int* status, int* nfev, double* cost, const double* signals, int64_t n,
                      hipStream_t st);
void set_hybrid_variant(int v);   // key 2

// (pia.hip and erd_siren.hip define public entry points only, and jet.hip little else; their launch families are counted through
// count_launch in api.hip's table like every other -- common.h: LF_PIA_BASE, LF_JET_BASE, and the ERD families at their public ids.)

// ---- jet.hip ------------------------------------------------------------------------------------------------------------------------------
// the jets of the Fourier features [sin p | cos p], p = 2 pi x B^T: out [1 + dt + lap][.][pitch] planes `plane` floats apart (pitch
// = 2m rounded up to 32, pad columns zero).  x != null: the rows x [n_rows][d]; else rows row_begin .. of the grid `shape` [d]
int jet_launch_fourier(float* out, long long plane, int pitch, const float* x, const int64_t* shape, int d, int dt, int lap,
                       int64_t row_begin, int64_t n_rows, const float* B, int m, hipStream_t st);

// ---- wire.hip: the complex-Gabor (WIRE) layers in real arithmetic, f32-input MFMA 32x32x2 -------------------------------------------
constexpr int WIRE_MAX_LAYERS = 9;          // 1 + hidden_layers
struct WirePlan {
    int in_f = 0, H = 0, L = 0, K0 = 0;       // L = hidden (complex) layers; K0 = in_f rounded up to the K block (32)
    long long off[4 * WIRE_MAX_LAYERS + 2];   // inr_wire_param_offsets
    long long total = 0;
};
int wire_check_desc(const char* who, const inr_wire_desc_t* d);      // what inr_wire_forward serves
WirePlan wire_plan(const inr_wire_desc_t* d);
// parameters -> the layers' block images img[l] ([2][H][K0] for l = 0, else [4][H][2H]) and packed biases pb[l] ([4][H]), l <= L
int wire_pack_images(const WirePlan& p, float* const* img, float* const* pb, const float* params, hipStream_t st);
// in [n][K] (K a multiple of 32) times the block image img [Q][H][K] (Q = 2 for the real first layer, else 4), Gabor epilogue:
// out [n][2H] = [out_r | out_i]; stash (nullable) [n][Q H] receives lin_r (, lin_i), orth_r (, orth_i)
int wire_gabor_forward(float* out, float* stash, const float* in, const float* img, const float* pb, int K, int H, int first,
                       int64_t n, float omega, float s2, hipStream_t st);
// G [n][2H] = dZ [n][4H] times the image, read through its transpose imgT [2H][4H]
int wire_input_grad(float* G, const float* dZ, const float* imgT, int H, int64_t n, hipStream_t st);
// dx [n][in_f] (unpadded, any in_f) = dZ0 [n][2H] times the real layer-0 image, read through its transpose imgT0 [in_f][2H]
int wire_first_input_grad(float* dx, const float* dZ0, const float* imgT0, int in_f, int H, int64_t n, hipStream_t st);
// slabs [splits][R][C] = per-split dZ^T X and bslab [splits][R] = per-split column sums of dZ (dZ [n][R], X [n][C])
int wire_param_grad_slabs(float* slabs, float* bslab, const float* dZ, int R, const float* X, int C, int64_t n, hipStream_t st);

// ---- rams.hip (+ rams_train.inc) ---------------------------------------------------------------------------------------------------------
long long rams_param_floats(const inr_rams_desc_t* d);
size_t rams_workspace_floats(const inr_rams_desc_t* d, int B, int H, int W);
int rams_forward_impl(const inr_rams_desc_t* d, const float* params, const float* x, float* out, int B, int H, int W,
                      int clip_round, void* workspace, size_t workspace_bytes, hipStream_t st);   // checks the workspace itself
size_t rams_conv3d_wgrad_ws_floats(long long nvox);
int rams_conv3d_forward(float* y, const float* x, const float* w, const float* bias, int B, int D1, int D2, int D3, int pad,
                        int relu, hipStream_t st);
int rams_conv3d_dgrad_same(float* dx, const float* dy, const float* w, int B, int D1, int D2, int D3, float* ws, hipStream_t st);
int rams_conv3d_wgrad(float* gw, float* gb, const float* x, const float* dy, int B, int D1, int D2, int D3, int pad, float* ws,
                      hipStream_t st);
int rams_conv3d_wgrad_auto(float* gw, float* gb, const float* x, const float* dy, int B, int D1, int D2, int D3, int pad, float* ws,
                           hipStream_t st);
long long rams_train_param_floats(const inr_rams_desc_t* d);
int rams_train_param_offsets(const inr_rams_desc_t* d, int64_t* offsets, int max_layers);
size_t rams_train_workspace_floats(const inr_rams_desc_t* d, int B, int H, int W);
int rams_train_grads(const inr_rams_desc_t* d, const float* raw, float* raw_grad, const float* x, const float* y_true,
                     const float* mask, double* loss, float* pred, int B, int H, int W, void* workspace, size_t workspace_bytes,
                     hipStream_t st);   // checks the workspace itself, before the first launch
extern tune_int g_rams_h3, g_rams_force_lds;   // key 14 (bits 0-1, bit 2)
extern tune_int g_rams_lds_waves;              // key 15
extern tune_int g_rams_epi_fuse;               // key 24
extern tune_int g_rams_pregate_min_vox;        // key 26

// ---- siren_small.hip: the fused small-network fit ---------------------------------------------------------------------------------------
bool small_path_ok(const inr_siren_desc_t* d, int64_t n);
size_t small_workspace_floats(const inr_siren_desc_t* d, int64_t n, long long P);
int small_fit_step(const inr_siren_desc_t* d, const long long* w_off, const long long* b_off, long long P, float* params,
                   float* grads, float* m, float* v, const float* x, const float* target, const float* weight, int64_t n,
                   int64_t step, double lr, double b1, double b2, double eps, float* loss_out, float* ws, hipStream_t st);
bool small_multi_ok(const inr_siren_desc_t* d, int64_t n);
size_t small_multi_workspace_floats(const inr_siren_desc_t* d, int64_t n, long long P);
int small_fit_multi(const inr_siren_desc_t* d, const long long* w_off, const long long* b_off, long long P, float* params,
                    float* grads, float* m, float* v, const float* x, const float* targets, const float* weights, int n_acq,
                    int first_acq, int64_t n, int64_t first_step, int n_steps, double lr, double b1, double b2, double eps,
                    float* losses, float* ws, hipStream_t st);
int small_batch_per_launch(const inr_siren_desc_t* d, int64_t n);
int small_fit_batch(const inr_siren_desc_t* d, const long long* w_off, const long long* b_off, long long P, int n_fits,
                    float* const* params, float* const* grads, float* const* m, float* const* v, const float* x,
                    const float* const* targets, const float* const* weights, const int* n_acq, const int* first_acq, int64_t n,
                    int64_t first_step, int n_steps, double lr, double b1, double b2, double eps, float* const* losses,
                    void* const* ws, hipStream_t st);
extern tune_int g_small_rows;         // key 13
extern tune_int g_small_spin_limit;   // key 17

}  // namespace inr
