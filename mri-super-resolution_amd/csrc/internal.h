// What crosses a translation unit of libinrhip.so, and nothing else: host launchers, planners and the diagnostic switches behind
// inr_debug_set, grouped by the file that defines them.  ONE rule: a unit holds its family's kernels, launchers, workspace view,
// argument checks and, in an extern "C" block at its end, its public entry points; a name is declared here only if a unit other
// than the one that defines it uses it, and everything else in a unit is file-local.  Every .hip file includes this header -- the
// defining one too, so that a declaration that has drifted from its definition fails to compile in the file that is wrong.
// Default arguments live here and nowhere else.  One exception to "file-local": jet_host.h, the host code the two derivative units
// (jet.hip, wire_deriv.hip) share and no other unit includes; it includes this header for them.  (set_error, count_launch, launch_finalize and the profiler hooks are in common.h,
// beside their types; the launch families of every unit are counted through count_launch in api.hip's one table.)
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
constexpr int64_t MAX_ROWS = (1ll << 31) - 256;   // rows of one GEMM call (the entry points of gemm_f32.hip and api.hip check it)
int gemm_build_flags();   // inr_build_flags: this unit's diagnostic macros | hp_build_flags()
int gemm_sine_forward(float* act, float* dact, const float* x, const float* W, const float* b, int64_t n,
                      int in_f, int out_f, float omega, hipStream_t stream, const H3Args* h3 = nullptr);
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
extern tune_int g_hp_grid_cap;                    // key 32: test-only cap on the persistent grids (and on tvsr3d.hip's stride-loop grids)

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
extern tune_int g_reduce_onepass;   // key 25

// ---- metrics.hip: the cL1 loss gradient, which the RAMS training step (rams_train.inc) calls ------------------------------------------
int launch_shift_loss_grad(double* loss, float* grad, const float* y_true, const float* y_pred, const float* mask,
                           const float* upstream, int nimg, int size, int border, double* ws, hipStream_t st);

// ---- hybrid_fit.hip -----------------------------------------------------------------------------------------------------------------------
void set_hybrid_variant(int v);   // key 2

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

// ---- rams.hip (+ rams_train.inc): the switches api.hip's table sets ---------------------------------------------------------------------
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
