/*
 * inrhip.h -- C ABI of libinrhip.so: the MI355X (gfx950) kernels for the INR / SIREN
 * super-resolution fit path of MRIRC/MRI-super-resolution.
 *
 * The reference has no FFI of its own: its boundary is the Python module surface of SRDWI.py /
 * INRmodel.py / nn_mri.py, and all arithmetic is stock PyTorch ops.  Every entry point below
 * therefore replaces a *framework op sequence* of the reference; the file:line of that sequence
 * (relative to /root/reference/implicit-neural-representations) is cited per function.
 * INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *  - plain C: raw DEVICE pointers, int64 sizes, scalar hyper-parameters, a hipStream_t passed as
 *    void* (0 = the null stream).  No torch types, no ownership transfer: the caller allocates every
 *    output and every workspace (size from the matching *_workspace_bytes query).
 *  - every function only ENQUEUES work on `stream` and returns without synchronising.  Everything a call launches goes onto
 *    `stream` itself, in program order: the library owns NO stream and creates no events of its own for ordering (rounds 1-3
 *    forked the parameter-gradient GEMMs onto a library-owned side stream; since round 4 they are one merged launch on
 *    `stream`).  Consequently (a) whatever the caller enqueues on `stream` after the call is ordered behind all of its work,
 *    (b) calls on DIFFERENT streams are not ordered against each other by the library, and (c) the calls contain no
 *    allocation and no host synchronisation, so a sequence of them can be captured into a HIP graph.  TWO documented
 *    exceptions to "no host sync": when inr_siren_fit / inr_siren_fit_cycle / inr_siren_fit_cycle_batch take the persistent
 *    cooperative small-network kernel (hidden 32 / 64, <= 32 input features, one output, few thousand rows) they wait for
 *    `stream` once at the end of the call to read the kernel's completion word(s), and return INR_E_TIMEOUT if a launch
 *    was abandoned (cooperative launches cannot be captured into a graph in any case); and inr_prof_read() waits for the
 *    events it reports on.
 *  - threading / concurrency: entry points may be called concurrently from several host threads on different streams with
 *    DISJOINT output and workspace buffers (read-only inputs may be shared); this is what
 *    drivers.run_volumes(concurrent=k) relies on -- k fits of one process, each on a host thread and a stream of its own,
 *    each with its own parameter / moment / workspace buffers.  One call uses one workspace; the same workspace must not be
 *    in use by two calls that may overlap on the device.  The cooperative small-network kernel needs its whole grid
 *    co-resident: two such launches on different streams at the same time can each hold part of the chip and stall until the
 *    grid barrier's poll limit reports INR_E_TIMEOUT -- run those fits one after the other (run_volumes does), or together
 *    in ONE inr_siren_fit_cycle_batch call (one cooperative grid that carries them all).
 *    Process-global state, all of it safe to touch from several threads, none of it carrying tensor data:
 *      (i)   the thread-local message behind inr_last_error();
 *      (ii)  the event profiler behind inr_prof_* (a mutex; off unless enabled);
 *      (iii) the launch counters behind inr_launch_count (atomics);
 *      (iv)  the workspace stamps that guard INR_REUSE_* flags and the pending inr_siren_forward_train stash: 64 entries
 *            keyed on the workspace ADDRESS (a mutex; least recently used entry replaced).  A stamp says which (n, x,
 *            target, weight) the operand image in that workspace was built from; it cannot know that the caller freed the
 *            workspace and received the same address again -- a caller that recycles workspace memory must not pass
 *            INR_REUSE_* on the first call after doing so;
 *      (v)   the per-device co-residency limits of the cooperative kernel (atomics, computed once per device);
 *      (vi)  the DIAGNOSTIC switches behind inr_debug_set / inr_debug_set_ptr, which select kernel families for A/B
 *            measurements and tests.  They are atomics, but process-wide: flipping one while another thread is enqueueing
 *            changes what that thread launches next (and whether inr_siren_hp_eligible says yes).  A production caller never
 *            touches them; a test harness restores them with inr_debug_reset().
 *  - return value: 0 = ok; negative = invalid argument (INR_E_*); positive = hipError_t.
 *    inr_last_error() returns a thread-local human-readable message for the last failure.
 *  - all tensors are dense row-major fp32.  Linear weights are [out_features][in_features] exactly as
 *    torch.nn.Linear stores them.
 *  - reductions (loss, bias/weight gradients) use fixed-order two-stage sums: no float atomics, so
 *    two runs on the same inputs are bitwise identical.
 */
#ifndef INRHIP_H
#define INRHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INR_ABI_VERSION 1

#define INR_E_INVALID   (-1)  /* null pointer / non-positive size / unsupported shape            */
#define INR_E_WORKSPACE (-2)  /* workspace pointer null or smaller than the *_workspace_bytes query */
#define INR_E_ALIGN     (-3)  /* pointer not 16-byte aligned where the kernel requires it         */
#define INR_E_TIMEOUT   (-4)  /* a persistent kernel abandoned its launch (grid barrier poll limit): outputs of the call are
                                 partly written and must be discarded                                */

typedef struct inr_device_caps {
    int  abi_version;
    int  device;
    int  compute_units;
    int  wavefront_size;
    int  lds_bytes_per_cu;
    int  clock_khz;
    int64_t hbm_bytes;
    char arch[32];          /* "gfx950..." */
} inr_device_caps_t;

/* Description of one SIREN: Siren(in, hidden, hidden_layers, out, first_omega_0, hidden_omega_0)
 * (SRDWI.py:67-85).  Sine layers: 1 + hidden_layers; then the linear head. */
typedef struct inr_siren_desc {
    int   in_features;
    int   hidden_features;
    int   hidden_layers;
    int   out_features;
    float first_omega;
    float hidden_omega;
} inr_siren_desc_t;

/* RAMS multi-image network (multi-image-super-resolution/utils/network.py:91-155): RAMS(scale, filters, kernel_size,
 * channels, r, N).  The kernels are written for filters == 32 and kernel_size == 3 (the reference's only
 * configuration, multi-image-super-resolution/master.py:20-25). */
typedef struct inr_rams_desc {
    int   scale;        /* 3 */
    int   filters;      /* 32 */
    int   kernel_size;  /* 3 */
    int   channels;     /* T = 9 acquisitions per stack */
    int   r;            /* squeeze ratio 8 */
    int   n_rfab;       /* N = 12 */
    float mean;         /* 7433.6436 (network.py:18) */
    float std;          /* 2353.0723 (network.py:19) */
} inr_rams_desc_t;

/* Flat parameter layout used by the fused entry points (network order):
 *   W_0[hidden][in], b_0[hidden], W_1[hidden][hidden], b_1, ..., W_head[out][hidden], b_head[out]
 * Every tensor starts at a multiple of 4 floats (16 B): offsets come from inr_siren_param_offsets. */

int         inr_version(void);
/* 0 for the product build.  Non-zero = a diagnostic build (bit 0: in-kernel time stamps -DINR_STAMPS, bit 1: ablated
 * kernels -DH3_ABLATE, bit 2: padded LDS -DH3_EXTRA_LDS): its timings and, with bit 1, its RESULTS are not the product's.
 * The Python binding refuses such a library unless it was selected explicitly (INR_LIB=...). */
int         inr_build_flags(void);
const char* inr_last_error(void);
int         inr_device_caps(int device, inr_device_caps_t* out);

/* ---- a-1: get_mgrid (SRDWI.py:12-18, nn_mri.py:87-94) ------------------------------------------
 * rows [row_begin, row_begin+n_rows) of the flattened 'ij' meshgrid of linspace(-1,1,shape[a]),
 * last axis fastest; bit-exact with torch.linspace (single-rounding fma rule).  dim<=8. */
int inr_mgrid(float* out, const int64_t* shape, int dim, int64_t row_begin, int64_t n_rows, void* stream);

/* ---- a-3: input_mapping (SRDWI.py:111-116) -----------------------------------------------------
 * out[n][2m] = [sin(2*pi*x @ B^T) | cos(2*pi*x @ B^T)],  x[n][d], B[m][d]. */
int inr_fourier_map(float* out, const float* x, const float* B, int64_t n, int d, int m, void* stream);
/* Same, with x generated in-kernel from the grid (K1+K2 fused: the coordinate grid never reaches HBM;
 * replaces get_mgrid(...).cuda() -> input_mapping at superresDWI.py:125-126). */
int inr_grid_fourier_map(float* out, const int64_t* shape, int dim, int64_t row_begin, int64_t n_rows,
                         const float* B, int m, void* stream);

/* ---- a-4: SineLayer.forward (SRDWI.py:58-59): act = sin(omega*(x W^T + b)) ----------------------
 * x[n][in], W[out][in], b[out] (nullable), act[n][out]; dact (nullable) receives
 * omega*cos(omega*(x W^T + b)) -- the factor autograd multiplies by in backward. */
int inr_sine_layer_forward(float* act, float* dact, const float* x, const float* W, const float* b,
                           int64_t n, int in_features, int out_features, float omega, void* stream);

/* ---- a-10: PerturbNet layers (SRDWI.py:93-109) ---------------------------------------------------------
 * hidden layer:  act = scale*tanh(x W^T + b), dact (nullable) = scale*(1 - tanh^2)   [same GEMM as the sine layer]
 * output layer:  y[n][out] = scale*tanh(a W^T + b) (scale = eps, SRDWI.py:107), dy (nullable) its derivative;
 *                row-dot per output with a wavefront shuffle reduction (out = d = 2..4 columns).
 * The constant acquisition column of SRDWI.py:102-104 is folded into the bias by the caller:
 * b_eff = b + (sample/10) * W[:, in]  (so x stays the [n, in] feature matrix and nothing is concatenated). */
int inr_tanh_layer_forward(float* act, float* dact, const float* x, const float* W, const float* b, int64_t n,
                           int in_features, int out_features, float scale, void* stream);
int inr_linear_tanh_head_forward(float* y, float* dy, const float* a, const float* W, const float* b, int64_t n,
                                 int in_features, int out_features, float scale, void* stream);

/* element-wise out = a*b over `count` floats: dz = grad_out * dact, the first step of a stand-alone
 * SineLayer's backward (what autograd does for torch.sin(omega*z), SRDWI.py:59).  out may alias a or b. */
int inr_mul(float* out, const float* a, const float* b, int64_t count, void* stream);

/* ---- a-5: final nn.Linear (SRDWI.py:75-77,83): y = a W^T + b, optional clamp(min) ---------------
 * (clamp fuses torch.clamp(..., min=0) of superresDWI.py:161; pass use_clamp=0 for the raw head). */
int inr_linear_head_forward(float* y, const float* a, const float* W, const float* b, int64_t n,
                            int in_features, int out_features, int use_clamp, float clamp_min, void* stream);

/* ---- a-6: ((y-t)**2).mean() and its gradient (superresDWI.py:135; weighted: master.py:143-145) ---
 * gy[i] = 2*w[i]*(y[i]-t[i])/count ; *loss = mean(w*(y-t)^2).  w nullable.  count = n*out. */
size_t inr_mse_workspace_bytes(int64_t count);
int inr_mse_loss_grad(float* gy, float* loss, const float* y, const float* t, const float* w,
                      int64_t count, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a-6: backward pieces (what autograd runs for SRDWI.py:58-59,83) -----------------------------
 * head:   dz_last[n][hidden] = (gy[n][out] @ W_head[out][hidden]) * dact_last   (in place over dact ok)
 *         gW_head[out][hidden] = gy^T a_last ; gb_head[out] = colsum(gy)
 *         gb_last[hidden] (nullable, needs dz_last) = colsum(dz_last): the bias gradient of the last sine
 *         layer, produced by the same pass (one fused kernel when out_features == 1). */
size_t inr_head_backward_workspace_bytes(int64_t n, int hidden, int out_features);
int inr_linear_head_backward(float* dz_last, float* gW, float* gb, float* gb_last, const float* gy,
                             const float* a_last, const float* dact_last, const float* W, int64_t n, int hidden,
                             int out_features, void* workspace, size_t workspace_bytes, void* stream);
/* input grad through one sine layer: dz_prev[n][in] = (dz[n][out] @ W[out][in]) * dact_prev[n][in]
 * (dz_prev may alias dact_prev).  With dact_prev == NULL writes the plain product dz @ W.
 * gb_prev[in] (nullable) = colsum(dz_prev), the bias gradient of the layer below, accumulated in the GEMM
 * epilogue; it needs the workspace (otherwise workspace may be NULL). */
size_t inr_sine_layer_backward_input_workspace_bytes(int64_t n, int in_features);
int inr_sine_layer_backward_input(float* dz_prev, float* gb_prev, const float* dz, const float* W,
                                  const float* dact_prev, int64_t n, int in_features, int out_features,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* parameter grads: gW[out][in] = dz^T x ; gb[out] = colsum(dz).  Split over rows + fixed-order reduce. */
size_t inr_linear_param_grad_workspace_bytes(int64_t n, int in_features, int out_features);
int inr_linear_param_grad(float* gW, float* gb, const float* dz, const float* x, int64_t n,
                          int in_features, int out_features, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---- a-7: torch.optim.Adam.step (superresDWI.py:116,138; defaults b=(0.9,0.999), eps=1e-8) ------
 * One launch over `count` contiguous fp32 elements.  bias corrections are computed on the host in
 * double exactly like torch's single-tensor path: step_size = lr/(1-b1^t), denom =
 * sqrt(v)/sqrt(1-b2^t) + eps.  `step` is the 1-based step number. */
int inr_adam_step(float* p, const float* g, float* m, float* v, int64_t count, int64_t step,
                  double lr, double beta1, double beta2, double eps, void* stream);

/* ---- fused SIREN entry points (flat parameter buffer) ------------------------------------------ */
int64_t inr_siren_param_count(const inr_siren_desc_t* desc);      /* padded flat length in floats */
/* offsets[2*(hidden_layers+2)]: (W_l, b_l) float offsets in network order, head last */
int  inr_siren_param_offsets(const inr_siren_desc_t* desc, int64_t* offsets);

/* a-5 + a-9: y[n][out] = head(sine layers(x[n][in])), optional clamp; forward only, no stash. */
size_t inr_siren_forward_workspace_bytes(const inr_siren_desc_t* desc, int64_t n);
int inr_siren_forward(const inr_siren_desc_t* desc, const float* params, const float* x, int64_t n,
                      float* y, int use_clamp, float clamp_min, void* workspace, size_t workspace_bytes,
                      void* stream);

/* a-9: dense re-sampling clamp(INR(input_mapping(get_mgrid(shape), B)), min) -> y[prod(shape)][out]
 * (superresDWI.py:125-126,161-162; superresHybrid.py:103-104,119).  Grid + Fourier features are
 * generated chunk by chunk in the workspace (never the whole [N_test,2m] feature matrix).
 * B == NULL means raw coordinates feed the network (nn_mri path, master.py:149-153). */
size_t inr_siren_reconstruct_workspace_bytes(const inr_siren_desc_t* desc, int64_t chunk_rows);
int inr_siren_reconstruct(const inr_siren_desc_t* desc, const float* params, const int64_t* shape, int dim,
                          const float* B, int m, float* y, int use_clamp, float clamp_min,
                          int64_t chunk_rows, void* workspace, size_t workspace_bytes, void* stream);

/* a-8: `n_steps` full-batch fit steps (superresDWI.py:132-138; superresHybrid.py:109-114):
 * forward with stash -> MSE (+optional weights) -> backward -> Adam, all enqueued on `stream`,
 * no host sync.  params/grads/m/v are flat buffers of inr_siren_param_count floats.  losses[n_steps]
 * (device, nullable) receives the loss of every step.  first_step is the 1-based Adam step of the
 * first iteration (so a fit can be continued).
 * Arithmetic: when every sine layer is a multiple of 32 wide, the three dense contractions of a step run on the fp16
 * matrix cores with hi/lo-split operands (three fp16 products per fp32 product, fp32 accumulation, power-of-two
 * tensor scales from exact on-device maxima) -- fp32-class accuracy, same parity tolerances; otherwise
 * (and in every stand-alone layer entry point above) on the f32-input MFMA.  The workspace holds the fp16 weight
 * planes of that path; size it with the query function. */
size_t inr_siren_fit_workspace_bytes(const inr_siren_desc_t* desc, int64_t n);
int inr_siren_fit(const inr_siren_desc_t* desc, float* params, float* grads, float* m, float* v,
                  const float* x, const float* target, const float* weight, int64_t n,
                  int64_t first_step, int n_steps, double lr, double beta1, double beta2, double eps,
                  float* losses, void* workspace, size_t workspace_bytes, void* stream);

/* a-11 / master.py:137-148: the same loop when the target (and weight) image changes every step -- `targets` and
 * `weights` (nullable) hold n_acq images of n*out_features floats back to back, step `it` fits image
 * (first_acq + it) % n_acq.  inr_siren_fit is the n_acq = 1 case.  For small networks (hidden 32 or 64, <= 32 inputs,
 * one output, n <= 16,384) all steps run inside ONE persistent cooperative launch per 64 steps (grid barriers between
 * the backward pass, the fixed-order gradient reduction + Adam, and the next forward): no launch per step at all. */
int inr_siren_fit_cycle(const inr_siren_desc_t* desc, float* params, float* grads, float* m, float* v,
                        const float* x, const float* targets, const float* weights, int n_acq, int first_acq,
                        int64_t n, int64_t first_step, int n_steps, double lr, double beta1, double beta2, double eps,
                        float* losses, void* workspace, size_t workspace_bytes, void* stream);

/* Several independent fits of ONE shape at once (master.py: one small network per gradient direction, per case, per seed).
 * Fit i has its own params[i], grads[i], m[i], v[i], targets[i] / weights[i] ([n_acq[i]][n*out_features], weights and any of
 * its entries nullable), acquisition cycle (n_acq[i], first_acq[i]), losses[i] ([n_steps], array and entries nullable) and
 * workspaces[i] (each of workspace_bytes >= inr_siren_fit_workspace_bytes(desc, n)); x, n, the step schedule and the Adam
 * constants are shared.  Pointer arrays are HOST arrays of device pointers.
 * Contract: the call is equivalent, bit for bit, to calling inr_siren_fit_cycle for i = 0 .. n_fits-1 in order on the same
 * stream, for every network shape and every inr_debug_set setting.  Where the persistent cooperative kernel serves the shape
 * and at least two fits' grids are co-resident, the fits share launches: ONE cooperative launch per 64 steps carries up to
 * 16 of them (fit k owns its own blocks, its own grid barriers and its own reduction), further groups follow on `stream`.
 * Like that path it waits for `stream` once at the end to read every fit's completion word (INR_E_TIMEOUT names the fits
 * whose launch was abandoned) and cannot be captured into a HIP graph.  Validation (INR_E_INVALID, before any device work):
 * n_fits >= 1, no null array or required entry, no params buffer or workspace used twice, 16-byte aligned x / params /
 * grads / workspaces, 0 <= first_acq[i] < n_acq[i]. */
int inr_siren_fit_cycle_batch(const inr_siren_desc_t* desc, int n_fits, float* const* params, float* const* grads,
                              float* const* m, float* const* v, const float* x, const float* const* targets,
                              const float* const* weights, const int* n_acq, const int* first_acq, int64_t n,
                              int64_t first_step, int n_steps, double lr, double beta1, double beta2, double eps,
                              float* const* losses, void* const* workspaces, size_t workspace_bytes, void* stream);

/* (e) one fit split over several GPUs: forward + loss + backward of THIS rank's row shard, no optimizer.
 * The mean of the loss runs over count_total elements (0 = n*out_features, i.e. an unsplit fit), so gradients and
 * losses of the shards add up to the full-batch step: all-reduce(sum) `grads` (flat, inr_siren_param_count floats)
 * and `loss`, then call inr_adam_step on every rank.  Workspace: inr_siren_fit_workspace_bytes(desc, n). */
#define INR_REUSE_INPUT_IMAGE  1   /* x, n and `workspace` are those of the previous call on this workspace: keep the
                                      operand image of x and its scale (skips two passes over x per call) */
#define INR_REUSE_TARGET_STATS 2   /* target / weight are those of the previous call: keep their maxima */
int inr_siren_loss_grad(const inr_siren_desc_t* desc, const float* params, float* grads, const float* x,
                        const float* target, const float* weight, int64_t n, int64_t count_total, float* loss,
                        void* workspace, size_t workspace_bytes, void* stream);
/* the same with `flags` (INR_REUSE_*): a fit whose rows are split over GPUs calls this once per step on unchanged inputs --
 * without the flags every call re-measures and re-converts x (0.25 ms at 524,288 rows x 256 features).  The caller vouches for
 * "unchanged": same x contents, same n, same workspace, nothing else written to it in between. */
int inr_siren_loss_grad_ex(const inr_siren_desc_t* desc, const float* params, float* grads, const float* x,
                        const float* target, const float* weight, int64_t n, int64_t count_total, float* loss,
                        void* workspace, size_t workspace_bytes, int flags, void* stream);

/* (f) the reference's OWN loop, unmodified (superresDWI.py:132-138): `out = INR(x)` -> torch forms the loss -> `loss.backward()`
 * -> `torch.optim.Adam.step()`.  The autograd Function behind `Siren.forward` (replaces SRDWI.py:87-91 + autograd's backward of
 * it) calls these two instead of the layer-by-layer entry points when inr_siren_hp_eligible(desc) != 0:
 *   inr_siren_forward_train  y[n] = network(x) on the pre-split kernels of the fused fit, every layer's stash kept in `workspace`
 *                            (the last sine layer stashes z + b only); flags: INR_REUSE_INPUT_IMAGE as above.
 *   inr_siren_backward_train grads (flat, network order, inr_siren_param_count floats; every element written) = d(sum_r gy[r] y[r])
 *                            / d params from the stash of the LAST inr_siren_forward_train on this workspace (INR_E_INVALID when
 *                            there is none, or n differs); gy = dL/dy [n] as autograd hands it over.  `params` must still hold
 *                            the values the forward ran on.  One backward per forward.
 * Workspace: inr_siren_fit_workspace_bytes(desc, n).  Both only enqueue.  (What a workspace holds -- a pending forward, an operand
 * image for the INR_REUSE_* flags -- is remembered on the host for the 64 most recently used workspaces of the process: the least recently used entry makes room.) */
int inr_siren_hp_eligible(const inr_siren_desc_t* desc);
int inr_siren_forward_train(const inr_siren_desc_t* desc, const float* params, const float* x, float* y, int64_t n,
                            void* workspace, size_t workspace_bytes, int flags, void* stream);
int inr_siren_backward_train(const inr_siren_desc_t* desc, const float* params, float* grads, const float* gy, int64_t n,
                             void* workspace, size_t workspace_bytes, void* stream);

/* (g) the voxel-footprint forward model (csrc/footprint.hip): a datum is not a point sample of the network but a
 * weighted average over K sub-sample positions x_i + delta_k,
 *     p_i = sum_k fw[k] y[i K + k],   loss = inv_count sum_i wt_i (p_i - t_i)^2,   inv_count = 1 / (count_total ? count_total : n).
 * Sub-sample k of datum i is row i K + k (sub-sample minor) everywhere.  Limits: 1 <= K <= INR_FOOTPRINT_MAX_SAMPLES, 1 <= d <= 4,
 * n >= 1, n K below 2^31 - 256 (the rows of one GEMM call).  Everything is validated before any device work: null pointer or bad
 * n / K / d INR_E_INVALID, short workspace INR_E_WORKSPACE, misaligned workspace / params / grads / x_sub INR_E_ALIGN.  Workspaces
 * are counted in floats.  All entries only enqueue; none uses float atomics, so repeated calls are bit-equal.
 *   expand     out[(i K + k) d + a] = x[i d + a] + offsets[k d + a]: one fp32 addition (features then come from the Fourier map of a-3)
 *   reduce     pred[i] = p_i, ONE fma chain over ascending k starting from 0
 *   loss_grad  p_i by that same chain (the same bits; stored to `pred` when it is not null), r = p_i - t_i,
 *              gy[i K + k] = fw[k] (2 wt_i r inv_count) (wt null: 1), *loss = inv_count sum_i wt_i r^2 from per-block partials in a fixed
 *              grid.  count_total (0 = n, else >= n): the divisor when the call sees one row shard of a larger fit, as in (e).
 *              Workspace: the planner's floats, 16-byte aligned.
 *   fit        n_steps full-batch Adam steps enqueued by one call, no host read.  x_sub [n K][in_features] are the features of the
 *              sub-samples, target / weight (nullable) [n], fw [K].  Per step: the training forward of (f) on the n K rows (the first
 *              step of EVERY call re-images x_sub, later steps of the call keep the image), loss_grad, the backward of (f),
 *              the Adam step of inr_adam_step with step number first_step + it (first_step >= 1).  losses (nullable) [n_steps].
 *              Served: exactly what inr_siren_hp_eligible(desc) serves, asked per call (it depends on the diagnostic switches);
 *              anything else is INR_E_INVALID, and the planner returns 0 for it (as for a bad n / K).
 *              Workspace, every region 16-byte aligned: the fit workspace of n K rows | y [n K] | gy [n K] | the loss partials. */
#define INR_FOOTPRINT_MAX_SAMPLES 64
int inr_footprint_expand(float* out, const float* x, const float* offsets, int64_t n, int d, int K, void* stream);
int inr_footprint_reduce(float* pred, const float* y, const float* fw, int64_t n, int K, void* stream);
int64_t inr_footprint_loss_workspace_floats(int64_t n);
int inr_footprint_loss_grad(float* gy, float* loss, float* pred, const float* y, const float* t, const float* wt, const float* fw,
                            int64_t n, int K, int64_t count_total, void* workspace, int64_t workspace_floats, void* stream);
int64_t inr_siren_fit_footprint_workspace_floats(const inr_siren_desc_t* desc, int64_t n, int K);
int inr_siren_fit_footprint(const inr_siren_desc_t* desc, float* params, float* grads, float* m, float* v, const float* x_sub,
                            const float* target, const float* weight, const float* fw, int64_t n, int K, int64_t first_step,
                            int n_steps, double lr, double beta1, double beta2, double eps, float* losses, void* workspace,
                            int64_t workspace_floats, void* stream);

/* ---- a-12: end-of-fit metrics on the device (fp64 accumulation, fixed-order reductions) -----------------
 * workspace for all three image metrics: inr_metric_workspace_bytes(n_images).
 * inr_psnr:   out[b] (double) = 10*log10(data_range^2 / mean((x_b - y_b)^2)); x, y are [n_images][per_image] fp32.
 *             (the definition of skimage.metrics.peak_signal_noise_ratio, imported at master.py:14)
 * inr_ssim2d: out[b] (double) = skimage-0.20 structural_similarity(x_b, y_b, data_range) with default arguments
 *             (uniform win x win window, sample covariance, K1=.01, K2=.03, border crop) on [n_images][H][W] fp32;
 *             use_mask != 0 multiplies both images by (x > mask_thr) first -- the protocol of
 *             superresDWI.py:183-186.
 * inr_adc_map: calculate_ADC (SRDWI.py:118-130): out[p] = clip(-slope of lstsq(log(data[p][:] + 1e-7) ~ b/1000), -10, 3)
 *             for data [n_pixels][n_b] fp32, bvals [n_b] fp32 (n_b <= 32). */
size_t inr_metric_workspace_bytes(int n_images);
int inr_psnr(double* out, const float* x, const float* y, int n_images, int64_t per_image, double data_range,
             void* workspace, size_t workspace_bytes, void* stream);
int inr_ssim2d(double* out, const float* x, const float* y, int n_images, int height, int width, int win,
               double data_range, int use_mask, float mask_thr, void* workspace, size_t workspace_bytes,
               void* stream);
int inr_adc_map(float* out, const float* data, const float* bvals, int64_t n_pixels, int n_b, void* stream);

/* ---- a-15 / (f)-4: RAMS training step (utils/training.py:193-209 train_step; utils/loss.py:26-75 l1_loss; weight
 * normalisation utils/network.py:29-35).  Parameters in the reference's own variables ("raw" layout): per layer, in graph
 * order, v [taps * cin][cout] (the TensorFlow kernel [k..., cin, cout] flattened), g [cout], b [cout], every segment padded to
 * 4 floats -- inr_rams_train_param_offsets returns the three offsets per layer (and the layer count).
 * inr_rams_train_grads: forward (every intermediate kept) -> per-image cL1 loss[b] (double) -> d(sum_b loss[b]) / d params
 * into `grads` (same layout); `pred` (nullable) receives the un-clipped prediction [B][scale*H][scale*W].
 * x [B][H][W][9] fp32, y_true / mask [B][scale*H][scale*W] fp32, H == W.
 * inr_rams_train_step: the same, then Adam in Keras' form (p -= lr sqrt(1-b2^t)/(1-b1^t) m / (sqrt(v) + eps)). */
int64_t inr_rams_train_param_count(const inr_rams_desc_t* desc);
int     inr_rams_train_param_offsets(const inr_rams_desc_t* desc, int64_t* offsets, int max_layers);
size_t  inr_rams_train_workspace_bytes(const inr_rams_desc_t* desc, int batch, int height, int width);
int inr_rams_train_grads(const inr_rams_desc_t* desc, const float* params, float* grads, const float* x, const float* y_true,
                         const float* mask, double* loss, float* pred, int batch, int height, int width, void* workspace,
                         size_t workspace_bytes, void* stream);
int inr_rams_train_step(const inr_rams_desc_t* desc, float* params, float* grads, float* m, float* v, const float* x,
                        const float* y_true, const float* mask, double* loss, int batch, int height, int width, int64_t step,
                        double lr, double beta1, double beta2, double eps, void* workspace, size_t workspace_bytes, void* stream);

/* ---- (f)-2: per-voxel acquisition combinations (SRDWI.py:143-152 calculate_combinations, mapped over all voxels by a
 * 32-process pool at superresDWI.py:57-76).  raw_b0 [n_voxels], raw_bk [n_voxels][nk] (k = 1..3) fp32 ->
 * out [n_voxels][4][K], K = n1*n2*n3, combination index in itertools.product order (the last b-value's index fastest). */
int inr_acquisition_products(float* out, const float* raw_b0, const float* raw_b1, const float* raw_b2, const float* raw_b3,
                             int64_t n_voxels, int n1, int n2, int n3, void* stream);

/* ---- (f)-3: the spline baseline every SSIM row is reported against (superresDWI.py:172-191) -----------------------
 * skimage.transform.rescale(img, s, anti_aliasing=True) with its default order (1) for s >= 1: skimage 0.20 hands this
 * to scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True); the anti-aliasing filter has sigma 0 when up-scaling.
 * in [n_images][H][W] fp32 -> out [n_images][OH][OW] fp32; coordinates and weights in double. */
int inr_rescale2d_linear(float* out, const float* in, int n_images, int height, int width, int out_height, int out_width,
                         void* stream);

/* ---- (f)-3: skimage 0.20 resize for 2-D images: down-scaling with the anti-aliasing Gaussian, orders 1 and 3 --------------------
 * Replaces rescale(x, .5, anti_aliasing=True) of prepare_qual_images.py:152,198,207,267 (order 1, mode 'reflect') and
 * rescale(X, scale=3, order=3, mode='edge', anti_aliasing=False, multichannel=True, preserve_range=True) of
 * multi-image-super-resolution/utils/preprocessing.py:271-294 (bicubic), through the scipy calls skimage makes:
 * ndi.gaussian_filter(img, max(0, (f - 1)/2), mode=M) when anti_aliasing != 0, f = in/out per axis (radius int(4 sigma + .5), at most
 * INR_RESCALE_MAX_RADIUS: INR_E_INVALID beyond), then ndi.zoom(., 1/f, order, mode=M, grid_mode=True) -- order 3 with scipy's
 * mirror-start B-spline prefilter, behind a 12-sample edge pad for M = 'nearest' -- then skimage's clip to the input's range.
 * mode: INR_RESCALE_REFLECT (skimage 'reflect' = scipy 'mirror') or INR_RESCALE_EDGE ('edge' = 'nearest'); order: 1 or 3.
 * in [n_images][H][W] fp32 -> out [n_images][OH][OW] fp32, fp64 arithmetic; every size 1..INR_RESCALE_MAX_LINE.
 * clip_group: 0 = no clip; else n_images is a multiple of it and every run of clip_group consecutive images is clamped to the
 * minimum and maximum of its own inputs (the images of one skimage call: 1 for a 2-D call, T for an (H, W, T) item of bicubic).
 * workspace: inr_rescale2d_workspace_doubles(...) doubles (the filtered plane, the padded coefficient plane, the min/max slots),
 * 16-byte aligned; 0 for arguments inr_rescale2d would refuse.  Plain launches, fixed-order reductions: calls are bit-equal.
 * inr_rescale2d_linear below is unchanged and stays the path of up-scaling calls. */
#define INR_RESCALE_REFLECT 0
#define INR_RESCALE_EDGE 1
#define INR_RESCALE_MAX_RADIUS 64
#define INR_RESCALE_MAX_LINE 4096
int64_t inr_rescale2d_workspace_doubles(int n_images, int height, int width, int order, int mode);
int inr_rescale2d(float* out, const float* in, int n_images, int height, int width, int out_height, int out_width, int order,
                  int mode, int anti_aliasing, int clip_group, double* workspace, int64_t workspace_doubles, void* stream);

/* ---- register_imgset of the multi-image tree (multi-image-super-resolution/utils/preprocessing.py:138-161) --------------------------
 * Per image of a set: the masked normalised cross-correlation against the set's clearest image (masked_register_translation, :155;
 * Padfield 2012) and the cubic-spline scipy.ndimage.shift of the image (:156, 'reflect') and of its quality mask (:157, 'constant').
 * Images and masks are [n_sets][T][H][W] fp32 (a mask pixel is set where it is != 0), arithmetic is fp64.  Plain launches, one thread
 * per displacement in a fixed pixel order, fixed-order reductions, no floating-point atomics: repeated calls are bit-equal.
 *
 * inr_image_means (:149, and the clearances of select_T_images, :188): means [n_sets][T] = mean over H x W of each image (pass the
 * masks); argmax (nullable) [n_sets] DEVICE ints = np.argmax of each set's means, the first maximum.
 *
 * inr_masked_xcorr (:155): image t of set s against image ref_index[s] (DEVICE ints, clamped to 0..T-1) of the same set, with the one
 * mask m of image t on both sides, as skimage does when target_mask is None.  For every displacement d with |dy| <= max_dy,
 * |dx| <= max_dx (H - 1, W - 1 is the reference's full search) pixel p of ref pairs with pixel p - d of x, and the pairs with m(p)
 * and m(p - d) set give n, num = S_ab - S_a S_b / n, da = max(S_aa - S_a^2 / n, 0), db likewise, den = sqrt(da db) (all 0 for n = 0);
 * tol = 1e3 2^-52 max den; C = clip(num / den, -1, 1) where den > tol, else 0; C = 0 where n < overlap_ratio max n.  The window only
 * limits which displacements are evaluated: max den and max n are taken OVER THE WINDOW.  Per image: shifts [.][2] = the mean
 * (dy, dx) of every d with C(d) == max C -- the translation to apply to x, scipy.ndimage.shift's argument --, peak = max C, n_max =
 * the number of such d; map (nullable) [n_sets T][2 max_dy + 1][2 max_dx + 1] doubles = C, d = (-max_dy, -max_dx) first.
 * 1 <= H, W <= INR_XCORR_MAX_SIDE, n_sets T <= 65535, 0 <= overlap_ratio <= 1.  workspace: inr_masked_xcorr_workspace_doubles(...)
 * doubles (six sums per displacement and image), 16-byte aligned; 0 for arguments that would be refused, and every refusal comes
 * before any device work.
 *
 * inr_shift2d (:156-157): scipy.ndimage.shift(in[b], shifts[b], order=3, mode, cval) as scipy 1.15 computes it: spline_filter with
 * the half-sample-symmetric start for 'reflect' and the 'mirror' one for 'constant', the four B-spline weights per axis at o - s, taps
 * beyond the line mapped by 'reflect' (d c b a | a b c d | d c b a), for 'constant' by 'mirror'; in 'constant' an output whose source
 * coordinate leaves [0, n - 1] on either axis is cval exactly.  in / out [n_images][H][W] fp32 (the fp64 result rounded once), shifts
 * [n_images][2] DEVICE doubles (dy, dx) -- inr_masked_xcorr's output, no host read in between; a shift of 1e9 or more, or NaN,
 * gives NaN.  H, W <= INR_RESCALE_MAX_LINE.  workspace: inr_shift2d_workspace_doubles(...) doubles (the coefficient plane), 16-byte
 * aligned; 0 for arguments that would be refused, before any device work. */
#define INR_SHIFT_REFLECT 0
#define INR_SHIFT_CONSTANT 1
#define INR_XCORR_MAX_SIDE 4096
int inr_image_means(double* means, int* argmax, const float* images, int n_sets, int T, int height, int width, void* stream);
int64_t inr_masked_xcorr_workspace_doubles(int n_sets, int T, int height, int width, int max_dy, int max_dx);
int inr_masked_xcorr(double* shifts, double* peak, int* n_max, double* map, const float* images, const float* masks,
                     const int* ref_index, int n_sets, int T, int height, int width, int max_dy, int max_dx, double overlap_ratio,
                     double* workspace, int64_t workspace_doubles, void* stream);
int64_t inr_shift2d_workspace_doubles(int n_images, int height, int width, int mode);
int inr_shift2d(float* out, const float* in, const double* shifts, int n_images, int height, int width, int mode, double cval,
                double* workspace, int64_t workspace_doubles, void* stream);

/* ---- (f)-3: the through-plane spline baseline (SRDWI.py:132-141 resize_array, used at superresDWI.py:231) -------------------
 * scipy.interpolate.interp1d(linspace(0, 1, n_in), y, kind='cubic') evaluated at linspace(0, 1, n_out): make_interp_spline(k=3),
 * not-a-knot end conditions, fp64 throughout.  in [n_lines][n_in] -> out [n_lines][n_out] (the last axis is contiguous:
 * arr[X, Y, Z] as the reference passes it).  n_out == 1 gives y[0]; n_out < n_in down-samples.  4 <= n_in <= 8192 (scipy refuses
 * n_in < 4 too: INR_E_INVALID), 1 <= n_lines < 2^31, n_out >= 1; all checked before any device work.
 * workspace: inr_resize_z_cubic_workspace_bytes(n_lines, n_in) (the per-line spline coefficients). */
size_t inr_resize_z_cubic_workspace_bytes(int64_t n_lines, int n_in);
int inr_resize_z_cubic(double* out, const double* in, int64_t n_lines, int n_in, int n_out, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---- Fourier re-sampling: k-space zero-fill (up) and truncation (down), the interpolation an MR scanner applies ---------
 * No counterpart in the reference, whose only interpolation baseline is skimage's spline; the definition is scipy.signal.resample's.
 * A line x[0..n) becomes y = A x, A [m][n]:
 *   A[i][j] = (1/n) sum_{k = 0..K} c_k w(k) cos(2 pi k (p_i - j) / n),  L = min(n, m), K = floor(L/2),  p_i = i n/m + delta
 *   c_0 = 1, c_k = 2 for 0 < k < L/2; at k = L/2 of an even L: 1 if L == n (the input's Nyquist bin), 2 if L == m < n (both bins folded).
 * align:    INR_FOURIER_SAMPLE  delta = 0: sample 0 stays on sample 0, the grid of a decimation (scipy.signal.resample);
 *           INR_FOURIER_CENTER  delta = (n/m - 1)/2: pixel centres, the grid of skimage's rescale.
 * apodize:  alpha in [0, 1], a Tukey window over the kept band: r = k / (L/2), w = 1 for r <= 1 - alpha, else
 *           (1 + cos(pi (r - 1 + alpha) / alpha)) / 2.  0 = no window, 1 = Hann.
 * boundary: INR_FOURIER_PERIODIC  the above;
 *           INR_FOURIER_MIRROR    the periodic operator E of the mirrored line, folded back onto the n samples, its first m rows.  SAMPLE:
 *           the line [x, x[n-2:0:-1]] of period P = 2n - 2, E: P -> P m/n, A[:, j] = E[:, j] + E[:, P - j] for 0 < j < n - 1 -- needs
 *           n >= 2 and (2n - 2) m divisible by n (INR_E_INVALID otherwise).  CENTER: [x, x[::-1]] of period 2n, E: 2n -> 2m,
 *           A[:, j] = E[:, j] + E[:, 2n - 1 - j], any n and m.
 * Rows of A sum to 1.  Every line length is 1..INR_FOURIER_MAX_LINE.  Two dimensions are the two axes in turn, Y = A_rows X A_cols^T.
 *
 * inr_fourier_operator: op [m][n] DEVICE doubles = A; one thread per entry, every phase reduced exactly in int64 before cospi, the terms
 * added in ascending k.
 * inr_fourier_resample2d: in [n_images][H][W] -> out [n_images][OH][OW] (out must not overlap in), fp64; the _f32 form reads and writes
 * fp32 with fp64 inside and rounds once.  Each axis is one launch of a batched fp64 GEMM on v_mfma_f64_16x16x4_f64 (fixed K order, no
 * atomics: calls are bit-equal); an axis with m == n, INR_FOURIER_SAMPLE and apodize == 0 is skipped and its data pass through bit for
 * bit; so is an axis of one sample that stays one (its operator is [1] in every mode, and the mirror rule does not apply to it: the 1-D
 * form is a batch of 1 x n images).  n_images == 0 succeeds and launches nothing; n_images max(H, OH) < 2^36.
 * workspace: inr_fourier_resample_workspace_doubles(...) doubles (the two operators and the plane between the two passes), 16-byte
 * aligned; 0 for sizes that would be refused.  Every refusal comes before any device work. */
#define INR_FOURIER_SAMPLE 0
#define INR_FOURIER_CENTER 1
#define INR_FOURIER_PERIODIC 0
#define INR_FOURIER_MIRROR 1
#define INR_FOURIER_MAX_LINE 1024
int inr_fourier_operator(double* op, int n, int m, int align, int boundary, double apodize, void* stream);
int64_t inr_fourier_resample_workspace_doubles(int n_images, int height, int width, int out_height, int out_width);
int inr_fourier_resample2d(double* out, const double* in, int n_images, int height, int width, int out_height, int out_width, int align,
                           int boundary, double apodize, double* workspace, int64_t workspace_doubles, void* stream);
int inr_fourier_resample2d_f32(float* out, const float* in, int n_images, int height, int width, int out_height, int out_width,
                               int align, int boundary, double apodize, double* workspace, int64_t workspace_doubles, void* stream);

/* ---- model-based super-resolution with a TV / Huber prior: the variational comparator of the fitted networks ------------
 * No counterpart in the reference.  Images are [n_images][H][W] (HR) and [n_images][h][w] (LR), H = f0 h, W = f1 w, 1 <= f0, f1 <=
 * INR_TVSR_MAX_FACTOR (1 x 1: denoising), H, W <= INR_TVSR_MAX_SIDE.  `kernel` is a HOST array k [f0][f1] of finite doubles that sum to
 * 1 (to 1e-9): 1 / (f0 f1) is the block mean, the delta at (0, 0) the decimation (LR sample j on HR sample f j).
 *   (A x)[i][j] = sum_{a, b} k[a][b] x[f0 i + a][f1 j + b] (the terms added in ascending (a, b)),  A^T r spreads k[a][b] r[i][j],
 *   A A^T = |k|^2 I;  grad: forward differences, zero last row / column;  div = -grad^T.
 * inr_block_apply2d: out [n][h][w] = A in.  inr_block_adjoint2d: out [n][H][W] = A^T in.  fp64, out must not overlap in.
 * inr_tvsr_solve2d: out [n][H][W] = n_iter iterations of Chambolle-Pock (tau = sigma = 1/sqrt(8)) on
 *   min_x 1/2 sum_i w_i ((A x)_i - y_i)^2 + lambda sum_j H_alpha(|(grad x)_j|),  H_0(t) = t,  H_alpha(t) = t^2 / (2 alpha) for t <= alpha,
 *   t - alpha / 2 above, from x = xbar = x0, p = 0:
 *     p <- (p + sigma grad(xbar)) / (1 + sigma alpha / lambda);  p <- p / max(1, |p| / lambda)   (lambda == 0: p = 0)
 *     v <- x + tau div(p);  x' <- v - A^T(c (A v - y)), c_i = tau w_i / (1 + tau w_i |k|^2);  xbar <- 2 x' - x;  x <- x'
 *   y [n][h][w]; weight [n][h][w] or null (= 1; must be >= 0 and finite -- device data, not checked; 0 is a missing datum, whose y is
 *   never used); x0 [n][H][W] or null (block replication of y).  energy / change [n] DEVICE doubles or null: the objective at the
 *   returned image (reduced in a fixed order: no float atomics, calls are bit-equal) and max |x' - x| of the last iteration (0 for
 *   n_iter == 0, which returns x0).  ONE launch, no host read: one workgroup per image runs all iterations with workgroup barriers
 *   only; a batch larger than the CU count is queued.  fp64 throughout; the _f32 form reads y / weight / x0 and writes out as fp32,
 *   with fp64 inside, and rounds once (energy is that of the fp64 image).  n_images == 0 succeeds and launches nothing.
 * workspace: inr_tvsr_workspace_doubles(n_images, H, W) doubles (the state x | xbar | p0 | p1 of every image), 16-byte aligned; 0 for
 * sizes that would be refused.  Refusals, all before any device work: INR_E_INVALID (null out / y / kernel, n_images < 0, factors or
 * sizes out of range, H or W no multiple of its factor, n_iter < 0, a negative or non-finite lambda / alpha, a kernel that is not
 * finite or does not sum to 1), INR_E_WORKSPACE (null or short workspace), INR_E_ALIGN (workspace off a 16-byte boundary). */
#define INR_TVSR_MAX_FACTOR 8
#define INR_TVSR_MAX_SIDE 1024
int inr_block_apply2d(double* out, const double* in, int n_images, int height, int width, int f0, int f1, const double* kernel,
                      void* stream);
int inr_block_adjoint2d(double* out, const double* in, int n_images, int height, int width, int f0, int f1, const double* kernel,
                        void* stream);
int64_t inr_tvsr_workspace_doubles(int n_images, int height, int width);
int inr_tvsr_solve2d(double* out, double* energy, double* change, const double* y, const double* weight, const double* x0, int n_images,
                     int height, int width, int f0, int f1, const double* kernel, double lambda, double alpha, int n_iter,
                     double* workspace, int64_t workspace_doubles, void* stream);
int inr_tvsr_solve2d_f32(float* out, double* energy, double* change, const float* y, const float* weight, const float* x0, int n_images,
                         int height, int width, int f0, int f1, const double* kernel, double lambda, double alpha, int n_iter,
                         double* workspace, int64_t workspace_doubles, void* stream);

/* ---- the same on volumes: a slice profile in the operator, a 3-D prior, one volume over many workgroups ----------------
 * Volumes are [n_volumes][D][H][W] (HR) and [n_volumes][d][h][w] (LR), D = f0 d, H = f1 h, W = f2 w, factors 1 .. INR_TVSR_MAX_FACTOR,
 * D, H, W <= INR_TVSR_MAX_SIDE; indices are 64-bit.  k0 [f0] (the slice profile), k1 [f1], k2 [f2] are HOST arrays of finite doubles,
 * each summing to 1 (to 1e-9); the block kernel is k[a][b][c] = (k1[b] * k2[c]) * k0[a], formed in fp64 in that order.
 *   (A x)[l][i][j] = sum_{a, b, c} k[a][b][c] x[f0 l + a][f1 i + b][f2 j + c] (the terms added in ascending (a, b, c)),  A A^T = |k|^2 I
 *   with |k|^2 summed over the formed table in memory order;  grad = (g0 d0, g1 d1, g2 d2): forward differences along slice / row /
 *   column with a zero last plane / row / column, scaled by the HOST weights grad_weights = {g0, g1, g2}, finite and >= 0 (the voxel
 *   spacing: g0 = in-plane spacing / slice spacing);  div = -grad^T.
 * inr_tvsr3d_block_apply: out [n][d][h][w] = A in.  inr_tvsr3d_block_adjoint: out [n][D][H][W] = A^T in.  fp64, one launch, out must not
 *   overlap in.
 * inr_tvsr3d_solve: out = n_iter iterations of the Chambolle-Pock iteration of inr_tvsr_solve2d on
 *   min_x 1/2 sum_i w_i ((A x)_i - y_i)^2 + lambda sum_j H_alpha(sqrt((g1 d1 x)_j^2 + (g2 d2 x)_j^2 + (g0 d0 x)_j^2))
 *   with tau = sigma = 1 / sqrt(4 sum g_a^2), the sum in the order (1, 2, 0) over the axes whose HR extent exceeds 1 (a zero sum: the
 *   prior vanishes -- lambda = 0, tau = 1 / sqrt(8)).  Wherever the 2-D iteration combines its two axes this one combines row, column,
 *   then slice: div p = + g1 p1[e] - g1 p1[e - W] + g2 p2[e] - g2 p2[e - 1] + g0 p0[e] - g0 p0[e - HW], |q| = sqrt((q1^2 + q2^2) +
 *   q0^2); so D == 1 or g0 == 0 (with g1 = g2 = 1) is inr_tvsr_solve2d of every slice with the kernel k1[b] * k2[c], bit for bit.
 *   Op sequence: init (x = xbar = x0 or the block replication of y, p = 0); per iteration a dual launch (thread per voxel; skipped
 *   for lambda == 0) and a primal launch (workgroup per tile of whole LR blocks); a final launch (the result, the objective's
 *   partials) and a fixed-order finish (energy, change).  Plain launches on `stream`, no host read, no float atomics: calls are
 *   bit-equal on any stream and at any place in a batch.  y, weight, x0, energy, change: as for inr_tvsr_solve2d.  The _f32 form
 *   reads y / weight / x0 and writes out as fp32, with fp64 inside, and rounds once (energy is that of the fp64 volume).
 *   n_volumes == 0 succeeds and launches nothing.
 * workspace: inr_tvsr3d_workspace_doubles(n_volumes, D, H, W, f0, f1, f2) doubles (the state x | xbar | p0 | p1 | p2 of every volume
 * and the partials of energy and change), 16-byte aligned; 0 for sizes that would be refused.  Refusals, all before any device work:
 * INR_E_INVALID (null out / y / in / factors / grad_weights, n_volumes < 0, factors or sizes out of range, an extent no multiple of
 * its factor, n_iter outside 0 .. INR_TVSR3D_MAX_ITER, a negative or non-finite lambda / alpha / gradient weight, a factor that is
 * not finite or does not sum to 1), INR_E_WORKSPACE (null or short workspace), INR_E_ALIGN (workspace off a 16-byte boundary). */
#define INR_TVSR3D_MAX_ITER 100000
int inr_tvsr3d_block_apply(double* out, const double* in, int n_volumes, int depth, int height, int width, int f0, int f1, int f2,
                      const double* k0, const double* k1, const double* k2, void* stream);
int inr_tvsr3d_block_adjoint(double* out, const double* in, int n_volumes, int depth, int height, int width, int f0, int f1, int f2,
                        const double* k0, const double* k1, const double* k2, void* stream);
int64_t inr_tvsr3d_workspace_doubles(int n_volumes, int depth, int height, int width, int f0, int f1, int f2);
int inr_tvsr3d_solve(double* out, double* energy, double* change, const double* y, const double* weight, const double* x0, int n_volumes,
                     int depth, int height, int width, int f0, int f1, int f2, const double* k0, const double* k1, const double* k2,
                     const double* grad_weights, double lambda, double alpha, int n_iter, double* workspace, int64_t workspace_doubles,
                     void* stream);
int inr_tvsr3d_solve_f32(float* out, double* energy, double* change, const float* y, const float* weight, const float* x0, int n_volumes,
                         int depth, int height, int width, int f0, int f1, int f2, const double* k0, const double* k1, const double* k2,
                         const double* grad_weights, double lambda, double alpha, int n_iter, double* workspace,
                         int64_t workspace_doubles, void* stream);

/* ---- multi-frame TV / Huber super-resolution: K sub-pixel-shifted acquisitions of one image ---------------------------
 * No counterpart in the reference.  Images are [n_images][H][W] (HR), frames [n_images][K][h][w] (LR), H = f0 h, W = f1 w, factors and
 * sides as for inr_tvsr_solve2d, K = n_frames in 1 .. INR_TVMF_MAX_FRAMES; `kernel` is the HOST block kernel k [f0][f1] of
 * inr_block_apply2d.  shifts [n_images][K][2] are DEVICE doubles, (rows, columns) in HR pixels.  Per frame and axis n = floor(s),
 * t = s - n, and A_k = B S_k with the bilinear translation (S x)[i][j] = sum_{da, db in {0, 1}} wa wb x[i + n0 + da][j + n1 + db],
 * wa = (1 - t0, t0)[da], wb likewise, is one sum over the effective kernel ke [f0 + 1][f1 + 1], formed on the device:
 *   ke[a][b] = sum_{da, db} (wa wb) k[a - da][b - db] (ascending (da, db); a tap whose t is exactly 0 is not visited),
 *   (A_k x)[i][j] = sum_{a, b} ke[a][b] x[n0 + f0 i + a][n1 + f1 j + b] (ascending (a, b); f0 (+ 1 if t0 > 0) rows, columns alike):
 *   zero shifts give inr_block_apply2d bit for bit.
 * A datum (k, i, j) is VALID when its footprint -- rows n0 + f0 i .. n0 + f0 i + f0 - 1 (+ 1 if t0 > 0), columns alike -- lies inside
 * the image.  An invalid datum has weight 0 whatever `weight` holds; its y and weight are never read (they may be NaN).  A frame whose
 * shift is not finite or exceeds 2^20 in magnitude is invalid as a whole; the range test precedes every conversion, so no shift value
 * leads to an index outside the image.
 * inr_frame_apply2d: out [n][K][h][w] = (A_k in)_k with 0 at invalid data; valid [n][K][h][w] bytes (1 / 0) or null.
 * inr_frame_adjoint2d: out [n][H][W] = sum_k A_k^T in_k, a gather over the at most 2 x 2 valid LR pixels of every frame that reach an HR
 *   pixel -- frames ascending, then LR rows, then columns; no atomics.  fp64, one launch each, out must not overlap in.
 * inr_tvmf_solve2d: out [n][H][W] = n_iter iterations of Chambolle-Pock with both terms dual on
 *   min_x 1/2 sum_k sum_i w_ki ((A_k x)_i - y_ki)^2 + lambda sum_j H_alpha(|(grad x)_j|)   (grad, div, H_alpha: inr_tvsr_solve2d),
 *   from x = xbar = x0, p = 0, q = 0:
 *     p <- (p + sigma grad(xbar)) / (1 + sigma alpha / lambda);  p <- p / max(1, |p| / lambda)   (lambda == 0: p = 0)
 *     q_k <- (q_k + sigma (A_k xbar - y_k)) / (1 + sigma / w_k) at valid data with w_k > 0, else 0
 *     x' <- x - tau (sum_k A_k^T q_k - div p);  xbar <- 2 x' - x;  x <- x'
 *   tau = sigma = 1 / sqrt(8 + K' c), c = (sum |k|) (max |k|) >= |A_k|^2 for every shift, K' the number of the image's frames that hold a
 *   valid datum (K unless a frame lies outside the image; such a frame is the zero operator).  The objective is NOT divided by K.
 *   y [n][K][h][w]; weight [n][K][h][w] or null (= 1; finite and >= 0 -- device data, not checked; <= 0 or NaN is a missing datum); x0
 *   [n][H][W] or null (the block replication of frame 0, all of which is then read).  energy / change / valid_fraction [n] DEVICE
 *   doubles or null: the objective at the returned fp64 image, max |x' - x| of the last iteration (0 for n_iter == 0, which returns
 *   x0), and the valid share of the K h w data.  Op sequence: init; per iteration a dual launch (thread per HR pixel and per LR datum)
 *   and a primal launch (thread per HR pixel); a final launch and a fixed-order finish.  Plain launches on `stream`, no host read, no
 *   float atomics: calls are bit-equal on any stream and at any place in a batch.  The _f32 form reads y / weight / x0 and writes out
 *   as fp32, with fp64 inside, and rounds once.  n_images == 0 succeeds and launches nothing.
 * workspace: inr_tvmf_workspace_doubles(n_images, K, H, W, f0, f1) doubles, 16-byte aligned; 0 for sizes that would be refused.
 * Refusals, all before any device work: INR_E_INVALID (null out / y / in / shifts / kernel, n_images < 0, K, factors or sizes out of
 * range, H or W no multiple of its factor, n_iter outside 0 .. INR_TVSR3D_MAX_ITER, a negative or non-finite lambda / alpha, a kernel
 * that is not finite or does not sum to 1), INR_E_WORKSPACE (null or short workspace), INR_E_ALIGN (workspace off a 16-byte boundary). */
#define INR_TVMF_MAX_FRAMES 64
int inr_frame_apply2d(double* out, unsigned char* valid, const double* in, const double* shifts, int n_images, int n_frames, int height,
                      int width, int f0, int f1, const double* kernel, void* stream);
int inr_frame_adjoint2d(double* out, const double* in, const double* shifts, int n_images, int n_frames, int height, int width, int f0,
                        int f1, const double* kernel, void* stream);
int64_t inr_tvmf_workspace_doubles(int n_images, int n_frames, int height, int width, int f0, int f1);
int inr_tvmf_solve2d(double* out, double* energy, double* change, double* valid_fraction, const double* y, const double* shifts,
                     const double* weight, const double* x0, int n_images, int n_frames, int height, int width, int f0, int f1,
                     const double* kernel, double lambda, double alpha, int n_iter, double* workspace, int64_t workspace_doubles,
                     void* stream);
int inr_tvmf_solve2d_f32(float* out, double* energy, double* change, double* valid_fraction, const float* y, const double* shifts,
                         const float* weight, const float* x0, int n_images, int n_frames, int height, int width, int f0, int f1,
                         const double* kernel, double lambda, double alpha, int n_iter, double* workspace, int64_t workspace_doubles,
                         void* stream);

/* ---- multi-stack 3-D TV / Huber reconstruction with general slice profiles ---------------------------------------------
 * No counterpart in the reference.  Volumes are [n_volumes][D][H][W] (HR: slice, row, column), D, H, W <= INR_TVSR_MAX_SIDE.  A call
 * has n_stacks in 1 .. INR_TVMS_MAX_STACKS stacks, the same for every volume of the batch.  `geometry` is a HOST array int [S][12] =
 * (f0, f1, f2, L0, L1, L2, o0, o1, o2, n0, n1, n2) per stack: per axis a spacing f in 1 .. INR_TVSR_MAX_FACTOR, a tap count L in
 * 1 .. INR_TVMS_MAX_TAPS, an offset o in HR voxels with |o| <= 2^20 (it may be negative) and an LR extent n in 1 .. 2048.  `taps` are
 * HOST doubles, per stack k0 [L0] | k1 [L1] | k2 [L2] concatenated, the stacks in order; each k_a is finite and sums to 1 (to 1e-9).
 * Data (y, weight, the result of inr_tvms_apply) are [n_volumes][M], M = sum_s n0 n1 n2, the stacks in order, each [n0][n1][n2].
 *   (A_s x)[l][i][j] = sum_{a, b, c} k[a][b][c] x[o0 + f0 l + a][o1 + f1 i + b][o2 + f2 j + c],  k[a][b][c] = (k1[b] * k2[c]) * k0[a],
 *   the terms added in ascending (a, b, c): a stack with L = f, o = 0, n = N / f is inr_tvsr3d_block_apply bit for bit.  L > f: slices
 *   overlap; L < f: gaps.  A datum is VALID when its footprint lies inside the volume on every axis (0 <= o + f i, o + f i + L <= N).
 *   An invalid datum has weight 0 whatever `weight` holds; its y and weight are never read (they may be NaN) and its dual variable is
 *   0.  Every range test precedes the address it guards, and the limits above keep o + f i + L within an int.
 * inr_tvms_apply: out [n][M] = (A_s in)_s with 0 at invalid data; valid [n][M] bytes (1 / 0) or null.
 * inr_tvms_adjoint: out [n][D][H][W] = sum_s A_s^T in_s, a gather: HR voxel m sums k[a][b][c] in[l][i][j] over the valid data whose
 *   footprint holds m -- stacks ascending, then l, i, j ascending, per axis the indices floordiv(m - o - L + 1 + f - 1, f) ..
 *   floordiv(m - o, f); no atomics.  For a block stack it is inr_tvsr3d_block_adjoint bit for bit.  fp64, one launch each, out must not
 *   overlap in.
 * inr_tvms_solve: out [n][D][H][W] = n_iter iterations of Chambolle-Pock with both terms dual on
 *   min_x 1/2 sum_s sum_i w_si ((A_s x)_i - y_si)^2 + lambda sum_j H_alpha(sqrt((g1 d1 x)_j^2 + (g2 d2 x)_j^2 + (g0 d0 x)_j^2))
 *   (differences, grad_weights, combining order, "axes longer than 1" rule, H_alpha: inr_tvsr3d_solve), from x = xbar = x0, p = 0, q = 0:
 *     p   <- (p + sigma g d(xbar)) / (1 + sigma alpha / lambda);  p <- p / max(1, |p| / lambda)   (lambda == 0 or no axis longer than 1: p = 0)
 *     q_s <- (q_s + sigma (A_s xbar - y_s)) / (1 + sigma / w_s)   at valid data with w_s > 0, else 0
 *     x'  <- x - tau (sum_s A_s^T q_s - div p);  xbar <- 2 x' - x;  x <- x'
 *   tau = sigma = 1 / sqrt(4 sum_a g_a^2 + sum_{s live} c_s): the first sum over the axes longer than 1 in the order (1, 2, 0), c_s =
 *   prod_a (sum_t |k_a[t]|) (max_{r < f_a} sum_{t = r mod f_a} |k_a[t]|) in the order a = 0, 1, 2, the stacks ascending, a stack LIVE
 *   when it holds a valid datum; formed on the host in fp64 (a zero bound: tau = 1 / sqrt(8)).  The objective is not divided by the
 *   number of stacks.  x0 [n][D][H][W] or null: the normalised back-projection (sum_s A_s^T y_s) / (sum_s A_s^T 1) over the usable data
 *   (valid, w > 0), 0 where no usable datum reaches.  weight [n][M] or null (1).  energy / change / valid_fraction [n] or null: the
 *   objective at the result, max |x' - x| of the last iteration (0 for n_iter == 0), the valid share of the M data.
 *   Launches: init; a back-projection launch without x0; per iteration a dual launch (thread per HR voxel where the prior is on, and
 *   per datum) and a primal launch (thread per HR voxel); a final launch and a fixed-order finish.  Plain launches on `stream`, no
 *   host read, no float atomics: calls are bit-equal on any stream and at any place in a batch.  The _f32 form reads y / weight / x0
 *   and writes out as fp32, with fp64 inside, and rounds once.  n_volumes == 0 succeeds and launches nothing.
 * workspace: inr_tvms_workspace_doubles(n_volumes, D, H, W, n_stacks, geometry) doubles (the state x | xbar | p0 | p1 | p2, q and the
 * partials), 16-byte aligned; 0 for sizes that would be refused.  Refusals, all before any device work: INR_E_INVALID (null out / y /
 * in / geometry / taps / grad_weights, n_volumes < 0, n_stacks, f, L, o, n or the HR sides out of range, n_iter outside 0 ..
 * INR_TVSR3D_MAX_ITER, a negative or non-finite lambda / alpha / gradient weight, taps that are not finite or do not sum to 1),
 * INR_E_WORKSPACE (null or short workspace), INR_E_ALIGN (workspace off a 16-byte boundary). */
#define INR_TVMS_MAX_STACKS 8
#define INR_TVMS_MAX_TAPS 16
int inr_tvms_apply(double* out, unsigned char* valid, const double* in, int n_volumes, int depth, int height, int width, int n_stacks,
                   const int* geometry, const double* taps, void* stream);
int inr_tvms_adjoint(double* out, const double* in, int n_volumes, int depth, int height, int width, int n_stacks, const int* geometry,
                     const double* taps, void* stream);
int64_t inr_tvms_workspace_doubles(int n_volumes, int depth, int height, int width, int n_stacks, const int* geometry);
int inr_tvms_solve(double* out, double* energy, double* change, double* valid_fraction, const double* y, const double* weight,
                   const double* x0, int n_volumes, int depth, int height, int width, int n_stacks, const int* geometry,
                   const double* taps, const double* grad_weights, double lambda, double alpha, int n_iter, double* workspace,
                   int64_t workspace_doubles, void* stream);
int inr_tvms_solve_f32(float* out, double* energy, double* change, double* valid_fraction, const float* y, const float* weight,
                       const float* x0, int n_volumes, int depth, int height, int width, int n_stacks, const int* geometry,
                       const double* taps, const double* grad_weights, double lambda, double alpha, int n_iter, double* workspace,
                       int64_t workspace_doubles, void* stream);

/* ---- TV / Huber super-resolution under a dense separable acquisition model ---------------------------------------------
 * No counterpart in the reference.  Images are [n_images][H][W] (HR) and [n_images][h][w] (LR); H = height, W = width, h = lr_height,
 * w = lr_width, each 1 .. INR_TVSR_MAX_SIDE, h and w below, equal to or above H and W.  The acquisition model is ANY separable linear
 * operator given by r0 [h][H] and r1 [w][W], dense DEVICE doubles shared by the whole batch (inr_fourier_operator forms k-space
 * truncation in this layout):
 *   A x = (R0 x) R1^T [h][w],   A^T r = R0^T (r R1) [H][W].
 * Their values are not inspected: no operator, weight or datum value reaches an index, and a NaN gives NaNs and no fault.  Every
 * contraction is a batched fp64 GEMM on v_mfma_f64_16x16x4_f64 with a fixed K order and no atomics (the tile loop of
 * inr_fourier_resample2d); both directions pass through a plane [n][h][W] of the workspace.
 * inr_tvop_apply: out [n][h][w] = A in.  inr_tvop_adjoint: out [n][H][W] = A^T in.  fp64, two launches each, out must not overlap in.
 *   They are the launches of the solver with a plain store: A x has the same bits in both.
 * inr_tvop_solve2d: out [n][H][W] = n_iter iterations of Chambolle-Pock with both terms dual (the iteration of inr_tvmf_solve2d) on
 *   min_x 1/2 sum_i w_i ((A x)_i - y_i)^2 + lambda sum_j H_alpha(|(grad x)_j|)   (grad, div, H_alpha: inr_tvsr_solve2d),
 *   from x = xbar = x0, p = 0, q = 0:
 *     p <- (p + sigma grad(xbar)) / (1 + sigma alpha / lambda);  p <- p / max(1, |p| / lambda)   (lambda == 0: p = 0)
 *     q <- (q + sigma (A xbar - y)) / (1 + sigma / w) where w > 0, else 0
 *     x' <- x - tau (A^T q - div p);  xbar <- 2 x' - x;  x <- x'
 *   tau = sigma = 1 / sqrt(8 + c0 c1), c_a = (max_i sum_j |R_a[i][j]|) (max_j sum_i |R_a[i][j]|) >= |R_a|_2^2, the sums in ascending
 *   index, formed by a kernel and read from the workspace by the others: there is no host read in a solve.
 *   y [n][h][w]; weight [n][h][w] or null (= 1; finite and >= 0 -- device data, not checked; <= 0 or NaN is a missing datum, whose y is
 *   never used and may be NaN); x0 [n][H][W] or null: the normalised back-projection through the absolute operators,
 *   (|R0|^T (u y) |R1|) / (|R0|^T u |R1|) with u = [w > 0], 0 where the denominator is not > 0.  energy / change [n] DEVICE doubles or
 *   null: the objective at the returned fp64 image and max |x' - x| of the last iteration (0 for n_iter == 0, which returns the start).
 *   Launches: step, init, without x0 the back-projection (the adjoint's two launches twice); per iteration a dual launch (thread per HR
 *   pixel; skipped for lambda == 0) and four GEMM launches -- R0 xbar, (.) R1^T with the q update as its epilogue, q R1, R0^T (.) with
 *   the primal update as its epilogue --; A x once more with the data term summed per tile, an HR-tile launch (the result, the prior)
 *   and a fixed-order finish.  Plain launches on `stream`, no host read, no atomics: calls are bit-equal on any stream and at any place
 *   in a batch.  The _f32 form reads y / weight / x0 and writes out as fp32, with fp64 operators and state, and rounds once.
 *   n_images == 0 succeeds and launches nothing.
 * workspace: inr_tvop_workspace_doubles(n_images, H, W, h, w) doubles for every entry above, 16-byte aligned; 0 for sizes that would be
 * refused.  With e(v) = v rounded up to even, T(v) = ceil(v / 64), TL = T(h) T(w), TH = T(H) T(W) it is
 *   2 + e(4 n H W) + e(n h w) + e(n h W) + e(n (TL + TH)) + e(n TH)
 * (the step, the state x | xbar | p0 | p1, q, the plane, the partials of energy and of change; n = 1 for n_images == 0).
 * Refusals, all before any device work: INR_E_INVALID (null out / y / in / r0 / r1, n_images < 0, a side out of range, n_iter outside
 * 0 .. INR_TVSR3D_MAX_ITER, a negative or non-finite lambda / alpha), INR_E_WORKSPACE (null or short workspace), INR_E_ALIGN (workspace
 * off a 16-byte boundary). */
int64_t inr_tvop_workspace_doubles(int n_images, int height, int width, int lr_height, int lr_width);
int inr_tvop_apply(double* out, const double* in, const double* r0, const double* r1, int n_images, int height, int width, int lr_height,
                   int lr_width, double* workspace, int64_t workspace_doubles, void* stream);
int inr_tvop_adjoint(double* out, const double* in, const double* r0, const double* r1, int n_images, int height, int width, int lr_height,
                     int lr_width, double* workspace, int64_t workspace_doubles, void* stream);
int inr_tvop_solve2d(double* out, double* energy, double* change, const double* y, const double* weight, const double* x0,
                     const double* r0, const double* r1, int n_images, int height, int width, int lr_height, int lr_width, double lambda,
                     double alpha, int n_iter, double* workspace, int64_t workspace_doubles, void* stream);
int inr_tvop_solve2d_f32(float* out, double* energy, double* change, const float* y, const float* weight, const float* x0,
                         const double* r0, const double* r1, int n_images, int height, int width, int lr_height, int lr_width,
                         double lambda, double alpha, int n_iter, double* workspace, int64_t workspace_doubles, void* stream);

/* ---- channel-coupled (vectorial) TV / Huber super-resolution: one prior over the channels of a group --------------------
 * No counterpart in the reference.  A group is C = channels images of one anatomy (the b-values of a DWI slice), 1 <= C <=
 * INR_TVJ_MAX_CHANNELS: x [n_groups][C][H][W] (HR), y [n_groups][C][h][w] (LR); sides, factors and the HOST `kernel` as for
 * inr_tvsr_solve2d.  `channel_weights` is a HOST array mu [C] of finite doubles in [0, 1], or null (all 1): with max mu <= 1 the
 * operator K x = (mu_c grad x_c)_c keeps |K|^2 <= 8 and the steps tau = sigma = 1/sqrt(8); larger weights are a rescaled lambda / alpha.
 * inr_tvj_solve2d: out = n_iter iterations of Chambolle-Pock on
 *   min_x 1/2 sum_c sum_i w_ci ((A x_c)_i - y_ci)^2 + lambda sum_j H_alpha( sqrt( sum_c mu_c^2 |(grad x_c)_j|^2 ) )   (coupling 1: joint)
 *   min_x 1/2 sum_c sum_i w_ci ((A x_c)_i - y_ci)^2 + lambda sum_c sum_j H_alpha( mu_c |(grad x_c)_j| )               (coupling 0: none)
 *   (A, grad, div, H_alpha: inr_tvsr_solve2d), from x = xbar = x0, p = 0:
 *     q_c <- (p_c + sigma (mu_c grad(xbar_c))) / (1 + sigma alpha / lambda)
 *     n <- sqrt(sum_c |q_c|^2) / lambda (ascending c; none: per channel);  p_c <- n > 1 ? q_c / n : q_c       (lambda == 0: p = 0)
 *     v_c <- x_c + tau (mu_c div(p_c));  x'_c <- v_c - A^T(c_c (A v_c - y_c)), c_ci = tau w_ci / (1 + tau w_ci |k|^2)
 *     xbar <- 2 x' - x;  x <- x'
 *   It replaces, per iteration, C gradients, C scalings, the reduction of the squared norms over the channel axis, the projection, C
 *   divergences and C data proximal maps.  The expression order is that of inr_tvsr_solve2d with the products by mu_c placed as written:
 *   C == 1, and coupling 0 with mu = 1 per channel, give its bits.  y, weight, x0 [.][C][..] as for inr_tvsr_solve2d (weight 0: a
 *   missing datum whose y is never read; x0 null: block replication).  energy / change [n_groups] DEVICE doubles or null: the objective
 *   at the returned fp64 x (fixed order, no float atomics) and max |x' - x| of the last iteration over all channels.  ONE launch, no
 *   host read: one workgroup of 1,024 threads per group runs all iterations with workgroup barriers only; groups beyond the CU count
 *   are queued.  The _f32 form reads y / weight / x0 and writes out as fp32, fp64 inside, rounded once.  n_groups == 0 succeeds and
 *   launches nothing.
 * workspace: inr_tvj_workspace_doubles(n_groups, C, H, W) = 4 n C H W doubles (the state x | xbar | p0 | p1 of every group; n = 1 for
 * n_groups == 0), 16-byte aligned; 0 for sizes that would be refused.  Refusals, all before any device work: INR_E_INVALID (null out / y /
 * kernel, n_groups < 0, channels outside 1 .. INR_TVJ_MAX_CHANNELS, factors or sizes out of range, H or W no multiple of its factor,
 * n_iter < 0, a negative or non-finite lambda / alpha, coupling not 0 / 1, a kernel that is not finite or does not sum to 1, a channel
 * weight that is not finite or outside [0, 1]), INR_E_WORKSPACE (null or short workspace), INR_E_ALIGN (workspace off a 16-byte
 * boundary). */
#define INR_TVJ_MAX_CHANNELS 16
int64_t inr_tvj_workspace_doubles(int n_groups, int channels, int height, int width);
int inr_tvj_solve2d(double* out, double* energy, double* change, const double* y, const double* weight, const double* x0, int n_groups,
                    int channels, int height, int width, int f0, int f1, const double* kernel, const double* channel_weights,
                    double lambda, double alpha, int coupling, int n_iter, double* workspace, int64_t workspace_doubles, void* stream);
int inr_tvj_solve2d_f32(float* out, double* energy, double* change, const float* y, const float* weight, const float* x0, int n_groups,
                        int channels, int height, int width, int f0, int f1, const double* kernel, const double* channel_weights,
                        double lambda, double alpha, int coupling, int n_iter, double* workspace, int64_t workspace_doubles,
                        void* stream);

/* ---- model-based S0 / ADC super-resolution: the mono-exponential model inside the solver, a TV prior on the maps ------
 * No counterpart in the reference.  A group is the C = channels b-values of one slice, 2 <= C <= INR_TVJ_MAX_CHANNELS, y
 * [n_groups][C][h][w] (LR); the unknowns are the two parameter maps, out [n_groups][2][H][W]: map 0 the b = 0 signal s, map 1 the ADC d.
 * Sides, factors and the HOST `kernel` as for inr_tvsr_solve2d.  `b` is a HOST array [C] of finite b-values >= 0, not all equal;
 * `map_weights` a HOST array (mu_s, mu_u) of finite doubles in [0, 1], or null (both 1).
 * inr_tvadc_solve2d: out = n_iter iterations of the exact nonlinear primal-dual method (Valkonen 2014) on
 *   min 1/2 sum_c sum_i w_ci ((A (s .* exp(-b_c d)))_i - y_ci)^2 + lambda R(s, d),   0 <= s <= s_max,  0 <= d <= adc_max
 *   R = sum_j H_alpha( sqrt( mu_s^2 |(grad s)_j|^2 + mu_u^2 |(grad u)_j|^2 ) )   (coupling 1: joint)
 *   R = sum_j H_alpha( mu_s |(grad s)_j| ) + sum_j H_alpha( mu_u |(grad u)_j| ) (coupling 0: none)
 *   in the normalised ADC u = d b_max (beta_c = b_c / b_max, u_max = adc_max b_max), from s = sbar, u = ubar, p = 0, z = 0:
 *     q_m <- (p_m + sigma (mu_m grad(mbar))) / (1 + sigma alpha / lambda), m in {s, u};  n <- sqrt(|q_s|^2 + |q_u|^2) / lambda (none:
 *     per map);  p_m <- n > 1 ? q_m / n : q_m                                                              (lambda == 0: p = 0)
 *     r <- (A (sbar .* exp(-beta_c ubar)))_i - y_ci;  z_ci <- (z_ci + sigma r) / (1 + sigma / w_ci)         (w_ci == 0: z_ci = 0)
 *     g_s <- sum_c exp(-beta_c u) (A^T z_c) - mu_s div(p_s);  g_u <- sum_c (-beta_c s exp(-beta_c u)) (A^T z_c) - mu_u div(p_u)
 *     s' <- fmin(fmax(s - tau g_s, 0), s_max);  u' <- fmin(fmax(u - tau g_u, 0), u_max);  sbar <- 2 s' - s;  ubar <- 2 u' - u
 *   with tau = sigma = 1 / sqrt(8 + c_A sum_c (1 + beta_c^2 s_max^2)), c_A = (sum |k|)(max |k|): a bound on the Jacobian of the whole
 *   operator that holds everywhere on the box.  Convergence of the nonlinear method is local; the objective is not convex.  The start:
 *   x0 [n_groups][2][H][W] (s, d) clamped into the box, or (x0 null) the block replication of the first channel of smallest b, clamped,
 *   and d = adc0.  weight [n_groups][C][h][w] or null (all 1): weight 0 is a missing datum whose y is never read by the iteration.
 *   energy / change [n_groups] DEVICE doubles or null: the objective at the returned fp64 maps (fixed order, no float atomics) and
 *   max(|s' - s|, |u' - u|) of the last iteration.  ONE launch, no host read: one workgroup of 1,024 threads per group runs all
 *   iterations with workgroup barriers only; groups beyond the CU count are queued.  fp64 exp, 2 C calls per pixel and iteration.  The
 *   _f32 form reads y / weight / x0 and writes out as fp32, fp64 inside, rounded once.  n_groups == 0 succeeds and launches nothing.
 * workspace: inr_tvadc_workspace_doubles(n_groups, C, H, W, f0, f1) = n (8 H W + C h w) doubles (s | u | sbar | ubar | p_s0 | p_s1 | p_u0
 * | p_u1 and z of every group; n = 1 for n_groups == 0), 16-byte aligned; 0 for sizes that would be refused.  Refusals, all before any
 * device work: INR_E_INVALID (null out / y / b / kernel, n_groups < 0, channels outside 2 .. INR_TVJ_MAX_CHANNELS, factors or sizes out
 * of range, H or W no multiple of its factor, n_iter < 0, a negative or non-finite lambda / alpha, coupling not 0 / 1, a kernel that is
 * not finite or does not sum to 1, a b-value that is not finite or negative, b-values all equal, s_max or adc_max not finite and > 0,
 * adc0 outside [0, adc_max], a map weight that is not finite or outside [0, 1]), INR_E_WORKSPACE (null or short workspace), INR_E_ALIGN
 * (workspace off a 16-byte boundary).
 * inr_adc_signal: out [n_maps][C][pixels] = s0 [n_maps][pixels] exp(-b_c adc [n_maps][pixels]), the model's images of two maps; `b` a HOST
 * array [C] of finite doubles, 1 <= C <= INR_TVJ_MAX_CHANNELS; fp64 inside, the _f32 form rounds once. */
int64_t inr_tvadc_workspace_doubles(int n_groups, int channels, int height, int width, int f0, int f1);
int inr_tvadc_solve2d(double* out, double* energy, double* change, const double* y, const double* weight, const double* x0, int n_groups,
                      int channels, int height, int width, int f0, int f1, const double* kernel, const double* b,
                      const double* map_weights, double lambda, double alpha, int coupling, int n_iter, double s_max, double adc_max,
                      double adc0, double* workspace, int64_t workspace_doubles, void* stream);
int inr_tvadc_solve2d_f32(float* out, double* energy, double* change, const float* y, const float* weight, const float* x0, int n_groups,
                          int channels, int height, int width, int f0, int f1, const double* kernel, const double* b,
                          const double* map_weights, double lambda, double alpha, int coupling, int n_iter, double s_max,
                          double adc_max, double adc0, double* workspace, int64_t workspace_doubles, void* stream);
int inr_adc_signal(double* out, const double* s0, const double* adc, const double* b, int64_t n_maps, int channels, int64_t pixels,
                   void* stream);
int inr_adc_signal_f32(float* out, const float* s0, const float* adc, const double* b, int64_t n_maps, int channels, int64_t pixels,
                       void* stream);

/* ---- Marchenko-Pastur PCA denoising of a multi-measurement stack, with a noise map -----------------------------------
 * No counterpart in the reference tree, whose later driver reads a stack denoised elsewhere (`hybrid_raw_clean`).  Veraart et al.,
 * NeuroImage 2016; the cutoff estimators of Cordero-Grande et al. 2019 (`dwidenoise`).  x [M][D][H][W] DEVICE, measurement-major, every
 * volume contiguous; the window (w0, w1, w2) has odd sides w_a <= n_a, N = w0 w1 w2 voxels; mask [D][H][W] DEVICE bytes or null (all
 * inside).  r = min(M, N) <= INR_MPPCA_MAX_RANK, q = max(M, N) <= INR_MPPCA_MAX_LONG.  For every voxel (z, y, x) inside the mask:
 *   1. the window starts at clamp(i - w / 2, 0, n - w) along each axis: shifted inward at the edges, never mirrored or padded (mirroring
 *      duplicates columns, the matrix loses rank and the smallest eigenvalues become rounding noise).  X is the M x N matrix of its
 *      voxels in (dz, dy, dx) order, c the column of the voxel itself (N / 2 only in the interior).  The mask removes no column.
 *   2. G = X X^T (M <= N) or X^T X (N < M), r x r, summed over the long index in ascending order.
 *   3. s_0 <= ... <= s_{r-1} the eigenvalues of G, lam_p = max(s_p, 0) / q; an eigenvalue s_p <= q eps s_{r-1} is numerically zero (what
 *      summing q products leaves of an exact zero): its lam_p is 0 and it is noise whatever step 4 decides.
 *   4. clam = 0, cut = 0, sigma2 = 0;  for p = 0 .. r - 1:  clam += lam_p;  gam = (p + 1) / (q - (r - p - 1)) (estimator 2, "exp2") or
 *      (p + 1) / q (estimator 1, "exp1");  a = clam / (p + 1);  b = (lam_p - lam_0) / (4 sqrt(gam));  if b < a: sigma2 = a, cut = p + 1.
 *      Then cut = max(cut, the number of numerically zero eigenvalues): exact low-rank data comes back with its rank and sigma = 0.
 *   5. sigma = sqrt(sigma2), rank = r - cut; with V_s the eigenvectors cut .. r - 1:  xhat = V_s (V_s^T X[:, c]) (M <= N) or
 *      X (V_s V_s[c, :]^T) (N < M);  out[:, z, y, x] = xhat -- the voxel's own column only (sliding window, no overlap averaging).
 * Outside the mask out = x, sigma = 0, rank = -1.  out [M][D][H][W], sigma [D][H][W] (null: not wanted), rank [D][H][W] (null: not
 * wanted) DEVICE; out must not overlap x.  ONE launch, no workspace, no host read, no float atomics: one workgroup per voxel (a capped
 * grid with a stride loop) forms G in LDS, diagonalises it by cyclic two-sided Jacobi in round-robin ordering, fp64 throughout, until
 * the off-diagonal sum of squares is at most (r eps)^2 ||G||_F^2, ranks the eigenvalues and projects.  A voxel that has not converged
 * after 30 sweeps (data that is not finite) gets rank = -2, sigma = 0, out = x.  Two runs give the same bits, whatever the grid.  The
 * _f32 form reads x and writes out / sigma as fp32, fp64 inside, rounded once.  D H W == 0 succeeds and launches nothing.
 * Refusals, all INR_E_INVALID and before any device work: null out or x, M < 2, a negative size, a window side that is even or < 1,
 * N < 2, min(M, N) > INR_MPPCA_MAX_RANK (shrink the window or split the measurements), max(M, N) > INR_MPPCA_MAX_LONG, an estimator
 * that is not 1 or 2, a window side larger than its axis. */
#define INR_MPPCA_MAX_RANK 64
#define INR_MPPCA_MAX_LONG 1024
int inr_mppca_denoise(double* out, double* sigma, int32_t* rank, const double* x, const uint8_t* mask, int M, int D, int H, int W, int w0,
                      int w1, int w2, int estimator, void* stream);
int inr_mppca_denoise_f32(float* out, float* sigma, int32_t* rank, const float* x, const uint8_t* mask, int M, int D, int H, int W,
                          int w0, int w1, int w2, int estimator, void* stream);

/* ---- Gibbs-ringing removal by local sub-voxel shifts ---------------------------------------------------------------------
 * No counterpart in the reference.  Kellner et al., MRM 2016 (`mrdegibbs`, DIPY's `gibbs_removal`); pinned to the definition below,
 * which tests/degibbs_common.py restates in float64 numpy.  The data must lie on the acquired grid: scanner-interpolated or
 * partial-Fourier data ring at another period and are not served.  All arithmetic is fp64.
 * One line x[0..n), periodic, nshifts = N, window (w_min, w_max), all indices mod n:
 *   shifts   s_0 = 0, s_j = j / (2N) and s_{N+j} = -j / (2N) for j = 1 .. N: 2N + 1 candidates in this order.
 *   copies   x_s[i] = sum_j h_s((i - j) mod n) x[j] in ascending j, h_s(d) = (1/n) sum_{k = 0 .. floor(n/2)} c_k cos(2 pi k (d + s) / n)
 *            in ascending k, c_0 = 1, c_k = 2, c_{n/2} = 1 for even n (the Nyquist bin split between +n/2 and -n/2); with s = j / (2N)
 *            the phase is pi ((k (2N d + j)) mod (2N n)) / (N n), reduced exactly in integers.  x_s[i] is the band-limited interpolant
 *            at i + s.  The copy for s_0 is the line itself, bit for bit.
 *   measure  d_s[i] = |x_s[i] - x_s[i-1]|;  L_s[i] = sum_{t = w_min .. w_max} d_s[i - t],  R_s[i] = sum_t d_s[i + t + 1], ascending t;
 *            tv_s[i] = min(L_s[i], R_s[i]).
 *   choice   choice[i] = the first index in list order with the smallest tv (a strict < while walking the list).
 *   output   with s the chosen shift: out[i] = x[i] (s = 0), (1 - s) x_s[i] + s x_s[i-1] (s > 0), (1 + s) x_s[i] - s x_s[i+1] (s < 0).
 * One image I [H][W]:  c_a(k) = 1 + cos(2 pi k / n_a), exactly 0 at k = n_a / 2;  G1(k0, k1) = c_0(k0) / (c_0(k0) + c_1(k1)), and 1/2 at
 * the one bin where both vanish (the published code zeroes that bin; with 1/2 the two parts sum to the image);  I1 = Re IDFT2(G1 DFT2(I)),
 * I0 = I - I1;  out = U1(I1) + U0(I0) with U_a the line operation along axis a (0: down the rows, 1: along the columns).
 * inr_degibbs_lines: in, out [n_lines][n] DEVICE, lines contiguous; choice [n_lines][n] DEVICE int32 or null (not wanted).
 * inr_degibbs2d: in, out [n_images][H][W] DEVICE; choice [2][n_images][H][W] DEVICE int32, the axis-0 pass first, or null.
 * out must not overlap in.  The workspace (DEVICE, 16-byte aligned, the planner's doubles) holds the table h [2 nshifts][n] of an axis
 * -- never a dense operator per shift -- and, for images, the DFT matrices of the split and six planes of a chunk of images: a batch
 * whose planes would exceed INR_DEGIBBS_CHUNK_DOUBLES doubles is walked in chunks of whole images inside the call, and its bits do not
 * depend on that.  One kernel runs the whole shift loop of a pass on v_mfma_f64_16x16x4_f64; fixed-order sums, no atomics, no host
 * read: two runs give the same bits, whatever the grid, the stream and an image's place in the batch.  The _f32 forms convert on load and
 * round once on the last store.  n_lines == 0 / n_images == 0 succeed and launch nothing.  The planners return 0 for sizes every call
 * refuses (they do not know the window: a line of 5 .. 2 w_max + 2 samples is planned and then refused).
 * Refusals, before any device work: INR_E_INVALID for a null out or in, a negative count, nshifts outside 1 .. INR_DEGIBBS_MAX_SHIFTS,
 * a window that does not satisfy 1 <= w_min <= w_max <= INR_DEGIBBS_MAX_WINDOW, a line (rows, columns) outside 2 w_max + 3 ..
 * INR_DEGIBBS_MAX_LINE samples, out overlapping in; INR_E_WORKSPACE for a workspace smaller than planned (INR_E_ALIGN: misaligned). */
#define INR_DEGIBBS_MAX_LINE 1024
#define INR_DEGIBBS_MAX_SHIFTS 64
#define INR_DEGIBBS_MAX_WINDOW 8
#define INR_DEGIBBS_CHUNK_DOUBLES 2097152
int64_t inr_degibbs_lines_workspace_doubles(long long n_lines, int n, int nshifts);
int64_t inr_degibbs2d_workspace_doubles(int n_images, int height, int width, int nshifts);
int inr_degibbs_lines(double* out, int32_t* choice, const double* in, long long n_lines, int n, int nshifts, int w_min, int w_max,
                      double* workspace, int64_t workspace_doubles, void* stream);
int inr_degibbs_lines_f32(float* out, int32_t* choice, const float* in, long long n_lines, int n, int nshifts, int w_min, int w_max,
                          double* workspace, int64_t workspace_doubles, void* stream);
int inr_degibbs2d(double* out, int32_t* choice, const double* in, int n_images, int height, int width, int nshifts, int w_min, int w_max,
                  double* workspace, int64_t workspace_doubles, void* stream);
int inr_degibbs2d_f32(float* out, int32_t* choice, const float* in, int n_images, int height, int width, int nshifts, int w_min,
                      int w_max, double* workspace, int64_t workspace_doubles, void* stream);

/* ---- non-local means on volumes and non-local MRI upsampling --------------------------------------------------------------
 * No counterpart in the reference.  Buades et al. 2005 in its MRI form (Rician bias correction: Wiest-Daessle et al. 2008, Manjon et al.
 * 2008; a per-voxel strength) and the upsampling of Manjon et al., Medical Image Analysis 2010; pinned to the definition below, which
 * tests/nlm_common.py restates in float64 numpy.  All arithmetic is fp64.
 * A guide G [D][H][W], C value volumes X_c [D][H][W], search radii s = (s0, s1, s2), 0 .. INR_NLM_MAX_SEARCH each, patch radii
 * r = (r0, r1, r2), 0 .. INR_NLM_MAX_PATCH each, a strength h2_p > 0 (one scalar, or one value per voxel):
 *   offsets   for a voxel p and an offset t != 0 of the search box, q = p + t; an offset whose q lies outside the volume is skipped.
 *   distance  d2(p, t) = (1 / n) sum_d (G[p + d] - G[q + d])^2 over the patch offsets d for which both p + d and q + d lie inside the
 *             volume, n their number (d = 0 always counts).  Indices are never clamped or mirrored, so the squared-difference field of t
 *             followed by a separable box sum is exact at the borders too, and n is a product of three per-axis counts.
 *   weights   w(p, t) = exp(-d2 / h2_p), no cutoff;  wmax_p = max_t w;  the centre weight wc = wmax_p, or 1 where wmax_p is not > 0
 *             (INR_NLM_CENTER_MAX), or wc = 1 (INR_NLM_CENTER_ONE).
 *   output    V_c = X_c, or X_c^2 under Rician correction;  m_c(p) = (sum_t w V_c[q] + wc V_c[p]) / (sum_t w + wc), the offsets in
 *             ascending (t0, t1, t2), the centre last;  out_c(p) = m_c(p), or sqrt(max(m_c(p) - 2 sigma2_p, 0)) under Rician correction.
 *   copies    a voxel whose h2_p is not > 0 (zero, negative, NaN) or that lies outside the mask is copied, out = X; it still serves as a
 *             neighbour of others.
 * inr_nlm3d: out, x [n_groups][C][D][H][W] DEVICE; guide [n_groups][D][H][W] DEVICE or null (C must be 1: the guide is x); h2_map
 * [n_groups][D][H][W] DEVICE or null (the scalar h2 holds everywhere; with a map the scalar is ignored); sigma2 [n_groups][D][H][W] DEVICE
 * or null (no Rician correction); mask [n_groups][D][H][W] DEVICE bytes or null (all inside).  out must not overlap x or guide.  ONE
 * launch over n_groups x tiles: a workgroup owns a tile of 256 output voxels (4 x 8 x 8, or 1 x 16 x 16 where s0 + r0 == 0), stages the
 * guide with a halo of s + r in LDS, and per offset forms the field and its three box sums there (at most 85,056 bytes); the sums of a
 * voxel stay in registers.  No index depends on a data value: no value, NaN included, leads to an address outside a buffer.
 * inr_nlm_upsample: y [n][D/f0][H/f1][W/f2], out [n][D][H][W] DEVICE; x0 [n][D][H][W] DEVICE or null (the block replication of y);
 * guide [n][D][H][W] DEVICE or null (every pass is guided by its own input); k0 [f0], k1 [f1], k2 [f2] HOST, the block operator A of
 * inr_tvsr3d_block_apply; levels [n_levels] HOST.  From x = x0, for each level h_l and each of n_iter passes:
 *   x' = NLM(x) with INR_NLM_CENTER_ONE and the scalar h2 = h_l^2;   x <- x' - relax * N(A x' - y),  N the replication over a block:
 *   with relax = 1, A x = y afterwards up to rounding.  change [n_levels * n_iter][n] DEVICE or null: mean |x_new - x_old| of every pass,
 * from per-block partials added in a fixed order.  The workspace (DEVICE, 16-byte aligned, the planner's doubles) holds two HR states and
 * the partials.  No atomics and no host read anywhere: two runs give the same bits, whatever the grid, the stream and a volume's place
 * in the batch.  The _f32 forms convert on load and round once on the last store.  n_groups == 0 / n_volumes == 0 succeed and launch
 * nothing.  Refusals, before any device work: INR_E_INVALID for a null out, x or y, a size below 1 or a volume of 2^31 voxels or more,
 * a radius out of range, C outside 1 .. INR_NLM_MAX_CHANNELS, a null guide with C > 1, a scalar h2 that is not finite and > 0, a center
 * that is neither constant, out overlapping x or guide, factors outside 1 .. INR_TVSR_MAX_FACTOR, an extent that is no multiple of its
 * factor, a kernel factor that is not finite or does not sum to 1, n_levels * n_iter outside 0 .. INR_NLM_MAX_PASSES, a level that is not
 * finite and > 0, relax outside (0, 1]; INR_E_WORKSPACE for a null or short workspace (INR_E_ALIGN: misaligned).  The planner returns 0 for
 * sizes every call refuses. */
#define INR_NLM_MAX_SEARCH 5
#define INR_NLM_MAX_PATCH 2
#define INR_NLM_MAX_CHANNELS 16
#define INR_NLM_MAX_PASSES 10000
#define INR_NLM_CENTER_MAX 0
#define INR_NLM_CENTER_ONE 1
int inr_nlm3d(double* out, const double* x, const double* guide, double h2, const double* h2_map, const double* sigma2, const uint8_t* mask,
              int n_groups, int channels, int depth, int height, int width, int s0, int s1, int s2, int r0, int r1, int r2, int center,
              void* stream);
int inr_nlm3d_f32(float* out, const float* x, const float* guide, double h2, const float* h2_map, const float* sigma2, const uint8_t* mask,
                  int n_groups, int channels, int depth, int height, int width, int s0, int s1, int s2, int r0, int r1, int r2, int center,
                  void* stream);
int64_t inr_nlm_upsample_workspace_doubles(int n_volumes, int depth, int height, int width, int f0, int f1, int f2);
int inr_nlm_upsample(double* out, double* change, const double* y, const double* x0, const double* guide, int n_volumes, int depth, int height,
                     int width, int f0, int f1, int f2, const double* k0, const double* k1, const double* k2, const double* levels,
                     int n_levels, int n_iter, double relax, int s0, int s1, int s2, int r0, int r1, int r2, double* workspace,
                     int64_t workspace_doubles, void* stream);
int inr_nlm_upsample_f32(float* out, double* change, const float* y, const float* x0, const float* guide, int n_volumes, int depth, int height,
                         int width, int f0, int f1, int f2, const double* k0, const double* k1, const double* k2, const double* levels,
                         int n_levels, int n_iter, double relax, int s0, int s1, int s2, int r0, int r1, int r2, double* workspace,
                         int64_t workspace_doubles, void* stream);

/* ---- second-order TGV super-resolution under the block operator: a prior that does not terrace smooth intensity -------
 * No counterpart in the reference.  Images, sides, factors and the HOST `kernel` as for inr_tvsr_solve2d.  An auxiliary field
 * v = (v0, v1) [n_images][2][H][W] absorbs the smooth part of the gradient (Bredies, Kunisch, Pock 2010; Knoll et al. 2011):
 * inr_tgv_solve2d: out = n_iter iterations of Chambolle-Pock (tau = sigma = 1/sqrt(12)) on
 *   min_{x, v} 1/2 sum_i w_i ((A x)_i - y_i)^2 + lam1 sum_j H_alpha(|(grad x)_j - v_j|) + lam0 sum_j |(Ev)_j|_F,
 *   lam1 = lambda, lam0 = ratio * lambda;  Ev = (e00, e11, e01) = (d0 v0, d1 v1, (d1 v0 + d0 v1) / 2) with d0 / d1 the forward
 *   differences of grad (zero last row / column), |Ev|_F = sqrt(e00^2 + e11^2 + 2 e01^2), div0 / div1 the negative adjoints of d0 / d1
 *   (A, grad, div, H_alpha: inr_tvsr_solve2d), from x = xbar = x0, v = vbar = 0, p = 0, r = 0:
 *     q <- (p + sigma (grad(xbar) - vbar)) / (1 + sigma alpha / lam1);  p <- q / max(1, |q| / lam1)
 *     s <- r + sigma E(vbar);                                           r <- s / max(1, |s|_F / lam0)
 *     u <- x + tau div(p);  x' <- u - A^T(c (A u - y)), c_i = tau w_i / (1 + tau w_i |k|^2)
 *     v0' <- v0 + tau (p0 + div0 r00 + div1 r01);  v1' <- v1 + tau (p1 + div1 r11 + div0 r01)
 *     xbar <- 2 x' - x;  vbar <- 2 v' - v;  x <- x';  v <- v'
 *   The steps hold because |(grad x - v, Ev)|^2 <= 12 (|x|^2 + |v|^2) (csrc/tgv.hip).  lambda == 0 skips the dual phases: p, r and v
 *   stay 0 and the result is the data-only iteration (ratio is still checked).  y, weight, x0 as for inr_tvsr_solve2d (weight 0: a
 *   missing datum whose y is never read; x0 null: block replication).  v_out [n][2][H][W] DEVICE or null: the field at the end.
 *   energy / change [n] DEVICE doubles or null: the objective at the returned fp64 (x, v) (fixed order, no float atomics) and
 *   max |x' - x| of the last iteration, on x only (0 for n_iter == 0, which returns x0 and v = 0).  ONE launch, no host read: one
 *   workgroup of 1,024 threads per image runs all iterations with two workgroup barriers per iteration; images beyond the CU count are
 *   queued.  The _f32 form reads y / weight / x0 and writes out and v_out as fp32, fp64 inside, rounded once.  n_images == 0
 *   succeeds and launches nothing.
 * workspace: inr_tgv_workspace_doubles(n_images, H, W) = 11 n H W doubles (the state x | xbar | v0 | v1 | vbar0 | vbar1 | p0 | p1 |
 * r00 | r11 | r01 of every image; n = 1 for n_images == 0), 16-byte aligned; 0 for sizes that would be refused.  Refusals, all before
 * any device work: INR_E_INVALID (null out / y / kernel, n_images < 0, factors or sizes out of range, H or W no multiple of its
 * factor, n_iter < 0, a negative or non-finite lambda / alpha, a ratio that is not finite or <= 0, a kernel that is not finite or does
 * not sum to 1), INR_E_WORKSPACE (null or short workspace), INR_E_ALIGN (workspace off a 16-byte boundary). */
int64_t inr_tgv_workspace_doubles(int n_images, int height, int width);
int inr_tgv_solve2d(double* out, double* v_out, double* energy, double* change, const double* y, const double* weight, const double* x0,
                    int n_images, int height, int width, int f0, int f1, const double* kernel, double lambda, double ratio, double alpha,
                    int n_iter, double* workspace, int64_t workspace_doubles, void* stream);
int inr_tgv_solve2d_f32(float* out, float* v_out, double* energy, double* change, const float* y, const float* weight, const float* x0,
                        int n_images, int height, int width, int f0, int f1, const double* kernel, double lambda, double ratio,
                        double alpha, int n_iter, double* workspace, int64_t workspace_doubles, void* stream);

/* ---- the reader study's image scores (implicit-neural-representations/perceptual_similarity_tests/perceptual_similarity.m, HPF.m) -----
 * The scores that the reference computes in MATLAB on the panels of prepare_qual_images.py, by the DEFINITIONS of DESIGN.md 4g:
 * MATLAB's documented defaults for ssim, immse, imfilter and fspecial('unsharp'), and Wang et al. 2003 for MS-SSIM.  No MATLAB output
 * has ever been compared against; tests/perceptual_common.py restates the definitions in float64 NumPy / SciPy.  FSIM.m and SR_SIM.m
 * (perceptual_similarity.m:53-54) are third-party files under a research-only licence and have no counterpart here.
 * Images are [n_images][H][W] fp32, all arithmetic is fp64, results are doubles; 1 <= n_images <= 65535, H, W >= 1.
 * Window: r = ceil(3 sigma) <= INR_PERCEPTUAL_MAX_RADIUS, g[k] = exp(-k^2 / (2 sigma^2)) normalised, separable, indices clamped
 * to the edge.  Refusals, all before any device work: INR_E_INVALID (null pointers, n_images < 1, sizes < 1, sigma <= 0 or a
 * radius above 7, data_range <= 0, n_scales outside 1..INR_PERCEPTUAL_MAX_SCALES), INR_E_WORKSPACE (a null or short workspace),
 * INR_E_ALIGN (a device pointer off a 16-byte boundary).
 * workspace: typed, like inr_rescale2d's -- inr_perceptual_workspace_doubles(n_images, H, W, n_scales) DOUBLES serve every entry
 * point below for that many images of that shape and that many scales (n_scales = 1 for inr_ssim2d_gauss); inr_image_mse and
 * inr_hf_gain need inr_perceptual_workspace_doubles(n_images, 1, 1, 1), which every larger view of the same n_images covers.  0 for
 * arguments that would be refused.  Plain launches and fixed-order reductions: repeated calls are bit-equal, and an image's results depend
 * neither on the rest of the batch nor on where a pixel falls in a tile. */
#define INR_PERCEPTUAL_MAX_RADIUS 7
#define INR_PERCEPTUAL_MAX_SCALES 8
int64_t inr_perceptual_workspace_doubles(int n_images, int height, int width, int n_scales);
/* ssim(A, ref) of perceptual_similarity.m:50: mx = F x, vx = max(F(x^2) - mx^2, 0), vxy = F(xy) - mx my, C1 = (.01 L)^2,
 * C2 = (.03 L)^2, l = (2 mx my + C1) / (mx^2 + my^2 + C1), cs = (2 vxy + C2) / (vx + vy + C2); ssim[b] = the mean of l cs over the
 * FULL image (no border crop, biased variance: both unlike inr_ssim2d); mean_cs (nullable) [n_images] = the mean of cs; map
 * (nullable) [n_images][H][W] fp32 = l cs. */
int inr_ssim2d_gauss(double* ssim, double* mean_cs, float* map, const float* x, const float* y, int n_images, int height, int width,
                     double sigma, double data_range, double* workspace, int64_t workspace_doubles, void* stream);
/* multissim(A, ref) of perceptual_similarity.m:52: v_s = mean(cs) at scales 0 .. n_scales-2, v_last = mean(l cs), out[b] =
 * prod v_s ^ weights[s] (pow: a negative v_s under a fractional weight gives NaN); between scales both images become their 2 x 2
 * block means, indices clamped, ceil(H/2) x ceil(W/2), kept in fp64.  weights: n_scales HOST doubles.  per_scale (nullable)
 * [n_images][n_scales] receives the v_s. */
int inr_msssim2d(double* out, double* per_scale, const float* x, const float* y, int n_images, int height, int width,
                 const double* weights, int n_scales, double sigma, double data_range, double* workspace, int64_t workspace_doubles,
                 void* stream);
/* imfilter(single(image), H) of HPF.m:8 for any 3 x 3 H: correlation, ZERO padding, same size; k9: 9 HOST doubles, row-major; the
 * fp64 sum is rounded once to fp32. */
int inr_filter3x3(float* out, const float* in, int n_images, int height, int width, const double* k9, void* stream);
/* immse(A, ref) of perceptual_similarity.m:51: out[b] = mean (x - y)^2 over per_image samples. */
int inr_image_mse(double* out, const float* x, const float* y, int n_images, int64_t per_image, double* workspace,
                  int64_t workspace_doubles, void* stream);
/* power_diff / pow_inter of perceptual_similarity.m:42-47 on the high-passed images: out[b] = sum max(h_sr - h_inter, 0)^2 /
 * sum h_inter^2. */
int inr_hf_gain(double* out, const float* h_sr, const float* h_inter, int n_images, int64_t per_image, double* workspace,
                int64_t workspace_doubles, void* stream);

/* ---- a-13/a-14: RAMS forward + predict_tensor (network.py:91-155, prediction.py:76-83) --------------------------
 * x [B][H][W][channels] fp32 (uint16-range values) -> out [B][scale*H][scale*W] fp32.  clip_round != 0 applies
 * predict_tensor's clip to [0, 2^16] and round-half-to-even.
 * `params` is ONE packed fp32 buffer with weight normalisation already folded (kernel = g*v/||v||, norm over every
 * axis but the output channel); every segment starts at a multiple of 4 floats, in this order:
 *   stem: w[27][32], b[32];
 *   n_rfab x RFAB: conv1 w[27][32][32], b[32]; conv2 w, b; squeeze w[32][32/r], b[32/r]; excite w[32/r][32], b[32];
 *   trunk conv w, b;
 *   (channels/3) x { RFAB as above; reduction conv w[27][32][32], b[32] };
 *   up conv w[27][32][32] (output channels scale^2, zero-padded to 32), b[32];
 *   RTAB: conv1 w[9][T][T], b[T]; conv2 w, b; squeeze w[T][max(T/r,1)], b; excite w[max(T/r,1)][T], b[T];
 *   global conv w[9][T][scale^2], b[scale^2].
 * (conv kernels are in TensorFlow order: tap-major [k1][k2][k3], then input channel, then output channel.) */
int64_t inr_rams_param_count(const inr_rams_desc_t* desc);
size_t  inr_rams_workspace_bytes(const inr_rams_desc_t* desc, int batch, int height, int width);
int inr_rams_forward(const inr_rams_desc_t* desc, const float* params, const float* x, float* out, int batch,
                     int height, int width, int clip_round, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a-15 (loss side): RAMS shift-tolerant losses (multi-image-super-resolution/utils/loss.py:26-75 l1_loss, :77-127
 * psnr).  y_true, y_pred, mask: [n_images][size][size] fp32.  For every label shift (i, j) in [0, 2*border]^2 the
 * prediction cropped by `border` is compared with the shifted label window under the shifted mask after removing the
 * masked mean brightness difference; out[b] (double) = min over shifts of the masked mean |.| (mode 0, cL1) or
 * max over shifts of 10*log10(65535^2 / masked mean square) (mode 1, cPSNR; the reference then averages over b). */
size_t inr_rams_shift_loss_workspace_bytes(int n_images, int border);
int inr_rams_shift_loss(double* out, const float* y_true, const float* y_pred, const float* mask, int n_images, int size,
                        int border, int mode, void* workspace, size_t workspace_bytes, void* stream);
/* building blocks of the network half of `Trainer.train_step` (utils/training.py:193-209) for the 3x3x3 convolutions
 * 32 -> 32 that carry >= 99 % of RAMS' work (utils/network.py:29-35).  Layouts as in inr_rams_forward: activations
 * [B][D1][D2][D3][32] fp32 (NDHWC), folded kernel w[27 taps][32 cin][32 cout], bias[32]; pad 1 = 'same', 0 = 'valid'.
 *   forward: y = conv(x, w) + bias (+ReLU)                                   -- the inference kernel, on its own
 *   dgrad  : dx = d loss / d x of a 'same' convolution, given dy             -- the same kernel on the flipped, transposed w
 *   wgrad  : gw[27][32][32] = d loss / d w, gb[32] = d loss / d bias (nullable) -- MFMA contraction over the voxels,
 *            fixed-order slab reduction (bitwise reproducible); arithmetic as in the training step: split-fp16 MFMA on
 *            operands staged in LDS (default), f32-input MFMA under inr_debug_set(14, 0); x and dy 16-byte aligned
 * (forward and dgrad here are the f32-input kernels; inside inr_rams_forward / inr_rams_train_* they follow key 14 too) */
int inr_rams_conv3d_forward(float* y, const float* x, const float* w, const float* bias, int B, int D1, int D2, int D3, int pad,
                            int relu, void* stream);
size_t inr_rams_conv3d_dgrad_workspace_bytes(void);
int inr_rams_conv3d_dgrad(float* dx, const float* dy, const float* w, int B, int D1, int D2, int D3, void* workspace,
                          size_t workspace_bytes, void* stream);
size_t inr_rams_conv3d_wgrad_workspace_bytes(int B, int D1, int D2, int D3, int pad);
int inr_rams_conv3d_wgrad(float* gw, float* gb, const float* x, const float* dy, int B, int D1, int D2, int D3, int pad,
                          void* workspace, size_t workspace_bytes, void* stream);

/* the loss half of `Trainer.train_step` (utils/training.py:193-209): loss[b] = cL1 as above and grad_pred[b] =
 * upstream[b] * d loss[b] / d y_pred[b] ([n_images][size][size] fp32, zero on the `border` frame), taken through the
 * best shift as TensorFlow's reduce_min does; upstream nullable (= 1: the gradient of sum_b loss[b], what
 * tape.gradient of the loss vector returns). */
size_t inr_rams_shift_loss_grad_workspace_bytes(int n_images, int border);
int inr_rams_shift_loss_grad(double* loss, float* grad_pred, const float* y_true, const float* y_pred, const float* mask,
                             const float* upstream, int n_images, int size, int border, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- a-15 (loss side): the shift-tolerant SSIM, cSSIM (multi-image-super-resolution/utils/loss.py:131-177 `ssim`).
 * y_true, y_pred, mask: [n_images][size][size] fp32; c = size - 2*border, P = y_pred cropped by `border`.  For every label
 * shift (i, j) in [0, 2*border]^2, with L and M the c x c windows of y_true and mask at offset (i, j):
 *   tot = sum M;  b = sum(L M - P M) / tot;  x = (P M + b) M;  y = L M;  s_ij = SSIM_tf(x, y, max_val = 65535);
 *   clear_only != 0: s_ij = (s_ij - 1) * tot / c^2 + 1;            out[b] (double) = max over (i, j) of s_ij
 * (the reference then averages over b).  SSIM_tf is tf.image.ssim with its defaults: window = outer product of
 * g[k] ~ exp(-k^2 / (2 * 1.5^2)), k = -5..5, normalised to sum 1, applied as a 'VALID' correlation (maps of (c-10)^2);
 * mu_x = G*x, mu_y = G*y, l = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1), cs = (2 G*(xy) - 2 mu_x mu_y + C2) /
 * (G*(x^2 + y^2) - mu_x^2 - mu_y^2 + C2), C1 = (0.01 * 65535)^2, C2 = (0.03 * 65535)^2, no sample-covariance correction;
 * SSIM = mean of l * cs over the map.  The mask need not be binary (no power of M is folded).  All arithmetic is fp64 on the
 * fp32 inputs, every reduction has a fixed order: repeated calls are bit-equal.  On return the first
 * n_images * (2*border+1)^2 doubles of the workspace hold the table s_ij ([b][i][j]).
 * A window without a clear pixel (tot = 0) is undefined in the reference (0/0): its s_ij is NaN here, the maximum passes NaN
 * entries over, and out[b] is NaN only when every shift of image b is.
 * Checked before any device work: null pointers, 1 <= n_images <= 65535, 0 <= border <= 16, size <= 8192 and
 * size - 2*border >= 11 (INR_E_INVALID); workspace null or too small (INR_E_WORKSPACE), not 8-byte aligned (INR_E_ALIGN).
 * The definition is restated from TensorFlow's documentation and the reference's source: it is pinned to a float64
 * restatement and to analytic cases, not to TensorFlow's own output. */
size_t inr_rams_shift_ssim_workspace_bytes(int n_images, int size, int border);
int inr_rams_shift_ssim(double* out, const float* y_true, const float* y_pred, const float* mask, int n_images, int size,
                        int border, int clear_only, void* workspace, size_t workspace_bytes, void* stream);
/* loss[b] = 1 - cSSIM_b as above and grad_pred[b] = upstream[b] * d loss[b] / d y_pred[b] ([n_images][size][size] fp32, zero
 * on the `border` frame), taken through image b's best shift as TensorFlow's reduce_max does (the first best shift on an exact
 * tie), including the path through the brightness bias b, which depends on every masked pixel of P.  upstream nullable (= 1).
 * The table s_ij is left in the workspace as by inr_rams_shift_ssim; the same argument checks apply. */
size_t inr_rams_shift_ssim_grad_workspace_bytes(int n_images, int size, int border);
int inr_rams_shift_ssim_grad(double* loss, float* grad_pred, const float* y_true, const float* y_pred, const float* mask,
                             const float* upstream, int n_images, int size, int border, int clear_only, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- (f)-1: three-compartment hybrid fit (PIA.py:240-283 `three_compartment_fit` / `hybrid_fit`, called at
 * superresHybrid.py:140).  signals: [n_voxels][16] fp64, b-major over b = {0,150,1000,1500} x TE = {0,13,93,143}
 * (the order of PIA.py:263-265).  Runs scipy's bounded trust-region-reflective least squares (what
 * curve_fit(method='trf', maxfev=5000) executes: 2-point Jacobian, x_scale = 1, ftol = xtol = gtol = 1e-8, exact
 * trust-region solver) with the reference's p0 and bounds (PIA.py:269-272), one voxel per lane, fp64.
 * params: [n_voxels][8] = D_ep, D_st, D_lu, T2_ep, T2_st, T2_lu, V_ep, V_st (p0 where the fit exhausts maxfev,
 * PIA.py:276-277); status: scipy termination code (0 = maxfev, 1 gtol, 2 ftol, 3 xtol, 4 both); nfev; cost =
 * half the residual sum of squares at the returned point.  Non-finite input is the caller's to reject
 * (curve_fit(check_finite=True) raises). */
int inr_hybrid_fit(double* params, int* status, int* nfev, double* cost, const double* signals, int64_t n_voxels,
                   void* stream);

/* ---- PIA: the physics-informed autoencoder (PIA.py:16-155 `PIA`; PIA.py:286-327 `detect_PIDS_slice`) --------------------------
 * Encoder n_signals -> hidden[0] -> ... -> hidden[n_hidden-1] (Linear + LeakyReLU each), three predictors (D, T2, v) of
 * predictor_depth x (Linear + LeakyReLU) and a Linear to 3, then D = D_mean + D_delta tanh(.), T2 = T2_mean + T2_delta tanh(.),
 * v = softmax(.), and the analytic decoder signal[a] = 1000 float(sum_c v_c exp(-b_a / 1000 D_c) exp(-TE_a / T2_c)), acquisition
 * a = b index * n_te + TE index (PIA.py:123-129).  Dtypes are the reference's: D float64 (D_mean is a float64 tensor), T2 and v
 * float32, the decoder's sum in float64, rounded once into the float32 signal.
 * Flat parameter buffer: the 2 n_hidden + 3 (2 predictor_depth + 2) tensors of `named_parameters()` back to back WITHOUT padding
 * (968,169 floats for the default shape), so that it is the reference's parameter vector; tensors start at any 4-byte boundary
 * and the kernels load them accordingly.
 * inr_pia_param_count / _offsets are defined for every valid descriptor.  The kernels serve n_signals == 16, widths that are
 * multiples of 16, a last width of 256 or 512 and predictor_depth == 1 (INR_E_INVALID otherwise, before any device work).
 * GEMMs run on the f32-input MFMA (v_mfma_f32_16x16x4_f32); gradient slabs are summed in a fixed order: no float atomics. */
#define INR_PIA_MAX_HIDDEN 8
#define INR_PIA_MAX_TABLE  8
typedef struct inr_pia_desc {
    int    n_signals;                       /* 16 */
    int    n_hidden;                        /* encoder layers (5) */
    int    hidden[INR_PIA_MAX_HIDDEN];      /* 32, 64, 128, 256, 512 */
    int    predictor_depth;                 /* 1 */
    int    n_b, n_te;                       /* n_b * n_te == n_signals */
    float  leaky_slope;                     /* 0.01 (nn.LeakyReLU default) */
    double b_values[INR_PIA_MAX_TABLE];     /* 0, 150, 1000, 1500 */
    double te_values[INR_PIA_MAX_TABLE];    /* 0, 13, 93, 143 */
    double D_mean[3], D_delta[3], T2_mean[3], T2_delta[3];
} inr_pia_desc_t;
int64_t inr_pia_param_count(const inr_pia_desc_t* desc);                 /* -1 for a bad descriptor */
/* offsets[k] of tensor k in named_parameters() order; max_tensors >= 2 n_hidden + 3 (2 predictor_depth + 2) */
int     inr_pia_param_offsets(const inr_pia_desc_t* desc, int64_t* offsets, int max_tensors);
/* training != 0: what forward_train / backward_train / fit_step need for n rows (every activation, gradient buffers, slabs);
 * training == 0: what inr_pia_forward needs for chunks of n rows.  0 for a descriptor the kernels do not serve. */
size_t  inr_pia_workspace_bytes(const inr_pia_desc_t* desc, int64_t n, int training);
/* model(x) without a stash, `chunk_rows` rows at a time (a whole volume's voxels in one call; results do not depend on the
 * chunk size, bit for bit).  x [n][16]; signal [n][16] (nullable); D [n][3] float64, T2 [n][3], v [n][3] (nullable together). */
int inr_pia_forward(const inr_pia_desc_t* desc, const float* params, const float* x, int64_t n, float* signal, double* D, float* T2,
                    float* v, int64_t chunk_rows, void* workspace, size_t workspace_bytes, void* stream);
/* the reference's own loop (model(x) -> any torch loss -> backward() -> torch.optim.Adam) on these kernels: the forward keeps
 * every layer's ACTIVATION in `workspace` (the LeakyReLU derivative is its sign; the 3-wide outputs are re-computed), the
 * backward takes d loss / d signal, D, T2, v (each nullable = zero) and writes every element of `grads` (flat, parameter
 * order).  `params` and `x` must still hold what the forward ran on; one backward per forward on a workspace -- the library
 * keeps no record of it: the caller pairs them. */
int inr_pia_forward_train(const inr_pia_desc_t* desc, const float* params, const float* x, int64_t n, float* signal, double* D,
                          float* T2, float* v, void* workspace, size_t workspace_bytes, void* stream);
int inr_pia_backward_train(const inr_pia_desc_t* desc, const float* params, float* grads, const float* x, const float* g_signal,
                           const double* g_D, const float* g_T2, const float* g_v, int64_t n, void* workspace,
                           size_t workspace_bytes, void* stream);
/* one step on the loss the class trains with, mean(PIDS * (signal - x)^2) (PIA.py:153; pids [n][16], nullable = 1): forward,
 * loss, backward, fixed-order reduction and Adam (torch's single-tensor arithmetic, as inr_adam_step), all enqueued on
 * `stream`; *loss (device) receives the loss BEFORE the update.  `step` is the 1-based Adam step. */
int inr_pia_fit_step(const inr_pia_desc_t* desc, float* params, float* grads, float* m, float* v, const float* x, const float* pids,
                     int64_t n, int64_t step, double lr, double beta1, double beta2, double eps, float* loss, void* workspace,
                     size_t workspace_bytes, void* stream);
/* Launch families of the PIA kernels, counted like INR_LF_* but numbered from 0 and read through an entry point of their own
 * (the INR_LF_* ids and their count are pinned by callers); inr_launch_counts_reset() clears them too. */
#define INR_PIA_LF_FWD   0   /* pia_gemm_kernel<FWD>: layer forward, f32-input MFMA 16x16x4, LeakyReLU epilogue */
#define INR_PIA_LF_DX    1   /* pia_gemm_kernel<DX>: input gradient (the three heads' products in one K-loop) */
#define INR_PIA_LF_DW    2   /* pia_gemm_kernel<DW>: parameter gradient, row-split slabs */
#define INR_PIA_LF_HEAD  3   /* pia_head_kernel: 3-wide outputs, tanh / softmax, decoder, loss and their backward, a wave per row */
#define INR_PIA_LF_COUNT 4
int inr_pia_launch_count(int family, int64_t* count);
/* detect_PIDS_slice (PIA.py:286-327): S [n_pixels][4 (b)][4 (TE)] float64, bvals [4] float64 ->
 * adc_high [n_pixels] (ADC > 3), adc_negative [n_pixels] (ADC < 0), b_decay [n_pixels][4 (TE)][3], te_decay [n_pixels][4 (b)][3],
 * all 0 / 1 as fp32.  A decay entry is (s[k + 1] - trunc(s[k]) >= 0): the reference truncates the left neighbour toward zero
 * (it stores it into an integer array, PIA.py:312-313), and so does this. */
int inr_pids_slice(float* adc_high, float* adc_negative, float* b_decay, float* te_decay, const double* S, const double* bvals,
                   int64_t n_pixels, void* stream);

/* AutoERD acceptance weights -- the per-pixel outlier rejection master.py runs before a 2-D fit (master.py:77-93).
 * values: [n_pixels][n_acquisitions] fp64 (every acquisition of the slice at that pixel); accept: same shape, fp32, 1 = keep,
 * 0 = reject.  Each pixel's sample is split in two exactly as sklearn.cluster.AgglomerativeClustering(n_clusters=2,
 * affinity='euclidean', linkage='complete') splits it (scipy's nearest-neighbour chain + stable sort: ties fall as they do
 * there); rule 1 (--erd 1, majority voting): a cluster holding >= 2/3 of the acquisitions rejects the other; rule 2 (--erd 2,
 * intensity-cognisant): where erd_map (fp32 [n_pixels], nullable = everywhere) is positive, the cluster with the lower mean
 * is rejected.  2 <= n_acquisitions <= 32.
 * A pixel with a non-finite value (NaN, +-inf) among its n_acquisitions, or whose largest pairwise distance max - min overflows
 * to +inf, is not clustered: all its accept entries are 1 (sklearn refuses such input; inr_auto_erd_volume keeps everything on
 * exactly the same pixels).  The other pixels are unaffected. */
int inr_auto_erd(float* accept, const double* values, const float* erd_map, int64_t n_pixels, int n_acquisitions, int rule,
                 void* stream);

/* Whole-volume AutoERD with the ERD-weighted direction means and ADC maps of david.py:44-91, one launch for all pixels, float64.
 * Every array is a stack of planes, pixels contiguous: values, accept, accept_in, adc [n_acquisitions][n_pixels]; the four maps
 * [n_groups][n_pixels]; b0, erd_map [n_pixels].  group_sizes [n_groups] (HOST array, 1 <= n_groups <= INR_ERD_VOLUME_MAX_GROUPS, every
 * size >= 1, summing to n_acquisitions) cuts the acquisitions into consecutive groups (the gradient directions).
 * rule 1 / rule 2: the pixel's sample is split and acquisitions are rejected exactly as inr_auto_erd does it (the same partition,
 * ties included; erd_map is float64 here and nullable = positive everywhere; only entries > 0 reject, so 0, negative, -inf and NaN
 * keep everything); accept_in must be null.  rule 0: no clustering -- accept_in (nullable = all ones) is used as the acceptance
 * weights as it is.  A pixel with a NON-FINITE value among its acquisitions (or whose extent overflows) is not clustered and keeps
 * every acquisition; its sums follow IEEE.  2 <= n_acquisitions <= 32.
 * Per group, three sequential sums over its acquisitions in index order, each from 0.0: sum_image += v, sum_accepted += v * a,
 * sum_accepts += a; then direction_mean = sum_image / size, accepted_mean = sum_accepted / sum_accepts -- NaN (0 / 0) where a
 * group is wholly rejected, and then accepted_adc is NaN too -- and adc(v) = -log(v / (b0 + 1e-7) + 1e-7) / b * 1000 of both
 * means (ONE factor 1000: david.py:82-85); adc (nullable) receives adc(v) of every single acquisition (david.py:68-69).
 * Every output is nullable on its own; b0 is needed only where an ADC output is asked for.  accept receives 1.0 = keep, 0.0 =
 * reject (under rule 0 a copy of the weights used).  b != 0.  n_pixels == 0 is a no-op. */
#define INR_ERD_VOLUME_MAX_GROUPS 8
int inr_auto_erd_volume(double* accept, double* direction_mean, double* accepted_mean, double* direction_adc, double* accepted_adc,
                   double* adc, const double* values, const double* b0, const double* erd_map, const double* accept_in,
                   int64_t n_pixels, int n_acquisitions, const int* group_sizes, int n_groups, double b, int rule, void* stream);

/* ---- the soft-ERD INR family (INR_ERD.py:28-67 `Siren`, prepare_qual_images.py:66-102) --------------------------------------------
 * Trunk: SineLayer(in -> H, first), hidden_layers x SineLayer(H -> H), Linear(H -> H) + ReLU; head Linear(H -> 1) + ReLU; the
 * in-module perturbation p = eps tanh(W2 tanh(W1 [x, sample] + b1) + b2) ([n][1]) is ADDED TO EVERY coordinate component
 * before the trunk (INR_ERD.py:56-63; `sample` enters as the plain acquisition index).  The descriptor is inr_siren_desc_t
 * with out_features == 1, in_features <= 8, hidden_features in {64, 128}, hidden_layers <= 8 (INR_E_INVALID otherwise: there
 * is no other path).  Flat parameter buffer, every tensor padded to 16 bytes: trunk layer 0 .. hidden_layers + 1 (weight,
 * bias), head, perturb_linear, perturb_linear2.  Group A = trunk + head = [0, group_b), group B = the perturb branch.
 * Kernels: f32-input MFMA 32x32x2, hardware sin/cos, per-wave gradient slabs summed in a fixed order (bitwise reproducible). */
#define INR_ERD_RUNNING   0
#define INR_ERD_CONVERGED 1   /* the step whose forward loss was the first <= threshold has been applied; it was the last */
#define INR_ERD_COLLAPSED 2   /* every output of the last applied step's forward was 0 (tested first: it wins) */
int64_t inr_erd_param_count(const inr_siren_desc_t* desc);                  /* -1 for a descriptor the kernels do not serve */
/* offsets[2 t], offsets[2 t + 1] = weight / bias of tensor t (hidden_layers + 5 tensors), then group_b; max_entries counts them */
int     inr_erd_param_offsets(const inr_siren_desc_t* desc, int64_t* offsets, int max_entries);
size_t  inr_erd_workspace_bytes(const inr_siren_desc_t* desc, int64_t n);   /* 0 for a shape the kernels do not serve */
/* INR_ERD.py:54-67 forward at inference, `chunk_rows` rows per launch; the result does not depend on the chunk size, bit for bit */
int inr_erd_forward(const inr_siren_desc_t* desc, const float* params, const float* x, int64_t n, float* y, int sample, float eps,
                    int perturb, int64_t chunk_rows, void* stream);
/* One acquisition of INR_ERD.py:259-267: loss = mean(w (f(x; sample, eps) - target)^2) (weight nullable = 1) and its gradient
 * for every parameter.  accumulate != 0 adds loss and gradient to those of the previous calls on this workspace (same n), so
 * `grads` / `*loss` then hold the sums; the slabs are summed in a fixed order. */
int inr_erd_loss_grad(const inr_siren_desc_t* desc, const float* params, float* grads, const float* x, const float* target,
                      const float* weight, int64_t n, int sample, float eps, int perturb, int accumulate, float* loss,
                      void* workspace, size_t workspace_bytes, void* stream);
/* Adam with two parameter groups (INR_ERD.py:252-255, 272-273): lr_net for group A, lr_perturb for group B; the arithmetic of
 * inr_adam_step on each group's range.  `step` is the 1-based Adam step of both groups. */
int inr_erd_adam_step(const inr_siren_desc_t* desc, float* params, const float* grads, float* m, float* v, int64_t step,
                      double lr_net, double lr_perturb, double beta1, double beta2, double eps, void* stream);
/* The pre-training loop INR_ERD.py:201-217 without a host read per step: enqueues max_steps x (step kernel, reduce + Adam +
 * status kernel) and returns.  status (device, 16 bytes) = {int state, int steps_done, float last_loss, float y_max}; the
 * caller initialises it to {INR_ERD_RUNNING, 0, 0, 0} and reads it when it likes.  Every kernel returns at entry unless the
 * state is RUNNING, so a call on a finished status changes nothing.  Unweighted, perturbation off, one learning rate.
 * first_step = the 1-based Adam step of the first enqueued step (steps_done + 1 of a status that is still RUNNING).
 * Where the reference would, on a step that both converges and collapses, leave its loop with a freshly initialised network,
 * this reports COLLAPSED and the caller re-initialises and goes on. */
int inr_erd_pretrain(const inr_siren_desc_t* desc, float* params, float* grads, float* m, float* v, const float* x,
                     const float* target, int64_t n, int64_t first_step, int max_steps, double lr, double beta1, double beta2,
                     double eps, float threshold, int* status, void* workspace, size_t workspace_bytes, void* stream);
/* The fine-tuning step INR_ERD.py:252-273, n_steps times: loss = sum_s mean(w_s (f(x; s, eps) - g_s)^2) over the n_acq
 * acquisitions (targets, weights: [n_acq][n]; weights nullable) = n_acq accumulating step launches + one reduce / dual-Adam
 * launch.  losses [n_steps] (nullable) receives each step's loss before its update. */
int inr_erd_finetune(const inr_siren_desc_t* desc, float* params, float* grads, float* m, float* v, const float* x,
                     const float* targets, const float* weights, int n_acq, int64_t n, float perturb_eps, int64_t first_step,
                     int n_steps, double lr_perturb, double lr_net, double beta1, double beta2, double eps, float* losses,
                     void* workspace, size_t workspace_bytes, void* stream);
/* Soft-ERD acquisition weights and the weighted mean image (INR_ERD.py:143-158, 225-235), one launch for all pixels, float64:
 * values [n_pixels][K], b0 [n_pixels]; temp = max(mul exp(-slope mean(x) / b0), min_temp); where mean(x) > 2 noise_level:
 * weights = exp(x / temp) (UNNORMALISED, as the reference hands it to the loss) and mean_image = the softmax-weighted mean
 * (computed with the maximum subtracted); elsewhere weights = 1 / K and mean_image = mean(x).  b0 == 0 follows IEEE.
 * *nonfinite_count (device int) receives the number of non-finite weights. */
int inr_soft_erd(double* weights, double* mean_image, const double* values, const double* b0, int64_t n_pixels, int n_acquisitions,
                 double noise_level, double mul, double slope, double min_temp, int* nonfinite_count, void* stream);
/* Launch families of these kernels.  inr_launch_count serves them under ids of their own, above the INR_LF_* table (whose count
 * callers pin); inr_launch_counts_reset() clears them too. */
#define INR_LF_ERD_BASE    32
#define INR_LF_ERD_STEP    32   /* erd_step_kernel<H, train>: forward + loss + backward of 32 rows per wave */
#define INR_LF_ERD_REDUCE  33   /* erd_reduce_kernel: fixed-order slab sum (+ dual Adam, + status) */
#define INR_LF_ERD_FORWARD 34   /* erd_step_kernel<H, inference> */
#define INR_LF_ERD_SOFT    35   /* soft_erd_kernel */
#define INR_LF_ERD_END     36

/* ---- spatial derivatives of a fitted SIREN (nn_mri.py:205-221 `gradient`, `divergence`, `laplace`) -------------------------------
 * The reference differentiates the network with two torch.autograd.grad passes with create_graph=True (a graph of the first
 * backward pass, then its backward).  These entry points evaluate the same quantities in FORWARD mode, without a stash and
 * without autograd: per row and layer they carry the value, one tangent per coordinate axis and a Laplacian accumulator
 * (DESIGN.md 4d), on the f32-input MFMA (v_mfma_f32_32x32x2_f32) with the hardware sin / cos of the sine-layer epilogues.
 *   y[n]               = network(features(x))                          (no clamp)
 *   grad[n][d_tangent] = d y / d x_i, i < d_tangent                    (nullable)
 *   lap[n]             = sum_{i < d_tangent} d^2 y / d x_i^2           (nullable; without it the accumulator is neither computed
 *                                                                       nor carried)
 * x[n][d] are the network's coordinates -- the [-1, 1] coordinates of inr_mgrid; multiply a first derivative along axis a by
 * 2 / (shape[a] - 1) (a second one by its square) for per-voxel units.  B == NULL: the coordinates feed the network
 * (in_features == d); otherwise features = [sin(2 pi x B^T) | cos(2 pi x B^T)], B[m][d], in_features == 2 m, as inr_fourier_map.
 * d_tangent names the LEADING axes to differentiate along (1 <= d_tangent <= d): a DWI volume's grid (x, y, z, b) takes 3.
 * `params` is the flat buffer of inr_siren_param_offsets.  Rows are processed `chunk_rows` at a time in `workspace`
 * (inr_siren_jet_workspace_bytes(desc, d, m, min(chunk_rows, n), want_laplacian) bytes, m = 0 without B; sized for d tangents, so
 * it serves every d_tangent); a row's bits depend neither on the chunk size nor on which of grad / lap were asked for, and
 * repeated calls are bit-equal (fixed summation order, no float atomics).  Both calls only enqueue.
 * Served: out_features == 1, 1 <= d <= 4, hidden width a multiple of 32 up to 1024, at least one hidden layer; anything else,
 * and a null desc / params / x / shape / y, is INR_E_INVALID with a message before any device work; a null or short workspace is
 * INR_E_WORKSPACE, a params or workspace pointer off a 16-byte boundary INR_E_ALIGN, likewise before any device work.
 * The split-fp16 operand path of the fit is not used here. */
size_t inr_siren_jet_workspace_bytes(const inr_siren_desc_t* desc, int d, int m, int64_t chunk_rows, int want_laplacian);
/* nn_mri.py:205-221 on explicit coordinate rows: replaces gradient(y, x) / laplace(y, x) = two autograd.grad passes with
 * create_graph=True over model(x). */
int inr_siren_jet(const inr_siren_desc_t* desc, const float* params, const float* x, int64_t n, int d, int d_tangent, const float* B,
                  int m, float* y, float* grad, float* lap, int64_t chunk_rows, void* workspace, size_t workspace_bytes,
                  void* stream);
/* the same on the dense grid get_mgrid(shape) (dim == d axes), coordinates generated in the kernels as by inr_siren_reconstruct:
 * replaces laplace(model(input_mapping(get_mgrid(shape), B)), coords) of nn_mri.py:205-221, i.e. two autograd.grad passes with
 * create_graph=True over the whole re-sampling grid.  Bit-equal with inr_siren_jet on the rows of inr_mgrid(shape). */
int inr_siren_jet_grid(const inr_siren_desc_t* desc, const float* params, const int64_t* shape, int dim, int d_tangent,
                       const float* B, int m, float* y, float* grad, float* lap, int64_t chunk_rows, void* workspace,
                       size_t workspace_bytes, void* stream);
/* Launch families of these kernels (nn_mri.py:205-221 has no counterpart: each stands for a slice of the two autograd.grad
 * passes), counted like INR_LF_* but numbered from 0 and read through inr_jet_launch_count; inr_launch_counts_reset() clears
 * them too.  Per chunk of rows: one INPUT launch, one LAYER launch per sine layer (one fewer without B: the first layer is the
 * INPUT launch), one HEAD. */
#define INR_JET_LF_INPUT 0   /* jet_fourier_kernel / jet_first_kernel: jets of the Fourier features, or the first sine layer on the VALU */
#define INR_JET_LF_LAYER 1   /* jet_layer_kernel<J>: one sine layer on J planes, f32-input MFMA 32x32x2 */
#define INR_JET_LF_HEAD  2   /* jet_head_kernel: J row dots, a wave per row */
#define INR_JET_LF_COUNT 3
int inr_jet_launch_count(int family, int64_t* count);

/* ---- the WIRE complex-Gabor INR (INRmodel.py:66-120 `ComplexGaborLayer2D`; wiretest.ipynb cell 2 stacks it) -----------------------
 * Layer 0 holds two REAL Linear(in -> H) (`linear`, `scale_orth`), layers 1 .. hidden_layers two COMPLEX Linear(H -> H) each, the
 * head is a complex Linear(H -> 1) whose real part is the output.  With lin = linear(h), orth = scale_orth(h), w = omega_0,
 * s = scale_0 a layer gives  exp(i w lin) exp(-s^2 (|lin|^2 + |orth|^2)), evaluated in real arithmetic as
 *     A = exp(-w lin_i - s^2 (lin_r^2 + lin_i^2 + orth_r^2 + orth_i^2)),  out = A cos(w lin_r) + i A sin(w lin_r)
 * (ONE exponential of the summed exponent).  No complex type crosses this ABI: a complex tensor is its interleaved (re, im)
 * float pairs, torch's own layout (view_as_real).  s^2 is the fp32 product first_scale * first_scale (hidden_scale likewise).
 * Flat parameter buffer (fp32, every tensor padded to 16 bytes; omega_0 / scale_0 are NOT in it): per layer linear.weight,
 * linear.bias, scale_orth.weight, scale_orth.bias, layers front to back, then the head's weight and bias.
 * Served: out_features == 1, hidden_features in {32, 64, 128, 256}, 0 <= hidden_layers <= 8, 1 <= in_features <= 1024;
 * anything else, and a null desc / params / x / y, is INR_E_INVALID before any device work; a null or short workspace is
 * INR_E_WORKSPACE, a pointer off a 16-byte boundary INR_E_ALIGN.  Arithmetic: f32-input MFMA only, 32x32x2 and, in the
 * derivative kernels (inr_wire_derivatives), 16x16x4; plain launches, fixed-order reductions, no float atomics:
 * repeated calls are bit-equal.  Every call only enqueues. */
typedef struct {
    int   in_features, hidden_features, hidden_layers, out_features;
    float first_omega, hidden_omega, first_scale, hidden_scale;
} inr_wire_desc_t;
int64_t inr_wire_param_count(const inr_wire_desc_t* desc);                   /* -1 for a descriptor the kernels do not serve */
/* offsets[4 l + {0, 1, 2, 3}] = linear.weight, linear.bias, scale_orth.weight, scale_orth.bias of layer l <= hidden_layers, then
 * the head's weight and bias: 4 (hidden_layers + 1) + 2 float offsets; max_entries counts them */
int     inr_wire_param_offsets(const inr_wire_desc_t* desc, int64_t* offsets, int max_entries);
/* training: 0 = inr_wire_forward, 1 = inr_wire_loss_grad / inr_wire_fit, 2 = inr_wire_forward_stash + inr_wire_input_grad */
size_t  inr_wire_workspace_bytes(const inr_wire_desc_t* desc, int64_t n, int training);   /* 0 for what is not served */
/* INRmodel.py:109-120, one ComplexGaborLayer2D.forward.  is_first: x [n][in_features] real, real weights [H][in]; otherwise
 * x [n][2H] = planes [re | im], in_features == out_features == H and interleaved complex weights [H][H][2] / biases [H][2].
 * out [n][2H] = planes [re | im].  Workspace: inr_wire_layer_workspace_bytes(n, x's columns, out_features). */
size_t inr_wire_layer_workspace_bytes(int64_t n, int in_columns, int out_features);
int inr_wire_layer_forward(float* out, const float* x, const float* lin_w, const float* lin_b, const float* orth_w,
                           const float* orth_b, int64_t n, int in_features, int out_features, int is_first, float omega, float scale,
                           void* workspace, size_t workspace_bytes, void* stream);
/* wiretest.ipynb cell 2 `forward`: y[n] = Re head(layers(x[n][in_features])); workspace: inr_wire_workspace_bytes(desc, n, 0) */
int inr_wire_forward(const inr_wire_desc_t* desc, const float* params, const float* x, int64_t n, float* y, void* workspace,
                     size_t workspace_bytes, void* stream);
/* wiretest.ipynb cell 10: clamp(INR(input_mapping(get_mgrid(shape), B)), min) -> y[prod(shape)], grid + Fourier features made
 * chunk by chunk in the workspace with the kernel of inr_grid_fourier_map; B == NULL feeds the raw coordinates
 * (in_features == dim).  Arguments as inr_siren_reconstruct; bit-equal with inr_wire_forward on the same rows. */
size_t inr_wire_reconstruct_workspace_bytes(const inr_wire_desc_t* desc, int64_t chunk_rows);
int inr_wire_reconstruct(const inr_wire_desc_t* desc, const float* params, const int64_t* shape, int dim, const float* B, int m,
                         float* y, int use_clamp, float clamp_min, int64_t chunk_rows, void* workspace, size_t workspace_bytes,
                         void* stream);
/* wiretest.ipynb cell 10, `loss = ((model_output - LR_ground_truth)**2).mean(); loss.backward()`: *loss = mean(w (y - t)^2)
 * (weight nullable) and grads = its gradient in the flat layout, torch's convention for complex parameters
 * (grad = dL/dRe + i dL/dIm; the head bias's imaginary part gets exactly 0).  Workspace: inr_wire_workspace_bytes(desc, n, 1). */
int inr_wire_loss_grad(const inr_wire_desc_t* desc, const float* params, float* grads, const float* x, const float* target,
                       const float* weight, int64_t n, float* loss, void* workspace, size_t workspace_bytes, void* stream);
/* wiretest.ipynb cell 10's plain branch, n_steps times: forward, MSE, backward, Adam over the flat buffer (a complex parameter
 * is its two reals, as torch.optim.Adam views it; the arithmetic of inr_adam_step), with no host read.  first_step = the
 * 1-based Adam step of the first iteration; losses[n_steps] (device, nullable) receives each step's loss before its update.
 * One step is bit-equal with inr_wire_loss_grad + inr_adam_step.  Workspace: inr_wire_workspace_bytes(desc, n, 1). */
int inr_wire_fit(const inr_wire_desc_t* desc, float* params, float* grads, float* m, float* v, const float* x,
                 const float* target, const float* weight, int64_t n, int64_t first_step, int n_steps, double lr, double beta1,
                 double beta2, double eps, float* losses, void* workspace, size_t workspace_bytes, void* stream);
/* wiretest.ipynb cell 10's PerturbNet branch, `model_output = INR.forward(perturbed_input); loss.backward()` as far as the
 * network's INPUT (cell 2 leaves its `coords.clone().detach()` commented out, so the gradient flows on through input_mapping into
 * the PerturbNet): inr_wire_forward_stash gives y[n], bit-equal with inr_wire_forward, and leaves the four stashed quantities per
 * (row, unit) in the workspace; inr_wire_input_grad turns a caller-given gy[n] = dL/dy into dx [n][in_features] (unpadded) =
 * dL/dx, through G = gy (w_r, -w_i), the layers' backward epilogues, the input-gradient GEMMs against the transposed images and,
 * for layer 0, one more against the transposed real image [in][2H].  It runs no forward and forms NO parameter gradient (the
 * notebook's next inr_optim.zero_grad() discards them), and it CONSUMES the stash: one inr_wire_input_grad per
 * inr_wire_forward_stash, same desc, params (unchanged in between), n and workspace.  Each row of y and dx depends on its own
 * row of x and gy only, bit for bit, whatever n.  Refusals as above (n < 1 or n > 65535 * 2048 is INR_E_INVALID).
 * Workspace: inr_wire_workspace_bytes(desc, n, 2). */
int inr_wire_forward_stash(const inr_wire_desc_t* desc, const float* params, const float* x, int64_t n, float* y,
                           void* workspace, size_t workspace_bytes, void* stream);
int inr_wire_input_grad(const inr_wire_desc_t* desc, const float* params, const float* gy, int64_t n, float* dx,
                        void* workspace, size_t workspace_bytes, void* stream);
/* Spatial derivatives of a fitted WIRE network (nn_mri.py:205-221 `gradient`, `divergence`, `laplace` applied to the stack of
 * wiretest.ipynb cell 2, which leaves its `detach()` commented out): the reference takes two torch.autograd.grad passes with
 * create_graph=True; these entry points evaluate the same quantities in FORWARD mode, without a stash and without autograd.  Per
 * row and layer they carry the value, one tangent per coordinate axis and a Laplacian accumulator as planes [hr | hi], every plane
 * multiplied by the layer's block image on the f32-input MFMA (v_mfma_f32_16x16x4_f32) and combined in registers.
 *   y[n]               = Re head(layers(features(x)))                  (the raw network value, no clamp)
 *   grad[n][d_tangent] = d y / d x_i, i < d_tangent                    (nullable)
 *   lap[n]             = sum_{i < d_tangent} d^2 y / d x_i^2           (nullable; without it the accumulator is neither computed
 *                                                                       nor carried)
 * Semantics of inr_siren_jet / inr_siren_jet_grid: x[n][d] are the [-1, 1] coordinates of inr_mgrid (multiply a first derivative
 * along axis a by 2 / (shape[a] - 1), a second one by its square, for per-voxel units); B == NULL feeds the coordinates to the
 * network (in_features == d), otherwise features = [sin(2 pi x B^T) | cos(2 pi x B^T)], B[m][d], in_features == 2 m;
 * d_tangent names the LEADING axes to differentiate along (1 <= d_tangent <= d <= 4).  `params` is the flat buffer of
 * inr_wire_param_offsets.  Rows are processed `chunk_rows` at a time in `workspace`, which is counted in FLOATS
 * (inr_wire_derivatives_workspace_floats(desc, d, m, min(chunk_rows, n), want_laplacian), m = 0 without B; sized for d tangents,
 * so it serves every d_tangent): the layers' block images, the input jets and two buffers of planes the layers write in turn.
 * A row's bits depend neither on the chunk size, nor on its place in a chunk, nor on which of grad / lap were asked for, and
 * repeated calls are bit-equal (fixed summation order, no float atomics).  y agrees with inr_wire_forward to rounding, not bit for
 * bit (another tile shape).  Both calls only enqueue.
 * Served: what inr_wire_forward serves, with 1 <= d <= 4; anything else, and a null desc / params / x / shape / y, is
 * INR_E_INVALID with a message before any device work; a null or short workspace is INR_E_WORKSPACE, a params or workspace
 * pointer off a 16-byte boundary INR_E_ALIGN, likewise before any device work. */
int64_t inr_wire_derivatives_workspace_floats(const inr_wire_desc_t* desc, int d, int m, int64_t chunk_rows,
                                              int want_laplacian);   /* 0 for what is not served */
/* on explicit coordinate rows: replaces gradient(y, x) / laplace(y, x) over y = INR(input_mapping(x, B)) */
int inr_wire_derivatives(const inr_wire_desc_t* desc, const float* params, const float* x, int64_t n, int d, int d_tangent,
                         const float* B, int m, float* y, float* grad, float* lap, int64_t chunk_rows, void* workspace,
                         int64_t workspace_floats, void* stream);
/* the same on the dense grid get_mgrid(shape) (dim == d axes), coordinates generated in the kernels as by inr_wire_reconstruct.
 * Bit-equal with inr_wire_derivatives on the rows of inr_mgrid(shape). */
int inr_wire_derivatives_grid(const inr_wire_desc_t* desc, const float* params, const int64_t* shape, int dim, int d_tangent,
                              const float* B, int m, float* y, float* grad, float* lap, int64_t chunk_rows, void* workspace,
                              int64_t workspace_floats, void* stream);

/* ---- measurement hooks (bench.py roofline): per-kernel-class HIP-event timing on the launch stream.
 * class ids: 0 = GEMM forward (sine layer), 1 = GEMM input-grad, 2 = GEMM param-grad, 3 = other */
int  inr_prof_enable(int enable);
int  inr_prof_reset(void);
/* synchronises the recorded events; returns launches and total milliseconds for a class */
int  inr_prof_read(int kernel_class, int64_t* launches, double* total_ms);

/* tuning/debug switches (not for production use): key 0 = force the generic GEMM kernel (0/1); key 1 = fp32 MFMA shape
 * of the pipelined GEMM (1 = 16x16x4, default; 0 = 32x32x2); key 2 = hybrid-fit mapping (1 = eight lanes per voxel,
 * default; 0 = one lane per voxel, kept as an independent cross-check); key 3 = GEMM arithmetic of the whole-network
 * entry points (inr_siren_fit / _loss_grad / _forward / _reconstruct): 1 = split-fp16 MFMA (three fp16 products of
 * hi/lo-split operands per fp32 product, fp32 accumulate; default), 0 = f32-input MFMA, 2 = split-fp16 also in the
 * stand-alone layer calls (needs a >= 32 MiB device scratch buffer via inr_debug_set_ptr(1, ptr)); key 5 = serpentine
 * row-tile order between consecutive GEMMs (1 default, 0 off); key 6 = 128 x 256 tiles for the forward GEMMs (1
 * default, 0 = 128 x 128); key 7 = pre-split (HL32) operand path of the fused entry points (1 default); key 10 = its
 * kernel family (2 = persistent with deferred epilogue, default; 1 = persistent, epilogue in line; 0 = one block per
 * tile); key 11 = start stagger between CUs of the persistent kernels (K-steps x 100, 0 default); key 12 = small-network
 * fit (1 = persistent multi-step kernel, default; 0 = two launches per step); key 13 = its rows per block (0 choose,
 * 32, 64); key 14 = RAMS 32->32 convolutions (2 = split-fp16 MFMA, activations staged in LDS, default; 1 = split-fp16,
 * activations from global memory; 0 = f32-input MFMA; +4 forces the LDS-staged kernels); key 15 = which LDS-staged kernel
 * (42 = two blocks of 4 waves x 2 tiles per CU, one staged image each, default; 8 = 8 waves x 1 tile, two images; 4 = 4 waves
 * x 2 tiles, two images; 16 = two-pass 8 waves x 2 tiles); key 16 = last sine layer of a
 * fit step stashes z only (1 default, 0 = act + omega cos); key 17 = poll limit of the small-network kernel's grid barrier (0 = built-in 2^22;
 * tests force the abandon path with 1); key 18 = 64-row tiles for GEMM launches with too few 128-row tiles to fill the chip
 * (1 default); key 19 = cross-layer fused forward for inr_siren_forward / inr_siren_reconstruct (0 default = one launch per layer; 1 =
 * all layers of a 64-row panel in one launch: correct, measured slower, kept as a study -- DESIGN.md); key 20 = the parameter-gradient GEMMs of a fused step as ONE
 * launch behind the input-gradient chain, its row splits chosen for the whole launch (1 default, applied below 200,000 rows, where
 * it pays; 0 = one launch per layer, in line; the gradients' last bits differ between the two: other row ranges per partial sum;
 * inr_launch_count counts every GEMM of the merged launch); key 21 = fewest rows a block of the fused head step takes (16 default;
 * 4 .. 256, multiples of 4: more, smaller blocks at small row counts); key 22 = block count the merged parameter-gradient launch
 * aims at (256 default = one round over the chip; its row splits are this over the layers' tile count); key 23 = rows per block of
 * the fused head step (0 default = the library's rule, at most 128; set it before the workspace of a fit is sized); key 24 = RAMS
 * kernels: 1 = the fusions that keep every bit (training: the data-gradient convolutions apply the ReLU mask / add the residual
 * gradient in their epilogue; inference: long skip in the trunk-closing convolution's epilogue, padded outputs, the stem by rows),
 * 0 = the separate passes they replaced, 2 (default) = also the inference gate of an attention block computed from its first
 * convolution's output so that the second applies it and adds the residual itself (equal up to the rounding of a mean); key 25 = tall slab reductions (more than 128 partial sums per output) in one
 * launch (1, default) or two (0; the same additions in the same order); key 26 = fewest voxels (batch x image) for which RAMS
 * inference takes the gate-ahead form of key 24 = 2 (600,000 default: four 128 x 128 x 9 stacks); key 27 = 1 sends the K-contiguous
 * GEMMs of 512 output columns to the row-owning kernel (a block owns 128 rows x all 512 columns, epilogue in line; 0 = default: measured
 * slower, bit-identical) when they have at least key-28 (default 1024) row panels; key 29 = most 128 x 256 tiles (per 256 CUs; default 192) of a launch that
 * still takes the 64 x 128 tiles of gemm_hp_nt_kernel; key 30 = 0 keeps the head step a kernel of its own (1, default: from key-31 = 768
 * row panels on it rides in the epilogue of the last sine layer, gemm_hp_row_kernel<HPE_HEAD>); key 32 = test-only cap on the grid of the
 * persistent HL32 kernels (pkd, pkc, row-owning, fused head, fused forward; 0 .. 2^20, 0 default = no cap): small launches then walk several
 * tiles per block; the kernel family chosen and every result bit stay the same;
 * keys 8/9 = time-stamp selection of diagnostic builds.
 * PROCESS-GLOBAL and diagnostic only (see "threading" at the top of this file). */
int inr_debug_set(int key, int value);     /* INR_E_INVALID for an unknown key or a value outside the key's range */
int inr_debug_get(int key, int* value);    /* the value a key currently holds */
int inr_debug_reset(void);                 /* every key (and both inr_debug_set_ptr pointers) back to its default */
int inr_debug_set_ptr(int key, void* ptr);   /* key 0: per-wave time-stamp buffer (only honoured by -DINR_STAMPS builds);
                                                 key 1: device scratch for debug key 3 = 2 */

/* Launch-family counters (process-global, monotonic until reset): how many launches each kernel family has received from
 * the host launchers since the last inr_launch_counts_reset().  Lets a parity test assert WHICH family it covered. */
#define INR_LF_HP_PKD      0   /* gemm_hp_pkd_kernel: HL32 operands, persistent grid, epilogue deferred under the next K-loop */
#define INR_LF_HP_PKC      1   /* gemm_hp_pkc_kernel: HL32 operands, persistent grid, epilogue in line */
#define INR_LF_HP_TILE     2   /* gemm_hp_kernel<KC>: HL32 operands, one block per tile */
#define INR_LF_HP_RC       3   /* gemm_hp_kernel<RC>: HL32 parameter gradient */
#define INR_LF_H3          4   /* gemm_h3_kernel: split-fp16, fp32 operands split by the consumer */
#define INR_LF_F32_PIPE16  5   /* gemm_f32_pipe16_kernel: f32-input MFMA 16x16x4 */
#define INR_LF_F32_PIPE    6   /* gemm_f32_pipe_kernel: f32-input MFMA 32x32x2 */
#define INR_LF_F32_GENERIC 7   /* gemm_f32_kernel: guarded generic kernel */
#define INR_LF_SMALL_MULTI 8   /* siren_small_multi_kernel: persistent cooperative small-network fit */
#define INR_LF_SMALL_STEP  9   /* small-network step kernel + reduce/Adam kernel */
#define INR_LF_HP_NARROW   10  /* gemm_hp_nt_kernel: HL32 operands, 64 x 128 tiles (launches too small for the wide tiles) */
#define INR_LF_HP_FUSED_FWD 11 /* siren_fwd_fused_kernel: every sine layer + the head of a forward in ONE launch, panel in LDS */
#define INR_LF_HP_ROW      12  /* gemm_hp_row_kernel: HL32 operands, persistent, a block owns 128 rows x all 512 columns, epilogue in line */
#define INR_LF_SMALL_BATCH 13  /* siren_small_batch_kernel: several small-network fits in ONE persistent cooperative launch */
#define INR_LF_COUNT       14
int inr_launch_count(int family, int64_t* count);
int inr_launch_counts_reset(void);

/* diagnostic: s[i] = sin(x[i]), c[i] = cos(x[i]) with the device routine used in the epilogues */
int inr_sincos_probe(float* s, float* c, const float* x, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INRHIP_H */
