// The voxel-footprint forward model of a SIREN fit: a datum is a weighted average of the network over K sub-sample positions,
//   p_i = sum_k fw[k] y[i K + k],   y = INR(features(x_i + delta_k)),   loss = inv_count sum_i wt_i (p_i - t_i)^2,
// instead of a point sample.  Sub-sample k of datum i is row i K + k everywhere (sub-sample minor).
//
// Three element-wise kernels -- the expansion of the coordinates, the reduction (inference, diagnostics) and the loss with its
// gradient dL/dy -- and the fit: per step the training forward on the n K rows (inr_siren_forward_train), the loss kernel, the
// backward pass from that dL/dy (inr_siren_backward_train) and launch_adam.  The GEMM kernels are those calls', untouched.
// p_i is ONE fma chain over ascending k from 0 in all kernels (fp_reduce_row), so the reduction and the loss see the same bits;
// the loss is summed from per-block partials of a fixed grid and launch_finish_sum: no float atomics, calls are bit-equal.
#include "internal.h"

namespace inr {
namespace {

constexpr int FOOTPRINT_MAX_K = INR_FOOTPRINT_MAX_SAMPLES;
constexpr int FOOTPRINT_MAX_D = 4;

__global__ void __launch_bounds__(256) fp_expand_kernel(float* __restrict__ out, const float* __restrict__ x,
                                                        const float* __restrict__ offsets, int64_t n, int d, int K) {
    const int64_t total = n * K * d;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t row = e / d;
        const int a = (int)(e - row * d);
        const int64_t i = row / K;
        const int k = (int)(row - i * K);
        out[e] = x[i * d + a] + offsets[k * d + a];
    }
}

// p_i: the chain every kernel of this unit uses
__device__ __forceinline__ float fp_reduce_row(const float* __restrict__ y, const float* __restrict__ fw, int64_t i, int K) {
    const float* yr = y + i * K;
    float p = 0.f;
    for (int k = 0; k < K; ++k) p = fmaf(fw[k], yr[k], p);
    return p;
}

__global__ void __launch_bounds__(256) fp_reduce_kernel(float* __restrict__ pred, const float* __restrict__ y,
                                                        const float* __restrict__ fw, int64_t n, int K) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) pred[i] = fp_reduce_row(y, fw, i, K);
}

// residual of the averaged prediction, dL/dy of every sub-sample, per-block loss partials (the footprint form of mse_kernel)
__global__ void __launch_bounds__(256) fp_loss_kernel(float* __restrict__ gy, float* __restrict__ partial, float* __restrict__ pred,
                                                      const float* __restrict__ y, const float* __restrict__ t,
                                                      const float* __restrict__ wt, const float* __restrict__ fw, int64_t n, int K,
                                                      float inv_count) {
    __shared__ float red[4];
    float acc = 0.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float p = fp_reduce_row(y, fw, i, K);
        if (pred) pred[i] = p;
        const float r = p - t[i];
        const float wr = wt ? wt[i] * r : r;
        const float g = 2.0f * wr * inv_count;
        float* gr = gy + i * K;
        for (int k = 0; k < K; ++k) gr[k] = fw[k] * g;
        acc = fmaf(wr, r, acc);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

unsigned fp_grid(int64_t work) {
    const int64_t b = (work + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

// the rows of one call: n data of K sub-samples each
int fp_rows_check(const char* who, int64_t n, int K) {
    INR_REQUIRE(n >= 1 && n <= MAX_ROWS, INR_E_INVALID, "%s: bad datum count %lld", who, (long long)n);
    INR_REQUIRE(K >= 1 && K <= FOOTPRINT_MAX_K, INR_E_INVALID, "%s: a footprint has 1 .. %d sub-samples (got %d)", who, FOOTPRINT_MAX_K, K);
    INR_REQUIRE(n * K <= MAX_ROWS, INR_E_INVALID, "%s: too many rows (%lld data x %d sub-samples)", who, (long long)n, K);
    return 0;
}

int fp_workspace_check(const char* who, const void* workspace, int64_t workspace_floats, size_t need_bytes) {
    INR_REQUIRE(workspace && workspace_floats >= 0 && (size_t)workspace_floats * sizeof(float) >= need_bytes, INR_E_WORKSPACE,
                "%s: workspace too small (%lld floats, %zu needed)", who, workspace ? (long long)workspace_floats : 0ll,
                need_bytes / sizeof(float));
    INR_REQUIRE(aligned16(workspace), INR_E_ALIGN, "%s: workspace must be 16-byte aligned", who);
    return 0;
}

// the partials of the loss kernel's grid (mse_kernel's, by datum).  base == null: `total` only
struct LossView { float* partial; int blocks; size_t total; };
LossView loss_view(int64_t n, void* base) {
    LossView v;
    WsCarver c(base, 16);
    v.blocks = mse_blocks(n);
    v.partial = c.take<float>((size_t)v.blocks);
    v.total = c.bytes();
    return v;
}

// validated by the caller
int launch_fp_loss(float* gy, float* loss, float* pred, const float* y, const float* t, const float* wt, const float* fw, int64_t n,
                   int K, int64_t count_total, const LossView& v, hipStream_t st) {
    const float inv = (float)(1.0 / (double)(count_total > 0 ? count_total : n));
    {
        ProfScope ps(KC_OTHER, st);
        hipLaunchKernelGGL(fp_loss_kernel, dim3(v.blocks), dim3(256), 0, st, gy, v.partial, pred, y, t, wt, fw, n, K, inv);
        INR_LAUNCH_CHECK();
    }
    return launch_finish_sum(loss, v.partial, v.blocks, inv, st);
}

// the fit's workspace: the fit workspace of the n K rows | y | gy | loss partials and the word an unwanted loss goes to
struct FitFootprintView {
    void* fit;
    size_t fit_bytes;
    float *y, *gy, *loss_sink;
    LossView loss;
    size_t total;
};
FitFootprintView fit_footprint_view(const inr_siren_desc_t* desc, int64_t n, int K, void* base) {
    FitFootprintView v;
    const int64_t rows = n * K;
    WsCarver c(base, 16);
    v.fit_bytes = inr_siren_fit_workspace_bytes(desc, rows);
    v.fit = c.take<char>(v.fit_bytes);
    v.y = c.take<float>((size_t)rows);
    v.gy = c.take<float>((size_t)rows);
    const size_t at = c.bytes();
    v.loss = loss_view(n, base ? static_cast<char*>(base) + at : nullptr);
    c.take<char>(v.loss.total);
    v.loss_sink = c.take<float>(1);
    v.total = c.bytes();
    return v;
}

bool fit_footprint_served(const inr_siren_desc_t* desc, int64_t n, int K) {
    return n >= 1 && n <= MAX_ROWS && K >= 1 && K <= FOOTPRINT_MAX_K && n * K <= MAX_ROWS && inr_siren_hp_eligible(desc) != 0;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int inr_footprint_expand(float* out, const float* x, const float* offsets, int64_t n, int d, int K, void* stream) {
    INR_REQUIRE(out && x && offsets, INR_E_INVALID, "inr_footprint_expand: null pointer");
    INR_REQUIRE(d >= 1 && d <= FOOTPRINT_MAX_D, INR_E_INVALID, "inr_footprint_expand: 1 .. %d coordinates per row (got %d)",
                FOOTPRINT_MAX_D, d);
    if (int rc = fp_rows_check("inr_footprint_expand", n, K)) return rc;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL(fp_expand_kernel, dim3(fp_grid(n * K * d)), dim3(256), 0, st, out, x, offsets, n, d, K);
    INR_LAUNCH_CHECK();
    return 0;
}

int inr_footprint_reduce(float* pred, const float* y, const float* fw, int64_t n, int K, void* stream) {
    INR_REQUIRE(pred && y && fw, INR_E_INVALID, "inr_footprint_reduce: null pointer");
    if (int rc = fp_rows_check("inr_footprint_reduce", n, K)) return rc;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL(fp_reduce_kernel, dim3(fp_grid(n)), dim3(256), 0, st, pred, y, fw, n, K);
    INR_LAUNCH_CHECK();
    return 0;
}

int64_t inr_footprint_loss_workspace_floats(int64_t n) {
    if (n < 1 || n > MAX_ROWS) return 0;
    return (int64_t)(loss_view(n, nullptr).total / sizeof(float));
}

int inr_footprint_loss_grad(float* gy, float* loss, float* pred, const float* y, const float* t, const float* wt, const float* fw,
                            int64_t n, int K, int64_t count_total, void* workspace, int64_t workspace_floats, void* stream) {
    INR_REQUIRE(gy && loss && y && t && fw, INR_E_INVALID, "inr_footprint_loss_grad: null pointer");
    if (int rc = fp_rows_check("inr_footprint_loss_grad", n, K)) return rc;
    INR_REQUIRE(count_total == 0 || count_total >= n, INR_E_INVALID, "inr_footprint_loss_grad: count_total must be 0 or >= n");
    if (int rc = fp_workspace_check("inr_footprint_loss_grad", workspace, workspace_floats, loss_view(n, nullptr).total)) return rc;
    return launch_fp_loss(gy, loss, pred, y, t, wt, fw, n, K, count_total, loss_view(n, workspace), (hipStream_t)stream);
}

int64_t inr_siren_fit_footprint_workspace_floats(const inr_siren_desc_t* desc, int64_t n, int K) {
    if (!desc || !fit_footprint_served(desc, n, K)) return 0;
    return (int64_t)(fit_footprint_view(desc, n, K, nullptr).total / sizeof(float));
}

int inr_siren_fit_footprint(const inr_siren_desc_t* desc, float* params, float* grads, float* m, float* v, const float* x_sub,
                            const float* target, const float* weight, const float* fw, int64_t n, int K, int64_t first_step,
                            int n_steps, double lr, double beta1, double beta2, double eps, float* losses, void* workspace,
                            int64_t workspace_floats, void* stream) {
    INR_REQUIRE(desc && params && grads && m && v && x_sub && target && fw, INR_E_INVALID, "inr_siren_fit_footprint: null pointer");
    const int64_t count = inr_siren_param_count(desc);
    if (count < 0) return INR_E_INVALID;      // (the message is inr_siren_param_count's)
    if (int rc = fp_rows_check("inr_siren_fit_footprint", n, K)) return rc;
    INR_REQUIRE(first_step >= 1 && n_steps >= 0, INR_E_INVALID, "inr_siren_fit_footprint: first_step >= 1, n_steps >= 0");
    INR_REQUIRE(inr_siren_hp_eligible(desc) != 0, INR_E_INVALID,
                "inr_siren_fit_footprint: network shape not served (ask inr_siren_hp_eligible: sine layers a multiple of 32 wide, "
                "hidden 128 / 256 / 512 / 1024, one output)");
    if (int rc = fp_workspace_check("inr_siren_fit_footprint", workspace, workspace_floats,
                                    fit_footprint_view(desc, n, K, nullptr).total))
        return rc;
    INR_REQUIRE(aligned16(params) && aligned16(grads) && aligned16(x_sub), INR_E_ALIGN,
                "inr_siren_fit_footprint: params/grads/x_sub must be 16-byte aligned");
    const FitFootprintView fv = fit_footprint_view(desc, n, K, workspace);
    const int64_t rows = n * K;
    hipStream_t st = (hipStream_t)stream;
    for (int it = 0; it < n_steps; ++it) {
        // the first step of a call always re-images x_sub: what a previous call left in the workspace is never trusted
        if (int rc = inr_siren_forward_train(desc, params, x_sub, fv.y, rows, fv.fit, fv.fit_bytes, it > 0 ? INR_REUSE_INPUT_IMAGE : 0,
                                             stream))
            return rc;
        if (int rc = launch_fp_loss(fv.gy, losses ? losses + it : fv.loss_sink, nullptr, fv.y, target, weight, fw, n, K, 0, fv.loss, st))
            return rc;
        if (int rc = inr_siren_backward_train(desc, params, grads, fv.gy, rows, fv.fit, fv.fit_bytes, stream)) return rc;
        if (int rc = launch_adam(params, grads, m, v, count, first_step + it, lr, beta1, beta2, eps, st)) return rc;
    }
    return 0;
}

}  // extern "C"
