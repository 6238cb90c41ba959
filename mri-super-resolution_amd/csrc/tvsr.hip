// Model-based super-resolution with an edge-preserving prior, the classical variational comparator of the fitted networks:
//   x* = argmin_x 1/2 sum_i w_i ((A x)_i - y_i)^2 + lambda sum_j H_alpha(|(grad x)_j|)
// A: every LR pixel is the k-weighted sum of its f0 x f1 block of the HR image (k [f0][f1], sum k = 1: the block mean, the
// decimation delta, or the caller's), so A A^T = |k|^2 I and the proximal map of the data term is closed-form per block.  grad: forward
// differences with a zero last row / column; div = -grad^T.  H_0(t) = t (isotropic TV), H_alpha(t) = t^2 / (2 alpha) up to alpha and
// t - alpha / 2 above (Huber).  Chambolle-Pock with tau = sigma = 1/sqrt(8), from x = xbar = x0, p = 0:
//   p    <- (p + sigma grad(xbar)) / (1 + sigma alpha / lambda);  p <- p / max(1, |p| / lambda)       (lambda = 0: p = 0)
//   v    <- x + tau div(p)
//   x'   <- v - A^T(c (A v - y)),  c_i = tau w_i / (1 + tau w_i |k|^2)
//   xbar <- 2 x' - x;  x <- x'
//
// ONE launch solves a batch.  One workgroup of 1,024 threads owns one image and runs every iteration itself; workgroups share nothing,
// so there is no cooperative launch, no grid barrier and no spin, and a batch beyond the CU count is simply queued (the grid is the
// batch, capped, with a stride loop over the images).  The state x | xbar | p0 | p1 of an image is 4 H W doubles of the caller's
// workspace (global memory, L2-resident for the sizes of the driver); there is no LDS path, every size takes this one (the four
// fields of an image would pass the CU's 160 KiB of LDS from 72 x 72 on).  All arithmetic is fp64; the fp32 entry
// converts at load and rounds once at the store.  The unit is compiled with -ffp-contract=off (_build.py), so the fp32 and fp64 entries, whose kernels differ in their loads and
// stores only, compute the same bits between them.
//
// WHERE THE BARRIERS SIT, AND WHY.  An iteration has two phases and a __syncthreads() after each:
//   dual   (thread per HR pixel e):  reads xbar[e], xbar[e + W], xbar[e + 1] -- neighbours' --, reads and writes p0[e], p1[e] -- its own;
//   ---- barrier 1: every p of this iteration is written before any thread differences it
//   primal (thread per LR block):    reads p0 / p1 at the pixels of its block and their upper / left neighbours -- other blocks' --,
//                                    reads and writes x[e] and xbar[e] of ITS block only (xbar[e] holds v between the block's two passes);
//   ---- barrier 2: every xbar of this iteration is written before the next dual phase differences it
// So in each phase a field is either read (possibly across threads) or written by its owner alone, never both by different threads:
// xbar is read-only in the dual phase and owner-written in the primal one, p is owner-written in the dual phase and read-only in the
// primal one, x is touched by its block's thread only.  __syncthreads() is also the workgroup-scope fence that makes the global
// stores of one phase visible to the other threads of the workgroup (one CU, one vector L1) in the next.  The start (x = xbar = x0,
// p = 0) ends with the same barrier, and so does the last iteration, before the objective reads x across threads.
//
// energy: the objective at the returned x (the fp64 x, before the fp32 entry rounds it); every thread adds its LR blocks and then its
// HR pixels in ascending order, wave_sum's butterfly adds the lanes, thread 0 adds the 16 waves in ascending order: no float atomics,
// the same bits on every call and at every position in a batch.  change: max |x' - x| of the last iteration (0 for n_iter = 0).
//
// The start, the primal block step, the data term and the reduction of energy and change are tv_block.h's, shared with tvj.hip and
// tgv.hip; the Huber function, the parameter refusals and the workspace view are tv_shared.h's, shared with the whole family.
#include "tv_block.h"

namespace inr {
namespace {

constexpr int TV_FIELDS = 4;   // x | xbar | p0 | p1 of every image: the workspace is tv_state_view(n, TV_FIELDS, H, W, .)

template <typename T>
__global__ void __launch_bounds__(TV_THREADS) tv_solve_kernel(T* out, double* energy, double* change, const T* y, const T* weight,
                                                              const T* x0, double* state, int n_images, TvShape s, TvBlock kb,
                                                              double lam, double alpha, int n_iter) {
    __shared__ double ks[TV_MAX_FACTOR * TV_MAX_FACTOR];
    __shared__ double red[TV_WAVES];
    const int tid = threadIdx.x;
    const int HW = s.H * s.W, hw = s.h * s.w, W = s.W;
    const double tau = 1.0 / sqrt(8.0), sigma = tau;
    if (tid < s.f0 * s.f1) ks[tid] = kb.k[tid];
    for (int img = blockIdx.x; img < n_images; img += gridDim.x) {
        double* x = state + (size_t)img * TV_FIELDS * HW;
        double* xbar = x + HW;
        double* p0 = xbar + HW;
        double* p1 = p0 + HW;
        const T* yi = y + (size_t)img * hw;
        const T* wi = weight ? weight + (size_t)img * hw : nullptr;
        const T* x0i = x0 ? x0 + (size_t)img * HW : nullptr;
        for (int e = tid; e < HW; e += TV_THREADS) {
            tv_start_pixel(x, xbar, x0i, yi, s, e);
            p0[e] = 0.0;
            p1[e] = 0.0;
        }
        __syncthreads();   // the start is written (and ks, for the first image)
        double ch = 0.0;
        for (int it = 0; it < n_iter; ++it) {
            if (lam > 0.0) {
                const double den = 1.0 + sigma * alpha / lam;
                for (int e = tid; e < HW; e += TV_THREADS) {
                    const int i = e / W, j = e - i * W;
                    const double xb = xbar[e];
                    const double g0 = i + 1 < s.H ? xbar[e + W] - xb : 0.0;
                    const double g1 = j + 1 < W ? xbar[e + 1] - xb : 0.0;
                    double q0 = (p0[e] + sigma * g0) / den;
                    double q1 = (p1[e] + sigma * g1) / den;
                    const double nrm = sqrt(q0 * q0 + q1 * q1) / lam;
                    if (nrm > 1.0) {
                        q0 /= nrm;
                        q1 /= nrm;
                    }
                    p0[e] = q0;
                    p1[e] = q1;
                }
            }
            __syncthreads();   // barrier 1: p is complete
            const bool last = it + 1 == n_iter;
            for (int blk = tid; blk < hw; blk += TV_THREADS)
                tv_primal_block(x, xbar, p0, p1, ks, s, kb.k2, yi, wi, blk, 1.0, tau, last, ch);
            __syncthreads();   // barrier 2: x and xbar are complete
        }
        // the objective at x, and the image
        double en = 0.0;
        for (int blk = tid; blk < hw; blk += TV_THREADS) tv_add_data_term(en, x, ks, s, yi, wi, blk);
        double reg = 0.0;
        for (int e = tid; e < HW; e += TV_THREADS) {
            const int i = e / W, j = e - i * W;
            const double xe = x[e];
            out[(size_t)img * HW + e] = (T)xe;
            if (lam > 0.0) {
                const double g0 = i + 1 < s.H ? x[e + W] - xe : 0.0;
                const double g1 = j + 1 < W ? x[e + 1] - xe : 0.0;
                reg += tv_huber(sqrt(g0 * g0 + g1 * g1), alpha);
            }
        }
        if (lam > 0.0) en += lam * reg;
        tv_store_energy_change(en, ch, red, energy, change, (size_t)img);   // ends with a barrier: red is free for the next image
    }
}

// out [n][h][w] = A in [n][H][W]: one thread per LR pixel
__global__ void __launch_bounds__(256) tv_apply_kernel(double* __restrict__ out, const double* __restrict__ in, long long n_images,
                                                        TvShape s, TvBlock kb) {
    __shared__ double ks[TV_MAX_FACTOR * TV_MAX_FACTOR];
    if ((int)threadIdx.x < s.f0 * s.f1) ks[threadIdx.x] = kb.k[threadIdx.x];
    __syncthreads();
    const long long hw = (long long)s.h * s.w, total = n_images * hw;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const long long img = t / hw;
        const int blk = (int)(t - img * hw), bi = blk / s.w, bj = blk - bi * s.w;
        out[t] = tv_block_sum(in + img * s.H * s.W, ks, s, bi, bj);
    }
}

// out [n][H][W] = A^T in [n][h][w]: one thread per HR pixel
__global__ void __launch_bounds__(256) tv_adjoint_kernel(double* __restrict__ out, const double* __restrict__ in, long long n_images,
                                                          TvShape s, TvBlock kb) {
    __shared__ double ks[TV_MAX_FACTOR * TV_MAX_FACTOR];
    if ((int)threadIdx.x < s.f0 * s.f1) ks[threadIdx.x] = kb.k[threadIdx.x];
    __syncthreads();
    const long long HW = (long long)s.H * s.W, total = n_images * HW;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const long long img = t / HW;
        const int e = (int)(t - img * HW), i = e / s.W, j = e - i * s.W;
        const int bi = i / s.f0, bj = j / s.f1;
        out[t] = ks[(i - bi * s.f0) * s.f1 + (j - bj * s.f1)] * in[img * s.h * s.w + (long long)bi * s.w + bj];
    }
}

template <typename T>
int tv_solve(const char* who, T* out, double* energy, double* change, const T* y, const T* weight, const T* x0, int n_images, int H,
             int W, int f0, int f1, const double* kernel, double lam, double alpha, int n_iter, double* workspace,
             int64_t workspace_doubles, hipStream_t st) {
    INR_REQUIRE(out && y, INR_E_INVALID, "%s: null pointer", who);
    TvShape s;
    TvBlock kb;
    if (int rc = tv_shape_check(who, n_images, H, W, f0, f1, &s)) return rc;
    if (int rc = tv_params_check(who, lam, alpha, n_iter, -1)) return rc;
    if (int rc = tv_block_check(who, kernel, f0, f1, &kb)) return rc;
    if (int rc = check_ws_doubles(who, workspace, workspace_doubles, tv_state_view(n_images, TV_FIELDS, H, W, nullptr).total)) return rc;
    if (n_images == 0) return 0;
    const TvStateView v = tv_state_view(n_images, TV_FIELDS, H, W, workspace);
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL((tv_solve_kernel<T>), dim3((unsigned)(n_images < TV_MAX_GRID ? n_images : TV_MAX_GRID)), dim3(TV_THREADS), 0, st,
                       out, energy, change, y, weight, x0, v.state, n_images, s, kb, lam, alpha, n_iter);
    INR_LAUNCH_CHECK();
    return 0;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_tvsr_workspace_doubles(int n_images, int height, int width) {
    TvShape s;
    if (tv_shape_check("inr_tvsr_workspace_doubles", n_images, height, width, 1, 1, &s)) return 0;
    return (int64_t)(tv_state_view(n_images, TV_FIELDS, height, width, nullptr).total / sizeof(double));
}

int inr_tvsr_solve2d(double* out, double* energy, double* change, const double* y, const double* weight, const double* x0, int n_images,
                     int height, int width, int f0, int f1, const double* kernel, double lambda, double alpha, int n_iter,
                     double* workspace, int64_t workspace_doubles, void* stream) {
    return tv_solve("inr_tvsr_solve2d", out, energy, change, y, weight, x0, n_images, height, width, f0, f1, kernel, lambda, alpha, n_iter,
                    workspace, workspace_doubles, (hipStream_t)stream);
}

int inr_tvsr_solve2d_f32(float* out, double* energy, double* change, const float* y, const float* weight, const float* x0, int n_images,
                         int height, int width, int f0, int f1, const double* kernel, double lambda, double alpha, int n_iter,
                         double* workspace, int64_t workspace_doubles, void* stream) {
    return tv_solve("inr_tvsr_solve2d_f32", out, energy, change, y, weight, x0, n_images, height, width, f0, f1, kernel, lambda, alpha,
                    n_iter, workspace, workspace_doubles, (hipStream_t)stream);
}

int inr_block_apply2d(double* out, const double* in, int n_images, int height, int width, int f0, int f1, const double* kernel,
                      void* stream) {
    INR_REQUIRE(out && in, INR_E_INVALID, "inr_block_apply2d: null pointer");
    TvShape s;
    TvBlock kb;
    if (int rc = tv_shape_check("inr_block_apply2d", n_images, height, width, f0, f1, &s)) return rc;
    if (int rc = tv_block_check("inr_block_apply2d", kernel, f0, f1, &kb)) return rc;
    if (n_images == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL(tv_apply_kernel, dim3(tv_pixel_grid((long long)n_images * s.h * s.w)), dim3(256), 0, st, out, in, (long long)n_images, s,
                       kb);
    INR_LAUNCH_CHECK();
    return 0;
}

int inr_block_adjoint2d(double* out, const double* in, int n_images, int height, int width, int f0, int f1, const double* kernel,
                        void* stream) {
    INR_REQUIRE(out && in, INR_E_INVALID, "inr_block_adjoint2d: null pointer");
    TvShape s;
    TvBlock kb;
    if (int rc = tv_shape_check("inr_block_adjoint2d", n_images, height, width, f0, f1, &s)) return rc;
    if (int rc = tv_block_check("inr_block_adjoint2d", kernel, f0, f1, &kb)) return rc;
    if (n_images == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL(tv_adjoint_kernel, dim3(tv_pixel_grid((long long)n_images * s.H * s.W)), dim3(256), 0, st, out, in, (long long)n_images,
                       s, kb);
    INR_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
