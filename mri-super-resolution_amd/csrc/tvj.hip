// Channel-coupled (vectorial) TV / Huber super-resolution: the model-based reconstruction of tvsr.hip for a GROUP of C
// channels of one anatomy -- the b-values of a DWI slice -- under one prior that takes ONE gradient norm per pixel over all channels,
// so that the channels share their edges and not their noise:
//   E(x) = 1/2 sum_c sum_i w_ci ((A x_c)_i - y_ci)^2 + lambda sum_j H_alpha( sqrt( sum_c mu_c^2 |(grad x_c)_j|^2 ) )     (coupling 1, joint)
//   E(x) = 1/2 sum_c sum_i w_ci ((A x_c)_i - y_ci)^2 + lambda sum_c sum_j H_alpha( mu_c |(grad x_c)_j| )                 (coupling 0, none)
// A, grad, div, H_alpha: tvsr.hip's (tv_block.h).  mu_c in [0, 1] are the channel weights: with K x = (mu_c grad x_c)_c and max mu <= 1,
// |K|^2 <= 8 and tau = sigma = 1/sqrt(8) stay.  Chambolle-Pock from x = xbar = x0, p = 0:
//   q_c  <- (p_c + sigma (mu_c grad(xbar_c))) / (1 + sigma alpha / lambda)
//   n    <- sqrt(sum_c |q_c|^2) / lambda   (the terms |q_c|^2 = q_c0^2 + q_c1^2 added in ascending c; none: per channel)
//   p_c  <- n > 1 ? q_c / n : q_c          (lambda = 0: the dual phase is skipped, p stays 0)
//   v_c  <- x_c + tau (mu_c div(p_c))
//   x'_c <- v_c - A^T(c_c (A v_c - y_c)),  c_ci = tau w_ci / (1 + tau w_ci |k|^2)
//   xbar <- 2 x' - x;  x <- x'
// The expressions keep the order of tvsr.hip with the products by mu_c placed as written: a product by 1.0 is exact, so C = 1 and
// coupling none with mu = 1 give the bits of inr_tvsr_solve2d.
//
// ONE launch solves a batch of groups.  One workgroup of 1,024 threads owns one group and runs every iteration itself; workgroups share
// nothing: no cooperative launch, no grid barrier, no spin, no atomics; the grid is the groups, capped, with a stride loop.  The state
// of a group is x | xbar | p0 | p1, each [C][H][W], 4 C H W doubles of the caller's workspace.  fp64 throughout, compiled with
// -ffp-contract=off (_build.py); the fp32 entry converts at load and rounds once at the store.  Offsets are size_t (C H W reaches 2^24).
//
// WHERE THE BARRIERS SIT, AND WHY.  An iteration has two phases and a __syncthreads() after each:
//   dual   (thread per HR pixel e, a loop over the channels):  reads xbar[c][e], xbar[c][e + W], xbar[c][e + 1] -- neighbours' --; first
//                                    pass writes q_c to p0[c][e], p1[c][e] and adds |q_c|^2, second pass (joint, n > 1) reads and
//                                    rescales the same p0[c][e], p1[c][e]: every p it touches is ITS OWN pixel's, in every channel;
//   ---- barrier 1: every p of this iteration is written before any thread differences it
//   primal (work item per (channel, LR block)):  reads p0[c] / p1[c] at the pixels of its block and their upper / left neighbours --
//                                    other items' --, reads and writes x[c][e] and xbar[c][e] of ITS block of ITS channel only
//                                    (xbar holds v between the item's two passes);
//   ---- barrier 2: every xbar of this iteration is written before the next dual phase differences it
// The ownership rule of tvsr.hip holds with (channel, pixel) in place of the pixel: in each phase a field is either read (possibly
// across threads) or written by its owner alone.  The coupling adds no exchange between threads: the sum over c runs inside the thread
// that owns the pixel in all channels.  The start and the last iteration end with the same barrier.
//
// energy: E at the returned fp64 x; every thread adds its data terms in ascending (channel, block), then its pixels in ascending order
// (joint: one term per pixel, the sum over c in ascending c; none: the channels of a pixel in ascending c), wave_sum, thread 0 over the
// 16 waves: for C = 1 tvsr.hip's order.  change: max |x' - x| of the last iteration over all channels.
//
// The start, the primal block step, the data term and the reduction of energy and change are tv_block.h's, the ones tvsr.hip runs:
// each works on ONE channel's pointers with int indices (H W <= 2^20); the offsets between channels and groups stay size_t here.
#include "tv_block.h"

namespace inr {
namespace {

constexpr int TVJ_MAX_CHANNELS = INR_TVJ_MAX_CHANNELS;

// the channel weights, by value in the kernel arguments
struct TvjWeights {
    double mu[TVJ_MAX_CHANNELS];
};

template <typename T>
__global__ void __launch_bounds__(TV_THREADS) tvj_solve_kernel(T* out, double* energy, double* change, const T* y, const T* weight,
                                                               const T* x0, double* state, int n_groups, int C, TvShape s, TvBlock kb,
                                                               TvjWeights cw, double lam, double alpha, int joint, int n_iter) {
    __shared__ double ks[TV_MAX_FACTOR * TV_MAX_FACTOR];
    __shared__ double mu[TVJ_MAX_CHANNELS];
    __shared__ double red[TV_WAVES];
    const int tid = threadIdx.x;
    const size_t HW = (size_t)s.H * s.W, hw = (size_t)s.h * s.w, W = (size_t)s.W;
    const size_t CHW = (size_t)C * HW, Chw = (size_t)C * hw;
    const double tau = 1.0 / sqrt(8.0), sigma = tau;
    if (tid < s.f0 * s.f1) ks[tid] = kb.k[tid];
    if (tid < C) mu[tid] = cw.mu[tid];
    for (size_t g = blockIdx.x; g < (size_t)n_groups; g += gridDim.x) {
        double* x = state + g * 4 * CHW;   // [C][H][W] each
        double* xbar = x + CHW;
        double* p0 = xbar + CHW;
        double* p1 = p0 + CHW;
        const T* yg = y + g * Chw;
        const T* wg = weight ? weight + g * Chw : nullptr;
        for (size_t t = tid; t < CHW; t += TV_THREADS) {
            const size_t c = t / HW, e = t - c * HW;
            tv_start_pixel(x + c * HW, xbar + c * HW, x0 ? x0 + g * CHW + c * HW : nullptr, yg + c * hw, s, (int)e);
            p0[t] = 0.0;
            p1[t] = 0.0;
        }
        __syncthreads();   // the start is written (and ks, mu, for the first group)
        double ch = 0.0;
        for (int it = 0; it < n_iter; ++it) {
            if (lam > 0.0) {
                const double den = 1.0 + sigma * alpha / lam;
                for (size_t e = tid; e < HW; e += TV_THREADS) {
                    const size_t i = e / W, j = e - i * W;
                    const bool down = i + 1 < (size_t)s.H, right = j + 1 < W;
                    double ss = 0.0;
                    for (int c = 0; c < C; ++c) {
                        const size_t t = c * HW + e;
                        const double xb = xbar[t];
                        const double g0 = down ? xbar[t + W] - xb : 0.0;
                        const double g1 = right ? xbar[t + 1] - xb : 0.0;
                        double q0 = (p0[t] + sigma * (mu[c] * g0)) / den;
                        double q1 = (p1[t] + sigma * (mu[c] * g1)) / den;
                        if (joint) {
                            ss += q0 * q0 + q1 * q1;
                        } else {
                            const double nrm = sqrt(q0 * q0 + q1 * q1) / lam;
                            if (nrm > 1.0) {
                                q0 /= nrm;
                                q1 /= nrm;
                            }
                        }
                        p0[t] = q0;
                        p1[t] = q1;
                    }
                    if (joint) {
                        const double nrm = sqrt(ss) / lam;
                        if (nrm > 1.0)
                            for (int c = 0; c < C; ++c) {   // the pixel's own q, written just above by this thread
                                const size_t t = c * HW + e;
                                p0[t] = p0[t] / nrm;
                                p1[t] = p1[t] / nrm;
                            }
                    }
                }
            }
            __syncthreads();   // barrier 1: p is complete
            const bool last = it + 1 == n_iter;
            for (size_t item = tid; item < Chw; item += TV_THREADS) {
                const size_t c = item / hw, blk = item - c * hw;
                tv_primal_block(x + c * HW, xbar + c * HW, p0 + c * HW, p1 + c * HW, ks, s, kb.k2, yg + c * hw,
                                wg ? wg + c * hw : nullptr, (int)blk, mu[c], tau, last, ch);
            }
            __syncthreads();   // barrier 2: x and xbar are complete
        }
        // the objective at x, and the images
        double en = 0.0;
        for (size_t item = tid; item < Chw; item += TV_THREADS) {
            const size_t c = item / hw, blk = item - c * hw;
            tv_add_data_term(en, x + c * HW, ks, s, yg + c * hw, wg ? wg + c * hw : nullptr, (int)blk);
        }
        double reg = 0.0;
        for (size_t e = tid; e < HW; e += TV_THREADS) {
            const size_t i = e / W, j = e - i * W;
            const bool down = i + 1 < (size_t)s.H, right = j + 1 < W;
            double ss = 0.0;
            for (int c = 0; c < C; ++c) {
                const size_t t = c * HW + e;
                const double xe = x[t];
                out[g * CHW + t] = (T)xe;
                if (lam > 0.0) {
                    const double g0 = mu[c] * (down ? x[t + W] - xe : 0.0);
                    const double g1 = mu[c] * (right ? x[t + 1] - xe : 0.0);
                    if (joint)
                        ss += g0 * g0 + g1 * g1;
                    else
                        reg += tv_huber(sqrt(g0 * g0 + g1 * g1), alpha);
                }
            }
            if (lam > 0.0 && joint) reg += tv_huber(sqrt(ss), alpha);
        }
        if (lam > 0.0) en += lam * reg;
        tv_store_energy_change(en, ch, red, energy, change, g);   // ends with a barrier: red is free for the next group
    }
}

// the group count and the channel count of one call
int tvj_group_check(const char* who, int n_groups, int channels) {
    INR_REQUIRE(n_groups >= 0, INR_E_INVALID, "%s: bad sizes (n_groups = %d)", who, n_groups);
    INR_REQUIRE(channels >= 1 && channels <= TVJ_MAX_CHANNELS, INR_E_INVALID, "%s: channels are 1 .. %d per group (got %d)", who,
                TVJ_MAX_CHANNELS, channels);
    return 0;
}

// the workspace: the state x | xbar | p0 | p1, each [C][H][W], of every group.  base == null: `total` only
TvStateView tvj_view(int n_groups, int C, int H, int W, void* base) { return tv_state_view(n_groups, 4 * C, H, W, base); }

template <typename T>
int tvj_solve(const char* who, T* out, double* energy, double* change, const T* y, const T* weight, const T* x0, int n_groups, int C,
              int H, int W, int f0, int f1, const double* kernel, const double* channel_weights, double lam, double alpha, int coupling,
              int n_iter, double* workspace, int64_t workspace_doubles, hipStream_t st) {
    INR_REQUIRE(out && y, INR_E_INVALID, "%s: null pointer", who);
    TvShape s;
    TvBlock kb;
    TvjWeights cw;
    if (int rc = tvj_group_check(who, n_groups, C)) return rc;
    if (int rc = tv_shape_check(who, n_groups, H, W, f0, f1, &s)) return rc;
    if (int rc = tv_params_check(who, lam, alpha, n_iter, -1)) return rc;
    INR_REQUIRE(coupling == 0 || coupling == 1, INR_E_INVALID, "%s: coupling is 0 (none) or 1 (joint) (got %d)", who, coupling);
    if (int rc = tv_block_check(who, kernel, f0, f1, &kb)) return rc;
    for (int c = 0; c < TVJ_MAX_CHANNELS; ++c) {
        const double m = c < C && channel_weights ? channel_weights[c] : 1.0;
        // larger weights would break |K|^2 <= 8, the step bound: the caller rescales lambda and alpha instead
        INR_REQUIRE(std::isfinite(m) && m >= 0.0 && m <= 1.0, INR_E_INVALID,
                    "%s: channel_weights must be finite and within [0, 1] (entry %d is %g)", who, c, m);
        cw.mu[c] = m;
    }
    if (int rc = check_ws_doubles(who, workspace, workspace_doubles, tvj_view(n_groups, C, H, W, nullptr).total)) return rc;
    if (n_groups == 0) return 0;
    const TvStateView v = tvj_view(n_groups, C, H, W, workspace);
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL((tvj_solve_kernel<T>), dim3((unsigned)(n_groups < TV_MAX_GRID ? n_groups : TV_MAX_GRID)), dim3(TV_THREADS), 0, st,
                       out, energy, change, y, weight, x0, v.state, n_groups, C, s, kb, cw, lam, alpha, coupling, n_iter);
    INR_LAUNCH_CHECK();
    return 0;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_tvj_workspace_doubles(int n_groups, int channels, int height, int width) {
    TvShape s;
    if (tvj_group_check("inr_tvj_workspace_doubles", n_groups, channels)) return 0;
    if (tv_shape_check("inr_tvj_workspace_doubles", n_groups, height, width, 1, 1, &s)) return 0;
    return (int64_t)(tvj_view(n_groups, channels, height, width, nullptr).total / sizeof(double));
}

int inr_tvj_solve2d(double* out, double* energy, double* change, const double* y, const double* weight, const double* x0, int n_groups,
                    int channels, int height, int width, int f0, int f1, const double* kernel, const double* channel_weights,
                    double lambda, double alpha, int coupling, int n_iter, double* workspace, int64_t workspace_doubles, void* stream) {
    return tvj_solve("inr_tvj_solve2d", out, energy, change, y, weight, x0, n_groups, channels, height, width, f0, f1, kernel,
                     channel_weights, lambda, alpha, coupling, n_iter, workspace, workspace_doubles, (hipStream_t)stream);
}

int inr_tvj_solve2d_f32(float* out, double* energy, double* change, const float* y, const float* weight, const float* x0, int n_groups,
                        int channels, int height, int width, int f0, int f1, const double* kernel, const double* channel_weights,
                        double lambda, double alpha, int coupling, int n_iter, double* workspace, int64_t workspace_doubles,
                        void* stream) {
    return tvj_solve("inr_tvj_solve2d_f32", out, energy, change, y, weight, x0, n_groups, channels, height, width, f0, f1, kernel,
                     channel_weights, lambda, alpha, coupling, n_iter, workspace, workspace_doubles, (hipStream_t)stream);
}

}  // extern "C"
