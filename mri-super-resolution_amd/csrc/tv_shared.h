// What every TV / Huber solver unit shares (tvsr.hip, tvsr3d.hip, tvmf.hip, tvms.hip, tvop.hip, tvj.hip, tgv.hip): the
// Huber function, the floor division, the capped stride-loop grids, the refusals of the scalar parameters and the gradient weights,
// the step setup of the 3-D prior, the one-field-plan workspace view and the finish kernel that reduces a unit's partials.  One
// definition each: where two units state the same problem they compute the same bits by construction.
#pragma once
#include <cmath>

#include "internal.h"

namespace inr {

constexpr int TV_STRIDE_MAX_GRID = 2048;   // workgroups of a stride-loop launch, at most

// H_alpha(t) for t >= 0: t (alpha = 0), t^2 / (2 alpha) up to alpha and t - alpha / 2 above
__device__ __forceinline__ double tv_huber(double t, double alpha) {
    if (alpha == 0.0) return t;
    return t <= alpha ? t * t / (2.0 * alpha) : t - alpha / 2.0;
}

// floor(u / f) for f > 0
__device__ __host__ __forceinline__ int tv_floordiv(int u, int f) {
    const int q = u / f;
    return u - q * f < 0 ? q - 1 : q;
}

// maximum over a block of 256 threads, every thread receives it (red: 4 doubles of LDS); beside block_sum_f64 of common.h
__device__ __forceinline__ double block_max_f64(double v, double* red /*[4]*/) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return m;
}

// grids: capped, with a stride loop in every kernel; inr_debug_set(32, .) caps them further (tests walk the stride on small problems)
static inline unsigned tv_grid(long long workgroups) {
    long long g = workgroups < 1 ? 1 : (workgroups > TV_STRIDE_MAX_GRID ? TV_STRIDE_MAX_GRID : workgroups);
    const int cap = g_hp_grid_cap;
    if (cap > 0 && g > cap) g = cap;
    return (unsigned)g;
}
static inline unsigned tv_thread_grid(long long threads, int threads_per_block) {
    return tv_grid((threads + threads_per_block - 1) / threads_per_block);
}

// n_iter, lambda and alpha of a solve; max_iter < 0: any n_iter >= 0
static inline int tv_params_check(const char* who, double lam, double alpha, int n_iter, int max_iter) {
    if (max_iter < 0)
        INR_REQUIRE(n_iter >= 0, INR_E_INVALID, "%s: n_iter must be >= 0 (got %d)", who, n_iter);
    else
        INR_REQUIRE(n_iter >= 0 && n_iter <= max_iter, INR_E_INVALID, "%s: n_iter must be 0 .. %d (got %d)", who, max_iter, n_iter);
    INR_REQUIRE(std::isfinite(lam) && lam >= 0.0, INR_E_INVALID, "%s: lambda must be finite and >= 0 (got %g)", who, lam);
    INR_REQUIRE(std::isfinite(alpha) && alpha >= 0.0, INR_E_INVALID, "%s: alpha must be finite and >= 0 (got %g)", who, alpha);
    return 0;
}

// the caller's HOST gradient weights (g0, g1, g2), not null
static inline int tv_grad_weights_check(const char* who, const double* grad_weights) {
    for (int a = 0; a < 3; ++a)
        INR_REQUIRE(std::isfinite(grad_weights[a]) && grad_weights[a] >= 0.0, INR_E_INVALID,
                    "%s: the gradient weights must be finite and >= 0 (g%d is %g)", who, a, grad_weights[a]);
    return 0;
}

// sum g_a^2 of the 3-D prior in the order (1, 2, 0) over the axes whose HR extent exceeds 1; 0: the prior vanishes (lambda = 0)
static inline double tv_grad_weight_sum(const double* g, int D, int H, int W) {
    double gsum = 0.0;
    if (H > 1) gsum += g[1] * g[1];
    if (W > 1) gsum += g[2] * g[2];
    if (D > 1) gsum += g[0] * g[0];
    return gsum;
}

// the workspace of the single-workgroup units: `fields` planes [H][W] of doubles per image.  base == null: `total` only
struct TvStateView {
    double* state;
    size_t total;
};
static inline TvStateView tv_state_view(int n, int fields, int H, int W, void* base) {
    TvStateView v;
    WsCarver c(base, 16);
    v.state = c.take<double>((size_t)(n > 0 ? n : 1) * fields * (size_t)H * (size_t)W);
    v.total = c.bytes();
    return v;
}

// energy / change / valid_fraction [n] (each may be null) from a unit's partials: epart [n][n_epart], chpart [n][n_chpart] (n_chpart = 0:
// change is 0 and chpart is not read) and, where vpart is not null, the counts of valid data vpart [n][n_epart] over `denominator`.
// Thread t adds (maximises) partials t, t + 256, ... in ascending order, then the lanes by wave_sum's butterfly, then the four waves in
// order: the bits depend on the partials alone.  A template on the unit's workgroup size, so that only the units that launch it
// carry it
template <int THREADS>
__global__ void __launch_bounds__(THREADS) tv_finish_kernel(double* energy, double* change, double* valid_fraction, const double* epart,
                                                            long long n_epart, const double* chpart, long long n_chpart,
                                                            const double* vpart, double denominator, long long n) {
    static_assert(THREADS == 256, "block_sum_f64 and block_max_f64 reduce four waves");
    __shared__ double red[THREADS / 64];
    const int tid = threadIdx.x;
    for (long long img = blockIdx.x; img < n; img += gridDim.x) {
        double en = 0.0, ch = 0.0, cnt = 0.0;
        for (long long p = tid; p < n_epart; p += THREADS) {
            en += epart[img * n_epart + p];
            if (vpart) cnt += vpart[img * n_epart + p];
        }
        for (long long p = tid; p < n_chpart; p += THREADS) ch = fmax(ch, chpart[img * n_chpart + p]);
        en = block_sum_f64(en, red);
        if (vpart) cnt = block_sum_f64(cnt, red);   // uniform over the launch
        ch = block_max_f64(ch, red);
        if (tid == 0) {
            if (energy) energy[img] = en;
            if (change) change[img] = ch;
            if (valid_fraction) valid_fraction[img] = cnt / denominator;
        }
    }
}
template <int THREADS>
int tv_finish(double* energy, double* change, double* valid_fraction, const double* epart, long long n_epart, const double* chpart,
              long long n_chpart, const double* vpart, double denominator, long long n, hipStream_t st) {
    if (!energy && !change && !valid_fraction) return 0;
    hipLaunchKernelGGL(tv_finish_kernel<THREADS>, dim3(tv_grid(n)), dim3(THREADS), 0, st, energy, change, valid_fraction, epart, n_epart,
                       chpart, n_chpart, vpart, denominator, n);
    INR_LAUNCH_CHECK();
    return 0;
}

}  // namespace inr
