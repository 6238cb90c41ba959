// What the block-operator TV / Huber units share (tvsr.hip, tvj.hip, tgv.hip; the shape and kernel checks also serve tvmf.hip and
// tvadc.hip, whose nonlinear phases are its own, and tvadc.hip reduces with tv_store_energy_change): the shape
// and the block kernel of a call with their checks, the block sum (A x), and the phases that the three single-workgroup kernels have
// in common -- the start, the primal block step, the data term of the objective and the reduction of energy and change.  One
// definition: the units compute the same bits where their problems coincide.  What the whole family shares is in tv_shared.h.
//
// THE PHASE HELPERS HOLD NO BARRIER.  Each handles ONE work item (an HR pixel or an LR block of one image or channel) and touches
// only what that item owns in its phase; the loop over the items and every __syncthreads() of an iteration stay in the kernel that
// owns the loop, next to its ownership argument.  They take one image's or channel's pointers, where H W <= 2^20 fits an int.  The one
// exception is tv_store_energy_change, a reduction like block_sum_f64: it runs after the iterations and holds its own four barriers.
#pragma once
#include "tv_shared.h"

namespace inr {

constexpr int TV_THREADS = 1024;
constexpr int TV_WAVES = TV_THREADS / 64;
constexpr int TV_MAX_FACTOR = INR_TVSR_MAX_FACTOR;
constexpr int TV_MAX_SIDE = INR_TVSR_MAX_SIDE;
constexpr int TV_MAX_GRID = 1 << 16;   // the batch grid of the single-workgroup units (workgroups share nothing: no test-only cap)

// the block kernel, by value in the kernel arguments
struct TvBlock {
    double k[TV_MAX_FACTOR * TV_MAX_FACTOR];   // [f0][f1]
    double k2;                                  // sum k^2
    double c;                                   // (sum |k|) (max |k|): tvmf.hip's bound on |A_k|^2
};

struct TvShape {
    int H, W, h, w, f0, f1;
};

// (A x) of LR block (bi, bj) of one image: the terms in ascending (a, b)
__device__ __forceinline__ double tv_block_sum(const double* x, const double* ks, const TvShape& s, int bi, int bj) {
    double acc = 0.0;
    for (int a = 0; a < s.f0; ++a) {
        const double* row = x + (size_t)(bi * s.f0 + a) * s.W + bj * s.f1;
        for (int b = 0; b < s.f1; ++b) acc += ks[a * s.f1 + b] * row[b];
    }
    return acc;
}

// the start at HR pixel e of one image or channel: x = xbar = x0 (where given), else the block replication of y
template <typename T>
__device__ __forceinline__ void tv_start_pixel(double* x, double* xbar, const T* x0, const T* y, const TvShape& s, int e) {
    const int i = e / s.W, j = e - i * s.W;
    const double v = x0 ? (double)x0[e] : (double)y[(i / s.f0) * s.w + j / s.f1];
    x[e] = v;
    xbar[e] = v;
}

// the primal step of LR block blk of one image or channel with channel weight m: v = x + tau (m div p) into xbar, the weighted block
// residual, then x' = v - k r, xbar = 2 x' - x and x = x' over the block; ch takes max |x' - x| where `last`.  Reads p0 / p1 at the
// pixels of the block and their upper / left neighbours, reads and writes x and xbar of ITS block only
template <typename T>
__device__ __forceinline__ void tv_primal_block(double* x, double* xbar, const double* p0, const double* p1, const double* ks,
                                                const TvShape& s, double k2, const T* y, const T* weight, int blk, double m, double tau,
                                                bool last, double& ch) {
    const int W = s.W, bi = blk / s.w, bj = blk - bi * s.w;
    double acc = 0.0;
    for (int a = 0; a < s.f0; ++a)
        for (int b = 0; b < s.f1; ++b) {
            const int i = bi * s.f0 + a, j = bj * s.f1 + b, e = i * W + j;
            double d = 0.0;
            if (i + 1 < s.H) d += p0[e];
            if (i > 0) d -= p0[e - W];
            if (j + 1 < W) d += p1[e];
            if (j > 0) d -= p1[e - 1];
            const double v = x[e] + tau * (m * d);
            xbar[e] = v;   // v waits here for the second pass: nobody else reads this block of xbar in this phase
            acc += ks[a * s.f1 + b] * v;
        }
    const double wv = weight ? (double)weight[blk] : 1.0;
    // a missing datum (w = 0) takes no part, whatever y holds there
    const double r = wv == 0.0 ? 0.0 : tau * wv / (1.0 + tau * wv * k2) * (acc - (double)y[blk]);
    for (int a = 0; a < s.f0; ++a)
        for (int b = 0; b < s.f1; ++b) {
            const int e = (bi * s.f0 + a) * W + bj * s.f1 + b;
            const double xo = x[e];
            const double xn = xbar[e] - ks[a * s.f1 + b] * r;
            xbar[e] = 2.0 * xn - xo;
            x[e] = xn;
            if (last) ch = fmax(ch, fabs(xn - xo));
        }
}

// the data term of LR block blk of one image or channel, added to en: 1/2 w ((A x) - y)^2, nothing where w = 0
template <typename T>
__device__ __forceinline__ void tv_add_data_term(double& en, const double* x, const double* ks, const TvShape& s, const T* y,
                                                 const T* weight, int blk) {
    const int bi = blk / s.w, bj = blk - bi * s.w;
    const double wv = weight ? (double)weight[blk] : 1.0;
    if (wv != 0.0) {
        const double r = tv_block_sum(x, ks, s, bi, bj) - (double)y[blk];
        en += 0.5 * wv * r * r;
    }
}

// energy[idx] = the sum of en, change[idx] = the maximum of ch over the workgroup of TV_THREADS (each may be null): wave_sum / wave_max
// add the lanes, thread 0 the 16 waves in ascending order.  red: TV_WAVES doubles of LDS, free again at the return
__device__ __forceinline__ void tv_store_energy_change(double en, double ch, double* red, double* energy, double* change, size_t idx) {
    const int tid = threadIdx.x;
    en = wave_sum(en);
    if ((tid & 63) == 0) red[tid >> 6] = en;
    __syncthreads();
    if (tid == 0 && energy) {
        double sum = 0.0;
        for (int k = 0; k < TV_WAVES; ++k) sum += red[k];
        energy[idx] = sum;
    }
    __syncthreads();
    ch = wave_max(ch);
    if ((tid & 63) == 0) red[tid >> 6] = ch;
    __syncthreads();
    if (tid == 0 && change) {
        double m = 0.0;
        for (int k = 0; k < TV_WAVES; ++k) m = fmax(m, red[k]);
        change[idx] = m;
    }
    __syncthreads();
}

// the apply / adjoint launches of tvsr.hip, one thread per pixel: capped at TV_MAX_GRID workgroups, no test-only cap
static inline unsigned tv_pixel_grid(long long pixels) {
    const long long b = (pixels + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > TV_MAX_GRID ? TV_MAX_GRID : b));
}

// the HR sizes and the block factors of one call
static inline int tv_shape_check(const char* who, int n_images, int H, int W, int f0, int f1, TvShape* s) {
    INR_REQUIRE(n_images >= 0, INR_E_INVALID, "%s: bad sizes (n_images = %d)", who, n_images);
    INR_REQUIRE(f0 >= 1 && f0 <= TV_MAX_FACTOR && f1 >= 1 && f1 <= TV_MAX_FACTOR, INR_E_INVALID,
                "%s: block factors are 1 .. %d per axis (got %d x %d)", who, TV_MAX_FACTOR, f0, f1);
    INR_REQUIRE(H >= 1 && W >= 1 && H <= TV_MAX_SIDE && W <= TV_MAX_SIDE, INR_E_INVALID,
                "%s: bad sizes (HR images of 1 .. %d samples per axis, got %d x %d)", who, TV_MAX_SIDE, H, W);
    INR_REQUIRE(H % f0 == 0 && W % f1 == 0, INR_E_INVALID, "%s: the HR image %d x %d is no whole number of %d x %d blocks", who, H, W,
                f0, f1);
    *s = TvShape{H, W, H / f0, W / f1, f0, f1};
    return 0;
}

// the caller's HOST kernel [f0][f1]: finite entries that sum to 1
static inline int tv_block_check(const char* who, const double* kernel, int f0, int f1, TvBlock* kb) {
    INR_REQUIRE(kernel, INR_E_INVALID, "%s: null pointer (kernel)", who);
    double sum = 0.0, k2 = 0.0, l1 = 0.0, top = 0.0;
    for (int t = 0; t < TV_MAX_FACTOR * TV_MAX_FACTOR; ++t) kb->k[t] = 0.0;
    for (int t = 0; t < f0 * f1; ++t) {
        INR_REQUIRE(std::isfinite(kernel[t]), INR_E_INVALID, "%s: the block kernel must be finite (entry %d is %g)", who, t, kernel[t]);
        kb->k[t] = kernel[t];
        sum += kernel[t];
        k2 += kernel[t] * kernel[t];
        l1 += std::fabs(kernel[t]);
        top = std::fmax(top, std::fabs(kernel[t]));
    }
    INR_REQUIRE(std::isfinite(sum) && std::fabs(sum - 1.0) <= 1e-9, INR_E_INVALID, "%s: the block kernel must sum to 1 (got %.17g)", who,
                sum);
    kb->k2 = k2;
    kb->c = l1 * top;
    return 0;
}

}  // namespace inr
