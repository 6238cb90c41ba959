// What the block-operator TV / Huber units share (tvsr.hip, tvj.hip): the shape and the block kernel of a call with their checks, the
// block sum (A x) and the Huber function.  One definition: the units compute the same bits where their problems coincide.
#pragma once
#include <cmath>

#include "internal.h"

namespace inr {

constexpr int TV_THREADS = 1024;
constexpr int TV_WAVES = TV_THREADS / 64;
constexpr int TV_MAX_FACTOR = INR_TVSR_MAX_FACTOR;
constexpr int TV_MAX_SIDE = INR_TVSR_MAX_SIDE;
constexpr int TV_MAX_GRID = 1 << 16;

// the block kernel, by value in the kernel arguments
struct TvBlock {
    double k[TV_MAX_FACTOR * TV_MAX_FACTOR];   // [f0][f1]
    double k2;                                  // sum k^2
};

struct TvShape {
    int H, W, h, w, f0, f1;
};

__device__ __forceinline__ double tv_huber(double t, double alpha) {
    if (alpha == 0.0) return t;
    return t <= alpha ? t * t / (2.0 * alpha) : t - alpha / 2.0;
}

// (A x) of LR block (bi, bj) of one image: the terms in ascending (a, b)
__device__ __forceinline__ double tv_block_sum(const double* x, const double* ks, const TvShape& s, int bi, int bj) {
    double acc = 0.0;
    for (int a = 0; a < s.f0; ++a) {
        const double* row = x + (size_t)(bi * s.f0 + a) * s.W + bj * s.f1;
        for (int b = 0; b < s.f1; ++b) acc += ks[a * s.f1 + b] * row[b];
    }
    return acc;
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
    double sum = 0.0, k2 = 0.0;
    for (int t = 0; t < TV_MAX_FACTOR * TV_MAX_FACTOR; ++t) kb->k[t] = 0.0;
    for (int t = 0; t < f0 * f1; ++t) {
        INR_REQUIRE(std::isfinite(kernel[t]), INR_E_INVALID, "%s: the block kernel must be finite (entry %d is %g)", who, t, kernel[t]);
        kb->k[t] = kernel[t];
        sum += kernel[t];
        k2 += kernel[t] * kernel[t];
    }
    INR_REQUIRE(std::isfinite(sum) && std::fabs(sum - 1.0) <= 1e-9, INR_E_INVALID, "%s: the block kernel must sum to 1 (got %.17g)", who,
                sum);
    kb->k2 = k2;
    return 0;
}

}  // namespace inr
