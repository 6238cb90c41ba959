// scipy's cubic B-spline interpolation, the parts that rescale.hip (ndi.zoom) and register.hip (ndi.shift) both run: the prefilter of
// ni_splines.c on the lines of a double plane, the four B-spline weights and the separable four-by-four tap sum.  One definition;
// kernels are templates, so each unit that launches one instantiates its own.
#pragma once
#include <math.h>

#include "common.h"

namespace inr {

// how a line starts and ends: scipy's 'mirror' (whole-sample symmetric; what 'constant' and 'nearest' filter with as well) or
// 'reflect' (half-sample symmetric)
constexpr int SPLINE_MIRROR = 0, SPLINE_REFLECT = 1;

// d c b a | a b c d | d c b a: reflection about the half sample beyond the edge, period 2n, any number of periods
__device__ __forceinline__ int reflect_index(int i, int n) {
    const int period = 2 * n;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - 1 - i;
}

// the prefilter of one line of n >= 2 samples `stride` apart, in place (scipy ni_splines.c: gain, _init_causal_mirror, the causal
// recursion, _init_anticausal_mirror, the anticausal recursion)
__device__ __forceinline__ void rs_prefilter_line(double* c, long long stride, int n) {
    const double z = -0.26794919243112270647;   // sqrt(3) - 2
    const double gain = (1.0 - z) * (1.0 - 1.0 / z);
    for (int i = 0; i < n; ++i) c[i * stride] *= gain;
    const double zn = pow(z, (double)(n - 1));
    double c0 = c[0] + zn * c[(n - 1) * stride], zi = z;
    for (int i = 1; i < n - 1; ++i) {
        c0 += zi * (c[i * stride] + zn * c[(n - 1 - i) * stride]);
        zi *= z;
    }
    c[0] = c0 / (1.0 - zn * zn);
    for (int i = 1; i < n; ++i) c[i * stride] += z * c[(i - 1) * stride];
    c[(n - 1) * stride] = (z * c[(n - 2) * stride] + c[(n - 1) * stride]) * (z / (z * z - 1.0));
    for (int i = n - 2; i >= 0; --i) c[i * stride] = z * (c[(i + 1) * stride] - c[i * stride]);
}

// the same with _init_causal_reflect / _init_anticausal_reflect.  scipy accumulates the start in c[0] itself, so the last term of
// its sum (i = n - 1, which reads c[n - 1 - i]) takes the running sum and not the sample: kept, it is what scipy returns
__device__ __forceinline__ void rs_prefilter_line_reflect(double* c, long long stride, int n) {
    const double z = -0.26794919243112270647;
    const double gain = (1.0 - z) * (1.0 - 1.0 / z);
    for (int i = 0; i < n; ++i) c[i * stride] *= gain;
    const double zn = pow(z, (double)n);
    const double first = c[0];
    double acc = first + zn * c[(n - 1) * stride], zi = z;
    for (int i = 1; i < n; ++i) {
        acc += zi * (c[i * stride] + zn * (i == n - 1 ? acc : c[(n - 1 - i) * stride]));
        zi *= z;
    }
    acc *= z / (1.0 - zn * zn);
    c[0] = acc + first;
    for (int i = 1; i < n; ++i) c[i * stride] += z * c[(i - 1) * stride];
    c[(n - 1) * stride] *= z / (z - 1.0);
    for (int i = n - 2; i >= 0; --i) c[i * stride] = z * (c[(i + 1) * stride] - c[i * stride]);
}

template <int START>
__device__ __forceinline__ void spline_prefilter_line(double* c, long long stride, int n) {
    if (START == SPLINE_REFLECT)
        rs_prefilter_line_reflect(c, stride, n);
    else
        rs_prefilter_line(c, stride, n);
}

// axis 0: one thread per column, neighbouring lanes on neighbouring doubles of every row
template <int START>
__global__ void __launch_bounds__(256) rs_prefilter_cols_kernel(double* __restrict__ c, long long columns, int PH, int PW) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < columns; idx += (long long)gridDim.x * 256)
        spline_prefilter_line<START>(c + (idx / PW) * ((long long)PH * PW) + idx % PW, PW, PH);
}

// axis 1: the lines are contiguous, so a block stages `rows` of them in LDS (coalesced both ways) at an odd pitch in doubles, and
// one lane per staged row runs the recursion there: lanes a row apart sit an odd number of 8-byte words apart, on distinct banks
constexpr int RS_ROW_THREADS = 64, RS_ROWS_MAX = 16, RS_LDS_BYTES = 65536;
template <int START>
__global__ void __launch_bounds__(RS_ROW_THREADS) rs_prefilter_rows_kernel(double* __restrict__ c, long long lines, int PW, int rows,
                                                                           int pitch) {
    extern __shared__ double stage[];   // [rows][pitch]
    for (long long first = (long long)blockIdx.x * rows; first < lines; first += (long long)gridDim.x * rows) {
        const int have = (int)(lines - first < rows ? lines - first : rows);
        double* g = c + first * PW;
        for (int i = threadIdx.x; i < have * PW; i += RS_ROW_THREADS) stage[(i / PW) * pitch + i % PW] = g[i];
        __syncthreads();
        if ((int)threadIdx.x < have) spline_prefilter_line<START>(stage + threadIdx.x * pitch, 1, PW);
        __syncthreads();
        for (int i = threadIdx.x; i < have * PW; i += RS_ROW_THREADS) g[i] = stage[(i / PW) * pitch + i % PW];
        __syncthreads();
    }
}

inline unsigned rs_blocks(long long work) {
    const long long b = (work + 255) / 256;
    return (unsigned)(b > 65536 ? 65536 : b);
}

// both prefilter passes over the [nimg][PH][PW] plane c, axis 0 first; scipy leaves lines of one sample alone
template <int START>
int launch_spline_prefilter(double* c, int nimg, int PH, int PW, hipStream_t st) {
    if (PH > 1) {
        hipLaunchKernelGGL(rs_prefilter_cols_kernel<START>, dim3(rs_blocks((long long)nimg * PW)), dim3(256), 0, st, c,
                           (long long)nimg * PW, PH, PW);
        INR_LAUNCH_CHECK();
    }
    if (PW > 1) {
        const int pitch = PW | 1;
        int rows = RS_LDS_BYTES / (pitch * (int)sizeof(double));
        rows = rows > RS_ROWS_MAX ? RS_ROWS_MAX : rows;
        const long long lines = (long long)nimg * PH;
        const long long blocks = (lines + rows - 1) / rows;
        hipLaunchKernelGGL(rs_prefilter_rows_kernel<START>, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(RS_ROW_THREADS),
                           (size_t)rows * pitch * sizeof(double), st, c, lines, PW, rows, pitch);
        INR_LAUNCH_CHECK();
    }
    return 0;
}

// the cubic B-spline weights of the taps floor(x) - 1 .. floor(x) + 2 at t = x - floor(x)
__device__ __forceinline__ void bspline3_weights(double t, double* w) {
    const double u = 1.0 - t;
    w[0] = u * u * u / 6.0;
    w[1] = (4.0 - 6.0 * t * t + 3.0 * t * t * t) / 6.0;
    w[2] = (1.0 + 3.0 * t + 3.0 * t * t - 3.0 * t * t * t) / 6.0;
    w[3] = t * t * t / 6.0;
}

// sum_kx wx[kx] sum_ky wy[ky] img[iy[ky]][ix[kx]]: the separable tap sum, axis 0 innermost
template <int TAPS>
__device__ __forceinline__ double spline_tap_sum(const double* __restrict__ img, int PW, const int* iy, const int* ix, const double* wy,
                                                 const double* wx) {
    double v = 0.0;
#pragma unroll
    for (int kx = 0; kx < TAPS; ++kx) {
        double col = 0.0;
#pragma unroll
        for (int ky = 0; ky < TAPS; ++ky) col += wy[ky] * img[(long long)iy[ky] * PW + ix[kx]];
        v += wx[kx] * col;
    }
    return v;
}

}  // namespace inr
