// skimage 0.20 `resize` for 2-D images -- down-scaling with its anti-aliasing Gaussian, orders 1 and 3, modes 'reflect' and 'edge'
// -- restated through the scipy calls it makes (prepare_qual_images.py:152,198,207,267 rescale(x, .5, anti_aliasing=True);
// multi-image-super-resolution/utils/preprocessing.py:271-294 bicubic).  tests/rescale_common.py restates the same steps in numpy.
//
//   f = in / out per axis (from the rounded shapes, not from the scale)
//   anti-aliasing: ndi.gaussian_filter(img, sigma = max(0, (f - 1)/2), mode = M): separable, axis 0 first, radius int(4 sigma + .5),
//       weights exp(-x^2 / (2 sigma^2)) / sum formed in double on the host; sigma = 0 skips the axis
//   re-sampling:   ndi.zoom(., 1/f, order, mode = M, grid_mode = True): x = (o + .5) in/out - .5;
//       order 1: (1 - t) c[m(i)] + t c[m(i + 1)], i = floor(x), t = x - i  (the formula of rescale_linear_kernel, metrics.hip)
//       order 3: cubic B-spline prefilter on every line of axis 0, then of axis 1 (pole z = sqrt(3) - 2, gain (1 - z)(1 - 1/z),
//                scipy's mirror start and end), then the four B-spline weights per axis on c[m(i - 1 .. i + 2)];
//                M = 'nearest' first pads the image by 12 edge samples per side and evaluates at x + 12
//   M = 'mirror' (skimage 'reflect'): m = reflection about the edge samples, period 2n - 2, any number of periods (a Gaussian
//       radius may exceed the line);  M = 'nearest' (skimage 'edge'): m = clamp
//   clip: the result is clamped to [min, max] of its input group (skimage clip=True; a group is the images of one skimage call)
// All arithmetic in fp64, images fp32 in and out.  Nothing here is bandwidth- or latency-critical: the boundary rules are the job.
#include <math.h>

#include "internal.h"
#include "spline.h"

namespace inr {
namespace {

constexpr int RESCALE_MAX_RADIUS = INR_RESCALE_MAX_RADIUS;   // Gaussian taps per side that the kernel arguments carry
constexpr int RESCALE_MAX_LINE = INR_RESCALE_MAX_LINE;       // one padded line, staged in LDS as doubles, fits 64 KiB
constexpr int RS_PAD = 12;   // scipy: _prepad_for_spline_filter
struct RescaleView { double *filtered, *coef, *minmax; size_t total; };

__device__ __forceinline__ int rs_index(int i, int n, int mode) {
    if (mode == INR_RESCALE_EDGE) return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    return mirror_index(i, n);
}

// half of a symmetric Gaussian: w[k] weighs the samples k away; radius 0 is the identity
struct RsTaps {
    int radius;
    double w[RESCALE_MAX_RADIUS + 1];
};

// one separable pass along `axis` (0: rows apart, 1: within a row) of [nimg][H][W]; T = float (the input) or double
template <typename T>
__global__ void __launch_bounds__(256) rs_gauss_kernel(double* __restrict__ out, const T* __restrict__ in, long long total, int H, int W,
                                                       int axis, int mode, RsTaps taps) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int x = (int)(idx % W);
        const int y = (int)((idx / W) % H);
        const T* img = in + (idx / ((long long)W * H)) * ((long long)W * H);
        const int n = axis == 0 ? H : W, p = axis == 0 ? y : x;
        const long long stride = axis == 0 ? W : 1, base = axis == 0 ? x : (long long)y * W;
        double acc = taps.w[0] * (double)img[base + p * stride];
        for (int k = 1; k <= taps.radius; ++k)
            acc += taps.w[k] * ((double)img[base + rs_index(p - k, n, mode) * stride] + (double)img[base + rs_index(p + k, n, mode) * stride]);
        out[idx] = acc;
    }
}

// minimum and maximum of each group of `per_group` consecutive floats: one block per group, a fixed order (and min / max are
// exact in any order) -> mm[2 g], mm[2 g + 1]
__global__ void __launch_bounds__(256) rs_minmax_kernel(double* __restrict__ mm, const float* __restrict__ in, long long per_group) {
    __shared__ float red[8];
    const float* g = in + blockIdx.x * per_group;
    float lo = g[0], hi = g[0];
    for (long long i = threadIdx.x; i < per_group; i += 256) {
        lo = fminf(lo, g[i]);
        hi = fmaxf(hi, g[i]);
    }
    lo = -wave_max(-lo);
    hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = lo;
        red[4 + (threadIdx.x >> 6)] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        mm[2 * blockIdx.x] = (double)fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
        mm[2 * blockIdx.x + 1] = (double)fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    }
}

// [nimg][H][W] -> [nimg][H + 2 pad][W + 2 pad], the border filled with the edge value
__global__ void __launch_bounds__(256) rs_pad_kernel(double* __restrict__ out, const double* __restrict__ in, long long total, int H, int W,
                                                     int pad) {
    const int PH = H + 2 * pad, PW = W + 2 * pad;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int x = rs_index((int)(idx % PW) - pad, W, INR_RESCALE_EDGE);
        const int y = rs_index((int)((idx / PW) % PH) - pad, H, INR_RESCALE_EDGE);
        out[idx] = in[(idx / ((long long)PW * PH)) * ((long long)W * H) + (long long)y * W + x];
    }
}

// samples the [nimg][PH][PW] plane c (PH = H + 2 pad) at the grid of the [OH][OW] output, separable with axis 0 first, clips, rounds
// once to fp32.  mm == null: no clip; else image b belongs to group b / clip_group
template <int ORDER>
__global__ void __launch_bounds__(256) rs_sample_kernel(float* __restrict__ out, const double* __restrict__ c, const double* __restrict__ mm,
                                                        long long total, int H, int W, int OH, int OW, int pad, int mode, int clip_group) {
    const int PH = H + 2 * pad, PW = W + 2 * pad;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int ox = (int)(idx % OW);
        const int oy = (int)((idx / OW) % OH);
        const long long b = idx / ((long long)OW * OH);
        const double y = (oy + 0.5) * ((double)H / OH) - 0.5 + pad, x = (ox + 0.5) * ((double)W / OW) - 0.5 + pad;
        const double fy0 = floor(y), fx0 = floor(x);
        const double ty = y - fy0, tx = x - fx0;
        const double* img = c + b * ((long long)PH * PW);
        constexpr int TAPS = ORDER == 1 ? 2 : 4;
        double wy[TAPS], wx[TAPS];
        int iy[TAPS], ix[TAPS];
        if (ORDER == 1) {
            wy[0] = 1.0 - ty, wy[1] = ty, wx[0] = 1.0 - tx, wx[1] = tx;
        } else {
            bspline3_weights(ty, wy);
            bspline3_weights(tx, wx);
        }
        const int first = ORDER == 1 ? 0 : -1;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            iy[k] = rs_index((int)fy0 + first + k, PH, mode);
            ix[k] = rs_index((int)fx0 + first + k, PW, mode);
        }
        double v = spline_tap_sum<TAPS>(img, PW, iy, ix, wy, wx);
        if (mm) {
            const double lo = mm[2 * (b / clip_group)], hi = mm[2 * (b / clip_group) + 1];
            v = v < lo ? lo : (v > hi ? hi : v);
        }
        out[idx] = (float)v;
    }
}

// sigma and taps of one axis; false when the radius is beyond what RsTaps carries
bool rs_taps(RsTaps& t, int n_in, int n_out, int anti_aliasing) {
    const double f = (double)n_in / (double)n_out;
    const double sigma = anti_aliasing && f > 1.0 ? (f - 1.0) / 2.0 : 0.0;
    t.radius = (int)(4.0 * sigma + 0.5);
    if (t.radius > RESCALE_MAX_RADIUS) return false;
    t.w[0] = 1.0;
    if (sigma <= 0.0) {
        t.radius = 0;
        return true;
    }
    double sum = 0.0;   // numpy's order is not reproduced: the sum of <= 129 positive terms differs by rounding only
    for (int k = -t.radius; k <= t.radius; ++k) sum += exp(-0.5 / (sigma * sigma) * (double)k * (double)k);
    for (int k = 0; k <= t.radius; ++k) t.w[k] = exp(-0.5 / (sigma * sigma) * (double)k * (double)k) / sum;
    return true;
}

int rs_pad_of(int order, int mode) { return order == 3 && mode == INR_RESCALE_EDGE ? RS_PAD : 0; }

// the workspace: the filtered plane, the (padded) coefficient plane -- which first serves as the buffer between the two Gaussian
// passes -- and one (min, max) pair per image (an upper bound on the number of clip groups).  base == null: `total` only
RescaleView rescale_view(int nimg, int H, int W, int order, int mode, void* base) {
    RescaleView v;
    WsCarver c(base, 256);
    const int pad = rs_pad_of(order, mode);
    const size_t images = nimg > 0 ? (size_t)nimg : 1;
    v.filtered = c.take<double>(images * (size_t)H * (size_t)W);
    v.coef = c.take<double>(images * (size_t)(H + 2 * pad) * (size_t)(W + 2 * pad));
    v.minmax = c.take<double>(2 * images);
    v.total = c.bytes();
    return v;
}

int rescale_check(const char* who, int nimg, int H, int W, int OH, int OW, int order, int mode, int anti_aliasing, int clip_group) {
    INR_REQUIRE(order == 1 || order == 3, INR_E_INVALID, "%s: order must be 1 or 3 (got %d)", who, order);
    INR_REQUIRE(mode == INR_RESCALE_REFLECT || mode == INR_RESCALE_EDGE, INR_E_INVALID,
                "%s: mode must be INR_RESCALE_REFLECT or INR_RESCALE_EDGE (got %d)", who, mode);
    INR_REQUIRE(nimg >= 0 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1, INR_E_INVALID, "%s: bad sizes", who);
    INR_REQUIRE(H <= RESCALE_MAX_LINE && W <= RESCALE_MAX_LINE && OH <= RESCALE_MAX_LINE && OW <= RESCALE_MAX_LINE, INR_E_INVALID,
                "%s: lines of at most %d samples (got %d x %d -> %d x %d)", who, RESCALE_MAX_LINE, H, W, OH, OW);
    INR_REQUIRE(clip_group >= 0 && (clip_group == 0 || nimg % clip_group == 0), INR_E_INVALID,
                "%s: clip_group (%d) must be 0 or divide n_images (%d)", who, clip_group, nimg);
    RsTaps t;
    INR_REQUIRE(rs_taps(t, H, OH, anti_aliasing) && rs_taps(t, W, OW, anti_aliasing), INR_E_INVALID,
                "%s: anti-aliasing radius beyond %d taps (%d x %d -> %d x %d)", who, RESCALE_MAX_RADIUS, H, W, OH, OW);
    return 0;
}

// everything validated (rescale_check) and the workspace checked by the caller
int launch_rescale2d(float* out, const float* in, int nimg, int H, int W, int OH, int OW, int order, int mode, int anti_aliasing,
                     int clip_group, const RescaleView& v, hipStream_t st) {
    if (nimg == 0) return 0;
    RsTaps t0, t1;
    rs_taps(t0, H, OH, anti_aliasing);
    rs_taps(t1, W, OW, anti_aliasing);
    const int pad = rs_pad_of(order, mode), PH = H + 2 * pad, PW = W + 2 * pad;
    const long long plane = (long long)nimg * H * W;
    ProfScope ps(KC_OTHER, st);
    if (clip_group > 0) {
        hipLaunchKernelGGL(rs_minmax_kernel, dim3((unsigned)(nimg / clip_group)), dim3(256), 0, st, v.minmax, in,
                           (long long)clip_group * H * W);
        INR_LAUNCH_CHECK();
    }
    // in -> coef (axis 0) -> filtered (axis 1); a radius of 0 copies
    hipLaunchKernelGGL(rs_gauss_kernel<float>, dim3(rs_blocks(plane)), dim3(256), 0, st, v.coef, in, plane, H, W, 0, mode, t0);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rs_gauss_kernel<double>, dim3(rs_blocks(plane)), dim3(256), 0, st, v.filtered, (const double*)v.coef, plane, H, W,
                       1, mode, t1);
    INR_LAUNCH_CHECK();
    const double* mm = clip_group > 0 ? v.minmax : nullptr;
    const long long total = (long long)nimg * OH * OW;
    if (order == 1) {
        hipLaunchKernelGGL(rs_sample_kernel<1>, dim3(rs_blocks(total)), dim3(256), 0, st, out, (const double*)v.filtered, mm, total, H, W,
                           OH, OW, 0, mode, clip_group);
        INR_LAUNCH_CHECK();
        return 0;
    }
    const long long padded = (long long)nimg * PH * PW;
    hipLaunchKernelGGL(rs_pad_kernel, dim3(rs_blocks(padded)), dim3(256), 0, st, v.coef, (const double*)v.filtered, padded, H, W, pad);
    INR_LAUNCH_CHECK();
    static_assert(((RESCALE_MAX_LINE + 2 * RS_PAD) | 1) * sizeof(double) <= RS_LDS_BYTES, "one staged row must fit the LDS");
    if (int rc = launch_spline_prefilter<SPLINE_MIRROR>(v.coef, nimg, PH, PW, st)) return rc;
    hipLaunchKernelGGL(rs_sample_kernel<3>, dim3(rs_blocks(total)), dim3(256), 0, st, out, (const double*)v.coef, mm, total, H, W, OH, OW,
                       pad, mode, clip_group);
    INR_LAUNCH_CHECK();
    return 0;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_rescale2d_workspace_doubles(int n_images, int height, int width, int order, int mode) {
    if (rescale_check("inr_rescale2d_workspace_doubles", n_images, height, width, 1, 1, order, mode, 0, 0)) return 0;
    return (int64_t)(rescale_view(n_images, height, width, order, mode, nullptr).total / sizeof(double));
}

int inr_rescale2d(float* out, const float* in, int n_images, int height, int width, int out_height, int out_width, int order,
                  int mode, int anti_aliasing, int clip_group, double* workspace, int64_t workspace_doubles, void* stream) {
    INR_REQUIRE(out && in, INR_E_INVALID, "inr_rescale2d: null pointer");
    if (int rc = rescale_check("inr_rescale2d", n_images, height, width, out_height, out_width, order, mode, anti_aliasing, clip_group))
        return rc;
    const RescaleView v = rescale_view(n_images, height, width, order, mode, workspace);
    if (int rc = check_ws_doubles("inr_rescale2d", workspace, workspace_doubles, v.total)) return rc;
    return launch_rescale2d(out, in, n_images, height, width, out_height, out_width, order, mode, anti_aliasing, clip_group, v,
                            (hipStream_t)stream);
}

}  // extern "C"
