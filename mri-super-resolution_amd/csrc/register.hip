// register_imgset of the multi-image tree (multi-image-super-resolution/utils/preprocessing.py:138-161): per image of a set the masked
// normalised cross-correlation against the set's clearest image (masked_register_translation, Padfield 2012) and the cubic-spline
// scipy.ndimage.shift of the image ('reflect') and of its quality mask ('constant').  tests/register_common.py restates all of it.
//
//   clearance: mean(mask, axis=(0, 1)) per image; the reference image of a set is the FIRST maximum (np.argmax)
//   correlation, by definition (scikit-image forms the same six sums with FFTs): for the displacement d, pixel p of ref pairs with
//       pixel p - d of x; with the one mask m of x on both sides the pairs with m(p) and m(p - d) set give
//       n, num = S_ab - S_a S_b / n, da = max(S_aa - S_a^2 / n, 0), db likewise, den = sqrt(da db)   (n = 0: all of them 0)
//       tol = 1e3 2^-52 max den; C = clip(num / den, -1, 1) where den > tol, else 0; C = 0 where n < overlap_ratio max n
//       shift = the mean position of every d with C(d) == max C: the translation to apply to x
//       One thread owns one displacement and adds its pairs in a fixed pixel order; the maxima are exact in any order.
//   shift: scipy 1.15: spline_filter(order 3) with the half-sample-symmetric start for 'reflect' and the 'mirror' one for 'constant',
//       then the four B-spline weights per axis at o - s, taps outside the line mapped by 'reflect' (d c b a | a b c d | d c b a) or,
//       for 'constant', by 'mirror'; in 'constant' an output whose source coordinate leaves [0, n - 1] on any axis is cval exactly.
// Images fp32, arithmetic fp64, no floating-point atomics: two calls on the same input are bit-equal.
#include <math.h>

#include "internal.h"
#include "spline.h"

namespace inr {
namespace {

constexpr int RG_TILE = 16;                  // displacements per block and pixels per staged tile, per axis
constexpr int RG_HALO = 2 * RG_TILE - 1;     // the pixels of x that a tile of displacements pairs with a tile of ref
// the halo rows lie 48 (value, mask) pairs apart: the 16 lanes of one dy read 16 consecutive pairs, and the rows of the two dy of a
// 32-lane half start 48 pairs = 96 dwords = 32 banks (of 64, ds_read_b64) apart -- 2 x 16 pairs x 2 dwords cover the 64 banks once
constexpr int RG_PITCH = 48;
constexpr int RG_SUMS = 6;

// ---- clearances and the reference index -------------------------------------------------------------------------------------------------
// one block per image: thread-strided partial sums in double, then the block in a fixed order
__global__ void __launch_bounds__(256) rg_means_kernel(double* __restrict__ means, const float* __restrict__ images, long long per_image) {
    __shared__ double red[4];
    const float* img = images + blockIdx.x * per_image;
    double acc = 0.0;
    for (long long i = threadIdx.x; i < per_image; i += 256) acc += (double)img[i];
    const double s = block_sum_f64(acc, red);
    if (threadIdx.x == 0) means[blockIdx.x] = s / (double)per_image;
}

// np.argmax per set: the first maximum
__global__ void __launch_bounds__(64) rg_argmax_kernel(int* __restrict__ best, const double* __restrict__ means, int n_sets, int T) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_sets) return;
    int at = 0;
    for (int t = 1; t < T; ++t)
        if (means[(long long)s * T + t] > means[(long long)s * T + at]) at = t;
    best[s] = at;
}

// ---- the six sums ----------------------------------------------------------------------------------------------------------------------------
// grid (displacement tiles, images); thread (tx, ty) owns d = (dy0 + ty - max_dy, dx0 + tx - max_dx).  The block walks ref in
// 16 x 16 pixel tiles, row-major, staged as (ref m, m) beside the 31 x 31 tile of (x m, m) that the block's displacements reach
// from it; pixels outside the image are (0, 0) and add nothing.  sums [image][6][NDY][NDX]
__global__ void __launch_bounds__(RG_TILE* RG_TILE) rg_sums_kernel(double* __restrict__ sums, const float* __restrict__ images,
                                                                    const float* __restrict__ masks, const int* __restrict__ ref_index,
                                                                    int T, int H, int W, int max_dy, int max_dx) {
    __shared__ float2 a_tile[RG_TILE][RG_TILE];
    __shared__ float2 b_tile[RG_HALO][RG_PITCH];
    const int ndy = 2 * max_dy + 1, ndx = 2 * max_dx + 1;
    const int tiles_x = (ndx + RG_TILE - 1) / RG_TILE;
    const int img = blockIdx.y;
    const int iy0 = (int)(blockIdx.x / tiles_x) * RG_TILE, ix0 = (int)(blockIdx.x % tiles_x) * RG_TILE;   // map indices of the tile
    const int tx = threadIdx.x & (RG_TILE - 1), ty = threadIdx.x / RG_TILE;
    const int dy0 = iy0 - max_dy, dx0 = ix0 - max_dx;                                                         // the tile's first d
    const long long plane = (long long)H * W;
    int r = ref_index[img / T];
    r = r < 0 ? 0 : (r > T - 1 ? T - 1 : r);                                  // a bad index must not read beyond the set
    const float* ref = images + ((long long)(img / T) * T + r) * plane;
    const float* x = images + img * plane;
    const float* m = masks + img * plane;

    double n = 0.0, sa = 0.0, sb = 0.0, saa = 0.0, sbb = 0.0, sab = 0.0;
    for (int py0 = 0; py0 < H; py0 += RG_TILE) {
        // rows of x that this ref tile pairs with: py0 + i - dy0 - ty, i, ty in 0..15
        const int qy0 = py0 - dy0 - (RG_TILE - 1);
        if (qy0 + RG_HALO <= 0 || qy0 >= H) continue;                         // block-uniform: no row of x is met
        for (int px0 = 0; px0 < W; px0 += RG_TILE) {
            const int qx0 = px0 - dx0 - (RG_TILE - 1);
            if (qx0 + RG_HALO <= 0 || qx0 >= W) continue;
            __syncthreads();                                                  // the tiles of the previous step are read out
            {
                const int py = py0 + ty, px = px0 + tx;
                float2 v = make_float2(0.f, 0.f);
                if (py < H && px < W) {
                    const float mk = m[(long long)py * W + px] != 0.f ? 1.f : 0.f;
                    v = make_float2(mk != 0.f ? ref[(long long)py * W + px] : 0.f, mk);
                }
                a_tile[ty][tx] = v;
            }
            for (int i = threadIdx.x; i < RG_HALO * RG_HALO; i += RG_TILE * RG_TILE) {
                const int hy = i / RG_HALO, hx = i % RG_HALO;
                const int qy = qy0 + hy, qx = qx0 + hx;
                float2 v = make_float2(0.f, 0.f);
                if (qy >= 0 && qy < H && qx >= 0 && qx < W) {
                    const float mk = m[(long long)qy * W + qx] != 0.f ? 1.f : 0.f;
                    v = make_float2(mk != 0.f ? x[(long long)qy * W + qx] : 0.f, mk);
                }
                b_tile[hy][hx] = v;
            }
            __syncthreads();
            for (int i = 0; i < RG_TILE; ++i) {
                const float2* brow = &b_tile[i - ty + RG_TILE - 1][RG_TILE - 1 - tx];
#pragma unroll
                for (int j = 0; j < RG_TILE; ++j) {
                    const float2 a = a_tile[i][j];                            // one address for the whole wave: a broadcast
                    const float2 b = brow[j];
                    const double av = a.x, am = a.y, bv = b.x, bm = b.y;
                    n += am * bm;
                    sa += av * bm;
                    sb += am * bv;
                    saa += av * av * bm;
                    sbb += am * (bv * bv);
                    sab += av * bv;
                }
            }
        }
    }
    const int iy = iy0 + ty, ix = ix0 + tx;
    if (iy < ndy && ix < ndx) {
        const long long nd = (long long)ndy * ndx;
        double* out = sums + (long long)img * RG_SUMS * nd + (long long)iy * ndx + ix;
        out[0] = n, out[nd] = sa, out[2 * nd] = sb, out[3 * nd] = saa, out[4 * nd] = sbb, out[5 * nd] = sab;
    }
}

// maximum over a block of 256 threads, every thread receives it (exact in any order)
__device__ __forceinline__ double rg_block_max(double v, double* red /*[4]*/) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return s;
}

// integer sum over a block of 256 threads (exact in any order)
__device__ __forceinline__ long long rg_block_sum_ll(long long v, long long* red /*[4]*/) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const long long s = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return s;
}

struct RgTerms { double n, num, den; };
__device__ __forceinline__ RgTerms rg_terms(const double* __restrict__ s, long long nd, long long e) {
    RgTerms t;
    t.n = s[e];
    if (!(t.n > 0.0)) {
        t.num = t.den = 0.0;
        return t;
    }
    const double sa = s[nd + e], sb = s[2 * nd + e];
    t.num = s[5 * nd + e] - sa * sb / t.n;
    const double da = fmax(s[3 * nd + e] - sa * sa / t.n, 0.0), db = fmax(s[4 * nd + e] - sb * sb / t.n, 0.0);
    t.den = sqrt(da * db);
    return t;
}

// one block per image: max den and max n over the window, then C (kept in the image's first sums plane, whose n every thread has
// read for its own entries only), its maximum, and the mean position of the maxima
__global__ void __launch_bounds__(256) rg_finish_kernel(double* __restrict__ shifts, double* __restrict__ peak, int* __restrict__ n_max,
                                                        double* __restrict__ map, double* __restrict__ sums, int max_dy, int max_dx,
                                                        double overlap_ratio) {
    __shared__ double red[4];
    __shared__ long long red_ll[4];
    const long long nd = (long long)(2 * max_dy + 1) * (2 * max_dx + 1);
    const int ndx = 2 * max_dx + 1;
    double* s = sums + (long long)blockIdx.x * RG_SUMS * nd;
    double den_max = 0.0, cnt_max = 0.0;
    for (long long e = threadIdx.x; e < nd; e += 256) {
        const RgTerms t = rg_terms(s, nd, e);
        den_max = fmax(den_max, t.den);
        cnt_max = fmax(cnt_max, t.n);
    }
    den_max = rg_block_max(den_max, red);
    cnt_max = rg_block_max(cnt_max, red);
    const double tol = 1e3 * 2.220446049250313e-16 * den_max, need = overlap_ratio * cnt_max;
    double best = -2.0;
    for (long long e = threadIdx.x; e < nd; e += 256) {
        const RgTerms t = rg_terms(s, nd, e);
        double c = 0.0;
        if (t.den > tol && !(t.n < need)) {
            c = t.num / t.den;
            c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
        }
        s[e] = c;                                                             // the same thread reads it back below
        if (map) map[(long long)blockIdx.x * nd + e] = c;
        best = fmax(best, c);
    }
    best = rg_block_max(best, red);
    long long count = 0, sum_y = 0, sum_x = 0;
    for (long long e = threadIdx.x; e < nd; e += 256)
        if (s[e] == best) {
            ++count;
            sum_y += e / ndx;
            sum_x += e % ndx;
        }
    count = rg_block_sum_ll(count, red_ll);
    sum_y = rg_block_sum_ll(sum_y, red_ll);
    sum_x = rg_block_sum_ll(sum_x, red_ll);
    if (threadIdx.x == 0) {
        shifts[2 * blockIdx.x] = (double)sum_y / (double)count - (double)max_dy;
        shifts[2 * blockIdx.x + 1] = (double)sum_x / (double)count - (double)max_dx;
        peak[blockIdx.x] = best;
        n_max[blockIdx.x] = (int)(count > 2147483647ll ? 2147483647ll : count);
    }
}

// ---- the shift ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rg_widen_kernel(double* __restrict__ out, const float* __restrict__ in, long long total) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) out[idx] = (double)in[idx];
}

// out(o) = the spline of the coefficient plane c at o - shift[image]; a coordinate that is not below 1e9 in size (NaN included)
// gives NaN, so that every tap index fits an int
__global__ void __launch_bounds__(256) rg_shift_kernel(float* __restrict__ out, const double* __restrict__ c, const double* __restrict__ shifts,
                                                       long long total, int H, int W, int mode, double cval) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int ox = (int)(idx % W);
        const int oy = (int)((idx / W) % H);
        const long long b = idx / ((long long)W * H);
        const double y = (double)oy - shifts[2 * b], x = (double)ox - shifts[2 * b + 1];
        if (!(fabs(y) < 1e9 && fabs(x) < 1e9)) {
            out[idx] = __builtin_nanf("");
            continue;
        }
        if (mode == INR_SHIFT_CONSTANT && (y < 0.0 || y > (double)(H - 1) || x < 0.0 || x > (double)(W - 1))) {
            out[idx] = (float)cval;
            continue;
        }
        const double fy0 = floor(y), fx0 = floor(x);
        double wy[4], wx[4];
        int iy[4], ix[4];
        bspline3_weights(y - fy0, wy);
        bspline3_weights(x - fx0, wx);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ty = (int)fy0 - 1 + k, tx = (int)fx0 - 1 + k;
            iy[k] = mode == INR_SHIFT_REFLECT ? reflect_index(ty, H) : mirror_index(ty, H);
            ix[k] = mode == INR_SHIFT_REFLECT ? reflect_index(tx, W) : mirror_index(tx, W);
        }
        out[idx] = (float)spline_tap_sum<4>(c + b * ((long long)H * W), W, iy, ix, wy, wx);
    }
}

int xcorr_check(const char* who, int n_sets, int T, int H, int W, int max_dy, int max_dx) {
    INR_REQUIRE(n_sets >= 1 && T >= 1 && H >= 1 && W >= 1, INR_E_INVALID, "%s: bad sizes (%d sets of %d images of %d x %d)", who, n_sets, T,
                H, W);
    INR_REQUIRE(H <= INR_XCORR_MAX_SIDE && W <= INR_XCORR_MAX_SIDE, INR_E_INVALID, "%s: images of at most %d x %d (got %d x %d)", who,
                INR_XCORR_MAX_SIDE, INR_XCORR_MAX_SIDE, H, W);
    INR_REQUIRE((long long)n_sets * T <= 65535, INR_E_INVALID, "%s: at most 65535 images per call (got %lld)", who, (long long)n_sets * T);
    INR_REQUIRE(max_dy >= 0 && max_dy <= H - 1 && max_dx >= 0 && max_dx <= W - 1, INR_E_INVALID,
                "%s: the window must satisfy 0 <= max_dy <= H - 1 and 0 <= max_dx <= W - 1 (got %d, %d for %d x %d)", who, max_dy, max_dx, H,
                W);
    return 0;
}

size_t xcorr_doubles(int n_sets, int T, int max_dy, int max_dx) {
    return (size_t)n_sets * (size_t)T * RG_SUMS * (size_t)(2 * max_dy + 1) * (size_t)(2 * max_dx + 1);
}

int shift_check(const char* who, int n, int H, int W, int mode, double cval) {
    INR_REQUIRE(mode == INR_SHIFT_REFLECT || mode == INR_SHIFT_CONSTANT, INR_E_INVALID,
                "%s: mode must be INR_SHIFT_REFLECT or INR_SHIFT_CONSTANT (got %d)", who, mode);
    INR_REQUIRE(n >= 0 && H >= 1 && W >= 1, INR_E_INVALID, "%s: bad sizes", who);
    INR_REQUIRE(H <= INR_RESCALE_MAX_LINE && W <= INR_RESCALE_MAX_LINE, INR_E_INVALID, "%s: lines of at most %d samples (got %d x %d)", who,
                INR_RESCALE_MAX_LINE, H, W);
    INR_REQUIRE(cval == cval, INR_E_INVALID, "%s: cval is NaN", who);
    return 0;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int inr_image_means(double* means, int* argmax, const float* images, int n_sets, int T, int height, int width, void* stream) {
    INR_REQUIRE(means && images, INR_E_INVALID, "inr_image_means: null pointer");
    INR_REQUIRE(n_sets >= 1 && T >= 1 && height >= 1 && width >= 1, INR_E_INVALID, "inr_image_means: bad sizes");
    INR_REQUIRE((long long)n_sets * T < (1ll << 31), INR_E_INVALID, "inr_image_means: too many images");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL(rg_means_kernel, dim3((unsigned)(n_sets * T)), dim3(256), 0, st, means, images, (long long)height * width);
    INR_LAUNCH_CHECK();
    if (argmax) {
        hipLaunchKernelGGL(rg_argmax_kernel, dim3((unsigned)((n_sets + 63) / 64)), dim3(64), 0, st, argmax, (const double*)means, n_sets, T);
        INR_LAUNCH_CHECK();
    }
    return 0;
}

int64_t inr_masked_xcorr_workspace_doubles(int n_sets, int T, int height, int width, int max_dy, int max_dx) {
    if (xcorr_check("inr_masked_xcorr_workspace_doubles", n_sets, T, height, width, max_dy, max_dx)) return 0;
    return (int64_t)xcorr_doubles(n_sets, T, max_dy, max_dx);
}

int inr_masked_xcorr(double* shifts, double* peak, int* n_max, double* map, const float* images, const float* masks,
                     const int* ref_index, int n_sets, int T, int height, int width, int max_dy, int max_dx, double overlap_ratio,
                     double* workspace, int64_t workspace_doubles, void* stream) {
    INR_REQUIRE(shifts && peak && n_max && images && masks && ref_index, INR_E_INVALID, "inr_masked_xcorr: null pointer");
    if (int rc = xcorr_check("inr_masked_xcorr", n_sets, T, height, width, max_dy, max_dx)) return rc;
    INR_REQUIRE(overlap_ratio >= 0.0 && overlap_ratio <= 1.0, INR_E_INVALID, "inr_masked_xcorr: overlap_ratio must lie in [0, 1] (got %g)",
                overlap_ratio);
    const size_t need = xcorr_doubles(n_sets, T, max_dy, max_dx) * sizeof(double);
    if (int rc = check_ws_doubles("inr_masked_xcorr", workspace, workspace_doubles, need)) return rc;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(KC_OTHER, st);
    const int nimg = n_sets * T;
    const unsigned tiles = (unsigned)(((2 * max_dy + 1 + RG_TILE - 1) / RG_TILE) * ((2 * max_dx + 1 + RG_TILE - 1) / RG_TILE));
    hipLaunchKernelGGL(rg_sums_kernel, dim3(tiles, (unsigned)nimg), dim3(RG_TILE * RG_TILE), 0, st, workspace, images, masks, ref_index, T,
                       height, width, max_dy, max_dx);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rg_finish_kernel, dim3((unsigned)nimg), dim3(256), 0, st, shifts, peak, n_max, map, workspace, max_dy, max_dx,
                       overlap_ratio);
    INR_LAUNCH_CHECK();
    return 0;
}

int64_t inr_shift2d_workspace_doubles(int n_images, int height, int width, int mode) {
    if (shift_check("inr_shift2d_workspace_doubles", n_images, height, width, mode, 0.0)) return 0;
    return (int64_t)((size_t)(n_images > 0 ? n_images : 1) * (size_t)height * (size_t)width);
}

int inr_shift2d(float* out, const float* in, const double* shifts, int n_images, int height, int width, int mode, double cval,
                double* workspace, int64_t workspace_doubles, void* stream) {
    INR_REQUIRE(out && in && shifts, INR_E_INVALID, "inr_shift2d: null pointer");
    if (int rc = shift_check("inr_shift2d", n_images, height, width, mode, cval)) return rc;
    const size_t need = (size_t)inr_shift2d_workspace_doubles(n_images, height, width, mode) * sizeof(double);
    if (int rc = check_ws_doubles("inr_shift2d", workspace, workspace_doubles, need)) return rc;
    if (n_images == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(KC_OTHER, st);
    const long long total = (long long)n_images * height * width;
    hipLaunchKernelGGL(rg_widen_kernel, dim3(rs_blocks(total)), dim3(256), 0, st, workspace, in, total);
    INR_LAUNCH_CHECK();
    if (int rc = mode == INR_SHIFT_REFLECT ? launch_spline_prefilter<SPLINE_REFLECT>(workspace, n_images, height, width, st)
                                           : launch_spline_prefilter<SPLINE_MIRROR>(workspace, n_images, height, width, st))
        return rc;
    hipLaunchKernelGGL(rg_shift_kernel, dim3(rs_blocks(total)), dim3(256), 0, st, out, (const double*)workspace, shifts, total, height, width,
                       mode, cval);
    INR_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
