// The reader study's image scores (implicit-neural-representations/perceptual_similarity_tests/perceptual_similarity.m:41-52, HPF.m):
// Gaussian-window SSIM, MS-SSIM (Wang et al. 2003), the 3 x 3 high-pass, MSE and the high-frequency gain, on the device.  There is
// no MATLAB here: the kernels follow the DEFINITIONS of DESIGN.md 4g (MATLAB's documented defaults for ssim / immse / imfilter /
// fspecial('unsharp')), which tests/perceptual_common.py restates in float64 NumPy / SciPy.
//
//   window   r = ceil(3 sigma) <= 7, g[k] = exp(-k^2 / (2 sigma^2)) / sum, separable (rows, then columns), indices clamped to the edge
//   ssim     mx = F x, my = F y, vx = max(F(x^2) - mx^2, 0), vy likewise, vxy = F(xy) - mx my, C1 = (.01 L)^2, C2 = (.03 L)^2
//            l = (2 mx my + C1) / (mx^2 + my^2 + C1), cs = (2 vxy + C2) / (vx + vy + C2); the map l cs on the FULL image; its mean
//   ms-ssim  mean(cs) at scales 0 .. S-2, mean(l cs) at scale S-1, prod v_s^w_s; between scales the 2 x 2 block means with the
//            indices clamped (ceil(H/2) x ceil(W/2)); the levels stay fp64
//   filter   3 x 3 correlation, zero padding, fp64 sum rounded once to fp32
// All arithmetic fp64.  Plain launches, one partial per (image, block, quantity), added front to back by one thread per image: calls
// are bit-equal, and an image's bits depend on neither its neighbours in the batch nor on where a pixel falls in a tile (every
// pixel runs the same operations in the same order).
#include <math.h>

#include "internal.h"

namespace inr {
namespace {

constexpr int PERCEPTUAL_MAX_RADIUS = INR_PERCEPTUAL_MAX_RADIUS;   // window taps per side: what the tile's halo in LDS holds
constexpr int PERCEPTUAL_MAX_SCALES = INR_PERCEPTUAL_MAX_SCALES;
struct PerceptualView { double *reduce, *partial, *vals, *lx[2], *ly[2]; size_t total; };

constexpr int PC_TW = 32, PC_TH = 16;                                  // the output tile of one block of 256 threads: 2 pixels per thread
constexpr int PC_RMAX = PERCEPTUAL_MAX_RADIUS;
constexpr int PC_SW = PC_TW + 2 * PC_RMAX, PC_SH = PC_TH + 2 * PC_RMAX;   // the staged tile with its halo: 46 x 30
constexpr int PC_RED_BLOCKS = 64;                                      // blocks per image of the two flat reductions
// static LDS of pc_ssim_kernel: x and y tiles 2 * 30 * 46 * 8 = 22,080 B, the row pass 5 * 30 * 32 * 8 = 38,400 B, 32 B for the
// block sum: 60,512 B (a 32 x 32 tile would need 92,768 B)
static_assert((2 * PC_SH * PC_SW + 5 * PC_SH * PC_TW + 4) * sizeof(double) < 65536, "pc_ssim_kernel: static LDS under 64 KiB");

struct PcTaps {
    int r;
    double w[PC_RMAX + 1];   // w[k] weighs the samples k away
};
struct PcK9 { double k[9]; };
struct PcWeights { int n; double w[PERCEPTUAL_MAX_SCALES]; };

__device__ __forceinline__ int pc_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// One block per (tile, image).  The x and y tiles with their r-wide halo go to LDS once (the clamp is applied here), the row pass
// writes the five filtered quantities x, y, x^2, y^2, xy for every staged row to LDS, the column pass reads them back; l and cs
// are formed in registers.  partial[(b * tiles + tile) * 2 + {0, 1}] = the tile's sums of l cs and of cs; map (nullable) [b][H][W].
template <typename T>
__global__ void __launch_bounds__(256) pc_ssim_kernel(double* __restrict__ partial, float* __restrict__ map, const T* __restrict__ x,
                                                      const T* __restrict__ y, int H, int W, int tiles_x, PcTaps taps, double c1,
                                                      double c2) {
    __shared__ double sx[PC_SH][PC_SW], sy[PC_SH][PC_SW];
    __shared__ double rp[5][PC_SH][PC_TW];
    __shared__ double red[4];
    const int r = taps.r, tid = threadIdx.x;
    const int b = blockIdx.y, tile = blockIdx.x;
    const int ty0 = (tile / tiles_x) * PC_TH, tx0 = (tile % tiles_x) * PC_TW;
    const int sh = PC_TH + 2 * r, sw = PC_TW + 2 * r;
    const T* xb = x + (int64_t)b * H * W;
    const T* yb = y + (int64_t)b * H * W;
    for (int i = tid; i < sh * sw; i += 256) {
        const int rr = i / sw, cc = i - rr * sw;
        const int64_t at = (int64_t)pc_clamp(ty0 + rr - r, H) * W + pc_clamp(tx0 + cc - r, W);
        sx[rr][cc] = (double)xb[at];
        sy[rr][cc] = (double)yb[at];
    }
    __syncthreads();
    for (int i = tid; i < sh * PC_TW; i += 256) {
        const int rr = i / PC_TW, c = i - rr * PC_TW;
        double ax = 0, ay = 0, axx = 0, ayy = 0, axy = 0;
        for (int k = -r; k <= r; ++k) {
            const double w = taps.w[k < 0 ? -k : k], xv = sx[rr][c + r + k], yv = sy[rr][c + r + k];
            ax += w * xv;
            ay += w * yv;
            axx += w * (xv * xv);
            ayy += w * (yv * yv);
            axy += w * (xv * yv);
        }
        rp[0][rr][c] = ax;
        rp[1][rr][c] = ay;
        rp[2][rr][c] = axx;
        rp[3][rr][c] = ayy;
        rp[4][rr][c] = axy;
    }
    __syncthreads();
    const int c = tid & (PC_TW - 1);
    double s_lcs = 0.0, s_cs = 0.0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int row = (tid >> 5) + 8 * half;
        double mx = 0, my = 0, fxx = 0, fyy = 0, fxy = 0;
        for (int k = -r; k <= r; ++k) {
            const double w = taps.w[k < 0 ? -k : k];
            mx += w * rp[0][row + r + k][c];
            my += w * rp[1][row + r + k][c];
            fxx += w * rp[2][row + r + k][c];
            fyy += w * rp[3][row + r + k][c];
            fxy += w * rp[4][row + r + k][c];
        }
        const int gy = ty0 + row, gx = tx0 + c;
        if (gy < H && gx < W) {
            // no fused multiply-adds here: with x == y, mx my and mx^2 (and 2 vxy and vx + vy) must round alike, so that the
            // map of identical images is exactly 1
#pragma clang fp contract(off)
            const double pxx = mx * mx, pyy = my * my, pxy = mx * my;
            double vx = fxx - pxx, vy = fyy - pyy;
            vx = vx > 0.0 ? vx : 0.0;
            vy = vy > 0.0 ? vy : 0.0;
            const double vxy = fxy - pxy;
            const double l = (2.0 * pxy + c1) / (pxx + pyy + c1);
            const double cs = (2.0 * vxy + c2) / (vx + vy + c2);
            const double lcs = l * cs;
            s_lcs += lcs;
            s_cs += cs;
            if (map) map[(int64_t)b * H * W + (int64_t)gy * W + gx] = (float)lcs;
        }
    }
    s_lcs = block_sum_f64(s_lcs, red);
    s_cs = block_sum_f64(s_cs, red);
    if (tid == 0) {
        double* p = partial + ((int64_t)b * gridDim.x + tile) * 2;
        p[0] = s_lcs;
        p[1] = s_cs;
    }
}

// partial [nimg][nblk][2] -> a[b] = sum_k partial[b][k][0] / da (, b_[b] = sum_k partial[b][k][1] / db); ratio != 0: a[b] =
// sum0 / sum1 instead.  Front to back, one thread per image; null outputs are skipped.
__global__ void pc_finish_kernel(double* __restrict__ a, double* __restrict__ b_, const double* __restrict__ partial, int nblk, double da,
                                 double db, int ratio, int nimg) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nimg) return;
    double s0 = 0.0, s1 = 0.0;
    for (int k = 0; k < nblk; ++k) {
        s0 += partial[((int64_t)b * nblk + k) * 2];
        s1 += partial[((int64_t)b * nblk + k) * 2 + 1];
    }
    if (ratio) {
        a[b] = s0 / s1;
        return;
    }
    if (a) a[b] = s0 / da;
    if (b_) b_[b] = s1 / db;
}

// out[b] = prod_s vals[s][b] ^ w[s] (pow: NaN for a negative base under a fractional weight); per_scale (nullable) [nimg][n]
__global__ void pc_msssim_finish_kernel(double* __restrict__ out, double* __restrict__ per_scale, const double* __restrict__ vals,
                                        PcWeights wt, int nimg) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nimg) return;
    double p = 1.0;
    for (int s = 0; s < wt.n; ++s) {
        const double v = vals[(int64_t)s * nimg + b];
        p *= pow(v, wt.w[s]);
        if (per_scale) per_scale[(int64_t)b * wt.n + s] = v;
    }
    out[b] = p;
}

// [nimg][H][W] -> [nimg][ceil(H/2)][ceil(W/2)] fp64: the mean of the 2 x 2 block, indices clamped
template <typename T>
__global__ void __launch_bounds__(256) pc_down2_kernel(double* __restrict__ out, const T* __restrict__ in, long long total, int H, int W) {
    const int OH = (H + 1) / 2, OW = (W + 1) / 2;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int j = (int)(idx % OW), i = (int)((idx / OW) % OH);
        const T* img = in + (idx / ((long long)OW * OH)) * ((long long)H * W);
        const int y0 = 2 * i, y1 = pc_clamp(2 * i + 1, H), x0 = 2 * j, x1 = pc_clamp(2 * j + 1, W);
        const double s = ((double)img[(long long)y0 * W + x0] + (double)img[(long long)y0 * W + x1]) +
                         ((double)img[(long long)y1 * W + x0] + (double)img[(long long)y1 * W + x1]);
        out[idx] = 0.25 * s;
    }
}

// out[b][i][j] = sum_{a, c} k[a][c] in[b][i + a - 1][j + c - 1], samples outside the image are zero; one rounding to fp32
__global__ void __launch_bounds__(256) pc_filter3x3_kernel(float* __restrict__ out, const float* __restrict__ in, long long total, int H,
                                                           int W, PcK9 k9) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int j = (int)(idx % W), i = (int)((idx / W) % H);
        const float* img = in + (idx / ((long long)W * H)) * ((long long)W * H);
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int yy = i + a - 1, xx = j + c - 1;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) acc += k9.k[3 * a + c] * (double)img[(long long)yy * W + xx];
            }
        out[idx] = (float)acc;
    }
}

// partial[b][blk][2]: MODE 0 = (sum (x - y)^2, 0); MODE 1 = (sum max(x - y, 0)^2, sum y^2)
template <int MODE>
__global__ void __launch_bounds__(256) pc_pair_sums_kernel(double* __restrict__ partial, const float* __restrict__ x,
                                                           const float* __restrict__ y, int64_t per_image) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const float* xb = x + (int64_t)b * per_image;
    const float* yb = y + (int64_t)b * per_image;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_image; i += (int64_t)PC_RED_BLOCKS * 256) {
        const double yv = (double)yb[i];
        double d = (double)xb[i] - yv;
        if (MODE == 1) {
            d = d > 0.0 ? d : 0.0;
            s1 += yv * yv;
        }
        s0 += d * d;
    }
    s0 = block_sum_f64(s0, red);
    s1 = block_sum_f64(s1, red);
    if (threadIdx.x == 0) {
        double* p = partial + ((int64_t)b * PC_RED_BLOCKS + blockIdx.x) * 2;
        p[0] = s0;
        p[1] = s1;
    }
}

inline unsigned pc_blocks(long long work) {
    const long long b = (work + 255) / 256;
    return (unsigned)(b > 65536 ? 65536 : b);
}

inline int pc_tiles(int H, int W) { return ((H + PC_TH - 1) / PC_TH) * ((W + PC_TW - 1) / PC_TW); }

bool pc_taps(PcTaps& t, double sigma) {
    if (!(sigma > 0.0) || !(sigma <= (double)PC_RMAX)) return false;   // (also refuses NaN)
    const int r = (int)ceil(3.0 * sigma);
    if (r > PC_RMAX) return false;
    t.r = r;
    double sum = 0.0;
    for (int k = -r; k <= r; ++k) sum += exp(-(double)(k * k) / (2.0 * sigma * sigma));
    for (int k = 0; k <= PC_RMAX; ++k) t.w[k] = k <= r ? exp(-(double)(k * k) / (2.0 * sigma * sigma)) / sum : 0.0;
    return true;
}

template <typename T>
int pc_ssim_level(double* lcs, double* cs, float* map, const T* x, const T* y, int nimg, int H, int W, const PcTaps& t, double c1,
                  double c2, double* partial, hipStream_t st) {
    const int tiles_x = (W + PC_TW - 1) / PC_TW, tiles = pc_tiles(H, W);
    hipLaunchKernelGGL(pc_ssim_kernel<T>, dim3((unsigned)tiles, (unsigned)nimg), dim3(256), 0, st, partial, map, x, y, H, W, tiles_x, t,
                       c1, c2);
    INR_LAUNCH_CHECK();
    const double count = (double)H * (double)W;
    hipLaunchKernelGGL(pc_finish_kernel, dim3((nimg + 63) / 64), dim3(64), 0, st, lcs, cs, (const double*)partial, tiles, count, count,
                       0, nimg);
    INR_LAUNCH_CHECK();
    return 0;
}

// the workspace of every entry point of this unit: the two flat reductions' partials first (so that a view sized for any image
// shape serves inr_image_mse and inr_hf_gain), the tile partials, the per-scale means, and two pairs of fp64 levels (level s lives
// in pair s & 1).  base == null: `total` only
PerceptualView perceptual_view(int nimg, int H, int W, int n_scales, void* base) {
    PerceptualView v;
    WsCarver c(base, 256);
    const size_t images = nimg > 0 ? (size_t)nimg : 1;
    H = H > 0 ? H : 1;
    W = W > 0 ? W : 1;
    v.reduce = c.take<double>(images * PC_RED_BLOCKS * 2);
    v.partial = c.take<double>(images * (size_t)pc_tiles(H, W) * 2);
    v.vals = c.take<double>(images * PERCEPTUAL_MAX_SCALES);
    const size_t h1 = (size_t)(H + 1) / 2, w1 = (size_t)(W + 1) / 2, h2 = (h1 + 1) / 2, w2 = (w1 + 1) / 2;
    const size_t odd = n_scales > 1 ? images * h1 * w1 : 0, even = n_scales > 2 ? images * h2 * w2 : 0;
    v.lx[1] = c.take<double>(odd);
    v.ly[1] = c.take<double>(odd);
    v.lx[0] = c.take<double>(even);
    v.ly[0] = c.take<double>(even);
    v.total = c.bytes();
    return v;
}

int perceptual_check(const char* who, int nimg, int H, int W, double sigma, double data_range, int n_scales) {
    INR_REQUIRE(nimg >= 1 && nimg <= 65535, INR_E_INVALID, "%s: 1 <= n_images <= 65535 (got %d)", who, nimg);
    INR_REQUIRE(H >= 1 && W >= 1, INR_E_INVALID, "%s: bad sizes (%d x %d)", who, H, W);
    INR_REQUIRE((long long)H * W < (1ll << 31), INR_E_INVALID, "%s: image too large (%d x %d)", who, H, W);
    PcTaps t;
    INR_REQUIRE(pc_taps(t, sigma), INR_E_INVALID, "%s: sigma must be positive with a window radius ceil(3 sigma) <= %d (got %g)", who,
                PC_RMAX, sigma);
    INR_REQUIRE(data_range > 0.0, INR_E_INVALID, "%s: data_range must be positive (got %g)", who, data_range);
    INR_REQUIRE(n_scales >= 1 && n_scales <= PERCEPTUAL_MAX_SCALES, INR_E_INVALID, "%s: 1 <= n_scales <= %d (got %d)", who,
                PERCEPTUAL_MAX_SCALES, n_scales);
    return 0;
}

// everything validated (perceptual_check) and the workspace checked by the caller
int launch_ssim_gauss(double* ssim, double* mean_cs, float* map, const float* x, const float* y, int nimg, int H, int W, double sigma,
                      double data_range, const PerceptualView& v, hipStream_t st) {
    PcTaps t;
    pc_taps(t, sigma);
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    ProfScope ps(KC_OTHER, st);
    return pc_ssim_level<float>(ssim, mean_cs, map, x, y, nimg, H, W, t, c1, c2, v.partial, st);
}

int launch_msssim(double* out, double* per_scale, const float* x, const float* y, int nimg, int H, int W, const double* weights,
                  int n_scales, double sigma, double data_range, const PerceptualView& v, hipStream_t st) {
    PcTaps t;
    pc_taps(t, sigma);
    PcWeights wt;
    wt.n = n_scales;
    for (int s = 0; s < PERCEPTUAL_MAX_SCALES; ++s) wt.w[s] = s < n_scales ? weights[s] : 0.0;
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    ProfScope ps(KC_OTHER, st);
    int h = H, w = W;
    for (int s = 0; s < n_scales; ++s) {
        const bool last = s == n_scales - 1;
        double* val = v.vals + (size_t)s * nimg;
        double* lcs = last ? val : nullptr;
        double* cs = last ? nullptr : val;
        if (s == 0) {
            if (int rc = pc_ssim_level<float>(lcs, cs, nullptr, x, y, nimg, h, w, t, c1, c2, v.partial, st)) return rc;
            continue;
        }
        const int oh = (h + 1) / 2, ow = (w + 1) / 2;
        const long long total = (long long)nimg * oh * ow;
        double *dx = v.lx[s & 1], *dy = v.ly[s & 1];
        if (s == 1) {
            hipLaunchKernelGGL(pc_down2_kernel<float>, dim3(pc_blocks(total)), dim3(256), 0, st, dx, x, total, h, w);
            INR_LAUNCH_CHECK();
            hipLaunchKernelGGL(pc_down2_kernel<float>, dim3(pc_blocks(total)), dim3(256), 0, st, dy, y, total, h, w);
            INR_LAUNCH_CHECK();
        } else {
            hipLaunchKernelGGL(pc_down2_kernel<double>, dim3(pc_blocks(total)), dim3(256), 0, st, dx, (const double*)v.lx[(s - 1) & 1],
                               total, h, w);
            INR_LAUNCH_CHECK();
            hipLaunchKernelGGL(pc_down2_kernel<double>, dim3(pc_blocks(total)), dim3(256), 0, st, dy, (const double*)v.ly[(s - 1) & 1],
                               total, h, w);
            INR_LAUNCH_CHECK();
        }
        h = oh;
        w = ow;
        if (int rc = pc_ssim_level<double>(lcs, cs, nullptr, (const double*)dx, (const double*)dy, nimg, h, w, t, c1, c2, v.partial, st))
            return rc;
    }
    hipLaunchKernelGGL(pc_msssim_finish_kernel, dim3((nimg + 63) / 64), dim3(64), 0, st, out, per_scale, (const double*)v.vals, wt, nimg);
    INR_LAUNCH_CHECK();
    return 0;
}

int launch_filter3x3(float* out, const float* in, int nimg, int H, int W, const double* k9, hipStream_t st) {
    PcK9 k;
    for (int i = 0; i < 9; ++i) k.k[i] = k9[i];
    const long long total = (long long)nimg * H * W;
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL(pc_filter3x3_kernel, dim3(pc_blocks(total)), dim3(256), 0, st, out, in, total, H, W, k);
    INR_LAUNCH_CHECK();
    return 0;
}

// mode 0: out[b] = mean (x - y)^2; mode 1: out[b] = sum max(x - y, 0)^2 / sum y^2
int launch_pair_score(double* out, const float* x, const float* y, int nimg, int64_t per_image, int mode, const PerceptualView& v,
                      hipStream_t st) {
    ProfScope ps(KC_OTHER, st);
    if (mode == 0)
        hipLaunchKernelGGL(pc_pair_sums_kernel<0>, dim3(PC_RED_BLOCKS, (unsigned)nimg), dim3(256), 0, st, v.reduce, x, y, per_image);
    else
        hipLaunchKernelGGL(pc_pair_sums_kernel<1>, dim3(PC_RED_BLOCKS, (unsigned)nimg), dim3(256), 0, st, v.reduce, x, y, per_image);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(pc_finish_kernel, dim3((nimg + 63) / 64), dim3(64), 0, st, out, (double*)nullptr, (const double*)v.reduce,
                       PC_RED_BLOCKS, (double)per_image, 1.0, mode, nimg);
    INR_LAUNCH_CHECK();
    return 0;
}

int pair_score(const char* who, double* out, const float* x, const float* y, int n_images, int64_t per_image, int mode,
               double* workspace, int64_t workspace_doubles, void* stream) {
    INR_REQUIRE(out && x && y, INR_E_INVALID, "%s: null pointer", who);
    INR_REQUIRE(n_images >= 1 && n_images <= 65535 && per_image >= 1, INR_E_INVALID, "%s: bad sizes (n_images=%d, per_image=%lld)", who,
                n_images, (long long)per_image);
    const PerceptualView v = perceptual_view(n_images, 1, 1, 1, workspace);
    if (int rc = check_ws_doubles(who, workspace, workspace_doubles, v.total)) return rc;
    INR_REQUIRE(aligned16(out) && aligned16(x) && aligned16(y), INR_E_ALIGN, "%s: pointers must be 16-byte aligned", who);
    return launch_pair_score(out, x, y, n_images, per_image, mode, v, (hipStream_t)stream);
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_perceptual_workspace_doubles(int n_images, int height, int width, int n_scales) {
    if (perceptual_check("inr_perceptual_workspace_doubles", n_images, height, width, 1.5, 1.0, n_scales)) return 0;
    return (int64_t)(perceptual_view(n_images, height, width, n_scales, nullptr).total / sizeof(double));
}

int inr_ssim2d_gauss(double* ssim, double* mean_cs, float* map, const float* x, const float* y, int n_images, int height, int width,
                     double sigma, double data_range, double* workspace, int64_t workspace_doubles, void* stream) {
    INR_REQUIRE(ssim && x && y, INR_E_INVALID, "inr_ssim2d_gauss: null pointer");
    if (int rc = perceptual_check("inr_ssim2d_gauss", n_images, height, width, sigma, data_range, 1)) return rc;
    const PerceptualView v = perceptual_view(n_images, height, width, 1, workspace);
    if (int rc = check_ws_doubles("inr_ssim2d_gauss", workspace, workspace_doubles, v.total)) return rc;
    INR_REQUIRE(aligned16(ssim) && aligned16(mean_cs) && aligned16(map) && aligned16(x) && aligned16(y), INR_E_ALIGN,
                "inr_ssim2d_gauss: pointers must be 16-byte aligned");
    return launch_ssim_gauss(ssim, mean_cs, map, x, y, n_images, height, width, sigma, data_range, v, (hipStream_t)stream);
}

int inr_msssim2d(double* out, double* per_scale, const float* x, const float* y, int n_images, int height, int width,
                 const double* weights, int n_scales, double sigma, double data_range, double* workspace, int64_t workspace_doubles,
                 void* stream) {
    INR_REQUIRE(out && x && y && weights, INR_E_INVALID, "inr_msssim2d: null pointer");
    if (int rc = perceptual_check("inr_msssim2d", n_images, height, width, sigma, data_range, n_scales)) return rc;
    const PerceptualView v = perceptual_view(n_images, height, width, n_scales, workspace);
    if (int rc = check_ws_doubles("inr_msssim2d", workspace, workspace_doubles, v.total)) return rc;
    INR_REQUIRE(aligned16(out) && aligned16(per_scale) && aligned16(x) && aligned16(y), INR_E_ALIGN,
                "inr_msssim2d: pointers must be 16-byte aligned");
    return launch_msssim(out, per_scale, x, y, n_images, height, width, weights, n_scales, sigma, data_range, v, (hipStream_t)stream);
}

int inr_filter3x3(float* out, const float* in, int n_images, int height, int width, const double* k9, void* stream) {
    INR_REQUIRE(out && in && k9, INR_E_INVALID, "inr_filter3x3: null pointer");
    if (int rc = perceptual_check("inr_filter3x3", n_images, height, width, 1.5, 1.0, 1)) return rc;
    INR_REQUIRE(aligned16(out) && aligned16(in), INR_E_ALIGN, "inr_filter3x3: pointers must be 16-byte aligned");
    return launch_filter3x3(out, in, n_images, height, width, k9, (hipStream_t)stream);
}

int inr_image_mse(double* out, const float* x, const float* y, int n_images, int64_t per_image, double* workspace,
                  int64_t workspace_doubles, void* stream) {
    return pair_score("inr_image_mse", out, x, y, n_images, per_image, 0, workspace, workspace_doubles, stream);
}

int inr_hf_gain(double* out, const float* h_sr, const float* h_inter, int n_images, int64_t per_image, double* workspace,
                int64_t workspace_doubles, void* stream) {
    return pair_score("inr_hf_gain", out, h_sr, h_inter, n_images, per_image, 1, workspace, workspace_doubles, stream);
}

}  // extern "C"
