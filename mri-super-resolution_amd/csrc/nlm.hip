// Non-local means on volumes and non-local MRI upsampling (include/inrhip.h: inr_nlm3d, inr_nlm_upsample).  Buades et
// al. 2005 in its MRI form -- Rician bias correction (Wiest-Daessle 2008, Manjon 2008), a per-voxel strength -- and the upsampling of
// Manjon et al., Medical Image Analysis 2010: NLM passes at falling strengths, each followed by the mean correction that restores
// A x = lr under the block operator of tvsr3d.hip.  tests/nlm_common.py restates all of it in float64 numpy.
//
// nlm_kernel: ONE launch per call over n_groups x tiles, a capped grid with a stride loop.  A workgroup of 256 threads owns a tile of 256
// output voxels, one per thread: 4 x 8 x 8, or 1 x 16 x 16 where axis 0 takes no part (s0 + r0 == 0: images, slice-wise filtering) --
// nlm_tile, the one rule.  It stages the guide over the tile plus a halo of s + r in LDS.  Per offset t of the search box, ascending
// (t0, t1, t2), it writes the field (G[u] - G[u + t])^2 over the tile plus a halo of r -- exactly 0 where u or u + t lies outside the
// volume -- and sums it along axis 2, axis 1 (in LDS) and axis 0 (in the owner's registers): 3 (2r + 1) adds per voxel and offset
// against (2r + 1)^3.  Because an outside sample contributes an exact 0 and the count n is the product of three per-axis counts, the
// separable sum is the definition's patch distance at the borders too.  sum w V_c (C <= 16), sum w and wmax stay in the owner's
// registers over all offsets; the value volumes are read from global memory at p + t.  An offset that moves the whole tile out of the
// volume is skipped by the whole workgroup.  No index depends on a data value.  LDS at the largest radii (s = 5, r = 2, tile 4 x 8 x 8):
// guide 18 x 22 x 22, field 8 x 12 x 12, axis-2 sums 8 x 12 x 8 doubles = 85,056 bytes; at the defaults (s = 3, r = 1) 33,216 bytes.
//
// The mean correction runs a thread per LR voxel: the block residual in the order and with the roundings of tv3_apply_kernel (no
// contraction), the f0 f1 f2 HR voxels x' - relax * res, and the block's sum of |x_new - x_old| as that LR voxel's partial; one
// workgroup per volume then adds the partials in a fixed order.  No atomics, no host read; the bits depend on the shapes alone.
#include "tv_shared.h"

namespace inr {
namespace {

constexpr int NLM_THREADS = 256;
constexpr int NLM_MAX_SEARCH = INR_NLM_MAX_SEARCH, NLM_MAX_PATCH = INR_NLM_MAX_PATCH, NLM_MAX_CHANNELS = INR_NLM_MAX_CHANNELS;
constexpr int NLM_MAX_FACTOR = INR_TVSR_MAX_FACTOR;
constexpr int NLM_MAX_PASSES = INR_NLM_MAX_PASSES;
constexpr int NLM_FE = 5;   // field samples per thread, at most: 8 x 12 x 12 / 256
constexpr int NLM_F2 = 3;   // axis-2 sums per thread, at most: 8 x 12 x 8 / 256
constexpr int NLM_F1 = 2;   // axis-1 sums per thread, at most: 8 x 8 x 8 / 256

struct NlmShape {
    int D, H, W, C;
    int s[3], r[3];
    int T[3];    // the tile
    int nt[3];   // tiles per axis
    int g[3];    // the staged guide: T + 2 (s + r)
    int e[3];    // the field: T + 2 r
    int center, rician;
    long long tiles;   // per group
};

// the one rule: the tile of the radii
void nlm_tile(const int* s, const int* r, int* T) {
    if (s[0] + r[0] == 0)
        T[0] = 1, T[1] = 16, T[2] = 16;
    else
        T[0] = 4, T[1] = 8, T[2] = 8;
}
size_t nlm_lds_bytes(const NlmShape& s) {
    return sizeof(double) * ((size_t)s.g[0] * s.g[1] * s.g[2] + (size_t)s.e[0] * s.e[1] * s.e[2] + (size_t)s.e[0] * s.e[1] * s.T[2]);
}

// how many patch offsets d in -r .. r keep both p + d and p + t + d inside 0 .. n - 1 (p and p + t are inside)
__device__ __forceinline__ int nlm_count(int p, int t, int r, int n) {
    const int lo = max(-r, max(-p, -p - t)), hi = min(r, min(n - 1 - p, n - 1 - p - t));
    return hi - lo + 1;
}

// out [G][C][D][H][W] from x [G][C][D][H][W] under guide [G][D][H][W]; h2map / sigma2 [G][D][H][W] or null, mask [G][D][H][W] or null
template <typename TX, typename TG, typename TO, int CMAX>
__global__ void __launch_bounds__(NLM_THREADS) nlm_kernel(TO* __restrict__ out, const TX* __restrict__ x, const TG* __restrict__ guide,
                                                          double h2s, const TX* __restrict__ h2map, const TX* __restrict__ sigma2,
                                                          const uint8_t* __restrict__ mask, long long G, NlmShape s) {
    extern __shared__ double nlm_lds[];
    double* gt = nlm_lds;                                // [g0][g1][g2]
    double* fa = gt + s.g[0] * s.g[1] * s.g[2];          // the field [e0][e1][e2], then the axis-1 sums [e0][T1][T2]
    double* fb = fa + s.e[0] * s.e[1] * s.e[2];          // the axis-2 sums [e0][e1][T2]
    const int tid = threadIdx.x;
    const long long HW = (long long)s.H * s.W, DHW = HW * s.D, items = G * s.tiles;
    const int N[3] = {s.D, s.H, s.W};
    const int nE = s.e[0] * s.e[1] * s.e[2], nF2 = s.e[0] * s.e[1] * s.T[2], nF1 = s.e[0] * s.T[1] * s.T[2];
    const int ghalo[3] = {s.s[0] + s.r[0], s.s[1] + s.r[1], s.s[2] + s.r[2]};

    // what does not depend on the tile: this thread's voxel of the tile and its samples of the three stages
    const int pc = tid % s.T[2], pb = (tid / s.T[2]) % s.T[1], pa = tid / (s.T[2] * s.T[1]);
    const int own_src = (pa * s.T[1] + pb) * s.T[2] + pc, own_stride = s.T[1] * s.T[2];
    int fe_i[NLM_FE], fe_g[NLM_FE];      // packed (i0, i1, i2) of the field sample and its place in the staged guide; -1: none
#pragma unroll
    for (int m = 0; m < NLM_FE; ++m) {
        const int idx = tid + NLM_THREADS * m;
        fe_i[m] = -1, fe_g[m] = 0;
        if (idx < nE) {
            const int i0 = idx / (s.e[1] * s.e[2]), rem = idx - i0 * (s.e[1] * s.e[2]), i1 = rem / s.e[2], i2 = rem - i1 * s.e[2];
            fe_i[m] = i0 | (i1 << 8) | (i2 << 16);
            fe_g[m] = ((i0 + s.s[0]) * s.g[1] + (i1 + s.s[1])) * s.g[2] + (i2 + s.s[2]);
        }
    }
    int f2_src[NLM_F2];                  // first field sample of the axis-2 sum idx = tid + 256 m; -1: none
#pragma unroll
    for (int m = 0; m < NLM_F2; ++m) {
        const int idx = tid + NLM_THREADS * m;
        f2_src[m] = -1;
        if (idx < nF2) {
            const int row = idx / s.T[2], c = idx - row * s.T[2];
            f2_src[m] = row * s.e[2] + c;
        }
    }
    int f1_src[NLM_F1];                  // first axis-2 sum of the axis-1 sum idx = tid + 256 m; -1: none
#pragma unroll
    for (int m = 0; m < NLM_F1; ++m) {
        const int idx = tid + NLM_THREADS * m;
        f1_src[m] = -1;
        if (idx < nF1) {
            const int i0 = idx / own_stride, rem = idx - i0 * own_stride, b = rem / s.T[2], c = rem - b * s.T[2];
            f1_src[m] = (i0 * s.e[1] + b) * s.T[2] + c;
        }
    }

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long grp = item / s.tiles;
        const int tile = (int)(item - grp * s.tiles);
        const int ti0 = tile / (s.nt[1] * s.nt[2]), trem = tile - ti0 * (s.nt[1] * s.nt[2]), ti1 = trem / s.nt[2], ti2 = trem - ti1 * s.nt[2];
        const int o[3] = {ti0 * s.T[0], ti1 * s.T[1], ti2 * s.T[2]};
        const TG* gv = guide + grp * DHW;
        __syncthreads();   // the previous item is done with the staged guide and the sums
        for (int idx = tid; idx < s.g[0] * s.g[1] * s.g[2]; idx += NLM_THREADS) {
            const int j0 = idx / (s.g[1] * s.g[2]), rem = idx - j0 * (s.g[1] * s.g[2]), j1 = rem / s.g[2], j2 = rem - j1 * s.g[2];
            const int v0 = o[0] - ghalo[0] + j0, v1 = o[1] - ghalo[1] + j1, v2 = o[2] - ghalo[2] + j2;
            const bool in = (unsigned)v0 < (unsigned)N[0] && (unsigned)v1 < (unsigned)N[1] && (unsigned)v2 < (unsigned)N[2];
            gt[idx] = in ? (double)gv[((long long)v0 * s.H + v1) * s.W + v2] : 0.0;
        }
        // this thread's voxel
        const int p0 = o[0] + pa, p1 = o[1] + pb, p2 = o[2] + pc;
        const bool inside = p0 < N[0] && p1 < N[1] && p2 < N[2];
        const long long pl = inside ? ((long long)p0 * s.H + p1) * s.W + p2 : 0;
        double h2 = h2s;
        if (inside && h2map) h2 = (double)h2map[grp * DHW + pl];
        const bool filter = inside && h2 > 0.0 && (!mask || mask[grp * DHW + pl] != 0);
        if (!filter) h2 = 1.0;
        double acc[CMAX], sw = 0.0, wmax = 0.0;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) acc[c] = 0.0;
        const TX* xg = x + grp * s.C * DHW;

        for (int t0 = -s.s[0]; t0 <= s.s[0]; ++t0) {
            if (o[0] + t0 >= N[0] || o[0] + s.T[0] - 1 + t0 < 0) continue;     // the whole tile leaves the volume: uniform
            for (int t1 = -s.s[1]; t1 <= s.s[1]; ++t1) {
                if (o[1] + t1 >= N[1] || o[1] + s.T[1] - 1 + t1 < 0) continue;
                for (int t2 = -s.s[2]; t2 <= s.s[2]; ++t2) {
                    if (o[2] + t2 >= N[2] || o[2] + s.T[2] - 1 + t2 < 0) continue;
                    if (t0 == 0 && t1 == 0 && t2 == 0) continue;
                    const int gdelta = (t0 * s.g[1] + t1) * s.g[2] + t2;
                    __syncthreads();   // the staged guide is complete; the previous offset's sums are consumed
#pragma unroll
                    for (int m = 0; m < NLM_FE; ++m) {
                        if (fe_i[m] < 0) continue;
                        const int i0 = fe_i[m] & 255, i1 = (fe_i[m] >> 8) & 255, i2 = fe_i[m] >> 16;
                        const int u0 = o[0] - s.r[0] + i0, u1 = o[1] - s.r[1] + i1, u2 = o[2] - s.r[2] + i2;
                        const bool both = (unsigned)u0 < (unsigned)N[0] && (unsigned)u1 < (unsigned)N[1] && (unsigned)u2 < (unsigned)N[2] &&
                                          (unsigned)(u0 + t0) < (unsigned)N[0] && (unsigned)(u1 + t1) < (unsigned)N[1] &&
                                          (unsigned)(u2 + t2) < (unsigned)N[2];
                        const double d = gt[fe_g[m]] - gt[fe_g[m] + gdelta];
                        fa[tid + NLM_THREADS * m] = both ? d * d : 0.0;
                    }
                    __syncthreads();
#pragma unroll
                    for (int m = 0; m < NLM_F2; ++m) {
                        if (f2_src[m] < 0) continue;
                        double a = 0.0;
                        for (int d = 0; d <= 2 * s.r[2]; ++d) a += fa[f2_src[m] + d];
                        fb[tid + NLM_THREADS * m] = a;
                    }
                    __syncthreads();
#pragma unroll
                    for (int m = 0; m < NLM_F1; ++m) {
                        if (f1_src[m] < 0) continue;
                        double a = 0.0;
                        for (int d = 0; d <= 2 * s.r[1]; ++d) a += fb[f1_src[m] + d * s.T[2]];
                        fa[tid + NLM_THREADS * m] = a;
                    }
                    __syncthreads();
                    const int q0 = p0 + t0, q1 = p1 + t1, q2 = p2 + t2;
                    if (filter && (unsigned)q0 < (unsigned)N[0] && (unsigned)q1 < (unsigned)N[1] && (unsigned)q2 < (unsigned)N[2]) {
                        double a = 0.0;
                        for (int d = 0; d <= 2 * s.r[0]; ++d) a += fa[own_src + d * own_stride];
                        const int n = nlm_count(p0, t0, s.r[0], N[0]) * nlm_count(p1, t1, s.r[1], N[1]) * nlm_count(p2, t2, s.r[2], N[2]);
                        const double w = exp(-(a / (double)n) / h2);
                        const long long ql = ((long long)q0 * s.H + q1) * s.W + q2;
#pragma unroll
                        for (int c = 0; c < CMAX; ++c)
                            if (c < s.C) {
                                const double v = (double)xg[c * DHW + ql];
                                acc[c] += w * (s.rician ? v * v : v);
                            }
                        sw += w;
                        if (w > wmax) wmax = w;
                    }
                }
            }
        }
        if (!inside) continue;
        const double wc = s.center ? 1.0 : (wmax > 0.0 ? wmax : 1.0);
        const double two_s2 = (s.rician && filter) ? 2.0 * (double)sigma2[grp * DHW + pl] : 0.0;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < s.C) {
                const TX xv = xg[c * DHW + pl];
                const long long at = (grp * s.C + c) * DHW + pl;
                if (!filter) {
                    out[at] = (TO)xv;
                    continue;
                }
                const double v = (double)xv;
                double m = (acc[c] + wc * (s.rician ? v * v : v)) / (sw + wc);
                if (s.rician) {
                    m -= two_s2;
                    m = sqrt(m < 0.0 ? 0.0 : m);   // a NaN stays one
                }
                out[at] = (TO)m;
            }
    }
}

// ---- the mean correction of the upsampling -----------------------------------------------------------------------------------------------
struct NlmUpShape {
    int D, H, W, d, h, w, f0, f1, f2;
};
struct NlmBlockKernel {
    double k0[NLM_MAX_FACTOR], k1[NLM_MAX_FACTOR], k2[NLM_MAX_FACTOR];
};

// state = x0, or the block replication of y; `out` (nullable): the same, rounded once (a solve without passes)
template <typename T>
__global__ void __launch_bounds__(NLM_THREADS) nlm_up_init_kernel(double* __restrict__ state, T* __restrict__ out, const T* __restrict__ y,
                                                                  const T* __restrict__ x0, long long n, NlmUpShape s) {
    const long long HW = (long long)s.H * s.W, DHW = HW * s.D, dhw = (long long)s.d * s.h * s.w, total = n * DHW;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const long long img = t / DHW, e = t - img * DHW;
        const int z = (int)(e / HW), r = (int)(e - z * HW), i = r / s.W, j = r - i * s.W;
        const T v = x0 ? x0[t] : y[img * dhw + ((long long)(z / s.f0) * s.h + i / s.f1) * s.w + j / s.f2];
        state[t] = (double)v;
        if (out) out[t] = v;
    }
}

// x <- x' - relax * N(A x' - y), a thread per LR voxel; part [n][d][h][w]: the block's sum of |x_new - x_old|; `out` (nullable): x_new,
// rounded once
template <typename T>
__global__ void __launch_bounds__(NLM_THREADS) nlm_correct_kernel(double* __restrict__ x, T* __restrict__ out, double* __restrict__ part,
                                                                  const double* __restrict__ xp, const T* __restrict__ y, double relax,
                                                                  long long n, NlmUpShape s, NlmBlockKernel kb) {
#pragma clang fp contract(off)   // the residual and the update round as block_apply3d and two tensor operations do
    __shared__ double ks[NLM_MAX_FACTOR * NLM_MAX_FACTOR * NLM_MAX_FACTOR];
    for (int t = threadIdx.x; t < s.f0 * s.f1 * s.f2; t += blockDim.x) {
        const int a = t / (s.f1 * s.f2), r = t - a * (s.f1 * s.f2), b = r / s.f2, c = r - b * s.f2;
        ks[t] = (kb.k1[b] * kb.k2[c]) * kb.k0[a];
    }
    __syncthreads();
    const long long HW = (long long)s.H * s.W, DHW = HW * s.D, hw = (long long)s.h * s.w, dhw = hw * s.d, total = n * dhw;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const long long img = t / dhw, l = t - img * dhw;
        const int bd = (int)(l / hw), r = (int)(l - bd * hw), bi = r / s.w, bj = r - bi * s.w;
        const long long first = img * DHW + ((long long)(bd * s.f0) * s.H + bi * s.f1) * s.W + bj * s.f2;
        double acc = 0.0;
        for (int a = 0; a < s.f0; ++a)
            for (int b = 0; b < s.f1; ++b) {
                const double* row = xp + first + a * HW + (long long)b * s.W;
                const double* kr = ks + (a * s.f1 + b) * s.f2;
                for (int c = 0; c < s.f2; ++c) acc += kr[c] * row[c];
            }
        const double step = relax * (acc - (double)y[t]);
        double ch = 0.0;
        for (int a = 0; a < s.f0; ++a)
            for (int b = 0; b < s.f1; ++b) {
                const long long at = first + a * HW + (long long)b * s.W;
                for (int c = 0; c < s.f2; ++c) {
                    const double v = xp[at + c] - step;
                    ch += fabs(v - x[at + c]);
                    x[at + c] = v;
                    if (out) out[at + c] = (T)v;
                }
            }
        part[t] = ch;
    }
}

// change [n] = (sum of part [n][count]) / voxels: thread t adds the partials t, t + 256, ... in ascending order, thread 0 the 256 sums
__global__ void __launch_bounds__(NLM_THREADS) nlm_change_kernel(double* __restrict__ change, const double* __restrict__ part,
                                                                 long long count, double voxels, long long n) {
    __shared__ double red[NLM_THREADS];
    for (long long img = blockIdx.x; img < n; img += gridDim.x) {
        double a = 0.0;
        for (long long p = threadIdx.x; p < count; p += NLM_THREADS) a += part[img * count + p];
        red[threadIdx.x] = a;
        __syncthreads();
        if (threadIdx.x == 0) {
            double tot = 0.0;
            for (int i = 0; i < NLM_THREADS; ++i) tot += red[i];
            change[img] = tot / voxels;
        }
        __syncthreads();
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
int nlm_radii_check(const char* who, const int* s, const int* r) {
    for (int a = 0; a < 3; ++a) {
        INR_REQUIRE(s[a] >= 0 && s[a] <= NLM_MAX_SEARCH, INR_E_INVALID, "%s: search radii are 0 .. %d per axis (s%d is %d)", who,
                    NLM_MAX_SEARCH, a, s[a]);
        INR_REQUIRE(r[a] >= 0 && r[a] <= NLM_MAX_PATCH, INR_E_INVALID, "%s: patch radii are 0 .. %d per axis (r%d is %d)", who,
                    NLM_MAX_PATCH, a, r[a]);
    }
    return 0;
}
int nlm_volume_check(const char* who, int D, int H, int W) {
    INR_REQUIRE(D >= 1 && H >= 1 && W >= 1, INR_E_INVALID, "%s: bad sizes (volumes of at least 1 sample per axis, got %d x %d x %d)", who, D,
                H, W);
    INR_REQUIRE((long long)D * H < (1ll << 31) && (long long)D * H * W < (1ll << 31), INR_E_INVALID,
                "%s: a volume holds fewer than 2^31 voxels (got %d x %d x %d)", who, D, H, W);
    return 0;
}
int nlm_overlap_check(const char* who, const char* name, const void* out, size_t out_bytes, const void* in, size_t in_bytes) {
    const char *o = static_cast<const char*>(out), *i = static_cast<const char*>(in);
    INR_REQUIRE(o + out_bytes <= i || i + in_bytes <= o, INR_E_INVALID, "%s: out must not overlap %s", who, name);
    return 0;
}

NlmShape nlm_shape(int C, int D, int H, int W, const int* s, const int* r, int center, int rician) {
    NlmShape v{};
    v.D = D, v.H = H, v.W = W, v.C = C, v.center = center, v.rician = rician;
    nlm_tile(s, r, v.T);
    const int N[3] = {D, H, W};
    for (int a = 0; a < 3; ++a) {
        v.s[a] = s[a], v.r[a] = r[a];
        v.nt[a] = (N[a] + v.T[a] - 1) / v.T[a];
        v.g[a] = v.T[a] + 2 * (s[a] + r[a]);
        v.e[a] = v.T[a] + 2 * r[a];
    }
    v.tiles = (long long)v.nt[0] * v.nt[1] * v.nt[2];
    return v;
}

template <typename TX, typename TG, typename TO, int CMAX>
int nlm_launch_c(TO* out, const TX* x, const TG* guide, double h2, const TX* h2map, const TX* sigma2, const uint8_t* mask, long long G,
                 const NlmShape& s, hipStream_t st) {
    const size_t lds = nlm_lds_bytes(s);
    if (lds > 64 * 1024)
        INR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&nlm_kernel<TX, TG, TO, CMAX>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
    hipLaunchKernelGGL((nlm_kernel<TX, TG, TO, CMAX>), dim3(tv_grid(G * s.tiles)), dim3(NLM_THREADS), lds, st, out, x, guide, h2, h2map,
                       sigma2, mask, G, s);
    INR_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int nlm3d(const char* who, T* out, const T* x, const T* guide, double h2, const T* h2map, const T* sigma2, const uint8_t* mask, int G, int C,
          int D, int H, int W, int s0, int s1, int s2, int r0, int r1, int r2, int center, hipStream_t st) {
    INR_REQUIRE(out && x, INR_E_INVALID, "%s: null pointer (out and x are required)", who);
    INR_REQUIRE(G >= 0, INR_E_INVALID, "%s: bad sizes (n_groups = %d)", who, G);
    INR_REQUIRE(C >= 1 && C <= NLM_MAX_CHANNELS, INR_E_INVALID, "%s: channels must be 1 .. %d (got %d)", who, NLM_MAX_CHANNELS, C);
    INR_REQUIRE(guide || C == 1, INR_E_INVALID, "%s: a null guide needs channels == 1 (got %d): the guide is x itself", who, C);
    if (int rc = nlm_volume_check(who, D, H, W)) return rc;
    const int s[3] = {s0, s1, s2}, r[3] = {r0, r1, r2};
    if (int rc = nlm_radii_check(who, s, r)) return rc;
    INR_REQUIRE(center == INR_NLM_CENTER_MAX || center == INR_NLM_CENTER_ONE, INR_E_INVALID, "%s: center must be %d (max) or %d (one) (got %d)",
                who, INR_NLM_CENTER_MAX, INR_NLM_CENTER_ONE, center);
    if (!h2map) INR_REQUIRE(std::isfinite(h2) && h2 > 0.0, INR_E_INVALID, "%s: a scalar h2 must be finite and > 0 (got %g)", who, h2);
    const size_t vol = (size_t)D * H * W * sizeof(T);
    INR_REQUIRE((long long)G * C * ((long long)D * H * W) < (1ll << 40), INR_E_INVALID, "%s: the batch is too large", who);
    if (int rc = nlm_overlap_check(who, "x", out, vol * G * C, x, vol * G * C)) return rc;
    if (guide)
        if (int rc = nlm_overlap_check(who, "guide", out, vol * G * C, guide, vol * G)) return rc;
    if (G == 0) return 0;
    ProfScope ps(KC_OTHER, st);
    const NlmShape sh = nlm_shape(C, D, H, W, s, r, center, sigma2 != nullptr);
    const T* gd = guide ? guide : x;
    if (C == 1) return nlm_launch_c<T, T, T, 1>(out, x, gd, h2, h2map, sigma2, mask, G, sh, st);
    if (C <= 4) return nlm_launch_c<T, T, T, 4>(out, x, gd, h2, h2map, sigma2, mask, G, sh, st);
    return nlm_launch_c<T, T, T, NLM_MAX_CHANNELS>(out, x, gd, h2, h2map, sigma2, mask, G, sh, st);
}

int nlm_up_shape_check(const char* who, int n, int D, int H, int W, int f0, int f1, int f2, NlmUpShape* s) {
    INR_REQUIRE(n >= 0, INR_E_INVALID, "%s: bad sizes (n_volumes = %d)", who, n);
    INR_REQUIRE(f0 >= 1 && f0 <= NLM_MAX_FACTOR && f1 >= 1 && f1 <= NLM_MAX_FACTOR && f2 >= 1 && f2 <= NLM_MAX_FACTOR, INR_E_INVALID,
                "%s: block factors are 1 .. %d per axis (got %d x %d x %d)", who, NLM_MAX_FACTOR, f0, f1, f2);
    if (int rc = nlm_volume_check(who, D, H, W)) return rc;
    INR_REQUIRE(D % f0 == 0 && H % f1 == 0 && W % f2 == 0, INR_E_INVALID,
                "%s: the HR volume %d x %d x %d is no whole number of %d x %d x %d blocks", who, D, H, W, f0, f1, f2);
    INR_REQUIRE((long long)(n > 0 ? n : 1) * ((long long)D * H * W) < (1ll << 40), INR_E_INVALID, "%s: the batch is too large", who);
    *s = NlmUpShape{D, H, W, D / f0, H / f1, W / f2, f0, f1, f2};
    return 0;
}

// the caller's HOST factors k0 [f0], k1 [f1], k2 [f2]: finite, each summing to 1
int nlm_kernel_check(const char* who, const double* k0, const double* k1, const double* k2, const NlmUpShape& s, NlmBlockKernel* kb) {
    INR_REQUIRE(k0 && k1 && k2, INR_E_INVALID, "%s: null pointer (kernel factors)", who);
    const double* in[3] = {k0, k1, k2};
    double* out[3] = {kb->k0, kb->k1, kb->k2};
    const int f[3] = {s.f0, s.f1, s.f2};
    for (int axis = 0; axis < 3; ++axis) {
        double sum = 0.0;
        for (int t = 0; t < NLM_MAX_FACTOR; ++t) out[axis][t] = 0.0;
        for (int t = 0; t < f[axis]; ++t) {
            INR_REQUIRE(std::isfinite(in[axis][t]), INR_E_INVALID, "%s: the kernel factors must be finite (k%d[%d] is %g)", who, axis, t,
                        in[axis][t]);
            out[axis][t] = in[axis][t];
            sum += in[axis][t];
        }
        INR_REQUIRE(std::isfinite(sum) && std::fabs(sum - 1.0) <= 1e-9, INR_E_INVALID, "%s: every kernel factor must sum to 1 (k%d sums to %.17g)",
                    who, axis, sum);
    }
    return 0;
}

// the workspace: the state x and the filtered x' of every volume, then the partials of `change`.  base == null: `total` only
struct NlmUpView {
    double *x, *xp, *part;
    size_t total;
};
NlmUpView nlm_up_view(int n, const NlmUpShape& s, void* base) {
    NlmUpView v;
    WsCarver c(base, 16);
    const size_t nn = (size_t)(n > 0 ? n : 1);
    v.x = c.take<double>(nn * (size_t)s.D * (size_t)s.H * (size_t)s.W);
    v.xp = c.take<double>(nn * (size_t)s.D * (size_t)s.H * (size_t)s.W);
    v.part = c.take<double>(nn * (size_t)s.d * (size_t)s.h * (size_t)s.w);
    v.total = c.bytes();
    return v;
}

template <typename T>
int nlm_upsample(const char* who, T* out, double* change, const T* y, const T* x0, const T* guide, int n, int D, int H, int W, int f0, int f1,
                 int f2, const double* k0, const double* k1, const double* k2, const double* levels, int n_levels, int n_iter, double relax,
                 int s0, int s1, int s2, int r0, int r1, int r2, double* workspace, int64_t workspace_doubles, hipStream_t st) {
    INR_REQUIRE(out && y, INR_E_INVALID, "%s: null pointer (out and y are required)", who);
    NlmUpShape s;
    NlmBlockKernel kb;
    if (int rc = nlm_up_shape_check(who, n, D, H, W, f0, f1, f2, &s)) return rc;
    const int sr[3] = {s0, s1, s2}, pr[3] = {r0, r1, r2};
    if (int rc = nlm_radii_check(who, sr, pr)) return rc;
    if (int rc = nlm_kernel_check(who, k0, k1, k2, s, &kb)) return rc;
    INR_REQUIRE(n_levels >= 0 && n_iter >= 0 && (long long)n_levels * n_iter <= NLM_MAX_PASSES, INR_E_INVALID,
                "%s: levels * n_iter must be 0 .. %d (got %d levels, n_iter = %d)", who, NLM_MAX_PASSES, n_levels, n_iter);
    INR_REQUIRE(n_levels == 0 || levels, INR_E_INVALID, "%s: null pointer (levels)", who);
    for (int l = 0; l < n_levels; ++l)
        INR_REQUIRE(std::isfinite(levels[l]) && levels[l] > 0.0 && std::isfinite(levels[l] * levels[l]) && levels[l] * levels[l] > 0.0,
                    INR_E_INVALID, "%s: every level must be finite and > 0, and so its square (levels[%d] is %g)", who, l, levels[l]);
    INR_REQUIRE(relax > 0.0 && relax <= 1.0, INR_E_INVALID, "%s: relax must lie in (0, 1] (got %g)", who, relax);
    if (int rc = check_ws_doubles(who, workspace, workspace_doubles, nlm_up_view(n, s, nullptr).total)) return rc;
    if (n == 0) return 0;
    ProfScope ps(KC_OTHER, st);
    const NlmUpView v = nlm_up_view(n, s, workspace);
    const long long voxels = (long long)D * H * W, blocks = (long long)s.d * s.h * s.w;
    const int passes = n_levels * n_iter;
    hipLaunchKernelGGL((nlm_up_init_kernel<T>), dim3(tv_thread_grid(n * voxels, NLM_THREADS)), dim3(NLM_THREADS), 0, st, v.x,
                       passes == 0 ? out : (T*)nullptr, y, x0, (long long)n, s);
    INR_LAUNCH_CHECK();
    const NlmShape sh = nlm_shape(1, D, H, W, sr, pr, INR_NLM_CENTER_ONE, 0);
    for (int pass = 0; pass < passes; ++pass) {
        const double h = levels[pass / n_iter], h2 = h * h;
        if (guide) {
            if (int rc = nlm_launch_c<double, T, double, 1>(v.xp, v.x, guide, h2, nullptr, nullptr, nullptr, n, sh, st)) return rc;
        } else if (int rc = nlm_launch_c<double, double, double, 1>(v.xp, v.x, v.x, h2, nullptr, nullptr, nullptr, n, sh, st))
            return rc;
        hipLaunchKernelGGL((nlm_correct_kernel<T>), dim3(tv_thread_grid(n * blocks, NLM_THREADS)), dim3(NLM_THREADS), 0, st, v.x,
                           pass + 1 == passes ? out : (T*)nullptr, v.part, v.xp, y, relax, (long long)n, s, kb);
        INR_LAUNCH_CHECK();
        if (change) {
            hipLaunchKernelGGL(nlm_change_kernel, dim3(tv_grid(n)), dim3(NLM_THREADS), 0, st, change + (long long)pass * n, v.part, blocks,
                               (double)voxels, (long long)n);
            INR_LAUNCH_CHECK();
        }
    }
    return 0;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int inr_nlm3d(double* out, const double* x, const double* guide, double h2, const double* h2_map, const double* sigma2, const uint8_t* mask,
              int n_groups, int channels, int depth, int height, int width, int s0, int s1, int s2, int r0, int r1, int r2, int center,
              void* stream) {
    return nlm3d("inr_nlm3d", out, x, guide, h2, h2_map, sigma2, mask, n_groups, channels, depth, height, width, s0, s1, s2, r0, r1, r2, center,
                 (hipStream_t)stream);
}

int inr_nlm3d_f32(float* out, const float* x, const float* guide, double h2, const float* h2_map, const float* sigma2, const uint8_t* mask,
                  int n_groups, int channels, int depth, int height, int width, int s0, int s1, int s2, int r0, int r1, int r2, int center,
                  void* stream) {
    return nlm3d("inr_nlm3d_f32", out, x, guide, h2, h2_map, sigma2, mask, n_groups, channels, depth, height, width, s0, s1, s2, r0, r1, r2,
                 center, (hipStream_t)stream);
}

int64_t inr_nlm_upsample_workspace_doubles(int n_volumes, int depth, int height, int width, int f0, int f1, int f2) {
    NlmUpShape s;
    if (nlm_up_shape_check("inr_nlm_upsample_workspace_doubles", n_volumes, depth, height, width, f0, f1, f2, &s)) return 0;
    return (int64_t)(nlm_up_view(n_volumes, s, nullptr).total / sizeof(double));
}

int inr_nlm_upsample(double* out, double* change, const double* y, const double* x0, const double* guide, int n_volumes, int depth, int height,
                     int width, int f0, int f1, int f2, const double* k0, const double* k1, const double* k2, const double* levels,
                     int n_levels, int n_iter, double relax, int s0, int s1, int s2, int r0, int r1, int r2, double* workspace,
                     int64_t workspace_doubles, void* stream) {
    return nlm_upsample("inr_nlm_upsample", out, change, y, x0, guide, n_volumes, depth, height, width, f0, f1, f2, k0, k1, k2, levels, n_levels,
                        n_iter, relax, s0, s1, s2, r0, r1, r2, workspace, workspace_doubles, (hipStream_t)stream);
}

int inr_nlm_upsample_f32(float* out, double* change, const float* y, const float* x0, const float* guide, int n_volumes, int depth, int height,
                         int width, int f0, int f1, int f2, const double* k0, const double* k1, const double* k2, const double* levels,
                         int n_levels, int n_iter, double relax, int s0, int s1, int s2, int r0, int r1, int r2, double* workspace,
                         int64_t workspace_doubles, void* stream) {
    return nlm_upsample("inr_nlm_upsample_f32", out, change, y, x0, guide, n_volumes, depth, height, width, f0, f1, f2, k0, k1, k2, levels,
                        n_levels, n_iter, relax, s0, s1, s2, r0, r1, r2, workspace, workspace_doubles, (hipStream_t)stream);
}

}  // extern "C"
