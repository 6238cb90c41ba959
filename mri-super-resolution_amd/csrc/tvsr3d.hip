// The model-based TV / Huber super-resolution of tvsr.hip on VOLUMES, with a slice profile in the operator and one volume spread over
// many workgroups:
//   x* = argmin_x 1/2 sum_i w_i ((A x)_i - y_i)^2 + lambda sum_j H_alpha(sqrt((g1 d1 x)_j^2 + (g2 d2 x)_j^2 + (g0 d0 x)_j^2))
// Volumes are HR [n][D][H][W] and LR [n][d][h][w], D = f0 d, H = f1 h, W = f2 w.  A: every LR voxel is the k-weighted sum of its
// f0 x f1 x f2 block, k[a][b][c] = (k1[b] * k2[c]) * k0[a] -- k0 [f0] the slice profile, k1 / k2 the in-plane factors, each summing to
// 1 --, the terms added in ascending (a, b, c); A A^T = |k|^2 I (|k|^2 summed over the formed table in memory order), so the proximal
// map of the data term is closed-form per block.  d0 / d1 / d2: forward differences along slice / row / column with a zero last
// plane / row / column, each scaled by its weight g_a >= 0 (the voxel spacing: g0 = in-plane spacing / slice spacing); div = -grad^T.
// Chambolle-Pock exactly as tvsr.hip states it, from x = xbar = x0, p = 0, with tau = sigma = 1 / sqrt(4 sum g_a^2), the sum in the
// order (1, 2, 0) over the axes whose HR extent exceeds 1 (sum = 0: the prior vanishes, lambda = 0 and tau = 1 / sqrt(8)).
//
// THE ORDER OF OPERATIONS IS PART OF THE CONTRACT.  Wherever tvsr.hip combines its two axes, this unit combines row, column, then
// slice, the slice term last: div = + g1 p1[e] - g1 p1[e - W] + g2 p2[e] - g2 p2[e - 1], then + g0 p0[e] - g0 p0[e - HW]; the norm is
// sqrt((q1^2 + q2^2) + q0^2).  With D = 1 or g0 = 0 (and g1 = g2 = 1) the slice terms are exact zeros and the solve is the 2-D solve of
// every slice, bit for bit (the unit is compiled with -ffp-contract=off, like tvsr.hip).
//
// LAUNCHES.  Plain launches on the caller's stream: no cooperative launch, no grid barrier, no spin, no host read.
//   init    (thread per HR voxel):   writes its own x, xbar, p0, p1, p2;
//   dual    (thread per HR voxel e): reads xbar[e], xbar[e + 1], xbar[e + W], xbar[e + HW] -- neighbours' --, reads and writes
//                                    p0[e], p1[e], p2[e] -- its own;
//   primal  (workgroup per tile of whole LR blocks): reads p at its voxels and their upper / left / previous-slice neighbours --
//                                    other tiles' --, forms v = x + tau div p per voxel with coalesced loads and keeps v in LDS, takes
//                                    the block sums from LDS in ascending (a, b, c), writes x and xbar of ITS tile only;
//   final   (workgroup per tile):    reads x (its tile's, and the neighbours' for the prior), writes the result and the partials of
//                                    the objective; finish: one workgroup per volume adds / maximises the partials in a fixed order.
// Within a launch a field is either read across threads or written by its owner alone: xbar is read-only in the dual kernel and
// owner-written in the primal one, p is owner-written in the dual kernel and read-only in the primal one, x is touched by its
// tile's workgroup only.  STREAM ORDER IS THE BARRIER between launches (a kernel's stores are visible to the next kernel of the
// stream); inside the primal and final kernels __syncthreads() orders the LDS tile.
//
// A volume's tiles are dealt to at most TV3_PARTS "parts" (part j owns tiles j, j + parts, ...), and a workgroup takes whole parts
// in a grid-stride loop.  The partials of energy and change are per PART, not per workgroup, so their bits depend on the shape
// alone: not on the grid (capped at TV_STRIDE_MAX_GRID, or by the test-only inr_debug_set(32, .)), the stream, or the place in a batch.
// No float atomics.  All arithmetic is fp64; the fp32 entry converts at load and rounds once at the store.
//
// The Huber function, the grids, the refusals of the scalar parameters, the step setup and the finish kernel are tv_shared.h's.
#include "tv_shared.h"

namespace inr {
namespace {

constexpr int TV3_THREADS = 256;
constexpr int TV3_MAX_FACTOR = INR_TVSR_MAX_FACTOR;
constexpr int TV3_MAX_SIDE = INR_TVSR_MAX_SIDE;
constexpr int TV3_PARTS = 1024;                 // parts per volume, at most
constexpr int TV3_TILE = 2048;                  // HR voxels of a tile, at most (16 KiB of LDS for v, 16 KiB for the blocks' residuals)
constexpr int TV3_TILE_COLS = 64;               // HR columns of a tile, at most
constexpr int TV3_TABLE = TV3_MAX_FACTOR * TV3_MAX_FACTOR * TV3_MAX_FACTOR;

// the three 1-D factors of the block kernel, by value in the kernel arguments (the [8][8][8] table would not fit them)
struct Tv3Kernel {
    double k0[TV3_MAX_FACTOR], k1[TV3_MAX_FACTOR], k2[TV3_MAX_FACTOR];
    double ksq;   // sum k^2 over the formed table
};

struct Tv3Shape {
    int D, H, W, d, h, w, f0, f1, f2;
    int th, tw;             // LR rows / columns of a full tile (one LR slice deep)
    int tiles_h, tiles_w;   // tiles per LR slice
    int tiles;              // per volume: d * tiles_h * tiles_w
    int parts;              // min(tiles, TV3_PARTS)
};

struct Tv3Step {
    double g0, g1, g2, tau, lam, alpha;   // lam: 0 where the prior vanishes
};

// k[a][b][c] = (k1[b] * k2[c]) * k0[a] into ks [f0][f1][f2]; the caller synchronises
__device__ __forceinline__ void tv3_form_table(double* ks, const Tv3Kernel& kb, const Tv3Shape& s) {
    for (int t = threadIdx.x; t < s.f0 * s.f1 * s.f2; t += blockDim.x) {
        const int a = t / (s.f1 * s.f2), r = t - a * (s.f1 * s.f2), b = r / s.f2, c = r - b * s.f2;
        ks[t] = (kb.k1[b] * kb.k2[c]) * kb.k0[a];
    }
}

// one tile of one volume: LR slice bd, LR rows bh0 .. bh0 + nh, LR columns bw0 .. bw0 + nw; RH x CW HR samples per slice of the tile
struct Tv3Tile {
    int bd, bh0, bw0, nh, nw, RH, CW, vox, blocks;
};
__device__ __forceinline__ Tv3Tile tv3_tile(const Tv3Shape& s, int tile) {
    Tv3Tile t;
    const int per_slice = s.tiles_h * s.tiles_w;
    t.bd = tile / per_slice;
    const int r = tile - t.bd * per_slice, ti = r / s.tiles_w, tj = r - ti * s.tiles_w;
    t.bh0 = ti * s.th;
    t.bw0 = tj * s.tw;
    t.nh = min(s.th, s.h - t.bh0);
    t.nw = min(s.tw, s.w - t.bw0);
    t.RH = t.nh * s.f1;
    t.CW = t.nw * s.f2;
    t.vox = s.f0 * t.RH * t.CW;
    t.blocks = t.nh * t.nw;
    return t;
}

// voxel idx of a tile ([f0][RH][CW], columns fastest: consecutive threads on consecutive addresses) -> its HR coordinates
struct Tv3Voxel {
    int a, z, i, j;
    long long e;   // within the volume
};
__device__ __forceinline__ Tv3Voxel tv3_voxel(const Tv3Shape& s, const Tv3Tile& t, int idx) {
    Tv3Voxel v;
    const int plane = t.RH * t.CW;
    v.a = idx / plane;
    const int r = idx - v.a * plane, rr = r / t.CW, cc = r - rr * t.CW;
    v.z = t.bd * s.f0 + v.a;
    v.i = t.bh0 * s.f1 + rr;
    v.j = t.bw0 * s.f2 + cc;
    v.e = ((long long)v.z * s.H + v.i) * s.W + v.j;
    return v;
}

// (A v) of block b of the tile from its LDS image vt [f0][RH][CW]: the terms in ascending (a, b, c)
__device__ __forceinline__ double tv3_tile_block_sum(const double* vt, const double* ks, const Tv3Shape& s, const Tv3Tile& t, int b) {
    const int bi = b / t.nw, bj = b - bi * t.nw;
    double acc = 0.0;
    for (int a = 0; a < s.f0; ++a)
        for (int bb = 0; bb < s.f1; ++bb) {
            const double* row = vt + (a * t.RH + bi * s.f1 + bb) * t.CW + bj * s.f2;
            const double* kr = ks + (a * s.f1 + bb) * s.f2;
            for (int c = 0; c < s.f2; ++c) acc += kr[c] * row[c];
        }
    return acc;
}
__device__ __forceinline__ long long tv3_lr_index(const Tv3Shape& s, const Tv3Tile& t, int b) {
    const int bi = b / t.nw, bj = b - bi * t.nw;
    return ((long long)t.bd * s.h + (t.bh0 + bi)) * s.w + (t.bw0 + bj);
}

// the state of volume img: x | xbar | p0 | p1 | p2
struct Tv3State {
    double *x, *xbar, *p0, *p1, *p2;
};
__device__ __forceinline__ Tv3State tv3_state(double* state, long long img, long long DHW) {
    Tv3State v;
    v.x = state + img * 5 * DHW;
    v.xbar = v.x + DHW;
    v.p0 = v.xbar + DHW;
    v.p1 = v.p0 + DHW;
    v.p2 = v.p1 + DHW;
    return v;
}

template <typename T>
__global__ void __launch_bounds__(TV3_THREADS) tv3_init_kernel(double* state, const T* y, const T* x0, long long n, Tv3Shape s) {
    const long long HW = (long long)s.H * s.W, DHW = HW * s.D, dhw = (long long)s.d * s.h * s.w, total = n * DHW;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const long long img = t / DHW, e = t - img * DHW;
        double v;
        if (x0) {
            v = (double)x0[t];
        } else {
            const int z = (int)(e / HW), r = (int)(e - z * HW), i = r / s.W, j = r - i * s.W;
            v = (double)y[img * dhw + ((long long)(z / s.f0) * s.h + i / s.f1) * s.w + j / s.f2];
        }
        const Tv3State st = tv3_state(state, img, DHW);
        st.x[e] = v;
        st.xbar[e] = v;
        st.p0[e] = 0.0;
        st.p1[e] = 0.0;
        st.p2[e] = 0.0;
    }
}

__global__ void __launch_bounds__(TV3_THREADS) tv3_dual_kernel(double* state, long long n, Tv3Shape s, Tv3Step c) {
    const long long HW = (long long)s.H * s.W, DHW = HW * s.D, total = n * DHW;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const double sigma = c.tau, den = 1.0 + sigma * c.alpha / c.lam;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const long long img = t / DHW, e = t - img * DHW;
        const int z = (int)(e / HW), r = (int)(e - z * HW), i = r / s.W, j = r - i * s.W;
        const Tv3State st = tv3_state(state, img, DHW);
        const double xb = st.xbar[e];
        const double d1 = i + 1 < s.H ? st.xbar[e + s.W] - xb : 0.0;
        const double d2 = j + 1 < s.W ? st.xbar[e + 1] - xb : 0.0;
        const double d0 = z + 1 < s.D ? st.xbar[e + HW] - xb : 0.0;
        double q1 = (st.p1[e] + sigma * (c.g1 * d1)) / den;
        double q2 = (st.p2[e] + sigma * (c.g2 * d2)) / den;
        double q0 = (st.p0[e] + sigma * (c.g0 * d0)) / den;
        const double nrm = sqrt((q1 * q1 + q2 * q2) + q0 * q0) / c.lam;
        if (nrm > 1.0) {
            q1 /= nrm;
            q2 /= nrm;
            q0 /= nrm;
        }
        st.p1[e] = q1;
        st.p2[e] = q2;
        st.p0[e] = q0;
    }
}

// chpart [n][parts]: written in the last iteration only
template <typename T>
__global__ void __launch_bounds__(TV3_THREADS) tv3_primal_kernel(double* state, double* chpart, const T* y, const T* weight, long long n,
                                                                 Tv3Shape s, Tv3Kernel kb, Tv3Step c, int last) {
    __shared__ double ks[TV3_TABLE];
    __shared__ double vt[TV3_TILE];
    __shared__ double rs[TV3_TILE];
    __shared__ double red[TV3_THREADS / 64];
    const int tid = threadIdx.x;
    const long long HW = (long long)s.H * s.W, DHW = HW * s.D, dhw = (long long)s.d * s.h * s.w;
    tv3_form_table(ks, kb, s);
    __syncthreads();
    for (long long item = blockIdx.x; item < n * s.parts; item += gridDim.x) {
        const long long img = item / s.parts;
        const int part = (int)(item - img * s.parts);
        const Tv3State st = tv3_state(state, img, DHW);
        const T* yi = y + img * dhw;
        const T* wi = weight ? weight + img * dhw : nullptr;
        double ch = 0.0;
        for (int tile = part; tile < s.tiles; tile += s.parts) {
            const Tv3Tile t = tv3_tile(s, tile);
            for (int idx = tid; idx < t.vox; idx += TV3_THREADS) {
                const Tv3Voxel v = tv3_voxel(s, t, idx);
                double dv = 0.0;
                if (v.i + 1 < s.H) dv += c.g1 * st.p1[v.e];
                if (v.i > 0) dv -= c.g1 * st.p1[v.e - s.W];
                if (v.j + 1 < s.W) dv += c.g2 * st.p2[v.e];
                if (v.j > 0) dv -= c.g2 * st.p2[v.e - 1];
                if (v.z + 1 < s.D) dv += c.g0 * st.p0[v.e];
                if (v.z > 0) dv -= c.g0 * st.p0[v.e - HW];
                vt[idx] = st.x[v.e] + c.tau * dv;
            }
            __syncthreads();   // v of the tile is in LDS
            for (int b = tid; b < t.blocks; b += TV3_THREADS) {
                const long long l = tv3_lr_index(s, t, b);
                const double wv = wi ? (double)wi[l] : 1.0;
                // a missing datum (w = 0) takes no part, whatever y holds there
                rs[b] = wv == 0.0 ? 0.0 : c.tau * wv / (1.0 + c.tau * wv * kb.ksq) * (tv3_tile_block_sum(vt, ks, s, t, b) - (double)yi[l]);
            }
            __syncthreads();   // the blocks' residuals are in LDS
            const int plane = t.RH * t.CW;
            for (int idx = tid; idx < t.vox; idx += TV3_THREADS) {
                const Tv3Voxel v = tv3_voxel(s, t, idx);
                const int r = idx - v.a * plane, rr = r / t.CW, cc = r - rr * t.CW;
                const int bb = rr % s.f1, bc = cc % s.f2, b = (rr / s.f1) * t.nw + cc / s.f2;
                const double xo = st.x[v.e];
                const double xn = vt[idx] - ks[(v.a * s.f1 + bb) * s.f2 + bc] * rs[b];
                st.xbar[v.e] = 2.0 * xn - xo;
                st.x[v.e] = xn;
                if (last) ch = fmax(ch, fabs(xn - xo));
            }
            __syncthreads();   // vt and rs are free for the next tile
        }
        if (last) {
            ch = block_max_f64(ch, red);
            if (tid == 0) chpart[item] = ch;
        }
    }
}

// the result and the objective's partials epart [n][parts]: x is read-only here
template <typename T>
__global__ void __launch_bounds__(TV3_THREADS) tv3_final_kernel(T* out, double* epart, const double* state, const T* y, const T* weight,
                                                                long long n, Tv3Shape s, Tv3Kernel kb, Tv3Step c) {
    __shared__ double ks[TV3_TABLE];
    __shared__ double vt[TV3_TILE];
    __shared__ double red[TV3_THREADS / 64];
    const int tid = threadIdx.x;
    const long long HW = (long long)s.H * s.W, DHW = HW * s.D, dhw = (long long)s.d * s.h * s.w;
    tv3_form_table(ks, kb, s);
    __syncthreads();
    for (long long item = blockIdx.x; item < n * s.parts; item += gridDim.x) {
        const long long img = item / s.parts;
        const int part = (int)(item - img * s.parts);
        const double* x = state + img * 5 * DHW;
        const T* yi = y + img * dhw;
        const T* wi = weight ? weight + img * dhw : nullptr;
        double en = 0.0, reg = 0.0;
        for (int tile = part; tile < s.tiles; tile += s.parts) {
            const Tv3Tile t = tv3_tile(s, tile);
            for (int idx = tid; idx < t.vox; idx += TV3_THREADS) {
                const Tv3Voxel v = tv3_voxel(s, t, idx);
                const double xe = x[v.e];
                vt[idx] = xe;
                out[img * DHW + v.e] = (T)xe;
                if (c.lam > 0.0) {
                    const double d1 = v.i + 1 < s.H ? x[v.e + s.W] - xe : 0.0;
                    const double d2 = v.j + 1 < s.W ? x[v.e + 1] - xe : 0.0;
                    const double d0 = v.z + 1 < s.D ? x[v.e + HW] - xe : 0.0;
                    const double t1 = c.g1 * d1, t2 = c.g2 * d2, t0 = c.g0 * d0;
                    reg += tv_huber(sqrt((t1 * t1 + t2 * t2) + t0 * t0), c.alpha);
                }
            }
            __syncthreads();
            for (int b = tid; b < t.blocks; b += TV3_THREADS) {
                const long long l = tv3_lr_index(s, t, b);
                const double wv = wi ? (double)wi[l] : 1.0;
                if (wv != 0.0) {
                    const double r = tv3_tile_block_sum(vt, ks, s, t, b) - (double)yi[l];
                    en += 0.5 * wv * r * r;
                }
            }
            __syncthreads();
        }
        if (c.lam > 0.0) en += c.lam * reg;
        en = block_sum_f64(en, red);
        if (tid == 0) epart[item] = en;
    }
}

// out [n][d][h][w] = A in [n][D][H][W]: one thread per LR voxel
__global__ void __launch_bounds__(TV3_THREADS) tv3_apply_kernel(double* __restrict__ out, const double* __restrict__ in, long long n,
                                                                Tv3Shape s, Tv3Kernel kb) {
    __shared__ double ks[TV3_TABLE];
    tv3_form_table(ks, kb, s);
    __syncthreads();
    const long long HW = (long long)s.H * s.W, DHW = HW * s.D, hw = (long long)s.h * s.w, dhw = hw * s.d, total = n * dhw;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const long long img = t / dhw, l = t - img * dhw;
        const int bd = (int)(l / hw), r = (int)(l - bd * hw), bi = r / s.w, bj = r - bi * s.w;
        const double* x = in + img * DHW;
        double acc = 0.0;
        for (int a = 0; a < s.f0; ++a)
            for (int b = 0; b < s.f1; ++b) {
                const double* row = x + ((long long)(bd * s.f0 + a) * s.H + (bi * s.f1 + b)) * s.W + bj * s.f2;
                const double* kr = ks + (a * s.f1 + b) * s.f2;
                for (int cc = 0; cc < s.f2; ++cc) acc += kr[cc] * row[cc];
            }
        out[t] = acc;
    }
}

// out [n][D][H][W] = A^T in [n][d][h][w]: one thread per HR voxel
__global__ void __launch_bounds__(TV3_THREADS) tv3_adjoint_kernel(double* __restrict__ out, const double* __restrict__ in, long long n,
                                                                  Tv3Shape s, Tv3Kernel kb) {
    __shared__ double ks[TV3_TABLE];
    tv3_form_table(ks, kb, s);
    __syncthreads();
    const long long HW = (long long)s.H * s.W, DHW = HW * s.D, dhw = (long long)s.d * s.h * s.w, total = n * DHW;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const long long img = t / DHW, e = t - img * DHW;
        const int z = (int)(e / HW), r = (int)(e - z * HW), i = r / s.W, j = r - i * s.W;
        const int bd = z / s.f0, bi = i / s.f1, bj = j / s.f2;
        out[t] = ks[((z - bd * s.f0) * s.f1 + (i - bi * s.f1)) * s.f2 + (j - bj * s.f2)] *
                 in[img * dhw + ((long long)bd * s.h + bi) * s.w + bj];
    }
}

// the HR sizes and the block factors of one call, and the tiling they imply
int tv3_shape_check(const char* who, int n, int D, int H, int W, int f0, int f1, int f2, Tv3Shape* s) {
    INR_REQUIRE(n >= 0, INR_E_INVALID, "%s: bad sizes (n_volumes = %d)", who, n);
    INR_REQUIRE(f0 >= 1 && f0 <= TV3_MAX_FACTOR && f1 >= 1 && f1 <= TV3_MAX_FACTOR && f2 >= 1 && f2 <= TV3_MAX_FACTOR, INR_E_INVALID,
                "%s: block factors are 1 .. %d per axis (got %d x %d x %d)", who, TV3_MAX_FACTOR, f0, f1, f2);
    INR_REQUIRE(D >= 1 && H >= 1 && W >= 1 && D <= TV3_MAX_SIDE && H <= TV3_MAX_SIDE && W <= TV3_MAX_SIDE, INR_E_INVALID,
                "%s: bad sizes (HR volumes of 1 .. %d samples per axis, got %d x %d x %d)", who, TV3_MAX_SIDE, D, H, W);
    INR_REQUIRE(D % f0 == 0 && H % f1 == 0 && W % f2 == 0, INR_E_INVALID,
                "%s: the HR volume %d x %d x %d is no whole number of %d x %d x %d blocks", who, D, H, W, f0, f1, f2);
    Tv3Shape v{};
    v.D = D, v.H = H, v.W = W, v.d = D / f0, v.h = H / f1, v.w = W / f2, v.f0 = f0, v.f1 = f1, v.f2 = f2;
    // a tile: up to TV3_TILE_COLS HR columns and TV3_TILE HR voxels (f0 f1 f2 <= 512, so one block always fits)
    int tw = TV3_TILE_COLS / f2;
    if (tw > TV3_TILE / (f0 * f1 * f2)) tw = TV3_TILE / (f0 * f1 * f2);
    if (tw > v.w) tw = v.w;
    int th = TV3_TILE / (f0 * f1 * f2 * tw);
    if (th > v.h) th = v.h;
    v.tw = tw, v.th = th;
    v.tiles_w = (v.w + tw - 1) / tw;
    v.tiles_h = (v.h + th - 1) / th;
    v.tiles = v.d * v.tiles_h * v.tiles_w;   // <= 2^30 voxels / 1
    v.parts = v.tiles < TV3_PARTS ? v.tiles : TV3_PARTS;
    *s = v;
    return 0;
}

// the caller's HOST factors k0 [f0], k1 [f1], k2 [f2]: finite, each summing to 1
int tv3_kernel_check(const char* who, const double* k0, const double* k1, const double* k2, const Tv3Shape& s, Tv3Kernel* kb) {
    INR_REQUIRE(k0 && k1 && k2, INR_E_INVALID, "%s: null pointer (kernel factors)", who);
    const double* in[3] = {k0, k1, k2};
    double* out[3] = {kb->k0, kb->k1, kb->k2};
    const int f[3] = {s.f0, s.f1, s.f2};
    for (int axis = 0; axis < 3; ++axis) {
        double sum = 0.0;
        for (int t = 0; t < TV3_MAX_FACTOR; ++t) out[axis][t] = 0.0;
        for (int t = 0; t < f[axis]; ++t) {
            INR_REQUIRE(std::isfinite(in[axis][t]), INR_E_INVALID, "%s: the kernel factors must be finite (k%d[%d] is %g)", who, axis, t,
                        in[axis][t]);
            out[axis][t] = in[axis][t];
            sum += in[axis][t];
        }
        INR_REQUIRE(std::isfinite(sum) && std::fabs(sum - 1.0) <= 1e-9, INR_E_INVALID, "%s: every kernel factor must sum to 1 (k%d sums to %.17g)",
                    who, axis, sum);
    }
    double ksq = 0.0;
    for (int a = 0; a < s.f0; ++a)
        for (int b = 0; b < s.f1; ++b)
            for (int c = 0; c < s.f2; ++c) {
                const double k = (kb->k1[b] * kb->k2[c]) * kb->k0[a];
                ksq += k * k;
            }
    kb->ksq = ksq;
    return 0;
}

// the workspace: the state x | xbar | p0 | p1 | p2 of every volume, then the partials of energy and change.  base == null: `total` only
struct Tv3View {
    double *state, *epart, *chpart;
    size_t total;
};
Tv3View tv3_view(int n, const Tv3Shape& s, void* base) {
    Tv3View v;
    WsCarver c(base, 16);
    const size_t nn = (size_t)(n > 0 ? n : 1);
    v.state = c.take<double>(nn * 5 * (size_t)s.D * (size_t)s.H * (size_t)s.W);
    v.epart = c.take<double>(nn * (size_t)s.parts);
    v.chpart = c.take<double>(nn * (size_t)s.parts);
    v.total = c.bytes();
    return v;
}

template <typename T>
int tv3_solve(const char* who, T* out, double* energy, double* change, const T* y, const T* weight, const T* x0, int n, int D, int H, int W,
              int f0, int f1, int f2, const double* k0, const double* k1, const double* k2, const double* grad_weights, double lam,
              double alpha, int n_iter, double* workspace, int64_t workspace_doubles, hipStream_t st) {
    INR_REQUIRE(out && y, INR_E_INVALID, "%s: null pointer", who);
    Tv3Shape s;
    Tv3Kernel kb;
    if (int rc = tv3_shape_check(who, n, D, H, W, f0, f1, f2, &s)) return rc;
    if (int rc = tv_params_check(who, lam, alpha, n_iter, INR_TVSR3D_MAX_ITER)) return rc;
    INR_REQUIRE(grad_weights, INR_E_INVALID, "%s: null pointer (grad_weights)", who);
    if (int rc = tv_grad_weights_check(who, grad_weights)) return rc;
    if (int rc = tv3_kernel_check(who, k0, k1, k2, s, &kb)) return rc;
    if (int rc = check_ws_doubles(who, workspace, workspace_doubles, tv3_view(n, s, nullptr).total)) return rc;
    if (n == 0) return 0;
    Tv3Step c;
    c.g0 = grad_weights[0], c.g1 = grad_weights[1], c.g2 = grad_weights[2];
    const double gsum = tv_grad_weight_sum(grad_weights, D, H, W);
    c.lam = gsum > 0.0 ? lam : 0.0;
    c.tau = gsum > 0.0 ? 1.0 / std::sqrt(4.0 * gsum) : 1.0 / std::sqrt(8.0);
    c.alpha = alpha;
    const Tv3View v = tv3_view(n, s, workspace);
    const long long voxels = (long long)n * D * H * W, items = (long long)n * s.parts;
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL((tv3_init_kernel<T>), dim3(tv_thread_grid(voxels, TV3_THREADS)), dim3(TV3_THREADS), 0, st, v.state, y, x0, (long long)n, s);
    INR_LAUNCH_CHECK();
    for (int it = 0; it < n_iter; ++it) {
        if (c.lam > 0.0) {
            hipLaunchKernelGGL(tv3_dual_kernel, dim3(tv_thread_grid(voxels, TV3_THREADS)), dim3(TV3_THREADS), 0, st, v.state, (long long)n, s, c);
            INR_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL((tv3_primal_kernel<T>), dim3(tv_grid(items)), dim3(TV3_THREADS), 0, st, v.state, v.chpart, y, weight,
                           (long long)n, s, kb, c, (int)(it + 1 == n_iter));
        INR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((tv3_final_kernel<T>), dim3(tv_grid(items)), dim3(TV3_THREADS), 0, st, out, v.epart, v.state, y, weight,
                       (long long)n, s, kb, c);
    INR_LAUNCH_CHECK();
    // chpart is written in the last iteration only: without one there is nothing to read
    return tv_finish<TV3_THREADS>(energy, change, nullptr, v.epart, s.parts, v.chpart, n_iter > 0 ? s.parts : 0, nullptr, 1.0, n, st);
}

int tv3_operator(const char* who, bool adjoint, double* out, const double* in, int n, int D, int H, int W, int f0, int f1, int f2,
                 const double* k0, const double* k1, const double* k2, hipStream_t st) {
    INR_REQUIRE(out && in, INR_E_INVALID, "%s: null pointer", who);
    Tv3Shape s;
    Tv3Kernel kb;
    if (int rc = tv3_shape_check(who, n, D, H, W, f0, f1, f2, &s)) return rc;
    if (int rc = tv3_kernel_check(who, k0, k1, k2, s, &kb)) return rc;
    if (n == 0) return 0;
    ProfScope ps(KC_OTHER, st);
    if (adjoint)
        hipLaunchKernelGGL(tv3_adjoint_kernel, dim3(tv_thread_grid((long long)n * D * H * W, TV3_THREADS)), dim3(TV3_THREADS), 0, st, out, in,
                           (long long)n, s, kb);
    else
        hipLaunchKernelGGL(tv3_apply_kernel, dim3(tv_thread_grid((long long)n * s.d * s.h * s.w, TV3_THREADS)), dim3(TV3_THREADS), 0, st, out, in,
                           (long long)n, s, kb);
    INR_LAUNCH_CHECK();
    return 0;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int inr_tvsr3d_block_apply(double* out, const double* in, int n_volumes, int depth, int height, int width, int f0, int f1, int f2,
                      const double* k0, const double* k1, const double* k2, void* stream) {
    return tv3_operator("inr_tvsr3d_block_apply", false, out, in, n_volumes, depth, height, width, f0, f1, f2, k0, k1, k2, (hipStream_t)stream);
}

int inr_tvsr3d_block_adjoint(double* out, const double* in, int n_volumes, int depth, int height, int width, int f0, int f1, int f2,
                        const double* k0, const double* k1, const double* k2, void* stream) {
    return tv3_operator("inr_tvsr3d_block_adjoint", true, out, in, n_volumes, depth, height, width, f0, f1, f2, k0, k1, k2, (hipStream_t)stream);
}

int64_t inr_tvsr3d_workspace_doubles(int n_volumes, int depth, int height, int width, int f0, int f1, int f2) {
    Tv3Shape s;
    if (tv3_shape_check("inr_tvsr3d_workspace_doubles", n_volumes, depth, height, width, f0, f1, f2, &s)) return 0;
    return (int64_t)(tv3_view(n_volumes, s, nullptr).total / sizeof(double));
}

int inr_tvsr3d_solve(double* out, double* energy, double* change, const double* y, const double* weight, const double* x0, int n_volumes,
                     int depth, int height, int width, int f0, int f1, int f2, const double* k0, const double* k1, const double* k2,
                     const double* grad_weights, double lambda, double alpha, int n_iter, double* workspace, int64_t workspace_doubles,
                     void* stream) {
    return tv3_solve("inr_tvsr3d_solve", out, energy, change, y, weight, x0, n_volumes, depth, height, width, f0, f1, f2, k0, k1, k2,
                     grad_weights, lambda, alpha, n_iter, workspace, workspace_doubles, (hipStream_t)stream);
}

int inr_tvsr3d_solve_f32(float* out, double* energy, double* change, const float* y, const float* weight, const float* x0, int n_volumes,
                         int depth, int height, int width, int f0, int f1, int f2, const double* k0, const double* k1, const double* k2,
                         const double* grad_weights, double lambda, double alpha, int n_iter, double* workspace,
                         int64_t workspace_doubles, void* stream) {
    return tv3_solve("inr_tvsr3d_solve_f32", out, energy, change, y, weight, x0, n_volumes, depth, height, width, f0, f1, f2, k0, k1, k2,
                     grad_weights, lambda, alpha, n_iter, workspace, workspace_doubles, (hipStream_t)stream);
}

}  // extern "C"
