// Gibbs-ringing removal by local sub-voxel shifts (Kellner et al., MRM 2016; include/inrhip.h: inr_degibbs_lines, inr_degibbs2d;
// DESIGN.md 4v).  A line x[0..n) is re-sampled at the 2N shifts +-j/(2N), j = 1..N (the unshifted line itself is the first candidate,
// bit for bit); per sample the candidate whose neighbourhood oscillates least is chosen -- tv = min(L, R), the sums of |differences| over
// the window (w_min, w_max) to the left and to the right -- and interpolated back onto the grid.  An image is split by the filter G1
// into I1 + I0 = I; I1 is unrung along the columns, I0 along the rows.  tests/degibbs_common.py restates all of it in float64 numpy.
//
// A shifted copy is a product with a circulant matrix, x_s[i] = sum_j h_s((i - j) mod n) x[j], so the B operand of the tile loop
// (gemm_f64.h: gf_tile_fn) is generated from the table h [2N][n] that one small kernel forms per call and axis length -- never a dense
// [n][n] operator per shift.  dg_lines_kernel runs the whole shift loop: a workgroup owns a panel of 64 lines and one column tile; the
// windows and the interpolation reach w_max + 2 columns either way, so the 64 computed columns carry a halo and DG_TILE - 2 (w_max + 2)
// are owned (54 at the default window); column indices wrap mod n, which also serves n < 64.  Per shift the 64 x 64 tile of x_s is
// computed on v_mfma_f64_16x16x4_f64 with K ascending (the A panel re-read from L2: 64 lines of 1,024 doubles do not fit in LDS), staged
// in LDS, and every thread walks its fixed samples: the running best tv, its index and the interpolated value stay in registers over
// all shifts and are stored once.  Lines are addressed by three strides, so the pass along an image's rows axis is the same kernel: no
// transpose through memory.  LDS: the two staging planes (20.7 KB), the tile [64][65] (33.3 KB) and 64 column indices: two workgroups
// share a CU, which __launch_bounds__(256, 2) asks the compiler for -- it then holds the kernel to 256 VGPRs and spills 144 of the
// kernel's state to scratch.  Measured together with the prefetching tile loop, not apart: 320 images of 128 x 128 in 7.5 ms against
// 14.3 ms with one workgroup per CU (334 VGPRs, no spill) and a loop that fetched, waited and multiplied.
//
// The split uses the dense real cosine / sine DFT matrices C_a, S_a [n_a][n_a] (formed on the device, phases reduced exactly in
// integers) in four products per image, their block operands composed by functors, G1 applied in the second epilogue and I0 = I - I1
// formed in the last.  A batch is walked in chunks of images so that the workspace holds six planes of at most
// INR_DEGIBBS_CHUNK_DOUBLES each; an image's bits do not depend on its place in the batch or the chunk.  Every kernel walks its work
// items in a stride loop over a capped grid (tv_grid: inr_debug_set(32, .) caps it further); fixed-order sums, no atomics.
#include "gemm_f64.h"
#include "tv_shared.h"

namespace inr {
namespace {

constexpr int DG_TILE = GF_TILE;
constexpr int DG_TP = DG_TILE + 1;                                   // doubles per line of the staged tile
constexpr int DG_MAX_OWN = DG_TILE - 2 * 3;                          // w_max = 1
constexpr int DG_SAMPLES = (DG_TILE * DG_MAX_OWN + 255) / 256;       // samples of a tile per thread, at most

// lines of n samples: element (image g, line l, sample i) at g * img_stride + l * line_stride + i * es, in every array of the call
struct DgLines {
    long long n_img, lpi, ppi;         // groups of lines, lines and panels per group
    long long img_stride, line_stride, es;
    int n, nshifts, w_min, w_max, halo, own, ntiles;
};

// h [2N][n]: rows 0 .. N - 1 the shifts +j/(2N), rows N .. 2N - 1 the shifts -j/(2N), j = 1 .. N
__global__ void __launch_bounds__(256) dg_table_kernel(double* __restrict__ table, int n, int N) {
    const long long total = 2ll * N * n;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int sidx = (int)(idx / n), d = (int)(idx % n);
        const long long j = sidx < N ? sidx + 1 : -(sidx - N + 1);
        const long long D = 2ll * N * n;
        long long q = (2ll * N * d + j) % D;
        if (q < 0) q += D;
        const double half = (double)((long long)N * n);
        double s = 0.0;
        for (int k = 0; k <= n / 2; ++k) {
            const double c = k == 0 ? 1.0 : (2 * k == n ? 1.0 : 2.0);
            s += c * cospi((double)((k * q) % D) / half);
        }
        table[idx] = s / (double)n;
    }
}

// cs [2][n][n]: cos and sin of 2 pi k j / n
__global__ void __launch_bounds__(256) dg_dft_kernel(double* __restrict__ cs, int n) {
    const long long total = (long long)n * n;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long k = idx / n, j = idx % n;
        const double ph = 2.0 * (double)((k * j) % n) / (double)n;
        cs[idx] = cospi(ph);
        cs[total + idx] = sinpi(ph);
    }
}

// B(k, c) = h_s((g(c) - k) mod n): column c of the tile is sample g(c) of the line
struct DgCirculant {
    const double* __restrict__ h;
    const int* gcol;
    int n;
    __device__ __forceinline__ double operator()(int k, int c) const {
        int d = gcol[c] - k;
        if (d < 0) d += n;
        return h[d];
    }
};
struct DgStage {
    double (*T)[DG_TP];
    long long row0;
    __device__ __forceinline__ void operator()(long long row, int col, int, double v) const { T[(int)(row - row0)][col] = v; }
};

// min(L, R) of the sample at Tp[0]
__device__ __forceinline__ double dg_tv(const double* Tp, int w_min, int w_max) {
    double L = 0.0, R = 0.0;
    for (int t = w_min; t <= w_max; ++t) L += fabs(Tp[-t] - Tp[-t - 1]);
    for (int t = w_min; t <= w_max; ++t) R += fabs(Tp[t + 1] - Tp[t]);
    return fmin(L, R);
}

// out = (add ? add + U(in) : U(in)), rounded once to TO; choice (nullable) the index of the chosen shift in list order
template <typename TI, typename TO>
__global__ void __launch_bounds__(256, 2) dg_lines_kernel(TO* __restrict__ out, int32_t* __restrict__ choice, const TI* __restrict__ in,
                                                       const double* __restrict__ add, const double* __restrict__ table, DgLines g) {
    __shared__ double As[GF_KS][GF_PITCH];
    __shared__ double Bs[GF_KS][GF_PITCH];
    __shared__ double T[DG_TILE][DG_TP];
    __shared__ int gcol[DG_TILE];
    const int t = threadIdx.x;
    const long long items = g.n_img * g.ppi * g.ntiles;
    const double inv2N = 1.0 / (2.0 * g.nshifts);
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int tile = (int)(item % g.ntiles);
        const long long panel = (item / g.ntiles) % g.ppi, img = item / (g.ntiles * g.ppi);
        const long long row0 = panel * DG_TILE, base = img * g.img_stride;
        const int c0 = tile * g.own, nown = g.n - c0 < g.own ? g.n - c0 : g.own;
        __syncthreads();                          // the previous item's samples are done with T and gcol
        if (t < DG_TILE) {
            int c = (c0 - g.halo + t) % g.n;
            gcol[t] = c < 0 ? c + g.n : c;
        }
        __syncthreads();
        // the first candidate: the line itself; the contiguous direction of the lines goes over neighbouring threads
        for (int e = t; e < DG_TILE * DG_TILE; e += 256) {
            const int r = g.es == 1 ? e / DG_TILE : e & (DG_TILE - 1), c = g.es == 1 ? e & (DG_TILE - 1) : e / DG_TILE;
            if (row0 + r < g.lpi) T[r][c] = (double)in[base + (row0 + r) * g.line_stride + gcol[c] * g.es];
        }
        __syncthreads();
        int off[DG_SAMPLES];
        double best_tv[DG_SAMPLES], best_val[DG_SAMPLES];
        int best_idx[DG_SAMPLES];
#pragma unroll
        for (int m = 0; m < DG_SAMPLES; ++m) {
            const int e = t + 256 * m, r = e / g.own, j = e - r * g.own;
            const bool valid = r < DG_TILE && row0 + r < g.lpi && j < nown;
            off[m] = valid ? r * DG_TP + g.halo + j : -1;
            best_idx[m] = 0;
            best_tv[m] = 0.0;
            best_val[m] = 0.0;
            if (valid) {
                const double* Tp = &T[0][0] + off[m];
                best_tv[m] = dg_tv(Tp, g.w_min, g.w_max);
                best_val[m] = Tp[0];
            }
        }
        const GfStrided<GfIdentity, TI> la{in + base, g.line_stride, g.es};
        DgStage stage{T, row0};
        for (int sidx = 0; sidx < 2 * g.nshifts; ++sidx) {
            const DgCirculant lb{table + (long long)sidx * g.n, gcol, g.n};
            // the loop's first barrier comes after every thread's samples of the previous candidate
            gf_tile_fn(As, Bs, la, g.es == 1, lb, false, row0, 0, g.lpi, DG_TILE, g.n, 0, stage);
            __syncthreads();
            const bool pos = sidx < g.nshifts;
            const double s = (double)(pos ? sidx + 1 : sidx - g.nshifts + 1) * inv2N;   // |shift|
#pragma unroll
            for (int m = 0; m < DG_SAMPLES; ++m) {
                if (off[m] < 0) continue;
                const double* Tp = &T[0][0] + off[m];
                const double tv = dg_tv(Tp, g.w_min, g.w_max);
                if (tv < best_tv[m]) {
                    best_tv[m] = tv;
                    best_idx[m] = sidx + 1;
                    best_val[m] = (1.0 - s) * Tp[0] + s * (pos ? Tp[-1] : Tp[1]);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < DG_SAMPLES; ++m) {
            if (off[m] < 0) continue;
            const int e = t + 256 * m, r = e / g.own, j = e - r * g.own;
            const long long at = base + (row0 + r) * g.line_stride + (long long)(c0 + j) * g.es;
            out[at] = (TO)(add ? add[at] + best_val[m] : best_val[m]);
            if (choice) choice[at] = best_idx[m];
        }
    }
}

// ---- the split I = I1 + I0 --------------------------------------------------------------------------------------------------------------
// one batched product per step: Op gives the operands and the epilogue of batch entry b
template <class Op>
__global__ void __launch_bounds__(256) dg_gemm_kernel(Op op) {
    __shared__ double As[GF_KS][GF_PITCH];
    __shared__ double Bs[GF_KS][GF_PITCH];
    const int rt = (op.M + DG_TILE - 1) / DG_TILE, ct = (op.N + DG_TILE - 1) / DG_TILE;
    const long long items = (long long)op.batch * rt * ct;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int b = (int)(item / (rt * ct)), rem = (int)(item % (rt * ct));
        const auto la = op.a(b);
        const auto lb = op.b(b);
        auto epi = op.epi(b);
        gf_tile_fn(As, Bs, la, Op::A_KFAST, lb, Op::B_KFAST, (long long)(rem / ct) * DG_TILE, (rem % ct) * DG_TILE, op.M, op.N, op.K, b, epi);
    }
}

// [C | -S] [n][2n] (wide) or [C; -S] [2n][n] (tall) of one axis
struct DgDftB {
    const double* __restrict__ cs;
    int n, wide;
    __device__ __forceinline__ double operator()(int k, int col) const {
        const long long nn = (long long)n * n;
        if (wide) return col < n ? cs[(long long)k * n + col] : -cs[nn + (long long)k * n + col - n];
        return k < n ? cs[(long long)k * n + col] : -cs[nn + (long long)(k - n) * n + col];
    }
};
// [[C, sgn S], [-sgn S, C]] [2n][2n]: sgn = +1 the forward transform of (re; im), -1 its inverse
struct DgDftA {
    const double* __restrict__ cs;
    int n;
    double sgn;
    __device__ __forceinline__ double operator()(long long row, int k) const {
        const int rq = row >= n, kq = k >= n;
        const long long at = (row - (rq ? n : 0)) * n + (k - (kq ? n : 0));
        if (rq == kq) return cs[at];
        const double s = cs[(long long)n * n + at];
        return rq ? -sgn * s : sgn * s;
    }
};

// 1. (P | Q) = I [C1 | -S1], stored as the planes [2][H][W]
template <typename T>
struct DgStep1 {
    static constexpr bool A_KFAST = true, B_KFAST = false;
    const T* in;
    double* pq;
    const double* cs1;
    int batch, H, W, M, N, K;
    struct Epi {
        double* pq;
        int H, W;
        __device__ __forceinline__ void operator()(long long row, int col, int, double v) const {
            const int plane = col >= W;
            pq[((long long)plane * H + row) * W + col - plane * W] = v;
        }
    };
    __device__ GfStrided<GfIdentity, T> a(int b) const { return {in + (long long)b * H * W, W, 1}; }
    __device__ DgDftB b(int) const { return {cs1, W, 1}; }
    __device__ Epi epi(int b) const { return {pq + 2ll * b * H * W, H, W}; }
};
// 2. (Xr; Xi) = G1 . [[C0, S0], [-S0, C0]] (P; Q)  and  3. (Yr; Yi) = (1/H) [[C0, -S0], [S0, C0]] (Xr; Xi), stored as [H][2][W]
struct DgStep23 {
    static constexpr bool A_KFAST = true, B_KFAST = false;
    const double* src;
    double* dst;
    const double *cs0, *cs1;
    int batch, H, W, M, N, K, inverse;
    struct Epi {
        double* dst;
        const double *cs0, *cs1;
        int H, W, inverse;
        __device__ __forceinline__ void operator()(long long row, int col, int, double v) const {
            const int plane = row >= H, r = (int)row - plane * H;
            if (inverse) {
                dst[((long long)r * 2 + plane) * W + col] = v / (double)H;
                return;
            }
            // c_a(k) = 1 + cos(2 pi k / n_a) from row 1 of the cosine matrix: exactly 0 at k = n_a / 2
            const double ca = 1.0 + cs0[H + r], cb = 1.0 + cs1[W + col], den = ca + cb;
            dst[row * W + col] = (den == 0.0 ? 0.5 : ca / den) * v;
        }
    };
    __device__ DgDftA a(int) const { return {cs0, H, inverse ? -1.0 : 1.0}; }
    __device__ GfStridedB<GfIdentity, double> b(int b_) const { return {src + 2ll * b_ * H * W, W, 1}; }
    __device__ Epi epi(int b_) const { return {dst + 2ll * b_ * H * W, cs0, cs1, H, W, inverse}; }
};
// 4. I1 = (1/W) (Yr | Yi) [C1; -S1],  I0 = I - I1
template <typename T>
struct DgStep4 {
    static constexpr bool A_KFAST = true, B_KFAST = false;
    const T* in;
    const double* y;
    double *i1, *i0;
    const double* cs1;
    int batch, H, W, M, N, K;
    struct Epi {
        const T* in;
        double *i1, *i0;
        int W;
        __device__ __forceinline__ void operator()(long long row, int col, int, double v) const {
            const long long at = row * W + col;
            const double a = v / (double)W;
            i1[at] = a;
            i0[at] = (double)in[at] - a;
        }
    };
    __device__ GfStrided<GfIdentity, double> a(int b) const { return {y + 2ll * b * H * W, 2ll * W, 1}; }
    __device__ DgDftB b(int) const { return {cs1, W, 0}; }
    __device__ Epi epi(int b) const {
        const long long o = (long long)b * H * W;
        return {in + o, i1 + o, i0 + o, W};
    }
};

template <class Op>
int dg_gemm(const Op& op, hipStream_t st) {
    const long long items = (long long)op.batch * ((op.M + DG_TILE - 1) / DG_TILE) * ((op.N + DG_TILE - 1) / DG_TILE);
    hipLaunchKernelGGL(dg_gemm_kernel<Op>, dim3(tv_grid(items)), dim3(256), 0, st, op);
    INR_LAUNCH_CHECK();
    return 0;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
constexpr int DG_MAX_LINE = INR_DEGIBBS_MAX_LINE, DG_MAX_SHIFTS = INR_DEGIBBS_MAX_SHIFTS, DG_MAX_WINDOW = INR_DEGIBBS_MAX_WINDOW;
constexpr long long DG_CHUNK = INR_DEGIBBS_CHUNK_DOUBLES;

int dg_params_check(const char* who, int nshifts, int w_min, int w_max) {
    INR_REQUIRE(nshifts >= 1 && nshifts <= DG_MAX_SHIFTS, INR_E_INVALID, "%s: nshifts must be 1 .. %d (got %d)", who, DG_MAX_SHIFTS, nshifts);
    INR_REQUIRE(w_min >= 1 && w_min <= w_max && w_max <= DG_MAX_WINDOW, INR_E_INVALID,
                "%s: the window must satisfy 1 <= w_min <= w_max <= %d (got %d, %d)", who, DG_MAX_WINDOW, w_min, w_max);
    return 0;
}
// w_max < 0: the planners, which do not know the window, take the least any window asks for
int dg_line_check(const char* who, const char* axis, int n, int w_max) {
    const int least = 2 * (w_max < 0 ? 1 : w_max) + 3;
    INR_REQUIRE(n >= least && n <= DG_MAX_LINE, INR_E_INVALID, "%s: %s of 2 w_max + 3 = %d .. %d samples (got %d)", who, axis, least,
                DG_MAX_LINE, n);
    return 0;
}
int dg_overlap_check(const char* who, const void* out, const void* in, size_t out_bytes, size_t in_bytes) {
    const char *o = static_cast<const char*>(out), *i = static_cast<const char*>(in);
    INR_REQUIRE(o + out_bytes <= i || i + in_bytes <= o, INR_E_INVALID, "%s: out must not overlap in", who);
    return 0;
}

long long dg_chunk_images(int n_images, int H, int W) {
    long long c = DG_CHUNK / ((long long)H * W);
    if (c < 1) c = 1;
    return n_images < c ? (n_images > 0 ? n_images : 1) : c;
}

struct DgLinesView { double* table; size_t total; };
DgLinesView dg_lines_view(int n, void* base) {
    DgLinesView v;
    WsCarver c(base, 256);
    v.table = c.take<double>((size_t)2 * DG_MAX_SHIFTS * (size_t)n);
    v.total = c.bytes();
    return v;
}
// the two tables, the DFT matrices of the two axes and six planes of a chunk: I1, I0, (P; Q) / (Yr, Yi), (Xr; Xi) / U1(I1)
struct Dg2dView { double *table0, *table1, *cs0, *cs1, *i1, *i0, *pq, *x; size_t total; };
Dg2dView dg_2d_view(int n_images, int H, int W, void* base) {
    Dg2dView v;
    WsCarver c(base, 256);
    const size_t plane = (size_t)dg_chunk_images(n_images, H, W) * (size_t)H * (size_t)W;
    v.table0 = c.take<double>((size_t)2 * DG_MAX_SHIFTS * (size_t)H);
    v.table1 = c.take<double>((size_t)2 * DG_MAX_SHIFTS * (size_t)W);
    v.cs0 = c.take<double>((size_t)2 * H * H);
    v.cs1 = c.take<double>((size_t)2 * W * W);
    v.i1 = c.take<double>(plane);
    v.i0 = c.take<double>(plane);
    v.pq = c.take<double>(2 * plane);
    v.x = c.take<double>(2 * plane);
    v.total = c.bytes();
    return v;
}

int dg_lines_sizes_check(const char* who, long long n_lines, int n, int nshifts, int w_min, int w_max, bool planner) {
    INR_REQUIRE(n_lines >= 0 && n_lines <= (1ll << 40), INR_E_INVALID, "%s: bad sizes (n_lines = %lld)", who, n_lines);
    if (planner)
        INR_REQUIRE(nshifts >= 1 && nshifts <= DG_MAX_SHIFTS, INR_E_INVALID, "%s: nshifts must be 1 .. %d (got %d)", who, DG_MAX_SHIFTS, nshifts);
    else if (int rc = dg_params_check(who, nshifts, w_min, w_max))
        return rc;
    return dg_line_check(who, "lines", n, planner ? -1 : w_max);
}
int dg_2d_sizes_check(const char* who, int n_images, int H, int W, int nshifts, int w_min, int w_max, bool planner) {
    INR_REQUIRE(n_images >= 0, INR_E_INVALID, "%s: bad sizes (n_images = %d)", who, n_images);
    if (planner)
        INR_REQUIRE(nshifts >= 1 && nshifts <= DG_MAX_SHIFTS, INR_E_INVALID, "%s: nshifts must be 1 .. %d (got %d)", who, DG_MAX_SHIFTS, nshifts);
    else if (int rc = dg_params_check(who, nshifts, w_min, w_max))
        return rc;
    if (int rc = dg_line_check(who, "rows", H, planner ? -1 : w_max)) return rc;
    return dg_line_check(who, "columns", W, planner ? -1 : w_max);
}

int dg_table(double* table, int n, int nshifts, hipStream_t st) {
    hipLaunchKernelGGL(dg_table_kernel, dim3(tv_thread_grid(2ll * nshifts * n, 256)), dim3(256), 0, st, table, n, nshifts);
    INR_LAUNCH_CHECK();
    return 0;
}

DgLines dg_lines_shape(long long n_img, long long lpi, int n, long long img_stride, long long line_stride, long long es, int nshifts,
                       int w_min, int w_max) {
    DgLines g;
    g.n_img = n_img, g.lpi = lpi, g.ppi = (lpi + DG_TILE - 1) / DG_TILE;
    g.img_stride = img_stride, g.line_stride = line_stride, g.es = es;
    g.n = n, g.nshifts = nshifts, g.w_min = w_min, g.w_max = w_max;
    g.halo = w_max + 2, g.own = DG_TILE - 2 * g.halo, g.ntiles = (n + g.own - 1) / g.own;
    return g;
}

template <typename TI, typename TO>
int dg_lines(TO* out, int32_t* choice, const TI* in, const double* add, const double* table, const DgLines& g, hipStream_t st) {
    hipLaunchKernelGGL((dg_lines_kernel<TI, TO>), dim3(tv_grid(g.n_img * g.ppi * g.ntiles)), dim3(256), 0, st, out, choice, in, add, table, g);
    INR_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int degibbs_lines(const char* who, T* out, int32_t* choice, const T* in, long long n_lines, int n, int nshifts, int w_min, int w_max,
                  double* workspace, int64_t workspace_doubles, hipStream_t st) {
    INR_REQUIRE(out && in, INR_E_INVALID, "%s: null pointer (out and in are required)", who);
    if (int rc = dg_lines_sizes_check(who, n_lines, n, nshifts, w_min, w_max, false)) return rc;
    const size_t bytes = (size_t)n_lines * n * sizeof(T);
    if (int rc = dg_overlap_check(who, out, in, bytes, bytes)) return rc;
    if (int rc = check_ws_doubles(who, workspace, workspace_doubles, dg_lines_view(n, nullptr).total)) return rc;
    if (n_lines == 0) return 0;
    ProfScope ps(KC_OTHER, st);
    const DgLinesView v = dg_lines_view(n, workspace);
    if (int rc = dg_table(v.table, n, nshifts, st)) return rc;
    return dg_lines<T, T>(out, choice, in, nullptr, v.table, dg_lines_shape(1, n_lines, n, 0, n, 1, nshifts, w_min, w_max), st);
}

template <typename T>
int degibbs2d(const char* who, T* out, int32_t* choice, const T* in, int n_images, int H, int W, int nshifts, int w_min, int w_max,
              double* workspace, int64_t workspace_doubles, hipStream_t st) {
    INR_REQUIRE(out && in, INR_E_INVALID, "%s: null pointer (out and in are required)", who);
    if (int rc = dg_2d_sizes_check(who, n_images, H, W, nshifts, w_min, w_max, false)) return rc;
    const size_t bytes = (size_t)n_images * H * W * sizeof(T);
    if (int rc = dg_overlap_check(who, out, in, bytes, bytes)) return rc;
    if (int rc = check_ws_doubles(who, workspace, workspace_doubles, dg_2d_view(n_images, H, W, nullptr).total)) return rc;
    if (n_images == 0) return 0;
    ProfScope ps(KC_OTHER, st);
    const Dg2dView v = dg_2d_view(n_images, H, W, workspace);
    if (int rc = dg_table(v.table0, H, nshifts, st)) return rc;
    if (int rc = dg_table(v.table1, W, nshifts, st)) return rc;
    hipLaunchKernelGGL(dg_dft_kernel, dim3(tv_thread_grid((long long)H * H, 256)), dim3(256), 0, st, v.cs0, H);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(dg_dft_kernel, dim3(tv_thread_grid((long long)W * W, 256)), dim3(256), 0, st, v.cs1, W);
    INR_LAUNCH_CHECK();
    const long long chunk = dg_chunk_images(n_images, H, W), hw = (long long)H * W, all = (long long)n_images * hw;
    for (long long first = 0; first < n_images; first += chunk) {
        const int nb = (int)(n_images - first < chunk ? n_images - first : chunk);
        const T* src = in + first * hw;
        if (int rc = dg_gemm(DgStep1<T>{src, v.pq, v.cs1, nb, H, W, H, 2 * W, W}, st)) return rc;
        if (int rc = dg_gemm(DgStep23{v.pq, v.x, v.cs0, v.cs1, nb, H, W, 2 * H, W, 2 * H, 0}, st)) return rc;
        if (int rc = dg_gemm(DgStep23{v.x, v.pq, v.cs0, v.cs1, nb, H, W, 2 * H, W, 2 * H, 1}, st)) return rc;
        if (int rc = dg_gemm(DgStep4<T>{src, v.pq, v.i1, v.i0, v.cs1, nb, H, W, H, W, 2 * W}, st)) return rc;
        // U1(I1), along the columns axis, into a plane of v.x; then out = that + U0(I0), along the rows axis: lines of stride W
        int32_t* ch = choice ? choice + first * hw : nullptr;
        if (int rc = dg_lines<double, double>(v.x, ch ? ch + all : nullptr, v.i1, nullptr, v.table1,
                                              dg_lines_shape(1, (long long)nb * H, W, 0, W, 1, nshifts, w_min, w_max), st))
            return rc;
        if (int rc = dg_lines<double, T>(out + first * hw, ch, v.i0, v.x, v.table0,
                                         dg_lines_shape(nb, W, H, hw, 1, W, nshifts, w_min, w_max), st))
            return rc;
    }
    return 0;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_degibbs_lines_workspace_doubles(long long n_lines, int n, int nshifts) {
    if (dg_lines_sizes_check("inr_degibbs_lines_workspace_doubles", n_lines, n, nshifts, 0, 0, true)) return 0;
    return (int64_t)(dg_lines_view(n, nullptr).total / sizeof(double));
}

int64_t inr_degibbs2d_workspace_doubles(int n_images, int height, int width, int nshifts) {
    if (dg_2d_sizes_check("inr_degibbs2d_workspace_doubles", n_images, height, width, nshifts, 0, 0, true)) return 0;
    return (int64_t)(dg_2d_view(n_images, height, width, nullptr).total / sizeof(double));
}

int inr_degibbs_lines(double* out, int32_t* choice, const double* in, long long n_lines, int n, int nshifts, int w_min, int w_max,
                      double* workspace, int64_t workspace_doubles, void* stream) {
    return degibbs_lines("inr_degibbs_lines", out, choice, in, n_lines, n, nshifts, w_min, w_max, workspace, workspace_doubles,
                         (hipStream_t)stream);
}

int inr_degibbs_lines_f32(float* out, int32_t* choice, const float* in, long long n_lines, int n, int nshifts, int w_min, int w_max,
                          double* workspace, int64_t workspace_doubles, void* stream) {
    return degibbs_lines("inr_degibbs_lines_f32", out, choice, in, n_lines, n, nshifts, w_min, w_max, workspace, workspace_doubles,
                         (hipStream_t)stream);
}

int inr_degibbs2d(double* out, int32_t* choice, const double* in, int n_images, int height, int width, int nshifts, int w_min, int w_max,
                  double* workspace, int64_t workspace_doubles, void* stream) {
    return degibbs2d("inr_degibbs2d", out, choice, in, n_images, height, width, nshifts, w_min, w_max, workspace, workspace_doubles,
                     (hipStream_t)stream);
}

int inr_degibbs2d_f32(float* out, int32_t* choice, const float* in, int n_images, int height, int width, int nshifts, int w_min, int w_max,
                      double* workspace, int64_t workspace_doubles, void* stream) {
    return degibbs2d("inr_degibbs2d_f32", out, choice, in, n_images, height, width, nshifts, w_min, w_max, workspace, workspace_doubles,
                     (hipStream_t)stream);
}

}  // extern "C"
