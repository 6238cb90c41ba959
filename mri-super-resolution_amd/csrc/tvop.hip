// TV / Huber super-resolution under a dense separable acquisition model: the prior of tvsr.hip and ANY linear operator
// of the form A x = R0 x R1^T, R0 [h][H] and R1 [w][W] dense DEVICE doubles shared by the whole batch -- k-space truncation
// (inr_fourier_operator), a point-spread function wider than the pixel, a non-integer ratio; h may be below, equal to or above H.
//   x* = argmin_x 1/2 sum_i w_i ((A x)_i - y_i)^2 + lambda sum_j H_alpha(|(grad x)_j|),   A x = (R0 x) R1^T,  A^T r = R0^T (r R1).
// Images are HR [n][H][W] and LR [n][h][w].  grad, div and H_alpha are those of tvsr.hip.  tests/tvop_common.py restates all of it.
//
// Chambolle-Pock with BOTH terms dual (the iteration of tvmf.hip), from x = xbar = x0, p = 0, q = 0:
//   p    <- (p + sigma grad(xbar)) / (1 + sigma alpha / lambda);  p <- p / max(1, |p| / lambda)        (lambda = 0: skipped, p = 0)
//   q    <- (q + sigma (A xbar - y)) / (1 + sigma / w)   where w > 0, else 0 (such a datum is never read: it may be NaN)
//   x'   <- x - tau (A^T q - div p);  xbar <- 2 x' - x;  x <- x'
// tau = sigma = 1 / sqrt(8 + c0 c1), c_a = (max_i sum_j |R_a[i][j]|) (max_j sum_i |R_a[i][j]|) = |R_a|_inf |R_a|_1 >= |R_a|_2^2, the sums
// in ascending index: |A|^2 = |R0|^2 |R1|^2 <= c0 c1 and |grad|^2 <= 8, so |(grad, A)|^2 <= 8 + c0 c1 with no power iteration.  The step
// kernel forms it ON THE DEVICE and leaves it in the workspace, where every later kernel reads it: no host read anywhere.
// Without x0 the start is the normalised back-projection through the absolute operators,
//   x0 = (|R0|^T (u y) |R1|) / (|R0|^T u |R1|),  u = [w > 0],  0 where the denominator is not > 0,
// two passes of the adjoint's two launches with GfAbs on the operator load.
//
// Every contraction is the fp64 tile loop of gemm_f64.h (v_mfma_f64_16x16x4_f64, fixed K order) under ONE kernel template,
// op_gemm_kernel, with a flattened grid-stride loop over (image, tile row, tile column) and an epilogue functor; inr_tvop_apply and
// inr_tvop_adjoint are launches 2 + 3 and 4 + 5 of the solver with a plain store, so A x comes out of both with the same bits.
//
// LAUNCHES.  Plain launches on the caller's stream: no cooperative launch, no atomics, no spin, no host read.  Per iteration:
//   1 dual    (thread per HR pixel e):   reads xbar[e], xbar[e + W], xbar[e + 1] -- neighbours' --, reads and writes p0[e], p1[e] -- its own;
//   2 rows    mid = R0 xbar:             reads R0 and xbar across threads, writes its own mid [h][W] element;
//   3 cols    u = mid R1^T:              reads mid and R1 across threads; the epilogue reads y, w and reads and writes q of its own
//                                        element; u never reaches memory;
//   4 rowsT   mid = q R1:                reads q and R1 across threads, writes its own mid element;
//   5 colsT   a = R0^T mid:              reads R0 and mid across threads; the epilogue reads p0[e], p0[e - W], p1[e], p1[e - 1] -- others',
//                                        read-only here --, reads and writes x[e], xbar[e] -- its own; in the last iteration the block
//                                        writes the tile's maximum of |x' - x|.
// Around them: step (one workgroup: tau), init (thread per element: its own x, xbar, p0, p1, q), the back-projection (launches 4 + 5
// twice, thread-per-datum fills of q between them), final = launches 2 + 3 on x with 1/2 w (u - y)^2 summed per LR tile, an HR-tile
// launch (the result rounded once to the caller's type, the prior per HR tile) and finish (one workgroup per image adds the
// partials and takes their maximum, thread t those at t, t + 256, ... in ascending order).
// Within a launch a field is either read across threads or written by its owner alone: xbar is read-only in 1 and 2 and owner-written
// in 5, p is owner-written in 1 and read-only in 5, q is owner-written in 3 and read-only in 4, mid is owner-written in 2 and 4 and
// read-only in 3 and 5, x is touched by its own thread only, tau is written by step and read-only after it.
// STREAM ORDER IS THE BARRIER between launches.
//
// The partials are per TILE and the tile count depends on the shape alone, so the bits of energy and change depend neither on the
// grid (capped at TV_STRIDE_MAX_GRID, or by the test-only inr_debug_set(32, .)), nor on the stream, nor on the place in a batch.  All
// arithmetic is fp64; the fp32 entry converts y / weight / x0 at the load and rounds the result once.  The unit is compiled with
// -ffp-contract=off (_build.py), so the two entries agree bit for bit in their fp64 state.  No operator, weight or datum VALUE reaches
// an index: a NaN anywhere gives NaNs and no fault.
//
// The Huber function, the block maximum, the grids, the refusals of the scalar parameters and the finish kernel are tv_shared.h's.
#include "gemm_f64.h"
#include "tv_shared.h"

namespace inr {
namespace {

constexpr int OP_THREADS = 256;
constexpr int OP_MAX_SIDE = INR_TVSR_MAX_SIDE;

struct OpShape {
    int H, W, h, w;
    int th_r, th_c, tl_r, tl_c;   // 64 x 64 tiles of the HR image and of the LR image
    int TH, TL;                   // th_r th_c, tl_r tl_c
};

// the workspace: tau (and c0 c1 beside it), the state x | xbar | p0 | p1 of every image, q [n][h][w], the plane mid [n][h][W] between
// the two contractions of either direction, the energy partials [n][TL + TH] (data per LR tile, then prior per HR tile) and the change
// partials [n][TH].  Every region is rounded up to 16 bytes.  base == null: `total` only
struct OpView {
    double *tau, *state, *q, *mid, *epart, *chpart;
    size_t total;
};
OpView op_view(int n, const OpShape& s, void* base) {
    OpView v;
    WsCarver c(base, 16);
    const size_t nn = (size_t)(n > 0 ? n : 1), HW = (size_t)s.H * s.W;
    v.tau = c.take<double>(2);
    v.state = c.take<double>(nn * 4 * HW);
    v.q = c.take<double>(nn * (size_t)s.h * s.w);
    v.mid = c.take<double>(nn * (size_t)s.h * s.W);
    v.epart = c.take<double>(nn * (size_t)(s.TL + s.TH));
    v.chpart = c.take<double>(nn * (size_t)s.TH);
    v.total = c.bytes();
    return v;
}

// ---- the contraction: C [M][N] = A [M][K] B [K][N] per image, operands by strides (a batch stride of 0 shares an operator) --------------
struct OpGemm {
    long long M;
    int N, K;
    long long a_batch, a_row, a_k;
    long long b_batch, b_k, b_col;
    int tiles_r, tiles_c;
    long long items;   // n tiles_r tiles_c
};

// item = (image, tile row, tile column) flattened in that order; an epilogue has begin() before a tile, (row, col, image, value) per
// element and end(item, red) after it, the last two called by every thread of the block
template <class XA, class XB, class Epi>
__global__ void __launch_bounds__(OP_THREADS) op_gemm_kernel(const double* __restrict__ A, const double* __restrict__ B, OpGemm g, Epi epi) {
    __shared__ double As[GF_KS][GF_PITCH];   // [k][row]
    __shared__ double Bs[GF_KS][GF_PITCH];   // [k][column]
    __shared__ double red[OP_THREADS / 64];
    const int per = g.tiles_r * g.tiles_c;
    for (long long item = blockIdx.x; item < g.items; item += gridDim.x) {
        const long long img = item / per;
        const int tile = (int)(item - img * per), tr = tile / g.tiles_c, tc = tile - tr * g.tiles_c;
        epi.begin();
        gf_tile<XA, XB>(As, Bs, A + img * g.a_batch, g.a_row, g.a_k, B + img * g.b_batch, g.b_k, g.b_col, (long long)tr * GF_TILE,
                        tc * GF_TILE, g.M, g.N, g.K, (int)img, epi);
        epi.end(item, red);
    }
}

// a plain store: C [n][M][N]
struct OpStore {
    double* C;
    long long c_batch, c_row;
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void operator()(long long row, int col, int b, double v) const { C[b * c_batch + row * c_row + col] = v; }
    __device__ __forceinline__ void end(long long, double*) {}
};

// launch 3: the dual update of the data term at the element's own q
template <typename T>
struct OpDualData {
    double* q;
    const T *y, *weight;
    const double* tau;
    long long hw;
    int w;
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void operator()(long long row, int col, int b, double u) const {
        const long long d = b * hw + row * w + col;
        const double wv = weight ? (double)weight[d] : 1.0;
        double qn = 0.0;
        if (wv > 0.0) {
            const double sigma = *tau;
            qn = (q[d] + sigma * (u - (double)y[d])) / (1.0 + sigma / wv);
        }
        q[d] = qn;
    }
    __device__ __forceinline__ void end(long long, double*) {}
};

// launch 5: the primal update at the element's own x and xbar; p is read-only
struct OpPrimal {
    double* state;
    const double* tau;
    double* chpart;
    int H, W, last;
    double ch;
    __device__ __forceinline__ void begin() { ch = 0.0; }
    __device__ __forceinline__ void operator()(long long row, int col, int b, double a) {
        const long long HW = (long long)H * W, e = row * W + col;
        double* x = state + b * 4 * HW;
        double* xbar = x + HW;
        const double* p0 = xbar + HW;
        const double* p1 = p0 + HW;
        double d = 0.0;
        if (row + 1 < H) d += p0[e];
        if (row > 0) d -= p0[e - W];
        if (col + 1 < W) d += p1[e];
        if (col > 0) d -= p1[e - 1];
        const double xo = x[e];
        const double xn = xo - *tau * (a - d);
        xbar[e] = 2.0 * xn - xo;
        x[e] = xn;
        ch = fmax(ch, fabs(xn - xo));
    }
    __device__ __forceinline__ void end(long long item, double* red) {
        if (!last) return;                       // uniform over the launch
        const double m = block_max_f64(ch, red);
        if (threadIdx.x == 0) chpart[item] = m;
    }
};

// final: 1/2 w (u - y)^2 of the tile into its partial; parts = TL + TH per image, the LR tiles first
template <typename T>
struct OpEnergy {
    const T *y, *weight;
    double* epart;
    long long hw;
    int w, TL, parts;
    double en;
    __device__ __forceinline__ void begin() { en = 0.0; }
    __device__ __forceinline__ void operator()(long long row, int col, int b, double u) {
        const long long d = b * hw + row * w + col;
        const double wv = weight ? (double)weight[d] : 1.0;
        if (wv > 0.0) {
            const double res = u - (double)y[d];
            en += 0.5 * wv * res * res;
        }
    }
    __device__ __forceinline__ void end(long long item, double* red) {
        const double s = block_sum_f64(en, red);
        const long long img = item / TL;
        if (threadIdx.x == 0) epart[img * parts + (item - img * TL)] = s;
    }
};

// the back-projection: the numerator into x, then x = xbar = x / denominator where that is > 0, else 0
struct OpSetX {
    double* state;
    int H, W;
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void operator()(long long row, int col, int b, double v) const {
        state[b * 4 * ((long long)H * W) + row * W + col] = v;
    }
    __device__ __forceinline__ void end(long long, double*) {}
};
struct OpNormX {
    double* state;
    int H, W;
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void operator()(long long row, int col, int b, double den) const {
        const long long HW = (long long)H * W, e = row * W + col;
        double* x = state + b * 4 * HW;
        const double val = den > 0.0 ? x[e] / den : 0.0;
        x[e] = val;
        x[HW + e] = val;
    }
    __device__ __forceinline__ void end(long long, double*) {}
};

// ---- the thread-per-element kernels -------------------------------------------------------------------------------------------------
// tau[0] = 1 / sqrt(8 + c0 c1), tau[1] = c0 c1.  One workgroup: thread t sums rows (columns) t, t + 256, ... of |R|, each in ascending
// index, and keeps the largest
__device__ double op_norm_bound(const double* __restrict__ R, int m, int n, double* red) {
    double rmax = 0.0, cmax = 0.0;
    for (int i = threadIdx.x; i < m; i += OP_THREADS) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += fabs(R[(size_t)i * n + j]);
        rmax = fmax(rmax, s);
    }
    for (int j = threadIdx.x; j < n; j += OP_THREADS) {
        double s = 0.0;
        for (int i = 0; i < m; ++i) s += fabs(R[(size_t)i * n + j]);
        cmax = fmax(cmax, s);
    }
    rmax = block_max_f64(rmax, red);
    cmax = block_max_f64(cmax, red);
    return rmax * cmax;
}
__global__ void __launch_bounds__(OP_THREADS) op_step_kernel(double* __restrict__ tau, const double* __restrict__ R0,
                                                             const double* __restrict__ R1, OpShape s) {
    __shared__ double red[OP_THREADS / 64];
    const double c0 = op_norm_bound(R0, s.h, s.H, red);
    const double c1 = op_norm_bound(R1, s.w, s.W, red);
    if (threadIdx.x == 0) {
        tau[0] = 1.0 / sqrt(8.0 + c0 * c1);
        tau[1] = c0 * c1;
    }
}

// HR pixels: p = 0 and, with x0, x = xbar = x0.  LR data: q = 0 with x0, else u y for the back-projection
template <typename T>
__global__ void __launch_bounds__(OP_THREADS) op_init_kernel(OpView v, const T* __restrict__ y, const T* __restrict__ weight,
                                                             const T* __restrict__ x0, long long n, OpShape s) {
    const long long HW = (long long)s.H * s.W, n_pix = n * HW, total = n_pix + n * s.h * s.w;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        if (t < n_pix) {
            const long long img = t / HW, e = t - img * HW;
            double* x = v.state + img * 4 * HW;
            if (x0) {
                const double val = (double)x0[t];
                x[e] = val;
                x[HW + e] = val;
            }
            x[2 * HW + e] = 0.0;
            x[3 * HW + e] = 0.0;
        } else {
            const long long d = t - n_pix;
            double val = 0.0;
            if (!x0 && (!weight || (double)weight[d] > 0.0)) val = (double)y[d];
            v.q[d] = val;
        }
    }
}

// q = u = [w > 0] (mask) or 0
template <typename T>
__global__ void __launch_bounds__(OP_THREADS) op_fill_kernel(double* __restrict__ q, const T* __restrict__ weight, long long total, int mask) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x; d < total; d += stride)
        q[d] = mask && (!weight || (double)weight[d] > 0.0) ? 1.0 : 0.0;
}

__global__ void __launch_bounds__(OP_THREADS) op_dual_kernel(OpView v, long long n, OpShape s, double lam, double alpha) {
    const long long HW = (long long)s.H * s.W, total = n * HW;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const double sigma = v.tau[0], den = 1.0 + sigma * alpha / lam;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const long long img = t / HW;
        const int e = (int)(t - img * HW), i = e / s.W, j = e - i * s.W;
        const double* xbar = v.state + img * 4 * HW + HW;
        double* p0 = v.state + img * 4 * HW + 2 * HW;
        double* p1 = p0 + HW;
        const double xb = xbar[e];
        const double g0 = i + 1 < s.H ? xbar[e + s.W] - xb : 0.0;
        const double g1 = j + 1 < s.W ? xbar[e + 1] - xb : 0.0;
        double q0 = (p0[e] + sigma * g0) / den;
        double q1 = (p1[e] + sigma * g1) / den;
        const double nrm = sqrt(q0 * q0 + q1 * q1) / lam;
        if (nrm > 1.0) {
            q0 /= nrm;
            q1 /= nrm;
        }
        p0[e] = q0;
        p1[e] = q1;
    }
}

// an HR tile: the result, rounded once to the caller's type, and the tile's share of the prior
template <typename T>
__global__ void __launch_bounds__(OP_THREADS) op_final_hr_kernel(T* __restrict__ out, OpView v, long long n, OpShape s, double lam,
                                                                 double alpha) {
    __shared__ double red[OP_THREADS / 64];
    const int tid = threadIdx.x, parts = s.TL + s.TH;
    const long long HW = (long long)s.H * s.W;
    for (long long item = blockIdx.x; item < n * s.TH; item += gridDim.x) {
        const long long img = item / s.TH;
        const int tile = (int)(item - img * s.TH), tr = tile / s.th_c, tc = tile - tr * s.th_c;
        const double* x = v.state + img * 4 * HW;
        double reg = 0.0;
        for (int r = 0; r < GF_TILE * GF_TILE / OP_THREADS; ++r) {
            const int local = r * OP_THREADS + tid, i = tr * GF_TILE + local / GF_TILE, j = tc * GF_TILE + (local & (GF_TILE - 1));
            if (i >= s.H || j >= s.W) continue;
            const long long e = (long long)i * s.W + j;
            const double xe = x[e];
            out[img * HW + e] = (T)xe;
            if (lam > 0.0) {
                const double g0 = i + 1 < s.H ? x[e + s.W] - xe : 0.0;
                const double g1 = j + 1 < s.W ? x[e + 1] - xe : 0.0;
                reg += tv_huber(sqrt(g0 * g0 + g1 * g1), alpha);
            }
        }
        reg = block_sum_f64(reg, red);
        if (tid == 0) v.epart[img * parts + s.TL + tile] = lam > 0.0 ? lam * reg : 0.0;
    }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------
int op_shape_check(const char* who, int n, int H, int W, int h, int w, OpShape* s) {
    INR_REQUIRE(n >= 0, INR_E_INVALID, "%s: bad sizes (n_images = %d)", who, n);
    INR_REQUIRE(H >= 1 && W >= 1 && H <= OP_MAX_SIDE && W <= OP_MAX_SIDE, INR_E_INVALID,
                "%s: bad sizes (height and width are 1 .. %d, got %d x %d)", who, OP_MAX_SIDE, H, W);
    INR_REQUIRE(h >= 1 && w >= 1 && h <= OP_MAX_SIDE && w <= OP_MAX_SIDE, INR_E_INVALID,
                "%s: bad sizes (lr_height and lr_width are 1 .. %d, got %d x %d)", who, OP_MAX_SIDE, h, w);
    OpShape v{H, W, h, w, (H + GF_TILE - 1) / GF_TILE, (W + GF_TILE - 1) / GF_TILE, (h + GF_TILE - 1) / GF_TILE, (w + GF_TILE - 1) / GF_TILE, 0, 0};
    v.TH = v.th_r * v.th_c;   // <= 256
    v.TL = v.tl_r * v.tl_c;
    *s = v;
    return 0;
}

template <class XA, class XB, class Epi>
int op_gemm(const double* A, const double* B, OpGemm g, int n, const Epi& epi, hipStream_t st) {
    g.items = (long long)n * g.tiles_r * g.tiles_c;
    hipLaunchKernelGGL((op_gemm_kernel<XA, XB, Epi>), dim3(tv_grid(g.items)), dim3(OP_THREADS), 0, st, A, B, g, epi);
    INR_LAUNCH_CHECK();
    return 0;
}

// launch 2: [n][h][W] = R0 [h][H] times in [n][H][W]
template <class Epi>
int op_rows(const double* R0, const double* in, int n, const OpShape& s, const Epi& epi, hipStream_t st) {
    return op_gemm<GfIdentity, GfIdentity>(R0, in, OpGemm{s.h, s.W, s.H, 0, s.H, 1, (long long)s.H * s.W, s.W, 1, s.tl_r, s.th_c, 0}, n, epi, st);
}
// launch 3: [n][h][w] = mid [n][h][W] times R1^T, R1 [w][W]
template <class Epi>
int op_cols(const double* mid, const double* R1, int n, const OpShape& s, const Epi& epi, hipStream_t st) {
    return op_gemm<GfIdentity, GfIdentity>(mid, R1, OpGemm{s.h, s.w, s.W, (long long)s.h * s.W, s.W, 1, 0, 1, s.W, s.tl_r, s.tl_c, 0}, n, epi, st);
}
// launch 4: [n][h][W] = r [n][h][w] times R1 [w][W]; XR transforms the operator
template <class XR, class Epi>
int op_cols_t(const double* r, const double* R1, int n, const OpShape& s, const Epi& epi, hipStream_t st) {
    return op_gemm<GfIdentity, XR>(r, R1, OpGemm{s.h, s.W, s.w, (long long)s.h * s.w, s.w, 1, 0, s.W, 1, s.tl_r, s.th_c, 0}, n, epi, st);
}
// launch 5: [n][H][W] = R0^T times mid [n][h][W]
template <class XR, class Epi>
int op_rows_t(const double* R0, const double* mid, int n, const OpShape& s, const Epi& epi, hipStream_t st) {
    return op_gemm<XR, GfIdentity>(R0, mid, OpGemm{s.H, s.W, s.h, 0, 1, s.H, (long long)s.h * s.W, s.W, 1, s.th_r, s.th_c, 0}, n, epi, st);
}

OpStore op_store_mid(const OpView& v, const OpShape& s) { return OpStore{v.mid, (long long)s.h * s.W, s.W}; }

int op_call_check(const char* who, const void* out, const void* in, const double* r0, const double* r1, int n, int H, int W, int h, int w,
                  const double* workspace, int64_t workspace_doubles, OpShape* s) {
    INR_REQUIRE(out && in, INR_E_INVALID, "%s: null pointer", who);
    INR_REQUIRE(r0 && r1, INR_E_INVALID, "%s: null pointer (r0 / r1)", who);
    if (int rc = op_shape_check(who, n, H, W, h, w, s)) return rc;
    return check_ws_doubles(who, workspace, workspace_doubles, op_view(n, *s, nullptr).total);
}

template <typename T>
int op_solve(const char* who, T* out, double* energy, double* change, const T* y, const T* weight, const T* x0, const double* r0,
             const double* r1, int n, int H, int W, int h, int w, double lam, double alpha, int n_iter, double* workspace,
             int64_t workspace_doubles, hipStream_t st) {
    INR_REQUIRE(out && y, INR_E_INVALID, "%s: null pointer", who);
    INR_REQUIRE(r0 && r1, INR_E_INVALID, "%s: null pointer (r0 / r1)", who);
    OpShape s;
    if (int rc = op_shape_check(who, n, H, W, h, w, &s)) return rc;
    if (int rc = tv_params_check(who, lam, alpha, n_iter, INR_TVSR3D_MAX_ITER)) return rc;
    if (int rc = check_ws_doubles(who, workspace, workspace_doubles, op_view(n, s, nullptr).total)) return rc;
    if (n == 0) return 0;
    const OpView v = op_view(n, s, workspace);
    const long long pixels = (long long)n * H * W, data = (long long)n * h * w;
    const double* xbar = v.state + (size_t)H * W;
    const long long img = 4ll * H * W;   // the state's stride from image to image
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL(op_step_kernel, dim3(1), dim3(OP_THREADS), 0, st, v.tau, r0, r1, s);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL((op_init_kernel<T>), dim3(tv_thread_grid(pixels + data, OP_THREADS)), dim3(OP_THREADS), 0, st, v, y, weight, x0, (long long)n, s);
    INR_LAUNCH_CHECK();
    if (!x0) {
        if (int rc = op_cols_t<GfAbs>(v.q, r1, n, s, op_store_mid(v, s), st)) return rc;
        if (int rc = op_rows_t<GfAbs>(r0, v.mid, n, s, OpSetX{v.state, H, W}, st)) return rc;
        hipLaunchKernelGGL((op_fill_kernel<T>), dim3(tv_thread_grid(data, OP_THREADS)), dim3(OP_THREADS), 0, st, v.q, weight, data, 1);
        INR_LAUNCH_CHECK();
        if (int rc = op_cols_t<GfAbs>(v.q, r1, n, s, op_store_mid(v, s), st)) return rc;
        if (int rc = op_rows_t<GfAbs>(r0, v.mid, n, s, OpNormX{v.state, H, W}, st)) return rc;
        hipLaunchKernelGGL((op_fill_kernel<T>), dim3(tv_thread_grid(data, OP_THREADS)), dim3(OP_THREADS), 0, st, v.q, weight, data, 0);
        INR_LAUNCH_CHECK();
    }
    OpGemm rows{s.h, s.W, s.H, 0, s.H, 1, img, s.W, 1, s.tl_r, s.th_c, 0};   // launch 2 on a field of the state: the image stride is 4 H W
    for (int it = 0; it < n_iter; ++it) {
        if (lam > 0.0) {
            hipLaunchKernelGGL(op_dual_kernel, dim3(tv_thread_grid(pixels, OP_THREADS)), dim3(OP_THREADS), 0, st, v, (long long)n, s, lam, alpha);
            INR_LAUNCH_CHECK();
        }
        if (int rc = op_gemm<GfIdentity, GfIdentity>(r0, xbar, rows, n, op_store_mid(v, s), st)) return rc;
        if (int rc = op_cols(v.mid, r1, n, s, OpDualData<T>{v.q, y, weight, v.tau, (long long)h * w, w}, st)) return rc;
        if (int rc = op_cols_t<GfIdentity>(v.q, r1, n, s, op_store_mid(v, s), st)) return rc;
        if (int rc = op_rows_t<GfIdentity>(r0, v.mid, n, s, OpPrimal{v.state, v.tau, v.chpart, H, W, (int)(it + 1 == n_iter), 0.0}, st)) return rc;
    }
    if (int rc = op_gemm<GfIdentity, GfIdentity>(r0, v.state, rows, n, op_store_mid(v, s), st)) return rc;
    if (int rc = op_cols(v.mid, r1, n, s, OpEnergy<T>{y, weight, v.epart, (long long)h * w, w, s.TL, s.TL + s.TH, 0.0}, st)) return rc;
    hipLaunchKernelGGL((op_final_hr_kernel<T>), dim3(tv_grid((long long)n * s.TH)), dim3(OP_THREADS), 0, st, out, v, (long long)n, s, lam,
                       alpha);
    INR_LAUNCH_CHECK();
    // the energy partials: data per LR tile, then prior per HR tile; the change partials are written in the last iteration only
    return tv_finish<OP_THREADS>(energy, change, nullptr, v.epart, s.TL + s.TH, v.chpart, n_iter > 0 ? s.TH : 0, nullptr, 1.0, n, st);
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_tvop_workspace_doubles(int n_images, int height, int width, int lr_height, int lr_width) {
    OpShape s;
    if (op_shape_check("inr_tvop_workspace_doubles", n_images, height, width, lr_height, lr_width, &s)) return 0;
    return (int64_t)(op_view(n_images, s, nullptr).total / sizeof(double));
}

int inr_tvop_apply(double* out, const double* in, const double* r0, const double* r1, int n_images, int height, int width, int lr_height,
                   int lr_width, double* workspace, int64_t workspace_doubles, void* stream) {
    OpShape s;
    if (int rc = op_call_check("inr_tvop_apply", out, in, r0, r1, n_images, height, width, lr_height, lr_width, workspace, workspace_doubles, &s))
        return rc;
    if (n_images == 0) return 0;
    const OpView v = op_view(n_images, s, workspace);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(KC_OTHER, st);
    if (int rc = op_rows(r0, in, n_images, s, op_store_mid(v, s), st)) return rc;
    return op_cols(v.mid, r1, n_images, s, OpStore{out, (long long)lr_height * lr_width, lr_width}, st);
}

int inr_tvop_adjoint(double* out, const double* in, const double* r0, const double* r1, int n_images, int height, int width, int lr_height,
                     int lr_width, double* workspace, int64_t workspace_doubles, void* stream) {
    OpShape s;
    if (int rc = op_call_check("inr_tvop_adjoint", out, in, r0, r1, n_images, height, width, lr_height, lr_width, workspace, workspace_doubles, &s))
        return rc;
    if (n_images == 0) return 0;
    const OpView v = op_view(n_images, s, workspace);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(KC_OTHER, st);
    if (int rc = op_cols_t<GfIdentity>(in, r1, n_images, s, op_store_mid(v, s), st)) return rc;
    return op_rows_t<GfIdentity>(r0, v.mid, n_images, s, OpStore{out, (long long)height * width, width}, st);
}

int inr_tvop_solve2d(double* out, double* energy, double* change, const double* y, const double* weight, const double* x0,
                     const double* r0, const double* r1, int n_images, int height, int width, int lr_height, int lr_width, double lambda,
                     double alpha, int n_iter, double* workspace, int64_t workspace_doubles, void* stream) {
    return op_solve("inr_tvop_solve2d", out, energy, change, y, weight, x0, r0, r1, n_images, height, width, lr_height, lr_width, lambda,
                    alpha, n_iter, workspace, workspace_doubles, (hipStream_t)stream);
}

int inr_tvop_solve2d_f32(float* out, double* energy, double* change, const float* y, const float* weight, const float* x0,
                         const double* r0, const double* r1, int n_images, int height, int width, int lr_height, int lr_width,
                         double lambda, double alpha, int n_iter, double* workspace, int64_t workspace_doubles, void* stream) {
    return op_solve("inr_tvop_solve2d_f32", out, energy, change, y, weight, x0, r0, r1, n_images, height, width, lr_height, lr_width,
                    lambda, alpha, n_iter, workspace, workspace_doubles, (hipStream_t)stream);
}

}  // extern "C"
