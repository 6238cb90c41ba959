// Fourier re-sampling of real lines and images: zero-filling k-space (up) and truncating it (down) -- the interpolation an MR scanner
// itself applies, and the baseline a DWI super-resolution result is judged against first.  DESIGN.md 4j; tests/fourier_common.py restates
// the operator in numpy and checks it against scipy.signal.resample.
//
//   y = A x,  A [m][n],  A[i][j] = (1/n) sum_{k = 0..K} c_k w(k) cos(2 pi k (p_i - j) / n),  L = min(n, m), K = floor(L/2),
//   p_i = i n/m + delta;  delta = 0 (INR_FOURIER_SAMPLE: sample 0 stays on sample 0, scipy.signal.resample) or (n/m - 1)/2
//   (INR_FOURIER_CENTER: pixel centres);  c_0 = 1, c_k = 2, and at k = L/2 of an even L: 1 when L == n (the input's Nyquist bin, split
//   between +n/2 and -n/2), 2 when L == m < n (both bins folded onto the output's Nyquist);  w = Tukey window over the kept band.
//   INR_FOURIER_MIRROR: the periodic operator E of the mirrored line, folded back onto the n samples, its first m rows:
//     SAMPLE: [x, x[n-2:0:-1]], period P = 2n - 2, E: P -> P m/n, A[:, j] = E[:, j] + E[:, P - j] for 0 < j < n - 1
//     CENTER: [x, x[::-1]],     period 2n,         E: 2n -> 2m,   A[:, j] = E[:, j] + E[:, 2n - 1 - j]
//
// The operator kernel forms one entry per thread: with q = 2 i En - 2 j Em (+ En - Em for CENTER) every phase is
// pi (k q mod 2 En Em) / (En Em), reduced exactly in int64 before cospi; the terms are added in ascending k, a mirror entry is the sum
// of its two cosine sums.  The apply kernel is a batched, strided fp64 GEMM on v_mfma_f64_16x16x4_f64 with a fixed K order and no
// atomics: calls are bit-equal.  All arithmetic is fp64; the fp32 entry point converts on load and rounds once on the last store.
#include <math.h>

#include "gemm_f64.h"
#include "internal.h"

namespace inr {
namespace {

constexpr int FOURIER_MAX_LINE = INR_FOURIER_MAX_LINE;
struct FourierView { double *op_rows, *op_cols, *mid; size_t total; };

constexpr int FR_TILE = GF_TILE;   // the block's output tile (gemm_f64.h)

// one axis: A [m][n] from the periodic operator E: En -> Em
struct FrAxis {
    int n, m;
    int En, Em;
    int center;    // q gains En - Em
    int fold;      // 0: none; 1: column En - j for 0 < j < n - 1 (whole-sample mirror); 2: column En - 1 - j (half-sample mirror)
    double apodize;
};

FrAxis fr_axis(int n, int m, int align, int boundary, double apodize) {
    FrAxis a{n, m, n, m, align == INR_FOURIER_CENTER, 0, apodize};
    if (boundary == INR_FOURIER_MIRROR) {
        if (a.center) {
            a.En = 2 * n, a.Em = 2 * m, a.fold = 2;
        } else {
            a.En = 2 * n - 2, a.Em = (int)((long long)(2 * n - 2) * m / n), a.fold = 1;
        }
    }
    return a;
}

// an axis whose data pass through bit for bit; the operator of a 1 -> 1 axis is [1] in every mode
bool fr_identity(int n, int m, int align, double apodize) {
    return n == m && (n == 1 || (align == INR_FOURIER_SAMPLE && apodize == 0.0));
}

// sum_{k = 0..K} c_k w(k) cos(pi (k q mod D) / (D/2)), D = 2 En Em, ascending k
__device__ double fr_cos_sum(long long q, long long D, int L, double nyquist, double alpha) {
    q %= D;
    if (q < 0) q += D;
    const double half = (double)(D / 2);
    double s = 0.0;
    for (int k = 0; k <= L / 2; ++k) {
        const double c = k == 0 ? 1.0 : (2 * k == L ? nyquist : 2.0);
        double w = 1.0;
        if (alpha > 0.0) {
            const double r = 2.0 * k / L;
            if (r > 1.0 - alpha) w = 0.5 * (1.0 + cospi((r - 1.0 + alpha) / alpha));
        }
        s += c * w * cospi((double)((k * q) % D) / half);
    }
    return s;
}

__global__ void __launch_bounds__(256) fr_operator_kernel(double* __restrict__ op, FrAxis a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.m * a.n) return;
    const long long i = idx / a.n, j = idx % a.n;
    const long long En = a.En, Em = a.Em, D = 2 * En * Em, off = a.center ? En - Em : 0;
    const int L = a.En < a.Em ? a.En : a.Em;
    const double nyquist = L == a.En ? 1.0 : 2.0;
    double s = fr_cos_sum(2 * En * i - 2 * Em * j + off, D, L, nyquist, a.apodize);
    if (a.fold == 1 && j > 0 && j < a.n - 1) s += fr_cos_sum(2 * En * i - 2 * Em * (En - j) + off, D, L, nyquist, a.apodize);
    if (a.fold == 2) s += fr_cos_sum(2 * En * i - 2 * Em * (En - 1 - j) + off, D, L, nyquist, a.apodize);
    op[idx] = s / (double)En;
}

// C [M][N] = A [M][K] B [K][N] per batch entry; A has k contiguous, C its columns; a batch stride of 0 shares the operand
struct FrGemm {
    long long M;
    int N, K, batch;
    long long a_batch, a_row;
    long long b_batch, b_k, b_col;
    long long c_batch, c_row;
};

// the plain store of an element, rounded once to the result's type
template <typename TC>
struct FrStore {
    TC* C;
    long long c_row;
    __device__ __forceinline__ void operator()(long long row, int col, int, double v) const { C[row * c_row + col] = (TC)v; }
};

// the tile loop is gf_tile (gemm_f64.h), shared with tvop.hip
template <typename TA, typename TB, typename TC>
__global__ void __launch_bounds__(256) fr_gemm_kernel(TC* __restrict__ C, const TA* __restrict__ A, const TB* __restrict__ B, FrGemm g) {
    __shared__ double As[GF_KS][GF_PITCH];   // [k][row]
    __shared__ double Bs[GF_KS][GF_PITCH];   // [k][column]
    const long long row0 = (long long)blockIdx.x * FR_TILE;
    const int col0 = blockIdx.y * FR_TILE;
    for (int b = blockIdx.z; b < g.batch; b += gridDim.z) {
        FrStore<TC> store{C + b * g.c_batch, g.c_row};
        gf_tile<GfIdentity, GfIdentity>(As, Bs, A + b * g.a_batch, g.a_row, 1, B + b * g.b_batch, g.b_k, g.b_col, row0, col0, g.M, g.N, g.K, b,
                                        store);
    }
}

template <typename TA, typename TB, typename TC>
int fr_gemm(TC* C, const TA* A, const TB* B, const FrGemm& g, hipStream_t st) {
    const dim3 grid((unsigned)((g.M + FR_TILE - 1) / FR_TILE), (unsigned)((g.N + FR_TILE - 1) / FR_TILE),
                    (unsigned)(g.batch < 65535 ? g.batch : 65535));
    hipLaunchKernelGGL((fr_gemm_kernel<TA, TB, TC>), grid, dim3(256), 0, st, C, A, B, g);
    INR_LAUNCH_CHECK();
    return 0;
}

// the last axis of [rows][n] -> [rows][m]: every line times op^T
template <typename TI, typename TO>
int fr_apply_last(TO* out, const TI* in, const double* op, long long rows, int n, int m, hipStream_t st) {
    return fr_gemm(out, in, op, FrGemm{rows, m, n, 1, 0, n, 0, 1, n, 0, m}, st);
}

// the second-last axis of [nimg][n][width] -> [nimg][m][width]: op times every image
template <typename TI, typename TO>
int fr_apply_rows(TO* out, const TI* in, const double* op, int nimg, int n, int m, int width, hipStream_t st) {
    return fr_gemm(out, op, in, FrGemm{m, width, n, nimg, 0, n, (long long)n * width, width, 1, (long long)m * width, width}, st);
}

// passes: a 1 -> 1 axis is passed through (fr_identity) and needs no mirrored line
int fr_axis_check(const char* who, int n, int m, int align, int boundary, bool passes) {
    INR_REQUIRE(n >= 1 && m >= 1, INR_E_INVALID, "%s: bad sizes (a line of %d samples to %d)", who, n, m);
    INR_REQUIRE(n <= FOURIER_MAX_LINE && m <= FOURIER_MAX_LINE, INR_E_INVALID, "%s: lines of at most %d samples (got %d -> %d)", who,
                FOURIER_MAX_LINE, n, m);
    if (boundary == INR_FOURIER_MIRROR && align == INR_FOURIER_SAMPLE && !(passes && n == 1 && m == 1))
        INR_REQUIRE(n >= 2 && ((long long)(2 * n - 2) * m) % n == 0, INR_E_INVALID,
                    "%s: the mirror boundary with align 'sample' needs n >= 2 and (2n - 2) m divisible by n (got %d -> %d)", who, n, m);
    return 0;
}

int fr_mode_check(const char* who, int align, int boundary, double apodize) {
    INR_REQUIRE(align == INR_FOURIER_SAMPLE || align == INR_FOURIER_CENTER, INR_E_INVALID,
                "%s: align must be INR_FOURIER_SAMPLE or INR_FOURIER_CENTER (got %d)", who, align);
    INR_REQUIRE(boundary == INR_FOURIER_PERIODIC || boundary == INR_FOURIER_MIRROR, INR_E_INVALID,
                "%s: boundary must be INR_FOURIER_PERIODIC or INR_FOURIER_MIRROR (got %d)", who, boundary);
    INR_REQUIRE(apodize >= 0.0 && apodize <= 1.0, INR_E_INVALID, "%s: apodize must be in [0, 1] (got %g)", who, apodize);
    return 0;
}

// validated by fourier_operator_check
int launch_fourier_operator(double* op, int n, int m, int align, int boundary, double apodize, hipStream_t st) {
    const long long total = (long long)m * n;
    hipLaunchKernelGGL(fr_operator_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, op, fr_axis(n, m, align, boundary, apodize));
    INR_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int fr_resample2d(T* out, const T* in, int nimg, int H, int W, int OH, int OW, int align, int boundary, double apodize,
                  const FourierView& v, hipStream_t st) {
    if (nimg == 0) return 0;
    ProfScope ps(KC_OTHER, st);
    const bool cols = !fr_identity(W, OW, align, apodize), rows = !fr_identity(H, OH, align, apodize);
    if (cols)
        if (int rc = launch_fourier_operator(v.op_cols, W, OW, align, boundary, apodize, st)) return rc;
    if (rows)
        if (int rc = launch_fourier_operator(v.op_rows, H, OH, align, boundary, apodize, st)) return rc;
    const long long lines = (long long)nimg * H;
    if (cols && rows) {
        if (int rc = fr_apply_last(v.mid, in, v.op_cols, lines, W, OW, st)) return rc;
        return fr_apply_rows(out, (const double*)v.mid, v.op_rows, nimg, H, OH, OW, st);
    }
    if (cols) return fr_apply_last(out, in, v.op_cols, lines, W, OW, st);
    if (rows) return fr_apply_rows(out, in, v.op_rows, nimg, H, OH, OW, st);
    INR_HIP(hipMemcpyAsync(out, in, (size_t)lines * W * sizeof(T), hipMemcpyDeviceToDevice, st));
    return 0;
}

// the workspace: the two operators and the plane between the two passes.  base == null: `total` only
FourierView fourier_view(int nimg, int H, int W, int OH, int OW, void* base) {
    FourierView v;
    WsCarver c(base, 256);
    v.op_rows = c.take<double>((size_t)OH * (size_t)H);
    v.op_cols = c.take<double>((size_t)OW * (size_t)W);
    v.mid = c.take<double>((size_t)(nimg > 0 ? nimg : 1) * (size_t)H * (size_t)OW);
    v.total = c.bytes();
    return v;
}

int fourier_sizes_check(const char* who, int nimg, int H, int W, int OH, int OW) {
    INR_REQUIRE(nimg >= 0, INR_E_INVALID, "%s: bad sizes (n_images = %d)", who, nimg);
    if (int rc = fr_axis_check(who, H, OH, INR_FOURIER_CENTER, INR_FOURIER_PERIODIC, true)) return rc;
    if (int rc = fr_axis_check(who, W, OW, INR_FOURIER_CENTER, INR_FOURIER_PERIODIC, true)) return rc;
    // the row tiles of one launch are a grid's x extent
    INR_REQUIRE((long long)nimg * (H > OH ? H : OH) < (1ll << 36), INR_E_INVALID, "%s: batch too large (%d images of %d rows)", who, nimg,
                H > OH ? H : OH);
    return 0;
}

int fourier_operator_check(const char* who, int n, int m, int align, int boundary, double apodize) {
    if (int rc = fr_mode_check(who, align, boundary, apodize)) return rc;
    return fr_axis_check(who, n, m, align, boundary, false);
}

int fourier_check(const char* who, int nimg, int H, int W, int OH, int OW, int align, int boundary, double apodize) {
    if (int rc = fr_mode_check(who, align, boundary, apodize)) return rc;
    if (int rc = fourier_sizes_check(who, nimg, H, W, OH, OW)) return rc;
    if (int rc = fr_axis_check(who, H, OH, align, boundary, true)) return rc;
    return fr_axis_check(who, W, OW, align, boundary, true);
}

// everything validated (fourier_check) and the workspace checked by the caller
int launch_fourier_resample2d(double* out, const double* in, int nimg, int H, int W, int OH, int OW, int align, int boundary,
                              double apodize, const FourierView& v, hipStream_t st) {
    return fr_resample2d(out, in, nimg, H, W, OH, OW, align, boundary, apodize, v, st);
}

int launch_fourier_resample2d(float* out, const float* in, int nimg, int H, int W, int OH, int OW, int align, int boundary,
                              double apodize, const FourierView& v, hipStream_t st) {
    return fr_resample2d(out, in, nimg, H, W, OH, OW, align, boundary, apodize, v, st);
}

// the arguments and the workspace of one re-sampling call, before any device work
int fourier_call_check(const char* who, const void* out, const void* in, int n_images, int height, int width, int out_height,
                       int out_width, int align, int boundary, double apodize, const double* workspace, int64_t workspace_doubles) {
    INR_REQUIRE(out && in, INR_E_INVALID, "%s: null pointer", who);
    if (int rc = fourier_check(who, n_images, height, width, out_height, out_width, align, boundary, apodize)) return rc;
    return check_ws_doubles(who, workspace, workspace_doubles, fourier_view(n_images, height, width, out_height, out_width, nullptr).total);
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int inr_fourier_operator(double* op, int n, int m, int align, int boundary, double apodize, void* stream) {
    INR_REQUIRE(op, INR_E_INVALID, "inr_fourier_operator: null pointer");
    if (int rc = fourier_operator_check("inr_fourier_operator", n, m, align, boundary, apodize)) return rc;
    return launch_fourier_operator(op, n, m, align, boundary, apodize, (hipStream_t)stream);
}

int64_t inr_fourier_resample_workspace_doubles(int n_images, int height, int width, int out_height, int out_width) {
    if (fourier_sizes_check("inr_fourier_resample_workspace_doubles", n_images, height, width, out_height, out_width)) return 0;
    return (int64_t)(fourier_view(n_images, height, width, out_height, out_width, nullptr).total / sizeof(double));
}

int inr_fourier_resample2d(double* out, const double* in, int n_images, int height, int width, int out_height, int out_width, int align,
                           int boundary, double apodize, double* workspace, int64_t workspace_doubles, void* stream) {
    if (int rc = fourier_call_check("inr_fourier_resample2d", out, in, n_images, height, width, out_height, out_width, align, boundary,
                                    apodize, workspace, workspace_doubles))
        return rc;
    return launch_fourier_resample2d(out, in, n_images, height, width, out_height, out_width, align, boundary, apodize,
                                     fourier_view(n_images, height, width, out_height, out_width, workspace), (hipStream_t)stream);
}

int inr_fourier_resample2d_f32(float* out, const float* in, int n_images, int height, int width, int out_height, int out_width,
                               int align, int boundary, double apodize, double* workspace, int64_t workspace_doubles, void* stream) {
    if (int rc = fourier_call_check("inr_fourier_resample2d_f32", out, in, n_images, height, width, out_height, out_width, align, boundary,
                                    apodize, workspace, workspace_doubles))
        return rc;
    return launch_fourier_resample2d(out, in, n_images, height, width, out_height, out_width, align, boundary, apodize,
                                     fourier_view(n_images, height, width, out_height, out_width, workspace), (hipStream_t)stream);
}

}  // extern "C"
