// Shift-tolerant SSIM (cSSIM) of the RAMS tree: multi-image-super-resolution/utils/loss.py:131-177 `ssim`, with
// tf.image.ssim's defaults written out (11 x 11 Gaussian window of sigma 1.5, 'VALID', K1 = 0.01, K2 = 0.03, max_val 65535,
// no sample-covariance correction).  For each label shift (i, j), with P the prediction cropped by `border`, L / M the
// c x c windows of label / mask at (i, j):  b = sum(L M - P M) / sum(M),  x = (P M + b) M = P M^2 + b M,  y = L M,
// s_ij = mean over the (c-10)^2 map of l * cs,
//     l  = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1),   cs = (2 G*(xy) - 2 mu_x mu_y + C2) / (G*(x^2 + y^2) - mu_x^2 - mu_y^2 + C2).
//
// Data flow.  A 'VALID' filter commutes with cropping, so everything that does not contain P is filtered ONCE on the full
// size x size image and read at offset (i, j):  Y1 = G*(LM), Y2 = G*(L^2 M^2), M1 = G*M, M2 = G*M^2, Y3 = G*(L M^2)
// (cssim_invariant_kernel).  The bias enters the moments polynomially, so it is applied after filtering; per shift only
//     A1 = G*(P M^2), A2 = G*(P L M^3), A3 = G*(P^2 M^4), A4 = G*(P M^3)
// are filtered (cssim_shift_kernel) and
//     mu_x = A1 + b M1,  mu_y = Y1,  G*(xy) = A2 + b Y3,  G*(x^2) = A3 + 2 b A4 + b^2 M2,  G*(y^2) = Y2.
// No power of the mask is folded (M^2 != M for a soft mask).  Every filter is separable: one 11-tap pass along the rows into
// LDS, one along the columns out of it, on 16 x 32 output tiles whose 26 x 42 inputs are staged in LDS.  Values reach 65535 and
// the variance terms cancel, so all arithmetic is fp64; every reduction has a fixed order (tile sums by a block tree, tiles
// and shifts by one thread in index order): repeated runs are bit-equal.
//
// Gradient (cssim_shift_kernel<true>, cssim_grad_filter_kernel, cssim_grad_finish_kernel): through the best shift only, as
// reduce_max does.  With f = l cs per map position and a = df/dmu_x, e = df/dG*(xy), d = df/dG*(x^2),
//     gx = G^T*a + y G^T*e + 2 x G^T*d            (G^T* = the 'full' correlation, (c-10)^2 -> c^2)
//     d ssim / d P_q = (1/N) [ gx_q M_q^2 - (M_q / tot) sum_p gx_p M_p ]            (the second term is the path through b).
#include "internal.h"

#include <cmath>

namespace inr {
namespace {

constexpr int KW = 11;                 // window taps
constexpr int TH = 16, TW = 32;        // output tile
constexpr int IH = TH + KW - 1, IW = TW + KW - 1;   // input tile 26 x 42
constexpr int IWP = IW + 1;            // staged row pitch: the row pass reads rows 43 apart conflict-free (fp32 and fp64)
constexpr int HP = TW + 1;             // pitch of the row-filtered image: the 4-doubles-apart writes of a half-wave spread to 2-way
constexpr int SEG = 4, NSEG = TW / SEG;   // the row pass: one lane = 4 adjacent outputs of one row (a sliding window of 14 inputs)
static_assert(IH * NSEG <= 256 && TH * TW == 2 * 256, "one work item per thread in the row pass, two outputs in the column pass");

struct GaussWin {
    double g[KW];
};

// The separable window on one tile for NM maps at once.  prod(row, col, v[NM]) gives the NM map values at position (row, col)
// of the staged 26 x 42 input tile (it may form them from fewer staged sources).  Row pass: thread t < 208 filters 4 adjacent
// outputs of input row t / 8 into h[NM][IH][HP]; column pass: thread t filters outputs (2 (t / 32) + {0, 1}, t % 32) -> out.
// The caller has synchronised after staging; h is free again after the caller's next barrier.
template <int NM, class Prod>
__device__ __forceinline__ void tile_filter(double (&out)[NM][2], const GaussWin& G, double* __restrict__ h, Prod prod) {
    const int t = threadIdx.x;
    if (t < IH * NSEG) {
        const int row = t / NSEG, c0 = (t % NSEG) * SEG;
        double o[NM][SEG];
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int s = 0; s < SEG; ++s) o[m][s] = 0.0;
#pragma unroll
        for (int k = 0; k < SEG + KW - 1; ++k) {
            double v[NM];
            prod(row, c0 + k, v);
#pragma unroll
            for (int s = 0; s < SEG; ++s) {
                if (k - s >= 0 && k - s < KW) {
#pragma unroll
                    for (int m = 0; m < NM; ++m) o[m][s] += G.g[k - s] * v[m];
                }
            }
        }
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int s = 0; s < SEG; ++s) h[(m * IH + row) * HP + c0 + s] = o[m][s];
    }
    __syncthreads();
    const int col = t & (TW - 1), r0 = (t / TW) * 2;
#pragma unroll
    for (int m = 0; m < NM; ++m) out[m][0] = out[m][1] = 0.0;
#pragma unroll
    for (int k = 0; k < KW + 1; ++k) {
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const double hv = h[(m * IH + r0 + k) * HP + col];
            if (k < KW) out[m][0] += G.g[k] * hv;
            if (k >= 1) out[m][1] += G.g[k - 1] * hv;
        }
    }
}

// inv[b][5][nf][nf], nf = size - 10: the window applied to LM, (LM)^2, M, M^2, L M^2 on the whole image
__global__ void __launch_bounds__(256) cssim_invariant_kernel(double* __restrict__ inv, const float* __restrict__ y_true,
                                                              const float* __restrict__ mask, int size, GaussWin G) {
    __shared__ float sL[IH * IWP], sM[IH * IWP];
    __shared__ double h[5 * IH * HP];
    const int nf = size - (KW - 1), ntx = (nf + TW - 1) / TW;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x % ntx, b = blockIdx.z;
    const float* yt = y_true + (long long)b * size * size;
    const float* mk = mask + (long long)b * size * size;
    for (int idx = threadIdx.x; idx < IH * IW; idx += 256) {
        const int r = idx / IW, q = idx - r * IW, gr = ty * TH + r, gq = tx * TW + q;
        const bool ok = gr < size && gq < size;
        sL[r * IWP + q] = ok ? yt[(long long)gr * size + gq] : 0.f;
        sM[r * IWP + q] = ok ? mk[(long long)gr * size + gq] : 0.f;
    }
    __syncthreads();
    double o[5][2];
    tile_filter<5>(o, G, h, [&](int r, int q, double* v) {
        const double l = sL[r * IWP + q], m = sM[r * IWP + q], lm = l * m;
        v[0] = lm;
        v[1] = lm * lm;
        v[2] = m;
        v[3] = m * m;
        v[4] = lm * m;
    });
    const int col = threadIdx.x & (TW - 1), r0 = (threadIdx.x / TW) * 2;
    const long long plane = (long long)nf * nf;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int orow = ty * TH + r0 + s, ocol = tx * TW + col;
        if (orow < nf && ocol < nf) {
#pragma unroll
            for (int m = 0; m < 5; ++m) inv[((long long)b * 5 + m) * plane + (long long)orow * nf + ocol] = o[m][s];
        }
    }
}

// tot[b][shift] = sum M, bias[b][shift] = sum(L M - P M) / tot over the c x c window; one block per (shift, image)
__global__ void __launch_bounds__(256) cssim_bias_kernel(double* __restrict__ bias, double* __restrict__ tot,
                                                         const float* __restrict__ y_true, const float* __restrict__ y_pred,
                                                         const float* __restrict__ mask, int size, int border) {
    __shared__ double red[4];
    const int ns = 2 * border + 1, c = size - 2 * border;
    const int si = blockIdx.x / ns, sj = blockIdx.x % ns, b = blockIdx.y;
    const float* yt = y_true + (long long)b * size * size;
    const float* yp = y_pred + (long long)b * size * size;
    const float* mk = mask + (long long)b * size * size;
    double sm = 0.0, sd = 0.0;
    for (int i = threadIdx.x; i < c * c; i += 256) {
        const int r = i / c, q = i - r * c;
        const double m = mk[(long long)(si + r) * size + sj + q];
        sm += m;
        sd += m * (double)yt[(long long)(si + r) * size + sj + q] - m * (double)yp[(long long)(border + r) * size + border + q];
    }
    sm = block_sum_f64(sm, red);
    sd = block_sum_f64(sd, red);
    if (threadIdx.x == 0) {
        tot[(long long)b * ns * ns + blockIdx.x] = sm;
        bias[(long long)b * ns * ns + blockIdx.x] = sd / sm;
    }
}

// !GRAD: grid (tiles, shifts, images); partial[b][shift][tile] = sum over the tile of l * cs.
//  GRAD: grid (tiles, 1, images) at shift arg[b]; dst = aed[b][3][n][n] = df/dmu_x, df/dG*(xy), df/dG*(x^2) per map position.
template <bool GRAD>
__global__ void __launch_bounds__(256) cssim_shift_kernel(double* __restrict__ dst, const float* __restrict__ y_true,
                                                          const float* __restrict__ y_pred, const float* __restrict__ mask,
                                                          const double* __restrict__ inv, const double* __restrict__ bias,
                                                          const int* __restrict__ arg, int size, int border, GaussWin G,
                                                          double c1, double c2) {
    __shared__ float sP[IH * IWP], sL[IH * IWP], sM[IH * IWP];
    __shared__ double h[4 * IH * HP];
    __shared__ double red[4];
    const int ns = 2 * border + 1, c = size - 2 * border, n = c - (KW - 1), nf = size - (KW - 1);
    const int ntx = (n + TW - 1) / TW;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x % ntx, b = blockIdx.z;
    const int shift = GRAD ? arg[b] : (int)blockIdx.y;
    const int si = shift / ns, sj = shift % ns;
    const float* yt = y_true + (long long)b * size * size;
    const float* yp = y_pred + (long long)b * size * size;
    const float* mk = mask + (long long)b * size * size;
    for (int idx = threadIdx.x; idx < IH * IW; idx += 256) {
        const int r = idx / IW, q = idx - r * IW, gr = ty * TH + r, gq = tx * TW + q;
        const bool ok = gr < c && gq < c;
        sP[r * IWP + q] = ok ? yp[(long long)(border + gr) * size + border + gq] : 0.f;
        sL[r * IWP + q] = ok ? yt[(long long)(si + gr) * size + sj + gq] : 0.f;
        sM[r * IWP + q] = ok ? mk[(long long)(si + gr) * size + sj + gq] : 0.f;
    }
    __syncthreads();
    double o[4][2];
    tile_filter<4>(o, G, h, [&](int r, int q, double* v) {
        const double p = sP[r * IWP + q], l = sL[r * IWP + q], m = sM[r * IWP + q];
        const double pm2 = p * m * m;
        v[0] = pm2;
        v[1] = pm2 * l * m;
        v[2] = pm2 * pm2;
        v[3] = pm2 * m;
    });
    const double bb = bias[(long long)b * ns * ns + shift];
    const int col = threadIdx.x & (TW - 1), r0 = (threadIdx.x / TW) * 2;
    const long long plane = (long long)nf * nf;
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int orow = ty * TH + r0 + s, ocol = tx * TW + col;
        if (orow < n && ocol < n) {
            const double* ib = inv + (long long)b * 5 * plane + (long long)(si + orow) * nf + sj + ocol;
            const double Y1 = ib[0], Y2 = ib[plane], M1 = ib[2 * plane], M2 = ib[3 * plane], Y3 = ib[4 * plane];
            const double mux = o[0][s] + bb * M1, muy = Y1;
            const double exy = o[1][s] + bb * Y3;
            const double exx = o[2][s] + bb * (2.0 * o[3][s] + bb * M2);
            const double dl = mux * mux + muy * muy + c1;
            const double l = (2.0 * mux * muy + c1) / dl;
            const double dc = exx + Y2 - mux * mux - muy * muy + c2;
            const double cs = (2.0 * exy - 2.0 * mux * muy + c2) / dc;
            if (!GRAD) {
                acc += l * cs;
            } else {
                double* ob = dst + (long long)b * 3 * n * n + (long long)orow * n + ocol;
                ob[0] = cs * (2.0 * muy - 2.0 * mux * l) / dl + l * (2.0 * mux * cs - 2.0 * muy) / dc;
                ob[(long long)n * n] = 2.0 * l / dc;
                ob[2ll * n * n] = -l * cs / dc;
            }
        }
    }
    if (!GRAD) {
        acc = block_sum_f64(acc, red);
        if (threadIdx.x == 0) dst[((long long)b * ns * ns + shift) * gridDim.x + blockIdx.x] = acc;
    }
}

// table[b][shift] = s_ij (tiles summed in index order, / count, the clear_only rescaling); out[b] = max over the shifts
// (the first best shift wins ties, NaN entries -- windows without a clear pixel -- are passed over), 1 - max when as_loss.
__global__ void __launch_bounds__(64) cssim_finish_kernel(double* __restrict__ out, int* __restrict__ arg, double* __restrict__ table,
                                                          const double* __restrict__ partial, const double* __restrict__ tot,
                                                          int ns2, int ntiles, double count, double clear, int clear_only,
                                                          int as_loss) {
    const int b = blockIdx.x;
    for (int k = threadIdx.x; k < ns2; k += 64) {
        const double* p = partial + ((long long)b * ns2 + k) * ntiles;
        double s = 0.0;
        for (int j = 0; j < ntiles; ++j) s += p[j];
        s /= count;
        if (clear_only) s = (s - 1.0) * tot[(long long)b * ns2 + k] / clear + 1.0;
        table[(long long)b * ns2 + k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double best = NAN;
        int at = 0;
        for (int k = 0; k < ns2; ++k) {
            const double v = table[(long long)b * ns2 + k];
            if (v == v && (!(best == best) || v > best)) {
                best = v;
                at = k;
            }
        }
        out[b] = as_loss ? 1.0 - best : best;
        if (arg) arg[b] = at;
    }
}

// gx[b][c][c] = G^T*a + y G^T*e + 2 x G^T*d at the best shift; gpart[b][tile] = sum over the tile of gx M
__global__ void __launch_bounds__(256) cssim_grad_filter_kernel(double* __restrict__ gx, double* __restrict__ gpart,
                                                                const double* __restrict__ aed, const float* __restrict__ y_true,
                                                                const float* __restrict__ y_pred, const float* __restrict__ mask,
                                                                const double* __restrict__ bias, const int* __restrict__ arg,
                                                                int size, int border, GaussWin G) {
    __shared__ double sA[3 * IH * IWP];
    __shared__ double h[3 * IH * HP];
    __shared__ double red[4];
    const int ns = 2 * border + 1, c = size - 2 * border, n = c - (KW - 1);
    const int ntx = (c + TW - 1) / TW;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x % ntx, b = blockIdx.z;
    const int shift = arg[b], si = shift / ns, sj = shift % ns;
    const double* ab = aed + (long long)b * 3 * n * n;
    for (int idx = threadIdx.x; idx < IH * IW; idx += 256) {
        const int r = idx / IW, q = idx - r * IW;
        const int mr = ty * TH + r - (KW - 1), mq = tx * TW + q - (KW - 1);   // the map zero-padded by 10 on every side
        const bool ok = mr >= 0 && mr < n && mq >= 0 && mq < n;
#pragma unroll
        for (int m = 0; m < 3; ++m) sA[(m * IH + r) * IWP + q] = ok ? ab[((long long)m * n + mr) * n + mq] : 0.0;
    }
    __syncthreads();
    double o[3][2];
    tile_filter<3>(o, G, h, [&](int r, int q, double* v) {
#pragma unroll
        for (int m = 0; m < 3; ++m) v[m] = sA[(m * IH + r) * IWP + q];
    });
    const double bb = bias[(long long)b * ns * ns + shift];
    const float* yt = y_true + (long long)b * size * size;
    const float* yp = y_pred + (long long)b * size * size;
    const float* mk = mask + (long long)b * size * size;
    const int col = threadIdx.x & (TW - 1), r0 = (threadIdx.x / TW) * 2;
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int prow = ty * TH + r0 + s, pcol = tx * TW + col;
        if (prow < c && pcol < c) {
            const double p = yp[(long long)(border + prow) * size + border + pcol];
            const double l = yt[(long long)(si + prow) * size + sj + pcol];
            const double m = mk[(long long)(si + prow) * size + sj + pcol];
            const double x = (p * m + bb) * m, y = l * m;
            const double g = o[0][s] + y * o[1][s] + 2.0 * x * o[2][s];
            gx[((long long)b * c + prow) * c + pcol] = g;
            acc += g * m;
        }
    }
    acc = block_sum_f64(acc, red);
    if (threadIdx.x == 0) gpart[(long long)b * gridDim.x + blockIdx.x] = acc;
}

// grad[b] = -upstream[b] * scale / N * (gx M^2 - (M / tot) sum_p gx_p M_p) inside the cropped window, 0 on the border frame;
// scale = tot / c^2 under clear_only, else 1
__global__ void __launch_bounds__(256) cssim_grad_finish_kernel(float* __restrict__ grad, const double* __restrict__ gx,
                                                                const double* __restrict__ gpart, const double* __restrict__ tot,
                                                                const float* __restrict__ mask, const int* __restrict__ arg,
                                                                const float* __restrict__ upstream, int size, int border,
                                                                int ntiles, double count, int clear_only) {
    __shared__ double s_sum;
    const int ns = 2 * border + 1, c = size - 2 * border, b = blockIdx.y;
    const int shift = arg[b], si = shift / ns, sj = shift % ns;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int j = 0; j < ntiles; ++j) s += gpart[(long long)b * ntiles + j];
        s_sum = s;
    }
    __syncthreads();
    const double T = tot[(long long)b * ns * ns + shift];
    const double scale = clear_only ? T / ((double)c * (double)c) : 1.0;
    const double coef = -(upstream ? (double)upstream[b] : 1.0) * scale / count;
    const double through_bias = s_sum / T;
    const float* mk = mask + (long long)b * size * size;
    float* gr = grad + (long long)b * size * size;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < size * size; i += gridDim.x * 256) {
        const int r = i / size - border, q = i % size - border;
        float val = 0.f;
        if (r >= 0 && r < c && q >= 0 && q < c) {
            const double m = mk[(long long)(si + r) * size + sj + q];
            val = (float)(coef * (gx[((long long)b * c + r) * c + q] * m * m - m * through_bias));
        }
        gr[i] = val;
    }
}

GaussWin gauss_window() {   // tf.image.ssim: filter_size 11, filter_sigma 1.5, normalised to sum 1
    GaussWin w;
    double sum = 0.0;
    for (int k = 0; k < KW; ++k) {
        const double d = (double)(k - KW / 2);
        w.g[k] = std::exp(-d * d / (2.0 * 1.5 * 1.5));
        sum += w.g[k];
    }
    for (int k = 0; k < KW; ++k) w.g[k] /= sum;
    return w;
}

int tiles_of(int rows, int cols) { return ((rows + TH - 1) / TH) * ((cols + TW - 1) / TW); }

// the workspace, carved in doubles with no padding; the per-shift table comes first (callers may read it back).  ws == null: `total` only
struct CssimPlan {
    double *table, *bias, *tot, *partial, *inv, *aed, *gx, *gpart;
    int* arg;
    size_t total;   // doubles
};

CssimPlan cssim_plan(int nimg, int size, int border, bool grad, double* ws) {
    const size_t B = (size_t)(nimg > 0 ? nimg : 1);
    const size_t ns2 = (size_t)(2 * border + 1) * (2 * border + 1);
    const int c = size - 2 * border, n = c - (KW - 1), nf = size - (KW - 1);
    CssimPlan p{};
    WsCarver cv(ws, sizeof(double));
    p.table = cv.take<double>(B * ns2);
    p.bias = cv.take<double>(B * ns2);
    p.tot = cv.take<double>(B * ns2);
    p.partial = cv.take<double>(B * ns2 * (size_t)tiles_of(n, n));
    p.inv = cv.take<double>(B * 5 * (size_t)nf * nf);
    if (grad) {
        p.aed = cv.take<double>(B * 3 * (size_t)n * n);
        p.gx = cv.take<double>(B * (size_t)c * c);
        p.gpart = cv.take<double>(B * (size_t)tiles_of(c, c));
        p.arg = cv.take<int>(B);
    }
    p.total = cv.bytes() / sizeof(double);
    return p;
}

int cssim_forward(double* out, int* arg, const float* y_true, const float* y_pred, const float* mask, int nimg, int size,
                  int border, int clear_only, int as_loss, const CssimPlan& p, const GaussWin& G, hipStream_t st) {
    const int ns = 2 * border + 1, c = size - 2 * border, n = c - (KW - 1), nf = size - (KW - 1);
    const double c1 = (0.01 * 65535.0) * (0.01 * 65535.0), c2 = (0.03 * 65535.0) * (0.03 * 65535.0);
    hipLaunchKernelGGL(cssim_invariant_kernel, dim3(tiles_of(nf, nf), 1, nimg), dim3(256), 0, st, p.inv, y_true, mask, size, G);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(cssim_bias_kernel, dim3(ns * ns, nimg), dim3(256), 0, st, p.bias, p.tot, y_true, y_pred, mask, size,
                       border);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(cssim_shift_kernel<false>, dim3(tiles_of(n, n), ns * ns, nimg), dim3(256), 0, st, p.partial, y_true,
                       y_pred, mask, p.inv, p.bias, (const int*)nullptr, size, border, G, c1, c2);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(cssim_finish_kernel, dim3(nimg), dim3(64), 0, st, out, arg, p.table, p.partial, p.tot, ns * ns,
                       tiles_of(n, n), (double)n * (double)n, (double)c * (double)c, clear_only, as_loss);
    INR_LAUNCH_CHECK();
    return 0;
}

int cssim_min_crop() { return KW; }   // the cropped window must hold one 11 x 11 filter window

size_t cssim_workspace_doubles(int nimg, int size, int border, bool grad) { return cssim_plan(nimg, size, border, grad, nullptr).total; }

int launch_cssim(double* out, const float* y_true, const float* y_pred, const float* mask, int nimg, int size, int border,
                 int clear_only, double* ws, hipStream_t st) {
    const CssimPlan p = cssim_plan(nimg, size, border, false, ws);
    const GaussWin G = gauss_window();
    ProfScope ps(KC_OTHER, st);
    return cssim_forward(out, nullptr, y_true, y_pred, mask, nimg, size, border, clear_only, 0, p, G, st);
}

int launch_cssim_grad(double* loss, float* grad, const float* y_true, const float* y_pred, const float* mask,
                      const float* upstream, int nimg, int size, int border, int clear_only, double* ws, hipStream_t st) {
    const CssimPlan p = cssim_plan(nimg, size, border, true, ws);
    const GaussWin G = gauss_window();
    const int c = size - 2 * border, n = c - (KW - 1);
    const double c1 = (0.01 * 65535.0) * (0.01 * 65535.0), c2 = (0.03 * 65535.0) * (0.03 * 65535.0);
    int* arg = p.arg;
    ProfScope ps(KC_OTHER, st);
    if (int rc = cssim_forward(loss, arg, y_true, y_pred, mask, nimg, size, border, clear_only, 1, p, G, st)) return rc;
    hipLaunchKernelGGL(cssim_shift_kernel<true>, dim3(tiles_of(n, n), 1, nimg), dim3(256), 0, st, p.aed, y_true, y_pred, mask,
                       p.inv, p.bias, arg, size, border, G, c1, c2);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(cssim_grad_filter_kernel, dim3(tiles_of(c, c), 1, nimg), dim3(256), 0, st, p.gx, p.gpart,
                       p.aed, y_true, y_pred, mask, p.bias, arg, size, border, G);
    INR_LAUNCH_CHECK();
    const int blocks = (size * size + 255) / 256 < 1024 ? (size * size + 255) / 256 : 1024;
    hipLaunchKernelGGL(cssim_grad_finish_kernel, dim3(blocks, nimg), dim3(256), 0, st, grad, p.gx, p.gpart, p.tot,
                       mask, arg, upstream, size, border, tiles_of(c, c), (double)n * (double)n, clear_only);
    INR_LAUNCH_CHECK();
    return 0;
}

int shift_ssim_args_ok(const char* who, int n_images, int size, int border) {
    INR_REQUIRE(n_images >= 1 && n_images <= 65535 && border >= 0 && border <= 16 && size <= 8192 &&
                    size - 2 * border >= cssim_min_crop(),
                INR_E_INVALID, "%s: bad arguments (n_images=%d size=%d border=%d; size - 2*border >= %d)", who, n_images, size,
                border, cssim_min_crop());
    return 0;
}

size_t shift_ssim_bytes(int n_images, int size, int border, bool grad) {
    if (border < 0 || border > 16 || size > 8192 || size - 2 * border < cssim_min_crop()) return 0;
    return cssim_workspace_doubles(n_images, size, border, grad) * sizeof(double);
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

size_t inr_rams_shift_ssim_workspace_bytes(int n_images, int size, int border) {
    return shift_ssim_bytes(n_images, size, border, false);
}

int inr_rams_shift_ssim(double* out, const float* y_true, const float* y_pred, const float* mask, int n_images, int size,
                        int border, int clear_only, void* workspace, size_t workspace_bytes, void* stream) {
    INR_REQUIRE(out && y_true && y_pred && mask, INR_E_INVALID, "inr_rams_shift_ssim: null pointer");
    if (int rc = shift_ssim_args_ok("inr_rams_shift_ssim", n_images, size, border)) return rc;
    INR_REQUIRE(workspace && workspace_bytes >= inr_rams_shift_ssim_workspace_bytes(n_images, size, border), INR_E_WORKSPACE,
                "inr_rams_shift_ssim: workspace too small");
    INR_REQUIRE(((uintptr_t)workspace & 7) == 0, INR_E_ALIGN, "inr_rams_shift_ssim: workspace must be 8-byte aligned");
    return launch_cssim(out, y_true, y_pred, mask, n_images, size, border, clear_only != 0, (double*)workspace,
                        (hipStream_t)stream);
}

size_t inr_rams_shift_ssim_grad_workspace_bytes(int n_images, int size, int border) {
    return shift_ssim_bytes(n_images, size, border, true);
}

int inr_rams_shift_ssim_grad(double* loss, float* grad_pred, const float* y_true, const float* y_pred, const float* mask,
                             const float* upstream, int n_images, int size, int border, int clear_only, void* workspace,
                             size_t workspace_bytes, void* stream) {
    INR_REQUIRE(loss && grad_pred && y_true && y_pred && mask, INR_E_INVALID, "inr_rams_shift_ssim_grad: null pointer");
    if (int rc = shift_ssim_args_ok("inr_rams_shift_ssim_grad", n_images, size, border)) return rc;
    INR_REQUIRE(workspace && workspace_bytes >= inr_rams_shift_ssim_grad_workspace_bytes(n_images, size, border), INR_E_WORKSPACE,
                "inr_rams_shift_ssim_grad: workspace too small");
    INR_REQUIRE(((uintptr_t)workspace & 7) == 0, INR_E_ALIGN, "inr_rams_shift_ssim_grad: workspace must be 8-byte aligned");
    return launch_cssim_grad(loss, grad_pred, y_true, y_pred, mask, upstream, n_images, size, border, clear_only != 0,
                             (double*)workspace, (hipStream_t)stream);
}

}  // extern "C"
