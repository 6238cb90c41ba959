// Second-order total generalized variation (TGV) super-resolution under the block operator: the model-based
// reconstruction of tvsr.hip with a prior that does not terrace smooth intensity.  An auxiliary vector field v = (v0, v1) [2][H][W]
// absorbs the smooth part of the gradient, so a ramp costs nothing and an edge still costs its jump (Bredies, Kunisch, Pock, SIIMS
// 2010; Knoll et al., MRM 2011):
//   E(x, v) = 1/2 sum_i w_i ((A x)_i - y_i)^2 + lam1 sum_j H_alpha(|(grad x)_j - v_j|) + lam0 sum_j |(Ev)_j|_F,  lam1 = lambda, lam0 = ratio lambda
// A, grad, div, H_alpha: tvsr.hip's (tv_block.h).  d0 / d1 are the forward differences along rows / columns that grad uses (zero last
// row / column), div0 / div1 their negative adjoints, Ev = (e00, e11, e01) = (d0 v0, d1 v1, (d1 v0 + d0 v1) / 2) the symmetrised
// derivative and |Ev|_F = sqrt(e00^2 + e11^2 + 2 e01^2) its Frobenius norm (the off-diagonal entry counts twice).
//
// THE STEP BOUND.  K(x, v) = (grad x - v, Ev).  |grad|^2 <= 8.  |E|^2 <= 8: |Ev|_F^2 <= |d0 v0|^2 + |d1 v1|^2 + (|d1 v0|^2 + |d0 v1|^2)
// (2 ((a + b) / 2)^2 <= a^2 + b^2), which is at most 4 |v0|^2 + 4 |v1|^2 + 4 |v0|^2 + 4 |v1|^2 -- every 1-D difference has norm^2 <= 4.
// With a = |x|, b = |v|: |K(x, v)|^2 <= (sqrt 8 a + b)^2 + 8 b^2 = 8 a^2 + 2 sqrt 8 a b + 9 b^2, the quadratic form of
// [[8, sqrt 8], [sqrt 8, 9]], whose largest eigenvalue is (17 + sqrt 33) / 2 = 11.4.  So |K|^2 <= 12 and tau = sigma = 1/sqrt(12) satisfy
// tau sigma |K|^2 <= 1.  Chambolle-Pock from x = xbar = x0, v = vbar = 0, p = 0, r = 0:
//   q   <- (p + sigma (grad(xbar) - vbar)) / (1 + sigma alpha / lam1);   n = |q| / lam1;    p <- n > 1 ? q / n : q
//   s   <- r + sigma E(vbar);                                            n = |s|_F / lam0;  r <- n > 1 ? s / n : s
//   u   <- x + tau div(p);  x' <- u - A^T(c (A u - y)),  c_i = tau w_i / (1 + tau w_i |k|^2)      (w = 0: the datum is never read)
//   v0' <- v0 + tau (p0 + div0 r00 + div1 r01);   v1' <- v1 + tau (p1 + div1 r11 + div0 r01)
//   xbar <- 2 x' - x;  vbar <- 2 v' - v;  x <- x';  v <- v'
// lambda = 0 skips both dual phases and the v update: p, r and v stay 0 and the iteration is the data-only one of tvsr.hip.  Where the
// expressions coincide with tvsr.hip's they keep its order of operations; the rest is fixed in tests/tgv_common.py, which this
// kernel follows operation by operation (the unit is compiled with -ffp-contract=off, _build.py).
//
// ONE launch solves a batch.  One workgroup of 1,024 threads owns one image and runs every iteration itself; workgroups share
// nothing: no cooperative launch, no grid barrier, no spin, no atomics; the grid is the batch, capped, with a stride loop.  The state
// of an image is x | xbar | v0 | v1 | vbar0 | vbar1 | p0 | p1 | r00 | r11 | r01, 11 H W doubles of the caller's workspace.  fp64
// throughout; the fp32 entry converts at load and rounds once at the store (out and v_out).
//
// WHERE THE BARRIERS SIT, AND WHY.  An iteration has two phases and a __syncthreads() after each:
//   phase                          reads (possibly other threads')                              reads and writes (its own only)
//   dual, thread per HR pixel e    xbar, vbar0, vbar1 at e, e + W, e + 1                         p0, p1, r00, r11, r01 at e
//   ---- barrier 1: every p and r of this iteration is written before any thread differences it
//   primal, item per LR block      p0, p1 at the pixels of its block and at e - W, e - 1         x, xbar at the pixels of ITS block
//                                                                                               (xbar holds u between its two passes)
//   primal, item per HR pixel e    p0, p1 at e; r00 at e, e - W; r11 at e, e - 1;                v0, v1, vbar0, vbar1 at e
//                                  r01 at e, e - W, e - 1
//   ---- barrier 2: every xbar and vbar of this iteration is written before the next dual phase differences it
// The ownership rule of tvsr.hip holds: in each phase a field is either read (possibly across threads) or written by its owner alone.
// The two kinds of primal item need no barrier between them: the block items write x and xbar only, the pixel items v and vbar
// only, and neither reads what the other writes.  The start and the last iteration end with the same barrier.
//
// energy: E at the returned fp64 (x, v); every thread adds its LR blocks and then its HR pixels in ascending order (the first-order
// terms into one sum, the second-order terms into another, scaled by lam1 and lam0 and added in that order), wave_sum adds the lanes,
// thread 0 the 16 waves in ascending order: tvsr.hip's order, no float atomics.  change: max |x' - x| of the last iteration, on x only.
//
// The start of x and xbar, the block items of the primal phase, the data term and the reduction of energy and change are tv_block.h's,
// the ones tvsr.hip runs (which is why lambda = 0 gives its bits); those helpers hold no barrier, the two of an iteration stand below.
#include "tv_block.h"

namespace inr {
namespace {

constexpr int TGV_FIELDS = 11;

template <typename T>
__global__ void __launch_bounds__(TV_THREADS) tgv_solve_kernel(T* out, T* v_out, double* energy, double* change, const T* y,
                                                               const T* weight, const T* x0, double* state, int n_images, TvShape s,
                                                               TvBlock kb, double lam1, double lam0, double alpha, int n_iter) {
    __shared__ double ks[TV_MAX_FACTOR * TV_MAX_FACTOR];
    __shared__ double red[TV_WAVES];
    const int tid = threadIdx.x;
    const int HW = s.H * s.W, hw = s.h * s.w, W = s.W;
    const double tau = 1.0 / sqrt(12.0), sigma = tau;
    if (tid < s.f0 * s.f1) ks[tid] = kb.k[tid];
    for (int img = blockIdx.x; img < n_images; img += gridDim.x) {
        double* x = state + (size_t)img * TGV_FIELDS * HW;
        double* xbar = x + HW;
        double* v0 = xbar + HW;
        double* v1 = v0 + HW;
        double* vbar0 = v1 + HW;
        double* vbar1 = vbar0 + HW;
        double* p0 = vbar1 + HW;
        double* p1 = p0 + HW;
        double* r00 = p1 + HW;
        double* r11 = r00 + HW;
        double* r01 = r11 + HW;
        const T* yi = y + (size_t)img * hw;
        const T* wi = weight ? weight + (size_t)img * hw : nullptr;
        const T* x0i = x0 ? x0 + (size_t)img * HW : nullptr;
        for (int e = tid; e < HW; e += TV_THREADS) {
            tv_start_pixel(x, xbar, x0i, yi, s, e);
            v0[e] = 0.0;
            v1[e] = 0.0;
            vbar0[e] = 0.0;
            vbar1[e] = 0.0;
            p0[e] = 0.0;
            p1[e] = 0.0;
            r00[e] = 0.0;
            r11[e] = 0.0;
            r01[e] = 0.0;
        }
        __syncthreads();   // the start is written (and ks, for the first image)
        double ch = 0.0;
        for (int it = 0; it < n_iter; ++it) {
            if (lam1 > 0.0) {
                const double den = 1.0 + sigma * alpha / lam1;
                for (int e = tid; e < HW; e += TV_THREADS) {
                    const int i = e / W, j = e - i * W;
                    const bool down = i + 1 < s.H, right = j + 1 < W;
                    const double xb = xbar[e], a0 = vbar0[e], a1 = vbar1[e];
                    const double g0 = down ? xbar[e + W] - xb : 0.0;
                    const double g1 = right ? xbar[e + 1] - xb : 0.0;
                    double q0 = (p0[e] + sigma * (g0 - a0)) / den;
                    double q1 = (p1[e] + sigma * (g1 - a1)) / den;
                    const double nrm = sqrt(q0 * q0 + q1 * q1) / lam1;
                    if (nrm > 1.0) {
                        q0 /= nrm;
                        q1 /= nrm;
                    }
                    p0[e] = q0;
                    p1[e] = q1;
                    const double e00 = down ? vbar0[e + W] - a0 : 0.0;
                    const double e11 = right ? vbar1[e + 1] - a1 : 0.0;
                    const double c01 = right ? vbar0[e + 1] - a0 : 0.0;
                    const double c10 = down ? vbar1[e + W] - a1 : 0.0;
                    const double e01 = (c01 + c10) / 2.0;
                    double s00 = r00[e] + sigma * e00;
                    double s11 = r11[e] + sigma * e11;
                    double s01 = r01[e] + sigma * e01;
                    const double nr = sqrt(s00 * s00 + s11 * s11 + 2.0 * (s01 * s01)) / lam0;
                    if (nr > 1.0) {
                        s00 /= nr;
                        s11 /= nr;
                        s01 /= nr;
                    }
                    r00[e] = s00;
                    r11[e] = s11;
                    r01[e] = s01;
                }
            }
            __syncthreads();   // barrier 1: p and r are complete
            const bool last = it + 1 == n_iter;
            for (int blk = tid; blk < hw; blk += TV_THREADS)   // the block items: tvsr.hip's step with u in place of v
                tv_primal_block(x, xbar, p0, p1, ks, s, kb.k2, yi, wi, blk, 1.0, tau, last, ch);
            if (lam1 > 0.0)
                for (int e = tid; e < HW; e += TV_THREADS) {
                    const int i = e / W, j = e - i * W;
                    const bool down = i + 1 < s.H, right = j + 1 < W, up = i > 0, left = j > 0;
                    double d00 = 0.0, d01 = 0.0, d11 = 0.0, d10 = 0.0;   // div0 r00, div1 r01, div1 r11, div0 r01
                    if (down) d00 += r00[e];
                    if (up) d00 -= r00[e - W];
                    if (right) d01 += r01[e];
                    if (left) d01 -= r01[e - 1];
                    if (right) d11 += r11[e];
                    if (left) d11 -= r11[e - 1];
                    if (down) d10 += r01[e];
                    if (up) d10 -= r01[e - W];
                    const double o0 = v0[e], o1 = v1[e];
                    const double n0 = o0 + tau * (p0[e] + d00 + d01);
                    const double n1 = o1 + tau * (p1[e] + d11 + d10);
                    vbar0[e] = 2.0 * n0 - o0;
                    vbar1[e] = 2.0 * n1 - o1;
                    v0[e] = n0;
                    v1[e] = n1;
                }
            __syncthreads();   // barrier 2: x, xbar, v and vbar are complete
        }
        // the objective at (x, v), the image and the field
        double en = 0.0;
        for (int blk = tid; blk < hw; blk += TV_THREADS) tv_add_data_term(en, x, ks, s, yi, wi, blk);
        double reg1 = 0.0, reg0 = 0.0;
        for (int e = tid; e < HW; e += TV_THREADS) {
            const int i = e / W, j = e - i * W;
            const double xe = x[e], a0 = v0[e], a1 = v1[e];
            out[(size_t)img * HW + e] = (T)xe;
            if (v_out) {
                v_out[((size_t)img * 2) * HW + e] = (T)a0;
                v_out[((size_t)img * 2 + 1) * HW + e] = (T)a1;
            }
            if (lam1 > 0.0) {
                const bool down = i + 1 < s.H, right = j + 1 < W;
                const double g0 = (down ? x[e + W] - xe : 0.0) - a0;
                const double g1 = (right ? x[e + 1] - xe : 0.0) - a1;
                reg1 += tv_huber(sqrt(g0 * g0 + g1 * g1), alpha);
                const double e00 = down ? v0[e + W] - a0 : 0.0;
                const double e11 = right ? v1[e + 1] - a1 : 0.0;
                const double c01 = right ? v0[e + 1] - a0 : 0.0;
                const double c10 = down ? v1[e + W] - a1 : 0.0;
                const double e01 = (c01 + c10) / 2.0;
                reg0 += sqrt(e00 * e00 + e11 * e11 + 2.0 * (e01 * e01));
            }
        }
        if (lam1 > 0.0) {
            en += lam1 * reg1;
            en += lam0 * reg0;
        }
        tv_store_energy_change(en, ch, red, energy, change, (size_t)img);   // ends with a barrier: red is free for the next image
    }
}

// the workspace: the 11 fields of every image.  base == null: `total` only
TvStateView tgv_view(int n_images, int H, int W, void* base) { return tv_state_view(n_images, TGV_FIELDS, H, W, base); }

template <typename T>
int tgv_solve(const char* who, T* out, T* v_out, double* energy, double* change, const T* y, const T* weight, const T* x0, int n_images,
              int H, int W, int f0, int f1, const double* kernel, double lam, double ratio, double alpha, int n_iter, double* workspace,
              int64_t workspace_doubles, hipStream_t st) {
    INR_REQUIRE(out && y, INR_E_INVALID, "%s: null pointer", who);
    TvShape s;
    TvBlock kb;
    if (int rc = tv_shape_check(who, n_images, H, W, f0, f1, &s)) return rc;
    if (int rc = tv_params_check(who, lam, alpha, n_iter, -1)) return rc;
    INR_REQUIRE(std::isfinite(ratio) && ratio > 0.0, INR_E_INVALID, "%s: ratio must be finite and > 0 (got %g)", who, ratio);
    if (int rc = tv_block_check(who, kernel, f0, f1, &kb)) return rc;
    if (int rc = check_ws_doubles(who, workspace, workspace_doubles, tgv_view(n_images, H, W, nullptr).total)) return rc;
    if (n_images == 0) return 0;
    const TvStateView v = tgv_view(n_images, H, W, workspace);
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL((tgv_solve_kernel<T>), dim3((unsigned)(n_images < TV_MAX_GRID ? n_images : TV_MAX_GRID)), dim3(TV_THREADS), 0, st,
                       out, v_out, energy, change, y, weight, x0, v.state, n_images, s, kb, lam, ratio * lam, alpha, n_iter);
    INR_LAUNCH_CHECK();
    return 0;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_tgv_workspace_doubles(int n_images, int height, int width) {
    TvShape s;
    if (tv_shape_check("inr_tgv_workspace_doubles", n_images, height, width, 1, 1, &s)) return 0;
    return (int64_t)(tgv_view(n_images, height, width, nullptr).total / sizeof(double));
}

int inr_tgv_solve2d(double* out, double* v_out, double* energy, double* change, const double* y, const double* weight, const double* x0,
                    int n_images, int height, int width, int f0, int f1, const double* kernel, double lambda, double ratio, double alpha,
                    int n_iter, double* workspace, int64_t workspace_doubles, void* stream) {
    return tgv_solve("inr_tgv_solve2d", out, v_out, energy, change, y, weight, x0, n_images, height, width, f0, f1, kernel, lambda, ratio,
                     alpha, n_iter, workspace, workspace_doubles, (hipStream_t)stream);
}

int inr_tgv_solve2d_f32(float* out, float* v_out, double* energy, double* change, const float* y, const float* weight, const float* x0,
                        int n_images, int height, int width, int f0, int f1, const double* kernel, double lambda, double ratio,
                        double alpha, int n_iter, double* workspace, int64_t workspace_doubles, void* stream) {
    return tgv_solve("inr_tgv_solve2d_f32", out, v_out, energy, change, y, weight, x0, n_images, height, width, f0, f1, kernel, lambda,
                     ratio, alpha, n_iter, workspace, workspace_doubles, (hipStream_t)stream);
}

}  // extern "C"
