// Model-based S0 / ADC super-resolution: the reconstruction of tvj.hip with the mono-exponential signal model INSIDE the
// solver.  The unknowns of a group of C b-values are the two parameter maps themselves -- s [H][W], the b = 0 signal, and d [H][W], the
// ADC --, not C images:
//   E(s, d) = 1/2 sum_c sum_i w_ci ((A (s .* exp(-b_c d)))_i - y_ci)^2 + lambda R(s, d),     0 <= s <= s_max,  0 <= d <= adc_max
//   R = sum_j H_alpha( sqrt( mu_s^2 |(grad s)_j|^2 + mu_u^2 |(grad u)_j|^2 ) )               (coupling 1, joint)
//   R = sum_j H_alpha( mu_s |(grad s)_j| ) + sum_j H_alpha( mu_u |(grad u)_j| )             (coupling 0, none)
// A, grad, div, H_alpha: tvsr.hip's (tv_block.h).  The host normalises: beta_c = b_c / b_max, u = d b_max, u_max = adc_max b_max,
// u0 = adc0 b_max, so that beta_c u is O(1) and mu_u weighs a dimensionless map; the kernel works in (s, u), the ADC is stored as
// u / b_max.
//
// THE ITERATION is the exact nonlinear primal-dual method of Valkonen (Inverse Problems 30, 2014): Chambolle-Pock on
// min_x G(x) + F*(K(x)) with K(s, u) = ( (A (s .* exp(-beta_c u)))_c , mu_s grad s , mu_u grad u ) nonlinear, the adjoint taken of the
// Jacobian at the CURRENT iterate.  The data term is dual as well (z [C][h][w]): A composed with the per-pixel Jacobian has no
// diagonal K K^T, so the closed-form proximal step of tv_primal_block is gone.  From s = sbar, u = ubar, p = 0, z = 0:
//   q_m  <- (p_m + sigma (mu_m grad(mbar))) / (1 + sigma alpha / lambda),  m in {s, u}
//   n    <- sqrt(|q_s|^2 + |q_u|^2) / lambda, both divided by n where n > 1  (none: per map)   (lambda = 0: skipped, p stays 0)
//   r    <- sum_ab k_ab sbar_e exp(-beta_c ubar_e) - y_ci   (ascending (a, b));   z_ci <- (z_ci + sigma r) / (1 + sigma / w_ci)
//           (w_ci = 0: z_ci = 0 and y_ci is never read)
//   E_c  <- exp(-beta_c u_e);  g_s = sum_c E_c k_e z_c,i(e) - mu_s div(p_s)_e;  g_u = sum_c (-beta_c s_e E_c) k_e z_c,i(e) - mu_u div(p_u)_e
//   s'   <- fmin(fmax(s - tau g_s, 0), s_max);  u' <- fmin(fmax(u - tau g_u, 0), u_max)
//   sbar <- 2 s' - s;  ubar <- 2 u' - u;  s <- s';  u <- u'
// fp64 exp, 2 C calls per pixel and iteration, not approximated.
//
// THE STEPS.  tau = sigma = 1 / sqrt(8 + c_A L2), formed on the host.  The Jacobian of K at (s, u) is the prior part P = (mu_s grad,
// mu_u grad), |P|^2 <= 8 for mu <= 1 (tvj.hip), stacked on A J, where J acts per pixel e as the C x 2 matrix with rows
// (exp(-beta_c u_e), -beta_c s_e exp(-beta_c u_e)).  |J|_2^2 <= max_e |J_e|_F^2 = max_e sum_c exp(-2 beta_c u_e) (1 + beta_c^2 s_e^2)
// <= sum_c (1 + beta_c^2 s_max^2) = L2 on the box (u >= 0, 0 <= s <= s_max), and A, applied per channel, has |A|^2 <= |A|_1 |A|_inf
// = TvBlock::c = c_A, tvmf.hip's bound.  So |grad K|^2 <= 8 + c_A L2 everywhere on the box, and tau sigma |grad K|^2 <= 1.  The
// method's convergence is LOCAL (Valkonen, Theorem 4.1: near a solution, under a second-order condition): E is not convex in (s, u).
//
// ONE launch solves a batch of groups, as tvj.hip does: one workgroup of 1,024 threads owns one group and runs every iteration itself;
// workgroups share nothing: no cooperative launch, no grid barrier, no spin, no atomics; the grid is the groups, capped, with a stride
// loop.  The state of a group is s | u | sbar | ubar | p_s0 | p_s1 | p_u0 | p_u1, each [H][W], and z [C][h][w]: 8 H W + C h w doubles
// of the caller's workspace.  beta, mu and the block kernel come by value and are staged in LDS.  fp64 throughout, compiled with
// -ffp-contract=off (_build.py); the fp32 entry converts at load and rounds once at the store.  Offsets between groups are size_t.
// Nothing indexes by a data value: no y, x0 or b can produce an address outside a buffer.
//
// WHERE THE BARRIERS SIT, AND WHY.  An iteration has two phases and a __syncthreads() after each:
//   dual, prior (thread per HR pixel e):  reads sbar / ubar at e, e + W, e + 1 -- neighbours' --; reads and writes p_s0, p_s1, p_u0,
//                                    p_u1 at e: ITS OWN pixel's, in both maps (the joint norm is summed inside that thread);
//   dual, data  (work item per (channel, LR block)):  reads sbar / ubar at the pixels of its block, reads y and w of ITS datum, reads
//                                    and writes z of ITS datum only.  Both dual parts only read sbar / ubar and each writes only its
//                                    own p or z: they share one phase with no barrier between them;
//   ---- barrier 1: every p and z of this iteration is written before any thread differences p or gathers z
//   primal (thread per HR pixel e, its block i(e), its tap k_e):  reads p at e and its upper / left neighbours -- other threads' --,
//                                    reads z of its block in every channel -- other items' --, reads and writes s, u, sbar, ubar at e:
//                                    ITS OWN four values;
//   ---- barrier 2: every sbar / ubar of this iteration is written before the next dual phase differences or sums it
// In each phase a field is either read (possibly across threads) or written by its owner alone.  The start and the last iteration
// end with the same barrier.
//
// energy: E at the returned fp64 maps; every thread adds its data terms in ascending (channel, block), then its pixels in ascending
// order, wave_sum, thread 0 over the 16 waves (tv_store_energy_change).  change: max(|s' - s|, |u' - u|) of the last iteration, u
// normalised.
//
// adc_signal_kernel, in this unit: the model's images s0 exp(-b_c adc) of two given maps, one thread per pixel.
#include "tv_block.h"

namespace inr {
namespace {

constexpr int TVADC_MAX_CHANNELS = INR_TVJ_MAX_CHANNELS;

// the model of a call, by value in the kernel arguments: the host's normalisation and the steps
struct TvadcModel {
    double beta[TVADC_MAX_CHANNELS];   // b_c / b_max
    double mu[2];                      // the map weights (mu_s, mu_u)
    double tau;                        // = sigma = 1 / sqrt(8 + c_A L2)
    double s_max, u_max, u0, b_max;
    int c0;                            // the first channel of smallest b: the default start replicates it
};

// the b-values of inr_adc_signal, by value
struct AdcBvalues {
    double b[TVADC_MAX_CHANNELS];
};

template <typename T>
__global__ void __launch_bounds__(TV_THREADS) tvadc_solve_kernel(T* out, double* energy, double* change, const T* y, const T* weight,
                                                                 const T* x0, double* state, int n_groups, int C, TvShape sh, TvBlock kb,
                                                                 TvadcModel md, double lam, double alpha, int joint, int n_iter) {
    __shared__ double ks[TV_MAX_FACTOR * TV_MAX_FACTOR];
    __shared__ double beta[TVADC_MAX_CHANNELS];
    __shared__ double red[TV_WAVES];
    const int tid = threadIdx.x;
    const size_t HW = (size_t)sh.H * sh.W, hw = (size_t)sh.h * sh.w, W = (size_t)sh.W;
    const size_t Chw = (size_t)C * hw, per_group = 8 * HW + Chw;
    const double tau = md.tau, sigma = md.tau, mu_s = md.mu[0], mu_u = md.mu[1];
    if (tid < sh.f0 * sh.f1) ks[tid] = kb.k[tid];
    if (tid < C) beta[tid] = md.beta[tid];
    for (size_t g = blockIdx.x; g < (size_t)n_groups; g += gridDim.x) {
        double* sm = state + g * per_group;   // [H][W] each
        double* um = sm + HW;
        double* sbar = um + HW;
        double* ubar = sbar + HW;
        double* ps0 = ubar + HW;
        double* ps1 = ps0 + HW;
        double* pu0 = ps1 + HW;
        double* pu1 = pu0 + HW;
        double* z = pu1 + HW;                 // [C][h][w]
        const T* yg = y + g * Chw;
        const T* wg = weight ? weight + g * Chw : nullptr;
        const T* x0g = x0 ? x0 + g * 2 * HW : nullptr;
        for (size_t e = tid; e < HW; e += TV_THREADS) {
            const size_t i = e / W, j = e - i * W;
            double sv, uv;
            if (x0g) {
                sv = (double)x0g[e];
                uv = (double)x0g[HW + e] * md.b_max;
            } else {
                sv = (double)yg[(size_t)md.c0 * hw + (i / sh.f0) * sh.w + j / sh.f1];
                uv = md.u0;
            }
            sv = fmin(fmax(sv, 0.0), md.s_max);
            uv = fmin(fmax(uv, 0.0), md.u_max);
            sm[e] = sv;
            sbar[e] = sv;
            um[e] = uv;
            ubar[e] = uv;
            ps0[e] = 0.0;
            ps1[e] = 0.0;
            pu0[e] = 0.0;
            pu1[e] = 0.0;
        }
        for (size_t t = tid; t < Chw; t += TV_THREADS) z[t] = 0.0;
        __syncthreads();   // the start is written (and ks, beta, for the first group)
        double ch = 0.0;
        for (int it = 0; it < n_iter; ++it) {
            if (lam > 0.0) {
                const double den = 1.0 + sigma * alpha / lam;
                for (size_t e = tid; e < HW; e += TV_THREADS) {
                    const size_t i = e / W, j = e - i * W;
                    const bool down = i + 1 < (size_t)sh.H, right = j + 1 < W;
                    const double sb = sbar[e], ub = ubar[e];
                    double qs0 = (ps0[e] + sigma * (mu_s * (down ? sbar[e + W] - sb : 0.0))) / den;
                    double qs1 = (ps1[e] + sigma * (mu_s * (right ? sbar[e + 1] - sb : 0.0))) / den;
                    double qu0 = (pu0[e] + sigma * (mu_u * (down ? ubar[e + W] - ub : 0.0))) / den;
                    double qu1 = (pu1[e] + sigma * (mu_u * (right ? ubar[e + 1] - ub : 0.0))) / den;
                    const double sq_s = qs0 * qs0 + qs1 * qs1, sq_u = qu0 * qu0 + qu1 * qu1;
                    const double n_s = sqrt(joint ? sq_s + sq_u : sq_s) / lam;
                    const double n_u = joint ? n_s : sqrt(sq_u) / lam;
                    if (n_s > 1.0) {
                        qs0 /= n_s;
                        qs1 /= n_s;
                    }
                    if (n_u > 1.0) {
                        qu0 /= n_u;
                        qu1 /= n_u;
                    }
                    ps0[e] = qs0;
                    ps1[e] = qs1;
                    pu0[e] = qu0;
                    pu1[e] = qu1;
                }
            }
            for (size_t item = tid; item < Chw; item += TV_THREADS) {
                const size_t c = item / hw, blk = item - c * hw;
                const double wv = wg ? (double)wg[item] : 1.0;
                if (wv == 0.0) {   // a missing datum takes no part, whatever y holds there
                    z[item] = 0.0;
                    continue;
                }
                const size_t bi = blk / sh.w, bj = blk - bi * sh.w;
                const double bc = beta[c];
                double acc = 0.0;
                for (int a = 0; a < sh.f0; ++a) {
                    const size_t row = (bi * sh.f0 + a) * W + bj * sh.f1;
                    for (int b = 0; b < sh.f1; ++b) acc += ks[a * sh.f1 + b] * (sbar[row + b] * exp(-(bc * ubar[row + b])));
                }
                const double r = acc - (double)yg[item];
                z[item] = (z[item] + sigma * r) / (1.0 + sigma / wv);
            }
            __syncthreads();   // barrier 1: p and z are complete
            const bool last = it + 1 == n_iter;
            for (size_t e = tid; e < HW; e += TV_THREADS) {
                const size_t i = e / W, j = e - i * W;
                const size_t bi = i / sh.f0, bj = j / sh.f1, blk = bi * sh.w + bj;
                const double ke = ks[(i - bi * sh.f0) * sh.f1 + (j - bj * sh.f1)];
                const double se = sm[e], ue = um[e];
                double gs = 0.0, gu = 0.0;
                for (int c = 0; c < C; ++c) {
                    const double ec = exp(-(beta[c] * ue));
                    const double kz = ke * z[c * hw + blk];
                    gs += ec * kz;
                    gu += (-(beta[c] * se) * ec) * kz;
                }
                double ds = 0.0, du = 0.0;
                if (i + 1 < (size_t)sh.H) {
                    ds += ps0[e];
                    du += pu0[e];
                }
                if (i > 0) {
                    ds -= ps0[e - W];
                    du -= pu0[e - W];
                }
                if (j + 1 < W) {
                    ds += ps1[e];
                    du += pu1[e];
                }
                if (j > 0) {
                    ds -= ps1[e - 1];
                    du -= pu1[e - 1];
                }
                gs = gs - mu_s * ds;
                gu = gu - mu_u * du;
                const double sn = fmin(fmax(se - tau * gs, 0.0), md.s_max);
                const double un = fmin(fmax(ue - tau * gu, 0.0), md.u_max);
                sbar[e] = 2.0 * sn - se;
                ubar[e] = 2.0 * un - ue;
                sm[e] = sn;
                um[e] = un;
                if (last) ch = fmax(ch, fmax(fabs(sn - se), fabs(un - ue)));
            }
            __syncthreads();   // barrier 2: s, u, sbar and ubar are complete
        }
        // the objective at (s, u), and the maps
        double en = 0.0;
        for (size_t item = tid; item < Chw; item += TV_THREADS) {
            const size_t c = item / hw, blk = item - c * hw;
            const double wv = wg ? (double)wg[item] : 1.0;
            if (wv == 0.0) continue;
            const size_t bi = blk / sh.w, bj = blk - bi * sh.w;
            const double bc = beta[c];
            double acc = 0.0;
            for (int a = 0; a < sh.f0; ++a) {
                const size_t row = (bi * sh.f0 + a) * W + bj * sh.f1;
                for (int b = 0; b < sh.f1; ++b) acc += ks[a * sh.f1 + b] * (sm[row + b] * exp(-(bc * um[row + b])));
            }
            const double r = acc - (double)yg[item];
            en += 0.5 * wv * r * r;
        }
        double reg = 0.0;
        for (size_t e = tid; e < HW; e += TV_THREADS) {
            const size_t i = e / W, j = e - i * W;
            const bool down = i + 1 < (size_t)sh.H, right = j + 1 < W;
            const double se = sm[e], ue = um[e];
            out[g * 2 * HW + e] = (T)se;
            out[g * 2 * HW + HW + e] = (T)(ue / md.b_max);
            if (lam > 0.0) {
                const double gs0 = mu_s * (down ? sm[e + W] - se : 0.0), gs1 = mu_s * (right ? sm[e + 1] - se : 0.0);
                const double gu0 = mu_u * (down ? um[e + W] - ue : 0.0), gu1 = mu_u * (right ? um[e + 1] - ue : 0.0);
                const double sq_s = gs0 * gs0 + gs1 * gs1, sq_u = gu0 * gu0 + gu1 * gu1;
                if (joint)
                    reg += tv_huber(sqrt(sq_s + sq_u), alpha);
                else
                    reg += tv_huber(sqrt(sq_s), alpha) + tv_huber(sqrt(sq_u), alpha);
            }
        }
        if (lam > 0.0) en += lam * reg;
        tv_store_energy_change(en, ch, red, energy, change, g);   // ends with a barrier: red is free for the next group
    }
}

// out [n][C][P] = s0 [n][P] exp(-(b_c adc [n][P])): fp64 inside, rounded once
template <typename T>
__global__ void __launch_bounds__(256) adc_signal_kernel(T* out, const T* s0, const T* adc, AdcBvalues bv, long long n, int C, long long P) {
    const long long total = n * P;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long g = t / P, e = t - g * P;
        const double s = (double)s0[t], d = (double)adc[t];
        for (int c = 0; c < C; ++c) out[((size_t)g * C + c) * (size_t)P + e] = (T)(s * exp(-(bv.b[c] * d)));
    }
}

int tvadc_group_check(const char* who, int n_groups, int channels) {
    INR_REQUIRE(n_groups >= 0, INR_E_INVALID, "%s: bad sizes (n_groups = %d)", who, n_groups);
    INR_REQUIRE(channels >= 2 && channels <= TVADC_MAX_CHANNELS, INR_E_INVALID, "%s: b-values are 2 .. %d per group (got %d)", who,
                TVADC_MAX_CHANNELS, channels);
    return 0;
}

// the workspace: s | u | sbar | ubar | p_s0 | p_s1 | p_u0 | p_u1 [H][W] and z [C][h][w] of every group.  base == null: `total` only
TvStateView tvadc_view(int n_groups, int C, const TvShape& sh, void* base) {
    TvStateView v;
    WsCarver c(base, 16);
    v.state = c.take<double>((size_t)(n_groups > 0 ? n_groups : 1) * (8 * (size_t)sh.H * sh.W + (size_t)C * sh.h * sh.w));
    v.total = c.bytes();
    return v;
}

// the HOST b-values [C]: finite, >= 0, not all equal
int tvadc_b_check(const char* who, const double* b, int C, double* b_max, int* c0) {
    double lo = b[0], hi = b[0];
    *c0 = 0;
    for (int c = 0; c < C; ++c) {
        INR_REQUIRE(std::isfinite(b[c]) && b[c] >= 0.0, INR_E_INVALID, "%s: b-values must be finite and >= 0 (entry %d is %g)", who, c, b[c]);
        if (b[c] < lo) {
            lo = b[c];
            *c0 = c;
        }
        hi = std::fmax(hi, b[c]);
    }
    INR_REQUIRE(hi > lo, INR_E_INVALID, "%s: the b-values are all equal (%g): they determine no ADC", who, hi);
    *b_max = hi;
    return 0;
}

template <typename T>
int tvadc_solve(const char* who, T* out, double* energy, double* change, const T* y, const T* weight, const T* x0, int n_groups, int C,
                int H, int W, int f0, int f1, const double* kernel, const double* b, const double* map_weights, double lam, double alpha,
                int coupling, int n_iter, double s_max, double adc_max, double adc0, double* workspace, int64_t workspace_doubles,
                hipStream_t st) {
    INR_REQUIRE(out && y && b, INR_E_INVALID, "%s: null pointer (out, y or b)", who);
    TvShape sh;
    TvBlock kb;
    TvadcModel md;
    if (int rc = tvadc_group_check(who, n_groups, C)) return rc;
    if (int rc = tv_shape_check(who, n_groups, H, W, f0, f1, &sh)) return rc;
    if (int rc = tv_params_check(who, lam, alpha, n_iter, -1)) return rc;
    INR_REQUIRE(coupling == 0 || coupling == 1, INR_E_INVALID, "%s: coupling is 0 (none) or 1 (joint) (got %d)", who, coupling);
    if (int rc = tv_block_check(who, kernel, f0, f1, &kb)) return rc;
    if (int rc = tvadc_b_check(who, b, C, &md.b_max, &md.c0)) return rc;
    INR_REQUIRE(std::isfinite(s_max) && s_max > 0.0, INR_E_INVALID, "%s: s_max must be finite and > 0 (got %g)", who, s_max);
    INR_REQUIRE(std::isfinite(adc_max) && adc_max > 0.0 && std::isfinite(adc_max * md.b_max), INR_E_INVALID,
                "%s: adc_max must be finite and > 0 (got %g)", who, adc_max);
    INR_REQUIRE(adc0 >= 0.0 && adc0 <= adc_max, INR_E_INVALID, "%s: adc0 must be within [0, adc_max] (got %g, adc_max %g)", who, adc0,
                adc_max);
    for (int m = 0; m < 2; ++m) {
        const double v = map_weights ? map_weights[m] : 1.0;
        // larger weights would break |P|^2 <= 8, the step bound: the caller rescales lambda and alpha instead
        INR_REQUIRE(std::isfinite(v) && v >= 0.0 && v <= 1.0, INR_E_INVALID,
                    "%s: map_weights must be finite and within [0, 1] (entry %d is %g)", who, m, v);
        md.mu[m] = v;
    }
    if (int rc = check_ws_doubles(who, workspace, workspace_doubles, tvadc_view(n_groups, C, sh, nullptr).total)) return rc;
    if (n_groups == 0) return 0;
    double l2 = 0.0;
    for (int c = 0; c < TVADC_MAX_CHANNELS; ++c) {
        md.beta[c] = c < C ? b[c] / md.b_max : 0.0;
        if (c < C) l2 += 1.0 + md.beta[c] * md.beta[c] * (s_max * s_max);
    }
    md.tau = 1.0 / std::sqrt(8.0 + kb.c * l2);
    md.s_max = s_max;
    md.u_max = adc_max * md.b_max;
    md.u0 = adc0 * md.b_max;
    const TvStateView v = tvadc_view(n_groups, C, sh, workspace);
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL((tvadc_solve_kernel<T>), dim3((unsigned)(n_groups < TV_MAX_GRID ? n_groups : TV_MAX_GRID)), dim3(TV_THREADS), 0,
                       st, out, energy, change, y, weight, x0, v.state, n_groups, C, sh, kb, md, lam, alpha, coupling, n_iter);
    INR_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int adc_signal(const char* who, T* out, const T* s0, const T* adc, const double* b, int64_t n, int C, int64_t pixels, hipStream_t st) {
    INR_REQUIRE(out && s0 && adc && b, INR_E_INVALID, "%s: null pointer", who);
    INR_REQUIRE(n >= 0 && pixels >= 1 && pixels <= ((int64_t)1 << 40) && n <= ((int64_t)1 << 40) / pixels, INR_E_INVALID,
                "%s: bad sizes (n = %lld, pixels = %lld)", who, (long long)n, (long long)pixels);
    INR_REQUIRE(C >= 1 && C <= TVADC_MAX_CHANNELS, INR_E_INVALID, "%s: b-values are 1 .. %d (got %d)", who, TVADC_MAX_CHANNELS, C);
    AdcBvalues bv;
    for (int c = 0; c < TVADC_MAX_CHANNELS; ++c) {
        bv.b[c] = c < C ? b[c] : 0.0;
        INR_REQUIRE(std::isfinite(bv.b[c]), INR_E_INVALID, "%s: b-values must be finite (entry %d is %g)", who, c, bv.b[c]);
    }
    if (n == 0) return 0;
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL((adc_signal_kernel<T>), dim3(tv_pixel_grid((long long)(n * pixels))), dim3(256), 0, st, out, s0, adc, bv,
                       (long long)n, C, (long long)pixels);
    INR_LAUNCH_CHECK();
    return 0;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_tvadc_workspace_doubles(int n_groups, int channels, int height, int width, int f0, int f1) {
    TvShape sh;
    if (tvadc_group_check("inr_tvadc_workspace_doubles", n_groups, channels)) return 0;
    if (tv_shape_check("inr_tvadc_workspace_doubles", n_groups, height, width, f0, f1, &sh)) return 0;
    return (int64_t)(tvadc_view(n_groups, channels, sh, nullptr).total / sizeof(double));
}

int inr_tvadc_solve2d(double* out, double* energy, double* change, const double* y, const double* weight, const double* x0, int n_groups,
                      int channels, int height, int width, int f0, int f1, const double* kernel, const double* b,
                      const double* map_weights, double lambda, double alpha, int coupling, int n_iter, double s_max, double adc_max,
                      double adc0, double* workspace, int64_t workspace_doubles, void* stream) {
    return tvadc_solve("inr_tvadc_solve2d", out, energy, change, y, weight, x0, n_groups, channels, height, width, f0, f1, kernel, b,
                       map_weights, lambda, alpha, coupling, n_iter, s_max, adc_max, adc0, workspace, workspace_doubles,
                       (hipStream_t)stream);
}

int inr_tvadc_solve2d_f32(float* out, double* energy, double* change, const float* y, const float* weight, const float* x0, int n_groups,
                          int channels, int height, int width, int f0, int f1, const double* kernel, const double* b,
                          const double* map_weights, double lambda, double alpha, int coupling, int n_iter, double s_max,
                          double adc_max, double adc0, double* workspace, int64_t workspace_doubles, void* stream) {
    return tvadc_solve("inr_tvadc_solve2d_f32", out, energy, change, y, weight, x0, n_groups, channels, height, width, f0, f1, kernel, b,
                       map_weights, lambda, alpha, coupling, n_iter, s_max, adc_max, adc0, workspace, workspace_doubles,
                       (hipStream_t)stream);
}

int inr_adc_signal(double* out, const double* s0, const double* adc, const double* b, int64_t n_maps, int channels, int64_t pixels,
                   void* stream) {
    return adc_signal("inr_adc_signal", out, s0, adc, b, n_maps, channels, pixels, (hipStream_t)stream);
}

int inr_adc_signal_f32(float* out, const float* s0, const float* adc, const double* b, int64_t n_maps, int channels, int64_t pixels,
                       void* stream) {
    return adc_signal("inr_adc_signal_f32", out, s0, adc, b, n_maps, channels, pixels, (hipStream_t)stream);
}

}  // extern "C"
