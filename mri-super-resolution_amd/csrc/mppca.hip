// Marchenko-Pastur PCA denoising of a multi-measurement stack, with a noise map (include/inrhip.h: inr_mppca_denoise).
// x [M][D][H][W]; for every voxel inside the mask the M x N matrix X of its window (N = w0 w1 w2 voxels, the window shifted inward at
// the volume's edges, never mirrored) gives the r x r Gram matrix G = X X^T (M <= N) or X^T X (N < M), r = min(M, N); the spectrum of
// G alone decides the noise level and how many of its components are noise, and the voxel's own column is projected onto the rest.
//
// One workgroup of 256 threads per voxel, a capped grid with a stride loop (tv_grid, so inr_debug_set(32, .) walks the stride on a
// small volume), fp64 throughout, four steps:
//   1. G in LDS: X is staged in chunks of MP_CHUNK entries of the long index, never whole; each thread owns fixed (i, j) entries and adds
//      the long index in ascending order.
//   2. cyclic two-sided Jacobi in round-robin ordering: r padded to even (n), each of the n - 1 steps of a sweep rotates n / 2 disjoint
//      index pairs in two phases with a barrier after each: (c, s) of every pair | the rotation.  A thread takes the 2 x 2 block
//      (pair k) x (pair l) of G through the rows' rotation of pair k and then the columns' of pair l -- the blocks are disjoint, so rows
//      and columns need no barrier between them -- and the columns of V.  A pair's own 2 x 2 block is set to its exact values (G_pq =
//      G_qp = 0, G_pp -= t G_pq, G_qq += t G_pq), so off-diagonal entries only ever mix with off-diagonal entries and shrink far below
//      eps ||G||.  A sweep starts only while the off-diagonal sum of squares exceeds (r eps)^2 ||G||_F^2 (a block sum every thread
//      receives: a workgroup-uniform test); after MP_MAX_SWEEPS the voxel is given up (rank -2, sigma 0, out = x).
//   3. the eigenvalues are ranked (ties by index; the permutation is carried, not the vectors) and one thread runs the cutoff loop;
//      eigenvalues at or below q eps s_max are numerically zero and always cut.
//   4. the projection; the N < M branch reads X from global memory a second time.
// LDS: G and V are [R][R] doubles of the rank class R in {16, 32, 64} (unpadded: consecutive lanes take the different pairs of ONE row,
// or the blocks of one pair of rows, so no read meets a bank twice at R = 64), the staging chunk [R][MP_CHUNK + 1] and 7 R doubles of
// small arrays: 7.1 KB / 22.1 KB / 76.1 KB, dynamic, opted in above 64 KB -- 2 workgroups per CU at R = 64 (by LDS, and by its 210
// VGPRs), 4 at R = 32 and 5 at R = 16 (by their 90 - 100 VGPRs; LDS would allow 7 and 22).  No workspace, no atomics; a voxel's bits
// depend on its window alone.
#include "tv_shared.h"

namespace inr {
namespace {

constexpr int MP_THREADS = 256;
constexpr int MP_CHUNK = 16;        // entries of the long index staged at a time
constexpr int MP_MAX_SWEEPS = 30;
constexpr double MP_EPS = 2.220446049250313e-16;

struct MpShape {
    int M, D, H, W, w0, w1, w2, N, r, q, estimator;
    long long vol;
};

template <int R>
constexpr size_t mp_lds_bytes() {
    // G | V | staging | cs, sn, npp, nqq [R / 2 each] | ev, lam, xc, coef [R each] | red [4] | scalars [4] || ip, iq [R / 2] | perm [R]
    return sizeof(double) * (2 * R * R + R * (MP_CHUNK + 1) + 4 * (R / 2) + 4 * R + 8) + sizeof(int) * (2 * (R / 2) + R);
}

// the offset of window column `col` from the window's first voxel
__device__ __forceinline__ long long mp_col_offset(int col, const MpShape& s) {
    const int plane = s.w1 * s.w2;
    const int dz = col / plane, rem = col - dz * plane;
    const int dy = rem / s.w2, dx = rem - dy * s.w2;
    return ((long long)dz * s.H + dy) * s.W + dx;
}
__device__ __forceinline__ int mp_start(int i, int w, int n) {
    const int a = i - w / 2;
    return a < 0 ? 0 : (a > n - w ? n - w : a);
}

template <typename T, int R>
__global__ void __launch_bounds__(MP_THREADS) mppca_kernel(T* __restrict__ out, T* __restrict__ sigma, int32_t* __restrict__ rank,
                                                          const T* __restrict__ x, const uint8_t* __restrict__ mask, MpShape s) {
    extern __shared__ double mp_lds[];
    double* G = mp_lds;
    double* V = G + R * R;
    double* S = V + R * R;                        // [R][MP_CHUNK + 1]
    double* cs = S + R * (MP_CHUNK + 1);
    double* sn = cs + R / 2;
    double* npp = sn + R / 2;
    double* nqq = npp + R / 2;
    double* ev = nqq + R / 2;
    double* lam = ev + R;
    double* xc = lam + R;
    double* coef = xc + R;
    double* red = coef + R;                       // [4]
    double* scal = red + 4;                       // [4]: sigma2, cut
    int* ip = reinterpret_cast<int*>(scal + 4);
    int* iq = ip + R / 2;
    int* perm = iq + R / 2;
    constexpr int SP = MP_CHUNK + 1;
    constexpr int ENTRIES = R * R / MP_THREADS;   // entries of G a thread owns: e = tid + MP_THREADS m

    const int tid = threadIdx.x;
    const int r = s.r, n = (r + 1) & ~1, half = n >> 1;
    const bool wide = s.M <= s.N;                 // G = X X^T, the long index runs over the window

    for (long long vox = blockIdx.x; vox < s.vol; vox += gridDim.x) {
        const int vx = (int)(vox % s.W), vy = (int)((vox / s.W) % s.H), vz = (int)(vox / ((long long)s.W * s.H));
        if (mask && !mask[vox]) {                 // uniform over the workgroup
            for (int m = tid; m < s.M; m += MP_THREADS) out[m * s.vol + vox] = x[m * s.vol + vox];
            if (tid == 0) {
                if (sigma) sigma[vox] = (T)0;
                if (rank) rank[vox] = -1;
            }
            continue;
        }
        const int z0 = mp_start(vz, s.w0, s.D), y0 = mp_start(vy, s.w1, s.H), x0 = mp_start(vx, s.w2, s.W);
        const long long first = ((long long)z0 * s.H + y0) * s.W + x0;
        const int c = ((vz - z0) * s.w1 + (vy - y0)) * s.w2 + (vx - x0);

        // ---- 1. the Gram matrix ---------------------------------------------------------------------------------------------------
        double acc[ENTRIES];
#pragma unroll
        for (int m = 0; m < ENTRIES; ++m) acc[m] = 0.0;
        for (int l0 = 0; l0 < s.q; l0 += MP_CHUNK) {
            __syncthreads();                      // the previous chunk (and the previous voxel's last reads) are done with
            for (int item = tid; item < R * MP_CHUNK; item += MP_THREADS) {
                int i, k;
                if (wide) {
                    i = item / MP_CHUNK;
                    k = item - i * MP_CHUNK;
                } else {
                    k = item / R;
                    i = item - k * R;
                }
                const int l = l0 + k;
                double v = 0.0;
                if (i < r && l < s.q) {
                    const int meas = wide ? i : l, col = wide ? l : i;
                    v = (double)x[meas * s.vol + first + mp_col_offset(col, s)];
                }
                S[i * SP + k] = v;
            }
            __syncthreads();
#pragma unroll 2   // 4 takes the R = 64 kernel to 256 VGPRs and one workgroup per CU
            for (int k = 0; k < MP_CHUNK; ++k) {
#pragma unroll
                for (int m = 0; m < ENTRIES; ++m) {
                    const int e = tid + MP_THREADS * m;
                    acc[m] = fma(S[(e / R) * SP + k], S[(e % R) * SP + k], acc[m]);
                }
            }
        }
        double part = 0.0;
#pragma unroll
        for (int m = 0; m < ENTRIES; ++m) {
            const int e = tid + MP_THREADS * m;
            G[e] = acc[m];
            V[e] = (e / R == e % R) ? 1.0 : 0.0;
            part += acc[m] * acc[m];
        }
        const double tol = block_sum_f64(part, red) * ((double)r * MP_EPS) * ((double)r * MP_EPS);   // (syncs: G and V are whole)

        // ---- 2. Jacobi ----------------------------------------------------------------------------------------------------------------
        bool converged = false;
        for (int sweep = 0;; ++sweep) {
            double off = 0.0;
#pragma unroll
            for (int m = 0; m < ENTRIES; ++m) {
                const int e = tid + MP_THREADS * m;
                const double g = G[e];
                if (e / R != e % R) off += g * g;
            }
            off = block_sum_f64(off, red);
            if (off <= tol) {
                converged = true;
                break;
            }
            if (sweep == MP_MAX_SWEEPS) break;
            for (int step = 0; step < n - 1; ++step) {
                if (tid < half) {
                    int p, q;
                    if (tid == 0) {
                        p = step;
                        q = n - 1;
                    } else {
                        p = (step + tid) % (n - 1);
                        q = (step - tid + (n - 1)) % (n - 1);
                        if (p > q) {
                            const int t_ = p;
                            p = q;
                            q = t_;
                        }
                    }
                    const double app = G[p * R + p], aqq = G[q * R + q], apq = G[p * R + q];
                    double t = 0.0;
                    if (apq != 0.0) {
                        const double tau = (aqq - app) / (2.0 * apq);
                        t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));   // tau^2 = inf: t = 0
                    }
                    const double cc = 1.0 / sqrt(1.0 + t * t);
                    ip[tid] = p;
                    iq[tid] = q;
                    cs[tid] = cc;
                    sn[tid] = t * cc;
                    npp[tid] = app - t * apq;
                    nqq[tid] = aqq + t * apq;
                }
                __syncthreads();
                // G: the 2 x 2 block (pair k) x (pair l) takes the rows' rotation of pair k, then the columns' of pair l -- the blocks are
                // disjoint, so rows and columns need no barrier between them; consecutive lanes take the blocks of one pair of rows
                for (int item = tid; item < half * half; item += MP_THREADS) {
                    const int k = item / half, l = item - k * half;
                    const int pk = ip[k], qk = iq[k], pl = ip[l], ql = iq[l];
                    double g00 = G[pk * R + pl], g01 = G[pk * R + ql], g10 = G[qk * R + pl], g11 = G[qk * R + ql];
                    if (k == l) {                 // the pair's own block, exactly
                        g00 = npp[k];
                        g01 = 0.0;
                        g10 = 0.0;
                        g11 = nqq[k];
                    } else {
                        const double ck = cs[k], sk = sn[k], cl = cs[l], sl = sn[l];
                        const double r00 = ck * g00 - sk * g10, r10 = sk * g00 + ck * g10;
                        const double r01 = ck * g01 - sk * g11, r11 = sk * g01 + ck * g11;
                        g00 = cl * r00 - sl * r01;
                        g01 = sl * r00 + cl * r01;
                        g10 = cl * r10 - sl * r11;
                        g11 = sl * r10 + cl * r11;
                    }
                    G[pk * R + pl] = g00;
                    G[pk * R + ql] = g01;
                    G[qk * R + pl] = g10;
                    G[qk * R + ql] = g11;
                }
                for (int item = tid; item < half * n; item += MP_THREADS) {       // V: consecutive lanes take the pairs of one row
                    const int i = item / half, k = item - i * half;
                    const int p = ip[k], q = iq[k];
                    const double cc = cs[k], ss = sn[k];
                    const double vp = V[i * R + p], vq = V[i * R + q];
                    V[i * R + p] = cc * vp - ss * vq;
                    V[i * R + q] = ss * vp + cc * vq;
                }
                __syncthreads();
            }
        }

        if (!converged) {                         // uniform
            for (int m = tid; m < s.M; m += MP_THREADS) out[m * s.vol + vox] = x[m * s.vol + vox];
            if (tid == 0) {
                if (sigma) sigma[vox] = (T)0;
                if (rank) rank[vox] = -2;
            }
            continue;
        }

        // ---- 3. sort and cut ------------------------------------------------------------------------------------------------------
        if (tid < r) ev[tid] = G[tid * R + tid];
        __syncthreads();
        if (tid < r) {
            const double mine = ev[tid];
            int pos = 0;
            for (int j = 0; j < r; ++j) {
                const double other = ev[j];
                pos += (other < mine || (other == mine && j < tid)) ? 1 : 0;
            }
            perm[pos] = tid;
            lam[pos] = mine;                      // the sorted eigenvalues s_p; scaled and floored by the thread that cuts
        }
        if (wide)
            for (int m = tid; m < s.M; m += MP_THREADS) xc[m] = (double)x[m * s.vol + vox];
        __syncthreads();
        if (tid == 0) {
            // s_p <= q eps s_{r-1} is numerically zero (what summing q products leaves of an exact zero): lam_p = 0, and such a
            // component is noise whatever the loop decides -- G of exact low-rank data has nothing else below its signal
            const double tol = (double)s.q * MP_EPS * fmax(lam[r - 1], 0.0);
            double clam = 0.0, sigma2 = 0.0;
            int cut = 0, zeros = 0;
            const double lam0 = lam[0] <= tol ? 0.0 : lam[0] / (double)s.q;
            for (int p = 0; p < r; ++p) {
                const bool zero = lam[p] <= tol;
                const double lp = zero ? 0.0 : lam[p] / (double)s.q;
                zeros += zero ? 1 : 0;
                clam += lp;
                const double gam = s.estimator == 2 ? (double)(p + 1) / (double)(s.q - (r - p - 1)) : (double)(p + 1) / (double)s.q;
                const double a = clam / (double)(p + 1);
                const double b = (lp - lam0) / (4.0 * sqrt(gam));
                if (b < a) {
                    sigma2 = a;
                    cut = p + 1;
                }
            }
            if (cut < zeros) cut = zeros;
            scal[0] = sigma2;
            scal[1] = (double)cut;
            if (sigma) sigma[vox] = (T)sqrt(sigma2);
            if (rank) rank[vox] = r - cut;
        }
        __syncthreads();
        const int cut = (int)scal[1];

        // ---- 4. the projection ----------------------------------------------------------------------------------------------------
        if (wide) {                               // xhat = V_s (V_s^T x_c)
            if (tid >= cut && tid < r) {
                const int col = perm[tid];
                double a = 0.0;
                for (int i = 0; i < r; ++i) a = fma(V[i * R + col], xc[i], a);
                coef[tid] = a;
            }
            __syncthreads();
            if (tid < r) {
                double a = 0.0;
                for (int k = cut; k < r; ++k) a = fma(V[tid * R + perm[k]], coef[k], a);
                out[tid * s.vol + vox] = (T)a;
            }
        } else {                                  // xhat = X (V_s V_s[c, :]^T)
            if (tid < r) {
                double a = 0.0;
                for (int k = cut; k < r; ++k) a = fma(V[tid * R + perm[k]], V[c * R + perm[k]], a);
                coef[tid] = a;
            }
            __syncthreads();
            for (int m = tid; m < s.M; m += MP_THREADS) {
                double a = 0.0;
                for (int j = 0; j < r; ++j) a = fma((double)x[m * s.vol + first + mp_col_offset(j, s)], coef[j], a);
                out[m * s.vol + vox] = (T)a;
            }
        }
    }
}

template <typename T, int R>
int mppca_launch(T* out, T* sigma, int32_t* rank, const T* x, const uint8_t* mask, const MpShape& s, hipStream_t st) {
    constexpr size_t lds = mp_lds_bytes<R>();
    if (lds > 64 * 1024)
        INR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&mppca_kernel<T, R>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((mppca_kernel<T, R>), dim3(tv_grid(s.vol)), dim3(MP_THREADS), lds, st, out, sigma, rank, x, mask, s);
    INR_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int mppca_denoise(const char* who, T* out, T* sigma, int32_t* rank, const T* x, const uint8_t* mask, int M, int D, int H, int W, int w0,
                  int w1, int w2, int estimator, hipStream_t st) {
    INR_REQUIRE(out && x, INR_E_INVALID, "%s: null pointer (out and x are required)", who);
    INR_REQUIRE(M >= 2, INR_E_INVALID, "%s: at least 2 measurements are needed (got M = %d)", who, M);
    INR_REQUIRE(D >= 0 && H >= 0 && W >= 0, INR_E_INVALID, "%s: negative size (%d, %d, %d)", who, D, H, W);
    const int win[3] = {w0, w1, w2}, ext[3] = {D, H, W};
    for (int a = 0; a < 3; ++a)
        INR_REQUIRE(win[a] >= 1 && (win[a] & 1), INR_E_INVALID, "%s: window sides must be odd and >= 1 (side %d is %d)", who, a, win[a]);
    const long long N = (long long)w0 * w1 * w2;
    INR_REQUIRE(N >= 2, INR_E_INVALID, "%s: the window must hold at least 2 voxels (got %d x %d x %d)", who, w0, w1, w2);
    const long long lo = M < N ? M : N, hi = M < N ? N : M;
    INR_REQUIRE(lo <= INR_MPPCA_MAX_RANK, INR_E_INVALID,
                "%s: min(M, N) = min(%d, %lld) exceeds the rank limit %d: shrink the window or split the measurements", who, M, N,
                INR_MPPCA_MAX_RANK);
    INR_REQUIRE(hi <= INR_MPPCA_MAX_LONG, INR_E_INVALID, "%s: max(M, N) = max(%d, %lld) exceeds %d", who, M, N, INR_MPPCA_MAX_LONG);
    INR_REQUIRE(estimator == 1 || estimator == 2, INR_E_INVALID, "%s: estimator must be 1 (exp1) or 2 (exp2) (got %d)", who, estimator);
    const long long vol = (long long)D * H * W;
    if (vol == 0) return 0;
    for (int a = 0; a < 3; ++a)
        INR_REQUIRE(win[a] <= ext[a], INR_E_INVALID, "%s: window side %d (%d) is larger than its axis (%d)", who, a, win[a], ext[a]);
    INR_REQUIRE(vol <= ((long long)1 << 40) / M, INR_E_INVALID, "%s: the stack is too large (%d x %lld voxels)", who, M, vol);
    MpShape s{M, D, H, W, w0, w1, w2, (int)N, (int)lo, (int)hi, estimator, vol};
    ProfScope ps(KC_OTHER, st);
    if (lo <= 16) return mppca_launch<T, 16>(out, sigma, rank, x, mask, s, st);
    if (lo <= 32) return mppca_launch<T, 32>(out, sigma, rank, x, mask, s, st);
    return mppca_launch<T, 64>(out, sigma, rank, x, mask, s, st);
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int inr_mppca_denoise(double* out, double* sigma, int32_t* rank, const double* x, const uint8_t* mask, int M, int D, int H, int W, int w0,
                      int w1, int w2, int estimator, void* stream) {
    return mppca_denoise("inr_mppca_denoise", out, sigma, rank, x, mask, M, D, H, W, w0, w1, w2, estimator, (hipStream_t)stream);
}

int inr_mppca_denoise_f32(float* out, float* sigma, int32_t* rank, const float* x, const uint8_t* mask, int M, int D, int H, int W, int w0,
                          int w1, int w2, int estimator, void* stream) {
    return mppca_denoise("inr_mppca_denoise_f32", out, sigma, rank, x, mask, M, D, H, W, w0, w1, w2, estimator, (hipStream_t)stream);
}

}  // extern "C"
