// The fp64 tile loop shared by fourier.hip and tvop.hip: one 64 x 64 tile of C = A B on v_mfma_f64_16x16x4_f64, by a block of 256
// threads (4 waves, 32 x 32 each: 2 x 2 MFMA tiles).  K is walked in stages of GF_KS = 16 through LDS, four MFMA steps per stage, in
// ascending k: the K order is fixed, there are no atomics, and the bits of a result depend on the operands and on K alone -- not on
// the grid, the tile's place in it or the operand's element type beyond its conversion to double.  A kernel declares the two LDS
// planes, walks its own tiles and hands every finished element to an epilogue functor; the loop ends on a barrier, so the planes are
// free for the next tile as soon as it returns.  The next stage's operands travel from memory while a stage is multiplied.  gf_tile_fn is the loop, gf_tile the same loop over two operands in memory.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace inr {

typedef double gf_f64x4 __attribute__((ext_vector_type(4)));

constexpr int GF_TILE = 64;    // the block's output tile
constexpr int GF_KS = 16;      // K per LDS stage: 4 MFMA steps
constexpr int GF_PITCH = 81;   // doubles per staged k: the 16 k of a k-fastest store fall on 16 bank pairs, the two k of a read's lane
                               // group on disjoint halves of the 64 banks (but for one pair)

// the transform of an operand at its load
struct GfIdentity {
    __device__ __forceinline__ double operator()(double v) const { return v; }
};
struct GfAbs {
    __device__ __forceinline__ double operator()(double v) const { return fabs(v); }
};

// The loop itself, over operands that two functors supply: la(row, k) for row < M and lb(k, col) for col < N, both for k < K, each a
// double; everything beyond is staged as 0 and never asked for.  a_kfast / b_kfast: the operand's contiguous direction is k (neighbouring
// threads then take neighbouring k), else its rows (columns).  epi(row, col, batch, value) is called once for every element of the tile
// inside M x N, by the thread that holds it: in the f64 result layout that is column lane & 15, row (lane >> 4) + 4 reg -- not the
// f32 one.  A functor that generates its operand (degibbs.hip: a circulant from a table, the DFT blocks) pays no dense matrix for it.
template <class LA, class LB, class Epi>
__device__ __forceinline__ void gf_tile_fn(double (&As)[GF_KS][GF_PITCH], double (&Bs)[GF_KS][GF_PITCH], const LA& la, bool a_kfast,
                                           const LB& lb, bool b_kfast, long long row0, int col0, long long M, int N, int K, int batch,
                                           Epi& epi) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const int l15 = lane & 15, l4 = lane >> 4;
    gf_f64x4 acc[2][2] = {};
    // a stage's operands are fetched into registers while the stage before it is multiplied: GF_TILE * GF_KS / 256 = 4 values of each
    // operand per thread, the contiguous direction of an operand over neighbouring threads
    constexpr int GF_PER = GF_TILE * GF_KS / 256;
    double ra[GF_PER], rb[GF_PER];
    const auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < GF_PER; ++i) {
            const int e = t + 256 * i;
            const int kk = a_kfast ? e & (GF_KS - 1) : e / GF_TILE, r = a_kfast ? e / GF_KS : e & (GF_TILE - 1);
            const long long row = row0 + r;
            const int k = k0 + kk;
            ra[i] = row < M && k < K ? la(row, k) : 0.0;
        }
#pragma unroll
        for (int i = 0; i < GF_PER; ++i) {
            const int e = t + 256 * i;
            const int kk = b_kfast ? e & (GF_KS - 1) : e / GF_TILE, c = b_kfast ? e / GF_KS : e & (GF_TILE - 1);
            const int col = col0 + c, k = k0 + kk;
            rb[i] = col < N && k < K ? lb(k, col) : 0.0;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += GF_KS) {
#pragma unroll
        for (int i = 0; i < GF_PER; ++i) {
            const int e = t + 256 * i;
            As[a_kfast ? e & (GF_KS - 1) : e / GF_TILE][a_kfast ? e / GF_KS : e & (GF_TILE - 1)] = ra[i];
            Bs[b_kfast ? e & (GF_KS - 1) : e / GF_TILE][b_kfast ? e / GF_KS : e & (GF_TILE - 1)] = rb[i];
        }
        __syncthreads();
        if (k0 + GF_KS < K) fetch(k0 + GF_KS);
#pragma unroll
        for (int ks = 0; ks < GF_KS; ks += 4) {
            // A: lane holds A[row lane & 15][k lane >> 4]; B: B[k lane >> 4][column lane & 15]
            const double a0 = As[ks + l4][wr + l15], a1 = As[ks + l4][wr + 16 + l15];
            const double b0 = Bs[ks + l4][wc + l15], b1 = Bs[ks + l4][wc + 16 + l15];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const long long row = row0 + wr + 16 * mi + l4 + 4 * reg;
                const int col = col0 + wc + 16 * ni + l15;
                if (row < M && col < N) epi(row, col, batch, acc[mi][ni][reg]);
            }
}

// an operand in memory behind a transform of every loaded value: element (i, k) at P[i * s_i + k * s_k]
template <class X, typename T>
struct GfStrided {
    const T* __restrict__ P;
    long long s_i, s_k;
    __device__ __forceinline__ double operator()(long long i, int k) const { return X{}((double)P[i * s_i + k * s_k]); }
};
template <class X, typename T>
struct GfStridedB {
    const T* __restrict__ P;
    long long s_k, s_col;
    __device__ __forceinline__ double operator()(int k, int col) const { return X{}((double)P[k * s_k + col * s_col]); }
};

// A(row, k) = A[row * a_row + k * a_k] for row < M, B(k, col) = B[k * b_k + col * b_col] for col < N, both for k < K; XA / XB transform
// a loaded value.  The tile loop over two operands in memory
template <class XA, class XB, typename TA, typename TB, class Epi>
__device__ __forceinline__ void gf_tile(double (&As)[GF_KS][GF_PITCH], double (&Bs)[GF_KS][GF_PITCH], const TA* __restrict__ A,
                                        long long a_row, long long a_k, const TB* __restrict__ B, long long b_k, long long b_col,
                                        long long row0, int col0, long long M, int N, int K, int batch, Epi& epi) {
    const GfStrided<XA, TA> la{A, a_row, a_k};
    const GfStridedB<XB, TB> lb{B, b_k, b_col};
    gf_tile_fn(As, Bs, la, a_k == 1, lb, b_k == 1, row0, col0, M, N, K, batch, epi);
}

}  // namespace inr
