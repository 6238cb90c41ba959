// The WIRE complex-Gabor INR (INRmodel.py:66-120 `ComplexGaborLayer2D`, stacked by wiretest.ipynb cell 2) in REAL arithmetic: no
// complex type in any kernel.  Activations are planes [n][2H] = [hr | hi]; a complex layer is a real GEMM against the BLOCK IMAGE
// of its weights, four planes [H][2H] whose row j is
//     lin_r: [ Wr_j | -Wi_j ]    lin_i: [ Wi_j | Wr_j ]    orth_r, orth_i: the same of scale_orth
// so that [hr | hi] times plane q gives quantity q of unit j.  Layer 0 is real: two planes [H][K0] (lin_r, orth_r), K0 =
// in_features rounded up to the K block with zero columns.  The complex structure lives in wire_pack_* (parameters -> image, once
// per step), wire_fold_* (image gradient -> parameter gradient, the + / - pairing) and the epilogues.
//   wire_gemm_kernel<Q, GABOR> -- forward layer: a block owns 64 rows x 64 units of ALL Q quantities, a wave 32 x 32 of them, so
//       lin_r, lin_i, orth_r, orth_i of one (row, unit) sit in registers together:  A = exp(-w lin_i - s^2 (lin_r^2 + lin_i^2 +
//       orth_r^2 + orth_i^2)) as ONE exponential, out = A (cos, sin)(w lin_r).  Training also stashes the four quantities.
//   wire_gemm_kernel<1, STORE> -- input gradient [d hr | d hi] = dZ [n][4H] times the image (read through its transpose); with
//       the transposed layer-0 image (wire_pack_first_t_kernel) also dx [n][in] = dZ0 [n][2H] times it: the gradient with
//       respect to the network's real input (wiretest.ipynb cell 10's PerturbNet branch), any in_features, unpadded
//   wire_bwd_kernel            -- G, stash, out -> dZ (in place over the stash)
//   wire_pgrad_kernel          -- image gradient dZ^T [hr | hi], rows split into slabs of WIRE_SLAB_ROWS, one slab per split
//   wire_colsum_kernel         -- per-slab column sums (bias gradients; with a row weight the head's weight gradient)
//   wire_head_*                -- y = hr.w_r - hi.w_i + b_r (a wave per row) and G = gy (w_r, -w_i)
// Every reduction runs in a fixed order (slabs front to back), nothing is atomic: runs are bitwise reproducible.  MFMA:
// v_mfma_f32_32x32x2_f32 only -- the Gaussian window makes activation magnitudes collapse by orders, which rules the split-fp16
// operand path out.
#include "internal.h"

#include <cmath>

namespace inr {

namespace {

constexpr int WIRE_BM = 64, WIRE_BN = 64, WIRE_KB = 32;
constexpr int WIRE_LDS = WIRE_KB + 4;       // LDS row pitch in floats (144 B: 16-byte fragment reads, off one bank)
constexpr int WIRE_PG_LDS = 64 + 4;         // parameter-gradient tiles are [k][64]
constexpr int WIRE_THREADS = 256;
constexpr int64_t WIRE_MAX_ROWS = (1ll << 31) - 256;
constexpr int WIRE_SLAB_ROWS = 2048;       // rows per parameter-gradient slab: more rows than this split the sum
// (a slab per WIRE_SLAB_ROWS rows rides on a grid's y / z axis, which ends at 65,535; the input-gradient mode keeps the limit)
constexpr int64_t WIRE_MAX_STASH_ROWS = 65535ll * WIRE_SLAB_ROWS;

enum { WIRE_WS_INFER = 0, WIRE_WS_TRAIN = 1, WIRE_WS_INPUT_GRAD = 2 };     // inr_wire_workspace_bytes' third argument

enum { WIRE_EPI_GABOR = 0, WIRE_EPI_STORE = 1 };

// ---- x [n][in] -> [n][K0] with zero pad columns
__global__ void __launch_bounds__(256) wire_pad_kernel(float* __restrict__ out, const float* __restrict__ x, long long n, int in_f,
                                                       int K0) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * K0) return;
    const long long row = t / K0;
    const int k = (int)(t - row * K0);
    out[t] = k < in_f ? x[row * in_f + k] : 0.f;
}

// ---- parameters -> block image.  Layer 0: img [2][H][K0], pb [2][H]
__global__ void __launch_bounds__(256) wire_pack_first_kernel(float* __restrict__ img, float* __restrict__ pb,
                                                              const float* __restrict__ lw, const float* __restrict__ lb,
                                                              const float* __restrict__ ow, const float* __restrict__ ob, int H,
                                                              int in_f, int K0) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= H * K0) return;
    const int j = t / K0, k = t - j * K0;
    img[t] = k < in_f ? lw[j * in_f + k] : 0.f;
    img[H * K0 + t] = k < in_f ? ow[j * in_f + k] : 0.f;
    if (k == 0) {
        pb[j] = lb[j];
        pb[H + j] = ob[j];
    }
}

// layer 0 transposed, for the gradient with respect to the network's input: imgT [in][2H], row k = [lw[:, k] | ow[:, k]]
__global__ void __launch_bounds__(256) wire_pack_first_t_kernel(float* __restrict__ imgT, const float* __restrict__ lw,
                                                                const float* __restrict__ ow, int H, int in_f) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= in_f * 2 * H) return;
    const int k = t / (2 * H), c = t - k * (2 * H);
    imgT[t] = c < H ? lw[c * in_f + k] : ow[(c - H) * in_f + k];
}

// complex layer: img [4][H][2H], imgT (nullable: training only) [2H][4H] = its transpose as a [4H][2H] matrix, pb [4][H]
__global__ void __launch_bounds__(256) wire_pack_complex_kernel(float* __restrict__ img, float* __restrict__ imgT,
                                                                float* __restrict__ pb, const float* __restrict__ lw,
                                                                const float* __restrict__ lb, const float* __restrict__ ow,
                                                                const float* __restrict__ ob, int H) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= H * H) return;
    const int j = t / H, k = t - j * H;
    const int K = 2 * H, R = 4 * H;
    const float v[4][2] = {{lw[2 * t], -lw[2 * t + 1]}, {lw[2 * t + 1], lw[2 * t]}, {ow[2 * t], -ow[2 * t + 1]}, {ow[2 * t + 1], ow[2 * t]}};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        img[(q * H + j) * K + k] = v[q][0];
        img[(q * H + j) * K + H + k] = v[q][1];
        if (imgT) {
            imgT[k * R + q * H + j] = v[q][0];
            imgT[(H + k) * R + q * H + j] = v[q][1];
        }
    }
    if (k == 0) {
        pb[j] = lb[2 * j];
        pb[H + j] = lb[2 * j + 1];
        pb[2 * H + j] = ob[2 * j];
        pb[3 * H + j] = ob[2 * j + 1];
    }
}

// ---- C[n][.] = A [n][K] (K a multiple of WIRE_KB, 16-byte aligned rows) times Q planes B_q [ncols][K], both K-contiguous.
// GABOR: the layer epilogue on the Q quantities of a (row, unit); out [n][2 ncols], stash (nullable) [n][Q ncols].
// STORE (Q = 1): out [n][ncols] = the product, unpadded; ncols is arbitrary here (the tile load and the store guard the column
// per lane), which is what lets the layer-0 input gradient write dx [n][in_features] for any in_features.
template <int Q, int EPI>
__global__ void __launch_bounds__(WIRE_THREADS) wire_gemm_kernel(float* __restrict__ out, float* __restrict__ stash,
                                                                 const float* __restrict__ A, const float* __restrict__ B,
                                                                 const float* __restrict__ pb, int K, int ncols, long long n_rows,
                                                                 float omega, float s2) {
    __shared__ __attribute__((aligned(16))) float As[WIRE_BM * WIRE_LDS];
    __shared__ __attribute__((aligned(16))) float Bs[Q * WIRE_BN * WIRE_LDS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, l32 = lane & 31;
    const int wr = wave >> 1, wc = wave & 1;
    const long long row0 = (long long)blockIdx.x * WIRE_BM;
    const int col0 = blockIdx.y * WIRE_BN;
    const long long plane = (long long)ncols * K;

    f32x16 acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

    for (int k0 = 0; k0 < K; k0 += WIRE_KB) {
        __syncthreads();      // the previous K block's fragment reads are done
#pragma unroll
        for (int i = 0; i < (WIRE_BM * WIRE_KB / 4) / WIRE_THREADS; ++i) {
            const int f = tid + WIRE_THREADS * i;
            const int r = f >> 3, c4 = (f & 7) * 4;
            const long long row = row0 + r;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < n_rows) v = *reinterpret_cast<const f32x4*>(A + row * K + k0 + c4);
            *reinterpret_cast<f32x4*>(As + r * WIRE_LDS + c4) = v;
            const int col = col0 + r;      // the weight tiles have the same 64 x 32 shape: the same thread map
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                f32x4 w = {0.f, 0.f, 0.f, 0.f};
                if (col < ncols) w = *reinterpret_cast<const f32x4*>(B + q * plane + (long long)col * K + k0 + c4);
                *reinterpret_cast<f32x4*>(Bs + (q * WIRE_BN + r) * WIRE_LDS + c4) = w;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k8 = 0; k8 < WIRE_KB / 8; ++k8) {
            const f32x4 fa = *reinterpret_cast<const f32x4*>(As + (wr * 32 + l32) * WIRE_LDS + 8 * k8 + 4 * hh);
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const f32x4 fb = *reinterpret_cast<const f32x4*>(Bs + (q * WIRE_BN + wc * 32 + l32) * WIRE_LDS + 8 * k8 + 4 * hh);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s], fb[s], acc[q], 0, 0, 0);
            }
        }
    }

    const int col = col0 + wc * 32 + l32;
    if (col >= ncols) return;     // per lane (no barrier follows); GABOR callers pass a multiple of 32: uniform over the wave there
    if (EPI == WIRE_EPI_STORE) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long row = row0 + wr * 32 + mfma32_acc_row(r, hh);
            if (row < n_rows) out[row * ncols + col] = acc[0][r];
        }
        return;
    }
    float bq[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) bq[q] = pb[q * ncols + col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long row = row0 + wr * 32 + mfma32_acc_row(r, hh);
        if (row >= n_rows) continue;
        float z[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) z[q] = acc[q][r] + bq[q];
        const float lin_r = z[0];
        float sq = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) sq = fmaf(z[q], z[q], sq);
        float e = -(s2 * sq);
        if (Q == 4) e = fmaf(-omega, z[1], e);       // the imaginary part of lin damps or amplifies: exp(i w lin)
        const float amp = expf(e);
        float sn, cs;
        sincos_f32_ool(omega * lin_r, sn, cs);
        out[row * (2 * ncols) + col] = amp * cs;
        out[row * (2 * ncols) + ncols + col] = amp * sn;
        if (stash) {
#pragma unroll
            for (int q = 0; q < Q; ++q) stash[row * (Q * ncols) + q * ncols + col] = z[q];
        }
    }
}

// ---- head: y = hr . w_r - hi . w_i + b_r, a wave per row (w interleaved)
__global__ void __launch_bounds__(256) wire_head_forward_kernel(float* __restrict__ y, const float* __restrict__ act,
                                                                const float* __restrict__ w, const float* __restrict__ b, int H,
                                                                long long n_rows, int use_clamp, float clamp_min) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;      // uniform over the wave
    const float* a = act + row * 2 * H;
    float part = 0.f;
    for (int k = lane; k < H; k += 64) {
        part = fmaf(a[k], w[2 * k], part);
        part = fmaf(-a[H + k], w[2 * k + 1], part);
    }
    part = wave_sum(part);
    if (lane != 0) return;
    float v = part + b[0];
    if (use_clamp) v = fmaxf(v, clamp_min);
    y[row] = v;
}

// G [n][2H] = gy (w_r | -w_i)
__global__ void __launch_bounds__(256) wire_head_backward_kernel(float* __restrict__ G, const float* __restrict__ gy,
                                                                 const float* __restrict__ w, int H, long long n_rows) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows * H) return;
    const long long row = t / H;
    const int k = (int)(t - row * H);
    const float g = gy[row];
    G[row * 2 * H + k] = g * w[2 * k];
    G[row * 2 * H + H + k] = -(g * w[2 * k + 1]);
}

// ---- backward epilogue: dZ from G = dL/d out, the stash and out, in place over the stash ([n][Q H], Q = 2 for layer 0)
//   P = Gr out_r + Gi out_i,  Qm = Gi out_r - Gr out_i
//   d lin_r = -2 s^2 lin_r P + w Qm,  d lin_i = -(w + 2 s^2 lin_i) P,  d orth_* = -2 s^2 orth_* P
template <int Q>
__global__ void __launch_bounds__(256) wire_bwd_kernel(float* __restrict__ Z, const float* __restrict__ G,
                                                       const float* __restrict__ out, int H, long long n_rows, float omega,
                                                       float s2) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows * H) return;
    const long long row = t / H;
    const int j = (int)(t - row * H);
    const float gr = G[row * 2 * H + j], gi = G[row * 2 * H + H + j];
    const float o_r = out[row * 2 * H + j], o_i = out[row * 2 * H + H + j];
    const float P = fmaf(gr, o_r, gi * o_i);
    const float Qm = fmaf(gi, o_r, -(gr * o_i));
    const float m2 = -2.f * s2 * P;
    float* z = Z + row * (Q * H) + j;
    if (Q == 4) {
        z[0] = fmaf(m2, z[0], omega * Qm);
        z[H] = fmaf(m2, z[H], -(omega * P));
        z[2 * H] = m2 * z[2 * H];
        z[3 * H] = m2 * z[3 * H];
    } else {
        z[0] = fmaf(m2, z[0], omega * Qm);
        z[H] = m2 * z[H];
    }
}

// ---- image gradient: slab[split][R][C] = sum over the split's rows of dZ[row][r] X[row][c].  R a multiple of 64, C of 32.
__global__ void __launch_bounds__(WIRE_THREADS) wire_pgrad_kernel(float* __restrict__ slabs, const float* __restrict__ dZ, int R,
                                                                  const float* __restrict__ X, int C, long long n_rows,
                                                                  int slab_rows) {
    __shared__ __attribute__((aligned(16))) float Ds[WIRE_KB * WIRE_PG_LDS];
    __shared__ __attribute__((aligned(16))) float Xs[WIRE_KB * WIRE_PG_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, l32 = lane & 31;
    const int wr = wave >> 1, wc = wave & 1;
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const long long rbeg = (long long)blockIdx.z * slab_rows;
    const long long rend = rbeg + slab_rows < n_rows ? rbeg + slab_rows : n_rows;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    for (long long k0 = rbeg; k0 < rend; k0 += WIRE_KB) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < (WIRE_KB * 64 / 4) / WIRE_THREADS; ++i) {
            const int f = tid + WIRE_THREADS * i;
            const int rr = f >> 4, c4 = (f & 15) * 4;
            const long long row = k0 + rr;
            f32x4 dv = {0.f, 0.f, 0.f, 0.f}, xv = {0.f, 0.f, 0.f, 0.f};
            if (row < rend) {
                dv = *reinterpret_cast<const f32x4*>(dZ + row * R + r0 + c4);
                if (c0 + c4 < C) xv = *reinterpret_cast<const f32x4*>(X + row * C + c0 + c4);
            }
            *reinterpret_cast<f32x4*>(Ds + rr * WIRE_PG_LDS + c4) = dv;
            *reinterpret_cast<f32x4*>(Xs + rr * WIRE_PG_LDS + c4) = xv;
        }
        __syncthreads();
#pragma unroll
        for (int k2 = 0; k2 < WIRE_KB / 2; ++k2) {
            const float a = Ds[(2 * k2 + hh) * WIRE_PG_LDS + wr * 32 + l32];
            const float b = Xs[(2 * k2 + hh) * WIRE_PG_LDS + wc * 32 + l32];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
    const int c = c0 + wc * 32 + l32;
    if (c >= C) return;       // uniform over the wave
    float* dst = slabs + (long long)blockIdx.z * R * C;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = r0 + wr * 32 + mfma32_acc_row(r, hh);
        dst[(long long)m * C + c] = acc[r];
    }
}

// ---- slab[split][C] = sum over the split's rows of g[row] X[row][c] (g nullable = 1): four row phases, summed in a fixed order
__global__ void __launch_bounds__(256) wire_colsum_kernel(float* __restrict__ slab, const float* __restrict__ X,
                                                          const float* __restrict__ g, int C, long long n_rows, int slab_rows) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const long long rbeg = (long long)blockIdx.y * slab_rows;
    const long long rend = rbeg + slab_rows < n_rows ? rbeg + slab_rows : n_rows;
    float s = 0.f;
    if (c < C)
        for (long long row = rbeg + ph; row < rend; row += 4) s = fmaf(g ? g[row] : 1.f, X[row * C + c], s);
    red[ph][cl] = s;
    __syncthreads();
    if (ph == 0 && c < C) slab[(long long)blockIdx.y * C + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

__device__ __forceinline__ float wire_slab_sum(const float* __restrict__ slab, int nslabs, long long pitch, long long idx) {
    float s = 0.f;
    for (int i = 0; i < nslabs; ++i) s += slab[i * pitch + idx];
    return s;
}

// ---- image gradient -> parameter gradient.  Layer 0: slabs [S][2H][K0], bslab [S][2H]
__global__ void __launch_bounds__(256) wire_fold_first_kernel(float* __restrict__ glw, float* __restrict__ glb,
                                                              float* __restrict__ gow, float* __restrict__ gob,
                                                              const float* __restrict__ slabs, const float* __restrict__ bslab,
                                                              int nslabs, int H, int in_f, int K0) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= H * in_f) return;
    const int j = t / in_f, k = t - j * in_f;
    const long long pitch = 2ll * H * K0;
    glw[t] = wire_slab_sum(slabs, nslabs, pitch, (long long)j * K0 + k);
    gow[t] = wire_slab_sum(slabs, nslabs, pitch, (long long)(H + j) * K0 + k);
    if (k == 0) {
        glb[j] = wire_slab_sum(bslab, nslabs, 2 * H, j);
        gob[j] = wire_slab_sum(bslab, nslabs, 2 * H, H + j);
    }
}

// complex layer: slabs [S][4H][2H], bslab [S][4H].  With a = d(lin_r)^T [hr | hi], b = d(lin_i)^T [hr | hi]:
//   grad Wr = a[., k] + b[., H + k],  grad Wi = b[., k] - a[., H + k]      (torch: grad = dL/dRe + i dL/dIm)
__global__ void __launch_bounds__(256) wire_fold_complex_kernel(float* __restrict__ glw, float* __restrict__ glb,
                                                                float* __restrict__ gow, float* __restrict__ gob,
                                                                const float* __restrict__ slabs, const float* __restrict__ bslab,
                                                                int nslabs, int H) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= H * H) return;
    const int j = t / H, k = t - j * H;
    const int K = 2 * H;
    const long long pitch = 4ll * H * K;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        float* gw = p ? gow : glw;
        float* gb = p ? gob : glb;
        const long long ra = (long long)((2 * p) * H + j) * K, rb = (long long)((2 * p + 1) * H + j) * K;
        const float a_r = wire_slab_sum(slabs, nslabs, pitch, ra + k), a_i = wire_slab_sum(slabs, nslabs, pitch, ra + H + k);
        const float b_r = wire_slab_sum(slabs, nslabs, pitch, rb + k), b_i = wire_slab_sum(slabs, nslabs, pitch, rb + H + k);
        gw[2 * t] = a_r + b_i;
        gw[2 * t + 1] = b_r - a_i;
        if (k == 0) {
            gb[2 * j] = wire_slab_sum(bslab, nslabs, 4 * H, (2 * p) * H + j);
            gb[2 * j + 1] = wire_slab_sum(bslab, nslabs, 4 * H, (2 * p + 1) * H + j);
        }
    }
}

// head: hslab [S][2H] = sum gy [hr | hi], gslab [S] = sum gy:  grad w = gy^T hr - i gy^T hi, grad b real only
__global__ void __launch_bounds__(256) wire_fold_head_kernel(float* __restrict__ gw, float* __restrict__ gb,
                                                             const float* __restrict__ hslab, const float* __restrict__ gslab,
                                                             int nslabs, int H) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= H) return;
    gw[2 * t] = wire_slab_sum(hslab, nslabs, 2 * H, t);
    gw[2 * t + 1] = -wire_slab_sum(hslab, nslabs, 2 * H, H + t);
    if (t == 0) {
        gb[0] = wire_slab_sum(gslab, nslabs, 1, 0);
        gb[1] = 0.f;
    }
}

// ------------------------------------------------------ host ------------------------------------------------------
inline unsigned wire_blocks(long long work) { return (unsigned)((work + 255) / 256); }

}  // namespace

int wire_check_desc(const char* who, const inr_wire_desc_t* d) {
    INR_REQUIRE(d != nullptr, INR_E_INVALID, "%s: wire descriptor is null", who);
    INR_REQUIRE(d->out_features == 1, INR_E_INVALID, "%s: out_features must be 1 (got %d)", who, d->out_features);
    INR_REQUIRE(d->hidden_features == 32 || d->hidden_features == 64 || d->hidden_features == 128 || d->hidden_features == 256,
                INR_E_INVALID, "%s: hidden_features must be 32, 64, 128 or 256 (got %d)", who, d->hidden_features);
    INR_REQUIRE(d->hidden_layers >= 0 && d->hidden_layers <= WIRE_MAX_LAYERS - 1, INR_E_INVALID,
                "%s: 0 <= hidden_layers <= %d (got %d)", who, WIRE_MAX_LAYERS - 1, d->hidden_layers);
    INR_REQUIRE(d->in_features >= 1 && d->in_features <= 1024, INR_E_INVALID, "%s: 1 <= in_features <= 1024 (got %d)", who,
                d->in_features);
    INR_REQUIRE(std::isfinite(d->first_omega) && std::isfinite(d->hidden_omega) && std::isfinite(d->first_scale) &&
                    std::isfinite(d->hidden_scale),
                INR_E_INVALID, "%s: omega / scale must be finite", who);
    return 0;
}

WirePlan wire_plan(const inr_wire_desc_t* d) {
    WirePlan p;
    p.in_f = d->in_features;
    p.H = d->hidden_features;
    p.L = d->hidden_layers;
    p.K0 = (int)round_up((size_t)p.in_f, WIRE_KB);
    long long off = 0;
    int e = 0;
    for (int l = 0; l <= p.L; ++l) {
        const long long wn = l == 0 ? (long long)p.H * p.in_f : 2ll * p.H * p.H;
        const long long bn = l == 0 ? p.H : 2ll * p.H;
        for (int t = 0; t < 2; ++t) {
            p.off[e++] = off;
            off += (long long)round_up((size_t)wn, 4);
            p.off[e++] = off;
            off += (long long)round_up((size_t)bn, 4);
        }
    }
    p.off[e++] = off;
    off += (long long)round_up((size_t)2 * p.H, 4);
    p.off[e++] = off;
    off += 4;
    p.total = off;
    return p;
}

namespace {

int wire_splits(int64_t n) { return (int)((n + WIRE_SLAB_ROWS - 1) / WIRE_SLAB_ROWS); }

// the images of every layer (imgT nullable: training only, the complex layers' transposes)
int wire_pack_layers(const WirePlan& p, float* const* img, float* const* imgT, float* const* pb, const float* params,
                     hipStream_t st) {
    const int H = p.H;
    hipLaunchKernelGGL(wire_pack_first_kernel, dim3(wire_blocks((long long)H * p.K0)), dim3(256), 0, st, img[0], pb[0],
                       params + p.off[0], params + p.off[1], params + p.off[2], params + p.off[3], H, p.in_f, p.K0);
    INR_LAUNCH_CHECK();
    for (int l = 1; l <= p.L; ++l) {
        hipLaunchKernelGGL(wire_pack_complex_kernel, dim3(wire_blocks((long long)H * H)), dim3(256), 0, st, img[l],
                           imgT ? imgT[l] : (float*)nullptr, pb[l], params + p.off[4 * l], params + p.off[4 * l + 1],
                           params + p.off[4 * l + 2], params + p.off[4 * l + 3], H);
        INR_LAUNCH_CHECK();
    }
    return 0;
}

// what a workspace holds: every region on a 256-byte boundary and at least one element long.  base == null: sizes only.
struct WireView {
    float* feats = nullptr;     // the dense re-sampling only: fp32 features of one chunk, ahead of everything else
    float* x0 = nullptr;
    float *img[WIRE_MAX_LAYERS], *imgT[WIRE_MAX_LAYERS], *pb[WIRE_MAX_LAYERS];     // imgT[0]: WIRE_WS_INPUT_GRAD only
    float *act[WIRE_MAX_LAYERS], *Z[WIRE_MAX_LAYERS];     // inference: act[0], act[1] ping-pong, no Z
    float *G = nullptr, *y = nullptr, *gy = nullptr, *mse_part = nullptr, *loss_sink = nullptr;
    float *slabs = nullptr, *bslab = nullptr, *hslab = nullptr, *gslab = nullptr;
    size_t total = 0;
};

WireView wire_view(const WirePlan& p, int64_t n, int mode, void* base, bool with_feats = false) {
    WireView v;
    const bool training = mode != WIRE_WS_INFER;
    WsCarver c(base, 64 * sizeof(float));
    auto take = [&](size_t floats) { return c.take<float>(floats ? floats : 1); };
    const size_t H = (size_t)p.H, N = (size_t)n;
    if (with_feats) v.feats = take(N * p.in_f);
    v.x0 = take(N * p.K0);
    for (int l = 0; l <= p.L; ++l) {
        v.img[l] = take(l == 0 ? 2 * H * p.K0 : 8 * H * H);
        if (l == 0)
            v.imgT[l] = mode == WIRE_WS_INPUT_GRAD ? take((size_t)p.in_f * 2 * H) : nullptr;
        else
            v.imgT[l] = training ? take(8 * H * H) : nullptr;
        v.pb[l] = take(4 * H);
    }
    if (!training) {
        v.act[0] = take(N * 2 * H);
        v.act[1] = take(N * 2 * H);
    } else {
        for (int l = 0; l <= p.L; ++l) {
            v.act[l] = take(N * 2 * H);
            v.Z[l] = take(N * (l == 0 ? 2 : 4) * H);
        }
        v.G = take(N * 2 * H);
        if (mode == WIRE_WS_INPUT_GRAD) {       // no loss, no parameter gradients: y and gy are the caller's
            v.total = c.bytes();
            return v;
        }
        const size_t S = (size_t)wire_splits(n);
        const size_t img_max = p.L > 0 && 8 * H * H > 2 * H * p.K0 ? 8 * H * H : 2 * H * p.K0;
        v.y = take(N);
        v.gy = take(N);
        v.mse_part = take((size_t)mse_blocks(n > 0 ? n : 1));
        v.loss_sink = take(1);
        v.slabs = take(S * img_max);
        v.bslab = take(S * 4 * H);
        v.hslab = take(S * 2 * H);
        v.gslab = take(S);
    }
    v.total = c.bytes();
    return v;
}

// the workspace of one stand-alone layer (inr_wire_layer_forward): padded input x0, block image img[0], packed biases pb[0]
WireView wire_layer_view(int64_t n, int K, int H, void* base) {
    WireView v;
    WsCarver c(base, 64 * sizeof(float));
    v.x0 = c.take<float>((size_t)n * K); v.img[0] = c.take<float>(4 * (size_t)H * K); v.pb[0] = c.take<float>(4 * (size_t)H);
    v.total = c.bytes();
    return v;
}

int wire_pack(const WirePlan& p, const WireView& v, const float* params, bool training, hipStream_t st) {
    const int H = p.H;
    if (v.imgT[0]) {
        hipLaunchKernelGGL(wire_pack_first_t_kernel, dim3(wire_blocks((long long)p.in_f * 2 * H)), dim3(256), 0, st, v.imgT[0],
                           params + p.off[0], params + p.off[2], H, p.in_f);
        INR_LAUNCH_CHECK();
    }
    return wire_pack_layers(p, v.img, training ? v.imgT : nullptr, v.pb, params, st);
}

}  // namespace

// ---- the launcher wire_deriv.hip calls (internal.h) ---------------------------------------------------------------------------
int wire_pack_images(const WirePlan& p, float* const* img, float* const* pb, const float* params, hipStream_t st) {
    return wire_pack_layers(p, img, nullptr, pb, params, st);
}

namespace {

// in [n][K] (K a multiple of 32) times the block image img [Q][H][K] (Q = 2 for the real first layer, else 4), Gabor epilogue:
// out [n][2H] = [out_r | out_i]; stash (nullable) [n][Q H] receives lin_r (, lin_i), orth_r (, orth_i)
int wire_gabor_forward(float* out, float* stash, const float* in, const float* img, const float* pb, int K, int H, int first,
                       int64_t n, float omega, float s2, hipStream_t st) {
    const dim3 grid((unsigned)((n + WIRE_BM - 1) / WIRE_BM), (unsigned)((H + WIRE_BN - 1) / WIRE_BN));
    if (first)
        hipLaunchKernelGGL((wire_gemm_kernel<2, WIRE_EPI_GABOR>), grid, dim3(WIRE_THREADS), 0, st, out, stash, in, img, pb, K, H,
                           (long long)n, omega, s2);
    else
        hipLaunchKernelGGL((wire_gemm_kernel<4, WIRE_EPI_GABOR>), grid, dim3(WIRE_THREADS), 0, st, out, stash, in, img, pb, K, H,
                           (long long)n, omega, s2);
    INR_LAUNCH_CHECK();
    return 0;
}

// G [n][2H] = dZ [n][4H] times the image, read through its transpose imgT [2H][4H]
int wire_input_grad(float* G, const float* dZ, const float* imgT, int H, int64_t n, hipStream_t st) {
    const dim3 grid((unsigned)((n + WIRE_BM - 1) / WIRE_BM), (unsigned)(2 * H / WIRE_BN));
    hipLaunchKernelGGL((wire_gemm_kernel<1, WIRE_EPI_STORE>), grid, dim3(WIRE_THREADS), 0, st, G, (float*)nullptr, dZ, imgT,
                       (const float*)nullptr, 4 * H, 2 * H, (long long)n, 0.f, 0.f);
    INR_LAUNCH_CHECK();
    return 0;
}

// dx [n][in_f] (unpadded, any in_f) = dZ0 [n][2H] times the real layer-0 image, read through its transpose imgT0 [in_f][2H]
int wire_first_input_grad(float* dx, const float* dZ0, const float* imgT0, int in_f, int H, int64_t n, hipStream_t st) {
    const dim3 grid((unsigned)((n + WIRE_BM - 1) / WIRE_BM), (unsigned)((in_f + WIRE_BN - 1) / WIRE_BN));
    hipLaunchKernelGGL((wire_gemm_kernel<1, WIRE_EPI_STORE>), grid, dim3(WIRE_THREADS), 0, st, dx, (float*)nullptr, dZ0, imgT0,
                       (const float*)nullptr, 2 * H, in_f, (long long)n, 0.f, 0.f);
    INR_LAUNCH_CHECK();
    return 0;
}

// slabs [splits][R][C] = per-split dZ^T X and bslab [splits][R] = per-split column sums of dZ (dZ [n][R], X [n][C])
int wire_param_grad_slabs(float* slabs, float* bslab, const float* dZ, int R, const float* X, int C, int64_t n, hipStream_t st) {
    const int S = wire_splits(n);
    hipLaunchKernelGGL(wire_pgrad_kernel, dim3((unsigned)(R / 64), (unsigned)((C + 63) / 64), (unsigned)S), dim3(WIRE_THREADS), 0,
                       st, slabs, dZ, R, X, C, (long long)n, WIRE_SLAB_ROWS);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(wire_colsum_kernel, dim3((unsigned)(R / 64), (unsigned)S), dim3(256), 0, st, bslab, dZ, (const float*)nullptr,
                       R, (long long)n, WIRE_SLAB_ROWS);
    INR_LAUNCH_CHECK();
    return 0;
}

// rows already in v.x0.  training: stash everything, result in v.y; else ping-pong and write y_out (with the clamp)
int wire_forward_layers(const inr_wire_desc_t* d, const WirePlan& p, const WireView& v, const float* params, int64_t n,
                        bool training, float* y_out, int use_clamp, float clamp_min, hipStream_t st) {
    const int H = p.H;
    const float s2_first = d->first_scale * d->first_scale, s2_hidden = d->hidden_scale * d->hidden_scale;
    const float* in = v.x0;
    float* out = nullptr;
    for (int l = 0; l <= p.L; ++l) {
        out = training ? v.act[l] : v.act[l & 1];
        if (int rc = wire_gabor_forward(out, training ? v.Z[l] : nullptr, in, v.img[l], v.pb[l], l == 0 ? p.K0 : 2 * H, H, l == 0, n,
                                        l == 0 ? d->first_omega : d->hidden_omega, l == 0 ? s2_first : s2_hidden, st))
            return rc;
        in = out;
    }
    hipLaunchKernelGGL(wire_head_forward_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, y_out, in,
                       params + p.off[4 * (p.L + 1)], params + p.off[4 * (p.L + 1) + 1], H, (long long)n, use_clamp, clamp_min);
    INR_LAUNCH_CHECK();
    return 0;
}

int wire_pad_rows(const WirePlan& p, const WireView& v, const float* x, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(wire_pad_kernel, dim3(wire_blocks((long long)n * p.K0)), dim3(256), 0, st, v.x0, x, (long long)n, p.in_f,
                       p.K0);
    INR_LAUNCH_CHECK();
    return 0;
}

// one loss + gradient evaluation on the rows in v.x0 (images packed from `params` first)
int wire_loss_grad_impl(const inr_wire_desc_t* d, const WirePlan& p, const WireView& v, const float* params, float* grads,
                        const float* target, const float* weight, int64_t n, float* loss, hipStream_t st) {
    const int H = p.H, S = wire_splits(n);
    const float s2_first = d->first_scale * d->first_scale, s2_hidden = d->hidden_scale * d->hidden_scale;
    const long long* off = p.off;
    const int head = 4 * (p.L + 1);
    if (int rc = wire_pack(p, v, params, true, st)) return rc;
    if (int rc = wire_forward_layers(d, p, v, params, n, true, v.y, 0, 0.f, st)) return rc;
    if (int rc = launch_mse(v.gy, loss ? loss : v.loss_sink, v.y, target, weight, n, v.mse_part, st)) return rc;
    // head: G = gy (w_r, -w_i); weight gradient = gy-weighted column sums of the last activations, bias gradient = sum gy
    hipLaunchKernelGGL(wire_head_backward_kernel, dim3(wire_blocks((long long)n * H)), dim3(256), 0, st, v.G, v.gy,
                       params + off[head], H, (long long)n);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(wire_colsum_kernel, dim3((unsigned)(2 * H / 64), (unsigned)S), dim3(256), 0, st, v.hslab, v.act[p.L],
                       (const float*)v.gy, 2 * H, (long long)n, WIRE_SLAB_ROWS);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(wire_colsum_kernel, dim3(1, (unsigned)S), dim3(256), 0, st, v.gslab, (const float*)v.gy, (const float*)nullptr,
                       1, (long long)n, WIRE_SLAB_ROWS);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(wire_fold_head_kernel, dim3(wire_blocks(H)), dim3(256), 0, st, grads + off[head], grads + off[head + 1],
                       v.hslab, v.gslab, S, H);
    INR_LAUNCH_CHECK();
    for (int l = p.L; l >= 0; --l) {
        const long long work = (long long)n * H;
        if (l > 0) {
            hipLaunchKernelGGL(wire_bwd_kernel<4>, dim3(wire_blocks(work)), dim3(256), 0, st, v.Z[l], v.G, v.act[l], H, (long long)n,
                               d->hidden_omega, s2_hidden);
            INR_LAUNCH_CHECK();
            if (int rc = wire_param_grad_slabs(v.slabs, v.bslab, v.Z[l], 4 * H, v.act[l - 1], 2 * H, n, st)) return rc;
            hipLaunchKernelGGL(wire_fold_complex_kernel, dim3(wire_blocks((long long)H * H)), dim3(256), 0, st, grads + off[4 * l],
                               grads + off[4 * l + 1], grads + off[4 * l + 2], grads + off[4 * l + 3], v.slabs, v.bslab, S, H);
            INR_LAUNCH_CHECK();
            if (int rc = wire_input_grad(v.G, v.Z[l], v.imgT[l], H, n, st)) return rc;
        } else {
            hipLaunchKernelGGL(wire_bwd_kernel<2>, dim3(wire_blocks(work)), dim3(256), 0, st, v.Z[0], v.G, v.act[0], H, (long long)n,
                               d->first_omega, s2_first);
            INR_LAUNCH_CHECK();
            if (int rc = wire_param_grad_slabs(v.slabs, v.bslab, v.Z[0], 2 * H, v.x0, p.K0, n, st)) return rc;
            hipLaunchKernelGGL(wire_fold_first_kernel, dim3(wire_blocks((long long)H * p.in_f)), dim3(256), 0, st, grads + off[0],
                               grads + off[1], grads + off[2], grads + off[3], v.slabs, v.bslab, S, H, p.in_f, p.K0);
            INR_LAUNCH_CHECK();
        }
    }
    return 0;
}

int wire_check_train(const char* who, const inr_wire_desc_t* desc, const void* params, const void* grads, const void* x,
                     const void* target, int64_t n, void* workspace, size_t workspace_bytes, WirePlan& p, WireView& v) {
    if (int rc = wire_check_desc(who, desc)) return rc;
    INR_REQUIRE(params && grads && x && target, INR_E_INVALID, "%s: null pointer", who);
    INR_REQUIRE(n >= 1 && n <= WIRE_MAX_STASH_ROWS, INR_E_INVALID, "%s: bad row count %lld", who, (long long)n);
    p = wire_plan(desc);
    v = wire_view(p, n, WIRE_WS_TRAIN, workspace);
    INR_REQUIRE(workspace && workspace_bytes >= v.total, INR_E_WORKSPACE, "%s: workspace too small (%zu bytes, %zu needed)", who,
                workspace ? workspace_bytes : (size_t)0, v.total);
    INR_REQUIRE(aligned16(params) && aligned16(grads) && aligned16(workspace), INR_E_ALIGN,
                "%s: params, grads and workspace must be 16-byte aligned", who);
    return 0;
}

// the two halves of the input gradient share their refusals (and so their view): `a`, `b` are the call's two row arrays
int wire_check_stash(const char* who, const inr_wire_desc_t* desc, const void* params, const void* a, const void* b, int64_t n,
                     void* workspace, size_t workspace_bytes, WirePlan& p, WireView& v) {
    if (int rc = wire_check_desc(who, desc)) return rc;
    INR_REQUIRE(params && a && b, INR_E_INVALID, "%s: null pointer", who);
    INR_REQUIRE(n >= 1 && n <= WIRE_MAX_STASH_ROWS, INR_E_INVALID, "%s: bad row count %lld", who, (long long)n);
    p = wire_plan(desc);
    v = wire_view(p, n, WIRE_WS_INPUT_GRAD, workspace);
    INR_REQUIRE(workspace && workspace_bytes >= v.total, INR_E_WORKSPACE, "%s: workspace too small (%zu bytes, %zu needed)", who,
                workspace ? workspace_bytes : (size_t)0, v.total);
    INR_REQUIRE(aligned16(params) && aligned16(workspace), INR_E_ALIGN, "%s: params and workspace must be 16-byte aligned", who);
    return 0;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_wire_param_count(const inr_wire_desc_t* desc) {
    if (wire_check_desc("inr_wire_param_count", desc)) return -1;
    return wire_plan(desc).total;
}

int inr_wire_param_offsets(const inr_wire_desc_t* desc, int64_t* offsets, int max_entries) {
    if (int rc = wire_check_desc("inr_wire_param_offsets", desc)) return rc;
    INR_REQUIRE(offsets != nullptr, INR_E_INVALID, "inr_wire_param_offsets: offsets is null");
    const WirePlan p = wire_plan(desc);
    const int entries = 4 * (p.L + 1) + 2;
    INR_REQUIRE(max_entries >= entries, INR_E_INVALID, "inr_wire_param_offsets: %d entries needed (room for %d)", entries,
                max_entries);
    for (int e = 0; e < entries; ++e) offsets[e] = p.off[e];
    return 0;
}

size_t inr_wire_layer_workspace_bytes(int64_t n, int in_features, int out_features) {
    if (n < 1 || n > WIRE_MAX_ROWS || in_features < 1 || in_features > 1024 || out_features < 32 || out_features > 256) return 0;
    return wire_layer_view(n, (int)round_up((size_t)in_features, WIRE_KB), out_features, nullptr).total;
}

// INRmodel.py:109-120 `ComplexGaborLayer2D.forward` of one layer.  is_first: x [n][in] real, real weights; else x [n][2H] planes
// [re | im] with in_features == out_features == H and interleaved complex weights.  out [n][2H] planes [re | im].
int inr_wire_layer_forward(float* out, const float* x, const float* lin_w, const float* lin_b, const float* orth_w,
                           const float* orth_b, int64_t n, int in_features, int out_features, int is_first, float omega, float scale,
                           void* workspace, size_t workspace_bytes, void* stream) {
    const int H = out_features;
    INR_REQUIRE(out && x && lin_w && lin_b && orth_w && orth_b, INR_E_INVALID, "inr_wire_layer_forward: null pointer");
    INR_REQUIRE(H == 32 || H == 64 || H == 128 || H == 256, INR_E_INVALID,
                "inr_wire_layer_forward: out_features must be 32, 64, 128 or 256 (got %d)", H);
    INR_REQUIRE(in_features >= 1 && in_features <= 1024, INR_E_INVALID, "inr_wire_layer_forward: 1 <= in_features <= 1024 (got %d)",
                in_features);
    INR_REQUIRE(is_first || in_features == H, INR_E_INVALID,
                "inr_wire_layer_forward: a complex layer needs in_features == out_features (got %d, %d)", in_features, H);
    INR_REQUIRE(n >= 0 && n <= WIRE_MAX_ROWS, INR_E_INVALID, "inr_wire_layer_forward: bad row count %lld", (long long)n);
    INR_REQUIRE(std::isfinite(omega) && std::isfinite(scale), INR_E_INVALID, "inr_wire_layer_forward: omega / scale must be finite");
    if (n == 0) return 0;
    const int K = (int)round_up((size_t)(is_first ? in_features : 2 * H), WIRE_KB);
    const WireView v = wire_layer_view(n, K, H, workspace);
    INR_REQUIRE(workspace && workspace_bytes >= v.total, INR_E_WORKSPACE, "inr_wire_layer_forward: workspace too small (%zu bytes, %zu needed)",
                workspace ? workspace_bytes : (size_t)0, v.total);
    INR_REQUIRE(aligned16(workspace) && aligned16(out) && aligned16(x), INR_E_ALIGN,
                "inr_wire_layer_forward: out, x and workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float *const x0 = v.x0, *const img = v.img[0], *const pb = v.pb[0];
    const float* in = x;
    if (is_first) {
        hipLaunchKernelGGL(wire_pack_first_kernel, dim3(wire_blocks((long long)H * K)), dim3(256), 0, st, img, pb, lin_w, lin_b, orth_w,
                           orth_b, H, in_features, K);
        INR_LAUNCH_CHECK();
        hipLaunchKernelGGL(wire_pad_kernel, dim3(wire_blocks((long long)n * K)), dim3(256), 0, st, x0, x, (long long)n, in_features, K);
        INR_LAUNCH_CHECK();
        in = x0;
    } else {
        hipLaunchKernelGGL(wire_pack_complex_kernel, dim3(wire_blocks((long long)H * H)), dim3(256), 0, st, img, (float*)nullptr, pb,
                           lin_w, lin_b, orth_w, orth_b, H);
        INR_LAUNCH_CHECK();
    }
    return wire_gabor_forward(out, nullptr, in, img, pb, K, H, is_first, n, omega, scale * scale, st);
}

size_t inr_wire_workspace_bytes(const inr_wire_desc_t* desc, int64_t n, int training) {
    if (wire_check_desc("inr_wire_workspace_bytes", desc)) return 0;
    // (any non-zero mode other than the input-gradient one is the training workspace, as before)
    const int mode = training == WIRE_WS_INPUT_GRAD ? WIRE_WS_INPUT_GRAD : training != 0 ? WIRE_WS_TRAIN : WIRE_WS_INFER;
    if (n < 1 || n > (mode ? WIRE_MAX_STASH_ROWS : WIRE_MAX_ROWS)) {
        set_error("inr_wire_workspace_bytes: bad row count %lld", (long long)n);
        return 0;
    }
    return wire_view(wire_plan(desc), n, mode, nullptr).total;
}

// wiretest.ipynb cell 2 `Siren.forward` = nn.Sequential of ComplexGaborLayer2D.forward (INRmodel.py:109-120) + final_linear, .real
int inr_wire_forward(const inr_wire_desc_t* desc, const float* params, const float* x, int64_t n, float* y, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (int rc = wire_check_desc("inr_wire_forward", desc)) return rc;
    INR_REQUIRE(params && x && y, INR_E_INVALID, "inr_wire_forward: null pointer");
    INR_REQUIRE(n >= 0 && n <= WIRE_MAX_ROWS, INR_E_INVALID, "inr_wire_forward: bad row count %lld", (long long)n);
    if (n == 0) return 0;
    const WirePlan p = wire_plan(desc);
    const WireView v = wire_view(p, n, WIRE_WS_INFER, workspace);
    INR_REQUIRE(workspace && workspace_bytes >= v.total, INR_E_WORKSPACE, "inr_wire_forward: workspace too small (%zu bytes, %zu needed)",
                workspace ? workspace_bytes : (size_t)0, v.total);
    INR_REQUIRE(aligned16(params) && aligned16(workspace), INR_E_ALIGN, "inr_wire_forward: params and workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = wire_pack(p, v, params, false, st)) return rc;
    if (int rc = wire_pad_rows(p, v, x, n, st)) return rc;
    return wire_forward_layers(desc, p, v, params, n, false, y, 0, 0.f, st);
}

size_t inr_wire_reconstruct_workspace_bytes(const inr_wire_desc_t* desc, int64_t chunk_rows) {
    if (wire_check_desc("inr_wire_reconstruct_workspace_bytes", desc)) return 0;
    if (chunk_rows < 1 || chunk_rows > WIRE_MAX_ROWS) {
        set_error("inr_wire_reconstruct_workspace_bytes: bad chunk_rows %lld", (long long)chunk_rows);
        return 0;
    }
    return wire_view(wire_plan(desc), chunk_rows, WIRE_WS_INFER, nullptr, true).total;
}

// wiretest.ipynb cell 9-10: get_mgrid -> input_mapping -> INR.forward -> torch.clamp(min=0), on chunks of the grid
int inr_wire_reconstruct(const inr_wire_desc_t* desc, const float* params, const int64_t* shape, int dim, const float* B, int m,
                         float* y, int use_clamp, float clamp_min, int64_t chunk_rows, void* workspace, size_t workspace_bytes,
                         void* stream) {
    if (int rc = wire_check_desc("inr_wire_reconstruct", desc)) return rc;
    INR_REQUIRE(params && shape && y, INR_E_INVALID, "inr_wire_reconstruct: null pointer");
    INR_REQUIRE(dim >= 1 && dim <= 8, INR_E_INVALID, "inr_wire_reconstruct: dim must be 1..8");
    INR_REQUIRE(chunk_rows >= 1 && chunk_rows <= WIRE_MAX_ROWS, INR_E_INVALID, "inr_wire_reconstruct: bad chunk_rows");
    if (B)
        INR_REQUIRE(m >= 1 && 2 * m == desc->in_features, INR_E_INVALID, "inr_wire_reconstruct: in_features (%d) must equal 2*m (%d)",
                    desc->in_features, 2 * m);
    else
        INR_REQUIRE(dim == desc->in_features, INR_E_INVALID,
                    "inr_wire_reconstruct: without B the grid dim (%d) must equal in_features (%d)", dim, desc->in_features);
    int64_t total;
    if (int rc = check_grid_shape("inr_wire_reconstruct", shape, dim, WIRE_MAX_ROWS, &total)) return rc;
    const WirePlan p = wire_plan(desc);
    const WireView v = wire_view(p, chunk_rows, WIRE_WS_INFER, workspace, true);
    INR_REQUIRE(workspace && workspace_bytes >= v.total, INR_E_WORKSPACE, "inr_wire_reconstruct: workspace too small (%zu bytes, %zu needed)",
                workspace ? workspace_bytes : (size_t)0, v.total);
    INR_REQUIRE(aligned16(params) && aligned16(workspace), INR_E_ALIGN,
                "inr_wire_reconstruct: params and workspace must be 16-byte aligned");
    float* const feats = v.feats;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = wire_pack(p, v, params, false, st)) return rc;
    for (int64_t r0 = 0; r0 < total; r0 += chunk_rows) {
        const int64_t rows = (total - r0 < chunk_rows) ? (total - r0) : chunk_rows;
        int rc = B ? launch_fourier(feats, nullptr, shape, dim, r0, rows, B, m, st) : launch_mgrid(feats, shape, dim, r0, rows, st);
        if (rc) return rc;
        if ((rc = wire_pad_rows(p, v, feats, rows, st))) return rc;
        if ((rc = wire_forward_layers(desc, p, v, params, rows, false, y + r0, use_clamp, clamp_min, st))) return rc;
    }
    return 0;
}

// wiretest.ipynb cell 10: loss = ((INR.forward(model_input) - LR_ground_truth)**2).mean(); loss.backward()
int inr_wire_loss_grad(const inr_wire_desc_t* desc, const float* params, float* grads, const float* x, const float* target,
                       const float* weight, int64_t n, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    WirePlan p;
    WireView v;
    if (int rc = wire_check_train("inr_wire_loss_grad", desc, params, grads, x, target, n, workspace, workspace_bytes, p, v)) return rc;
    hipStream_t st = (hipStream_t)stream;
    INR_HIP(hipMemsetAsync(grads, 0, (size_t)p.total * sizeof(float), st));      // the padding between tensors
    if (int rc = wire_pad_rows(p, v, x, n, st)) return rc;
    return wire_loss_grad_impl(desc, p, v, params, grads, target, weight, n, loss, st);
}

// wiretest.ipynb cell 10's PerturbNet branch, first half: `model_output = INR.forward(perturbed_input)` with everything the
// backward needs left in the workspace.  The kernels of inr_wire_loss_grad's forward: y is bit-equal with inr_wire_forward's.
int inr_wire_forward_stash(const inr_wire_desc_t* desc, const float* params, const float* x, int64_t n, float* y, void* workspace,
                           size_t workspace_bytes, void* stream) {
    WirePlan p;
    WireView v;
    if (int rc = wire_check_stash("inr_wire_forward_stash", desc, params, x, y, n, workspace, workspace_bytes, p, v)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = wire_pack(p, v, params, true, st)) return rc;
    if (int rc = wire_pad_rows(p, v, x, n, st)) return rc;
    return wire_forward_layers(desc, p, v, params, n, true, y, 0, 0.f, st);
}

// ... second half: `loss.backward()` as far as the network's input, dx [n][in_features] = gy[row] dy[row]/dx[row].  Consumes the
// stash (dZ overwrites it layer by layer): one call per inr_wire_forward_stash.  No forward runs here and no parameter gradient
// is formed -- the notebook's next inr_optim.zero_grad() would discard it.
int inr_wire_input_grad(const inr_wire_desc_t* desc, const float* params, const float* gy, int64_t n, float* dx, void* workspace,
                        size_t workspace_bytes, void* stream) {
    WirePlan p;
    WireView v;
    if (int rc = wire_check_stash("inr_wire_input_grad", desc, params, gy, dx, n, workspace, workspace_bytes, p, v)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int H = p.H;
    const long long work = (long long)n * H;
    hipLaunchKernelGGL(wire_head_backward_kernel, dim3(wire_blocks(work)), dim3(256), 0, st, v.G, gy, params + p.off[4 * (p.L + 1)],
                       H, (long long)n);
    INR_LAUNCH_CHECK();
    for (int l = p.L; l > 0; --l) {
        hipLaunchKernelGGL(wire_bwd_kernel<4>, dim3(wire_blocks(work)), dim3(256), 0, st, v.Z[l], v.G, v.act[l], H, (long long)n,
                           desc->hidden_omega, desc->hidden_scale * desc->hidden_scale);
        INR_LAUNCH_CHECK();
        if (int rc = wire_input_grad(v.G, v.Z[l], v.imgT[l], H, n, st)) return rc;
    }
    hipLaunchKernelGGL(wire_bwd_kernel<2>, dim3(wire_blocks(work)), dim3(256), 0, st, v.Z[0], v.G, v.act[0], H, (long long)n,
                       desc->first_omega, desc->first_scale * desc->first_scale);
    INR_LAUNCH_CHECK();
    return wire_first_input_grad(dx, v.Z[0], v.imgT[0], p.in_f, H, n, st);
}

// wiretest.ipynb cell 10: the `ctr < number_of_epochs - pertubation_epochs` branch (forward, MSE, zero_grad, backward,
// inr_optim.step()), n_steps times
int inr_wire_fit(const inr_wire_desc_t* desc, float* params, float* grads, float* m, float* v_, const float* x, const float* target,
                 const float* weight, int64_t n, int64_t first_step, int n_steps, double lr, double beta1, double beta2, double eps,
                 float* losses, void* workspace, size_t workspace_bytes, void* stream) {
    WirePlan p;
    WireView v;
    if (int rc = wire_check_train("inr_wire_fit", desc, params, grads, x, target, n, workspace, workspace_bytes, p, v)) return rc;
    INR_REQUIRE(m && v_, INR_E_INVALID, "inr_wire_fit: null Adam state");
    INR_REQUIRE(first_step >= 1 && n_steps >= 0, INR_E_INVALID, "inr_wire_fit: first_step >= 1 and n_steps >= 0 (got %lld, %d)",
                (long long)first_step, n_steps);
    INR_REQUIRE(aligned16(m) && aligned16(v_), INR_E_ALIGN, "inr_wire_fit: m and v must be 16-byte aligned");
    if (n_steps == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    INR_HIP(hipMemsetAsync(grads, 0, (size_t)p.total * sizeof(float), st));
    if (int rc = wire_pad_rows(p, v, x, n, st)) return rc;
    for (int it = 0; it < n_steps; ++it) {
        if (int rc = wire_loss_grad_impl(desc, p, v, params, grads, target, weight, n, losses ? losses + it : nullptr, st)) return rc;
        if (int rc = launch_adam(params, grads, m, v_, p.total, first_step + it, lr, beta1, beta2, eps, st)) return rc;
    }
    return 0;
}

}  // extern "C"
