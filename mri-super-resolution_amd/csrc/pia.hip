// PIA, the physics-informed autoencoder of the reference's PIA.py:16-155, on gfx950.
//
//   encoder   n_signals -> hidden[0] -> ... -> hidden[L-1], every layer Linear + LeakyReLU          (PIA.py:47-59)
//   heads     three predictors (D, T2, v): hidden[L-1] -> hidden[L-1] (LeakyReLU) -> 3              (PIA.py:61-93)
//   encode    D = D_mean + D_delta tanh(.) (float64), T2 = T2_mean + T2_delta tanh(.), v = softmax  (PIA.py:97-110)
//   decode    signal[a] = 1000 * float(sum_c v_c exp(-b_a / 1000 D_c) exp(-TE_a / T2_c))            (PIA.py:112-130)
//
// Kernels of this file (all arithmetic of forward, backward and the fit step):
//   pia_gemm_kernel  one tiled GEMM on the exact f32-input MFMA (v_mfma_f32_16x16x4_f32), three epilogues:
//                    FWD  act = leaky(x W^T + b)            (the three head hidden layers ride as grid.z = 3 on one shared input)
//                    DX   dz_prev = (sum_seg dz_seg W_seg) * leaky'(act_prev)   (the heads' three products are one K-loop of 3 segments)
//                    DW   gW = dz^T x, gb = colsum(dz): K = rows, split over grid.z into slabs (fixed-order reduction afterwards)
//   pia_head_kernel  a wave owns a row: the nine 512-wide dot products of the 512 -> 3 outputs, tanh / softmax, the decoder
//                    with its float64 D branch, and -- in training -- the loss term, the decoder's backward, dz of the head
//                    hidden layers and the row's share of the 512 -> 3 parameter gradients.  Backward re-computes the nine
//                    outputs from the stashed hidden activation, so a training forward stashes activations only; the
//                    LeakyReLU derivative is the activation's sign.
//   pia_pids_kernel  detect_PIDS_slice (PIA.py:286-327)
// Gradient reduction, loss and Adam are the fused step's launch_finalize (kernels.hip): no float atomics anywhere.
#include "internal.h"

namespace inr {

namespace {

struct __attribute__((packed, aligned(4))) f4u {   // four floats at 4-byte alignment: tensors of the flat parameter buffer start anywhere
    float x, y, z, w;
};

constexpr int PIA_BK = 16;
enum { PIA_FWD = 0, PIA_DX = 1, PIA_DW = 2 };

struct PiaGemm {
    const float* A[3];
    const float* B[3];
    float* C[3];
    const float* bias[3];   // FWD: bias per output column
    const float* act[3];    // DX: the activation whose sign selects the LeakyReLU derivative ([M][ldc])
    float* colsum[3];       // DW: bias gradient rows (beside C in the slab)
    long long M, N, K;      // C is M x N; K per segment
    long long lda, ldb, ldc;
    int nseg;               // DX: K segments accumulated into one product (A[s], B[s])
    int splits;             // DW: K split into `splits` slabs
    long long slab_stride;  // DW: floats between two slabs of C (and of colsum)
    float slope;
};

template <int WM, int WN, bool A_KC, bool B_KC, int EPI>
__global__ void __launch_bounds__(256) pia_gemm_kernel(const PiaGemm p) {
    constexpr int BM = 32 * WM, BN = 32 * WN;
    constexpr int NA = BM / 64, NB = BN / 64;   // float4 loads per thread and stage
    __shared__ __attribute__((aligned(16))) float As[PIA_BK][BM + 4];
    __shared__ __attribute__((aligned(16))) float Bs[PIA_BK][BN + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const long long m0 = (long long)blockIdx.x * BM, n0 = (long long)blockIdx.y * BN;
    const int batch = EPI == PIA_DW ? (int)blockIdx.z / p.splits : (int)blockIdx.z;
    const int split = EPI == PIA_DW ? (int)blockIdx.z % p.splits : 0;
    long long kbeg = 0, kend = p.K;
    if (EPI == PIA_DW) {
        long long chunk = (p.K + p.splits - 1) / p.splits;
        chunk = (chunk + PIA_BK - 1) / PIA_BK * PIA_BK;
        kbeg = (long long)split * chunk;
        kend = kbeg + chunk < p.K ? kbeg + chunk : p.K;
        if (kbeg > kend) kbeg = kend;
    }
    const long long ksteps = (kend - kbeg + PIA_BK - 1) / PIA_BK;
    const long long T = ksteps * (EPI == PIA_DX ? p.nseg : 1);

    f32x4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float csum = 0.f;

    // Precondition of the guards below: a four-float read is checked on its FIRST element only.  Along m / n that is enough because
    // every feature width is a multiple of 16 (pia_kernel_shape).  Along k it needs K % 4 == 0 in the K-contiguous layouts (FWD, DX:
    // K is a feature width); DW, whose K is the row count and may be anything, reads both operands in the other layout.
    static_assert(EPI != PIA_DW || (!A_KC && !B_KC), "DW contracts over rows: its operands must not be read four-wide along k");
    f4u ra[NA], rb[NB];
    auto load = [&](long long t) {
        const int seg = EPI == PIA_DX ? (int)(t / ksteps) : batch;
        const long long k0 = kbeg + (t % ksteps) * PIA_BK;
        const float* __restrict__ Ap = p.A[seg];
        const float* __restrict__ Bp = p.B[seg];
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int idx = tid + i * 256;
            long long m, k;
            if (A_KC) { m = m0 + idx / 4; k = k0 + (idx % 4) * 4; }
            else      { k = k0 + idx / (BM / 4); m = m0 + (idx % (BM / 4)) * 4; }
            const bool ok = m < p.M && k < kend;
            ra[i] = ok ? *reinterpret_cast<const f4u*>(Ap + (A_KC ? m * p.lda + k : k * p.lda + m)) : f4u{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = tid + i * 256;
            long long n, k;
            if (B_KC) { n = n0 + idx / 4; k = k0 + (idx % 4) * 4; }
            else      { k = k0 + idx / (BN / 4); n = n0 + (idx % (BN / 4)) * 4; }
            const bool ok = n < p.N && k < kend;
            rb[i] = ok ? *reinterpret_cast<const f4u*>(Bp + (B_KC ? n * p.ldb + k : k * p.ldb + n)) : f4u{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int idx = tid + i * 256;
            if (A_KC) {
                const int m = idx / 4, k = (idx % 4) * 4;
                As[k][m] = ra[i].x; As[k + 1][m] = ra[i].y; As[k + 2][m] = ra[i].z; As[k + 3][m] = ra[i].w;
            } else {
                const int k = idx / (BM / 4), m = (idx % (BM / 4)) * 4;
                *reinterpret_cast<f32x4*>(&As[k][m]) = f32x4{ra[i].x, ra[i].y, ra[i].z, ra[i].w};
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = tid + i * 256;
            if (B_KC) {
                const int n = idx / 4, k = (idx % 4) * 4;
                Bs[k][n] = rb[i].x; Bs[k + 1][n] = rb[i].y; Bs[k + 2][n] = rb[i].z; Bs[k + 3][n] = rb[i].w;
            } else {
                const int k = idx / (BN / 4), n = (idx % (BN / 4)) * 4;
                *reinterpret_cast<f32x4*>(&Bs[k][n]) = f32x4{rb[i].x, rb[i].y, rb[i].z, rb[i].w};
            }
        }
    };

    if (T > 0) load(0);
    for (long long t = 0; t < T; ++t) {
        stage();
        __syncthreads();
        if (t + 1 < T) load(t + 1);   // the next stage's global loads fly under this stage's MFMAs
        if (EPI == PIA_DW && blockIdx.y == 0 && tid < BM) {
#pragma unroll
            for (int k = 0; k < PIA_BK; ++k) csum += As[k][tid];
        }
#pragma unroll
        for (int kk = 0; kk < PIA_BK / 4; ++kk) {
            const int k = kk * 4 + (lane >> 4);
            float a[WM], b[WN];
#pragma unroll
            for (int i = 0; i < WM; ++i) a[i] = As[k][wm * 16 * WM + i * 16 + (lane & 15)];
#pragma unroll
            for (int j = 0; j < WN; ++j) b[j] = Bs[k][wn * 16 * WN + j * 16 + (lane & 15)];
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    float* __restrict__ Cp = p.C[batch] + (EPI == PIA_DW ? (long long)split * p.slab_stride : 0);
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const long long n = n0 + wn * 16 * WN + j * 16 + (lane & 15);
            if (n >= p.N) continue;
            const float bias = EPI == PIA_FWD ? p.bias[batch][n] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long m = m0 + wm * 16 * WM + i * 16 + 4 * (lane >> 4) + r;
                if (m >= p.M) continue;
                float v = acc[i][j][r];
                if (EPI == PIA_FWD) {
                    v += bias;
                    v = v > 0.f ? v : v * p.slope;
                } else if (EPI == PIA_DX) {
                    v = p.act[0][m * p.ldc + n] > 0.f ? v : v * p.slope;
                }
                Cp[m * p.ldc + n] = v;
            }
        }
    if (EPI == PIA_DW && blockIdx.y == 0 && tid < BM && m0 + tid < p.M)
        p.colsum[batch][(long long)split * p.slab_stride + m0 + tid] = csum;
}

template <bool A_KC, bool B_KC, int EPI>
int pia_launch_gemm(const PiaGemm& p, int nbatch, bool big, hipStream_t st) {
    const unsigned z = (unsigned)(EPI == PIA_DW ? nbatch * p.splits : nbatch);
    if (big) {
        dim3 grid((unsigned)((p.M + 127) / 128), (unsigned)((p.N + 127) / 128), z);
        hipLaunchKernelGGL((pia_gemm_kernel<4, 4, A_KC, B_KC, EPI>), grid, dim3(256), 0, st, p);
    } else {
        dim3 grid((unsigned)((p.M + 63) / 64), (unsigned)((p.N + 63) / 64), z);
        hipLaunchKernelGGL((pia_gemm_kernel<2, 2, A_KC, B_KC, EPI>), grid, dim3(256), 0, st, p);
    }
    INR_LAUNCH_CHECK();
    count_launch(LF_PIA_BASE + (EPI == PIA_FWD ? INR_PIA_LF_FWD : EPI == PIA_DX ? INR_PIA_LF_DX : INR_PIA_LF_DW));
    return 0;
}

// 128 x 128 tiles once they fill the chip, 64 x 64 below (and for the narrow early layers)
inline bool pia_big(long long M, long long N, int z) {
    return M >= 128 && N >= 128 && ((M + 127) / 128) * ((N + 127) / 128) * z >= 256;
}

// K splits of one parameter-gradient GEMM: enough blocks for about two rounds over the chip, at least 64 rows per split,
// at most 128 slabs (what launch_finalize sums in one stage)
int pia_dw_splits(long long n, int out_f, int in_f, int nbatch) {
    const bool big = out_f >= 128 && in_f >= 128 && n >= 4096;
    const int t = big ? 128 : 64;
    const long long tiles = (long long)((out_f + t - 1) / t) * ((in_f + t - 1) / t) * nbatch;
    long long s = (512 + tiles - 1) / tiles;
    const long long by_rows = (n + 63) / 64;
    if (s > by_rows) s = by_rows;
    if (s > 128) s = 128;
    if (s < 1) s = 1;
    return (int)s;
}

// ---- the row kernel ------------------------------------------------------------------------------------------------------------
struct PiaHead {
    const float* h[3];      // head hidden activations [n][H]
    const float* W[3];      // [3][H]
    const float* b[3];      // [3]
    float* dzh[3];          // [n][H]: gradient at the head hidden layers' pre-activation
    float* slab[3];         // [waves][3 H + 3]: per-wave share of gW, gb of the 3-wide layers
    float* signal;          // [n][16]
    double* D;              // [n][3]
    float* T2;
    float* v;
    const float* x;         // fused loss: target signals and weights (nullable = 1)
    const float* pids;
    const float* g_signal;  // external gradients (train pair), each nullable
    const double* g_D;
    const float* g_T2;
    const float* g_v;
    float* part_loss;       // [waves]
    long long n;
    double inv_count;       // 1 / (n * 16)
    double nb[16], te[16];  // per acquisition: -b / 1000 and TE
    double Dm[3], Dd[3];
    float T2m[3], T2d[3];
    float slope;
    int fused;              // 1: the loss is formed here from x and pids
};

template <typename T>
__device__ __forceinline__ T group_sum16(T v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int Q, bool BWD>
__global__ void __launch_bounds__(256) pia_head_kernel(const PiaHead p) {
    constexpr int H = 256 * Q, E = 4 * Q;
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long nwaves = (long long)gridDim.x * 4;
    const long long per = (p.n + nwaves - 1) / nwaves;
    const long long r0 = wave * per, r1 = r0 + per < p.n ? r0 + per : p.n;
    const int a = lane & 15;

    float w[3][3][E], gw[BWD ? 3 : 1][3][BWD ? E : 1];
    float bo[3][3], gbo[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            bo[j][c] = p.b[j][c];
            gbo[j][c] = 0.f;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const f4u t = *reinterpret_cast<const f4u*>(p.W[j] + c * H + q * 256 + lane * 4);
                w[j][c][q * 4] = t.x; w[j][c][q * 4 + 1] = t.y; w[j][c][q * 4 + 2] = t.z; w[j][c][q * 4 + 3] = t.w;
            }
            if constexpr (BWD) {
#pragma unroll
                for (int e = 0; e < E; ++e) gw[j][c][e] = 0.f;
            }
        }
    const double nba = p.nb[a], tea = p.te[a];
    double loss_acc = 0.0;

    for (long long r = r0; r < r1; ++r) {
        float hv[3][E], o[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(p.h[j] + r * H + q * 256 + lane * 4);
                hv[j][q * 4] = t[0]; hv[j][q * 4 + 1] = t[1]; hv[j][q * 4 + 2] = t[2]; hv[j][q * 4 + 3] = t[3];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < E; ++e) s = fmaf(hv[j][e], w[j][c][e], s);
                o[j][c] = wave_sum(s) + bo[j][c];
            }
        }
        // encode (PIA.py:106-110)
        float th[2][3], T2[3], v[3];
        double D[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            th[0][c] = tanhf(o[0][c]);
            th[1][c] = tanhf(o[1][c]);
            D[c] = p.Dm[c] + p.Dd[c] * (double)th[0][c];
            T2[c] = p.T2m[c] + p.T2d[c] * th[1][c];
        }
        {
            const float mx = fmaxf(o[2][0], fmaxf(o[2][1], o[2][2]));
            const float e0 = expf(o[2][0] - mx), e1 = expf(o[2][1] - mx), e2 = expf(o[2][2] - mx);
            const float s = (e0 + e1) + e2;
            v[0] = e0 / s; v[1] = e1 / s; v[2] = e2 / s;
        }
        // decode (PIA.py:120-130): acquisition a of this row on lane a (the four 16-lane groups repeat it)
        double P[3], S = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            P[c] = exp(nba * D[c]) * (double)expf((float)(-tea) / T2[c]);
            S += (double)v[c] * P[c];
        }
        const float sig = 1000.f * (float)S;
        if (p.signal && lane < 16) p.signal[r * 16 + lane] = sig;
        if (p.D && lane < 3) {
            p.D[r * 3 + lane] = lane == 0 ? D[0] : lane == 1 ? D[1] : D[2];
            p.T2[r * 3 + lane] = lane == 0 ? T2[0] : lane == 1 ? T2[1] : T2[2];
            p.v[r * 3 + lane] = lane == 0 ? v[0] : lane == 1 ? v[1] : v[2];
        }
        if constexpr (BWD) {

        // d loss / d signal[a]
        double gs;
        if (p.fused) {
            const float d = sig - p.x[r * 16 + a];
            const float pw = p.pids ? p.pids[r * 16 + a] : 1.f;
            const float term = pw * (d * d);
            loss_acc += group_sum16((double)term);
            gs = 2.0 * (double)pw * (double)d * p.inv_count;
        } else {
            gs = p.g_signal ? (double)p.g_signal[r * 16 + a] : 0.0;
        }
        gs *= 1000.0;
        double gD[3], gT[3], gv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double t = gs * P[c];
            gv[c] = group_sum16(t);
            gD[c] = group_sum16(t * (double)v[c] * nba);
            gT[c] = group_sum16(t * (double)v[c] * tea / ((double)T2[c] * (double)T2[c]));
            if (p.g_D) gD[c] += p.g_D[r * 3 + c];
            if (p.g_T2) gT[c] += (double)p.g_T2[r * 3 + c];
            if (p.g_v) gv[c] += (double)p.g_v[r * 3 + c];
        }
        float go[3][3];
        const double vdot = gv[0] * (double)v[0] + gv[1] * (double)v[1] + gv[2] * (double)v[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            go[0][c] = (float)(gD[c] * p.Dd[c] * (1.0 - (double)th[0][c] * (double)th[0][c]));
            go[1][c] = (float)(gT[c] * (double)p.T2d[c] * (1.0 - (double)th[1][c] * (double)th[1][c]));
            go[2][c] = (float)((double)v[c] * (gv[c] - vdot));
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float dz[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                float t = go[j][0] * w[j][0][e];
                t = fmaf(go[j][1], w[j][1][e], t);
                t = fmaf(go[j][2], w[j][2][e], t);
                dz[e] = hv[j][e] > 0.f ? t : t * p.slope;
#pragma unroll
                for (int c = 0; c < 3; ++c) gw[j][c][e] = fmaf(go[j][c], hv[j][e], gw[j][c][e]);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) gbo[j][c] += go[j][c];
#pragma unroll
            for (int q = 0; q < Q; ++q)
                *reinterpret_cast<f32x4*>(p.dzh[j] + r * H + q * 256 + lane * 4) =
                    f32x4{dz[q * 4], dz[q * 4 + 1], dz[q * 4 + 2], dz[q * 4 + 3]};
        }
        }   // BWD
    }
    if constexpr (BWD) {
    // every wave writes its slab row (zeros when it owned no row): the reduction reads all of them
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float* s = p.slab[j] + wave * (3 * H + 3);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int q = 0; q < Q; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[c * H + q * 256 + lane * 4 + e] = gw[j][c][q * 4 + e];
            if (lane == c) s[3 * H + c] = c == 0 ? gbo[j][0] : c == 1 ? gbo[j][1] : gbo[j][2];
        }
    }
    if (lane == 0 && p.part_loss) p.part_loss[wave] = (float)loss_acc;
    }
}

// ---- detect_PIDS_slice (PIA.py:286-327), one thread per pixel ---------------------------------------------------------------------
// S [npix][4 (b)][4 (TE)] float64.  adc = -slope of the least-squares line through log(S[:, TE 0] + 1e-7) over b / 1000.
// Decay maps: entry (i, local) = (s[local + 1] - trunc(s[local]) >= 0): the reference writes the left neighbour into an
// integer array, which truncates it toward zero before the comparison (PIA.py:312-313).
__global__ void __launch_bounds__(256) pia_pids_kernel(float* __restrict__ adc1, float* __restrict__ adc2, float* __restrict__ bdec,
                                                       float* __restrict__ tedec, const double* __restrict__ S,
                                                       const double* __restrict__ bvals, long long npix) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    double s[4][4];
    for (int k = 0; k < 16; ++k) s[k / 4][k % 4] = S[i * 16 + k];
    double bm = 0.0, ym = 0.0, y[4];
    for (int k = 0; k < 4; ++k) {
        bm += bvals[k] / 1000.0;
        y[k] = log(s[k][0] + 1e-7);
        ym += y[k];
    }
    bm /= 4;
    ym /= 4;
    double num = 0.0, den = 0.0;
    for (int k = 0; k < 4; ++k) {
        const double db = bvals[k] / 1000.0 - bm;
        num += db * (y[k] - ym);
        den += db * db;
    }
    const double adc = -(num / den);
    adc1[i] = adc > 3.0 ? 1.f : 0.f;
    adc2[i] = adc < 0.0 ? 1.f : 0.f;
    for (int q = 0; q < 4; ++q)
        for (int l = 0; l < 3; ++l) {
            tedec[(i * 4 + q) * 3 + l] = (s[q][l + 1] - trunc(s[q][l]) >= 0.0) ? 1.f : 0.f;   // along TE at b index q
            bdec[(i * 4 + q) * 3 + l] = (s[l + 1][q] - trunc(s[l][q]) >= 0.0) ? 1.f : 0.f;    // along b at TE index q
        }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
struct PiaShape {
    int L;                 // encoder layers
    int in[8], out[8];
    int H;                 // head width
    int depth;
    long long w_off[8], b_off[8];          // encoder
    long long hw_off[3][4], hb_off[3][4];  // head hidden layers
    long long ow_off[3], ob_off[3];        // 3-wide output layers
    long long total;
    int ntensors;
};

int pia_shape(const inr_pia_desc_t* d, PiaShape& s, const char* who) {
    INR_REQUIRE(d != nullptr, INR_E_INVALID, "%s: null descriptor", who);
    INR_REQUIRE(d->n_signals >= 1 && d->n_hidden >= 1 && d->n_hidden <= INR_PIA_MAX_HIDDEN && d->predictor_depth >= 1 &&
                    d->predictor_depth <= 4 && d->n_b >= 1 && d->n_te >= 1 && d->n_b <= INR_PIA_MAX_TABLE &&
                    d->n_te <= INR_PIA_MAX_TABLE && d->n_b * d->n_te == d->n_signals,
                INR_E_INVALID, "%s: bad pia descriptor (n_signals %d, n_hidden %d, predictor_depth %d, n_b %d, n_te %d)", who,
                d->n_signals, d->n_hidden, d->predictor_depth, d->n_b, d->n_te);
    s.L = d->n_hidden;
    long long at = 0;
    int prev = d->n_signals;
    for (int l = 0; l < s.L; ++l) {
        INR_REQUIRE(d->hidden[l] >= 1, INR_E_INVALID, "%s: bad pia descriptor (hidden[%d] = %d)", who, l, d->hidden[l]);
        s.in[l] = prev;
        s.out[l] = d->hidden[l];
        s.w_off[l] = at;
        at += (long long)prev * d->hidden[l];
        s.b_off[l] = at;
        at += d->hidden[l];
        prev = d->hidden[l];
    }
    s.H = prev;
    s.depth = d->predictor_depth;
    for (int j = 0; j < 3; ++j) {
        for (int k = 0; k < s.depth; ++k) {
            s.hw_off[j][k] = at;
            at += (long long)s.H * s.H;
            s.hb_off[j][k] = at;
            at += s.H;
        }
        s.ow_off[j] = at;
        at += 3ll * s.H;
        s.ob_off[j] = at;
        at += 3;
    }
    s.total = at;
    s.ntensors = 2 * s.L + 3 * (2 * s.depth + 2);
    return 0;
}

// what the kernels serve (the parameter layout above is defined for every valid descriptor)
int pia_kernel_shape(const inr_pia_desc_t* d, PiaShape& s, const char* who) {
    if (int rc = pia_shape(d, s, who)) return rc;
    INR_REQUIRE(d->n_signals == 16, INR_E_INVALID, "%s: the kernels serve n_signals == 16 (got %d)", who, d->n_signals);
    INR_REQUIRE(s.depth == 1, INR_E_INVALID, "%s: the kernels serve predictor_depth == 1 (got %d)", who, s.depth);
    INR_REQUIRE(s.H == 256 || s.H == 512, INR_E_INVALID, "%s: the kernels serve a last hidden width of 256 or 512 (got %d)", who, s.H);
    for (int l = 0; l < s.L; ++l)
        INR_REQUIRE(s.out[l] % 16 == 0, INR_E_INVALID, "%s: hidden widths must be multiples of 16 (hidden[%d] = %d)", who, l, s.out[l]);
    for (int c = 0; c < 3; ++c)
        INR_REQUIRE(d->T2_mean[c] - fabs(d->T2_delta[c]) > 0.0, INR_E_INVALID, "%s: T2_mean - |T2_delta| must stay positive", who);
    return 0;
}

inline long long pia_head_waves(long long n) {
    long long w = (n + 3) / 4;
    if (w > 1024) w = 1024;
    return (w + 3) / 4 * 4;
}

// the forward-only row kernel writes no slabs, so nothing caps its grid
#ifndef PIA_FWD_ROWS_PER_WAVE
#define PIA_FWD_ROWS_PER_WAVE 16
#endif
inline long long pia_head_waves_fwd(long long n) {
    if (PIA_FWD_ROWS_PER_WAVE == 0) return pia_head_waves(n);
    const long long w = (n + PIA_FWD_ROWS_PER_WAVE - 1) / PIA_FWD_ROWS_PER_WAVE;
    return (w + 3) / 4 * 4;
}

// the training workspace: every activation, the gradient buffers and every slab of a step
struct PiaTrainWs {
    float* act[8];
    float* h[3];
    float* dzh[3];
    float* dz[2];
    float* enc_slab[8];
    int enc_splits[8];
    float* head_slab;      // [3][splits][H H + H]
    int head_splits;
    float* out_slab;       // [3][waves][3 H + 3]
    float* out_stage1;     // [3][ceil(waves / FIN_GROUP)][3 H + 3]
    float* part_loss;      // [waves]
    long long waves;
    size_t bytes;
};

void pia_train_ws(const PiaShape& s, long long n, void* base, PiaTrainWs& w) {
    WsCarver c(base, 256);
    int maxw = s.in[0];
    for (int l = 0; l < s.L; ++l) {
        w.act[l] = c.take<float>(n * s.out[l]);
        if (s.out[l] > maxw) maxw = s.out[l];
    }
    for (int j = 0; j < 3; ++j) w.h[j] = c.take<float>(n * s.H);
    for (int j = 0; j < 3; ++j) w.dzh[j] = c.take<float>(n * s.H);
    for (int k = 0; k < 2; ++k) w.dz[k] = c.take<float>(n * maxw);
    for (int l = 0; l < s.L; ++l) {
        w.enc_splits[l] = pia_dw_splits(n, s.out[l], s.in[l], 1);
        w.enc_slab[l] = c.take<float>((long long)w.enc_splits[l] * ((long long)s.out[l] * s.in[l] + s.out[l]));
    }
    w.head_splits = pia_dw_splits(n, s.H, s.H, 3);
    w.head_slab = c.take<float>(3ll * w.head_splits * ((long long)s.H * s.H + s.H));
    w.waves = pia_head_waves(n);
    w.out_slab = c.take<float>(3 * w.waves * (3ll * s.H + 3));
    w.out_stage1 = c.take<float>(3 * ((w.waves + FIN_GROUP - 1) / FIN_GROUP) * (3ll * s.H + 3));
    w.part_loss = c.take<float>(w.waves);
    w.bytes = c.bytes();
}

// the forward-only workspace of one chunk: two ping-pong encoder buffers and the three head hidden activations
struct PiaFwdWs { float *pp[2], *h[3]; size_t bytes; };
PiaFwdWs pia_fwd_ws(const PiaShape& s, long long rows, void* base) {
    PiaFwdWs w;
    int maxw = 0;
    for (int l = 0; l < s.L; ++l) maxw = s.out[l] > maxw ? s.out[l] : maxw;
    WsCarver c(base, 256);
    for (int k = 0; k < 2; ++k) w.pp[k] = c.take<float>(rows * maxw);
    for (int j = 0; j < 3; ++j) w.h[j] = c.take<float>(rows * s.H);
    w.bytes = c.bytes();
    return w;
}

void pia_head_tables(const inr_pia_desc_t* d, PiaHead& a) {
    for (int i = 0; i < 16; ++i) {
        a.nb[i] = -d->b_values[i / d->n_te] / 1000.0;   // the Python scalar -b/1000 of PIA.py:125
        a.te[i] = d->te_values[i % d->n_te];
    }
    for (int c = 0; c < 3; ++c) {
        a.Dm[c] = d->D_mean[c];
        a.Dd[c] = d->D_delta[c];
        a.T2m[c] = (float)d->T2_mean[c];
        a.T2d[c] = (float)d->T2_delta[c];
    }
    a.slope = d->leaky_slope;
}

template <bool BWD>
int pia_launch_head(const PiaHead& a, int H, long long waves, hipStream_t st) {
    const dim3 grid((unsigned)(waves / 4));
    if (H == 512)
        hipLaunchKernelGGL((pia_head_kernel<2, BWD>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((pia_head_kernel<1, BWD>), grid, dim3(256), 0, st, a);
    INR_LAUNCH_CHECK();
    count_launch(LF_PIA_BASE + INR_PIA_LF_HEAD);
    return 0;
}

// encoder + head hidden layers of rows [0, n): act[l] and h[j] receive the activations
int pia_forward_layers(const PiaShape& s, const inr_pia_desc_t* d, const float* params, const float* x, long long n,
                       float* const* act, float* const* h, hipStream_t st) {
    ProfScope ps(KC_GEMM_FWD, st);
    const float* in = x;
    for (int l = 0; l < s.L; ++l) {
        PiaGemm g{};
        g.A[0] = in;
        g.B[0] = params + s.w_off[l];
        g.C[0] = act[l];
        g.bias[0] = params + s.b_off[l];
        g.M = n; g.N = s.out[l]; g.K = s.in[l];
        g.lda = s.in[l]; g.ldb = s.in[l]; g.ldc = s.out[l];
        g.nseg = 1; g.splits = 1; g.slope = d->leaky_slope;
        if (int rc = pia_launch_gemm<true, true, PIA_FWD>(g, 1, pia_big(g.M, g.N, 1), st)) return rc;
        in = act[l];
    }
    PiaGemm g{};
    for (int j = 0; j < 3; ++j) {
        g.A[j] = in;
        g.B[j] = params + s.hw_off[j][0];
        g.C[j] = h[j];
        g.bias[j] = params + s.hb_off[j][0];
    }
    g.M = n; g.N = s.H; g.K = s.H;
    g.lda = s.H; g.ldb = s.H; g.ldc = s.H;
    g.nseg = 1; g.splits = 1; g.slope = d->leaky_slope;
    return pia_launch_gemm<true, true, PIA_FWD>(g, 3, pia_big(g.M, g.N, 3), st);
}

// backward of everything below the row kernel (which has left dzh and the 3-wide layers' slabs) + the reduction (+ Adam)
int pia_backward_layers(const PiaShape& s, const inr_pia_desc_t* d, const float* params, float* adam_params, float* grads, float* m, float* v, const float* x,
                        long long n, const PiaTrainWs& w, bool with_loss, float* loss_out, long long step, double lr, double b1,
                        double b2, double eps, hipStream_t st) {
    const float slope = d->leaky_slope;
    const int top = s.L - 1;
    {   // head hidden layers: gW_j = dzh_j^T act_top, gb_j = colsum(dzh_j)
        ProfScope ps(KC_GEMM_DW, st);
        const long long len = (long long)s.H * s.H + s.H;
        PiaGemm g{};
        for (int j = 0; j < 3; ++j) {
            g.A[j] = w.dzh[j];
            g.B[j] = w.act[top];
            g.C[j] = w.head_slab + (long long)j * w.head_splits * len;
            g.colsum[j] = g.C[j] + (long long)s.H * s.H;
        }
        g.M = s.H; g.N = s.H; g.K = n;
        g.lda = s.H; g.ldb = s.H; g.ldc = s.H;
        g.nseg = 1; g.splits = w.head_splits; g.slab_stride = len; g.slope = slope;
        if (int rc = pia_launch_gemm<false, false, PIA_DW>(g, 3, s.H >= 128 && n >= 4096, st)) return rc;
    }
    {   // dz_top = (sum_j dzh_j W_j) * leaky'(act_top)
        ProfScope ps(KC_GEMM_DX, st);
        PiaGemm g{};
        for (int j = 0; j < 3; ++j) {
            g.A[j] = w.dzh[j];
            g.B[j] = params + s.hw_off[j][0];
        }
        g.C[0] = w.dz[0];
        g.act[0] = w.act[top];
        g.M = n; g.N = s.H; g.K = s.H;
        g.lda = s.H; g.ldb = s.H; g.ldc = s.H;
        g.nseg = 3; g.splits = 1; g.slope = slope;
        if (int rc = pia_launch_gemm<true, false, PIA_DX>(g, 1, pia_big(g.M, g.N, 1), st)) return rc;
    }
    int cur = 0;
    for (int l = top; l >= 0; --l) {
        {
            ProfScope ps(KC_GEMM_DW, st);
            const long long len = (long long)s.out[l] * s.in[l] + s.out[l];
            PiaGemm g{};
            g.A[0] = w.dz[cur];
            g.B[0] = l > 0 ? w.act[l - 1] : x;
            g.C[0] = w.enc_slab[l];
            g.colsum[0] = w.enc_slab[l] + (long long)s.out[l] * s.in[l];
            g.M = s.out[l]; g.N = s.in[l]; g.K = n;
            g.lda = s.out[l]; g.ldb = s.in[l]; g.ldc = s.in[l];
            g.nseg = 1; g.splits = w.enc_splits[l]; g.slab_stride = len; g.slope = slope;
            if (int rc = pia_launch_gemm<false, false, PIA_DW>(g, 1, s.out[l] >= 128 && s.in[l] >= 128 && n >= 4096, st)) return rc;
        }
        if (l > 0) {
            ProfScope ps(KC_GEMM_DX, st);
            PiaGemm g{};
            g.A[0] = w.dz[cur];
            g.B[0] = params + s.w_off[l];
            g.C[0] = w.dz[cur ^ 1];
            g.act[0] = w.act[l - 1];
            g.M = n; g.N = s.in[l]; g.K = s.out[l];
            g.lda = s.out[l]; g.ldb = s.in[l]; g.ldc = s.in[l];
            g.nseg = 1; g.splits = 1; g.slope = slope;
            if (int rc = pia_launch_gemm<true, false, PIA_DX>(g, 1, pia_big(g.M, g.N, 1), st)) return rc;
            cur ^= 1;
        }
    }
    // one launch sums every slab stack in a fixed order, finishes the loss and (fit step) applies Adam
    FinalizeJob job{};
    int k = 0;
    for (int l = 0; l < s.L; ++l, ++k) {
        job.seg[k].slab = w.enc_slab[l];
        job.seg[k].stage1 = nullptr;
        job.seg[k].dst = s.w_off[l];
        job.seg[k].len = (long long)s.out[l] * s.in[l] + s.out[l];
        job.seg[k].nslabs = w.enc_splits[l];
    }
    for (int j = 0; j < 3; ++j) {
        const long long len = (long long)s.H * s.H + s.H;
        job.seg[k].slab = w.head_slab + (long long)j * w.head_splits * len;
        job.seg[k].stage1 = nullptr;
        job.seg[k].dst = s.hw_off[j][0];
        job.seg[k].len = len;
        job.seg[k].nslabs = w.head_splits;
        ++k;
        const long long olen = 3ll * s.H + 3;
        job.seg[k].slab = w.out_slab + (long long)j * w.waves * olen;
        job.seg[k].stage1 = w.out_stage1 + (long long)j * ((w.waves + FIN_GROUP - 1) / FIN_GROUP) * olen;
        job.seg[k].dst = s.ow_off[j];
        job.seg[k].len = olen;
        job.seg[k].nslabs = (int)w.waves;
        ++k;
    }
    job.nseg = k;
    job.part_loss = with_loss ? w.part_loss : nullptr;
    job.nparts = (int)w.waves;
    job.loss_scale = (float)(1.0 / ((double)n * 16.0));
    job.loss_out = loss_out;
    job.grads = grads;
    job.params = adam_params;
    job.m = m;
    job.v = v;
    return launch_finalize(job, step, lr, b1, b2, eps, st);
}

int pia_train_head_args(PiaHead& a, const PiaShape& s, const inr_pia_desc_t* d, const float* params, const PiaTrainWs& w, long long n) {
    pia_head_tables(d, a);
    for (int j = 0; j < 3; ++j) {
        a.h[j] = w.h[j];
        a.W[j] = params + s.ow_off[j];
        a.b[j] = params + s.ob_off[j];
        a.dzh[j] = w.dzh[j];
        a.slab[j] = w.out_slab + (long long)j * w.waves * (3ll * s.H + 3);
    }
    a.part_loss = w.part_loss;
    a.n = n;
    a.inv_count = 1.0 / ((double)n * 16.0);
    return 0;
}

}  // namespace

}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_pia_param_count(const inr_pia_desc_t* desc) {
    PiaShape s;
    if (pia_shape(desc, s, "inr_pia_param_count")) return -1;
    return s.total;
}

int inr_pia_param_offsets(const inr_pia_desc_t* desc, int64_t* offsets, int max_tensors) {
    PiaShape s;
    if (int rc = pia_shape(desc, s, "inr_pia_param_offsets")) return rc;
    INR_REQUIRE(offsets != nullptr && max_tensors >= s.ntensors, INR_E_INVALID, "inr_pia_param_offsets: need room for %d offsets",
                s.ntensors);
    int k = 0;
    for (int l = 0; l < s.L; ++l) {
        offsets[k++] = s.w_off[l];
        offsets[k++] = s.b_off[l];
    }
    for (int j = 0; j < 3; ++j) {
        for (int q = 0; q < s.depth; ++q) {
            offsets[k++] = s.hw_off[j][q];
            offsets[k++] = s.hb_off[j][q];
        }
        offsets[k++] = s.ow_off[j];
        offsets[k++] = s.ob_off[j];
    }
    return 0;
}

size_t inr_pia_workspace_bytes(const inr_pia_desc_t* desc, int64_t n, int training) {
    PiaShape s;
    if (pia_kernel_shape(desc, s, "inr_pia_workspace_bytes") || n < 1) return 0;
    if (training) {
        PiaTrainWs w;
        pia_train_ws(s, n, nullptr, w);
        return w.bytes;
    }
    return pia_fwd_ws(s, n, nullptr).bytes;
}

int inr_pia_forward(const inr_pia_desc_t* desc, const float* params, const float* x, int64_t n, float* signal, double* D, float* T2,
                    float* v, int64_t chunk_rows, void* workspace, size_t workspace_bytes, void* stream) {
    PiaShape s;
    if (int rc = pia_kernel_shape(desc, s, "inr_pia_forward")) return rc;
    INR_REQUIRE(params && x && n >= 1 && chunk_rows >= 1, INR_E_INVALID, "inr_pia_forward: null pointer or non-positive size");
    INR_REQUIRE((signal || D) && (!D || (T2 && v)), INR_E_INVALID, "inr_pia_forward: no output (D, T2 and v come together)");
    INR_REQUIRE(aligned16(x), INR_E_ALIGN, "inr_pia_forward: x must be 16-byte aligned");
    if (chunk_rows > n) chunk_rows = n;
    const PiaFwdWs w = pia_fwd_ws(s, chunk_rows, workspace);
    INR_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= w.bytes, INR_E_WORKSPACE,
                "inr_pia_forward: workspace too small for chunks of %lld rows", (long long)chunk_rows);
    hipStream_t st = (hipStream_t)stream;
    float* const* h = w.h;
    float* act[8];
    for (int l = 0; l < s.L; ++l) act[l] = w.pp[l & 1];
    PiaHead a{};
    pia_head_tables(desc, a);
    for (int j = 0; j < 3; ++j) {
        a.h[j] = h[j];
        a.W[j] = params + s.ow_off[j];
        a.b[j] = params + s.ob_off[j];
    }
    for (int64_t r = 0; r < n; r += chunk_rows) {
        const long long rows = n - r < chunk_rows ? n - r : chunk_rows;
        if (int rc = pia_forward_layers(s, desc, params, x + r * 16, rows, act, h, st)) return rc;
        a.signal = signal ? signal + r * 16 : nullptr;
        a.D = D ? D + r * 3 : nullptr;
        a.T2 = T2 ? T2 + r * 3 : nullptr;
        a.v = v ? v + r * 3 : nullptr;
        a.n = rows;
        ProfScope ps(KC_OTHER, st);
        if (int rc = pia_launch_head<false>(a, s.H, pia_head_waves_fwd(rows), st)) return rc;
    }
    return 0;
}

int inr_pia_forward_train(const inr_pia_desc_t* desc, const float* params, const float* x, int64_t n, float* signal, double* D,
                          float* T2, float* v, void* workspace, size_t workspace_bytes, void* stream) {
    PiaShape s;
    if (int rc = pia_kernel_shape(desc, s, "inr_pia_forward_train")) return rc;
    INR_REQUIRE(params && x && signal && D && T2 && v && n >= 1, INR_E_INVALID, "inr_pia_forward_train: null pointer or non-positive size");
    INR_REQUIRE(aligned16(x), INR_E_ALIGN, "inr_pia_forward_train: x must be 16-byte aligned");
    PiaTrainWs w;
    pia_train_ws(s, n, workspace, w);
    INR_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= w.bytes, INR_E_WORKSPACE,
                "inr_pia_forward_train: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pia_forward_layers(s, desc, params, x, n, w.act, w.h, st)) return rc;
    PiaHead a{};
    pia_train_head_args(a, s, desc, params, w, n);
    a.signal = signal; a.D = D; a.T2 = T2; a.v = v;
    ProfScope ps(KC_OTHER, st);
    return pia_launch_head<false>(a, s.H, w.waves, st);
}

int inr_pia_backward_train(const inr_pia_desc_t* desc, const float* params, float* grads, const float* x, const float* g_signal,
                           const double* g_D, const float* g_T2, const float* g_v, int64_t n, void* workspace,
                           size_t workspace_bytes, void* stream) {
    PiaShape s;
    if (int rc = pia_kernel_shape(desc, s, "inr_pia_backward_train")) return rc;
    INR_REQUIRE(params && grads && x && n >= 1, INR_E_INVALID, "inr_pia_backward_train: null pointer or non-positive size");
    INR_REQUIRE(aligned16(x), INR_E_ALIGN, "inr_pia_backward_train: x must be 16-byte aligned");
    PiaTrainWs w;
    pia_train_ws(s, n, workspace, w);
    INR_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= w.bytes, INR_E_WORKSPACE,
                "inr_pia_backward_train: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    PiaHead a{};
    pia_train_head_args(a, s, desc, params, w, n);
    a.g_signal = g_signal; a.g_D = g_D; a.g_T2 = g_T2; a.g_v = g_v;
    a.part_loss = nullptr;
    {
        ProfScope ps(KC_OTHER, st);
        if (int rc = pia_launch_head<true>(a, s.H, w.waves, st)) return rc;
    }
    return pia_backward_layers(s, desc, params, nullptr, grads, nullptr, nullptr, x, n, w, false, nullptr, 1, 0.0, 0.0, 0.0, 0.0, st);
}

int inr_pia_fit_step(const inr_pia_desc_t* desc, float* params, float* grads, float* m, float* v, const float* x, const float* pids,
                     int64_t n, int64_t step, double lr, double beta1, double beta2, double eps, float* loss, void* workspace,
                     size_t workspace_bytes, void* stream) {
    PiaShape s;
    if (int rc = pia_kernel_shape(desc, s, "inr_pia_fit_step")) return rc;
    INR_REQUIRE(params && grads && m && v && x && loss && n >= 1 && step >= 1, INR_E_INVALID,
                "inr_pia_fit_step: null pointer or non-positive size / step");
    INR_REQUIRE(aligned16(x), INR_E_ALIGN, "inr_pia_fit_step: x must be 16-byte aligned");
    PiaTrainWs w;
    pia_train_ws(s, n, workspace, w);
    INR_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= w.bytes, INR_E_WORKSPACE,
                "inr_pia_fit_step: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pia_forward_layers(s, desc, params, x, n, w.act, w.h, st)) return rc;
    PiaHead a{};
    pia_train_head_args(a, s, desc, params, w, n);
    a.x = x; a.pids = pids; a.fused = 1;
    {
        ProfScope ps(KC_OTHER, st);
        if (int rc = pia_launch_head<true>(a, s.H, w.waves, st)) return rc;
    }
    return pia_backward_layers(s, desc, params, params, grads, m, v, x, n, w, true, loss, step, lr, beta1, beta2, eps, st);
}

int inr_pids_slice(float* adc_high, float* adc_negative, float* b_decay, float* te_decay, const double* S, const double* bvals,
                   int64_t n_pixels, void* stream) {
    INR_REQUIRE(adc_high && adc_negative && b_decay && te_decay && S && bvals && n_pixels >= 1, INR_E_INVALID,
                "inr_pids_slice: null pointer or non-positive size");
    hipLaunchKernelGGL(pia_pids_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, adc_high,
                       adc_negative, b_decay, te_decay, S, bvals, (long long)n_pixels);
    INR_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
