// The soft-ERD INR family (INR_ERD.py:28-67 `Siren`; its two training loops INR_ERD.py:198-217 and 252-273; the soft-ERD
// weights INR_ERD.py:143-158, 225-235).  The network is a SIREN trunk closed by Linear + ReLU, a ReLU head, and an in-module
// coordinate perturbation p = eps tanh(W2 tanh(W1 [x, sample] + b1) + b2) that is added to EVERY coordinate component.
//   erd_step_kernel    -- in the style of siren_small_step_kernel: a wave owns 32 rows and carries them through the whole
//       network (perturbation prologue on the VALU, sine layers, ReLU layer, ReLU head, weighted loss partial, running max of
//       the outputs; backward through the head and ReLU masks, the sine layers, the layer-0 INPUT gradient dz0 W0 -- summed over
//       the components it is dL/dp -- and on through eps tanh and the two perturb layers).  Per-wave gradient slabs.
//   erd_reduce_kernel  -- fixed-order slab sum, loss, Adam with two parameter groups (trunk + head | perturb branch) in the
//       arithmetic of adam_kernel, and the device-resident status block {state, steps_done, last_loss, y_max}.
//   Both kernels read a gate word at entry and return unless it says RUNNING; the reduce kernel of step i reads gate[i & 1] and
//   its block 0 writes gate[(i + 1) & 1], so no block of a launch ever reads a word that a block of the same launch writes.
//   No cooperative launch, no cross-block atomics, no host read per step.
// LDS at H = 128: a 67.6 KB weight image + 2 waves x 2 stages x 16.9 KB = 135 KB of the CU's 160 KiB (one block per CU, one
// wave on each of two SIMDs); weights go global -> LDS directly (a register prefetch of a 128 x 128 matrix would be 128 VGPRs).
#include "internal.h"

#include <math.h>

namespace inr {

namespace {

constexpr int ERD_MAX_F = 8;
constexpr int ERD_MAX_HIDDEN_LAYERS = 8;
constexpr int ERD_MAX_TRUNK = ERD_MAX_HIDDEN_LAYERS + 2;   // sine layers + the ReLU layer
constexpr int ERD_TENSORS = ERD_MAX_TRUNK + 3;            // + head, perturb_linear, perturb_linear2
constexpr int ERD_WAVES = 2;
constexpr int ERD_THREADS = ERD_WAVES * 64;
constexpr int ERD_ROWS = ERD_WAVES * 32;

struct ErdLayout {
    long long w_off[ERD_TENSORS], b_off[ERD_TENSORS];
    long long group_b, P;
    int T;   // trunk layers: 1 + hidden_layers sine layers and the ReLU layer; tensor T = head, T + 1 / T + 2 = perturb layers
};

struct ErdStep {
    const float* params;
    float* slabs;          // [nwaves][P]
    float* loss_partial;   // [nwaves]
    float* ymax_partial;   // [nwaves]
    float* acts;           // [T - 1][N][H]: acts[l - 1] = input of trunk layer l
    float* dacts;          // [T - 1][N][H]: dacts[l] = d a_{l+1} / d z_l (omega cos, or the ReLU mask as 0 / 1)
    const float* x;        // [N][F]
    const float* target;   // [N]
    const float* weight;   // [N] or null
    float* y_out;          // [N] or null
    const int* gate;       // null = run
    ErdLayout L;
    int N, F, S;           // rows, in_features, sine layers
    float first_omega, hidden_omega, inv_count, sample, eps;
    int perturb, accumulate;
};

// u_j = tanh(b1[j] + W1[j] . [x, sample]) -- the same instruction sequence in the forward prologue and in the backward pass
__device__ __forceinline__ float erd_perturb_unit(const float* W1, const float* b1, const float* in, int F, int j) {
    float pre = b1[j];
#pragma unroll
    for (int c = 0; c <= ERD_MAX_F; ++c)
        if (c <= F) pre = fmaf(W1[j * (F + 1) + c], in[c], pre);
    return tanhf(pre);
}

template <int H, bool TRAIN>
__global__ void __launch_bounds__(ERD_THREADS) erd_step_kernel(const ErdStep p) {
    constexpr int CT = H / 32;
    constexpr int LDS_STRIDE = H + 4;
    __shared__ __attribute__((aligned(16))) float ldsW[H * LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) float stage[ERD_WAVES][TRAIN ? 2 : 1][32 * LDS_STRIDE];
    __shared__ float xs[ERD_WAVES][32][ERD_MAX_F];    // the perturbed coordinates x + p (layer 0's input)
    __shared__ float xr[ERD_WAVES][32][ERD_MAX_F + 1];   // [x, sample]: the perturb branch's input (zero rows beyond N)
    __shared__ float gbuf[ERD_WAVES][32];

    if (p.gate && *p.gate != INR_ERD_RUNNING) return;     // uniform over the grid: an earlier launch of this stream stored it

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, l32 = lane & 31;
    const int gwave = blockIdx.x * ERD_WAVES + wave;
    const int r0 = gwave * 32;
    const int T = p.L.T, F = p.F;
    float* stageA = stage[wave][0];
    float* stageD = stage[wave][TRAIN ? 1 : 0];
    float* slab = p.slabs + (long long)gwave * p.L.P;
    const long long NH = (long long)p.N * H;
    const int row = r0 + l32;
    const bool rvalid = row < p.N;
    const bool accumulate = p.accumulate != 0;
    auto put = [&](long long idx, float v) { slab[idx] = accumulate ? slab[idx] + v : v; };

    auto load_weights = [&](int l) {   // W_l [H][H] -> ldsW [H][H + 4], the whole block
        const f32x4* W = reinterpret_cast<const f32x4*>(p.params + p.L.w_off[l]);
        __syncthreads();
#pragma unroll 8
        for (int i = 0; i < (H * H / 4) / ERD_THREADS; ++i) {
            const int f = tid + ERD_THREADS * i;
            *reinterpret_cast<f32x4*>(ldsW + (f / (H / 4)) * LDS_STRIDE + (f % (H / 4)) * 4) = W[f];
        }
        __syncthreads();
    };

    // ---- perturbation prologue (INR_ERD.py:56-63): lane = (row, half of the hidden units) --------------------------------
    const float* W1 = p.params + p.L.w_off[T + 1];
    const float* b1 = p.params + p.L.b_off[T + 1];
    const float* W2 = p.params + p.L.w_off[T + 2];
    float in[ERD_MAX_F + 1];
#pragma unroll
    for (int c = 0; c < ERD_MAX_F; ++c) in[c] = (c < F && rvalid) ? p.x[(long long)row * F + c] : 0.f;
#pragma unroll
    for (int c = 0; c <= ERD_MAX_F; ++c)
        if (c == F) in[c] = p.sample;
    float t2 = 0.f, pv = 0.f;
    if (p.perturb) {
        float part = 0.f;
        for (int q = 0; q < H / 2; ++q) {
            const int j = hh * (H / 2) + q;
            part = fmaf(erd_perturb_unit(W1, b1, in, F, j), W2[j], part);
        }
        t2 = tanhf(part + __shfl_xor(part, 32, 64) + p.params[p.L.b_off[T + 2]]);
        pv = p.eps * t2;
    }
    if (hh == 0) {
#pragma unroll
        for (int c = 0; c < ERD_MAX_F; ++c) {
            xs[wave][l32][c] = (c < F) ? in[c] + pv : 0.f;      // p is added to every component
            xr[wave][l32][c] = in[c];
        }
        xr[wave][l32][ERD_MAX_F] = 0.f;
#pragma unroll
        for (int c = 0; c <= ERD_MAX_F; ++c)
            if (c == F) xr[wave][l32][c] = p.sample;
    }

    // ------------------------------------------------ forward ------------------------------------------------
    f32x16 acc[CT], dlast[CT];
    {   // layer 0: z0 = (x + p) W0^T, K = F (k = 2 kp + hh, zero beyond F)
        const float* W0 = p.params + p.L.w_off[0];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
        for (int kp = 0; kp < (F + 1) / 2; ++kp) {
            const int k = 2 * kp + hh;
            const float a = (k < F) ? xs[wave][l32][k] : 0.f;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const float b = (k < F) ? W0[(ct * 32 + l32) * F + k] : 0.f;
                acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[ct], 0, 0, 0);
            }
        }
    }
    for (int l = 0; l < T; ++l) {
        if (l > 0) {
            load_weights(l);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
#pragma unroll 4
            for (int kb = 0; kb < H / 8; ++kb) {
                const f32x4 fa = *reinterpret_cast<const f32x4*>(stageA + l32 * LDS_STRIDE + 8 * kb + 4 * hh);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const f32x4 fb = *reinterpret_cast<const f32x4*>(ldsW + (ct * 32 + l32) * LDS_STRIDE + 8 * kb + 4 * hh);
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s], fb[s], acc[ct], 0, 0, 0);
                }
            }
        }
        // epilogue: sine layers a = sin(omega z), d = omega cos(omega z); the last trunk layer a = max(z, 0), d = [z > 0]
        const bool sine = l < p.S;
        const float omega = (l == 0) ? p.first_omega : p.hidden_omega;
        const float* bias = p.params + p.L.b_off[l];
        const bool stash = TRAIN && l + 1 < T;
        float* a_out = p.acts + (long long)l * NH;          // acts[(l + 1) - 1]
        float* d_out = p.dacts + (long long)l * NH;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int j = ct * 32 + l32;
            const float bj = bias[j];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = mfma32_acc_row(r, hh);
                const float z = acc[ct][r] + bj;
                float av, dv;
                if (sine) {
                    float sv, cv;
                    sincos_f32_ool(omega * z, sv, cv);
                    av = sv;
                    dv = omega * cv;
                } else {
                    av = z > 0.f ? z : 0.f;
                    dv = z > 0.f ? 1.f : 0.f;
                }
                stageA[i * LDS_STRIDE + j] = av;
                dlast[ct][r] = dv;
                if (stash && r0 + i < p.N) {
                    a_out[(long long)(r0 + i) * H + j] = av;
                    d_out[(long long)(r0 + i) * H + j] = dv;
                }
            }
        }
    }
    // head (INR_ERD.py:65-66): y = max(a_T . w + b, 0)
    const float* wh = p.params + p.L.w_off[T];
    float part = 0.f;
#pragma unroll
    for (int q = 0; q < H / 8; ++q) {
        const int j0 = hh * (H / 2) + 4 * q;
        const f32x4 av = *reinterpret_cast<const f32x4*>(stageA + l32 * LDS_STRIDE + j0);
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wh + j0);
        part = fmaf(av[0], wv[0], part);
        part = fmaf(av[1], wv[1], part);
        part = fmaf(av[2], wv[2], part);
        part = fmaf(av[3], wv[3], part);
    }
    const float ypre = part + __shfl_xor(part, 32, 64) + p.params[p.L.b_off[T]];
    const float y = ypre > 0.f ? ypre : 0.f;
    if (p.y_out && rvalid && hh == 0) p.y_out[row] = y;
    if (!TRAIN) return;

    const float resid = rvalid ? y - p.target[row] : 0.f;
    const float wr = (p.weight && rvalid) ? p.weight[row] * resid : resid;
    const float g = (ypre > 0.f) ? 2.0f * wr * p.inv_count : 0.f;      // dL/d(head pre-activation)
    if (hh == 0) gbuf[wave][l32] = g;
    float lsum = (hh == 0) ? wr * resid : 0.f;
    float gsum = (hh == 0) ? g : 0.f;
    float ymax = rvalid ? y : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lsum += __shfl_xor(lsum, off, 64);
        gsum += __shfl_xor(gsum, off, 64);
        ymax = fmaxf(ymax, __shfl_xor(ymax, off, 64));
    }
    if (lane == 0) {
        p.loss_partial[gwave] = accumulate ? p.loss_partial[gwave] + lsum : lsum;
        p.ymax_partial[gwave] = accumulate ? fmaxf(p.ymax_partial[gwave], ymax) : ymax;
        put(p.L.b_off[T], gsum);
    } else if (lane < 4) {
        if (!accumulate) {
            slab[p.L.b_off[T] + lane] = 0.f;            // 16-byte padding of the two 1-float biases
            slab[p.L.b_off[T + 2] + lane] = 0.f;
        }
    }

    // ------------------------------------------------ backward -----------------------------------------------
    f32x16 dz[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int j = ct * 32 + l32;
        const float wj = wh[j];
        float gw = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = mfma32_acc_row(r, hh);
            const float gi = gbuf[wave][i];
            gw = fmaf(gi, stageA[i * LDS_STRIDE + j], gw);
            dz[ct][r] = gi * wj * dlast[ct][r];
        }
        gw += __shfl_xor(gw, 32, 64);
        if (hh == 0) put(p.L.w_off[T] + j, gw);
    }

    // (ldsW still holds W_{T-1}: the first backward layer needs no reload)
    for (int l = T - 1; l >= 0; --l) {
        const int K = (l == 0) ? F : H;
        f32x4 a_pref[(32 * H / 4) / 64];
        f32x16 d_pref[CT];
        if (l > 0) {
            const float* a_in = p.acts + (long long)(l - 1) * NH;
#pragma unroll
            for (int it = 0; it < (32 * H / 4) / 64; ++it) {
                const int f = it * 64 + lane, rr = f / (H / 4), c4 = (f % (H / 4)) * 4;
                a_pref[it] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (r0 + rr < p.N) a_pref[it] = *reinterpret_cast<const f32x4*>(a_in + (long long)(r0 + rr) * H + c4);
            }
            const float* d_in = p.dacts + (long long)(l - 1) * NH;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = mfma32_acc_row(r, hh);
                    d_pref[ct][r] = (r0 + i < p.N) ? d_in[(long long)(r0 + i) * H + ct * 32 + l32] : 0.f;
                }
        }
        // bias gradient + dz into its operand image
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int j = ct * 32 + l32;
            float gb = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                gb += dz[ct][r];
                stageD[mfma32_acc_row(r, hh) * LDS_STRIDE + j] = dz[ct][r];
            }
            gb += __shfl_xor(gb, 32, 64);
            if (hh == 0) put(p.L.b_off[l] + j, gb);
        }
        if (l > 0) {   // da_l = dz_l W_l, then dz_{l-1} = da_l * d_{l-1}
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
#pragma unroll 4
            for (int kb = 0; kb < H / 8; ++kb) {
                const f32x4 fa = *reinterpret_cast<const f32x4*>(stageD + l32 * LDS_STRIDE + 8 * kb + 4 * hh);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float* wrow = ldsW + (8 * kb + 4 * hh + s) * LDS_STRIDE + l32;
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct)
                        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s], wrow[ct * 32], acc[ct], 0, 0, 0);
                }
            }
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) dz[ct][r] = acc[ct][r] * d_pref[ct][r];
#pragma unroll
            for (int it = 0; it < (32 * H / 4) / 64; ++it) {
                const int f = it * 64 + lane, rr = f / (H / 4), c4 = (f % (H / 4)) * 4;
                *reinterpret_cast<f32x4*>(stageA + rr * LDS_STRIDE + c4) = a_pref[it];
            }
        }
        // weight gradient: gW_l[j][k] = sum_rows dz_l[row][j] * a_l[row][k]   (a_0 = x + p)
        const int KT = (K + 31) / 32;
        for (int ht = 0; ht < CT; ++ht) {
            for (int kt = 0; kt < KT; ++kt) {
                f32x16 wacc;
#pragma unroll
                for (int r = 0; r < 16; ++r) wacc[r] = 0.f;
                const int kc = kt * 32 + l32;
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int rr = 8 * kb + 4 * hh + s;
                        const float a = stageD[rr * LDS_STRIDE + ht * 32 + l32];
                        float b;
                        if (l > 0)
                            b = stageA[rr * LDS_STRIDE + kc];
                        else
                            b = (kc < F) ? xs[wave][rr][kc & (ERD_MAX_F - 1)] : 0.f;
                        wacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, wacc, 0, 0, 0);
                    }
                }
                if (kc < K) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) put(p.L.w_off[l] + (long long)(ht * 32 + mfma32_acc_row(r, hh)) * K + kc, wacc[r]);
                }
            }
        }
        if (l > 1) load_weights(l - 1);
    }

    // ---- perturbation branch: dL/dp = sum_k (dz0 W0)[row][k], through eps tanh and the two perturb layers ---------------------
    const long long pb0 = p.L.group_b, pbn = p.L.P - p.L.group_b;
    if (!p.perturb) {
        if (!accumulate)
            for (long long i = lane; i < pbn; i += 64) slab[pb0 + i] = 0.f;
        return;
    }
    {
        const float* W0 = p.params + p.L.w_off[0];
        float dx[ERD_MAX_F];
#pragma unroll
        for (int k = 0; k < ERD_MAX_F; ++k) dx[k] = 0.f;
        for (int q = 0; q < H / 2; ++q) {
            const int j = hh * (H / 2) + q;
            const float d0 = stageD[l32 * LDS_STRIDE + j];
#pragma unroll
            for (int k = 0; k < ERD_MAX_F; ++k)
                if (k < F) dx[k] = fmaf(d0, W0[j * F + k], dx[k]);
        }
        float dp = 0.f;
#pragma unroll
        for (int k = 0; k < ERD_MAX_F; ++k)
            if (k < F) dp += dx[k];
        dp += __shfl_xor(dp, 32, 64);
        const float dq = dp * p.eps * (1.f - t2 * t2);
        if (hh == 0) gbuf[wave][l32] = dq;
        for (int q = 0; q < H / 2; ++q) {
            const int j = hh * (H / 2) + q;
            const float u = erd_perturb_unit(W1, b1, in, F, j);
            stageA[l32 * LDS_STRIDE + j] = dq * W2[j] * (1.f - u * u);     // d loss / d (perturb_linear pre-activation)
            stageD[l32 * LDS_STRIDE + j] = u;
        }
        // lane = hidden unit: contraction over the wave's 32 rows in row order
        for (int t = 0; t < H / 64; ++t) {
            const int j = lane + 64 * t;
            float gb = 0.f, gw2 = 0.f, gw1[ERD_MAX_F + 1];
#pragma unroll
            for (int c = 0; c <= ERD_MAX_F; ++c) gw1[c] = 0.f;
            for (int rr = 0; rr < 32; ++rr) {
                const float dv = stageA[rr * LDS_STRIDE + j];
                gb += dv;
                gw2 = fmaf(gbuf[wave][rr], stageD[rr * LDS_STRIDE + j], gw2);
#pragma unroll
                for (int c = 0; c <= ERD_MAX_F; ++c)
                    if (c <= F) gw1[c] = fmaf(dv, xr[wave][rr][c], gw1[c]);
            }
            put(p.L.b_off[T + 1] + j, gb);
            put(p.L.w_off[T + 2] + j, gw2);
#pragma unroll
            for (int c = 0; c <= ERD_MAX_F; ++c)
                if (c <= F) put(p.L.w_off[T + 1] + (long long)j * (F + 1) + c, gw1[c]);
        }
        if (lane == 0) {
            float gb2 = 0.f;
            for (int rr = 0; rr < 32; ++rr) gb2 += gbuf[wave][rr];
            put(p.L.b_off[T + 2], gb2);
        }
    }
}

struct ErdReduce {
    float* params; float* grads; float* m; float* v;   // grads nullable; params / m / v used when do_adam
    const float* slabs;                                  // [nslabs][P]
    const float* loss_partial; const float* ymax_partial;   // [nparts] or null
    float* loss_out;                                     // or null
    const int* gate_in; int* gate_out;                   // or null
    int* status;                                         // {state, steps_done, last_loss, y_max} or null
    long long P, group_b;
    int nslabs, nparts, do_adam, check_stop;
    float one_minus_b1, b2, one_minus_b2, eps, bc2_sqrt, step_size_a, step_size_b, inv_count, threshold;
};

// A block owns 64 consecutive parameters; its 4 waves each sum a quarter of the slabs, the quarters are combined in a fixed
// order (as small_reduce_adam_kernel).  Block 0 also finishes the loss and the running max and decides the next state.
__global__ void __launch_bounds__(256) erd_reduce_kernel(const ErdReduce p) {
    __shared__ float part[4][64];
    __shared__ float red[2][256];
    const int state = p.gate_in ? *p.gate_in : INR_ERD_RUNNING;
    if (state != INR_ERD_RUNNING) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && p.gate_out) *p.gate_out = state;
        return;
    }
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * 64 + lane;
    float a0 = 0.f, a1 = 0.f;
    if (i < p.P) {
        int s = q;
        for (; s + 4 < p.nslabs; s += 8) {
            a0 += p.slabs[(long long)s * p.P + i];
            a1 += p.slabs[(long long)(s + 4) * p.P + i];
        }
        if (s < p.nslabs) a0 += p.slabs[(long long)s * p.P + i];
    }
    part[q][lane] = a0 + a1;
    __syncthreads();
    if (q == 0 && i < p.P) {
        const float gi = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        if (p.grads) p.grads[i] = gi;
        if (p.do_adam) {
            float* __restrict__ m = p.m;
            float* __restrict__ v = p.v;
            float* __restrict__ w = p.params;
            const float step_size = i < p.group_b ? p.step_size_a : p.step_size_b;
            adam_update(w[i], m[i], v[i], gi, AdamConsts{p.one_minus_b1, p.b2, p.one_minus_b2, step_size, p.bc2_sqrt, p.eps});
        }
    }
    if (blockIdx.x == 0 && (p.loss_out || p.status || p.gate_out)) {
        float acc = 0.f, mx = 0.f;
        if (p.loss_partial)
            for (int k = threadIdx.x; k < p.nparts; k += 256) {
                acc += p.loss_partial[k];
                mx = fmaxf(mx, p.ymax_partial[k]);
            }
        red[0][threadIdx.x] = acc;
        red[1][threadIdx.x] = mx;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) {
                red[0][threadIdx.x] += red[0][threadIdx.x + st];
                red[1][threadIdx.x] = fmaxf(red[1][threadIdx.x], red[1][threadIdx.x + st]);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const float loss = red[0][0] * p.inv_count, ymax = red[1][0];
            int next = INR_ERD_RUNNING;
            if (p.check_stop) {
                if (ymax == 0.f) next = INR_ERD_COLLAPSED;            // tested first: it wins over convergence
                else if (loss <= p.threshold) next = INR_ERD_CONVERGED;
            }
            if (p.loss_out) p.loss_out[0] = loss;
            if (p.status) {
                p.status[0] = next;
                p.status[1] = p.status[1] + 1;
                reinterpret_cast<float*>(p.status)[2] = loss;
                reinterpret_cast<float*>(p.status)[3] = ymax;
            }
            if (p.gate_out) *p.gate_out = next;
        }
    }
}

__global__ void erd_gate_init_kernel(int* gate, const int* status) {
    gate[0] = status[0];
    gate[1] = status[0];
}

// Soft-ERD (INR_ERD.py:143-158, 225-235), one pixel per thread, float64.
__global__ void __launch_bounds__(256) soft_erd_kernel(double* __restrict__ weights, double* __restrict__ mean_image,
                                                       const double* __restrict__ values, const double* __restrict__ b0,
                                                       long long n, int K, double noise_level, double mul, double slope,
                                                       double min_temp, int* __restrict__ nonfinite) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* x = values + i * K;
    double* w = weights + i * K;
    double sum = 0.0, xmax = x[0];
    for (int k = 0; k < K; ++k) {
        sum += x[k];
        xmax = fmax(xmax, x[k]);
    }
    const double mean = sum / (double)K;
    int bad = 0;
    if (mean > 2.0 * noise_level) {
        const double temp = fmax(mul * exp(-slope * (mean / b0[i])), min_temp);
        double den = 0.0, num = 0.0;
        for (int k = 0; k < K; ++k) {
            const double wk = exp(x[k] / temp);               // unnormalised, as the reference passes it to the loss
            w[k] = wk;
            bad += !isfinite(wk);
            const double e = exp((x[k] - xmax) / temp);
            den += e;
            num += e * x[k];
        }
        mean_image[i] = num / den;
    } else {
        for (int k = 0; k < K; ++k) w[k] = 1.0 / (double)K;
        mean_image[i] = mean;
    }
    if (bad) atomicAdd(nonfinite, bad);
}

bool erd_desc_ok(const inr_siren_desc_t* d) {
    return d && d->out_features == 1 && d->in_features >= 1 && d->in_features <= ERD_MAX_F &&
           (d->hidden_features == 64 || d->hidden_features == 128) && d->hidden_layers >= 0 &&
           d->hidden_layers <= ERD_MAX_HIDDEN_LAYERS;
}

void erd_layout(const inr_siren_desc_t* d, ErdLayout& L) {
    const int F = d->in_features, H = d->hidden_features;
    L.T = d->hidden_layers + 2;
    long long off = 0;
    auto pad4 = [](long long x) { return (x + 3) / 4 * 4; };
    for (int t = 0; t < L.T + 3; ++t) {
        const long long in_f = (t == 0) ? F : (t == L.T + 1) ? F + 1 : H;
        const long long out_f = (t == L.T || t == L.T + 2) ? 1 : H;
        L.w_off[t] = off;
        off += pad4(in_f * out_f);
        L.b_off[t] = off;
        off += pad4(out_f);
        if (t == L.T) L.group_b = off;
    }
    L.P = off;
}

inline int erd_blocks(int64_t n) { return (int)((n + ERD_ROWS - 1) / ERD_ROWS); }

struct ErdWs {
    float *acts, *dacts, *slabs, *loss_partial, *ymax_partial;
    int* gate;
    int nwaves;
    size_t bytes;
};

void erd_carve(const inr_siren_desc_t* d, const ErdLayout& L, int64_t n, void* ws, ErdWs& w) {
    const size_t nh = (size_t)n * d->hidden_features;
    w.nwaves = erd_blocks(n) * ERD_WAVES;
    WsCarver c(ws, 4 * sizeof(float));
    w.acts = c.take<float>((size_t)(L.T - 1) * nh);
    w.dacts = c.take<float>((size_t)(L.T - 1) * nh);
    w.slabs = c.take<float>((size_t)w.nwaves * (size_t)L.P);
    w.loss_partial = c.take<float>(w.nwaves);
    w.ymax_partial = c.take<float>(w.nwaves);
    w.gate = c.take<int>(4);
    w.bytes = c.bytes();
}

struct ErdCall {
    const float* target; const float* weight; float* y_out; const int* gate;
    float sample, eps;
    int perturb, accumulate;
};

template <bool TRAIN>
int erd_launch_step(const inr_siren_desc_t* d, const ErdLayout& L, const ErdWs& w, const float* params, const float* x, int64_t n,
                    const ErdCall& c, hipStream_t st) {
    ErdStep p{};
    p.params = params;
    p.slabs = w.slabs; p.loss_partial = w.loss_partial; p.ymax_partial = w.ymax_partial; p.acts = w.acts; p.dacts = w.dacts;
    p.x = x; p.target = c.target; p.weight = c.weight; p.y_out = c.y_out; p.gate = c.gate;
    p.L = L;
    p.N = (int)n; p.F = d->in_features; p.S = d->hidden_layers + 1;
    p.first_omega = d->first_omega; p.hidden_omega = d->hidden_omega;
    p.inv_count = (float)(1.0 / (double)n);
    p.sample = c.sample; p.eps = c.eps; p.perturb = c.perturb; p.accumulate = c.accumulate;
    ProfScope ps(KC_OTHER, st);
    if (d->hidden_features == 128)
        hipLaunchKernelGGL((erd_step_kernel<128, TRAIN>), dim3(erd_blocks(n)), dim3(ERD_THREADS), 0, st, p);
    else
        hipLaunchKernelGGL((erd_step_kernel<64, TRAIN>), dim3(erd_blocks(n)), dim3(ERD_THREADS), 0, st, p);
    INR_LAUNCH_CHECK();
    count_launch(TRAIN ? INR_LF_ERD_STEP : INR_LF_ERD_FORWARD);
    return 0;
}

void erd_adam_consts(ErdReduce& r, int64_t step, double lr_a, double lr_b, double b1, double b2, double eps) {
    const AdamConsts a = adam_consts(step, lr_a, b1, b2, eps);   // the two groups differ in the learning rate only
    r.do_adam = 1;
    r.one_minus_b1 = a.one_minus_b1;
    r.b2 = a.b2;
    r.one_minus_b2 = a.one_minus_b2;
    r.step_size_a = a.step_size;
    r.step_size_b = adam_consts(step, lr_b, b1, b2, eps).step_size;
    r.bc2_sqrt = a.bc2_sqrt;
    r.eps = a.eps;
}

int erd_launch_reduce(const ErdReduce& r, hipStream_t st) {
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL(erd_reduce_kernel, dim3((unsigned)((r.P + 63) / 64)), dim3(256), 0, st, r);
    INR_LAUNCH_CHECK();
    count_launch(INR_LF_ERD_REDUCE);
    return 0;
}

constexpr int64_t ERD_MAX_ROWS = 1 << 18;

// the refusals the training entry points share; on success L and w hold the call's layout and its workspace view
int erd_common_checks(const inr_siren_desc_t* desc, int64_t n, void* ws, size_t ws_bytes, const char* who, ErdLayout& L, ErdWs& w) {
    INR_REQUIRE(erd_desc_ok(desc), INR_E_INVALID,
                "%s: the soft-ERD kernels serve out_features == 1, in_features <= 8, hidden_features in {64, 128}, "
                "hidden_layers <= 8", who);
    INR_REQUIRE(n >= 1 && n <= ERD_MAX_ROWS, INR_E_INVALID, "%s: n = %lld outside 1 .. %lld", who, (long long)n,
                (long long)ERD_MAX_ROWS);
    erd_layout(desc, L);
    erd_carve(desc, L, n, ws, w);
    INR_REQUIRE(ws && aligned16(ws) && ws_bytes >= w.bytes, INR_E_WORKSPACE, "%s: workspace too small", who);
    return 0;
}

}  // namespace

}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_erd_param_count(const inr_siren_desc_t* desc) {
    INR_REQUIRE(erd_desc_ok(desc), -1, "inr_erd_param_count: bad soft-ERD descriptor");
    ErdLayout L;
    erd_layout(desc, L);
    return (int64_t)L.P;
}

int inr_erd_param_offsets(const inr_siren_desc_t* desc, int64_t* offsets, int max_entries) {
    INR_REQUIRE(erd_desc_ok(desc) && offsets, INR_E_INVALID, "inr_erd_param_offsets: bad soft-ERD descriptor or null pointer");
    ErdLayout L;
    erd_layout(desc, L);
    const int tensors = L.T + 3;
    INR_REQUIRE(max_entries >= 2 * tensors + 1, INR_E_INVALID, "inr_erd_param_offsets: room for %d entries needed", 2 * tensors + 1);
    for (int t = 0; t < tensors; ++t) {
        offsets[2 * t] = L.w_off[t];
        offsets[2 * t + 1] = L.b_off[t];
    }
    offsets[2 * tensors] = L.group_b;
    return 0;
}

size_t inr_erd_workspace_bytes(const inr_siren_desc_t* desc, int64_t n) {
    if (!erd_desc_ok(desc) || n < 1 || n > ERD_MAX_ROWS) return 0;
    ErdLayout L;
    erd_layout(desc, L);
    ErdWs w;
    erd_carve(desc, L, n, nullptr, w);
    return w.bytes;
}

int inr_erd_forward(const inr_siren_desc_t* desc, const float* params, const float* x, int64_t n, float* y, int sample, float eps,
                    int perturb, int64_t chunk_rows, void* stream) {
    INR_REQUIRE(erd_desc_ok(desc), INR_E_INVALID, "inr_erd_forward: shape not served by the soft-ERD kernels");
    INR_REQUIRE(params && x && y && n >= 1 && chunk_rows >= 1, INR_E_INVALID, "inr_erd_forward: null pointer or non-positive size");
    INR_REQUIRE(aligned16(params), INR_E_ALIGN, "inr_erd_forward: params must be 16-byte aligned");
    ErdLayout L;
    erd_layout(desc, L);
    if (chunk_rows > ERD_MAX_ROWS) chunk_rows = ERD_MAX_ROWS;
    ErdWs w{};
    for (int64_t r = 0; r < n; r += chunk_rows) {
        const int64_t rows = n - r < chunk_rows ? n - r : chunk_rows;
        ErdCall c{nullptr, nullptr, y + r, nullptr, (float)sample, eps, perturb != 0, 0};
        if (int rc = erd_launch_step<false>(desc, L, w, params, x + r * desc->in_features, rows, c, (hipStream_t)stream)) return rc;
    }
    return 0;
}

int inr_erd_loss_grad(const inr_siren_desc_t* desc, const float* params, float* grads, const float* x, const float* target,
                      const float* weight, int64_t n, int sample, float eps, int perturb, int accumulate, float* loss,
                      void* workspace, size_t workspace_bytes, void* stream) {
    ErdLayout L;
    ErdWs w;
    if (int rc = erd_common_checks(desc, n, workspace, workspace_bytes, "inr_erd_loss_grad", L, w)) return rc;
    INR_REQUIRE(params && grads && x && target && loss, INR_E_INVALID, "inr_erd_loss_grad: null pointer");
    INR_REQUIRE(aligned16(params), INR_E_ALIGN, "inr_erd_loss_grad: params must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ErdCall c{target, weight, nullptr, nullptr, (float)sample, eps, perturb != 0, accumulate != 0};
    if (int rc = erd_launch_step<true>(desc, L, w, params, x, n, c, st)) return rc;
    ErdReduce r{};
    r.grads = grads; r.slabs = w.slabs; r.nslabs = w.nwaves; r.P = L.P; r.group_b = L.group_b;
    r.loss_partial = w.loss_partial; r.ymax_partial = w.ymax_partial; r.nparts = w.nwaves; r.loss_out = loss;
    r.inv_count = (float)(1.0 / (double)n);
    return erd_launch_reduce(r, st);
}

int inr_erd_adam_step(const inr_siren_desc_t* desc, float* params, const float* grads, float* m, float* v, int64_t step,
                      double lr_net, double lr_perturb, double beta1, double beta2, double eps, void* stream) {
    INR_REQUIRE(erd_desc_ok(desc), INR_E_INVALID, "inr_erd_adam_step: shape not served by the soft-ERD kernels");
    INR_REQUIRE(params && grads && m && v && step >= 1, INR_E_INVALID, "inr_erd_adam_step: null pointer or non-positive step");
    ErdLayout L;
    erd_layout(desc, L);
    ErdReduce r{};
    r.params = params; r.m = m; r.v = v; r.slabs = grads; r.nslabs = 1; r.P = L.P; r.group_b = L.group_b;
    erd_adam_consts(r, step, lr_net, lr_perturb, beta1, beta2, eps);
    return erd_launch_reduce(r, (hipStream_t)stream);
}

int inr_erd_pretrain(const inr_siren_desc_t* desc, float* params, float* grads, float* m, float* v, const float* x,
                     const float* target, int64_t n, int64_t first_step, int max_steps, double lr, double beta1, double beta2,
                     double eps, float threshold, int* status, void* workspace, size_t workspace_bytes, void* stream) {
    ErdLayout L;
    ErdWs w;
    if (int rc = erd_common_checks(desc, n, workspace, workspace_bytes, "inr_erd_pretrain", L, w)) return rc;
    INR_REQUIRE(params && grads && m && v && x && target && status && first_step >= 1 && max_steps >= 0, INR_E_INVALID,
                "inr_erd_pretrain: null pointer or bad step numbers");
    INR_REQUIRE(aligned16(params), INR_E_ALIGN, "inr_erd_pretrain: params must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(erd_gate_init_kernel, dim3(1), dim3(1), 0, st, w.gate, status);
    INR_LAUNCH_CHECK();
    for (int it = 0; it < max_steps; ++it) {
        ErdCall c{target, nullptr, nullptr, w.gate + (it & 1), 0.f, 0.f, 0, 0};      // INR_ERD.py:204: perturb off, unweighted
        if (int rc = erd_launch_step<true>(desc, L, w, params, x, n, c, st)) return rc;
        ErdReduce r{};
        r.params = params; r.grads = grads; r.m = m; r.v = v; r.slabs = w.slabs; r.nslabs = w.nwaves; r.P = L.P; r.group_b = L.group_b;
        r.loss_partial = w.loss_partial; r.ymax_partial = w.ymax_partial; r.nparts = w.nwaves;
        r.inv_count = (float)(1.0 / (double)n);
        r.gate_in = w.gate + (it & 1); r.gate_out = w.gate + ((it + 1) & 1); r.status = status;
        r.check_stop = 1; r.threshold = threshold;
        erd_adam_consts(r, first_step + it, lr, lr, beta1, beta2, eps);
        if (int rc = erd_launch_reduce(r, st)) return rc;
    }
    return 0;
}

int inr_erd_finetune(const inr_siren_desc_t* desc, float* params, float* grads, float* m, float* v, const float* x,
                     const float* targets, const float* weights, int n_acq, int64_t n, float perturb_eps, int64_t first_step,
                     int n_steps, double lr_perturb, double lr_net, double beta1, double beta2, double eps, float* losses,
                     void* workspace, size_t workspace_bytes, void* stream) {
    ErdLayout L;
    ErdWs w;
    if (int rc = erd_common_checks(desc, n, workspace, workspace_bytes, "inr_erd_finetune", L, w)) return rc;
    INR_REQUIRE(params && grads && m && v && x && targets && n_acq >= 1 && first_step >= 1 && n_steps >= 0, INR_E_INVALID,
                "inr_erd_finetune: null pointer or bad counts");
    INR_REQUIRE(aligned16(params), INR_E_ALIGN, "inr_erd_finetune: params must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    for (int it = 0; it < n_steps; ++it) {
        for (int s = 0; s < n_acq; ++s) {
            ErdCall c{targets + (int64_t)s * n, weights ? weights + (int64_t)s * n : nullptr, nullptr, nullptr, (float)s, perturb_eps,
                      1, s > 0};
            if (int rc = erd_launch_step<true>(desc, L, w, params, x, n, c, st)) return rc;
        }
        ErdReduce r{};
        r.params = params; r.grads = grads; r.m = m; r.v = v; r.slabs = w.slabs; r.nslabs = w.nwaves; r.P = L.P; r.group_b = L.group_b;
        r.loss_partial = w.loss_partial; r.ymax_partial = w.ymax_partial; r.nparts = w.nwaves;
        r.loss_out = losses ? losses + it : nullptr;
        r.inv_count = (float)(1.0 / (double)n);
        erd_adam_consts(r, first_step + it, lr_net, lr_perturb, beta1, beta2, eps);
        if (int rc = erd_launch_reduce(r, st)) return rc;
    }
    return 0;
}

int inr_soft_erd(double* weights, double* mean_image, const double* values, const double* b0, int64_t n_pixels, int n_acquisitions,
                 double noise_level, double mul, double slope, double min_temp, int* nonfinite_count, void* stream) {
    INR_REQUIRE(weights && mean_image && values && b0 && nonfinite_count && n_pixels >= 1 && n_acquisitions >= 1, INR_E_INVALID,
                "inr_soft_erd: null pointer or non-positive size");
    hipStream_t st = (hipStream_t)stream;
    INR_HIP(hipMemsetAsync(nonfinite_count, 0, sizeof(int), st));
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL(soft_erd_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, st, weights, mean_image, values, b0,
                       (long long)n_pixels, n_acquisitions, noise_level, mul, slope, min_temp, nonfinite_count);
    INR_LAUNCH_CHECK();
    count_launch(INR_LF_ERD_SOFT);
    return 0;
}

}  // extern "C"
