// RAMS training step (SURVEY.md 8 a-15 / (f)-4): forward with stash -> cL1 loss -> backward through every layer ->
// weight-normalisation backward -> Adam.  Included by rams.hip (same translation unit: it drives that file's kernels).
//   /root/reference/multi-image-super-resolution/utils/training.py:193-209 (train_step: tape.gradient of the per-image
//   loss vector = gradient of its SUM, then apply_gradients), utils/loss.py:26-75 (l1_loss), utils/network.py:29-35
//   (tfa WeightNormalization: kernel = g * v / ||v||, norm over every axis but the output channel), :42-63 RFAB, :65-87 RTAB,
//   :37-39 reflective padding, :141,148 depth_to_space.
// Parameters travel in the reference's own form ("raw" layout): per layer v [rows = taps * cin][cout], g [cout], b [cout],
// every segment padded to 4 floats, layers in graph order (the order of rams.rams_layer_specs).  Each step folds them into
// the packed inference layout (include/inrhip.h), runs the forward kernels of rams.hip on it with every intermediate kept,
// walks back, and un-folds the gradient of the folded kernels into (dv, dg, db).
// The convolutions 32 -> 32 (>= 99 % of the work) use the MFMA kernels of rams.hip (forward, data gradient = forward on the
// flipped / transposed kernel, weight gradient = MFMA contraction over the voxels); everything else is direct kernels with
// fixed-order reductions (no float atomics: a step is bitwise reproducible).
#include <vector>

struct TLayer {
    int rows, cout, fcout;          // fcout: output channels of the folded tensor (the 32 -> 9 head is padded to 32)
    long long v, g, b;              // offsets (floats) into the raw buffer
    long long fw, fb;               // offsets into the folded buffer
};

__host__ __device__ static inline long long pad4(long long n) { return (n + 3) / 4 * 4; }

static void rams_train_layers(const inr_rams_desc_t* d, std::vector<TLayer>& L, long long* raw_total, long long* fold_total) {
    long long ro = 0, fo = 0;
    auto add = [&](int rows, int cout, int fcout) {
        TLayer t{rows, cout, fcout, 0, 0, 0, 0, 0};
        t.v = ro; ro += pad4((long long)rows * cout);
        t.g = ro; ro += pad4(cout);
        t.b = ro; ro += pad4(cout);
        t.fw = fo; fo += pad4((long long)rows * fcout);
        t.fb = fo; fo += pad4(fcout);
        L.push_back(t);
    };
    const int F = d->filters, Cr = F / d->r, T = d->channels, Tr = T / d->r > 0 ? T / d->r : 1, S2 = d->scale * d->scale;
    auto rfab = [&]() { add(27 * F, F, F); add(27 * F, F, F); add(F, Cr, Cr); add(Cr, F, F); };
    add(27, F, F);
    for (int i = 0; i < d->n_rfab; ++i) rfab();
    add(27 * F, F, F);
    for (int i = 0; i < T / 3; ++i) { rfab(); add(27 * F, F, F); }
    add(27 * F, S2, RC);
    add(9 * T, T, T); add(9 * T, T, T); add(T, Tr, Tr); add(Tr, T, T);
    add(9 * T, S2, S2);
    *raw_total = ro;
    *fold_total = fo;
}

// ---- weight normalisation: fold and its backward ----------------------------------------------------------------------------
struct FoldJobs {
    const float* raw;
    float* raw_grad;        // backward: receives dv, dg, db
    float* fold;            // forward: receives the folded kernels and biases;  backward: holds dK and db
    int n;
};
struct FoldLayer { int rows, cout, fcout; long long v, g, b, fw, fb; };
// The layer table travels BY VALUE in the kernel arguments (24 bytes per layer): round 3 uploaded it with hipMemcpyAsync and had
// to hipStreamSynchronize on every call (the host vector died with the scope) -- a host sync in an entry point the header
// promises only enqueues (include/inrhip.h).
constexpr int FOLD_MAX_LAYERS = 128;
struct FoldLayerC { unsigned short rows; unsigned char cout, fcout; int v, g, b, fw, fb; };
struct FoldTable { FoldLayerC l[FOLD_MAX_LAYERS]; };
__device__ __forceinline__ FoldLayer fold_layer(const FoldTable& T, int i) {
    const FoldLayerC c = T.l[i];
    return FoldLayer{(int)c.rows, (int)c.cout, (int)c.fcout, c.v, c.g, c.b, c.fw, c.fb};
}

// one block per layer; column c handled by threads c, c + 32, ... (8 row phases)
__global__ void __launch_bounds__(256) fold_kernel(const FoldJobs J, const FoldTable layers) {
    __shared__ float part[8][32];
    __shared__ float scale[32];
    const FoldLayer L = fold_layer(layers, blockIdx.x);
    const int c = threadIdx.x & 31, ph = threadIdx.x >> 5;
    const float* v = J.raw + L.v;
    float s = 0.f;
    if (c < L.cout)
        for (int r = ph; r < L.rows; r += 8) {
            const float x = v[(long long)r * L.cout + c];
            s = fmaf(x, x, s);
        }
    part[ph][c] = s;
    __syncthreads();
    if (threadIdx.x < 32) {
        float n2 = 0.f;
        for (int k = 0; k < 8; ++k) n2 += part[k][c];
        scale[c] = c < L.cout ? J.raw[L.g + c] / sqrtf(n2) : 0.f;
    }
    __syncthreads();
    float* w = J.fold + L.fw;
    for (int i = threadIdx.x; i < L.rows * L.fcout; i += 256) {
        const int r = i / L.fcout, cc = i % L.fcout;
        w[i] = cc < L.cout ? v[(long long)r * L.cout + cc] * scale[cc] : 0.f;
    }
    for (int i = threadIdx.x; i < L.fcout; i += 256) J.fold[L.fb + i] = i < L.cout ? J.raw[L.b + i] : 0.f;
}

// K = g v / n, n = ||v||:  dg = <dK, v> / n;  dv = (g / n) (dK - v <dK, v> / n^2);  db = db
__global__ void __launch_bounds__(256) fold_backward_kernel(const FoldJobs J, const FoldTable layers) {
    __shared__ float p_n2[8][32], p_dot[8][32];
    __shared__ float s_gn[32], s_coef[32];
    const FoldLayer L = fold_layer(layers, blockIdx.x);
    const int c = threadIdx.x & 31, ph = threadIdx.x >> 5;
    const float* v = J.raw + L.v;
    const float* dK = J.fold + L.fw;
    float n2 = 0.f, dot = 0.f;
    if (c < L.cout)
        for (int r = ph; r < L.rows; r += 8) {
            const float x = v[(long long)r * L.cout + c];
            n2 = fmaf(x, x, n2);
            dot = fmaf(dK[(long long)r * L.fcout + c], x, dot);
        }
    p_n2[ph][c] = n2;
    p_dot[ph][c] = dot;
    __syncthreads();
    if (threadIdx.x < 32 && c < L.cout) {
        float a = 0.f, b = 0.f;
        for (int k = 0; k < 8; ++k) {
            a += p_n2[k][c];
            b += p_dot[k][c];
        }
        const float n = sqrtf(a);
        J.raw_grad[L.g + c] = b / n;
        s_gn[c] = J.raw[L.g + c] / n;
        s_coef[c] = b / a;
        J.raw_grad[L.b + c] = J.fold[L.fb + c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < L.rows * L.cout; i += 256) {
        const int r = i / L.cout, cc = i % L.cout;
        J.raw_grad[L.v + i] = s_gn[cc] * (dK[(long long)r * L.fcout + cc] - v[i] * s_coef[cc]);
    }
}

// ---- small backward kernels ---------------------------------------------------------------------------------------------------
// (amax, nullable: slot that receives max|d| of the masked gradient -- the next convolution's operand scale.  Grid-stride over
// float4 with at most 2,048 blocks: one block reduction and one atomic per block -- with a block per 256 elements the maximum cost
// more than a separate pass over the tensor)
__global__ void __launch_bounds__(256) relu_backward_kernel(float* __restrict__ d, const float* __restrict__ a, long long total,
                                                            unsigned* amax = nullptr) {
    float m = 0.f;
    const long long n4 = total >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        float4 v = reinterpret_cast<float4*>(d)[i];
        const float4 w = reinterpret_cast<const float4*>(a)[i];
        v.x = w.x > 0.f ? v.x : 0.f; v.y = w.y > 0.f ? v.y : 0.f; v.z = w.z > 0.f ? v.z : 0.f; v.w = w.w > 0.f ? v.w : 0.f;
        reinterpret_cast<float4*>(d)[i] = v;
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    for (long long i = (n4 << 2) + (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {   // tail
        const float v = a[i] > 0.f ? d[i] : 0.f;
        d[i] = v;
        m = fmaxf(m, fabsf(v));
    }
    if (amax) r3_block_amax(m, amax);
}
__global__ void __launch_bounds__(256) accumulate_kernel(float* __restrict__ d, const float* __restrict__ a, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) d[i] += a[i];
}

// gate of the attention blocks with everything the backward pass needs: mean [B][C], sq [B][Cr] (after ReLU), gate [B][C]
__global__ void __launch_bounds__(256) gate_train_kernel(float* __restrict__ gate, float* __restrict__ mean_out,
                                                         float* __restrict__ sq_out, const float* __restrict__ slab, int nslab,
                                                         float inv_count, const float* __restrict__ wsq,
                                                         const float* __restrict__ bsq, const float* __restrict__ wex,
                                                         const float* __restrict__ bex, int C, int Cr) {
    __shared__ float part[256];
    __shared__ float mean[32];
    __shared__ float sq[8];
    const int b = blockIdx.x, t = threadIdx.x;
    const int c = t % 32, ph = t / 32;
    float acc = 0.f;
    if (c < C)
        for (int s = ph; s < nslab; s += 8) acc += slab[((long long)b * nslab + s) * C + c];
    part[t] = acc;
    __syncthreads();
    if (t < C) {
        float m = 0.f;
        for (int k = 0; k < 8; ++k) m += part[k * 32 + t];
        mean[t] = m * inv_count;
        mean_out[b * C + t] = mean[t];
    }
    __syncthreads();
    if (t < Cr) {
        float s = bsq[t];
        for (int k = 0; k < C; ++k) s = fmaf(mean[k], wsq[k * Cr + t], s);
        sq[t] = fmaxf(s, 0.f);
        sq_out[b * Cr + t] = sq[t];
    }
    __syncthreads();
    if (t < C) {
        float e = bex[t];
        for (int k = 0; k < Cr; ++k) e = fmaf(sq[k], wex[k * C + t], e);
        gate[b * C + t] = 1.0f / (1.0f + expf(-e));
    }
}

// slab[b][blk][C] = partial sums over the voxels of dout * y  (d gate, before the sigmoid)
__global__ void __launch_bounds__(256) chan_dot_partial_kernel(float* __restrict__ slab, const float* __restrict__ dout,
                                                               const float* __restrict__ y, long long per_b, int C, int nblk) {
    __shared__ float part[256];
    const int b = blockIdx.y, t = threadIdx.x;
    const int c = t % 32, ph = t / 32;
    float acc = 0.f;
    if (c < C)
        for (long long v = (long long)blockIdx.x * 8 + ph; v < per_b; v += (long long)nblk * 8) {
            const long long at = ((long long)b * per_b + v) * C + c;
            acc = fmaf(dout[at], y[at], acc);
        }
    part[t] = acc;
    __syncthreads();
    if (t < C) {
        float s = 0.f;
        for (int k = 0; k < 8; ++k) s += part[k * 32 + t];
        slab[((long long)b * nblk + blockIdx.x) * C + t] = s;
    }
}

// one block per batch element: backward of sigmoid(excite(relu(squeeze(mean)))).  Per-element partial gradients
// gpart[b][wsq C*Cr | bsq Cr | wex Cr*C | bex C] (each padded to 4), dpool[b][C] = d loss / d mean / voxels.
__global__ void __launch_bounds__(64) gate_backward_kernel(float* __restrict__ gpart, float* __restrict__ dpool,
                                                           const float* __restrict__ slab, int nslab,
                                                           const float* __restrict__ gate, const float* __restrict__ mean,
                                                           const float* __restrict__ sq, const float* __restrict__ wsq,
                                                           const float* __restrict__ wex, int C, int Cr, float inv_count,
                                                           long long gstride) {
    __shared__ float de[32], dsq[8];
    const int b = blockIdx.x, t = threadIdx.x;
    float* G = gpart + (long long)b * gstride;
    const long long o_bsq = pad4((long long)C * Cr), o_wex = o_bsq + pad4(Cr), o_bex = o_wex + pad4((long long)Cr * C);
    if (t < C) {
        // (eight loads in flight per step of the chain, the additions in the order they always had: one dependent load per slab was
        //  64 L2 latencies -- 19 of the kernel's 21 us)
        float dg = 0.f;
        int s = 0;
        for (; s + 8 <= nslab; s += 8) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = slab[((long long)b * nslab + s + k) * C + t];
#pragma unroll
            for (int k = 0; k < 8; ++k) dg += v[k];
        }
        for (; s < nslab; ++s) dg += slab[((long long)b * nslab + s) * C + t];
        const float gt = gate[b * C + t];
        de[t] = dg * gt * (1.0f - gt);
        G[o_bex + t] = de[t];
    }
    __syncthreads();
    if (t < Cr) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s = fmaf(de[c], wex[t * C + c], s);
        dsq[t] = sq[b * Cr + t] > 0.f ? s : 0.f;
        G[o_bsq + t] = dsq[t];
    }
    __syncthreads();
    for (int i = t; i < Cr * C; i += 64) G[o_wex + i] = sq[b * Cr + i / C] * de[i % C];
    for (int i = t; i < C * Cr; i += 64) G[i] = mean[b * C + i / Cr] * dsq[i % Cr];
    if (t < C) {
        float s = 0.f;
        for (int k = 0; k < Cr; ++k) s = fmaf(dsq[k], wsq[t * Cr + k], s);
        dpool[b * C + t] = s * inv_count;
    }
}

// dy = dout * gate[b][c] + dpool[b][c]   (C a multiple of 4 takes the float4 path; amax as in relu_backward_kernel)
__global__ void __launch_bounds__(256) gate_apply_backward_kernel(float* __restrict__ dy, const float* __restrict__ dout,
                                                                  const float* __restrict__ gate, const float* __restrict__ dpool,
                                                                  long long per_b, int C, long long total,
                                                                  unsigned* amax = nullptr) {
    float m = 0.f;
    if ((C & 3) == 0) {
        const long long n4 = total >> 2, pb4 = per_b * C >> 2;
        const int c4n = C >> 2;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
            const int c4 = (int)(i % c4n);
            const int b = (int)(i / pb4);
            const float4 g = reinterpret_cast<const float4*>(gate + (long long)b * C)[c4];
            const float4 p = reinterpret_cast<const float4*>(dpool + (long long)b * C)[c4];
            const float4 x = reinterpret_cast<const float4*>(dout)[i];
            const float4 v = make_float4(fmaf(x.x, g.x, p.x), fmaf(x.y, g.y, p.y), fmaf(x.z, g.z, p.z), fmaf(x.w, g.w, p.w));
            reinterpret_cast<float4*>(dy)[i] = v;
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
    } else {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
            const int c = (int)(i % C);
            const int b = (int)(i / (per_b * C));
            const float v = fmaf(dout[i], gate[b * C + c], dpool[b * C + c]);
            dy[i] = v;
            m = fmaxf(m, fabsf(v));
        }
    }
    if (amax) r3_block_amax(m, amax);
}

// backward of tf.pad REFLECT by 1 on axes 1, 2: every interior sample collects the padded positions that mirror onto it
__global__ void __launch_bounds__(256) reflect_pad_backward_kernel(float* __restrict__ dx, const float* __restrict__ dout, int B,
                                                                   int D1, int D2, int inner) {
    const long long total = (long long)B * D1 * D2 * inner;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % inner);
    long long v = i / inner;
    const int i2 = (int)(v % D2); v /= D2;
    const int i1 = (int)(v % D1);
    const int b = (int)(v / D1);
    int o1[2] = {i1 + 1, -1}, o2[2] = {i2 + 1, -1};
    if (i1 == 1) o1[1] = 0;
    else if (i1 == D1 - 2) o1[1] = D1 + 1;
    if (i2 == 1) o2[1] = 0;
    else if (i2 == D2 - 2) o2[1] = D2 + 1;
    float s = 0.f;
    for (int a = 0; a < 2; ++a)
        for (int c = 0; c < 2; ++c)
            if (o1[a] >= 0 && o2[c] >= 0) s += dout[(((long long)b * (D1 + 2) + o1[a]) * (D2 + 2) + o2[c]) * inner + k];
    // D1 == 3: rows 1 is both "second" and "second to last" -- both mirrors land on it
    if (D1 == 3 && i1 == 1)
        for (int c = 0; c < 2; ++c)
            if (o2[c] >= 0) s += dout[(((long long)b * (D1 + 2) + D1 + 1) * (D2 + 2) + o2[c]) * inner + k];
    if (D2 == 3 && i2 == 1)
        for (int a = 0; a < 2; ++a)
            if (o1[a] >= 0) s += dout[(((long long)b * (D1 + 2) + o1[a]) * (D2 + 2) + D2 + 1) * inner + k];
    if (D1 == 3 && i1 == 1 && D2 == 3 && i2 == 1) s += dout[(((long long)b * (D1 + 2) + D1 + 1) * (D2 + 2) + D2 + 1) * inner + k];
    dx[i] = s;
}

// the same by rows, 16 bytes per thread: one (b, i1, i2) position per block column, the sums in the order above (no index divisions:
// 30 us per call of a 9 ms step were mostly those)
__global__ void __launch_bounds__(256) reflect_pad_backward_v4_kernel(float* __restrict__ dx, const float* __restrict__ dout, int D1,
                                                                      int D2, int inner4) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const int i2 = blockIdx.x % D2, i1 = blockIdx.x / D2, b = blockIdx.y;
    int o1[2] = {i1 + 1, -1}, o2[2] = {i2 + 1, -1};
    if (i1 == 1) o1[1] = 0;
    else if (i1 == D1 - 2) o1[1] = D1 + 1;
    if (i2 == 1) o2[1] = 0;
    else if (i2 == D2 - 2) o2[1] = D2 + 1;
    const f4* img = reinterpret_cast<const f4*>(dout) + (long long)b * (D1 + 2) * (D2 + 2) * inner4;
    auto at = [&](int p1, int p2) { return img + ((long long)p1 * (D2 + 2) + p2) * inner4; };
    f4* dst = reinterpret_cast<f4*>(dx) + (((long long)b * D1 + i1) * D2 + i2) * inner4;
    for (int k = threadIdx.x; k < inner4; k += 256) {
        f4 s = {0.f, 0.f, 0.f, 0.f};
        for (int a = 0; a < 2; ++a)
            for (int c = 0; c < 2; ++c)
                if (o1[a] >= 0 && o2[c] >= 0) s += at(o1[a], o2[c])[k];
        if (D1 == 3 && i1 == 1)
            for (int c = 0; c < 2; ++c)
                if (o2[c] >= 0) s += at(D1 + 1, o2[c])[k];
        if (D2 == 3 && i2 == 1)
            for (int a = 0; a < 2; ++a)
                if (o1[a] >= 0) s += at(o1[a], D2 + 1)[k];
        if (D1 == 3 && i1 == 1 && D2 == 3 && i2 == 1) s += at(D1 + 1, D2 + 1)[k];
        dst[k] = s;
    }
}

// zero padding by 1 on the three spatial axes (the data gradient of a 'valid' convolution is the 'same'-style gradient of
// its padded output gradient), with the channel count widened from Cs to C (zeros)
__global__ void __launch_bounds__(256) zero_pad3_kernel(float* __restrict__ out, const float* __restrict__ x, int B, int D1,
                                                        int D2, int D3, int Cs, int C) {
    const long long total = (long long)B * (D1 + 2) * (D2 + 2) * (D3 + 2) * C;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    long long v = i / C;
    const int o3 = (int)(v % (D3 + 2)); v /= (D3 + 2);
    const int o2 = (int)(v % (D2 + 2)); v /= (D2 + 2);
    const int o1 = (int)(v % (D1 + 2));
    const int b = (int)(v / (D1 + 2));
    const int i1 = o1 - 1, i2 = o2 - 1, i3 = o3 - 1;
    float r = 0.f;
    if (c < Cs && (unsigned)i1 < (unsigned)D1 && (unsigned)i2 < (unsigned)D2 && (unsigned)i3 < (unsigned)D3)
        r = x[((((long long)b * D1 + i1) * D2 + i2) * D3 + i3) * Cs + c];
    out[i] = r;
}

// widen the channel axis Cs -> C with zeros (no spatial padding)
__global__ void __launch_bounds__(256) widen_channels_kernel(float* __restrict__ out, const float* __restrict__ x, long long nvox,
                                                             int Cs, int C) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvox * C) return;
    const int c = (int)(i % C);
    out[i] = c < Cs ? x[(i / C) * Cs + c] : 0.f;
}

// stem weight gradient: slab[blk][28][32]: rows 0..26 = sum_v x[v + tap - 1] dy[v][c], row 27 = sum_v dy[v][c]
// A block takes the voxels [v0, v1) in chunks of STEM_ROWS (b, i1, i2) rows: for every row of a chunk it stages the 3 x 3
// neighbouring rows of x with one zero either side of the depth axis; the 27 taps of a voxel are then 27 LDS reads at compile-time
// offsets -- no range tests, no index arithmetic (the 27 guarded global loads per voxel with their 64-bit decode were 214 us of
// a 10 ms step for 0.6 GFLOP).  Voxel -> (block, thread) and the order of every sum as before.  D3 <= STEM_TP - 2.
constexpr int STEM_ROWS = 24, STEM_TP = 16;
__global__ void __launch_bounds__(256) stem_wgrad_kernel(float* __restrict__ slab, const float* __restrict__ x,
                                                         const float* __restrict__ dy, int B, int D1, int D2, int D3,
                                                         long long vox_per_block) {
    __shared__ float part[8][28][32];
    __shared__ float tile[STEM_ROWS * 9 * STEM_TP];
    const int c = threadIdx.x & 31, ph = threadIdx.x >> 5;
    const long long nvox = (long long)B * D1 * D2 * D3;
    const long long v0 = (long long)blockIdx.x * vox_per_block, v1 = min(nvox, v0 + vox_per_block);
    const int TP = D3 + 2;
    float acc[28];
#pragma unroll
    for (int t = 0; t < 28; ++t) acc[t] = 0.f;
    long long v = v0 + ph;                                    // this thread's next voxel (they come in ascending order)
    for (unsigned rowA = (unsigned)(v0 / D3); (long long)rowA * D3 < v1; rowA += STEM_ROWS) {
        const long long cv1 = min(v1, ((long long)rowA + STEM_ROWS) * D3);          // the chunk's voxels end here
        const int nrow = (int)((unsigned)((cv1 - 1) / D3) - rowA + 1);
        __syncthreads();                                      // (the previous chunk's readers are done)
        for (int e = threadIdx.x; e < nrow * 9 * TP; e += 256) {
            const int tt = e % TP, k = (e / TP) % 9, rr = e / (TP * 9);
            unsigned row = rowA + (unsigned)rr;
            const int i2 = (int)(row % (unsigned)D2); row /= (unsigned)D2;
            const int i1 = (int)(row % (unsigned)D1);
            const int b = (int)(row / (unsigned)D1);
            const int j1 = i1 + k / 3 - 1, j2 = i2 + k % 3 - 1, j3 = tt - 1;
            const bool in = (unsigned)j1 < (unsigned)D1 && (unsigned)j2 < (unsigned)D2 && (unsigned)j3 < (unsigned)D3;
            tile[e] = in ? x[(((long long)b * D1 + j1) * D2 + j2) * D3 + j3] : 0.f;
        }
        __syncthreads();
        for (; v < cv1; v += 8) {
            const unsigned row = (unsigned)v / (unsigned)D3;
            const int i3 = (int)((unsigned)v - row * (unsigned)D3);
            const float* tp = tile + (int)(row - rowA) * 9 * TP + i3;       // tap (d1, d2, d3): tp[(3 d1 + d2) TP + d3]
            const float g = dy[v * RC + c];
            acc[27] += g;
#pragma unroll
            for (int t = 0; t < 27; ++t) acc[t] = fmaf(tp[(t / 3) * TP + t % 3], g, acc[t]);   // (outside the image: + 0 * g)
        }
    }
#pragma unroll
    for (int t = 0; t < 28; ++t) part[ph][t][c] = acc[t];
    __syncthreads();
    for (int i = threadIdx.x; i < 28 * 32; i += 256) {
        float s = 0.f;
        for (int k = 0; k < 8; ++k) s += part[k][i / 32][i % 32];
        slab[(long long)blockIdx.x * 28 * 32 + i] = s;
    }
}

// 2-D branch: data gradient of conv2d (w [9][Cin][Cout]); dx [B][D1][D2][Cin], dy [B][O1][O2][Cout]
__global__ void __launch_bounds__(256) conv2d_dgrad_kernel(float* __restrict__ dx, const float* __restrict__ dy,
                                                           const float* __restrict__ w, int B, int D1, int D2, int Cin, int Cout,
                                                           int pad) {
    const int O1 = D1 + 2 * pad - 2, O2 = D2 + 2 * pad - 2;
    const long long total = (long long)B * D1 * D2 * Cin;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % Cin);
    long long v = i / Cin;
    const int j2 = (int)(v % D2); v /= D2;
    const int j1 = (int)(v % D1);
    const int b = (int)(v / D1);
    float acc = 0.f;
    for (int d1 = 0; d1 < 3; ++d1)
        for (int d2 = 0; d2 < 3; ++d2) {
            const int o1 = j1 - d1 + pad, o2 = j2 - d2 + pad;
            if ((unsigned)o1 < (unsigned)O1 && (unsigned)o2 < (unsigned)O2) {
                const float* gp = dy + (((long long)b * O1 + o1) * O2 + o2) * Cout;
                const float* wp = w + ((d1 * 3 + d2) * Cin + k) * Cout;
                for (int c = 0; c < Cout; ++c) acc = fmaf(gp[c], wp[c], acc);
            }
        }
    dx[i] = acc;
}

// 2-D branch weight gradient: slab[blk][9*Cin*Cout + Cout]; block = a range of output pixels, thread = output entries
__global__ void __launch_bounds__(256) conv2d_wgrad_kernel(float* __restrict__ slab, const float* __restrict__ x,
                                                           const float* __restrict__ dy, int B, int D1, int D2, int Cin, int Cout,
                                                           int pad, long long pix_per_block) {
    const int O1 = D1 + 2 * pad - 2, O2 = D2 + 2 * pad - 2;
    const long long npix = (long long)B * O1 * O2;
    const long long p0 = (long long)blockIdx.x * pix_per_block, p1 = min(npix, p0 + pix_per_block);
    const int nw = 9 * Cin * Cout, nout = nw + Cout;
    for (int e = threadIdx.x; e < nout; e += 256) {
        float acc = 0.f;
        if (e < nw) {
            const int c = e % Cout, k = (e / Cout) % Cin, tap = e / (Cout * Cin);
            const int d1 = tap / 3, d2 = tap % 3;
            // (the pixel's coordinates walk along with p: three 64-bit divisions per pixel and element were most of the kernel's time)
            int o2 = (int)(p0 % O2), o1 = (int)((p0 / O2) % O1), b = (int)(p0 / ((long long)O1 * O2));
            for (long long p = p0; p < p1; ++p) {
                const int j1 = o1 + d1 - pad, j2 = o2 + d2 - pad;
                if ((unsigned)j1 < (unsigned)D1 && (unsigned)j2 < (unsigned)D2)
                    acc = fmaf(x[(((long long)b * D1 + j1) * D2 + j2) * Cin + k], dy[p * Cout + c], acc);
                if (++o2 == O2) {
                    o2 = 0;
                    if (++o1 == O1) {
                        o1 = 0;
                        ++b;
                    }
                }
            }
        } else {
            const int c = e - nw;
            for (long long p = p0; p < p1; ++p) acc += dy[p * Cout + c];
        }
        slab[(long long)blockIdx.x * nout + e] = acc;
    }
}

// backward of depth_to_space + denormalise: dup[b][h][w][i*s + j] = dout[b][s*h + i][s*w + j] * STD
__global__ void __launch_bounds__(256) shuffle_backward_kernel(float* __restrict__ dup, const float* __restrict__ dout, int B, int H,
                                                               int W, int s, float stdv) {
    const long long total = (long long)B * H * W * s * s;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % (s * s));
    long long v = i / (s * s);
    const int w = (int)(v % W); v /= W;
    const int h = (int)(v % H);
    const int b = (int)(v / H);
    dup[i] = dout[((long long)b * H * s + h * s + k / s) * (W * s) + w * s + k % s] * stdv;
}

// de-normalised, un-clipped prediction (what the loss sees): out = (up + glob) * STD + MEAN after depth_to_space
// = shuffle_sum_kernel with clip_round = 0 (rams.hip)

// ---- workspace of one training step --------------------------------------------------------------------------------------------
struct TrainDims {
    int B, H, W, T, N, S2, Cr, Tr;
    long long V;        // floats of a trunk activation [B][H+2][W+2][T][32]
    long long Vp;       // floats of the largest padded activation [B][H+4][W+4][T][32]
};
static TrainDims train_dims(const inr_rams_desc_t* d, int B, int H, int W) {
    TrainDims t;
    t.B = B; t.H = H; t.W = W; t.T = d->channels; t.N = d->n_rfab; t.S2 = d->scale * d->scale;
    t.Cr = d->filters / d->r; t.Tr = t.T / d->r > 0 ? t.T / d->r : 1;
    t.V = (long long)B * (H + 2) * (W + 2) * t.T * RC;
    t.Vp = (long long)B * (H + 4) * (W + 4) * t.T * RC;
    return t;
}

// per-channel partial sums: the convolution epilogue writes [B][waves_per_b][32], the gate backward [B][64][32]
static long long train_slab_floats(int B, int H, int W, int T) { return rams_slab_floats(B, (H + 4) * (W + 4) * T); }

// Every region of a step's workspace, in the order the step first touches them (forward, loss, backward), each on a 256-byte
// boundary.  Sizes depend on (d, B, H, W) alone, so the whole carve is known -- and checked against the caller's byte count --
// before the first launch.  base == null: `total` only.
struct RamsTrainView {
    std::vector<TLayer> L;                 // the layer table the regions are sized from
    long long raw_total, fold_total;
    struct Block { float *pin, *r1, *c2, *out, *gate, *mean, *sq; };   // one attention block; pin: the reduction stages' padded input
    float *fold, *gfold;                   // folded parameters and their gradients
    float *xn, *xpad, *a0;
    float *wgrad_ws, *slab, *gpart, *dpool;
    unsigned *wslots, *tslots;             // max|w| (forward k, data gradient n_conv3 + k); n_tslots slots of R3_SLOT words
    int n_conv3, n_tslots;
    _Float16* planes;
    float* zero_bias;
    std::vector<Block> blk;                // N trunk blocks, then T / 3 reduction stages
    float* tr;
    std::vector<float*> red_out;
    float *upo, *g1, *g2, *g3, *ggate, *gmean, *gsq, *glo, *pred, *dpred;
    double* lws;
    float *dA, *dB, *tmp, *tmp2, *dps, *keep, *dg1, *chain;
    size_t total;                          // bytes
};
static RamsTrainView rams_train_view(const inr_rams_desc_t* d, int B, int H, int W, void* base) {
    const TrainDims t = train_dims(d, B, H, W);
    const int T = t.T, nred = T / 3, D1 = H + 2, D2 = W + 2;
    const long long n_pad = (long long)B * D1 * D2 * T, n_hw = (long long)B * H * W;
    RamsTrainView v;
    rams_train_layers(d, v.L, &v.raw_total, &v.fold_total);
    WsCarver c(base, 256);
    auto f = [&](long long n) { return c.take<float>((size_t)n); };
    v.fold = f(v.fold_total); v.gfold = f(v.fold_total);
    f((long long)v.L.size() * (sizeof(FoldLayer) / 4 + 1));   // (round 3's device copy of the layer table: the workspace layout is kept)
    v.xn = f((long long)B * H * W * T); v.xpad = f(n_pad); v.a0 = f(t.V);
    v.wgrad_ws = f((long long)rams_conv3d_wgrad_ws_floats((long long)B * (H + 4) * (W + 4) * T));
    v.slab = f(train_slab_floats(B, H, W, T)); v.gpart = f((long long)B * 1024); v.dpool = f((long long)B * RC);
    // split-fp16 state of the 32 -> 32 convolutions; the max|w| words start on a 256-byte ADDRESS inside a region 64 words longer
    v.n_conv3 = rams_conv3d_count(d);
    v.n_tslots = 2 * v.n_conv3 + 4 * (t.N + nred) + 16;
    v.wslots = c.take<unsigned>(1024 + 64);
    v.wslots = reinterpret_cast<unsigned*>(round_up(reinterpret_cast<uintptr_t>(v.wslots), 256));
    v.tslots = c.take<unsigned>((size_t)v.n_tslots * R3_SLOT);
    v.planes = c.take<_Float16>(2 * (size_t)v.n_conv3 * R3_LAYER_HALVES);
    v.zero_bias = f(RC);
    v.blk.resize(t.N + nred);
    for (int i = 0; i < t.N; ++i) v.blk[i] = {nullptr, f(t.V), f(t.V), f(t.V), f(B * RC), f(B * RC), f(B * 8)};
    v.tr = f(t.V);
    v.red_out.resize(nred);
    for (int j = 0, D3 = T; j < nred; ++j, D3 -= 2) {
        const long long vp = (long long)B * (D1 + 2) * (D2 + 2) * D3 * RC;
        v.blk[t.N + j] = {f(vp), f(vp), f(vp), f(vp), f(B * RC), f(B * RC), f(B * 8)};
        v.red_out[j] = f((long long)B * D1 * D2 * (D3 - 2) * RC);
    }
    v.upo = f(n_hw * t.S2);
    v.g1 = f(n_pad); v.g2 = f(n_pad); v.g3 = f(n_pad);
    v.ggate = f(B * RC); v.gmean = f(B * RC); v.gsq = f(B * 8);
    v.glo = f(n_hw * t.S2); v.pred = f(n_hw * t.S2); v.dpred = f(n_hw * t.S2);
    v.lws = c.take<double>((size_t)B * 49 + B + 8);
    v.dA = f(t.Vp); v.dB = f(t.Vp); v.tmp = f(t.Vp); v.tmp2 = f(t.Vp);
    v.dps = f(n_hw * t.S2);      // gradient of both pixel-shuffled heads
    v.keep = f(n_pad); v.dg1 = f(n_pad);
    v.chain = f(t.V);
    v.total = c.bytes();
    return v;
}

static size_t rams_train_workspace_floats(const inr_rams_desc_t* d, int B, int H, int W) {
    return rams_train_view(d, B, H, W, nullptr).total / sizeof(float);
}

// ---- the step ---------------------------------------------------------------------------------------------------------------------
// One forward + loss + backward.  raw: parameters (raw layout); raw_grad: receives d(sum_b loss_b)/d raw.  loss: [B] doubles.
// pred (nullable): receives the un-clipped prediction [B][sH][sW].
static int rams_train_grads(const inr_rams_desc_t* d, const float* raw, float* raw_grad, const float* x, const float* y_true,
                            const float* mask, double* loss, float* pred_out, int B, int H, int W, void* workspace, size_t workspace_bytes,
                            hipStream_t st) {
    const TrainDims t = train_dims(d, B, H, W);
    const int T = t.T, Cr = t.Cr, Tr = t.Tr, S2 = t.S2, s = d->scale, nred = T / 3;
    INR_REQUIRE(d->filters == RC && d->kernel_size == 3 && T == 9 && s * s <= RC, INR_E_INVALID,
                "rams train: filters must be 32, kernel 3, channels 9");
    const RamsTrainView v = rams_train_view(d, B, H, W, workspace);
    const std::vector<TLayer>& L = v.L;
    const long long raw_total = v.raw_total, fold_total = v.fold_total;
    INR_REQUIRE(workspace && workspace_bytes >= v.total, INR_E_WORKSPACE, "inr_rams_train_grads: workspace too small");
    INR_REQUIRE(aligned16(workspace) && aligned16(raw) && aligned16(raw_grad), INR_E_ALIGN,
                "inr_rams_train_grads: params / grads / workspace must be 16-byte aligned");
    // the regions, under the names the step has always used
    float *const fold = v.fold, *const gfold = v.gfold, *const xn = v.xn, *const xpad = v.xpad, *const a0 = v.a0, *const wgrad_ws = v.wgrad_ws,
          *const slab = v.slab, *const gpart = v.gpart, *const dpool = v.dpool, *const zero_bias = v.zero_bias, *const tr = v.tr,
          *const upo = v.upo, *const g1 = v.g1, *const g2 = v.g2, *const g3 = v.g3, *const ggate = v.ggate, *const gmean = v.gmean,
          *const gsq = v.gsq, *const glo = v.glo, *const pred = v.pred, *const dpred = v.dpred, *const dA = v.dA, *const dB = v.dB,
          *const tmp = v.tmp, *const tmp2 = v.tmp2, *const dps = v.dps, *const keep = v.keep, *const dg1 = v.dg1, *const chain = v.chain;
    FoldTable dl{};
    INR_REQUIRE(L.size() <= (size_t)FOLD_MAX_LAYERS && raw_total < (1ll << 31) && fold_total < (1ll << 31), INR_E_INVALID,
                "rams train: %zu layers / %lld parameters exceed the by-value layer table", L.size(), raw_total);
    for (size_t i = 0; i < L.size(); ++i) {
        INR_REQUIRE(L[i].rows < 65536 && L[i].cout < 256 && L[i].fcout < 256, INR_E_INVALID, "rams train: layer %zu too large", i);
        dl.l[i] = FoldLayerC{(unsigned short)L[i].rows, (unsigned char)L[i].cout, (unsigned char)L[i].fcout, (int)L[i].v, (int)L[i].g,
                             (int)L[i].b, (int)L[i].fw, (int)L[i].fb};
    }
    ProfScope ps(KC_OTHER, st);
    const FoldJobs J{raw, raw_grad, fold, (int)L.size()};
    hipLaunchKernelGGL(fold_kernel, dim3((unsigned)L.size()), dim3(256), 0, st, J, dl);
    INR_LAUNCH_CHECK();
    INR_HIP(hipMemsetAsync(gfold, 0, (size_t)fold_total * 4, st));

    const int D1 = H + 2, D2 = W + 2;
    const long long n_in = (long long)B * H * W * T, n_pad = (long long)B * D1 * D2 * T;
    struct Rfab { float *in, *r1, *c2, *out, *gate, *mean, *sq; int D1, D2, D3; int l0; unsigned* out_slot = nullptr; };
    std::vector<Rfab> R(t.N + nred);

    // ---- split-fp16 state of the 32 -> 32 convolutions (forward and data gradient; debug key 14 = 0 keeps the f32-input kernels) ----
    const bool h3 = g_rams_h3 != 0;
    const int n_conv3 = v.n_conv3;
    INR_REQUIRE(2 * n_conv3 <= R3_MAX_CONVS, INR_E_INVALID, "rams train: too many 3-D convolutions (%d)", n_conv3);
    unsigned* const wslots = v.wslots;              // max|w|: forward k, data gradient n_conv3 + k
    // max|x| of each call's input: slots k / n_conv3 + k belong to forward / gradient call k (filled by a pass over the tensor when
    // nothing better is known), the rest to tensors whose PRODUCER records the maximum (convolution epilogues, the gated residual,
    // the ReLU and gate backward kernels): 63 of the 74 passes of a step are not needed
    const int n_tslots = v.n_tslots;
    unsigned* const tslots = v.tslots;
    int next_slot = 2 * n_conv3;
    auto new_slot = [&]() -> unsigned* {
        if (!h3 || next_slot >= n_tslots) return nullptr;      // (nullptr: the consumer measures the tensor itself)
        return tslots + (long long)(next_slot++) * R3_SLOT;
    };
    std::vector<const unsigned*> xslot_of((size_t)n_conv3, nullptr);     // the slot a forward call used: its weight gradient reads it
    _Float16* const planes = v.planes;
    std::vector<int> conv3_of(L.size(), -1);       // layer -> index among the 32 -> 32 convolutions
    int last_nslab = 0;                             // per-batch-element channel-sum slabs the last forward convolution wrote
    if (h3) {
        R3SplitJobs jobs{};
        int k = 0;
        for (size_t i = 1; i < L.size(); ++i)
            if (L[i].rows == 27 * RC) {
                conv3_of[i] = k;
                jobs.j[k] = {fold + L[i].fw, planes + (long long)k * R3_LAYER_HALVES, wslots + k, 0};
                jobs.j[n_conv3 + k] = {fold + L[i].fw, planes + (long long)(n_conv3 + k) * R3_LAYER_HALVES, wslots + n_conv3 + k, 1};
                ++k;
            }
        INR_REQUIRE(k == n_conv3, INR_E_INVALID, "rams train: %d 3-D convolutions found, %d expected", k, n_conv3);
        INR_HIP(hipMemsetAsync(tslots, 0, (size_t)n_tslots * R3_SLOT * sizeof(unsigned), st));
        INR_HIP(hipMemsetAsync(zero_bias, 0, RC * sizeof(float), st));
        hipLaunchKernelGGL(rams_weight_split_all_kernel, dim3(2 * n_conv3), dim3(512), 0, st, jobs);   // (after fold_kernel: same stream)
        INR_LAUNCH_CHECK();
    }
    auto amax_into = [&](unsigned* slot, const float* x, long long n) {
        const long long n4 = n / 4;
        long long g = (n4 + 255) / 256;
        if (g > 2048) g = 2048;
        hipLaunchKernelGGL(r3_tensor_amax_kernel, dim3((unsigned)g), dim3(256), 0, st, slot, x, n4);
    };
    // xs_known: slot that already holds max|in| (nullptr: measure it); ys: slot that receives max|out| (nullable)
    auto conv = [&](const float* in, float* out, int l, int d1, int d2, int d3, int pad, int relu, float* chan_slab, int cout,
                    int cstride, const unsigned* xs_known = nullptr, unsigned* ys = nullptr) -> int {
        const int ovox = (d1 + 2 * pad - 2) * (d2 + 2 * pad - 2) * (d3 + 2 * pad - 2);
        last_nslab = rams_waves_per_b(B, ovox);
        if (h3 && conv3_of[l] >= 0 && r3l_fits(d1, d2, d3)) {
            const int k = conv3_of[l];
            const unsigned* xs = xs_known;
            if (!xs) {
                unsigned* own = tslots + (long long)k * R3_SLOT;
                amax_into(own, in, (long long)B * d1 * d2 * d3 * RC);
                INR_LAUNCH_CHECK();
                xs = own;
            }
            xslot_of[k] = xs;
            return conv3d_h3_lds(in, out, planes + (long long)k * R3_LAYER_HALVES, fold + L[l].fb, chan_slab, xs, wslots + k, ys, B,
                                 d1, d2, d3, pad, cout, cstride, relu, &last_nslab, st, train_slab_floats(B, H, W, T));
        }
        if (ys) {                                          // (f32-input kernel: it does not record max|out|)
            const int rc = conv3d_mfma(in, out, fold + L[l].fw, fold + L[l].fb, chan_slab, B, d1, d2, d3, pad, cout, cstride, relu,
                                       last_nslab, st);
            if (rc) return rc;
            amax_into(ys, out, (long long)B * ovox * cstride);
            INR_LAUNCH_CHECK();
            return 0;
        }
        return conv3d_mfma(in, out, fold + L[l].fw, fold + L[l].fb, chan_slab, B, d1, d2, d3, pad, cout, cstride, relu, last_nslab,
                           st);
    };
    // forward of one attention block on `in` (layers l0 .. l0+3), everything kept
    auto rfab_fwd = [&](Rfab& r, const unsigned* in_slot) -> int {
        const int ovox = r.D1 * r.D2 * r.D3;
        unsigned* r1_slot = new_slot();
        if (int rc = conv(r.in, r.r1, r.l0, r.D1, r.D2, r.D3, 1, 1, nullptr, RC, RC, in_slot, r1_slot)) return rc;
        if (int rc = conv(r.r1, r.c2, r.l0 + 1, r.D1, r.D2, r.D3, 1, 0, slab, RC, RC, r1_slot)) return rc;
        hipLaunchKernelGGL(gate_train_kernel, dim3(B), dim3(256), 0, st, r.gate, r.mean, r.sq, slab, last_nslab, 1.0f / (float)ovox,
                           fold + L[r.l0 + 2].fw, fold + L[r.l0 + 2].fb, fold + L[r.l0 + 3].fw, fold + L[r.l0 + 3].fb, RC, Cr);
        INR_LAUNCH_CHECK();
        const long long total = (long long)B * ovox * RC;
        r.out_slot = new_slot();
        hipLaunchKernelGGL(scale_residual_kernel, dim3(nblk_capped(total / 4 + 1)), dim3(256), 0, st, r.out, r.c2, r.gate, r.in, (long long)ovox,
                           RC, total, r.out_slot);
        INR_LAUNCH_CHECK();
        return 0;
    };

    // ---- forward ----------------------------------------------------------------------------------------------------------------
    hipLaunchKernelGGL(normalize_kernel, dim3(nblk(n_in)), dim3(256), 0, st, xn, x, n_in, d->mean, d->std);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(reflect_pad_kernel, dim3(nblk(n_pad)), dim3(256), 0, st, xpad, xn, B, H, W, T);
    INR_LAUNCH_CHECK();
    const unsigned* cur_slot = new_slot();                 // max|.| of `cur`, recorded by its producer (nullptr: unknown)
    // (four output channels per thread -- and a whole depth row per thread at the depths the network uses --, the taps in the same
    //  order: the bits of conv3d_c1_kernel)
    if (((reinterpret_cast<uintptr_t>(a0) | reinterpret_cast<uintptr_t>(fold + L[0].fw) | reinterpret_cast<uintptr_t>(fold + L[0].fb)) & 15) == 0)
        launch_stem(a0, xpad, fold + L[0].fw, fold + L[0].fb, B, D1, D2, T, const_cast<unsigned*>(cur_slot), nullptr, st);
    else
        hipLaunchKernelGGL(conv3d_c1_kernel, dim3(nblk(t.V)), dim3(256), 0, st, a0, xpad, fold + L[0].fw, fold + L[0].fb, B, D1, D2, T,
                           const_cast<unsigned*>(cur_slot));
    INR_LAUNCH_CHECK();
    int l = 1;
    float* cur = a0;
    for (int i = 0; i < t.N; ++i) {
        Rfab& r = R[i];
        const RamsTrainView::Block& k = v.blk[i];
        r = Rfab{cur, k.r1, k.c2, k.out, k.gate, k.mean, k.sq, D1, D2, T, l};
        if (int rc = rfab_fwd(r, cur_slot)) return rc;
        cur = r.out;
        cur_slot = r.out_slot;
        l += 4;
    }
    const int l_trunk = l++;
    if (int rc = conv(cur, tr, l_trunk, D1, D2, T, 1, 0, nullptr, RC, RC, cur_slot)) return rc;
    hipLaunchKernelGGL(accumulate_kernel, dim3(nblk(t.V)), dim3(256), 0, st, tr, a0, t.V);   // + long skip (network.py:129)
    INR_LAUNCH_CHECK();
    const float* trunk_in = cur;
    cur = tr;
    cur_slot = nullptr;                                    // (conv + skip: measured by its consumer)
    int D3 = T;
    const std::vector<float*>& red_out = v.red_out;
    std::vector<int> red_conv(nred);
    for (int j = 0; j < nred; ++j) {
        Rfab& r = R[t.N + j];
        const RamsTrainView::Block& k = v.blk[t.N + j];
        float* const pin = k.pin;
        hipLaunchKernelGGL(reflect_pad_v4_kernel, dim3((D1 + 2) * (D2 + 2), B), dim3(256), 0, st, pin, cur, D1, D2, D3 * RC / 4);
        INR_LAUNCH_CHECK();
        r = Rfab{pin, k.r1, k.c2, k.out, k.gate, k.mean, k.sq, D1 + 2, D2 + 2, D3, l};
        if (int rc = rfab_fwd(r, cur_slot)) return rc;     // (reflect padding repeats samples: the maximum is that of `cur`)
        l += 4;
        red_conv[j] = l++;
        unsigned* ro_slot = new_slot();
        if (int rc = conv(r.out, red_out[j], red_conv[j], D1 + 2, D2 + 2, D3, 0, 1, nullptr, RC, RC, r.out_slot, ro_slot)) return rc;
        cur = red_out[j];
        cur_slot = ro_slot;
        D3 -= 2;
    }
    INR_REQUIRE(D3 == 3, INR_E_INVALID, "rams train: temporal depth before the head must be 3 (got %d)", D3);
    const int l_up = l++;
    const long long n_hw = (long long)B * H * W;
    if (int rc = conv(cur, upo, l_up, D1, D2, 3, 0, 0, nullptr, S2, S2, cur_slot)) return rc;
    const float* up_in = cur;
    // global path (network.py:144-148)
    const int l_g = l;   // rtab conv1, conv2, squeeze, excite, global
    const int nb2 = 64;
    launch_conv2d(g1, xpad, fold + L[l_g].fw, fold + L[l_g].fb, B, D1, D2, T, T, 1, 1, st);
    INR_LAUNCH_CHECK();
    launch_conv2d(g2, g1, fold + L[l_g + 1].fw, fold + L[l_g + 1].fb, B, D1, D2, T, T, 1, 0, st);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(chan_partial_kernel, dim3(nb2, B), dim3(256), 0, st, slab, g2, (long long)D1 * D2, T, nb2);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(gate_train_kernel, dim3(B), dim3(256), 0, st, ggate, gmean, gsq, slab, nb2, 1.0f / (float)(D1 * D2),
                       fold + L[l_g + 2].fw, fold + L[l_g + 2].fb, fold + L[l_g + 3].fw, fold + L[l_g + 3].fb, T, Tr);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(scale_residual_kernel, dim3(nblk(n_pad)), dim3(256), 0, st, g3, g2, ggate, xpad, (long long)D1 * D2, T, n_pad);
    INR_LAUNCH_CHECK();
    launch_conv2d(glo, g3, fold + L[l_g + 4].fw, fold + L[l_g + 4].fb, B, D1, D2, T, S2, 0, 0, st);
    INR_LAUNCH_CHECK();
    const long long n_out = n_hw * S2;
    hipLaunchKernelGGL(shuffle_sum_kernel, dim3(nblk(n_out)), dim3(256), 0, st, pred, upo, glo, B, H, W, s, d->mean, d->std, 0);
    INR_LAUNCH_CHECK();
    if (pred_out) INR_HIP(hipMemcpyAsync(pred_out, pred, (size_t)n_out * 4, hipMemcpyDeviceToDevice, st));

    // ---- loss and its gradient (utils/loss.py:26-75; tape.gradient of the per-image vector = gradient of its sum) --------------
    if (int rc = launch_shift_loss_grad(loss, dpred, y_true, pred, mask, nullptr, B, H * s, 3, v.lws, st)) return rc;

    // ---- backward ---------------------------------------------------------------------------------------------------------------
    hipLaunchKernelGGL(shuffle_backward_kernel, dim3(nblk(n_out)), dim3(256), 0, st, dps, dpred, B, H, W, s, d->std);
    INR_LAUNCH_CHECK();
    // weight gradient of a 32 -> 32 convolution: split-fp16 (default) needs max|x| -- the slot its forward call filled -- and max|dy|
    // -- the slot of the layer's data-gradient call, which follows on the same (or an equally valued, zero-padded) tensor
    std::vector<const float*> dy_amax_of(2 * (size_t)n_conv3, nullptr);
    // dy_known: slot that already holds max|dy| (recorded by the kernel that produced dy); nullptr: measure it
    auto wgrad3 = [&](int lyr, const float* xin, const float* dy, int d1, int d2, int d3, int pad, const unsigned* dy_known = nullptr) -> int {
        if (h3 && g_rams_h3 == 2 && conv3_of[lyr] >= 0 && r3l_fits(d1, d2, d3) && B <= WGRAD_BLOCKS_MAX) {
            const int k = conv3_of[lyr];
            const unsigned* ds = dy_known;
            if (!ds) {
                unsigned* own = tslots + (long long)(n_conv3 + k) * R3_SLOT;
                const int o1 = d1 + 2 * pad - 2, o2 = d2 + 2 * pad - 2, o3 = d3 + 2 * pad - 2;
                amax_into(own, dy, (long long)B * o1 * o2 * o3 * RC);
                INR_LAUNCH_CHECK();
                dy_amax_of[n_conv3 + k] = dy;
                ds = own;
            }
            const unsigned* xs = xslot_of[k];                 // what the forward call of this layer used
            if (!xs) {                                        // (the forward ran on the f32-input kernel: not reachable with one key value per step)
                unsigned* own = tslots + (long long)k * R3_SLOT;
                amax_into(own, xin, (long long)B * d1 * d2 * d3 * RC);
                INR_LAUNCH_CHECK();
                xs = own;
            }
            return rams_conv3d_wgrad_h3(gfold + L[lyr].fw, gfold + L[lyr].fb, xin, dy, xs, ds, B, d1, d2, d3, pad, wgrad_ws, st);
        }
        return rams_conv3d_wgrad(gfold + L[lyr].fw, gfold + L[lyr].fb, xin, dy, B, d1, d2, d3, pad, wgrad_ws, st);
    };
    // aux_mode (rams_h3.inc, AUX): 1 = dx = conv + aux (aux may be dx), 2 = dx = aux > 0 ? conv : 0 with max|dx| into `dx_slot`;
    // *fused says whether the convolution took the operand -- if not, the caller runs the separate pass
    auto dgrad3_takes_aux = [&](int lyr, int d1, int d2, int d3) { return h3 && conv3_of[lyr] >= 0 && r3l_fits(d1, d2, d3) && rams_lds_aux_ok(); };
    auto dgrad3 = [&](float* dx, const float* dy, int lyr, int d1, int d2, int d3, const unsigned* dy_known = nullptr,
                      const float* aux = nullptr, int aux_mode = 0, unsigned* dx_slot = nullptr, bool* fused = nullptr) -> int {
        if (fused) *fused = false;
        if (h3 && conv3_of[lyr] >= 0 && r3l_fits(d1, d2, d3)) {     // 'same' convolution of dy with the flipped kernel, split-fp16
            const int k = n_conv3 + conv3_of[lyr];
            const unsigned* xs = dy_known;
            if (!xs) {
                unsigned* own = tslots + (long long)k * R3_SLOT;
                if (dy_amax_of[k] != dy) {                   // (the weight-gradient call measured this very tensor already)
                    amax_into(own, dy, (long long)B * d1 * d2 * d3 * RC);
                    INR_LAUNCH_CHECK();
                }
                xs = own;
            }
            const bool with_aux = aux_mode != 0 && dgrad3_takes_aux(lyr, d1, d2, d3);
            if (fused) *fused = with_aux;
            // (Measured and dropped: the residual-sum convolution also forming the channel dot products of the NEXT block's gate backward
            //  -- sixteen more loads per tile in its epilogue cost what the 15 us pass saved: 9.39 against 9.35 ms per step.)
            return conv3d_h3_lds(dy, dx, planes + (long long)k * R3_LAYER_HALVES, zero_bias, nullptr, xs, wslots + k,
                                 with_aux ? dx_slot : nullptr, B, d1, d2, d3, 1, RC, RC, 0, nullptr, st, -1, with_aux ? aux : nullptr,
                                 with_aux ? aux_mode : 0);
        }
        return rams_conv3d_dgrad_same(dx, dy, fold + L[lyr].fw, B, d1, d2, d3, wgrad_ws, st);
    };
    // reduce per-batch-element partials [B][len] into out[len]
    auto reduce_b = [&](float* out, const float* parts, long long len, long long stride) -> int {
        // (partials of one field sit `stride` floats apart: the reduction reads them in place -- compacting them first took 2,060
        // copy launches per step at batch 32, 15 % of the step)
        return launch_reduce_slabs_pitched(out, parts, B, len, stride, tmp2, st);
    };
    // backward of the gate (2-D or 3-D): from dout (gradient of y * gate + res) and y -> dy (into `dy_out`), gate weight gradients
    auto gate_bwd = [&](float* dy_out, const float* dout, const float* y, const float* gate, const float* mean, const float* sq,
                        int l_sq, long long per_b, int C, int Cg, unsigned* dy_slot = nullptr) -> int {
        const int nb = 64;
        hipLaunchKernelGGL(chan_dot_partial_kernel, dim3(nb, B), dim3(256), 0, st, slab, dout, y, per_b, C, nb);
        INR_LAUNCH_CHECK();
        const long long o_bsq = pad4((long long)C * Cg), o_wex = o_bsq + pad4(Cg), o_bex = o_wex + pad4((long long)Cg * C);
        const long long gstride = o_bex + pad4(C);
        hipLaunchKernelGGL(gate_backward_kernel, dim3(B), dim3(64), 0, st, gpart, dpool, slab, nb, gate, mean, sq, fold + L[l_sq].fw,
                           fold + L[l_sq + 1].fw, C, Cg, 1.0f / (float)per_b, gstride);
        INR_LAUNCH_CHECK();
        // the four partial fields of a batch element (squeeze W, b; excite W, b) are packed exactly like the folded gradients of the
        // two layers (fw, fb, fw, fb, each padded to four floats): ONE reduction of the whole row where that holds
        if (L[l_sq].fb == L[l_sq].fw + o_bsq && L[l_sq + 1].fw == L[l_sq].fw + o_wex && L[l_sq + 1].fb == L[l_sq].fw + o_bex) {
            if (int rc = reduce_b(gfold + L[l_sq].fw, gpart, gstride, gstride)) return rc;
        } else {
            if (int rc = reduce_b(gfold + L[l_sq].fw, gpart, (long long)C * Cg, gstride)) return rc;
            if (int rc = reduce_b(gfold + L[l_sq].fb, gpart + o_bsq, Cg, gstride)) return rc;
            if (int rc = reduce_b(gfold + L[l_sq + 1].fw, gpart + o_wex, (long long)Cg * C, gstride)) return rc;
            if (int rc = reduce_b(gfold + L[l_sq + 1].fb, gpart + o_bex, C, gstride)) return rc;
        }
        const long long total = (long long)B * per_b * C;
        hipLaunchKernelGGL(gate_apply_backward_kernel, dim3(nblk_capped(total / 4 + 1)), dim3(256), 0, st, dy_out, dout, gate, dpool,
                           per_b, C, total, dy_slot);
        INR_LAUNCH_CHECK();
        return 0;
    };
    // backward of one attention block: dio holds d out on entry and d in on exit
    auto rfab_bwd = [&](const Rfab& r, float* dio) -> int {
        const long long per_b = (long long)r.D1 * r.D2 * r.D3, total = (long long)B * per_b * RC;
        unsigned* s_c2 = new_slot();                       // (fresh slots, zeroed with all others at the start of the step)
        unsigned* s_r1 = new_slot();
        if (int rc = gate_bwd(tmp, dio, r.c2, r.gate, r.mean, r.sq, r.l0 + 2, per_b, RC, Cr, s_c2)) return rc;  // tmp = d c2
        if (int rc = wgrad3(r.l0 + 1, r.r1, tmp, r.D1, r.D2, r.D3, 1, s_c2)) return rc;
        bool fused = false;                                                                                    // tmp2 = d r1, ReLU-masked
        if (int rc = dgrad3(tmp2, tmp, r.l0 + 1, r.D1, r.D2, r.D3, s_c2, r.r1, 2, s_r1, &fused)) return rc;
        if (!fused) {
            hipLaunchKernelGGL(relu_backward_kernel, dim3(nblk_capped(total / 4 + 1)), dim3(256), 0, st, tmp2, r.r1, total, s_r1);
            INR_LAUNCH_CHECK();
        }
        if (int rc = wgrad3(r.l0, r.in, tmp2, r.D1, r.D2, r.D3, 1, s_r1)) return rc;
        const bool sum_in_place = dgrad3_takes_aux(r.l0, r.D1, r.D2, r.D3);      // then the convolution adds dio itself, in place
        if (int rc = dgrad3(sum_in_place ? dio : tmp, tmp2, r.l0, r.D1, r.D2, r.D3, s_r1, dio, 1, nullptr, &fused)) return rc;   // d in (conv path)
        if (!fused) {                                                                                          // + residual path
            hipLaunchKernelGGL(accumulate_kernel, dim3(nblk(total)), dim3(256), 0, st, dio, tmp, total);
            INR_LAUNCH_CHECK();
        }
        return 0;
    };

    // global path
    {
        auto wgrad2 = [&](int lyr, const float* xin, const float* dy, int cin, int cout, int pad) -> int {
            const int O1 = D1 + 2 * pad - 2, O2 = D2 + 2 * pad - 2;
            const long long npix = (long long)B * O1 * O2;
            const int nout = 9 * cin * cout + cout;
            // eight blocks per CU (the pixel loop is latency-bound: 152 us on 256 blocks); the slabs live in `tmp`, reduced in `tmp2`
            long long nblocks = 2048;
            if (nblocks > t.Vp / (2ll * nout)) nblocks = t.Vp / (2ll * nout);
            if (nblocks < 1) nblocks = 1;
            const long long ppb = (npix + nblocks - 1) / nblocks;
            const int nb = (int)((npix + ppb - 1) / ppb);
            hipLaunchKernelGGL(conv2d_wgrad_kernel, dim3(nb), dim3(256), 0, st, tmp, xin, dy, B, D1, D2, cin, cout, pad, ppb);
            INR_LAUNCH_CHECK();
            if (int rc = launch_reduce_slabs(tmp2, tmp, nb, nout, tmp2 + 4096, st)) return rc;
            INR_HIP(hipMemcpyAsync(gfold + L[lyr].fw, tmp2, (size_t)9 * cin * cout * 4, hipMemcpyDeviceToDevice, st));
            INR_HIP(hipMemcpyAsync(gfold + L[lyr].fb, tmp2 + 9 * cin * cout, (size_t)cout * 4, hipMemcpyDeviceToDevice, st));
            return 0;
        };
        float* dg3 = dA;
        if (int rc = wgrad2(l_g + 4, g3, dps, T, S2, 0)) return rc;
        hipLaunchKernelGGL(conv2d_dgrad_kernel, dim3(nblk(n_pad)), dim3(256), 0, st, dg3, dps, fold + L[l_g + 4].fw, B, D1, D2, T, S2, 0);
        INR_LAUNCH_CHECK();
        // (`keep`: d g2 must survive wgrad2's use of tmp / tmp2)
        if (int rc = gate_bwd(keep, dg3, g2, ggate, gmean, gsq, l_g + 2, (long long)D1 * D2, T, Tr)) return rc;
        if (int rc = wgrad2(l_g + 1, g1, keep, T, T, 1)) return rc;
        hipLaunchKernelGGL(conv2d_dgrad_kernel, dim3(nblk(n_pad)), dim3(256), 0, st, dg1, keep, fold + L[l_g + 1].fw, B, D1, D2, T, T, 1);
        INR_LAUNCH_CHECK();
        hipLaunchKernelGGL(relu_backward_kernel, dim3(nblk_capped(n_pad / 4 + 1)), dim3(256), 0, st, dg1, g1, n_pad);
        INR_LAUNCH_CHECK();
        if (int rc = wgrad2(l_g, xpad, dg1, T, T, 1)) return rc;
    }
    // up-scaling head: 'valid' 32 -> s^2 (stored 32-wide in the folded layout)
    {
        const long long nv = n_hw;   // output voxels [B][H][W][1]
        hipLaunchKernelGGL(widen_channels_kernel, dim3(nblk(nv * RC)), dim3(256), 0, st, tmp, dps, nv, S2, RC);
        INR_LAUNCH_CHECK();
        if (int rc = wgrad3(l_up, up_in, tmp, D1, D2, 3, 0)) return rc;
        const long long np = (long long)B * D1 * D2 * 3 * RC;
        hipLaunchKernelGGL(zero_pad3_kernel, dim3(nblk(np)), dim3(256), 0, st, tmp2, dps, B, H, W, 1, S2, RC);
        INR_LAUNCH_CHECK();
        if (int rc = dgrad3(dA, tmp2, l_up, D1, D2, 3)) return rc;     // dA = d (input of the head) [B][D1][D2][3][32]
    }
    // temporal reduction stages, last to first
    int d3 = 3;
    for (int j = nred - 1; j >= 0; --j) {
        const Rfab& r = R[t.N + j];
        const int din3 = d3 + 2;   // depth of the stage's input
        const long long nout_v = (long long)B * D1 * D2 * d3 * RC;
        hipLaunchKernelGGL(relu_backward_kernel, dim3(nblk_capped(nout_v / 4 + 1)), dim3(256), 0, st, dA, red_out[j], nout_v);
        INR_LAUNCH_CHECK();
        if (int rc = wgrad3(red_conv[j], r.out, dA, D1 + 2, D2 + 2, din3, 0)) return rc;
        const long long np = (long long)B * (D1 + 2) * (D2 + 2) * din3 * RC;
        hipLaunchKernelGGL(zero_pad3_kernel, dim3(nblk(np)), dim3(256), 0, st, tmp2, dA, B, D1, D2, d3, RC, RC);
        INR_LAUNCH_CHECK();
        if (int rc = dgrad3(dB, tmp2, red_conv[j], D1 + 2, D2 + 2, din3)) return rc;    // dB = d (block output), padded dims
        if (int rc = rfab_bwd(r, dB)) return rc;                                       // dB = d (padded input)
        hipLaunchKernelGGL(reflect_pad_backward_v4_kernel, dim3(D1 * D2, B), dim3(256), 0, st, dA, dB, D1, D2, din3 * RC / 4);
        INR_LAUNCH_CHECK();
        d3 = din3;
    }
    // trunk close: a_t = conv(a_N) + a0
    // d a_t stays where it is and IS the long skip's gradient of a0; the chain through the blocks runs in a buffer of its own
    // (three device-to-device copies of the tensor stood here: d a_t aside, the convolution's result back over it, the copy again)
    float* const skip = dA;
    if (int rc = wgrad3(l_trunk, trunk_in, dA, D1, D2, T, 1)) return rc;
    if (int rc = dgrad3(chain, dA, l_trunk, D1, D2, T)) return rc;                       // chain = d a_N
    for (int i = t.N - 1; i >= 0; --i)
        if (int rc = rfab_bwd(R[i], chain)) return rc;
    hipLaunchKernelGGL(accumulate_kernel, dim3(nblk(t.V)), dim3(256), 0, st, chain, skip, t.V);   // d a0 = chain + skip
    INR_LAUNCH_CHECK();
    {   // stem
        const long long nvox = (long long)B * D1 * D2 * T;
        // eight blocks per CU: the loop is latency-bound (256 blocks: 0.56 ms of a 17 ms step); the slabs live in `tmp`
        long long nb = 2048;
        if (nb > t.Vp / (2 * 28 * 32)) nb = t.Vp / (2 * 28 * 32);
        if (nb < 1) nb = 1;
        const long long vpb = (nvox + nb - 1) / nb;
        const int nbb = (int)((nvox + vpb - 1) / vpb);
        INR_REQUIRE(nvox < (1ll << 31), INR_E_INVALID, "rams train: %lld voxels per batch exceed the stem gradient's 32-bit indices", nvox);
        INR_REQUIRE(T + 2 <= STEM_TP, INR_E_INVALID, "rams train: %d images per stack exceed the stem gradient's staged depth", T);
        hipLaunchKernelGGL(stem_wgrad_kernel, dim3(nbb), dim3(256), 0, st, tmp, xpad, chain, B, D1, D2, T, vpb);
        INR_LAUNCH_CHECK();
        if (int rc = launch_reduce_slabs(tmp2, tmp, nbb, 28 * 32, tmp2 + 4096, st)) return rc;
        INR_HIP(hipMemcpyAsync(gfold + L[0].fw, tmp2, 27 * 32 * 4, hipMemcpyDeviceToDevice, st));
        INR_HIP(hipMemcpyAsync(gfold + L[0].fb, tmp2 + 27 * 32, 32 * 4, hipMemcpyDeviceToDevice, st));
    }
    // un-fold: (dK, db) -> (dv, dg, db)
    const FoldJobs JB{raw, raw_grad, gfold, (int)L.size()};
    hipLaunchKernelGGL(fold_backward_kernel, dim3((unsigned)L.size()), dim3(256), 0, st, JB, dl);
    INR_LAUNCH_CHECK();
    return 0;
}

static long long rams_train_param_floats(const inr_rams_desc_t* d) {
    std::vector<TLayer> L;
    long long raw_total, fold_total;
    rams_train_layers(d, L, &raw_total, &fold_total);
    return raw_total;
}

// offsets[3 l .. 3 l + 2] = (v, g, b) of layer l; returns the number of layers (negative: buffer too small)
static int rams_train_param_offsets(const inr_rams_desc_t* d, int64_t* offsets, int max_layers) {
    std::vector<TLayer> L;
    long long raw_total, fold_total;
    rams_train_layers(d, L, &raw_total, &fold_total);
    INR_REQUIRE((int)L.size() <= max_layers, INR_E_INVALID, "rams: %d layers, room for %d", (int)L.size(), max_layers);
    for (size_t i = 0; i < L.size(); ++i) {
        offsets[3 * i] = L[i].v;
        offsets[3 * i + 1] = L[i].g;
        offsets[3 * i + 2] = L[i].b;
    }
    return (int)L.size();
}
