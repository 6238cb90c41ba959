// Weight gradient of the 32 -> 32 3x3x3 convolutions on split-fp16 MFMAs (included by rams.hip after rams_h3.inc).
//
//   gw[tap][ci][co] = sum_{b, v} x[b, v + tap - pad][ci] * dy[b, v][co]          (utils/training.py:193-209: tape.gradient)
//
// is a contraction over the VOXELS, the row index of both row-major operands.  The f32-input kernel (conv3d_c32_wgrad_kernel)
// does it with v_mfma_f32_32x32x2_f32 -- 64 cycles per 2 voxels and a VALU-shared issue port; here both operands are staged once
// per patch into LDS as fp16 hi/lo pairs (the patch geometry and the 144-byte voxel rows of conv3d_c32_lds_kernel: x with its
// halo, dy without) and v_mfma_f32_16x16x32_f16 contracts 32 voxels per instruction: 12 MFMAs (2 x 2 output tiles x the three
// products hi*lo, lo*hi, hi*hi) of 16 cycles per 32 voxels and tap, 5.3 x fewer matrix-core cycles.  The operand fragments
// (8 consecutive VOXELS of one channel per lane) come out of ds_read_b64_tr_b16: every lane names the LDS row of "its" voxel,
// so the 32 voxels of a k-step need not be evenly spaced in the halo image, and a tap outside the temporal range (or a row past
// the patch) names the zero block.
//
// A block (8 waves) walks patches; wave w owns taps w, w + 8, w + 16 (, w + 24): at most 16 accumulator tiles of 16 x 16, kept
// in registers over all its patches and written once: slab[block][27][32][32] (+ 32 floats), reduced in a fixed order by the caller.
// The bias gradient gb[co] = sum_v dy[v][co] rides along as a 28th "tap" whose x operand is the constant 1 (wave 3's idle slot:
// two more MFMAs per k-step): it saves the separate column-sum pass over dy per layer.
struct Conv3dWgradH3Params {
    const float* x;            // [B][D1][D2][D3][32]
    const float* dy;           // [B][O1][O2][O3][32]
    float* slab;               // [B * gridDim.x][W3_SLAB]: 27 x 32 x 32 partial gw, then 32 partial gb
    const unsigned* x_amax;    // slot (R3_SLOT words): max|x|
    const unsigned* dy_amax;   // slot: max|dy|
    int B, D1, D2, D3, O1, O2, O3, pad;
    int PO1, PO2, np1, np2;
    unsigned mD3, mHP2, mO3, mPO2, mNP2;
};

constexpr int W3_SLAB = 27 * RC * RC + RC;                     // floats per block: gw, then gb
constexpr int W3_XIMG = 256;                                   // zero block first
constexpr int W3_YIMG = W3_XIMG + R3L_MAX_HVOX * R3L_VOX_BYTES;
constexpr int W3_YVOX = 256;                                   // dy rows of a patch (8 k-steps of 32 voxels)
constexpr int W3_LDS = W3_YIMG + W3_YVOX * R3L_VOX_BYTES;

typedef unsigned int w3_u32x2 __attribute__((ext_vector_type(2)));
typedef float w3_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ w3_u32x2 w3_tr_read(unsigned addr) {      // (not counted in lgkmcnt by the compiler: see w3_wait8)
    w3_u32x2 r;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(addr) : "memory");     // (reads what split_store wrote)
    return r;
}
// every consumer of the eight transposed reads sits behind this wait (the operands travel through the asm, so no use can be
// scheduled in front of it)
__device__ __forceinline__ void w3_wait8(w3_u32x2 (&f)[8]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7]));
}
__device__ __forceinline__ half8 w3_frag(w3_u32x2 a, w3_u32x2 b) { return __builtin_bit_cast(half8, u32x4{a[0], a[1], b[0], b[1]}); }

__global__ void __launch_bounds__(512) conv3d_c32_wgrad_h3_kernel(const Conv3dWgradH3Params p) {
    constexpr int NT = 512;
    constexpr int XQ = (R3L_MAX_HVOX * 8 + NT - 1) / NT;       // 16-byte units of the x halo per thread
    constexpr int YQ = W3_YVOX * 8 / NT;                       // ... of the dy patch
    constexpr unsigned OOB = 0x40000000u;
    __shared__ __attribute__((aligned(16))) char lds[W3_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, l16 = lane & 15, qrow = l16 >> 2, p4 = l16 & 3;
    const int b = blockIdx.y;
    const int HP1 = p.PO1 + 2, HP2 = p.PO2 + 2;
    const int hvox = HP1 * HP2 * p.D3;
    const int pvox = p.PO1 * p.PO2 * p.O3;
    const int npatch = p.np1 * p.np2;
    if (tid < 64) reinterpret_cast<float*>(lds)[tid] = 0.f;
    const int ka = h3_scale_exp(r3_slot_max(p.x_amax)), kd = h3_scale_exp(r3_slot_max(p.dy_amax));
    const float sa = h3_pow2(ka), sd = h3_pow2(kd), ua = h3_pow2(-ka), ud = h3_pow2(-kd);
    const __amdgpu_buffer_rsrc_t xsrd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.x) + (long long)b * p.D1 * p.D2 * p.D3 * RC, 0, p.D1 * p.D2 * p.D3 * RC * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t ysrd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.dy) + (long long)b * p.O1 * p.O2 * p.O3 * RC, 0, p.O1 * p.O2 * p.O3 * RC * 4, 0x00020000);

    // ---- staging: the units of a thread sit at the same place of every patch -------------------------------------------------------
    unsigned x_rel[XQ], x_h12[XQ], y_rel[YQ], y_q12[YQ];
#pragma unroll
    for (int i = 0; i < XQ; ++i) {
        const int hv = (tid >> 3) + i * (NT / 8);
        const int hq = r3_div(hv, p.mD3), t = hv - hq * p.D3, h1 = r3_div(hq, p.mHP2), h2 = hq - h1 * HP2;
        x_rel[i] = hv < hvox ? (unsigned)(((h1 * p.D2 + h2) * p.D3 + t) * RC + 4 * (tid & 7)) * 4u : OOB;
        x_h12[i] = (unsigned)h1 | ((unsigned)h2 << 16);
    }
#pragma unroll
    for (int i = 0; i < YQ; ++i) {
        const int q = (tid >> 3) + i * (NT / 8);
        const int qq = r3_div(q, p.mO3), t = q - qq * p.O3, q1 = r3_div(qq, p.mPO2), q2 = qq - q1 * p.PO2;
        y_rel[i] = q < pvox ? (unsigned)(((q1 * p.O2 + q2) * p.O3 + t) * RC + 4 * (tid & 7)) * 4u : OOB;
        y_q12[i] = (unsigned)q1 | ((unsigned)q2 << 16);
    }
    const int dst0 = (tid >> 3) * R3L_VOX_BYTES + ((tid & 7) >> 1) * 16 + (tid & 1) * 8;
    auto split_store = [&](const f32x4 v, float s, char* at) __attribute__((always_inline)) {
        half2v h0, l0, h1, l1;
        h3_split2(v[0], v[1], s, h0, l0);
        h3_split2(v[2], v[3], s, h1, l1);
        *reinterpret_cast<uint2*>(at) = uint2{__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1)};
        *reinterpret_cast<uint2*>(at + 64) = uint2{__builtin_bit_cast(unsigned, l0), __builtin_bit_cast(unsigned, l1)};
    };

    // ---- accumulators: slot t = tap wave + 8 t; [ci tile][co tile] --------------------------------------------------------------------
    w3_f32x4 acc[4][2][2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[t][i][j] = w3_f32x4{0.f, 0.f, 0.f, 0.f};
    int dvb[4], d3s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int tap = wave + 8 * t;
        dvb[t] = (((tap / 9) * HP2 + (tap / 3) % 3) * p.D3 + tap % 3) * R3L_VOX_BYTES;
        d3s[t] = tap % 3;
    }
    const int ntap = wave + 24 < 27 ? 4 : 3;
    const bool bias_wave = wave == 3;                      // its fourth slot (tap index 27) sums dy: acc[3][0][j], every row alike
    // LDS byte address of this lane's 8-byte column group inside a row of the arena
    const unsigned chunk = (unsigned)(unsigned long long)(__attribute__((address_space(3))) const char*)lds + (unsigned)(p4 * 8);

    // the next patch's 16-byte units travel from global memory while the current patch is contracted; they are split into the
    // (single) LDS images behind the barrier that ends the patch
    f32x4 xr[XQ], yr[YQ];
    auto stage_load = [&](int patch) __attribute__((always_inline)) {
        const int p1 = r3_div(patch, p.mNP2);
        const int o1_0 = p1 * p.PO1, o2_0 = (patch - p1 * p.np2) * p.PO2;
        const int g1_0 = o1_0 - p.pad, g2_0 = o2_0 - p.pad;
        const int xbase = (g1_0 * p.D2 + g2_0) * p.D3 * RC * 4, ybase = (o1_0 * p.O2 + o2_0) * p.O3 * RC * 4;
#pragma unroll
        for (int i = 0; i < XQ; ++i) {
            const int g1 = g1_0 + (int)(x_h12[i] & 0xffffu), g2 = g2_0 + (int)(x_h12[i] >> 16);
            const bool in = (unsigned)g1 < (unsigned)p.D1 && (unsigned)g2 < (unsigned)p.D2;
            xr[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xsrd, (int)(in ? (unsigned)xbase + x_rel[i] : OOB), 0, 0));
        }
#pragma unroll
        for (int i = 0; i < YQ; ++i) {
            const int o1 = o1_0 + (int)(y_q12[i] & 0xffffu), o2 = o2_0 + (int)(y_q12[i] >> 16);
            const bool in = o1 < p.O1 && o2 < p.O2;
            yr[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ysrd, (int)(in ? (unsigned)ybase + y_rel[i] : OOB), 0, 0));
        }
    };
    auto stage_commit = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < XQ; ++i)
            if ((tid >> 3) + i * (NT / 8) < hvox) split_store(xr[i], sa, lds + W3_XIMG + dst0 + i * (NT / 8) * R3L_VOX_BYTES);
#pragma unroll
        for (int i = 0; i < YQ; ++i) split_store(yr[i], sd, lds + W3_YIMG + dst0 + i * (NT / 8) * R3L_VOX_BYTES);   // (rows past the patch: zeros)
    };
    if ((int)blockIdx.x < npatch) stage_load(blockIdx.x);
    __syncthreads();                                       // zero block visible
    if ((int)blockIdx.x < npatch) stage_commit();
    for (int patch = blockIdx.x; patch < npatch; patch += gridDim.x) {
        const int next = patch + gridDim.x;
        __syncthreads();                                   // this patch's images are complete
        if (next < npatch) stage_load(next);
        for (int s = 0; s < 8; ++s) {
            if (32 * s >= pvox) break;                     // (block-uniform: the patch has no voxel in this k-step)
            // rows of this lane in the 32-voxel group: voxel qa = 32 s + 8 g + qrow and qb = qa + 4
            unsigned xa[2], xm[2], ya[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int q = 32 * s + 8 * g + qrow + 4 * e;
                const int qq = r3_div(q, p.mO3), t = q - qq * p.O3, q1 = r3_div(qq, p.mPO2), q2 = qq - q1 * p.PO2;
                xa[e] = (unsigned)(W3_XIMG + ((q1 * HP2 + q2) * p.D3 + t - p.pad) * R3L_VOX_BYTES) + chunk;
                unsigned tm = 0;
#pragma unroll
                for (int d = 0; d < 3; ++d) tm |= ((unsigned)(t + d - p.pad) < (unsigned)p.D3) ? (1u << d) : 0u;
                xm[e] = q < pvox ? tm : 0u;
                ya[e] = (unsigned)(W3_YIMG + q * R3L_VOX_BYTES) + chunk;
            }
            // dy fragments: co tile j (channels 16 j ..): hi at + 32 j, lo at + 64 + 32 j
            w3_u32x2 fb[8];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int lo = 0; lo < 2; ++lo)
#pragma unroll
                    for (int e = 0; e < 2; ++e) fb[(j * 2 + lo) * 2 + e] = w3_tr_read(ya[e] + 32 * j + 64 * lo);
            w3_wait8(fb);
            half8 bh[2], bl[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                bh[j] = w3_frag(fb[(j * 2) * 2], fb[(j * 2) * 2 + 1]);
                bl[j] = w3_frag(fb[(j * 2 + 1) * 2], fb[(j * 2 + 1) * 2 + 1]);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < ntap) {
                    unsigned ra[2];
#pragma unroll
                    for (int e = 0; e < 2; ++e) ra[e] = ((xm[e] >> d3s[t]) & 1u) ? xa[e] + (unsigned)dvb[t] : chunk;   // zero block
                    w3_u32x2 fa[8];
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int lo = 0; lo < 2; ++lo)
#pragma unroll
                            for (int e = 0; e < 2; ++e) fa[(i * 2 + lo) * 2 + e] = w3_tr_read(ra[e] + 32 * i + 64 * lo);
                    w3_wait8(fa);
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const half8 ah = w3_frag(fa[(i * 2) * 2], fa[(i * 2) * 2 + 1]);
                        const half8 al = w3_frag(fa[(i * 2 + 1) * 2], fa[(i * 2 + 1) * 2 + 1]);
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            acc[t][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[j], acc[t][i][j], 0, 0, 0);
                            acc[t][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[j], acc[t][i][j], 0, 0, 0);
                            acc[t][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[j], acc[t][i][j], 0, 0, 0);
                        }
                    }
                }
            }
            if (bias_wave) {                               // x == 1: hi = 1, lo = 0 -> dy_lo + dy_hi, exact in fp32 accumulation
                const half8 one = {(_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1};
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[3][0][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(one, bl[j], acc[3][0][j], 0, 0, 0);
                    acc[3][0][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(one, bh[j], acc[3][0][j], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                   // every wave has read its last fragment of this patch
        if (next < npatch) stage_commit();
    }
    // D map of v_mfma_f32_16x16x32: column (co) = lane & 15, row (ci) = 4 (lane >> 4) + r
    const long long blk = (long long)b * gridDim.x + blockIdx.x;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t < ntap) {
            float* dst = p.slab + blk * W3_SLAB + (wave + 8 * t) * RC * RC;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[(16 * i + 4 * g + r) * RC + 16 * j + l16] = (acc[t][i][j][r] * ua) * ud;
        }
    }
    if (bias_wave && g == 0) {                             // row 0 of the "ones" tile: scaled by the dy scale only
#pragma unroll
        for (int j = 0; j < 2; ++j) p.slab[blk * W3_SLAB + 27 * RC * RC + 16 * j + l16] = acc[3][0][j][0] * ud;
    }
}
