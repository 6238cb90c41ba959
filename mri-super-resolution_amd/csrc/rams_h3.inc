// RAMS 3x3x3 convolution 32 -> 32 on the fp16 matrix cores with hi/lo-split operands (included by rams.hip, namespace inr).
//
// Same implicit GEMM as conv3d_c32_mfma_kernel (M = 32 output voxels per wave tile, N = 32 output channels, K = 27 taps
// x 32 input channels; folded kernel resident in LDS, A operand straight from global memory through a buffer resource),
// but every fp32 product is taken as three fp16 MFMA products: x*s = hi + lo with hi = fp16(x*s) rounded to nearest and
// lo = fp16(x*s - hi), products hi*lo + lo*hi + hi*hi on v_mfma_f32_32x32x16_f16 (fp32 accumulate; the lo*lo term,
// 2^-22 relative, is dropped).  One tap is 6 MFMAs of 32 cycles instead of 16 of 64.
//   * weights: split once per forward call by rams_weight_split_all_kernel (one block per convolution: max|w| -> power-of-two
//     scale -> hi/lo planes already in the LDS fragment order [tap][k-half][lane-half][cout][8 cin]);
//   * activations: split in the operand path (2-3 VALU per element, hidden behind the other wave's MFMAs) with a
//     power-of-two scale from the EXACT max|x| of the tensor, which every producer of a convolution input leaves in a
//     slot (atomic max on the float bits: order independent, so runs stay bitwise reproducible);
//   * epilogue: acc * 2^-ka * 2^-kb (two exact steps), bias, ReLU, channel sums, max|y| for the next convolution.

#ifndef R3_ABLATE
#define R3_ABLATE 0      // diagnostic builds: 1 = no operand split, 2 = no MFMAs, 4 = no global operand loads (wrong results)
#endif
constexpr int R3_PLANE_HALVES = 27 * RC * RC;            // one plane (hi or lo) of a folded kernel
constexpr int R3_LAYER_HALVES = 2 * R3_PLANE_HALVES;

// (the format -- h3_scale_exp, h3_pow2, h3_split2 -- is split_fp16.h's, shared with the GEMMs)

// eight consecutive channels (two 16-byte loads) -> one hi and one lo MFMA operand
__device__ __forceinline__ void r3_split8(const f32x4& x0, const f32x4& x1, float s, half8& hi, half8& lo) {
    half2v h[4], l[4];
    h3_split2(x0[0], x0[1], s, h[0], l[0]);
    h3_split2(x0[2], x0[3], s, h[1], l[1]);
    h3_split2(x1[0], x1[1], s, h[2], l[2]);
    h3_split2(x1[2], x1[3], s, h[3], l[3]);
    hi = half8{h[0][0], h[0][1], h[1][0], h[1][1], h[2][0], h[2][1], h[3][0], h[3][1]};
    lo = half8{l[0][0], l[0][1], l[1][0], l[1][1], l[2][0], l[2][1], l[3][0], l[3][1]};
}

// max|.| of a tensor without a hot atomic: a "slot" is R3_SLOT words (zeroed once per forward); every producer BLOCK folds
// its maximum (wave shuffles, LDS, one atomic max on the float bits -- order independent) into word (linear block id mod
// R3_SLOT), every consumer block takes the maximum over the R3_SLOT words when it starts.  (One word per tensor made the
// 8,192 waves of an element-wise pass queue on a single address: 50-60 us per launch, a third of a batch-1 forward.)
constexpr int R3_SLOT = 1024;
__device__ __forceinline__ void r3_block_amax(float v, unsigned* slot) {      // every thread of the block, exactly once
    __shared__ float r3_red[16];
    float m = fabsf(v);
    m = wave_max(m);
    const int nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) r3_red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nw; ++w) m = fmaxf(m, r3_red[w]);
        const unsigned bits = __float_as_uint(m);
        if (bits != 0u && bits < 0x7f800000u) atomicMax(slot + ((blockIdx.x + gridDim.x * blockIdx.y) & (R3_SLOT - 1)), bits);
    }
}
__device__ __forceinline__ unsigned r3_slot_max(const unsigned* slot) {       // every thread of the block; returns to all
    __shared__ unsigned r3_smax[16];
    unsigned m = 0;
    for (int i = threadIdx.x; i < R3_SLOT; i += blockDim.x) {
        const unsigned v = slot[i];
        m = v > m ? v : m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, off, 64);
        m = o > m ? o : m;
    }
    const int nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) r3_smax[threadIdx.x >> 6] = m;
    __syncthreads();
    m = r3_smax[0];
    for (int w = 1; w < nw; ++w) m = r3_smax[w] > m ? r3_smax[w] : m;
    return m;
}

// One block per convolution layer: w [27][32 cin][32 cout] fp32 -> amax slot + hi/lo planes in fragment order:
// element (tap, cin k, cout n) -> half index ((tap*2 + k/16)*2 + (k%16)/8) * 256 + n*8 + k%8.
struct R3SplitJob {
    const float* w;
    _Float16* planes;     // [2][27*1024]
    unsigned* amax;
    int flip;             // 1: split the DATA-GRADIENT kernel wd[tap][co][ci] = w[26 - tap][ci][co] (flipped taps, channel axes swapped)
};
__device__ __forceinline__ void rams_weight_split_body(const R3SplitJob j) {
    __shared__ float red[8];
    __shared__ float amax_s;
    float m = 0.f;
    for (int i = threadIdx.x; i < CONV_W_FLOATS; i += 512) m = fmaxf(m, fabsf(j.w[i]));
#pragma unroll   // wave_max(), open-coded: through the helper this translation unit's instruction schedule changes
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int k = 0; k < 8; ++k) t = fmaxf(t, red[k]);
        amax_s = t;
        *j.amax = __float_as_uint(t);
    }
    __syncthreads();
    const float s = h3_pow2(h3_scale_exp(__float_as_uint(amax_s)));
    // a thread takes one (tap, cin pair, cout): cin pairs keep cvt_pkrtz busy with two values
    for (int i = threadIdx.x; i < CONV_W_FLOATS / 2; i += 512) {
        const int n = i % RC, kp = (i / RC) % (RC / 2), tap = i / (RC * RC / 2);
        const int k = 2 * kp;
        half2v h, l;
        if (j.flip) h3_split2(j.w[((26 - tap) * RC + n) * RC + k], j.w[((26 - tap) * RC + n) * RC + k + 1], s, h, l);
        else h3_split2(j.w[(tap * RC + k) * RC + n], j.w[(tap * RC + k + 1) * RC + n], s, h, l);
        const int at = ((tap * 2 + k / 16) * 2 + (k % 16) / 8) * 256 + n * 8 + k % 8;
        *reinterpret_cast<half2v*>(j.planes + at) = h;
        *reinterpret_cast<half2v*>(j.planes + R3_PLANE_HALVES + at) = l;
    }
}

struct Conv3dH3Params {
    const float* x;       // [B][D1][D2][D3][32]
    float* y;             // [B][O1][O2][O3][y_cstride]
    const _Float16* planes;   // hi plane then lo plane, fragment order
    const float* bias;    // [32]
    float* chan_slab;     // nullable: [B][waves_per_b][32] per-channel sums of the (post-activation) output
    const unsigned* x_amax;   // slot (R3_SLOT words) of float bits whose maximum is max|x|
    const unsigned* w_amax;   // float bits of max|w|
    unsigned* y_amax;     // nullable: slot that receives max|y|
    int B, D1, D2, D3, O1, O2, O3;
    int pad;
    int cout, y_cstride;
    int relu;
    int tiles_per_b, waves_per_b;
    long long x_elems_per_b;
};

template <int MT>
__global__ void __launch_bounds__(CONV_THREADS) conv3d_c32_h3_kernel(const Conv3dH3Params p) {
    __shared__ __attribute__((aligned(16))) _Float16 sw[R3_LAYER_HALVES];      // 110,592 B
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l32 = lane & 31;
    const int b = blockIdx.y;
    for (int i = tid; i < R3_LAYER_HALVES / 8; i += CONV_THREADS)
        reinterpret_cast<u32x4*>(sw)[i] = reinterpret_cast<const u32x4*>(p.planes)[i];
    const int ka = h3_scale_exp(r3_slot_max(p.x_amax)), kb = h3_scale_exp(*p.w_amax);
    const float sa = h3_pow2(ka), ua = h3_pow2(-ka), ub = h3_pow2(-kb);
    __syncthreads();

    const long long xbytes = p.x_elems_per_b * 4;
    const __amdgpu_buffer_rsrc_t srd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.x + (long long)b * p.x_elems_per_b), 0, (int)(unsigned)(xbytes > 0x7FFFFFFFll ? 0x7FFFFFFFll : xbytes),
        0x00020000);
    const int ovox = p.O1 * p.O2 * p.O3;
    const float bias = p.bias[l32];
    float csum = 0.f, ymax = 0.f;
    const int half = p.waves_per_b >> 1;
    const int wid = (wave < 4) ? (blockIdx.x * 4 + wave) : (half + blockIdx.x * 4 + (wave - 4));
    const int groups = (p.tiles_per_b + MT - 1) / MT;
    const _Float16* swl = sw + R3_PLANE_HALVES;

    for (int grp = wid; grp < groups; grp += p.waves_per_b) {
        int base[MT];
        unsigned mask[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int v = (grp * MT + m) * 32 + l32;
            const bool vvalid = v < ovox;
            const int o3 = v % p.O3, o2 = (v / p.O3) % p.O2, o1 = v / (p.O3 * p.O2);
            // lane half h owns channels 16 i + 8 h .. + 7 of each 16-channel block i
            base[m] = ((((o1 - p.pad) * p.D2 + (o2 - p.pad)) * p.D3 + (o3 - p.pad)) * RC + 8 * h) * 4;
            unsigned m1 = 0, m2 = 0, m3 = 0;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                m1 |= ((unsigned)(o1 + d - p.pad) < (unsigned)p.D1) ? (1u << d) : 0u;
                m2 |= ((unsigned)(o2 + d - p.pad) < (unsigned)p.D2) ? (1u << d) : 0u;
                m3 |= ((unsigned)(o3 + d - p.pad) < (unsigned)p.D3) ? (1u << d) : 0u;
            }
            unsigned mk = 0;
#pragma unroll
            for (int d1 = 0; d1 < 3; ++d1)
#pragma unroll
                for (int d2 = 0; d2 < 3; ++d2)
                    mk |= (((m1 >> d1) & (m2 >> d2) & 1u) ? m3 : 0u) << (9 * d1 + 3 * d2);
            if (!vvalid) mk = 0;
            mask[m] = mk;
        }
        f32x16 acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

        // raw[.][m][2 i + q]: channels 16 i + 8 h + 4 q .. + 3 of tile m's voxel for one tap
        auto load_tap = [&](int tap, f32x4(&a)[MT][4]) {
#ifdef R3_ABLATE_SAME_VOXEL   // diagnostic: every tap re-reads the centre voxel (perfect L1 reuse) -- wrong results
            const int delta = ((1 * p.D2 + 1) * p.D3 + 1) * RC * 4 + 0 * tap;
#else
            const int delta = (((tap / 9) * p.D2 + (tap / 3) % 3) * p.D3 + tap % 3) * RC * 4;   // wave-uniform
#endif
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int off = ((mask[m] >> tap) & 1u) ? base[m] + delta : 0x7F000000;         // out of range reads 0
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        if (R3_ABLATE & 4) a[m][2 * i + q] = f32x4{(float)off, 1.f, 2.f, 3.f};
                        else a[m][2 * i + q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd, off + i * 64 + q * 16, 0, 0));
                    }
            }
        };
        auto convert = [&](const f32x4(&a)[MT][4], half8(&hi)[MT][2], half8(&lo)[MT][2]) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if (R3_ABLATE & 1) {
                        hi[m][i] = __builtin_bit_cast(half8, a[m][2 * i]);
                        lo[m][i] = __builtin_bit_cast(half8, a[m][2 * i + 1]);
                    } else {
                        r3_split8(a[m][2 * i], a[m][2 * i + 1], sa, hi[m][i], lo[m][i]);
                    }
                }
        };
        auto mma_tap = [&](int tap, const half8(&hi)[MT][2], const half8(&lo)[MT][2]) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int at = ((tap * 2 + i) * 2 + h) * 256 + l32 * 8;
                const half8 bh = *reinterpret_cast<const half8*>(sw + at);
                const half8 bl = *reinterpret_cast<const half8*>(swl + at);
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    if (R3_ABLATE & 2) {
                        acc[m][0] += (float)lo[m][i][0] + (float)hi[m][i][1] + (float)bh[2] + (float)bl[3];
                        continue;
                    }
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(lo[m][i], bh, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hi[m][i], bl, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hi[m][i], bh, acc[m], 0, 0, 0);
                }
            }
        };
        // raw operands two taps ahead of their MFMAs (three rotating sets), the split one tap ahead (two sets):
        // the pattern repeats every 6 taps; 27 = 4 x 6 + 3
        f32x4 r0[MT][4], r1[MT][4], r2[MT][4];
        half8 h0[MT][2], l0[MT][2], h1[MT][2], l1[MT][2];
        load_tap(0, r0);
        load_tap(1, r1);
        convert(r0, h0, l0);
#pragma unroll 1
        for (int tap = 0; tap < 24; tap += 6) {
            load_tap(tap + 2, r2); convert(r1, h1, l1); mma_tap(tap, h0, l0);
            load_tap(tap + 3, r0); convert(r2, h0, l0); mma_tap(tap + 1, h1, l1);
            load_tap(tap + 4, r1); convert(r0, h1, l1); mma_tap(tap + 2, h0, l0);
            load_tap(tap + 5, r2); convert(r1, h0, l0); mma_tap(tap + 3, h1, l1);
            load_tap(tap + 6, r0); convert(r2, h1, l1); mma_tap(tap + 4, h0, l0);
            load_tap(tap + 7, r1); convert(r0, h0, l0); mma_tap(tap + 5, h1, l1);
        }
        // taps 24, 25, 26: r0 = tap 24 (already split into h0/l0), r1 = tap 25
        load_tap(26, r2); convert(r1, h1, l1); mma_tap(24, h0, l0);
        convert(r2, h0, l0); mma_tap(25, h1, l1);
        mma_tap(26, h0, l0);

        // epilogue: C/D map col = lane&31 (cout), row = (r&3) + 8*(r>>2) + 4h (voxel inside the tile)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int tile = grp * MT + m;
            float tsum = 0.f;
            float* yb = p.y + ((long long)b * ovox + (long long)tile * 32) * p.y_cstride + l32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mfma32_acc_row(r, h);
                float o = (acc[m][r] * ua) * ub + bias;
                if (p.relu) o = fmaxf(o, 0.f);
                if (tile * 32 + row < ovox) {
                    tsum += o;
                    if (l32 < p.cout) {
                        yb[(long long)row * p.y_cstride] = o;
                        ymax = fmaxf(ymax, fabsf(o));
                    }
                }
            }
            if (p.chan_slab) csum += tsum + __shfl_xor(tsum, 32, 64);
        }
    }
    if (p.chan_slab && lane < 32) p.chan_slab[((long long)b * p.waves_per_b + wid) * RC + lane] = csum;
    if (p.y_amax) r3_block_amax(ymax, p.y_amax);
}

// =====================================================================================================================
// The same convolution with the roles of LDS and the global path swapped (default for inference).
//
// Measured on conv3d_c32_h3_kernel (-DR3_ABLATE builds, batch 25): the operand loads alone are 31 of 58 ms -- a wave's
// 16-byte load per lane touches 32 different 128-byte lines for 1 KB of data and every voxel line is fetched by 27 taps x 4
// instructions (making all taps read ONE voxel changes nothing: it is the line look-ups, not the misses) -- and the split
// of the operand costs its VALU 27 times per input element.  Here
//   * a block stages the input patch (PO1 x PO2 outputs in-plane, all temporal planes, +-1 halo; <= 486 voxels) ONCE:
//     coalesced 16-byte loads, split into hi/lo fp16 on the way, written to an LDS image of 128 B per voxel = eight 16-byte
//     chunks (hi of channels 0-7, 8-15, 16-23, 24-31, then the lo's), chunk c of voxel v at slot c ^ ((v >> 1) & 7) so that
//     the sixteen lanes of a ds_read_b128 phase hit sixteen different bank groups; out-of-image halo voxels are zeros;
//   * the K-loop has NO VALU work: per tap four ds_read_b128 (hi/lo of two 16-channel blocks) at lane address + a
//     wave-uniform tap offset, and the weights arrive straight from global/L2 in fragment order (lanes 0-31 / 32-63 read
//     consecutive 512-byte runs: 8 lines per instruction instead of 32), three taps of them in flight;
//   * two patch images alternate: the next patch is loaded into registers before the taps of the current one and
//     converted / written after them.
// Temporal borders ('same' padding along T) are a per-lane 3-bit mask that redirects the read to a zero chunk.
// =====================================================================================================================
constexpr int R3L_MAX_HVOX = 486;                 // voxels of one staged patch (6 x 9 x 9)
// Round 3: a voxel of the staged image takes 144 bytes -- its eight 16-byte chunks in natural order + 16 bytes of padding --
// instead of 128 with the chunks XOR-swizzled by the voxel index.  Consecutive lanes read consecutive voxels, and 36 dwords of
// stride walk the 64 banks without a collision inside any ds_read_b128 lane group, so the swizzle is not needed; without it a
// lane's read address is ONE per-tile base + a wave-uniform tap offset + a compile-time chunk offset: one v_add per tap and tile
// where the swizzled form spent ~20 VALU per tap and tile recomputing (voxel >> 1) & 7 and four slot addresses.  -DR3_ABLATE
// builds had shown the tap loop to be bound by vector-instruction issue, not by operand delivery: with every operand load removed
// it still ran at 2.7 x the MFMA time (tools/rams_ablate.sh).
constexpr int R3L_VOX_BYTES = 144;
constexpr int R3L_IMG_BYTES = R3L_MAX_HVOX * R3L_VOX_BYTES;
struct Conv3dLdsParams {
    const float* x;           // [B][D1][D2][D3][32]
    float* y;                 // [B][O1][O2][O3][y_cstride]
    const _Float16* planes;   // hi plane then lo plane, fragment order (rams_weight_split_body)
    const float* bias;
    float* chan_slab;         // nullable: [B][gridDim.x * 8][32]
    const unsigned* x_amax;
    const unsigned* w_amax;
    unsigned* y_amax;         // nullable
    const float* aux;         // AUX kernels: a tensor of y's shape read at every output's address (may BE y: each element is read by the
                              // lane that then writes it) -- AUX 1: y = conv + aux; AUX 2: y = aux > 0 ? conv : 0 (the ReLU of the forward);
                              // AUX 4: y = conv * gate[b][channel] + aux (the attention block's scale + residual, gate known beforehand)
    const float* gate;        // AUX 4: [B][32]
    int B, D1, D2, D3, O1, O2, O3;
    int y_pad;                // 1: y is an image of (O1 + 2) x (O2 + 2) x O3 voxels and output (o1, o2) goes to (o1 + 1, o2 + 1): the interior of
                              // the reflect-padded tensor the next block reads (its frame is filled by reflect_border_v4_kernel); AUX = 0 only
    int pad, cout, y_cstride, relu;
    int PO1, PO2;             // outputs of a patch in-plane
    int np1, np2;             // patches per image along each axis
    // ceil(2^32 / d) of the divisors the kernels decode indices with: q / d == __umulhi(q, magic) for q * d < 2^32 (patch-local
    // indices are < 2^13).  The compiler's run-time 32-bit division is ~35 VALU instructions; the staging loop did three per
    // 16-byte load and the tile decode three per tile -- about a thousand VALU per wave and patch, as much issue time as the
    // patch's MFMAs (R3_ABLATE builds without any operand load still ran at 4x the MFMA time).
    unsigned mD3, mHP2, mO3, mPO2, mNP2;
    unsigned long long* stamps;   // -DR3_STAMPS builds: [8] summed cycles per phase of the patch loop + [8] wave count (else unused)
};
__device__ __forceinline__ int r3_div(int q, unsigned magic) { return magic ? (int)__umulhi((unsigned)q, magic) : q; }
inline unsigned r3_magic(int d) { return d <= 1 ? 0u : (unsigned)((0x100000000ull + (unsigned)d - 1) / (unsigned)d); }   // 0: d = 1

// Wave-level hand-shakes of the staged kernel (LDS counters; the LDS unit of a CU executes the instructions of its waves in issue
// order, so a wave's ds_add is seen after its earlier ds_write / ds_read have taken effect).
__device__ __forceinline__ void r3_signal(unsigned* c, int lane) {
    asm volatile("" ::: "memory");
    if (lane == 0) atomicAdd(c, 1u);
    asm volatile("" ::: "memory");
}
__device__ __forceinline__ void r3_wait_count(unsigned* c, unsigned target) {
    while (*reinterpret_cast<volatile unsigned*>(c) < target) __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
}
#ifdef R3_STAMPS   // phase k ends here: add the cycles since the previous mark (one wave = one s_memtime stream)
#define R3_MARK(k) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); ph_[k] += now_ - tprev_; tprev_ = now_; }
#else
#define R3_MARK(k)
#endif
#ifndef R3_SKEW
#define R3_SKEW 56      // x 64 cycles: head start of the first wave of every SIMD over the second one (see the kernel comment)
#endif

// WAVES waves per block, MT wave tiles (32 outputs each) per wave that share every weight fragment: <8, 1> needs 8 KB of
// operands per 6 MFMAs per wave (LDS + L1 deliver ~190 B/clk per CU, the matrix cores would take 170: delivery-bound);
// <4, 2> needs 6 KB per 12 MFMAs (125 B/clk per CU: the matrix cores bind).
//
// SINGLE: one staged image instead of two, so that TWO blocks of <4, 2> share a CU (2 x 70 KB of LDS, two waves per SIMD): the
// tiles of a wave pair share every weight fragment -- half the L1 traffic of <8, 1>, whose 4 KB per six MFMAs per wave is more
// than the 64 B/clk of the L1 can deliver (13.8 k cycles per patch against 10.4 k of MFMA) -- and the block that is storing its
// tiles and splitting its next image leaves the matrix cores to the other one.
//
// What bounds it now (s_memtime phase sums, tools/rams_stamps.py; batch 25, one image): a wave spends 16 k cycles of 29 k per patch in
// the taps (10.4 k would be the matrix-core time of its two tiles), 6 k splitting the next image, 2.4 k issuing its loads, 2.5 k in
// the epilogue.  The vector-memory counter retires IN ORDER, so (a) the first wait for a load issued behind the epilogue's stores
// also waits for their acknowledgements and (b) the first weight wait of a tile also waits for the image loads issued before it:
// both latencies are exposed once per patch and only the other block of the CU covers them.  Tried on top and not kept: the next
// tile's first weights loaded BEFORE the stores, the image split before the epilogue, every load and store on one straight-line
// path so that the compiler's in-flight count is exact (vmcnt(55) at the first MFMA as intended; 26.6 ms against 25.4: the
// longer live ranges spill, and a spill reload behind the stores pays the same acknowledgement wait); a head start of one block
// of each CU (no change).
//
// AUX (training step, backward): the two element-wise passes that followed a data-gradient convolution -- the ReLU mask of the
// forward activation with the maximum of the masked gradient (relu_backward_kernel), the sum with the gradient of the residual
// path (accumulate_kernel) -- happen in the epilogue instead: one 4-byte load per output at the address it is stored to, issued
// for a whole tile before its arithmetic (the operand registers of the taps are dead by then).  Bit-identical to the two passes.
template <int WAVES, int MT, bool SINGLE = false, int AUX = 0>
__global__ void __launch_bounds__(WAVES * 64, SINGLE ? 2 : 1) conv3d_c32_lds_kernel(const Conv3dLdsParams p) {
    constexpr int NT = WAVES * 64;
    constexpr int R3L_STAGE_Q = (R3L_MAX_HVOX * 8 + NT - 1) / NT;      // 16-byte units of a patch per thread
    // one arena: 256 bytes of zeros (the operand of a tap outside the temporal range) at offset 0, then the two patch images --
    // a lane's read address is then a plain byte offset that a single multiply-add selects (see load_a)
    constexpr int R3L_IMG0 = 256;
    __shared__ __attribute__((aligned(16))) char lds[R3L_IMG0 + (SINGLE ? 1 : 2) * R3L_IMG_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l32 = lane & 31;
    const int b = blockIdx.y;
    const int HP1 = p.PO1 + 2, HP2 = p.PO2 + 2;
    const int hvox = HP1 * HP2 * p.D3;
    const int pvox = p.PO1 * p.PO2 * p.O3;                 // outputs of a full patch
    const int ptiles = (pvox + 31) / 32;
    const int npatch = p.np1 * p.np2;
    if (tid < 64) reinterpret_cast<float*>(lds)[tid] = 0.f;
    const int ka = h3_scale_exp(r3_slot_max(p.x_amax)), kb = h3_scale_exp(*p.w_amax);
    const float sa = h3_pow2(ka), ua = h3_pow2(-ka), ub = h3_pow2(-kb);
    const float bias = p.bias[l32];
    constexpr unsigned R3L_OOB = 0x40000000u;              // buffer offsets from here on are past every image: loads give 0, stores drop
    const __amdgpu_buffer_rsrc_t wsrd =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(p.planes), 0, R3_LAYER_HALVES * 2, 0x00020000);
    // input / output image of this block's batch element as buffers (the host checks that one image stays below 1 GiB): a halo
    // voxel outside the image, a tile row past the patch or an output channel >= cout is ONE out-of-range offset, no branch
    const __amdgpu_buffer_rsrc_t xsrd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.x) + (long long)b * p.D1 * p.D2 * p.D3 * RC, 0, p.D1 * p.D2 * p.D3 * RC * 4, 0x00020000);
    const int YO1 = p.O1 + 2 * p.y_pad, YO2 = p.O2 + 2 * p.y_pad;      // the output image as laid out in memory
    const __amdgpu_buffer_rsrc_t ysrd = __builtin_amdgcn_make_buffer_rsrc(
        p.y + (long long)b * YO1 * YO2 * p.O3 * p.y_cstride, 0, YO1 * YO2 * p.O3 * p.y_cstride * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t asrd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(AUX ? p.aux : p.y) + (long long)b * p.O1 * p.O2 * p.O3 * p.y_cstride, 0, p.O1 * p.O2 * p.O3 * p.y_cstride * 4,
        0x00020000);
    const float gate_c = AUX == 4 ? p.gate[b * RC + l32] : 1.f;
    const int wlane = (h * 256 + l32 * 8) * 2;             // byte offset of this lane inside a (tap, i) fragment block
    float csum = 0.f, ymax = 0.f;

    // ---- staging: global -> registers (issue early), registers -> split -> LDS ---------------------------------------------
    // A thread's 16-byte units sit at the same place of every patch: their byte offset from the patch's first halo voxel is decoded
    // ONCE; per patch a unit costs one add, and range checks only where the halo leaves the image (the decode with its divisions,
    // per unit and patch, was 1.7 k cycles of a wave's 25 k per patch: s_memtime phase sums, tools/rams_stamps.py).
    f32x4 sreg[R3L_STAGE_Q];
    unsigned s_rel[R3L_STAGE_Q];
    auto unit_rowcol = [&](int i, int& h1, int& h2, int& t) __attribute__((always_inline)) {
        const int hv = (tid >> 3) + i * (NT / 8);
        const int hq = r3_div(hv, p.mD3);
        t = hv - hq * p.D3;
        h1 = r3_div(hq, p.mHP2);
        h2 = hq - h1 * HP2;
    };
#pragma unroll
    for (int i = 0; i < R3L_STAGE_Q; ++i) {
        int h1, h2, t;
        unit_rowcol(i, h1, h2, t);
        s_rel[i] = (tid >> 3) + i * (NT / 8) < hvox ? (unsigned)(((h1 * p.D2 + h2) * p.D3 + t) * RC + 4 * (tid & 7)) * 4u : R3L_OOB;
    }
    const int s_dst0 = (tid >> 3) * R3L_VOX_BYTES + ((tid & 7) >> 1) * 16 + (tid & 1) * 8;   // unit i: + i * (NT / 8) voxels
    auto patch_origin = [&](int patch, int& o1_0, int& o2_0) __attribute__((always_inline)) {
        const int p1 = r3_div(patch, p.mNP2);
        o1_0 = p1 * p.PO1;
        o2_0 = (patch - p1 * p.np2) * p.PO2;
    };
    auto stage_load = [&](int patch) __attribute__((always_inline)) {
        int o1_0, o2_0;
        patch_origin(patch, o1_0, o2_0);
        // (valid convolutions read rows o..o+2: the patch starts at o_0; 'same' ones at o_0 - 1)
        const int g1_0 = o1_0 - p.pad, g2_0 = o2_0 - p.pad;
        const int base = (g1_0 * p.D2 + g2_0) * p.D3 * RC * 4;
        if (g1_0 >= 0 && g2_0 >= 0 && g1_0 + HP1 <= p.D1 && g2_0 + HP2 <= p.D2) {     // (wave-uniform) the halo is inside the image
#pragma unroll
            for (int i = 0; i < R3L_STAGE_Q; ++i)
                sreg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xsrd, (int)((unsigned)base + s_rel[i]), 0, 0));
        } else {                                           // a patch on the image border: range checks per unit
#pragma unroll
            for (int i = 0; i < R3L_STAGE_Q; ++i) {
                int h1, h2, t;
                unit_rowcol(i, h1, h2, t);
                const bool in = (unsigned)(g1_0 + h1) < (unsigned)p.D1 && (unsigned)(g2_0 + h2) < (unsigned)p.D2;
                const unsigned off = in ? (unsigned)base + s_rel[i] : R3L_OOB;
                sreg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xsrd, (int)off, 0, 0));
            }
        }
    };
    auto stage_commit = [&](char* dst) __attribute__((always_inline)) {
        char* at0 = dst + s_dst0;                           // hi chunk of channels 8 * (cc / 2) .. + 7 of this thread's first voxel
#pragma unroll
        for (int i = 0; i < R3L_STAGE_Q; ++i) {
            if ((tid >> 3) + i * (NT / 8) < hvox) {
                half2v h0, l0, h1, l1;
                h3_split2(sreg[i][0], sreg[i][1], sa, h0, l0);
                h3_split2(sreg[i][2], sreg[i][3], sa, h1, l1);
                char* at = at0 + i * (NT / 8) * R3L_VOX_BYTES;
                *reinterpret_cast<uint2*>(at) = uint2{__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1)};
                *reinterpret_cast<uint2*>(at + 64) = uint2{__builtin_bit_cast(unsigned, l0), __builtin_bit_cast(unsigned, l1)};
            }
        }
    };
    // byte offsets of a tile's 32 output voxels inside the output image (R3L_OOB: no such voxel), per wave: written by the lanes
    // that decode the tile, read back in accumulator-row order by the epilogue (four ds_read_b128 per tile instead of sixteen
    // 64-bit shuffles: the epilogue was 4.7 k cycles of a wave's 25 k per patch)
    __shared__ __attribute__((aligned(16))) unsigned rowtab[WAVES][MT][32];
    const unsigned lane_term = (unsigned)l32 * 4u + (l32 < p.cout ? 0u : R3L_OOB);
    const float relu_floor = p.relu ? 0.f : -__builtin_inff();

    // ---- patch loop: no block-wide barrier ------------------------------------------------------------------------------
    // A barrier per patch keeps the eight waves in one phase: while they store their tiles and split the next image the matrix
    // cores idle (SQ counters of the barrier version, batch 25: MFMA busy 39 % of the SIMD cycles; per wave 33 % issuing, 30 %
    // parked at a wait, 37 % stalled on a busy pipe).  Two counters replace it:
    //   sync_cnt[0] += 1 per wave once it has written its share of an image      (image k is complete at WAVES * (k + 1))
    //   sync_cnt[1] += 1 per wave once it has read the last operand of a patch   (image k is free at WAVES * (k + 1))
    // Iteration `it` of a wave: wait until image it - 1 is free, split image it + 1 into that buffer, post it, start the global
    // loads of image it + 2, wait for image it, run the taps, post "read", store the tile.  The two waves of a SIMD then run half
    // a phase apart -- one stores / splits while the other has the matrix core to itself -- and stay so: the lead is kept by
    // construction (the wave ahead never waits for the epilogue of the other), it only has to exist, hence the one-off R3_SKEW
    // sleep of the upper half of the waves (wave w runs on SIMD w % 4).
    __shared__ unsigned sync_cnt[2];
    if (tid < 2) sync_cnt[tid] = 0;
    int patch = blockIdx.x;
    const int G = gridDim.x;
    if (patch < npatch) stage_load(patch);
    __syncthreads();                                       // zeros[], sync_cnt[] visible
    if (patch < npatch) stage_commit(lds + R3L_IMG0);
    if constexpr (SINGLE) {
        __syncthreads();
    } else {
        r3_signal(&sync_cnt[0], lane);
        if (patch + G < npatch && !(R3_ABLATE & 64)) stage_load(patch + G);
        if (R3_SKEW > 0 && WAVES == 8 && wave >= 4) __builtin_amdgcn_s_sleep(R3_SKEW);
    }
    const int ngrp = (ptiles > wave * MT) ? (ptiles - wave * MT + WAVES * MT - 1) / (WAVES * MT) : 0;
#ifdef R3_STAMPS
    unsigned long long ph_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev_ = __builtin_amdgcn_s_memtime();
#endif
    for (unsigned it = 0; patch < npatch; patch += G, ++it) {
        const int next = patch + G;
        if constexpr (!SINGLE) {
            r3_wait_count(&sync_cnt[1], WAVES * it);           // every wave has left the taps of iteration it - 1
            R3_MARK(0)
            if (next < npatch && !(R3_ABLATE & 64)) stage_commit(lds + R3L_IMG0 + ((it + 1) & 1) * R3L_IMG_BYTES);
            R3_MARK(1)
            r3_signal(&sync_cnt[0], lane);
            if (next + G < npatch && !(R3_ABLATE & 64)) stage_load(next + G);
            R3_MARK(2)
            r3_wait_count(&sync_cnt[0], WAVES * (it + 1));     // image `it` complete
            R3_MARK(3)
        }
        // arena offset of image `it`
        const int im = R3L_IMG0 + ((SINGLE || (R3_ABLATE & 64)) ? 0 : (int)(it & 1) * R3L_IMG_BYTES);
        // leaving the taps (two images): post "read"
        auto taps_done = [&]() __attribute__((always_inline)) {
            if constexpr (!SINGLE) r3_signal(&sync_cnt[1], lane);
        };
        if constexpr (SINGLE) {     // the next patch's global loads travel during the taps; split after the block's barrier below
            if (next < npatch && !(R3_ABLATE & 64)) stage_load(next);
            R3_MARK(2)
        }
        int o1_0, o2_0;
        patch_origin(patch, o1_0, o2_0);
        if (ngrp == 0) taps_done();
        for (int gi = 0; gi < ngrp; ++gi) {
            const int grp = wave + gi * WAVES;
            // tile m of this wave: outputs q = (grp * MT + m) * 32 + l32 -> (q1, q2, t) inside the patch
            int abase[MT];                                  // LDS byte offset of the lane's tap (0, 0, 0) voxel + its chunk
            unsigned tmask[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int q = (grp * MT + m) * 32 + l32;
                const int qq = r3_div(q, p.mO3), t = q - qq * p.O3, q1 = r3_div(qq, p.mPO2), q2 = qq - q1 * p.PO2;
                const int o1 = o1_0 + q1, o2 = o2_0 + q2;
                const bool valid = q < pvox && o1 < p.O1 && o2 < p.O2;
                abase[m] = ((q1 * HP2 + q2) * p.D3 + t - p.pad) * R3L_VOX_BYTES + h * 16;   // halo voxel of tap (0, 0, 0)
                unsigned tm = 0;                                           // bit d: temporal tap d stays inside [0, D3)
#pragma unroll
                for (int d = 0; d < 3; ++d) tm |= ((unsigned)(t + d - p.pad) < (unsigned)p.D3) ? (1u << d) : 0u;
                tmask[m] = valid ? tm : 0u;
                rowtab[wave][m][l32] =
                    valid ? (unsigned)((((o1 + p.y_pad) * YO2 + o2 + p.y_pad) * p.O3 + t) * p.y_cstride) * 4u : R3L_OOB;
            }
            f32x16 acc[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
            u32x4 wq0[4], wq1[4], wq2[4];                  // weights of three taps: (i = 0 hi, i = 0 lo, i = 1 hi, i = 1 lo)
            auto load_w = [&](int tap, u32x4(&w)[4]) {      // (the tap part of the address travels in the scalar offset: no VALU)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int at = (tap * 2 + i) * 1024;                   // bytes inside the hi plane, wave-uniform
                    if (R3_ABLATE & 8) {
                        w[2 * i] = u32x4{(unsigned)at, 1u, 2u, 3u};
                        w[2 * i + 1] = u32x4{(unsigned)at, 5u, 6u, 7u};
                        continue;
                    }
                    w[2 * i] = __builtin_amdgcn_raw_buffer_load_b128(wsrd, wlane, at, 0);
                    w[2 * i + 1] = __builtin_amdgcn_raw_buffer_load_b128(wsrd, wlane, at + R3_PLANE_HALVES * 2, 0);
                }
            };
            half8 a0[MT][4], a1[MT][4];                 // operands of two taps: (i = 0 hi, i = 0 lo, i = 1 hi, i = 1 lo)
            // A lane's operand address for a tap: aB + dvb * aK with (aB, aK) = (image + lane base, 1) where the tap's temporal
            // offset d3 stays inside [0, D3) and (0, 0) -- the zero block -- where it does not; the pair is formed once per tile
            // for d3 = 0, 1, 2 (d3 is a compile-time constant of the unrolled loop: the groups of six start at multiples of three),
            // so a tap costs ONE v_mad_u32_u24 and no branch.
            unsigned aB[MT][3], aK[MT][3];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const bool ok = (tmask[m] >> d) & 1u;
                    aB[m][d] = ok ? (unsigned)(im + abase[m]) : (unsigned)(h * 16);
                    aK[m][d] = ok ? 1u : 0u;
                }
            auto load_a = [&](auto d3c, int tap, half8(&a)[MT][4]) {
                constexpr int d3 = decltype(d3c)::value;            // == tap % 3
                const int dvb = (((tap / 9) * HP2 + (tap / 3) % 3) * p.D3 + d3) * R3L_VOX_BYTES;     // wave-uniform
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const char* row = lds + (aB[m][d3] + __umul24((unsigned)dvb, aK[m][d3]));
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        if (R3_ABLATE & 16) {
                            a[m][2 * i] = half8{(_Float16)i, 1, 2, 3, 4, 5, 6, 7};
                            a[m][2 * i + 1] = half8{(_Float16)dvb, 1, 2, 3, 4, 5, 6, 7};
                            continue;
                        }
                        a[m][2 * i] = *reinterpret_cast<const half8*>(row + i * 32);            // hi chunk 2 i + h
                        a[m][2 * i + 1] = *reinterpret_cast<const half8*>(row + i * 32 + 64);   // its lo chunk
                    }
                }
                __builtin_amdgcn_sched_barrier(0);      // the reads stay AHEAD of the previous tap's MFMAs (the scheduler had sunk
                                                        // them behind five of the six: one MFMA of cover for four ds_read_b128)
            };
            auto mma = [&](const half8(&a)[MT][4], const u32x4(&w)[4]) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const half8 bh = __builtin_bit_cast(half8, w[2 * i]), bl = __builtin_bit_cast(half8, w[2 * i + 1]);
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        if (R3_ABLATE & 2) {
                            acc[m][0] += (float)a[m][2 * i][0] + (float)a[m][2 * i + 1][1] + (float)bh[2] + (float)bl[3];
                            continue;
                        }
                        acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[m][2 * i + 1], bh, acc[m], 0, 0, 0);
                        acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[m][2 * i], bl, acc[m], 0, 0, 0);
                        acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[m][2 * i], bh, acc[m], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            using D0 = std::integral_constant<int, 0>;
            using D1 = std::integral_constant<int, 1>;
            using D2 = std::integral_constant<int, 2>;
            R3_MARK(4)                                     // tile decode
            if constexpr (!SINGLE) {
                load_w(0, wq0);
                load_w(1, wq1);
                load_a(D0{}, 0, a0);
    #pragma unroll 1
                for (int tap = 0; tap < 24; tap += 6) {        // weights rotate over three sets, operands over two: period 6
                    load_w(tap + 2, wq2); load_a(D1{}, tap + 1, a1); mma(a0, wq0);
                    load_w(tap + 3, wq0); load_a(D2{}, tap + 2, a0); mma(a1, wq1);
                    load_w(tap + 4, wq1); load_a(D0{}, tap + 3, a1); mma(a0, wq2);
                    load_w(tap + 5, wq2); load_a(D1{}, tap + 4, a0); mma(a1, wq0);
                    load_w(tap + 6, wq0); load_a(D2{}, tap + 5, a1); mma(a0, wq1);
                    load_w(tap + 7, wq1); load_a(D0{}, tap + 6, a0); mma(a1, wq2);
                }
                load_w(26, wq2); load_a(D1{}, 25, a1); mma(a0, wq0);   // tap 24
                load_a(D2{}, 26, a0); mma(a1, wq1);                    // tap 25
                mma(a0, wq2);                                          // tap 26
            } else {
                // One staged image, two tiles per wave: a fine-grained pipeline.  Every operand register is reloaded for its NEXT
                // use as soon as the three MFMAs that read it have been issued -- an operand quad (hi, lo of 16 channels of one tile)
                // is then nine MFMAs (288 matrix-core cycles) ahead of its use, a weight quad eighteen -- which takes one set of
                // operand registers and two of weight registers instead of two and three.
                u32x4 wr[2][4];                            // weights of two taps (set = tap & 1)
                half8 ar[MT][4];                        // operands of one tap
                // operand address of tile m at the current tap: zero block + (run[m] * aK): run[m] walks the 27 taps by THREE
                // wave-uniform steps (next temporal tap, next column, next row), so nothing per tap lives in scalar registers
                unsigned rowoff[MT], run[MT];
                const unsigned zoff = h * 16;
                const int step_t = R3L_VOX_BYTES, step_c = (p.D3 - 2) * R3L_VOX_BYTES,
                          step_r = ((HP2 - 2) * p.D3 - 2) * R3L_VOX_BYTES;
                auto ld_w = [&](int tap, int i) __attribute__((always_inline)) {
                    const int at = (tap * 2 + i) * 1024;
                    wr[tap & 1][2 * i] = __builtin_amdgcn_raw_buffer_load_b128(wsrd, wlane, at, 0);
                    wr[tap & 1][2 * i + 1] = __builtin_amdgcn_raw_buffer_load_b128(wsrd, wlane, at + R3_PLANE_HALVES * 2, 0);
                };
                auto set_row = [&](int m, int tap) __attribute__((always_inline)) {                 // tap 0 first, then every tap in order
                    if (tap == 0) run[m] = (unsigned)(im + abase[m]) - zoff;
                    else run[m] += (tap % 3) ? step_t : ((tap / 3) % 3) ? step_c : step_r;
                    rowoff[m] = zoff + __umul24(run[m], aK[m][tap % 3]);
                };
                auto ld_a = [&](int m, int i) __attribute__((always_inline)) {
                    const char* row = lds + rowoff[m];
                    ar[m][2 * i] = *reinterpret_cast<const half8*>(row + i * 32);
                    ar[m][2 * i + 1] = *reinterpret_cast<const half8*>(row + i * 32 + 64);
                };
                auto mma3 = [&](int m, int i, int tap) __attribute__((always_inline)) {
                    const half8 bh = __builtin_bit_cast(half8, wr[tap & 1][2 * i]);
                    const half8 bl = __builtin_bit_cast(half8, wr[tap & 1][2 * i + 1]);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar[m][2 * i + 1], bh, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar[m][2 * i], bl, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ar[m][2 * i], bh, acc[m], 0, 0, 0);
                };
                ld_w(0, 0); ld_w(0, 1); ld_w(1, 0); ld_w(1, 1);
#pragma unroll
                for (int m = 0; m < MT; ++m) { set_row(m, 0); ld_a(m, 0); ld_a(m, 1); }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int tap = 0; tap < 27; ++tap) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
#pragma unroll
                        for (int m = 0; m < MT; ++m) {
                            mma3(m, i, tap);
                            if (tap + 1 < 27) {
                                if (i == 0) set_row(m, tap + 1);
                                ld_a(m, i);
                            }
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        if (tap + 2 < 27) ld_w(tap + 2, i);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            R3_MARK(5)                                     // taps
            if (gi == ngrp - 1) taps_done();               // this wave's last read of image `it` has been issued

            // epilogue: C/D map col = lane&31 (cout), row = (r&3) + 8*(r>>2) + 4h (voxel inside the tile)
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                float tsum = 0.f;
                u32x4 rov[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) rov[j] = *reinterpret_cast<const u32x4*>(&rowtab[wave][m][8 * j + 4 * h]);   // rows 8 j + 4 h + 0..3
                float ax[16];
                if constexpr (AUX != 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int k = 0; k < 4; ++k)     // (a row past the patch or a channel >= cout: out of range, reads 0)
                            ax[4 * j + k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(asrd, (int)(rov[j][k] + lane_term), 0, 0));
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u32x4 ro = rov[j];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float o = fmaxf((acc[m][4 * j + k] * ua) * ub + bias, relu_floor);
                        if constexpr (AUX == 1) o += ax[4 * j + k];
                        if constexpr (AUX == 4) o = fmaf(o, gate_c, ax[4 * j + k]);     // (scale_residual_c32_kernel's expression)
                        if constexpr (AUX == 2) o = ax[4 * j + k] > 0.f ? o : 0.f;
                        if (!(R3_ABLATE & 32))
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o), ysrd, (int)(ro[k] + lane_term), 0, 0);
                        o = ro[k] < R3L_OOB ? o : 0.f;
                        tsum += o;
                        ymax = fmaxf(ymax, fabsf(o));
                    }
                }
                if (p.chan_slab) csum += tsum + __shfl_xor(tsum, 32, 64);
            }
        }
        R3_MARK(6)                                             // epilogue (+ the next patch's global loads, one image)
        if constexpr (SINGLE) {
            __syncthreads();                                   // every wave has read its last operand
            R3_MARK(0)
            if (next < npatch && !(R3_ABLATE & 64)) stage_commit(lds + R3L_IMG0);
            R3_MARK(1)
            __syncthreads();
            R3_MARK(3)
        }
    }
#ifdef R3_STAMPS
    if (p.stamps && lane == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) atomicAdd(&p.stamps[k], ph_[k]);
        atomicAdd(&p.stamps[8], 1ull);
    }
#endif
    if (p.chan_slab && lane < 32) p.chan_slab[((long long)b * gridDim.x * WAVES + blockIdx.x * WAVES + wave) * RC + lane] = csum;
    if (p.y_amax) r3_block_amax(l32 < p.cout ? ymax : 0.f, p.y_amax);
}

// =====================================================================================================================
// Two-pass form of the LDS-staged kernel: 8 waves x TWO tiles per wave, the input channels taken 16 at a time.
//
// conv3d_c32_lds_kernel<8, 1> needs 8 KB of operands per 6 MFMAs per wave -- LDS (128 B/clk) and L1 (64 B/clk) deliver
// that at about the rate the matrix cores consume it, and the weight stream alone measures 5 of 25 ms.  Two tiles per wave
// share every weight fragment (6 KB per 12 MFMAs), but 16 tiles need a 504-output patch whose 810-voxel halo does not fit
// LDS twice at 128 B per voxel.  Here the staged image holds ONE HALF of the input channels (64 B per voxel: hi/lo of 16
// channels, 51.8 KB), the 27 taps run once per half with the accumulators kept, and the two images alternate between
// "this half" and "the next half / the next patch's first half".  Per tap and wave: four ds_read_b128 (two tiles x hi, lo),
// two weight loads (1 KB each, shared by both tiles), six MFMAs.
// =====================================================================================================================
constexpr int R3L2_MAX_HVOX = 810;                 // voxels of one staged patch (10 x 9 x 9)
constexpr int R3L2_IMG_BYTES = R3L2_MAX_HVOX * 64;
constexpr int R3L2_STAGE_Q = (R3L2_MAX_HVOX * 4 + CONV_THREADS - 1) / CONV_THREADS;   // 16-byte units of a half image per thread

__global__ void __launch_bounds__(CONV_THREADS) conv3d_c32_lds2_kernel(const Conv3dLdsParams p) {
    constexpr int MT = 2;
    __shared__ __attribute__((aligned(16))) char img[2][R3L2_IMG_BYTES];
    __shared__ __attribute__((aligned(16))) char zeros[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l32 = lane & 31;
    const int b = blockIdx.y;
    const int HP1 = p.PO1 + 2, HP2 = p.PO2 + 2;
    const int hvox = HP1 * HP2 * p.D3;
    const int pvox = p.PO1 * p.PO2 * p.O3;
    const int ptiles = (pvox + 31) / 32;
    const int npatch = p.np1 * p.np2;
    if (tid < 16) reinterpret_cast<float*>(zeros)[tid] = 0.f;
    const int ka = h3_scale_exp(r3_slot_max(p.x_amax)), kb = h3_scale_exp(*p.w_amax);
    const float sa = h3_pow2(ka), ua = h3_pow2(-ka), ub = h3_pow2(-kb);
    const float bias = p.bias[l32];
    const float* xb = p.x + (long long)b * p.D1 * p.D2 * p.D3 * RC;
    const __amdgpu_buffer_rsrc_t wsrd =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(p.planes), 0, R3_LAYER_HALVES * 2, 0x00020000);
    const int wlane = (h * 256 + l32 * 8) * 2;
    float csum = 0.f, ymax = 0.f;

    // ---- staging of one channel half (ch = 0: channels 0-15, 1: 16-31) of a patch ---------------------------------------
    // image: 64 B per voxel = four 16-byte chunks: hi of channels 8c..8c+7 (c = 0, 1 within the half), then the two lo's;
    // chunk c of voxel v at slot c ^ ((v >> 2) & 3): the sixteen lanes of a ds_read_b128 phase read sixteen bank groups
    f32x4 sreg[R3L2_STAGE_Q];
    auto stage_load = [&](int patch, int ch) {
        const int o1_0 = (patch / p.np2) * p.PO1, o2_0 = (patch % p.np2) * p.PO2;
#pragma unroll
        for (int i = 0; i < R3L2_STAGE_Q; ++i) {
            const int u = tid + CONV_THREADS * i;
            const int hv = u >> 2, cc = u & 3;
            const int hq = r3_div(hv, p.mD3), t = hv - hq * p.D3, h1 = r3_div(hq, p.mHP2), h2 = hq - h1 * HP2;
            const int g1 = o1_0 - p.pad + h1, g2 = o2_0 - p.pad + h2;
            const bool in = hv < hvox && (unsigned)g1 < (unsigned)p.D1 && (unsigned)g2 < (unsigned)p.D2;
            sreg[i] = in ? *reinterpret_cast<const f32x4*>(xb + (((long long)g1 * p.D2 + g2) * p.D3 + t) * RC + 16 * ch + 4 * cc)
                         : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto stage_commit = [&](char* dst) {
#pragma unroll
        for (int i = 0; i < R3L2_STAGE_Q; ++i) {
            const int u = tid + CONV_THREADS * i;
            const int hv = u >> 2, cc = u & 3;
            if (hv < hvox) {
                half2v h0, l0, h1, l1;
                h3_split2(sreg[i][0], sreg[i][1], sa, h0, l0);
                h3_split2(sreg[i][2], sreg[i][3], sa, h1, l1);
                const int slot = (cc >> 1) ^ ((hv >> 2) & 3);
                char* at = dst + hv * 64 + (cc & 1) * 8;
                *reinterpret_cast<uint2*>(at + slot * 16) = uint2{__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1)};
                *reinterpret_cast<uint2*>(at + (slot ^ 2) * 16) =
                    uint2{__builtin_bit_cast(unsigned, l0), __builtin_bit_cast(unsigned, l1)};
            }
        }
    };

    int patch = blockIdx.x;
    if (patch < npatch) stage_load(patch, 0);
    __syncthreads();                                       // zeros[] visible
    if (patch < npatch) stage_commit(img[0]);
    __syncthreads();
    int cur = 0;                                           // image that holds the half about to be consumed
    for (; patch < npatch; patch += gridDim.x) {
        const int next = patch + gridDim.x;
        const int o1_0 = (patch / p.np2) * p.PO1, o2_0 = (patch % p.np2) * p.PO2;
        const int grp = wave;                              // tiles 2 wave, 2 wave + 1 (a patch has at most 16)
        int hv0[MT];
        unsigned tmask[MT];
        long long gofs[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int q = (grp * MT + m) * 32 + l32;
            const int qq = r3_div(q, p.mO3), t = q - qq * p.O3, q1 = r3_div(qq, p.mPO2), q2 = qq - q1 * p.PO2;
            const int o1 = o1_0 + q1, o2 = o2_0 + q2;
            const bool valid = q < pvox && o1 < p.O1 && o2 < p.O2;
            hv0[m] = (q1 * HP2 + q2) * p.D3 + t - p.pad;
            unsigned tm = 0;
#pragma unroll
            for (int d = 0; d < 3; ++d) tm |= ((unsigned)(t + d - p.pad) < (unsigned)p.D3) ? (1u << d) : 0u;
            tmask[m] = valid ? tm : 0u;
            gofs[m] = valid ? (((long long)b * p.O1 + o1) * p.O2 + o2) * p.O3 + t : -1ll;
        }
        const bool busy = grp * MT < ptiles;               // (waves beyond the patch's tiles only help with the staging)
        f32x16 acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

#pragma unroll 1
        for (int ch = 0; ch < 2; ++ch) {
            // the half consumed after this one: the patch's second half, or the next patch's first
            const bool more = ch == 0 || next < npatch;
            if (more) stage_load(ch == 0 ? patch : next, ch == 0 ? 1 : 0);
            const char* im = img[cur];
            if (busy) {
                u32x4 wq0[2], wq1[2], wq2[2];              // weights of three taps for this half: (hi, lo)
                auto load_w = [&](int tap, u32x4(&w)[2]) {
                    const int at = (tap * 2 + ch) * 1024 + wlane;
                    w[0] = __builtin_amdgcn_raw_buffer_load_b128(wsrd, at, 0, 0);
                    w[1] = __builtin_amdgcn_raw_buffer_load_b128(wsrd, at + R3_PLANE_HALVES * 2, 0, 0);
                };
                half8 a0[MT][2], a1[MT][2];             // operands of two taps: (hi, lo) per tile
                auto load_a = [&](int tap, half8(&a)[MT][2]) {
                    const int d3 = tap % 3;
                    const int dv = ((tap / 9) * HP2 + (tap / 3) % 3) * p.D3 + d3;
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        const int hv = hv0[m] + dv;
                        const bool ok = (tmask[m] >> d3) & 1u;
                        const char* row = ok ? im + hv * 64 : zeros;
                        const int slot = ok ? (h ^ ((hv >> 2) & 3)) : 0;
                        a[m][0] = *reinterpret_cast<const half8*>(row + slot * 16);
                        a[m][1] = *reinterpret_cast<const half8*>(row + (ok ? (slot ^ 2) : 0) * 16);
                    }
                };
                auto mma = [&](const half8(&a)[MT][2], const u32x4(&w)[2]) {
                    const half8 bh = __builtin_bit_cast(half8, w[0]), bl = __builtin_bit_cast(half8, w[1]);
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[m][1], bh, acc[m], 0, 0, 0);
                        acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[m][0], bl, acc[m], 0, 0, 0);
                        acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[m][0], bh, acc[m], 0, 0, 0);
                    }
                };
                load_w(0, wq0);
                load_w(1, wq1);
                load_a(0, a0);
#pragma unroll 1
                for (int tap = 0; tap < 24; tap += 6) {
                    load_w(tap + 2, wq2); load_a(tap + 1, a1); mma(a0, wq0);
                    load_w(tap + 3, wq0); load_a(tap + 2, a0); mma(a1, wq1);
                    load_w(tap + 4, wq1); load_a(tap + 3, a1); mma(a0, wq2);
                    load_w(tap + 5, wq2); load_a(tap + 4, a0); mma(a1, wq0);
                    load_w(tap + 6, wq0); load_a(tap + 5, a1); mma(a0, wq1);
                    load_w(tap + 7, wq1); load_a(tap + 6, a0); mma(a1, wq2);
                }
                load_w(26, wq2); load_a(25, a1); mma(a0, wq0);
                load_a(26, a0); mma(a1, wq1);
                mma(a0, wq2);
            }
            if (more) stage_commit(img[cur ^ 1]);
            __syncthreads();
            cur ^= 1;
        }

        if (busy) {
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                float tsum = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = mfma32_acc_row(r, h);
                    const long long vo = __shfl(gofs[m], row, 64);
                    float o = (acc[m][r] * ua) * ub + bias;
                    if (p.relu) o = fmaxf(o, 0.f);
                    if (vo >= 0) {
                        tsum += o;
                        if (l32 < p.cout) {
                            p.y[vo * p.y_cstride + l32] = o;
                            ymax = fmaxf(ymax, fabsf(o));
                        }
                    }
                }
                if (p.chan_slab) csum += tsum + __shfl_xor(tsum, 32, 64);
            }
        }
    }
    if (p.chan_slab && lane < 32) p.chan_slab[((long long)b * gridDim.x * 8 + blockIdx.x * 8 + wave) * RC + lane] = csum;
    if (p.y_amax) r3_block_amax(ymax, p.y_amax);
}
