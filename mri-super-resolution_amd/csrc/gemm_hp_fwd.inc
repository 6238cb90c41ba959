// Cross-layer fused forward of a whole SIREN on pre-split (HL32) operands -- the inference / dense re-sampling path
// (inr_siren_forward, inr_siren_reconstruct: superresDWI.py:125-126,161-162).  Included by gemm_hp.hip behind gemm_hp.inc.
//
// The layer-wise forward writes every activation matrix to HBM and reads it back for the next layer: at hidden = 512 that is
// 4 KB per row and layer in, 4 KB out -- ~19 KB per voxel over Siren(256,512,3,1), 2.7 TB/s at the 142 M voxels/s it reached,
// with the matrix cores a third busy.  Nothing but the next layer ever reads those matrices, so here they never leave the CU:
//   * one 8-wave block owns a PANEL of 64 rows and walks it through ALL sine layers and the head;
//   * the panel lives in LDS as the A-operand image of gemm_hp.inc ([k-block][row][128 B HL32 line], slot-swizzled):
//     64 rows x 512 columns x 4 B = 128 KB, overwritten in place by each layer's output (every wave holds its 64 x (H/8)
//     slice of the output in accumulators until all waves are done reading);
//   * the B operand (this layer's HL32 weights, 1 MB at 512 x 512) is NOT staged: each lane loads its MFMA fragments straight
//     from global memory -- they are L2 residents, every panel of every CU re-reads them -- one K-tile ahead of the MFMAs
//     (8 x 16 B per lane and K-tile; 64 KB per K-tile and CU against 1,536 MFMA cycles = 42 B/clk of the CU's 64);
//   * the epilogue is the persistent kernels': bias through the accumulators' start value, chunk-wise through a per-wave 2 KB
//     staging area, sin on the transcendental unit, hi/lo split -- but the 16-byte pieces go to the panel, not to HBM; the last
//     layer feeds the head's row dots directly and only y (4 B per row) is stored.
// HBM traffic per row: the HL32 input features in (1 KB at 256 features), 4 B out; 86 k MFMA cycles per panel at
// Siren(256,512,3,1).
//
// MEASURED (round 3, dense x4 re-sampling of the synthetic 128^3, 8.4 M voxels, tools/recon_time.py): 71-72 ms = 117 M voxels/s
// against 58 ms = 144 M voxels/s for the layer-wise launches -- SLOWER, with the fragments requested one or two K-tiles ahead
// alike (not latency).  What the fusion trades: 19 KB per voxel of HBM traffic for 55 KB per voxel of weight traffic out of
// L2 (3.5 MB of HL32 weights per 64-row panel; LDS cannot hold a taller panel at 4 bytes per element), delivered as
// 16-byte-per-lane fragment loads that touch sixteen half lines each; the CUs receive them at ~26 GB/s each (6.6 TB/s chip-wide),
// a third of what the matrix cores would consume.  The study's answer is therefore NO for hidden = 512 on this part; the
// kernel stays selectable (inr_debug_set(19, 1)) and tested, the layer-wise launches stay the default.
//
// Arithmetic is the layer-wise path's (same three products per K-tile in pkd order, same folded bias, same sin, same split,
// head on hi + lo): results agree with it to the last bits of the fp32 head sum, and a row's value depends on nothing but
// the row (chunk invariance of the re-sampling holds by construction: every row takes this kernel).
constexpr int FW_ROWS = 64, FW_NTH = 512, FW_MAX_LAYERS = 8;
constexpr int FW_KB_BYTES = FW_ROWS * 128;          // one k-block of the panel image: 64 rows x 128 B

struct FwLayer {
    const char* W;          // HL32 [out = H][in = K]
    const float* bias;      // [H]
    const unsigned* w_amax; // scale slot of W
    int K;
    float omega;
};
struct FwParams {
    FwLayer layer[FW_MAX_LAYERS];
    int n_sine, H;
    const char* x;          // HL32 [n][F]
    const unsigned* x_amax; // scale slot of x
    long long n;
    const float* head_W;    // [H]
    const float* head_b;    // [1] (nullable)
    float* y;               // [n]
    int use_clamp;
    float clamp_min;
};

__device__ __forceinline__ float fw_sin_fast(float x) {   // the sin half of sincos_f32x2_fast (common.h)
    const float k = rintf(x * INR_INV_2PI_HI);
    float f = fmaf(x, INR_INV_2PI_HI, -k);
    f = fmaf(x, INR_INV_2PI_LO, f);
    return __builtin_amdgcn_sinf(f);
}

// NJ = 16-column MFMA tiles per wave = H / 128: 4 (H = 512), 2 (H = 256)
template <int NJ>
__global__ void __launch_bounds__(FW_NTH, 2) siren_fwd_fused_kernel(const FwParams p) {
    constexpr int H = 128 * NJ, WCOLS = 16 * NJ;              // columns a wave owns
    constexpr int PANEL = (H / 32) * FW_KB_BYTES;             // bytes (input features need F <= H: host checks)
    __shared__ __attribute__((aligned(1024))) char smem[PANEL + 8 * HP_EPI_WAVE + 8 * FW_ROWS * 4];
    char* const P = smem;
    float* const red = reinterpret_cast<float*>(smem + PANEL + 8 * HP_EPI_WAVE);     // [8 waves][64 rows] head partials

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, l16 = lane & 15;
    const int fx = (g ^ hp_f(l16)) << 4;
    const int fa_hi = l16 * 128 + fx, fa_lo = fa_hi ^ 64;     // + 16 i rows (2048 B), + kb * FW_KB_BYTES
    float* const stg = reinterpret_cast<float*>(smem + PANEL + wave * HP_EPI_WAVE);
    const int er = lane >> 2, ec = (lane & 3) * 8;            // epilogue: row er of a 16-row chunk, columns ec .. ec + 7

    const long long panels = (p.n + FW_ROWS - 1) / FW_ROWS;
    const int F = p.layer[0].K;
    for (long long panel = blockIdx.x; panel < panels; panel += gridDim.x) {
        const long long r0 = panel * FW_ROWS;
        // ---- input panel: HL32 lines of 64 rows x F / 32 k-blocks by LDS-DMA (one transfer = 8 rows of one k-block) ----------
        {
            const long long rows_left = p.n - r0;
            const __amdgpu_buffer_rsrc_t srdX =
                hp_srd(p.x + r0 * (long long)F * 4, (rows_left < FW_ROWS ? rows_left : FW_ROWS) * (long long)F * 4);
            const int transfers = (F / 32) * 8;               // rows past the end read zeros (SRD bound)
            for (int q = wave; q < transfers; q += 8) {
                const int kb = q >> 3, rb = q & 7;
                const int row = 8 * rb + (lane >> 3);
                const int c = (lane & 7) ^ hp_f(row);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(srdX, (__attribute__((address_space(3))) void*)(P + kb * FW_KB_BYTES + rb * 1024),
                                                         16, row * F * 4 + c * 16, kb * 128, 0, 0);
            }
            __builtin_amdgcn_s_waitcnt(hp_vmcnt(0));
            __syncthreads();
        }
        float head_part[4] = {0.f, 0.f, 0.f, 0.f};            // rows 16 i + er of this wave's columns (last layer)
        for (int l = 0; l < p.n_sine; ++l) {
            const FwLayer L = p.layer[l];
            const int ktiles = L.K / 32;
            const int ka = l == 0 ? h3_scale_exp(*p.x_amax) : 0, kb_ = h3_scale_exp(*L.w_amax);
            // B fragments of this wave's columns straight from global memory: lane (l16, g) of tile j holds
            // W[64 w' + 16 j + l16][32 kt + 8 g .. + 7] -- 16 contiguous bytes of the HL32 line (hi), + 64 (lo)
            const __amdgpu_buffer_rsrc_t srdW = hp_srd(L.W, (long long)H * L.K * 4);
            const int vb = ((WCOLS * wave + l16) * L.K) * 4 + g * 16;
            half8 bh[3][NJ], bl[3][NJ];      // three rotating sets: the fragments of K-tile kt + 2 are requested before the MFMAs of kt
            auto load_b = [&](int set, int kt) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    bh[set][j] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(srdW, vb + j * 16 * L.K * 4, kt * 128, 0));
                    bl[set][j] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(srdW, vb + j * 16 * L.K * 4 + 64, kt * 128, 0));
                }
            };
            f32x4v acc[4][NJ];
            {
                const float up = h3_pow2(ka) * h3_pow2(kb_);
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const float b = L.bias ? L.bias[WCOLS * wave + 16 * j + l16] * up : 0.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i][j] = f32x4v{b, b, b, b};
                }
            }
            load_b(0, 0);
            if (ktiles > 1) load_b(1, 1);
            auto ktile = [&](auto set_c, int kt) {
                constexpr int SET = decltype(set_c)::value;
                if (kt + 2 < ktiles) load_b((SET + 2) % 3, kt + 2);
                const char* A = P + kt * FW_KB_BYTES;
                half8 ah[4], al[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ah[i] = *reinterpret_cast<const half8*>(A + fa_hi + i * 2048);
                    al[i] = *reinterpret_cast<const half8*>(A + fa_lo + i * 2048);
                }
                // the three products in the order of gemm_hp_pkd_kernel: hi x lo, hi x hi, lo x hi
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl[SET][j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh[SET][j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh[SET][j], acc[i][j], 0, 0, 0);
            };
            using S0 = std::integral_constant<int, 0>;
            using S1 = std::integral_constant<int, 1>;
            using S2 = std::integral_constant<int, 2>;
            int kt = 0;
            for (; kt + 2 < ktiles; kt += 3) {
                ktile(S0{}, kt);
                ktile(S1{}, kt + 1);
                ktile(S2{}, kt + 2);
            }
            if (kt < ktiles) ktile(S0{}, kt);
            if (kt + 1 < ktiles) ktile(S1{}, kt + 1);
            __syncthreads();      // every wave is done reading the panel: it may be overwritten

            // ---- epilogue: 16 x 32 chunks through the wave's staging area; sin; HL32 pieces into the panel (or the head dot) ----
            const float inv_a = h3_pow2(-ka), inv_b = h3_pow2(-kb_);
            const bool last = l == p.n_sine - 1;
            constexpr int NCH = 4 * (NJ / 2);                 // chunks: 4 row blocks x NJ / 2 column blocks of 32
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int i = c & 3, jp = c >> 2;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) stg[(4 * g + r) * 32 + jj * 16 + l16] = acc[i][2 * jp + jj][r] * inv_a * inv_b;
                __builtin_amdgcn_s_waitcnt(0xC07F);
                __builtin_amdgcn_wave_barrier();
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(stg + er * 32 + ec);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(stg + er * 32 + ec + 4);
                __builtin_amdgcn_s_waitcnt(0xC07F);
                __builtin_amdgcn_wave_barrier();
                float sv[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    sv[e] = fw_sin_fast(L.omega * v0[e]);
                    sv[4 + e] = fw_sin_fast(L.omega * v1[e]);
                }
                u32x4 hi, lo;
                hp_split8_unit(sv, hi, lo);
                const int row = 16 * i + er;
                if (!last) {
                    const int col = WCOLS * wave + 32 * jp + ec;                 // first of the lane's 8 columns
                    char* line = P + (col >> 5) * FW_KB_BYTES + row * 128;
                    const int q = (col & 31) >> 3;
                    *reinterpret_cast<u32x4*>(line + ((q ^ hp_f(row)) << 4)) = hi;
                    *reinterpret_cast<u32x4*>(line + (((q + 4) ^ hp_f(row)) << 4)) = lo;
                } else {   // head: y = a . w + b on hi + lo, as hp_head_forward_kernel reads them
                    const half8 h8 = __builtin_bit_cast(half8, hi), l8 = __builtin_bit_cast(half8, lo);
                    const float* w = p.head_W + WCOLS * wave + 32 * jp + ec;
                    float d = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) d = fmaf((float)h8[e] + (float)l8[e], w[e], d);
                    head_part[i] += d;
                }
            }
            if (!last) __syncthreads();                       // the new panel is complete
        }
        // ---- head: fold the 4 lanes of a row, then the 8 waves (fixed order), bias, clamp, store ---------------------------------
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float d = head_part[i];
            d += __shfl_xor(d, 1, 64);
            d += __shfl_xor(d, 2, 64);
            if ((lane & 3) == 0) red[wave * FW_ROWS + 16 * i + er] = d;
        }
        __syncthreads();
        if (tid < FW_ROWS) {
            float s = ((red[tid] + red[FW_ROWS + tid]) + (red[2 * FW_ROWS + tid] + red[3 * FW_ROWS + tid])) +
                      ((red[4 * FW_ROWS + tid] + red[5 * FW_ROWS + tid]) + (red[6 * FW_ROWS + tid] + red[7 * FW_ROWS + tid]));
            s += p.head_b ? p.head_b[0] : 0.f;
            if (p.use_clamp) s = fmaxf(s, p.clamp_min);
            if (r0 + tid < p.n) p.y[r0 + tid] = s;
        }
        __syncthreads();                                      // red / the panel are free for the next panel
    }
}
