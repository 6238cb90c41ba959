// Pre-split fp16 MFMA GEMM ("hp"): the split-fp16 arithmetic of gemm_h3.inc with every operand ALREADY split in HBM, staged
// global -> LDS by buffer_load ... lds (no staging registers, no split VALU, no ds_write in the K-loop).  Included by
// gemm_hp.hip; the format's helpers are in split_fp16.h.
//
// HL32 storage of a matrix X[R][C] (C % 32 == 0): row r, 32-column block kb occupies the 128 bytes at
// (r * C/32 + kb) * 128: halves hi(X[r][32kb .. 32kb+31]) then lo(...), hi = fp16(x * s) rounded to nearest,
// lo = fp16(x * s - hi) -- the same two halves gemm_h3.inc forms on the fly.  4 bytes per element, the row pitch of the
// fp32 matrix; a product costs three v_mfma_f32_16x16x32_f16 (hi*lo, lo*hi, hi*hi), fp32 accumulate.  Producers write it
// from their epilogues (sine layers: act; input-grad / head: dz, scaled by a power of two from an a-priori BOUND of the
// tensor -- see hp_scale_exp), weights and the network input are converted once per step / per call.
//
// One 512-thread block (2 x 4 waves, each 64 x 64 of a 128 x 256 tile) per CU, three 48 KB LDS stages.
//   KC operands (contraction index contiguous: forward, input-grad): a stage row is the 128-byte HL32 line of one
//     (row, kb); one LDS-DMA instruction moves 8 whole lines.  16-byte slot c (0-3: hi octets, 4-7: lo octets) of row r
//     sits at slot c ^ f(r), f = [0,1,5,4,7,6,2,3][(r >> 1) & 7]: every ds_read_b128 lane group of gfx950
//     ({0-3,12-15,20-27}, ...: MI355X_MICROARCH.md) then covers the 16 slots of its 256-byte window exactly once.
//   RC operands (contraction over the ROWS: parameter gradient): a stage row is one matrix row's 512 / 1024 bytes of the
//     tile's columns; 32-byte chunk ch sits at ch ^ f2(r) (low three bits), f2 = (r & 3) | ((r >> 3) & 1) << 2, and the
//     fragments come out of ds_read_b64_tr_b16 (4 rows x 16 columns transposed per 16 lanes), conflict-free.
// K-loop, tile t in stage t % 3, 48 MFMAs per wave:
//   X: hi(A) x lo(B)   | fragment reads lo(A), hi(B) of tile t
//   Y: lo(A) x hi(B)   | then s_waitcnt vmcnt(6) (this wave's transfers of tile t+1 have landed; tile t+2 stays in
//                        flight) and the ONE barrier of the iteration: tile t+1 visible, nobody reads stage t % 3 any more
//   Z: hi(A) x hi(B)   | LDS-DMA of tile t+3 into stage t % 3; fragment reads hi(A) (second register set), lo(B) of t+1
__device__ __forceinline__ int hp_f(int r) {   // KC slot permutation
    const int p = (r >> 1) & 7;
    return (p & 1) ^ (((p >> 1) & 1) * 5) ^ (((p >> 2) & 1) * 7);
}
__device__ __forceinline__ int hp_f2(int r) { return (r & 3) | (((r >> 3) & 1) << 2); }

// Cache policy (buffer instruction aux bits; 2 = nt) of the operand transfers.  Round 4, interleaved A/B of the short bench on two boxes
// (tools/nt_ab.sh, profiles/r04_nt_ab.txt): the A operand of the deferred-epilogue kernel -- an activation panel streamed from HBM,
// read by the two column tiles of its rows and never again in the launch -- non-temporal: forward launch 0.782 -> 0.766 ms (-2 %),
// input-grad -0.6 %, step 8.69 -> 8.65 ms in every round (MI355X_MICROARCH.md, nt-weights: a once-read stream lands sooner and leaves
// the L2 to the weight panel).  NOT the parameter-gradient kernel's operands (each read by 2 / 4 tiles through L2: both nt = +12 % on
// that kernel, the dz operand alone = no change) and not the epilogue's once-read element-wise factor (+1.7 % on input-grad).
#ifndef HP_A_AUX
#define HP_A_AUX 2     // (-DHP_A_AUX=0: the default policy, as through round 3)
#endif
#ifndef HP_HEAD_NT
#define HP_HEAD_NT 0   // diagnostic builds: 1 = the head step reads z and writes dz non-temporal (both once-touched streams): measured
                       // +0.05 ms on the head step, -0.01 on the GEMMs behind it (profiles/r04_nt_ab.txt): off
#endif
#ifndef HP_RC_A_AUX
#define HP_RC_A_AUX 0  // diagnostic builds: cache policy of the row-contraction (parameter-gradient) kernel's operand transfers
#endif
#ifndef HP_RC_B_AUX
#define HP_RC_B_AUX 0
#endif
#ifndef HP_MUL_AUX
#define HP_MUL_AUX 0   // diagnostic builds: cache policy of the deferred epilogue's once-read element-wise factor (2 = nt)
#endif
#ifndef HP_COLSUM_TRANSPOSED
#define HP_COLSUM_TRANSPOSED 1   // gemm_hp_pkd_kernel<HPE_MUL>: column sums by a butterfly that halves the columns per stage (0: the A/B partner)
#endif
#ifndef HP_HEAD_PREFETCH
#define HP_HEAD_PREFETCH 1   // hp_head_step_kernel: the next row's loads are issued before the current row's arithmetic
#endif
#ifndef HP_UNSCALE_LDEXP
#define HP_UNSCALE_LDEXP 1   // gemm_hp_pkd_kernel: un-scale the parked accumulators with one v_ldexp_f32 (0: two v_mul_f32, the A/B partner)
#endif
#ifndef HP_DIAG_NO_OMEGA_STASH
#define HP_DIAG_NO_OMEGA_STASH 0   // diagnostic builds (results are WRONG): the deferred sine epilogue stashes cos instead of omega * cos -- the
                                   // time an omega folded into the backward weight image could save at best (round 5, profiles/r05_headline_ab.txt)
#endif
#ifndef HP_ABLATE
#define HP_ABLATE 0   // diagnostic builds (-DHP_ABLATE=bits; results are garbage): 1 no LDS-DMA in the K-loop, 2 no MFMA, 4 no
                      // epilogue work, 8 no fragment reads.  Compile-time: a run-time branch would split scheduling regions.
#endif
enum HpMode { HP_KC = 0, HP_RC = 1 };
enum HpEpi { HPE_SINE = 0, HPE_SINE_STASH = 1, HPE_MUL = 2, HPE_SLAB = 3, HPE_Z = 4, HPE_HEAD = 5 };
// HPE_HEAD (gemm_hp_row_kernel only, round 5): the last sine layer of a fit step WITH the head step in its epilogue -- the block owns whole
// rows, so y_n = sum_k sin(omega z_nk) w_k + b is complete inside it: residual, g = dL/dy, dz_L = g w omega cos (HL32, the only matrix the
// launch writes), the bias / head-weight gradient slabs and the loss partials.  No z round trip, no head step kernel.
// HPE_Z (gemm_hp_pkd_kernel only): the last sine layer of a fit step.  Its output feeds nothing but the head, so the
// epilogue stores the pre-activation z + b as ONE fp32 matrix (into the bytes of `dact`) and the head step forms
// sin / cos itself: 2 matrices written + 2 read become 1 + 1 (hp_head_step_kernel<CPL, true>).

__device__ __forceinline__ int hp_scale_exp(const HpScale& s) {
    if (s.mul == 0.f) return 0;
    float b = s.mul;
    if (s.meas) b *= __uint_as_float(*s.meas);
    if (s.wn) b *= *s.wn;
    if (!s.wn) return h3_scale_exp(__float_as_uint(b));   // inputs, weights: |k| <= 100 (their 2^k multiplies the bias fold)
    // gradients (bound = measured maximum x weight norm): the whole normal range -- a dz of 1e-32 three layers below a head
    // with 1e-23 weights kept 10 bits under the +-100 clamp (tests/test_gpu_hp_variants.py: weight magnitudes)
    return h3_scale_exp(__float_as_uint(b), s.kmax, -126);
}

// atomic max on the float bits of a non-negative value, skipped when the slot already holds at least as much.  The slot only
// grows, so a stale read costs an unnecessary atomic, never a lost maximum -- and all but the first few waves of a launch skip
// it: a thousand same-address atomics at the end of a 10 us kernel were half of its time (profiles/r03_small_n.txt).
__device__ __forceinline__ void hp_atomic_max_bits(unsigned* slot, float v) {
    const unsigned b = __float_as_uint(v);
    if (b > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, b);
}

struct HpParams {
    const char* A;          // HL32
    const char* B;          // HL32
    int M, N, K;            // KC: C[M][N] = A[M][K] B[N][K]^T.  RC: C[M][N] = sum_k A[k][M] B[k][N] (K = rows)
    long long pitchA, pitchB;   // bytes per matrix row
    long long a_rows, b_rows;   // matrix rows (SRD bounds)
    HpScale sa, sb, so;         // operand scales, output scale (HPE_MUL)
    // outputs
    char* C_hl;             // HPE_SINE*: act (HL32, pitch N*4); HPE_MUL: dz_prev (HL32, in place over `mul`)
    float* C2;              // HPE_SINE_STASH: dact fp32 [M][N]; HPE_SLAB: slabs [splits][M][N]
    const float* bias;      // HPE_SINE*
    const float* mul;       // HPE_MUL: fp32 [M][N]
    float* colsum;          // HPE_MUL: [2 * tiles_m][N] per-64-row column sums (nullable)
    unsigned* amax_out;     // HPE_MUL: atomic max of |dz_prev| (float bits), nullable
    float omega;
    int tiles_m, tiles_n, splits;
    int k_per_split;        // multiple of 32
    long long slab_stride;  // floats
    int reverse_m;
    int fold_bias;          // gemm_hp_nt_kernel: 1 = the bias enters through the accumulators' start value (as in the persistent
                            // kernels), 0 = it is added in the epilogue (as in gemm_hp_kernel) -- bit-for-bit like the wide kernel
                            // that serves the same K, so that a row's value does not depend on which kernel took it
    int stagger;            // persistent kernels: blocks start (blockIdx % 8) * stagger * 64 cycles apart, so that the CUs do not
                            // reach their (HBM-write-bound) epilogues all at once; 0 = off
    unsigned long long* stamps;   // diagnostic builds (-DINR_STAMPS): 16 x u64 per wave
    // HPE_HEAD: the head (out_features == 1) and the loss.  dz_L goes to C_hl (scale `so`), its column sums to `colsum`, max|dz| to `amax_out`
    const float* head_w;     // [N]
    const float* head_b;     // [1], nullable
    const float* target;     // [M]
    const float* tweight;    // [M], nullable
    float inv_count;
    float* slab_w;           // [2 * tiles_m][N]: per 64-row half panel, sum_n g_n sin(.)_nk
    float* part_loss;        // [2 * tiles_m]
    float* part_g;           // [2 * tiles_m]
};

#ifdef INR_STAMPS
#define HP_STAMP(slot)                                                                                  \
    do {                                                                                                \
        if (p.stamps && (threadIdx.x & 63) == 0) {                                                      \
            unsigned long long t_;                                                                      \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                  \
            p.stamps[((long long)blockIdx.x * 8 + (threadIdx.x >> 6)) * 16 + (slot)] = t_;               \
        }                                                                                               \
    } while (0)
#else
#define HP_STAMP(slot)
#endif

constexpr int HP_BM = 128, HP_BN = 256, HP_BK = 32, HP_NTH = 512;
constexpr int HP_A_IMG = 16384, HP_B_IMG = 32768, HP_STAGE = HP_A_IMG + HP_B_IMG, HP_NSTAGE = 3;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t hp_srd(const void* base, long long bytes) {
    if (bytes < 0) bytes = 0;
    if (bytes > 0xFFFFFFFFll) bytes = 0xFFFFFFFFll;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)(unsigned)bytes, 0x00020000);
}

// two transposed 4 x 16 blocks (rows r .. r+3 and r+4 .. r+7 of a [rows][ROWB bytes] image): lane i of each 16-lane group
// receives column i of the eight rows = one MFMA operand fragment.  Inline asm on purpose: behind an LDS-DMA in flight hipcc
// (ROCm 7.2) puts `s_waitcnt vmcnt(0)` in front of the __builtin_amdgcn_ds_read_tr16_b64 form (it cannot tell the read
// from the DMA's destination), which serialised every K-tile on the memory latency (0.84 -> 0.4 ms per launch).  The
// compiler does not count these reads in lgkmcnt: every consumer sits behind an explicit s_waitcnt lgkmcnt(0).
template <int ROWB>
__device__ __forceinline__ half8 hp_tr_read2(const char* lds) {
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    u32x2 a, b;
    const unsigned addr = (unsigned)(unsigned long long)(__attribute__((address_space(3))) const char*)lds;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(a) : "v"(addr));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(b) : "v"(addr), "n"(4 * ROWB));
    return __builtin_bit_cast(half8, u32x4{a[0], a[1], b[0], b[1]});
}


// Element-wise product of an input-gradient epilogue and its running column sum (the bias gradient), with the product ROUNDED before it is
// added: left to the compiler, `cs += a * b` becomes an fma in one kernel and a multiply + add in another (round 5: the row-owning kernel
// and the deferred one disagreed in the last bit of ~100 of 512 bias gradients).  Every HPE_MUL epilogue goes through here.
__device__ __forceinline__ f32x4 hp_mul_sum(const f32x4& a, const f32x4& b, f32x4& cs) {
#pragma clang fp contract(off)
    const f32x4 o = a * b;
    cs = cs + o;
    return o;
}

__device__ __forceinline__ void hp_split8(const float (&v)[8], float s, u32x4& hi, u32x4& lo) {
    half2v h[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) h3_split2<true>(v[2 * e], v[2 * e + 1], s, h[e], l[e]);
    hi = __builtin_bit_cast(u32x4, h);
    lo = __builtin_bit_cast(u32x4, l);
}
__device__ __forceinline__ void hp_split8_unit(const float (&v)[8], u32x4& hi, u32x4& lo) {
    half2v h[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) h3_split2<false>(v[2 * e], v[2 * e + 1], 1.f, h[e], l[e]);
    hi = __builtin_bit_cast(u32x4, h);
    lo = __builtin_bit_cast(u32x4, l);
}

// (the body takes its block index as an argument: gemm_hp_rc_multi_kernel below runs several of these GEMMs in one launch)
template <int MODE, int EPI>
__device__ __forceinline__ void gemm_hp_body(const HpParams& p, const int block_x) {
    constexpr int EPI_BYTES = 8 * 64 * SUB16 * 4;
    constexpr int SMEM_BYTES = HP_NSTAGE * HP_STAGE > EPI_BYTES ? HP_NSTAGE * HP_STAGE : EPI_BYTES;
    __shared__ __attribute__((aligned(1024))) char smem[SMEM_BYTES];
    constexpr bool KC = MODE == HP_KC;
    constexpr int A_ROWB = KC ? 128 : 512, B_ROWB = KC ? 128 : 1024;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int g = lane >> 4, l16 = lane & 15;

    // ---- tile decode (XCD-aware: logical neighbours -- which share the A panel -- on one XCD) -------------------------
    const int total = p.tiles_m * p.tiles_n * p.splits;
    int logical = xcd_remap(block_x, total);
    int tile_n = logical % p.tiles_n;
    logical /= p.tiles_n;
    int tile_m = logical % p.tiles_m;
    int split = logical / p.tiles_m;
    if (p.reverse_m) {
        if (p.splits > 1) split = p.splits - 1 - split;
        else tile_m = p.tiles_m - 1 - tile_m;
    }
    const int m0 = tile_m * HP_BM, n0 = tile_n * HP_BN;
    const int k_begin = split * p.k_per_split;
    const int k_end = min(p.K, k_begin + p.k_per_split);
    const int ktiles = (k_end - k_begin + HP_BK - 1) / HP_BK;

    // ---- operand windows and this wave's six LDS-DMA transfers per stage -----------------------------------------------
    __amdgpu_buffer_rsrc_t srdA, srdB;
    int step_a, step_b;   // soffset increment per K-tile
    if (KC) {
        srdA = hp_srd(p.A + (long long)m0 * p.pitchA, (p.a_rows - m0) * p.pitchA);
        srdB = hp_srd(p.B + (long long)n0 * p.pitchB, (p.b_rows - n0) * p.pitchB);
        step_a = step_b = 128;
    } else {
        const long long ra = min((long long)(k_end - k_begin), p.a_rows - k_begin);
        srdA = hp_srd(p.A + (long long)k_begin * p.pitchA + (m0 >> 5) * 128, ra * p.pitchA - (m0 >> 5) * 128);
        srdB = hp_srd(p.B + (long long)k_begin * p.pitchB + (n0 >> 5) * 128, ra * p.pitchB - (n0 >> 5) * 128);
        step_a = (int)(32 * p.pitchA);
        step_b = (int)(32 * p.pitchB);
    }
    int vdma[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int q = wave + 8 * i;   // i < 2: A image, else B image
        if (KC) {
            const int row = 8 * (i < 2 ? q : q - 16) + (lane >> 3);
            const int c = (lane & 7) ^ hp_f(row);
            vdma[i] = row * (int)(i < 2 ? p.pitchA : p.pitchB) + c * 16;
        } else if (i < 2) {
            const int row = 2 * q + (lane >> 5), u = lane & 31;
            const int ch = (u >> 1) ^ hp_f2(row);
            vdma[i] = row * (int)p.pitchA + ch * 32 + (u & 1) * 16;
        } else {
            const int row = q - 16, u = lane;
            const int ch = (u >> 1) ^ hp_f2(row);
            vdma[i] = row * (int)p.pitchB + ch * 32 + (u & 1) * 16;
        }
    }
    int soff_a = KC ? (k_begin >> 5) * 128 : 0, soff_b = soff_a;
    // third `part` (0: the two A transfers, 1 / 2: two B transfers each) of one K-tile into `stage`; part 2 advances the source
    auto dma_part = [&](int stage, int part) {
        char* S = smem + stage * HP_STAGE;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if ((i >> 1) != part) continue;
            const int q = wave + 8 * i;
            if (!KC && i < 2)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(srdA, (__attribute__((address_space(3))) void*)(S + q * 1024), 16, vdma[i],
                                                         soff_a, 0, HP_RC_A_AUX);
            else if (!KC)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(srdB, (__attribute__((address_space(3))) void*)(S + q * 1024), 16, vdma[i],
                                                         soff_b, 0, HP_RC_B_AUX);
            else
                __builtin_amdgcn_raw_ptr_buffer_load_lds(i < 2 ? srdA : srdB, (__attribute__((address_space(3))) void*)(S + q * 1024),
                                                         16, vdma[i], i < 2 ? soff_a : soff_b, 0, 0);
        }
        if (part == 2) {
            soff_a += step_a;
            soff_b += step_b;
        }
    };
    auto dma = [&](int stage) {
        dma_part(stage, 0);
        dma_part(stage, 1);
        dma_part(stage, 2);
    };

    // ---- fragment addresses ---------------------------------------------------------------------------------------------
    int fa[KC ? 2 : 8], fb[KC ? 2 : 8];
    if (KC) {
        const int fx = (g ^ hp_f(l16)) << 4;
        fa[0] = (64 * wm + l16) * 128 + fx;
        fa[1] = fa[0] ^ 64;
        fb[0] = HP_A_IMG + (64 * wn + l16) * 128 + fx;
        fb[1] = fb[0] ^ 64;
    } else {
        const int q = l16 >> 2, p4 = l16 & 3, row = 8 * g + q, f2 = hp_f2(row);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int lo = 0; lo < 2; ++lo) {
                const int mi = 4 * wm + t, ca = 4 * (mi >> 1) + (mi & 1) + 2 * lo;
                fa[2 * t + lo] = row * 512 + (ca ^ f2) * 32 + p4 * 8;
                const int ni = 4 * wn + t, cb = 4 * (ni >> 1) + (ni & 1) + 2 * lo;
                fb[2 * t + lo] = HP_A_IMG + row * 1024 + (cb ^ f2) * 32 + p4 * 8;
            }
    }
    auto frag_a = [&](const char* S, int i, int lo) -> half8 {
        if (KC) return *reinterpret_cast<const half8*>(S + fa[lo] + i * 2048);
        return hp_tr_read2<512>(S + fa[2 * i + lo]);
    };
    auto frag_b = [&](const char* S, int i, int lo) -> half8 {
        if (KC) return *reinterpret_cast<const half8*>(S + fb[lo] + i * 2048);
        return hp_tr_read2<1024>(S + fb[2 * i + lo]);
    };

    f32x4v acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4v{0.f, 0.f, 0.f, 0.f};
    half8 ah[2][4], bh[2][4], al[4], bl[4];

    // ---- prologue: three tiles in flight, wait for the first, fetch all of its fragments ---------------------------------
    HP_STAMP(0);
    if (ktiles > 0) dma(0);
    if (ktiles > 1) dma(1);
    if (ktiles > 2) dma(2);
    if (ktiles > 2) __builtin_amdgcn_s_waitcnt(0x0F70 | 12);
    else if (ktiles > 1) __builtin_amdgcn_s_waitcnt(0x0F70 | 6);
    else __builtin_amdgcn_s_waitcnt(0x0F70);
    __builtin_amdgcn_s_barrier();
    if (ktiles > 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ah[0][i] = frag_a(smem, i, 0);
            bl[i] = frag_b(smem, i, 1);
            al[i] = frag_a(smem, i, 1);
            bh[0][i] = frag_b(smem, i, 0);
        }
    }
    HP_STAMP(1);

    // One K-tile.  On entry ALL fragments of tile t sit in registers (hi sets PAR), so stage ST is dead as soon as every wave
    // has passed the barrier at the top: the transfers of tile t+3 into it are spread over the three MFMA blocks (a burst
    // of 48 one-KB transfers right behind a barrier queues up in the CU's address path for ~1000 cycles; two per block do
    // not), and the fragments of tile t+1 -- visible since the same barrier -- are read under Y and Z.
    constexpr int NRD = KC ? 8 : 16;   // LDS read instructions of four A + four B fragments
    auto body = [&](auto par_c, auto st_c, int t) {
        constexpr int PAR = decltype(par_c)::value, ST = decltype(st_c)::value;
        const char* S1 = smem + ((ST + 1) % 3) * HP_STAGE;
        const bool more3 = t + 3 < ktiles;
        if (t == 7) HP_STAMP(5);
        // this wave's transfers of tile t+1 have landed (tile t+2 stays in flight), its own fragment reads have returned
        if (t + 2 < ktiles) __builtin_amdgcn_s_waitcnt(0x0070 | 6);
        else __builtin_amdgcn_s_waitcnt(0x0070);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (t == 7) HP_STAMP(6);
        // X
        if (more3) dma_part(ST, 0);
        h3_mfma16(acc, ah[PAR], bl);
        __builtin_amdgcn_sched_barrier(0);
        if (t == 7) HP_STAMP(7);
        // Y
        if (more3) dma_part(ST, 1);
        if (KC) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bl[i] = frag_b(S1, i, 1);
                ah[PAR ^ 1][i] = frag_a(S1, i, 0);
            }
            h3_mfma16(acc, al, bh[PAR]);
            h3_sched<16, 0, 0, NRD, 0, 0>();
        } else {   // (asm reads are invisible to sched_group_barrier: interleave by hand, one fragment per two MFMAs)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh[PAR][j], acc[i][j], 0, 0, 0);
                    if (j == 1) bl[i] = frag_b(S1, i, 1);
                    if (j == 3) ah[PAR ^ 1][i] = frag_a(S1, i, 0);
                }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (t == 7) HP_STAMP(8);
        // Z
        if (more3) dma_part(ST, 2);
        if (KC) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                al[i] = frag_a(S1, i, 1);
                bh[PAR ^ 1][i] = frag_b(S1, i, 0);
            }
            h3_mfma16(acc, ah[PAR], bh[PAR]);
            h3_sched<16, 0, 0, NRD, 0, 0>();
        } else {   // al[i] was last used in Y: free.  bh[PAR ^ 1] is the other register set.
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[PAR][i], bh[PAR][j], acc[i][j], 0, 0, 0);
                    if (j == 1) al[i] = frag_a(S1, i, 1);
                    if (j == 3) bh[PAR ^ 1][i] = frag_b(S1, i, 0);
                }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (t == 7) HP_STAMP(9);
    };
    {
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        using I2 = std::integral_constant<int, 2>;
        int t = 0;
        for (; t + 6 <= ktiles; t += 6) {
            body(I0{}, I0{}, t);
            body(I1{}, I1{}, t + 1);
            body(I0{}, I2{}, t + 2);
            body(I1{}, I0{}, t + 3);
            body(I0{}, I1{}, t + 4);
            body(I1{}, I2{}, t + 5);
        }
        if (t < ktiles) {
            body(I0{}, I0{}, t);
            if (t + 1 < ktiles) {
                body(I1{}, I1{}, t + 1);
                if (t + 2 < ktiles) {
                    body(I0{}, I2{}, t + 2);
                    if (t + 3 < ktiles) {
                        body(I1{}, I0{}, t + 3);
                        if (t + 4 < ktiles) body(I0{}, I1{}, t + 4);
                    }
                }
            }
        }
    }

    // ---- epilogue ---------------------------------------------------------------------------------------------------------
    HP_STAMP(2);
    const int ka = hp_scale_exp(p.sa), kb = hp_scale_exp(p.sb);
    const float inv_a = h3_pow2(-ka), inv_b = h3_pow2(-kb);
    // lane's pass q: row 8q + lane/8, columns 8*(lane%8) .. +7 of the wave's 64 x 64 sub-tile
    const int er = lane >> 3, ec = (lane & 7) * 8;
    const int col_g = n0 + 64 * wn + ec;
    const bool col_ok = col_g < p.N;
    f32x4 mulreg[16];
    __amdgpu_buffer_rsrc_t srdMul, srdHL, srdC2;
    int voff32 = 0, voffhl = 0;
    if (EPI != HPE_SLAB) {
        const long long rows_left = p.M - m0;
        const long long win = (rows_left < HP_BM ? rows_left : HP_BM) * (long long)p.N * 4;
        const long long first = (long long)m0 * p.N * 4;
        srdHL = hp_srd(p.C_hl + first, win);
        srdC2 = hp_srd(EPI == HPE_SINE_STASH ? (const char*)p.C2 + first : p.C_hl, EPI == HPE_SINE_STASH ? win : 0);
        srdMul = hp_srd(EPI == HPE_MUL ? (const char*)p.mul + first : p.C_hl, EPI == HPE_MUL ? win : 0);
        const int row = 64 * wm + er;
        voff32 = col_ok ? (row * p.N + col_g) * 4 : 0x7FFFFF00;
        voffhl = col_ok ? row * p.N * 4 + (col_g >> 5) * 128 + (col_g & 31) * 2 : 0x7FFFFF00;
        if (EPI == HPE_MUL) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                mulreg[2 * q] = buf_load4(srdMul, voff32 + q * 8 * p.N * 4, 0);
                mulreg[2 * q + 1] = buf_load4(srdMul, voff32 + q * 8 * p.N * 4 + 16, 0);
            }
        }
    }
    __syncthreads();   // operand stages are dead: LDS becomes the epilogue staging area
    float* sub = reinterpret_cast<float*>(smem) + wave * (64 * SUB16);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) sub[(i * 16 + 4 * g + r) * SUB16 + j * 16 + l16] = acc[i][j][r] * inv_a * inv_b;
    const float* rd = sub + er * SUB16 + ec;
    HP_STAMP(3);

    if (EPI == HPE_SLAB) {
        float* C = p.C2 + (long long)split * p.slab_stride;
        const int row0 = m0 + 64 * wm + er;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int row = row0 + 8 * q;
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(rd + q * 8 * SUB16);
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(rd + q * 8 * SUB16 + 4);
            if (row < p.M && col_ok) {
                float* dst = C + (long long)row * p.N + col_g;
                *reinterpret_cast<f32x4*>(dst) = v0;
                *reinterpret_cast<f32x4*>(dst + 4) = v1;
            }
        }
        HP_STAMP(4);
        return;
    }

    if (EPI == HPE_SINE || EPI == HPE_SINE_STASH) {
        const float so_act = h3_pow2(hp_scale_exp(p.so));   // scale of the sine outputs' HL32 image (from the layer's a-priori bound)
        f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
        if (p.bias && col_ok) {
            b0 = *reinterpret_cast<const f32x4*>(p.bias + col_g);
            b1 = *reinterpret_cast<const f32x4*>(p.bias + col_g + 4);
        }
        float zmax = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const f32x4 z0 = p.omega * (*reinterpret_cast<const f32x4*>(rd + q * 8 * SUB16) + b0);
            const f32x4 z1 = p.omega * (*reinterpret_cast<const f32x4*>(rd + q * 8 * SUB16 + 4) + b1);
            zmax = fmaxf(zmax, fmaxf(fmaxf(fmaxf(fabsf(z0[0]), fabsf(z0[1])), fmaxf(fabsf(z0[2]), fabsf(z0[3]))),
                                     fmaxf(fmaxf(fabsf(z1[0]), fabsf(z1[1])), fmaxf(fabsf(z1[2]), fabsf(z1[3])))));
            f32x2_t s[4], c[4];
            sincos_f32x2_fast(f32x2_t{z0[0], z0[1]}, s[0], c[0]);
            sincos_f32x2_fast(f32x2_t{z0[2], z0[3]}, s[1], c[1]);
            sincos_f32x2_fast(f32x2_t{z1[0], z1[1]}, s[2], c[2]);
            sincos_f32x2_fast(f32x2_t{z1[2], z1[3]}, s[3], c[3]);
            const float sv[8] = {s[0][0], s[0][1], s[1][0], s[1][1], s[2][0], s[2][1], s[3][0], s[3][1]};
            u32x4 hi, lo;
            hp_split8(sv, so_act, hi, lo);
            const int ro = q * 8 * p.N * 4;
            __builtin_amdgcn_raw_buffer_store_b128(hi, srdHL, voffhl + ro, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(lo, srdHL, voffhl + ro + 64, 0, 0);
            if (EPI == HPE_SINE_STASH) {
                buf_store4(p.omega * f32x4{c[0][0], c[0][1], c[1][0], c[1][1]}, srdC2, voff32, ro);
                buf_store4(p.omega * f32x4{c[2][0], c[2][1], c[3][0], c[3][1]}, srdC2, voff32 + 16, ro);
            }
        }
        HP_STAMP(4);
        if (__builtin_expect(__any(!(zmax < INR_SINCOS_FAST_LIMIT)), 0)) {   // rare: redo the wave's tile through libm
#pragma unroll 1
            for (int q = 0; q < 8; ++q) {
                float sv[8], cv[8];
#pragma unroll 1
                for (int e = 0; e < 8; ++e) {
                    const float bia = (p.bias && col_ok) ? p.bias[col_g + e] : 0.f;
                    sincos_f32(p.omega * (rd[q * 8 * SUB16 + e] + bia), sv[e], cv[e]);
                }
                u32x4 hi, lo;
                hp_split8(sv, so_act, hi, lo);
                const int ro = q * 8 * p.N * 4;
                __builtin_amdgcn_raw_buffer_store_b128(hi, srdHL, voffhl + ro, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(lo, srdHL, voffhl + ro + 64, 0, 0);
                if (EPI == HPE_SINE_STASH) {
                    buf_store4(p.omega * f32x4{cv[0], cv[1], cv[2], cv[3]}, srdC2, voff32, ro);
                    buf_store4(p.omega * f32x4{cv[4], cv[5], cv[6], cv[7]}, srdC2, voff32 + 16, ro);
                }
            }
        }
        return;
    }

    // HPE_MUL: dz_prev = (dz W) * dact_prev, column sums (bias gradient of the layer below), max |dz_prev|, then the HL32
    // image of dz_prev * 2^ko over the very bytes `mul` came from (this wave has read all of its 64 x 256 bytes above)
    const int ko = hp_scale_exp(p.so);
    const float so = h3_pow2(ko);
    f32x4 cs0 = {0.f, 0.f, 0.f, 0.f}, cs1 = cs0;
    float omax = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const f32x4 o0 = hp_mul_sum(*reinterpret_cast<const f32x4*>(rd + q * 8 * SUB16), mulreg[2 * q], cs0);
        const f32x4 o1 = hp_mul_sum(*reinterpret_cast<const f32x4*>(rd + q * 8 * SUB16 + 4), mulreg[2 * q + 1], cs1);
        omax = fmaxf(omax, fmaxf(fmaxf(fmaxf(fabsf(o0[0]), fabsf(o0[1])), fmaxf(fabsf(o0[2]), fabsf(o0[3]))),
                                 fmaxf(fmaxf(fabsf(o1[0]), fabsf(o1[1])), fmaxf(fabsf(o1[2]), fabsf(o1[3])))));
        const float ov[8] = {o0[0], o0[1], o0[2], o0[3], o1[0], o1[1], o1[2], o1[3]};
        u32x4 hi, lo;
        hp_split8(ov, so, hi, lo);
        const int ro = q * 8 * p.N * 4;
        __builtin_amdgcn_raw_buffer_store_b128(hi, srdHL, voffhl + ro, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(lo, srdHL, voffhl + ro + 64, 0, 0);
    }
    HP_STAMP(4);
    if (p.amax_out) {
        omax = wave_max(omax);
        if (lane == 0) hp_atomic_max_bits(p.amax_out, omax);
    }
    if (p.colsum) {   // 8 rows per lane so far; the 8 lanes sharing a column group are lane ^ 8, ^ 16, ^ 32 (fixed order)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            cs0[e] += __shfl_xor(cs0[e], 8, 64);
            cs1[e] += __shfl_xor(cs1[e], 8, 64);
            cs0[e] += __shfl_xor(cs0[e], 16, 64);
            cs1[e] += __shfl_xor(cs1[e], 16, 64);
            cs0[e] += __shfl_xor(cs0[e], 32, 64);
            cs1[e] += __shfl_xor(cs1[e], 32, 64);
        }
        if (lane < 8 && col_ok) {
            float* dst = p.colsum + (long long)(tile_m * 2 + wm) * p.N + col_g;
            *reinterpret_cast<f32x4*>(dst) = cs0;
            *reinterpret_cast<f32x4*>(dst + 4) = cs1;
        }
    }
}

template <int MODE, int EPI>
__global__ void __launch_bounds__(HP_NTH, 2) gemm_hp_kernel(const HpParams p) {
    gemm_hp_body<MODE, EPI>(p, (int)blockIdx.x);
}

// Several row-contraction GEMMs (the parameter gradients of all layers of a step) in ONE launch: block b belongs to job j with
// first[j] <= b < first[j + 1] and does there exactly what block b - first[j] of a launch of its own would do (same tiles, same
// order: the slabs are bit-identical).  At a few thousand rows a parameter-gradient GEMM fills half the chip for 13 us and a
// launch boundary costs nearly as much: four of them behind the input-gradient chain -- or beside it on a second stream, whose
// event hand-shakes cost 7-13 us each -- were a quarter of the step.
constexpr int HP_MULTI_MAX = 8;
struct HpMultiParams {
    HpParams p[HP_MULTI_MAX];
    int first[HP_MULTI_MAX + 1];
    int jobs;
};
__global__ void __launch_bounds__(HP_NTH, 2) gemm_hp_rc_multi_kernel(const HpMultiParams m) {
    int j = 0;
    while (j + 1 < m.jobs && (int)blockIdx.x >= m.first[j + 1]) ++j;
    gemm_hp_body<HP_RC, HPE_SLAB>(m.p[j], (int)blockIdx.x - m.first[j]);
}

// =======================================================================================================================
// HL32 producers outside the GEMM epilogues
// =======================================================================================================================
__device__ __forceinline__ long long hp_off(long long row, int col, int cols) {   // byte offset of hi(X[row][col])
    return (row * (cols >> 5) + (col >> 5)) * 128 + (col & 31) * 2;
}

// fp32 [rows][cols] -> HL32, scaled by the power of two of `sc` (cols % 32 == 0; one thread per 8 elements)
__global__ void __launch_bounds__(256) INR_PACKED_F32 hp_convert_kernel(char* __restrict__ out, const float* __restrict__ x, long long rows, int cols,
                                                         const HpScale sc) {
    const float s = h3_pow2(hp_scale_exp(sc));
    const long long n8 = rows * (cols >> 3);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        const long long row = i / (cols >> 3);
        const int col = (int)(i % (cols >> 3)) * 8;
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + row * cols + col);
        const f32x4 b = *reinterpret_cast<const f32x4*>(x + row * cols + col + 4);
        const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        u32x4 hi, lo;
        hp_split8(v, s, hi, lo);
        char* dst = out + hp_off(row, col, cols);
        *reinterpret_cast<u32x4*>(dst) = hi;
        *reinterpret_cast<u32x4*>(dst + 64) = lo;
    }
}

// HL32 -> fp32 (diagnostics / tests): x = (hi + lo) * 2^-k
__global__ void __launch_bounds__(256) INR_PACKED_F32 hp_unconvert_kernel(float* __restrict__ out, const char* __restrict__ x, long long rows, int cols,
                                                           const HpScale sc) {
    const float inv = h3_pow2(-hp_scale_exp(sc));
    const long long n = rows * cols;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long row = i / cols;
        const int col = (int)(i % cols);
        const char* src = x + hp_off(row, col, cols);
        out[i] = ((float)*reinterpret_cast<const _Float16*>(src) + (float)*reinterpret_cast<const _Float16*>(src + 64)) * inv;
    }
}

// ---- per-step weight preparation: two launches ------------------------------------------------------------------------------
// (round 2 took five: memset of the scale slots, weight_amax, hp_wnorm -- 32 us on its own: 32 blocks walking 128 rows each --,
// hp_weight_split and hp_head_bound; at a few thousand rows per fit those 60 us were a sixth of the step)
//   A  hp_weight_stats_kernel: block (bx, l) owns the 16-column groups bx, bx + gridDim.x, ... of W_l: max|W| over its elements
//      and the largest column sum of |W| (wnorm_l = max_j sum_k |W_l[k][j]| bounds |dz W| by max|dz| * wnorm) -> one pair of
//      words per block.  No atomics, no zeroed slots.
//   B  hp_weight_split_kernel: every block folds its layer's <= 64 pairs (the scale of the split), block 0 of a layer also
//      publishes them in the scale slots the GEMMs read; one extra block row zeroes the dz maxima of the step and evaluates the
//      a-priori bound of the head's dz.
// W [out][in] fp32 -> HL32 [out][in] and HL32 [in][out] (the k-contiguous B operands of forward / input-grad).  One block per
// 64 x 64 tile; the transposed image goes through LDS.
constexpr int HP_PREP_MAXB = 64;   // stats blocks per layer
struct HpWeightJob {
    const float* W;
    char *hl, *hlT;
    unsigned* amax;    // slot: float bits of max|W|
    unsigned* wnorm;   // slot: float bits of max_j sum_k |W[k][j]|
    int out_f, in_f;
    const float* bias; // [out_f], nullable (the a-priori bound of the layer's output)
    float omega;
};
struct HpWeightJobs {
    HpWeightJob job[8];
    int layers;
    unsigned* part;            // [8][HP_PREP_MAXB][2] per-block (amax bits, wnorm bits)
    unsigned* dz_slots;        // 8 words zeroed every step (atomic-max targets of the backward kernels)
    // a-priori bound of every sine layer's output (the scale of its HL32 image; round 4 -- rounds 2-3 stored sine outputs
    // unscaled, which kept 22 bits only for elements >= 2^-3: a layer whose whole output is tiny was seen with a few bits):
    //   |sin(omega (a W^T + b))| <= min(1, |omega| (in_f max|W| max|a| + max|b|)),  max|a| = the previous layer's bound
    //   (layer 0: the measured max|x|, or 1 when `x_amax` is null: grids and Fourier features)
    float* act_bound;          // [layers] (nullable)
    const unsigned* x_amax;
    // a-priori bound of the head's dz (nullable: forward-only callers):
    //   |dz_L| = |g| |w_j| |omega cos| <= 2 wtmax (sum|w| + |b| + tmax) / count * max|w| * omega
    float* head_bound;
    const float* head_W;
    const float* head_b;
    const unsigned* tmax;
    const unsigned* wtmax;
    int hidden;
    float inv_count, omega;
};

__device__ __forceinline__ int hp_stats_blocks(int in_f) { return min(HP_PREP_MAXB, in_f >> 4); }

__global__ void __launch_bounds__(256) INR_PACKED_F32 hp_weight_stats_kernel(const HpWeightJobs jobs) {
    __shared__ float part[16][16];
    __shared__ unsigned red_a[4];
    __shared__ float red_c;
    const HpWeightJob j = jobs.job[blockIdx.y];
    const int nb = hp_stats_blocks(j.in_f);
    if ((int)blockIdx.x >= nb) return;
    const int cl = threadIdx.x & 15, ph = threadIdx.x >> 4;
    unsigned amax = 0;
    float cmax = 0.f;
    for (int cg = blockIdx.x; cg * 16 < j.in_f; cg += nb) {
        const int c = cg * 16 + cl;
        float acc = 0.f;
#pragma unroll 8
        for (int k = ph; k < j.out_f; k += 16) {
            const float w = fabsf(j.W[(long long)k * j.in_f + c]);
            acc += w;
            amax = max(amax, __float_as_uint(w));
        }
        part[ph][cl] = acc;
        __syncthreads();
        if (threadIdx.x < 16) {
            float sum = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) sum += part[q][threadIdx.x];
            cmax = fmaxf(cmax, sum);
        }
        __syncthreads();
    }
    amax = wave_max(amax);
    if ((threadIdx.x & 63) == 0) red_a[threadIdx.x >> 6] = amax;
    if (threadIdx.x < 64) {   // (lanes 16 .. 63 hold 0)
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) cmax = fmaxf(cmax, __shfl_xor(cmax, off, 64));
        if (threadIdx.x == 0) red_c = cmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned* out = jobs.part + ((long long)blockIdx.y * HP_PREP_MAXB + blockIdx.x) * 2;
        out[0] = max(max(red_a[0], red_a[1]), max(red_a[2], red_a[3]));
        out[1] = __float_as_uint(red_c);
    }
}

__global__ void __launch_bounds__(256) INR_PACKED_F32 hp_weight_split_kernel(const HpWeightJobs jobs) {
    __shared__ _Float16 th[64][66], tl[64][66];
    __shared__ unsigned s_amax;
    if ((int)blockIdx.y == jobs.layers) {   // the extra block row: step-wide scalars
        if (blockIdx.x != 0) return;
        if (threadIdx.x < 8) jobs.dz_slots[threadIdx.x] = 0u;
        __shared__ float s1[4], s2[4];
        if (jobs.act_bound) {   // wave w reduces layers w, w + 4 (max|b|, max|W| from the stats pairs); thread 0 then walks the chain
            __shared__ float s_b[8], s_w[8];
            const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
            for (int l = wv; l < jobs.layers; l += 4) {
                const HpWeightJob jl = jobs.job[l];
                float bm = 0.f;
                if (jl.bias)
                    for (int i = lane; i < jl.out_f; i += 64) bm = fmaxf(bm, fabsf(jl.bias[i]));
                unsigned am = 0u;      // (non-negative floats order like their bits)
                if (lane < hp_stats_blocks(jl.in_f)) am = jobs.part[((long long)l * HP_PREP_MAXB + lane) * 2];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    bm = fmaxf(bm, __shfl_xor(bm, off, 64));
                    am = max(am, (unsigned)__shfl_xor((int)am, off, 64));
                }
                if (lane == 0) {
                    s_b[l] = bm;
                    s_w[l] = __uint_as_float(am);
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                float prev = jobs.x_amax ? __uint_as_float(*jobs.x_amax) : 1.0f;
                for (int l = 0; l < jobs.layers; ++l) {
                    float bound = fabsf(jobs.job[l].omega) * ((float)jobs.job[l].in_f * s_w[l] * prev * 1.0001f + s_b[l]) * 1.001f;
                    bound = bound < 1.0f ? bound : 1.0f;     // (NaN -> 1: the comparison is false)
                    jobs.act_bound[l] = bound;
                    prev = bound;
                }
            }
            __syncthreads();
        }
        if (!jobs.head_bound) return;
        float a = 0.f, m = 0.f;
        for (int i = threadIdx.x; i < jobs.hidden; i += 256) {
            const float w = fabsf(jobs.head_W[i]);
            a += w;
            m = fmaxf(m, w);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_xor(a, off, 64);
            m = fmaxf(m, __shfl_xor(m, off, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            s1[threadIdx.x >> 6] = a;
            s2[threadIdx.x >> 6] = m;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const float sum = (s1[0] + s1[1]) + (s1[2] + s1[3]) + (jobs.head_b ? fabsf(jobs.head_b[0]) : 0.f);
            const float mx = fmaxf(fmaxf(s2[0], s2[1]), fmaxf(s2[2], s2[3]));
            const float wt = jobs.wtmax ? __uint_as_float(*jobs.wtmax) : 1.0f;
            jobs.head_bound[0] = 2.0f * wt * (sum * 1.0001f + __uint_as_float(*jobs.tmax)) * jobs.inv_count * mx * fabsf(jobs.omega) * 1.001f;
        }
        return;
    }
    const HpWeightJob j = jobs.job[blockIdx.y];
    const int ti = (j.in_f + 63) / 64, to = (j.out_f + 63) / 64;
    if ((int)blockIdx.x >= ti * to) return;
    if (threadIdx.x < 64) {   // fold the layer's stats pairs (every block needs the scale; block 0 publishes both)
        const int nb = hp_stats_blocks(j.in_f);
        const unsigned* pp = jobs.part + (long long)blockIdx.y * HP_PREP_MAXB * 2;
        unsigned am = (int)threadIdx.x < nb ? pp[2 * threadIdx.x] : 0u;
        unsigned wn = (int)threadIdx.x < nb ? pp[2 * threadIdx.x + 1] : 0u;   // (non-negative floats order like their bits)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            am = max(am, (unsigned)__shfl_xor((int)am, off, 64));
            wn = max(wn, (unsigned)__shfl_xor((int)wn, off, 64));
        }
        if (threadIdx.x == 0) {
            s_amax = am;
            if (blockIdx.x == 0) {
                *j.amax = am;
                *j.wnorm = wn;
            }
        }
    }
    __syncthreads();
    const int o0 = (blockIdx.x / ti) * 64, i0 = (blockIdx.x % ti) * 64;
    const float s = h3_pow2(h3_scale_exp(s_amax));
    const int c2 = (threadIdx.x & 31) * 2, r8 = threadIdx.x >> 5;
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
        const int o = o0 + r8 + 8 * rr, c = i0 + c2;
        half2v h = {(_Float16)0.f, (_Float16)0.f}, l = h;
        if (o < j.out_f && c + 1 < j.in_f) {
            const long long at = (long long)o * j.in_f + c;
            h3_split2<true>(j.W[at], j.W[at + 1], s, h, l);
            char* dst = j.hl + hp_off(o, c, j.in_f);
            *reinterpret_cast<half2v*>(dst) = h;
            *reinterpret_cast<half2v*>(dst + 64) = l;
        }
        th[c2][r8 + 8 * rr] = h[0];
        th[c2 + 1][r8 + 8 * rr] = h[1];
        tl[c2][r8 + 8 * rr] = l[0];
        tl[c2 + 1][r8 + 8 * rr] = l[1];
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
        const int c = i0 + r8 + 8 * rr, o = o0 + c2;
        if (c < j.in_f && o + 1 < j.out_f) {
            char* dst = j.hlT + hp_off(c, o, j.out_f);
            *reinterpret_cast<half2v*>(dst) = half2v{th[r8 + 8 * rr][c2], th[r8 + 8 * rr][c2 + 1]};
            *reinterpret_cast<half2v*>(dst + 64) = half2v{tl[r8 + 8 * rr][c2], tl[r8 + 8 * rr][c2 + 1]};
        }
    }
}

// a-priori bound of the head's dz when dL/dy comes from outside: |dz_L| = |g| |w_j| |omega cos| <= max|g| max|w| |omega|
__global__ void __launch_bounds__(256) INR_PACKED_F32 hp_head_bound_ext_kernel(float* __restrict__ head_bound, const unsigned* __restrict__ gmax,
                                                                const float* __restrict__ head_W, int hidden, float omega) {
    __shared__ float s2[4];
    float m = 0.f;
    for (int i = threadIdx.x; i < hidden; i += 256) m = fmaxf(m, fabsf(head_W[i]));
#pragma unroll   // wave_max(), open-coded: through the helper this translation unit's instruction schedule changes
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) s2[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        head_bound[0] = __uint_as_float(*gmax) * fmaxf(fmaxf(s2[0], s2[1]), fmaxf(s2[2], s2[3])) * fabsf(omega) * 1.001f;
}

// ---- head on HL32 activations -------------------------------------------------------------------------------------------
template <int CPL>
struct HpVec {
    typedef _Float16 H __attribute__((ext_vector_type(CPL)));
    typedef float F __attribute__((ext_vector_type(CPL)));
};

template <int CPL>
__device__ __forceinline__ void hp_load_row(const char* __restrict__ a, long long row, int hidden, int c0, float (&v)[CPL], float inv) {
    const char* src = a + hp_off(row, c0, hidden);
    const typename HpVec<CPL>::H hi = *reinterpret_cast<const typename HpVec<CPL>::H*>(src);
    const typename HpVec<CPL>::H lo = *reinterpret_cast<const typename HpVec<CPL>::H*>(src + 64);
#pragma unroll
    for (int e = 0; e < CPL; ++e) v[e] = ((float)hi[e] + (float)lo[e]) * inv;      // inv = 2^-k of the image's scale
}

// y = a W^T + b (out_features == 1), optional clamp; one wave per row, lane owns CPL = hidden / 64 consecutive columns
// FROMZ: `a` holds the fp32 pre-activations z + b of the last sine layer (HPE_Z): a = sin(omega z) formed here, exactly as
// hp_head_step_kernel<CPL, true> forms it (the two see the same activations)
template <int CPL, bool FROMZ = false>
__global__ void __launch_bounds__(256) INR_PACKED_F32 hp_head_forward_kernel(float* __restrict__ y, const char* __restrict__ a,
                                                              const float* __restrict__ W, const float* __restrict__ bias,
                                                              int64_t n, int use_clamp, float clamp_min, float omega = 0.f,
                                                              const HpScale sa = HpScale{}) {
    constexpr int H = 64 * CPL;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c0 = lane * CPL;
    const float inv_sa = h3_pow2(-hp_scale_exp(sa));
    float w[CPL];
#pragma unroll
    for (int e = 0; e < CPL; ++e) w[e] = W[c0 + e];
    const float b0 = bias ? bias[0] : 0.f;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n; r += (int64_t)gridDim.x * 4) {
        float v[CPL], acc = 0.f;
        if (FROMZ) {
            const typename HpVec<CPL>::F z = *reinterpret_cast<const typename HpVec<CPL>::F*>(reinterpret_cast<const float*>(a) + r * H + c0);
#pragma unroll
            for (int e = 0; e < CPL; e += 2) {
                f32x2_t s2, c2;
                sincos_f32x2_fast(f32x2_t{omega * z[e], omega * z[e + 1]}, s2, c2);
                v[e] = s2[0];
                v[e + 1] = s2[1];
            }
        } else
        hp_load_row<CPL>(a, r, H, c0, v, inv_sa);
#pragma unroll
        for (int e = 0; e < CPL; ++e) acc = fmaf(v[e], w[e], acc);
        float s = wave_sum(acc) + b0;
        if (use_clamp) s = fmaxf(s, clamp_min);
        if (lane == 0) y[r] = s;
    }
}

// the one-pass head step of the fused fit on HL32 operands (kernels.hip: head_step_fused_kernel is the fp32 original):
// y, residual, g = dL/dy, dz_L = g w omega cos (written as HL32 * 2^k over the dact bytes), gb_L / gW_head slabs, loss / sum-g
// FROMZ: `dact` holds z + b of the last sine layer (HPE_Z) and `a` is not read: a = sin(omega z), d = omega cos(omega z) here
template <int CPL, bool FROMZ = false, bool GEXT = false>
__global__ void __launch_bounds__(256) INR_PACKED_F32 hp_head_step_kernel(char* dz, float* __restrict__ slab_b, float* __restrict__ slab_w,
                                                           float* __restrict__ part_loss, float* __restrict__ part_g,
                                                           const char* __restrict__ a, const float* dact,
                                                           const float* __restrict__ W, const float* __restrict__ bias,
                                                           const float* __restrict__ t, const float* __restrict__ wgt, int64_t n,
                                                           float inv_count, unsigned* __restrict__ amax_out, const HpScale so,
                                                           int rows_per_block, float omega = 0.f,
                                                           const float* __restrict__ g_ext = nullptr, const HpScale sa = HpScale{}) {
    constexpr int H = 64 * CPL;
    __shared__ float red[2][4][H];
    __shared__ float red_s[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c0 = lane * CPL;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(n, r0 + rows_per_block);
    const float sc = h3_pow2(hp_scale_exp(so));
    const float inv_sa = h3_pow2(-hp_scale_exp(sa));     // scale of the activations' image (FROMZ: unused)
    float w[CPL], sb[CPL], sw[CPL];
#pragma unroll
    for (int e = 0; e < CPL; ++e) {
        w[e] = W[c0 + e];
        sb[e] = 0.f;
        sw[e] = 0.f;
    }
    const float b0 = bias ? bias[0] : 0.f;
    float loss_acc = 0.f, g_acc = 0.f, omax = 0.f;
    // A wave's rows are one dependent chain each (load -> sin / cos -> wave sum -> g -> store): the NEXT row's operands are
    // requested before this row's arithmetic, which doubles the bytes a wave keeps in flight (HP_HEAD_PREFETCH = 0: the A/B partner)
    auto load_d = [&](int64_t r) {
        if (HP_HEAD_NT && FROMZ) return __builtin_nontemporal_load(reinterpret_cast<const typename HpVec<CPL>::F*>(dact + r * H + c0));
        return *reinterpret_cast<const typename HpVec<CPL>::F*>(dact + r * H + c0);
    };
    typename HpVec<CPL>::F d_next = {};
    typename HpVec<CPL>::H ahi_next = {}, alo_next = {};
    auto prefetch = [&](int64_t r) {
        d_next = load_d(r);
        if (!FROMZ) {
            const char* src = a + hp_off(r, c0, H);
            ahi_next = *reinterpret_cast<const typename HpVec<CPL>::H*>(src);
            alo_next = *reinterpret_cast<const typename HpVec<CPL>::H*>(src + 64);
        }
    };
    if (HP_HEAD_PREFETCH && r0 + wave < r1) prefetch(r0 + wave);
    for (int64_t r = r0 + wave; r < r1; r += 4) {
        float v[CPL], acc = 0.f;
        typename HpVec<CPL>::F d;
        typename HpVec<CPL>::H ahi, alo;
        if (HP_HEAD_PREFETCH) {
            d = d_next;
            ahi = ahi_next;
            alo = alo_next;
            if (r + 4 < r1) prefetch(r + 4);
        } else {
            d = load_d(r);
        }
        if (FROMZ) {
#pragma unroll
            for (int e = 0; e < CPL; e += 2) {
                f32x2_t s2, c2;
                sincos_f32x2_fast(f32x2_t{omega * d[e], omega * d[e + 1]}, s2, c2);
                v[e] = s2[0];
                v[e + 1] = s2[1];
                d[e] = omega * c2[0];
                d[e + 1] = omega * c2[1];
            }
        } else if (HP_HEAD_PREFETCH) {
#pragma unroll
            for (int e = 0; e < CPL; ++e) v[e] = ((float)ahi[e] + (float)alo[e]) * inv_sa;      // as hp_load_row forms them
        } else {
            hp_load_row<CPL>(a, r, H, c0, v, inv_sa);
        }
#pragma unroll
        for (int e = 0; e < CPL; ++e) acc = fmaf(v[e], w[e], acc);
        // GEXT: dL/dy comes from the caller (the autograd path: torch formed the loss); no residual, no loss terms.  (A template
        // parameter: as a run-time branch it cost the fused fit's head step 8 us of 17 at 4,096 rows.)
        float g;
        if (GEXT) {
            g = g_ext[r];
        } else {
            const float y = wave_sum(acc) + b0;
            const float res = y - t[r];
            const float wr = wgt ? wgt[r] * res : res;
            g = 2.0f * wr * inv_count;
            loss_acc = fmaf(wr, res, loss_acc);
        }
        g_acc += g;
        typename HpVec<CPL>::H hi, lo;
#pragma unroll
        for (int e = 0; e < CPL; e += 2) {
            const float o0 = (g * w[e]) * d[e], o1 = (g * w[e + 1]) * d[e + 1];
            omax = fmaxf(omax, fmaxf(fabsf(o0), fabsf(o1)));
            sb[e] += o0;
            sb[e + 1] += o1;
            sw[e] = fmaf(g, v[e], sw[e]);
            sw[e + 1] = fmaf(g, v[e + 1], sw[e + 1]);
            half2v h2, l2;
            h3_split2<true>(o0, o1, sc, h2, l2);
            hi[e] = h2[0];
            hi[e + 1] = h2[1];
            lo[e] = l2[0];
            lo[e + 1] = l2[1];
        }
        char* dst = dz + hp_off(r, c0, H);
        if (HP_HEAD_NT) {
            __builtin_nontemporal_store(hi, reinterpret_cast<typename HpVec<CPL>::H*>(dst));
            __builtin_nontemporal_store(lo, reinterpret_cast<typename HpVec<CPL>::H*>(dst + 64));
        } else {
            *reinterpret_cast<typename HpVec<CPL>::H*>(dst) = hi;
            *reinterpret_cast<typename HpVec<CPL>::H*>(dst + 64) = lo;
        }
    }
#pragma unroll
    for (int e = 0; e < CPL; ++e) {
        red[0][wave][c0 + e] = sb[e];
        red[1][wave][c0 + e] = sw[e];
    }
    if (lane == 0) {
        red_s[0][wave] = loss_acc;
        red_s[1][wave] = g_acc;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < H; q += 256) {
        slab_b[(int64_t)blockIdx.x * H + q] = (red[0][0][q] + red[0][1][q]) + (red[0][2][q] + red[0][3][q]);
        slab_w[(int64_t)blockIdx.x * H + q] = (red[1][0][q] + red[1][1][q]) + (red[1][2][q] + red[1][3][q]);
    }
    if (threadIdx.x == 0) {
        part_loss[blockIdx.x] = (red_s[0][0] + red_s[0][1]) + (red_s[0][2] + red_s[0][3]);
        part_g[blockIdx.x] = (red_s[1][0] + red_s[1][1]) + (red_s[1][2] + red_s[1][3]);
    }
    if (amax_out) {
        omax = wave_max(omax);
        if (lane == 0 && omax > 0.f) hp_atomic_max_bits(amax_out, omax);
    }
}

// Column sums of an epilogue chunk layout (row = lane / 4, eight columns from (lane & 3) * 8 in cs0, cs1): the xor 4, 8, 16, 32
// butterfly over the sixteen row lanes with the columns split between the partners at every stage -- a lane keeps half of its
// columns and receives the partner's sums for exactly those: 8 exchanges instead of 32.  Lane l ends with the total of column
// (l & 3) * 8 + hp_colsum_index(l); both halves of the wave hold it.  Every addition has the operands the all-reduce form gave it
// (own + partner's), so the same bits; the 96 LDS permutes it saves per tile were 2.7 % of the input-gradient launch.
__device__ __forceinline__ int hp_colsum_index(int lane) { return ((lane & 4) ? 4 : 0) + ((lane & 8) ? 2 : 0) + ((lane & 16) ? 1 : 0); }
__device__ __forceinline__ float hp_colsum_fold(const f32x4& cs0, const f32x4& cs1, int lane) {
    const bool b2 = lane & 4, b3 = lane & 8, b4 = lane & 16;
    float k4[4], k8[2];
#pragma unroll
    for (int e = 0; e < 4; ++e) k4[e] = (b2 ? cs1[e] : cs0[e]) + __shfl_xor(b2 ? cs0[e] : cs1[e], 4, 64);
#pragma unroll
    for (int e = 0; e < 2; ++e) k8[e] = (b3 ? k4[2 + e] : k4[e]) + __shfl_xor(b3 ? k4[e] : k4[2 + e], 8, 64);
    float k16 = (b4 ? k8[1] : k8[0]) + __shfl_xor(b4 ? k8[0] : k8[1], 16, 64);
    k16 += __shfl_xor(k16, 32, 64);
    return k16;
}

// =======================================================================================================================
// Persistent form of the KC kernel (forward, input-grad): one block per CU walks the tiles idx, idx + G, ...; the LDS ring
// runs THROUGH the tile boundaries (the last three K-iterations of a tile already fetch the first K-tiles of the next
// one), the epilogue stages through 2 KB per wave of its own (the ring stays live) and its stores drain under the next
// tile's K-loop.  No prologue latency and no block turnaround except for the first tile of a block.
// =======================================================================================================================
constexpr int HP_EPI_WAVE = 2048;   // 16 rows x 32 columns fp32 per wave
__device__ __forceinline__ constexpr int hp_vmcnt(int n) { return 0x0F70 | (n & 0xF) | ((n >> 4) << 14); }

template <int EPI>
__global__ void __launch_bounds__(HP_NTH, 2) gemm_hp_pkc_kernel(const HpParams p) {
    __shared__ __attribute__((aligned(1024))) char smem[HP_NSTAGE * HP_STAGE + 8 * HP_EPI_WAVE];
    constexpr int NST = EPI == HPE_SINE_STASH ? 32 : 16;   // stores every wave issues per tile epilogue (lower bound)

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int g = lane >> 4, l16 = lane & 15;
    const int total = p.tiles_m * p.tiles_n;
    const int G = gridDim.x;
    const int ktiles = p.K / HP_BK;   // >= 3 (host)

    struct Tile {
        int m0, n0;
        __amdgpu_buffer_rsrc_t srdA, srdB;
    };
    auto decode = [&](int vp) {
        int logical = xcd_remap(vp, total);
        Tile t;
        const int tn = logical % p.tiles_n, tm = logical / p.tiles_n;
        t.m0 = (p.reverse_m ? p.tiles_m - 1 - tm : tm) * HP_BM;
        t.n0 = tn * HP_BN;
        t.srdA = hp_srd(p.A + (long long)t.m0 * p.pitchA, (p.a_rows - t.m0) * p.pitchA);
        t.srdB = hp_srd(p.B + (long long)t.n0 * p.pitchB, (p.b_rows - t.n0) * p.pitchB);
        return t;
    };
    int vp = blockIdx.x;
    Tile cur = decode(vp), nxt = cur;
    bool has_next = vp + G < total;
    if (has_next) nxt = decode(vp + G);

    // this wave's six transfers per stage are rows 8 wave + 64 i (+ lane / 8) of the A image (i = 0, 1) and of the B image
    // (i = 0 .. 3); the slot permutation only looks at (row >> 1) & 7, which 64 i does not touch: ONE per-lane offset per
    // operand, the piece offset travels in the scalar offset
    const int drow = 8 * wave + (lane >> 3);
    const int dslot = ((lane & 7) ^ hp_f(drow)) * 16;
    const int vdmaA = drow * (int)p.pitchA + dslot, vdmaB = drow * (int)p.pitchB + dslot;
    const int pieceA = 64 * (int)p.pitchA, pieceB = 64 * (int)p.pitchB;
    // third `part` (0: the two A transfers, 1 / 2: two B transfers each) of K-tile j of the current tile (j >= ktiles: K-tile
    // j - ktiles of the next one) into ring stage `stage`
    auto dma_part = [&](int stage, int j, int part) {
        char* S = smem + stage * HP_STAGE;
        const bool from_next = j >= ktiles;
        const int soff = (from_next ? j - ktiles : j) * 128;
        const __amdgpu_buffer_rsrc_t sa = from_next ? nxt.srdA : cur.srdA, sb = from_next ? nxt.srdB : cur.srdB;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if ((i >> 1) != part) continue;
            const int q = wave + 8 * i;
            if (i < 2)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(sa, (__attribute__((address_space(3))) void*)(S + q * 1024), 16, vdmaA,
                                                         soff + i * pieceA, 0, 0);
            else
                __builtin_amdgcn_raw_ptr_buffer_load_lds(sb, (__attribute__((address_space(3))) void*)(S + q * 1024), 16, vdmaB,
                                                         soff + (i - 2) * pieceB, 0, 0);
        }
    };
    auto dma = [&](int stage, int j) {
        dma_part(stage, j, 0);
        dma_part(stage, j, 1);
        dma_part(stage, j, 2);
    };

    const int fx = (g ^ hp_f(l16)) << 4;
    const int fa_hi = (64 * wm + l16) * 128 + fx, fa_lo = fa_hi ^ 64;
    const int fb_hi = HP_A_IMG + (64 * wn + l16) * 128 + fx, fb_lo = fb_hi ^ 64;

    // The bias enters through the accumulators' initial value (bias * 2^(ka + kb): the epilogue multiplies by 2^-(ka + kb)),
    // so the epilogue issues no load at all -- a load there would make hipcc wait for every older vector-memory operation
    // (the ring's transfers, the previous chunk's stores) eight times per tile.  Lane holds columns 16 j + lane % 16.
    const int ka = hp_scale_exp(p.sa), kb = hp_scale_exp(p.sb);
    float bias_s[4] = {0.f, 0.f, 0.f, 0.f};
    auto load_bias = [&](int n0) {
        if (EPI == HPE_MUL || !p.bias) return;
        const float upa = h3_pow2(ka), upb = h3_pow2(kb);   // (two steps: 2^(ka + kb) alone may leave the fp32 range)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + 64 * wn + 16 * j + l16;
            const float b = p.bias[col < p.N ? col : p.N - 1];   // unconditional (clamped) load: four loads in flight together
            bias_s[j] = col < p.N ? (b * upa) * upb : 0.f;
        }
    };
    load_bias(cur.n0);
    f32x4v acc[4][4];
    half8 ah[2][4], bh[2][4], al[4], bl[4];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4v{bias_s[j], bias_s[j], bias_s[j], bias_s[j]};
    };
    zero_acc();

    // epilogue addressing of this lane inside a 16 x 32 chunk: row lane/4, columns 8 * (lane % 4) .. +7
    const int er = lane >> 2, ec = (lane & 3) * 8;
    float* const stg = reinterpret_cast<float*>(smem + HP_NSTAGE * HP_STAGE + wave * HP_EPI_WAVE);
    const float inv_a = h3_pow2(-ka), inv_b = h3_pow2(-kb);
    const float so = h3_pow2(hp_scale_exp(p.so));   // HPE_MUL: scale of dz_prev; sine epilogues: scale of the activations' image
    f32x4 mulreg[16];   // chunk c uses [2c], [2c+1]; loaded one chunk ahead, so only four of them are live at a time
    float omax_run = 0.f;
    auto load_mul = [&](int c) {
        const __amdgpu_buffer_rsrc_t srdMul =
            hp_srd((const char*)p.mul + (long long)cur.m0 * p.N * 4, (long long)min(p.M - cur.m0, HP_BM) * p.N * 4);
        const int row = 64 * wm + 16 * (c & 3) + er, cc = cur.n0 + 64 * wn + 32 * (c >> 2) + ec;
        const int vo = cc < p.N ? (row * p.N + cc) * 4 : 0x7FFFFF00;
        mulreg[2 * c] = buf_load4(srdMul, vo, 0);
        mulreg[2 * c + 1] = buf_load4(srdMul, vo + 16, 0);
    };

    // ---- prologue of the block's first tile ------------------------------------------------------------------------------
    if (p.stagger > 0) {
        for (int k = ((blockIdx.x >> 3) + blockIdx.x) & 7; k > 0; --k)
            for (int q = 0; q < p.stagger; q += 100) __builtin_amdgcn_s_sleep(100);
    }
    HP_STAMP(0);
    dma(0, 0);
    dma(1, 1);
    dma(2, 2);
    __builtin_amdgcn_s_waitcnt(hp_vmcnt(12));
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ah[0][i] = *reinterpret_cast<const half8*>(smem + fa_hi + i * 2048);
        bl[i] = *reinterpret_cast<const half8*>(smem + fb_lo + i * 2048);
        al[i] = *reinterpret_cast<const half8*>(smem + fa_lo + i * 2048);
        bh[0][i] = *reinterpret_cast<const half8*>(smem + fb_hi + i * 2048);
    }
    HP_STAMP(1);
    int stage = 0;       // ring stage of the K-tile being computed
    int pend = 0;        // 1 right after an epilogue: NST stores of it may still be in flight behind the ring's transfers

    // One K-tile (see gemm_hp_kernel): all fragments of tile t are in registers on entry; barrier; the transfers of K-tile t+3
    // (of this tile or the next) into the now dead stage spread over X / Y / Z, the fragments of K-tile t+1 read under Y / Z.
    auto body = [&](auto par_c, int t) {
        constexpr int PAR = decltype(par_c)::value;
        const int s1 = stage == 2 ? 0 : stage + 1;
        const char* S1 = smem + s1 * HP_STAGE;
        const bool more2 = t + 2 < ktiles || has_next, more3 = t + 3 < ktiles || has_next;
        if (t == 7) HP_STAMP(5);
        // tile t+1 (or the next tile's first) has landed; the transfers of t+2 -- and, in the first two iterations after an
        // epilogue, that epilogue's stores -- stay in flight.  lgkmcnt(0): this wave's fragment reads of stage `stage` are done.
        if (!more2) __builtin_amdgcn_s_waitcnt(hp_vmcnt(0) & 0xF0FF);
        else if (pend && t < 2) __builtin_amdgcn_s_waitcnt(hp_vmcnt(6 + NST) & 0xF0FF);
        else __builtin_amdgcn_s_waitcnt(hp_vmcnt(6) & 0xF0FF);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (t == 7) HP_STAMP(6);
        // X
        if (more3 && !(HP_ABLATE & 1)) dma_part(stage, t + 3, 0);
        if (!(HP_ABLATE & 2)) h3_mfma16(acc, ah[PAR], bl);
        __builtin_amdgcn_sched_barrier(0);
        if (t == 7) HP_STAMP(7);
        // Y
        if (more3 && !(HP_ABLATE & 1)) dma_part(stage, t + 3, 1);
        if (!(HP_ABLATE & 8)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bl[i] = *reinterpret_cast<const half8*>(S1 + fb_lo + i * 2048);
                ah[PAR ^ 1][i] = *reinterpret_cast<const half8*>(S1 + fa_hi + i * 2048);
            }
        }
        if (!(HP_ABLATE & 2)) h3_mfma16(acc, al, bh[PAR]);
        if (!(HP_ABLATE & 10)) h3_sched<16, 0, 0, 8, 0, 0>();
        __builtin_amdgcn_sched_barrier(0);
        if (t == 7) HP_STAMP(8);
        // Z
        if (more3 && !(HP_ABLATE & 1)) dma_part(stage, t + 3, 2);
        if (EPI == HPE_MUL && t == ktiles - 1) load_mul(0);   // first chunk's element-wise factor under the last MFMAs
        if (!(HP_ABLATE & 8)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                al[i] = *reinterpret_cast<const half8*>(S1 + fa_lo + i * 2048);
                bh[PAR ^ 1][i] = *reinterpret_cast<const half8*>(S1 + fb_hi + i * 2048);
            }
        }
        if (!(HP_ABLATE & 2)) h3_mfma16(acc, ah[PAR], bh[PAR]);
        if (!(HP_ABLATE & 10)) h3_sched<16, 0, 0, 8, 0, 0>();
        __builtin_amdgcn_sched_barrier(0);
        if (t == 7) HP_STAMP(9);
        stage = s1;
    };

    auto epilogue = [&]() {
        const long long first = (long long)cur.m0 * p.N * 4;
        const long long win = (long long)min(p.M - cur.m0, HP_BM) * p.N * 4;
        const __amdgpu_buffer_rsrc_t srdHL = hp_srd(p.C_hl + first, win);
        const __amdgpu_buffer_rsrc_t srdC2 = hp_srd(EPI == HPE_SINE_STASH ? (const char*)p.C2 + first : p.C_hl,
                                                    EPI == HPE_SINE_STASH ? win : 0);
        const int colw = cur.n0 + 64 * wn;   // first column of the wave's sub-tile
        f32x4 cs0 = {0.f, 0.f, 0.f, 0.f}, cs1 = cs0;   // column sums of the column block in progress
        float zmax = 0.f;
        // chunk c = 16 rows x 32 columns: column block jp = c / 4 (outer), row block i = c % 4 (inner) -- the bias-gradient
        // sums of one column block are finished and stored before the other one starts
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int i = c & 3, jp = c >> 2;
            if (EPI == HPE_MUL && c + 1 < 8) load_mul(c + 1);
            // park the chunk and read it back row-contiguous
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int r = 0; r < 4; ++r) stg[(4 * g + r) * 32 + jj * 16 + l16] = acc[i][2 * jp + jj][r] * inv_a * inv_b;
            __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the wave's own stores have reached the LDS
            __builtin_amdgcn_wave_barrier();
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(stg + er * 32 + ec);
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(stg + er * 32 + ec + 4);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
            const int row = 64 * wm + 16 * i + er, col = colw + 32 * jp + ec;
            const bool ok = col < p.N;
            const int vhl = ok ? row * p.N * 4 + (col >> 5) * 128 + (col & 31) * 2 : 0x7FFFFF00;
            const int v32 = ok ? (row * p.N + col) * 4 : 0x7FFFFF00;
            if (EPI == HPE_MUL) {
                const f32x4 o0 = hp_mul_sum(v0, mulreg[2 * c], cs0), o1 = hp_mul_sum(v1, mulreg[2 * c + 1], cs1);
                omax_run = fmaxf(omax_run, fmaxf(fmaxf(fmaxf(fabsf(o0[0]), fabsf(o0[1])), fmaxf(fabsf(o0[2]), fabsf(o0[3]))),
                                                 fmaxf(fmaxf(fabsf(o1[0]), fabsf(o1[1])), fmaxf(fabsf(o1[2]), fabsf(o1[3])))));
                const float ov[8] = {o0[0], o0[1], o0[2], o0[3], o1[0], o1[1], o1[2], o1[3]};
                u32x4 hi, lo;
                hp_split8(ov, so, hi, lo);
                __builtin_amdgcn_raw_buffer_store_b128(hi, srdHL, vhl, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(lo, srdHL, vhl + 64, 0, 0);
                if (i == 3 && p.colsum) {   // rows of a chunk sit on lane / 4: the 16 of them folded, 4 chunks done (hp_colsum_fold)
                    const float total = hp_colsum_fold(cs0, cs1, lane);
                    if (lane < 32 && ok) p.colsum[(long long)((cur.m0 / HP_BM) * 2 + wm) * p.N + col + hp_colsum_index(lane)] = total;
                    cs0 = f32x4{0.f, 0.f, 0.f, 0.f};
                    cs1 = cs0;
                }
            } else {
                const f32x4 z0 = p.omega * v0, z1 = p.omega * v1;
                zmax = fmaxf(zmax, fmaxf(fmaxf(fmaxf(fabsf(z0[0]), fabsf(z0[1])), fmaxf(fabsf(z0[2]), fabsf(z0[3]))),
                                         fmaxf(fmaxf(fabsf(z1[0]), fabsf(z1[1])), fmaxf(fabsf(z1[2]), fabsf(z1[3])))));
                float sv[8], cv[8];
                if (__builtin_expect(__any(!(zmax < INR_SINCOS_FAST_LIMIT)), 0)) {   // rare: libm for the whole chunk
#pragma unroll 1
                    for (int e = 0; e < 8; ++e) sincos_f32(e < 4 ? z0[e & 3] : z1[e & 3], sv[e], cv[e]);
                } else {
                    f32x2_t s2[4], c2[4];
                    sincos_f32x2_fast(f32x2_t{z0[0], z0[1]}, s2[0], c2[0]);
                    sincos_f32x2_fast(f32x2_t{z0[2], z0[3]}, s2[1], c2[1]);
                    sincos_f32x2_fast(f32x2_t{z1[0], z1[1]}, s2[2], c2[2]);
                    sincos_f32x2_fast(f32x2_t{z1[2], z1[3]}, s2[3], c2[3]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        sv[e] = s2[e >> 1][e & 1];
                        cv[e] = c2[e >> 1][e & 1];
                    }
                }
                u32x4 hi, lo;
                hp_split8(sv, so, hi, lo);
                __builtin_amdgcn_raw_buffer_store_b128(hi, srdHL, vhl, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(lo, srdHL, vhl + 64, 0, 0);
                if (EPI == HPE_SINE_STASH) {
                    buf_store4(p.omega * f32x4{cv[0], cv[1], cv[2], cv[3]}, srdC2, v32, 0);
                    buf_store4(p.omega * f32x4{cv[4], cv[5], cv[6], cv[7]}, srdC2, v32 + 16, 0);
                }
            }
        }
    };

    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    while (true) {
        int t = 0;
        for (; t + 1 < ktiles; t += 2) {
            body(P0{}, t);
            body(P1{}, t + 1);
        }
        if (t < ktiles) {   // odd K-tile count: the next tile's first fragment landed in ah[1]
            body(P0{}, t);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ah[0][i] = ah[1][i];
                bh[0][i] = bh[1][i];
            }
        }
        HP_STAMP(2);
        if (!(HP_ABLATE & 4)) epilogue();
        else if (acc[0][0][0] == 12345.678f) p.C_hl[0] = (char)acc[1][1][1];   // keep the accumulators live
        HP_STAMP(4);
        if (!has_next) break;
        if (nxt.n0 != cur.n0) load_bias(nxt.n0);   // (with G a multiple of 8 * tiles_n a block keeps its column tile)
        zero_acc();
        pend = 1;
        cur = nxt;
        vp += G;
        has_next = vp + G < total;
        if (has_next) nxt = decode(vp + G);
    }
    if (EPI == HPE_MUL && p.amax_out) {
        omax_run = wave_max(omax_run);
        if (lane == 0) hp_atomic_max_bits(p.amax_out, omax_run);
    }
}

// =======================================================================================================================
// Persistent KC kernel with the epilogue of tile T running UNDER the K-loop of tile T+1.
// Measured on gemm_hp_pkc_kernel (-DHP_ABLATE builds, 128^3 workload): K-loop alone 0.34 ms per launch (MFMA-bound), epilogue
// alone 0.38 ms (8 waves of sin/cos + split + stores, nothing on the matrix pipe), together 0.82 ms -- they add, because all
// eight waves of the block are in the same phase.  Here the finished accumulators move to a second register set and are
// converted / stored in eight chunks of 16 x 32 per wave, one chunk per two K-iterations (K = 512; one per iteration at
// K = 256), in between the MFMAs of the next tile: the VALU and the store queue work while the matrix pipe does.
// Fragment registers are single-buffered to pay for the second accumulator set; the MFMA blocks run in the order X (hi x lo),
// Z (hi x hi), Y (lo x hi) so that every fragment of K-tile t+1 has a register to land in one block before it is needed:
//   X(t): MFMA(ah, bl)   | reads al(t), bh(t)            | LDS-DMA part 2 of K-tile t+2
//   -- s_waitcnt vmcnt(N) lgkmcnt(0); s_barrier: stage t is dead, K-tile t+1 visible
//   Z(t): MFMA(ah, bh)   | reads bl(t+1)                 | part 0 of K-tile t+3; chunk: accumulators -> per-wave LDS staging
//   Y(t): MFMA(al, bh)   | reads ah(t+1)                 | part 1 of K-tile t+3; chunk: read back, sin/cos (or * dact), split, stores
// KT = K / 32 is a template parameter: the loop over the K-tiles is fully unrolled (the chunk a given iteration converts
// indexes the register array, which must be static).
// =======================================================================================================================
template <int I, int N, typename F>
__device__ __forceinline__ void hp_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        hp_static_for<I + 1, N>(f);
    }
}

// Packed fp32 VALU instructions beside MFMAs (MI355X_MICROARCH.md, "packed FP32": a v_pk_fma_f32 as filler costs +22 cycles against
// two v_fma_f32).  This kernel's chunk code held 28 of them per chunk (sin / cos range reduction, the scale and omega multiplies);
// the translation unit is therefore compiled without packed fp32 (_build.py: SOURCE_FLAGS; identical results -- the same IEEE
// operations): input-grad launch 0.873 ms instead of 0.903 (-3.1 %) in both interleaved rounds (profiles/r04_nt_ab.txt).  The
// kernels with no MFMAs to share an issue port with (head step, head forward, weight preparation, the exact-fp32 GEMMs' own
// epilogues) carry INR_PACKED_F32 and keep them: the head step is 5 % slower without.  An attribute on THIS kernel alone does
// not work: its lambdas and the HIP header's __shfl_xor keep the default feature set and are then called, not inlined (127 ms/step).
template <int EPI, int KT>
__global__ void __launch_bounds__(HP_NTH, 2) gemm_hp_pkd_kernel(const HpParams p) {
    __shared__ __attribute__((aligned(1024))) char smem[HP_NSTAGE * HP_STAGE + 8 * HP_EPI_WAVE];
    constexpr int STORES = EPI == HPE_SINE_STASH ? 4 : 2;   // stores a chunk iteration issues in its Y block (lower bound)
    static_assert(EPI != HPE_SLAB, "row-split slabs are the one-block-per-tile kernel's business");
    constexpr int MULS = EPI == HPE_MUL ? 2 : 0;            // loads of the element-wise factor it issues in its X block

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int g = lane >> 4, l16 = lane & 15;
    const int total = p.tiles_m * p.tiles_n;
    const int G = gridDim.x;

    struct Tile {
        int m0, n0;
        __amdgpu_buffer_rsrc_t srdA, srdB;
    };
    auto decode = [&](int vp) {
        int logical = xcd_remap(vp, total);
        Tile t;
        const int tn = logical % p.tiles_n, tm = logical / p.tiles_n;
        t.m0 = (p.reverse_m ? p.tiles_m - 1 - tm : tm) * HP_BM;
        t.n0 = tn * HP_BN;
        t.srdA = hp_srd(p.A + (long long)t.m0 * p.pitchA, (p.a_rows - t.m0) * p.pitchA);
        t.srdB = hp_srd(p.B + (long long)t.n0 * p.pitchB, (p.b_rows - t.n0) * p.pitchB);
        return t;
    };
    int vp = blockIdx.x;
    Tile cur = decode(vp), nxt = cur;
    bool has_next = vp + G < total;
    if (has_next) nxt = decode(vp + G);
    int prv_m0 = 0, prv_n0 = 0;     // the tile whose epilogue is in progress
    bool have_prev = false;         // false for a block's first tile

    const int drow = 8 * wave + (lane >> 3);
    const int dslot = ((lane & 7) ^ hp_f(drow)) * 16;
    const int vdmaA = drow * (int)p.pitchA + dslot, vdmaB = drow * (int)p.pitchB + dslot;
    const int pieceA = 64 * (int)p.pitchA, pieceB = 64 * (int)p.pitchB;
    auto dma_part = [&](int stage_off, int j, int part) {
        char* S = smem + stage_off;
        const bool from_next = j >= KT;
        const int soff = (from_next ? j - KT : j) * 128;
        const __amdgpu_buffer_rsrc_t sa = from_next ? nxt.srdA : cur.srdA, sb = from_next ? nxt.srdB : cur.srdB;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if ((i >> 1) != part) continue;
            const int q = wave + 8 * i;
            if (i < 2)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(sa, (__attribute__((address_space(3))) void*)(S + q * 1024), 16, vdmaA,
                                                         soff + i * pieceA, 0, HP_A_AUX);
            else
                __builtin_amdgcn_raw_ptr_buffer_load_lds(sb, (__attribute__((address_space(3))) void*)(S + q * 1024), 16, vdmaB,
                                                         soff + (i - 2) * pieceB, 0, 0);
        }
    };

    const int fx = (g ^ hp_f(l16)) << 4;
    const int fa_hi = (64 * wm + l16) * 128 + fx, fa_lo = fa_hi ^ 64;
    const int fb_hi = HP_A_IMG + (64 * wn + l16) * 128 + fx, fb_lo = fb_hi ^ 64;

    const int ka = hp_scale_exp(p.sa), kb = hp_scale_exp(p.sb);
    float bias_s[4] = {0.f, 0.f, 0.f, 0.f};
    auto load_bias = [&](int n0) {
        if (EPI == HPE_MUL || !p.bias) return;
        const float upa = h3_pow2(ka), upb = h3_pow2(kb);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + 64 * wn + 16 * j + l16;
            const float b = p.bias[col < p.N ? col : p.N - 1];
            bias_s[j] = col < p.N ? (b * upa) * upb : 0.f;
        }
    };
    load_bias(cur.n0);
    f32x4v acc[4][4], accP[4][4];
    half8 ah[4], al[4], bh[4], bl[4];
    auto init_acc = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4v{bias_s[j], bias_s[j], bias_s[j], bias_s[j]};
    };
    init_acc();

    const int er = lane >> 2, ec = (lane & 3) * 8;
    float* const stg = reinterpret_cast<float*>(smem + HP_NSTAGE * HP_STAGE + wave * HP_EPI_WAVE);
    const float inv_a = h3_pow2(-ka), inv_b = h3_pow2(-kb);
    const float so = h3_pow2(hp_scale_exp(p.so));   // HPE_MUL: scale of dz_prev; sine epilogues: scale of the activations' image
    f32x4 mul0 = {0.f, 0.f, 0.f, 0.f}, mul1 = mul0;   // the chunk's element-wise factor: loaded in X, used in Y
    f32x4 cs0 = {0.f, 0.f, 0.f, 0.f}, cs1 = cs0;
    float omax_run = 0.f;

    // ---- the deferred epilogue, chunk c (compile time) of the tile at (prv_m0, prv_n0) ------------------------------------------
    // chunk c = 16 rows x 32 columns: column block jp = c / 4 (outer), row block i = c % 4
    auto load_mul = [&](int c, f32x4& d0, f32x4& d1) {
        const __amdgpu_buffer_rsrc_t srdMul =
            hp_srd((const char*)p.mul + (long long)prv_m0 * p.N * 4, (long long)min(p.M - prv_m0, HP_BM) * p.N * 4);
        const int row = 64 * wm + 16 * (c & 3) + er, cc = prv_n0 + 64 * wn + 32 * (c >> 2) + ec;
        const int vo = cc < p.N ? (row * p.N + cc) * 4 : 0x7FFFFF00;
        d0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdMul, vo, 0, HP_MUL_AUX));
        d1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdMul, vo + 16, 0, HP_MUL_AUX));
    };
    auto chunk_park = [&](auto cc) {
        constexpr int c = decltype(cc)::value, i = c & 3, jp = c >> 2;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int r = 0; r < 4; ++r)   // one v_ldexp_f32 for the two power-of-two factors (the same bits; exact where a product of
                                          // the two would leave the float range)
                stg[(4 * g + r) * 32 + jj * 16 + l16] =
                    HP_UNSCALE_LDEXP ? __builtin_amdgcn_ldexpf(accP[i][2 * jp + jj][r], -(ka + kb)) : accP[i][2 * jp + jj][r] * inv_a * inv_b;
    };
    // (Measured and not kept, round 4: no staging at all -- MFMAs issued as (B fragment, A fragment) leave C transposed per block, four
    //  v_permlane16_swap_b32 per chunk then give every lane eight consecutive columns of one row, the column sums fold by DPP: zero
    //  LDS instructions in the epilogue, but ~100 more VALU instructions per tile: input-grad launch 0.876 against 0.850 ms.)
    f32x4 cv0, cv1;   // the chunk as read back: row er, columns ec .. ec + 7
    auto chunk_read = [&]() {
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the wave's own staging stores have reached the LDS
        __builtin_amdgcn_wave_barrier();
        cv0 = *reinterpret_cast<const f32x4*>(stg + er * 32 + ec);
        cv1 = *reinterpret_cast<const f32x4*>(stg + er * 32 + ec + 4);
    };
    // sin / cos here are ALWAYS the two-FMA reduction to a fraction of a revolution + v_sin_f32 / v_cos_f32 (common.h): no libm
    // fallback (its register appetite would spill the whole kernel).  The reduced fraction stays valid far beyond the 2^20 the
    // in-line kernels switch at -- k = rint(x/2pi) is an exact float integer, fma(x, 1/2pi, -k) is one rounding of an exact
    // difference, and the hardware takes |fraction| up to 256 revolutions -- with an absolute error of about |x| * 2^-41 there
    // (3e-7 below 2^20); inf / NaN arguments give NaN like torch.sin.  SIREN pre-activations are O(10).
    auto chunk_finish = [&](auto cc) {
        constexpr int c = decltype(cc)::value, i = c & 3, jp = c >> 2;
        const long long first = (long long)prv_m0 * p.N * 4;
        const long long win = (long long)min(p.M - prv_m0, HP_BM) * p.N * 4;
        const __amdgpu_buffer_rsrc_t srdHL = hp_srd(p.C_hl + first, win);
        const int row = 64 * wm + 16 * i + er, col = prv_n0 + 64 * wn + 32 * jp + ec;
        const bool ok = col < p.N;
        const int vhl = ok ? row * p.N * 4 + (col >> 5) * 128 + (col & 31) * 2 : 0x7FFFFF00;
        if (EPI == HPE_MUL) {
            const f32x4 o0 = hp_mul_sum(cv0, mul0, cs0), o1 = hp_mul_sum(cv1, mul1, cs1);
            omax_run = fmaxf(omax_run, fmaxf(fmaxf(fmaxf(fabsf(o0[0]), fabsf(o0[1])), fmaxf(fabsf(o0[2]), fabsf(o0[3]))),
                                             fmaxf(fmaxf(fabsf(o1[0]), fabsf(o1[1])), fmaxf(fabsf(o1[2]), fabsf(o1[3])))));
            const float ov[8] = {o0[0], o0[1], o0[2], o0[3], o1[0], o1[1], o1[2], o1[3]};
            u32x4 hi, lo;
            hp_split8(ov, so, hi, lo);
            __builtin_amdgcn_raw_buffer_store_b128(hi, srdHL, vhl, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(lo, srdHL, vhl + 64, 0, 0);
            if (i == 3) {   // the column block's bias-gradient sums are complete: fold the 16 row lanes, store (no branches:
                            // lanes that have nothing to store point past the end of the buffer)
                const long long cbytes = p.colsum ? 2ll * p.tiles_m * p.N * 4 : 0;
                const __amdgpu_buffer_rsrc_t srdCS = hp_srd(p.colsum ? (const void*)p.colsum : (const void*)p.C_hl, cbytes);
                if (HP_COLSUM_TRANSPOSED) {     // (hp_colsum_fold: one 128-byte store of the chunk's 32 columns by the lower half-wave)
                    const float total = hp_colsum_fold(cs0, cs1, lane);
                    const int vcs = (lane < 32 && ok) ? (((prv_m0 / HP_BM) * 2 + wm) * p.N + col + hp_colsum_index(lane)) * 4 : 0x7FFFFF00;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, total), srdCS, vcs, 0, 0);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        cs0[e] += __shfl_xor(cs0[e], 4, 64);
                        cs1[e] += __shfl_xor(cs1[e], 4, 64);
                        cs0[e] += __shfl_xor(cs0[e], 8, 64);
                        cs1[e] += __shfl_xor(cs1[e], 8, 64);
                        cs0[e] += __shfl_xor(cs0[e], 16, 64);
                        cs1[e] += __shfl_xor(cs1[e], 16, 64);
                        cs0[e] += __shfl_xor(cs0[e], 32, 64);
                        cs1[e] += __shfl_xor(cs1[e], 32, 64);
                    }
                    const int vcs = (lane < 4 && ok) ? (((prv_m0 / HP_BM) * 2 + wm) * p.N + col) * 4 : 0x7FFFFF00;
                    buf_store4(cs0, srdCS, vcs, 0);
                    buf_store4(cs1, srdCS, vcs + 16, 0);
                }
                cs0 = f32x4{0.f, 0.f, 0.f, 0.f};
                cs1 = cs0;
            }
        } else if (EPI == HPE_Z) {
            const __amdgpu_buffer_rsrc_t srdC2 = hp_srd((const char*)p.C2 + first, win);
            const int v32 = ok ? (row * p.N + col) * 4 : 0x7FFFFF00;
            buf_store4(cv0, srdC2, v32, 0);
            buf_store4(cv1, srdC2, v32 + 16, 0);
        } else {
            const f32x4 z0 = p.omega * cv0, z1 = p.omega * cv1;
            float sv[8], cvv[8];
            {
                f32x2_t s2[4], c2[4];
                sincos_f32x2_fast(f32x2_t{z0[0], z0[1]}, s2[0], c2[0]);
                sincos_f32x2_fast(f32x2_t{z0[2], z0[3]}, s2[1], c2[1]);
                sincos_f32x2_fast(f32x2_t{z1[0], z1[1]}, s2[2], c2[2]);
                sincos_f32x2_fast(f32x2_t{z1[2], z1[3]}, s2[3], c2[3]);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    sv[e] = s2[e >> 1][e & 1];
                    cvv[e] = c2[e >> 1][e & 1];
                }
            }
            u32x4 hi, lo;
            hp_split8(sv, so, hi, lo);
            __builtin_amdgcn_raw_buffer_store_b128(hi, srdHL, vhl, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(lo, srdHL, vhl + 64, 0, 0);
            if (EPI == HPE_SINE_STASH) {
                const __amdgpu_buffer_rsrc_t srdC2 = hp_srd((const char*)p.C2 + first, win);
                const int v32 = ok ? (row * p.N + col) * 4 : 0x7FFFFF00;
                if (HP_DIAG_NO_OMEGA_STASH) {
                    buf_store4(f32x4{cvv[0], cvv[1], cvv[2], cvv[3]}, srdC2, v32, 0);
                    buf_store4(f32x4{cvv[4], cvv[5], cvv[6], cvv[7]}, srdC2, v32 + 16, 0);
                } else {
                    buf_store4(p.omega * f32x4{cvv[0], cvv[1], cvv[2], cvv[3]}, srdC2, v32, 0);
                    buf_store4(p.omega * f32x4{cvv[4], cvv[5], cvv[6], cvv[7]}, srdC2, v32 + 16, 0);
                }
            }
        }
    };
    // all eight chunks of the tile in accP, one after the other (the drain after the last tile)
    auto epilogue_now = [&]() {
        hp_static_for<0, 8>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            chunk_park(cc);
            if (EPI == HPE_MUL) load_mul(c, mul0, mul1);
            chunk_read();
            chunk_finish(cc);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
        });
    };

    // ---- prologue of the block's first tile: K-tiles 0, 1 and two thirds of 2 in flight -----------------------------------------
    if (p.stagger > 0) {
        for (int k = ((blockIdx.x >> 3) + blockIdx.x) & 7; k > 0; --k)
            for (int q = 0; q < p.stagger; q += 100) __builtin_amdgcn_s_sleep(100);
    }
    HP_STAMP(0);
    int so3[3] = {0, HP_STAGE, 2 * HP_STAGE};   // byte offset of the stage of tile-local K-tile t: so3[t % 3]
#pragma unroll
    for (int part = 0; part < 3; ++part) dma_part(so3[0], 0, part);
#pragma unroll
    for (int part = 0; part < 3; ++part) dma_part(so3[1], 1, part);
    dma_part(so3[2], 2, 0);
    dma_part(so3[2], 2, 1);
    __builtin_amdgcn_s_waitcnt(hp_vmcnt(10));
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ah[i] = *reinterpret_cast<const half8*>(smem + so3[0] + fa_hi + i * 2048);
        bl[i] = *reinterpret_cast<const half8*>(smem + so3[0] + fb_lo + i * 2048);
    }
    HP_STAMP(1);
    int last_extra = 0;   // 1: the previous iteration issued EXTRA chunk operations behind its transfers

    // One K-iteration; from a block's second tile on the previous tile's epilogue rides along: chunk t / PERIOD in the
    // iterations t that are multiples of PERIOD = KT / 8 -- parked in the staging LDS under the Z block, read back, converted
    // and stored behind the MFMAs of the Y block.
    // (Measured alternatives, 128^3 workload, ms per forward launch: epilogue in line (gemm_hp_pkc_kernel) 0.83; this 0.80;
    //  the two waves of a SIMD converting in alternate iterations, right behind the barrier, 1.01 -- a wave sits 2.5-3.8 k
    //  cycles in its four stores (the CU's store path takes about 20 B/clk) and the other half waits for it at the next barrier.)
    constexpr int PERIOD = KT / 8;
    static_assert(KT % 8 == 0 && KT >= 8, "one chunk per KT / 8 iterations");
    auto iteration = [&](auto tc) {
        constexpr int t = decltype(tc)::value;
        constexpr bool SLOT = t % PERIOD == 0;
        constexpr int c = t / PERIOD;
        const bool mine = SLOT && have_prev && !(HP_ABLATE & 4);   // (diagnostic builds: bit 4 = no epilogue work)
        const char* S = smem + so3[t % 3];
        const char* S1 = smem + so3[(t + 1) % 3];
        const bool more2 = t + 2 < KT || has_next, more3 = t + 3 < KT || has_next;
        // X: hi x lo
        if (EPI == HPE_MUL && mine) load_mul(c, mul0, mul1);   // (ahead of the transfers below: waiting for it must not wait for them)
        if (more2 && !(HP_ABLATE & 1)) dma_part(so3[(t + 2) % 3], t + 2, 2);
        if (!(HP_ABLATE & 8)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                al[i] = *reinterpret_cast<const half8*>(S + fa_lo + i * 2048);
                bh[i] = *reinterpret_cast<const half8*>(S + fb_hi + i * 2048);
            }
        }
        if (!(HP_ABLATE & 2)) h3_mfma16(acc, ah, bl);
        h3_sched<16, 0, 0, 8, 0, 0>();
        __builtin_amdgcn_sched_barrier(0);
        // K-tile t+1 has landed; allowed to stay in flight: the six transfers of K-tile t+2, the chunk stores of the previous
        // iteration and the factor loads of this one (all issued behind K-tile t+1's last transfer)
        {
            const bool now = mine && MULS > 0;
            if (!more2) __builtin_amdgcn_s_waitcnt(hp_vmcnt(0) & 0xF0FF);
            else if (last_extra && now) __builtin_amdgcn_s_waitcnt(hp_vmcnt(6 + STORES + MULS) & 0xF0FF);
            else if (last_extra) __builtin_amdgcn_s_waitcnt(hp_vmcnt(6 + STORES) & 0xF0FF);
            else if (now) __builtin_amdgcn_s_waitcnt(hp_vmcnt(6 + MULS) & 0xF0FF);
            else __builtin_amdgcn_s_waitcnt(hp_vmcnt(6) & 0xF0FF);
        }
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // Z: hi x hi
        if (more3 && !(HP_ABLATE & 1)) dma_part(so3[t % 3], t + 3, 0);
        if (mine) chunk_park(std::integral_constant<int, c>{});
        if (!(HP_ABLATE & 8)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) bl[i] = *reinterpret_cast<const half8*>(S1 + fb_lo + i * 2048);   // (stale bytes past the end)
        }
        if (!(HP_ABLATE & 2)) h3_mfma16(acc, ah, bh);
        __builtin_amdgcn_sched_barrier(0);
        // Y: lo x hi
        if (more3 && !(HP_ABLATE & 1)) dma_part(so3[t % 3], t + 3, 1);
        if (mine) chunk_read();
        if (!(HP_ABLATE & 8)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) ah[i] = *reinterpret_cast<const half8*>(S1 + fa_hi + i * 2048);
        }
        if (!(HP_ABLATE & 2)) h3_mfma16(acc, al, bh);
        if (mine) chunk_finish(std::integral_constant<int, c>{});
        __builtin_amdgcn_sched_barrier(0);
        last_extra = mine ? 1 : 0;
    };
    while (true) {
        hp_static_for<0, KT>(iteration);
        HP_STAMP(2);
        have_prev = true;
        // this tile's accumulators become the deferred set
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) accP[i][j] = acc[i][j];
        prv_m0 = cur.m0;
        prv_n0 = cur.n0;
        if (!has_next) break;
        last_extra = 0;
        if (nxt.n0 != cur.n0) load_bias(nxt.n0);
        init_acc();
        // rotate the ring bookkeeping: tile-local K-tile 0 of the next tile continues where this one stopped
        {
            const int a = so3[KT % 3], b = so3[(KT + 1) % 3], c2 = so3[(KT + 2) % 3];
            so3[0] = a;
            so3[1] = b;
            so3[2] = c2;
        }
        cur = nxt;
        vp += G;
        has_next = vp + G < total;
        if (has_next) nxt = decode(vp + G);
    }
    // drain: the last tile's epilogue, nothing left to hide it under
    if (!(HP_ABLATE & 4)) epilogue_now();
    else if (accP[0][0][0] == 12345.678f) p.C_hl[0] = (char)accP[1][1][1];   // (diagnostic builds: keep the accumulators live)
    HP_STAMP(4);
    if (EPI == HPE_MUL && p.amax_out) {
        omax_run = wave_max(omax_run);
        if (lane == 0) hp_atomic_max_bits(p.amax_out, omax_run);
    }
}
