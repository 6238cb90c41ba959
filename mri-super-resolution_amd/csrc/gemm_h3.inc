// Split-fp16 MFMA GEMM ("h3"): fp32-equivalent products on the half-precision matrix cores.  Included by gemm_f32.hip; the number
// format's helpers (h3_split2, h3_scale_exp, h3_mfma16, ...) are in split_fp16.h.
//
// Every fp32 operand element a is represented as hi + lo with hi = fp16(a * s), lo = fp16(a * s - hi), both rounded to nearest (hi + lo = a s to 2^-24)
// for a power-of-two tensor scale s that places max|a| * s in [2^14, 2^15); a * s - hi is exact in fp32, so
// a * s = hi + lo up to 2^-21 |a * s| (elements far below the tensor maximum bottom out at the fp16 subnormal spacing,
// 2^-39 of the maximum -- irrelevant in a norm-wise sense).  A product a * b then costs three
// v_mfma_f32_16x16x32_f16 (hi*lo, lo*hi, hi*hi; the lo*lo term, 2^-22 relative, is dropped) with fp32 accumulation,
// against one f32-input MFMA at 1/16 of the fp16 rate: 16/3 = 5.3x the fp32-MFMA ceiling per clock.
// Measured error of a 4-layer SIREN forward against fp64 (tools/split_emul.py): fp32 MFMA 6.1e-7, this 7.0e-7;
// parameter / input gradients 1.8e-7 / 3.4e-7 against 0.8e-7 / 2.7e-7 -- the parity tiers (1e-5) do not move.
//
// Who splits what (VALU is the scarce resource next to a 16-cycle MFMA):
//   * weights are split ONCE per optimizer step by weight_split_kernel into four fp16 planes (hi/lo, [out][in] and
//     [in][out]) -- the B operand of the forward and input-gradient GEMMs arrives ready-made (zero VALU);
//   * activations / Fourier features are in [-1, 1]: no scale, 2 VALU per element (cvt_pkrtz, fma_mix, cvt_pkrtz);
//   * dz is scaled by 2^k from the exact max|dz| of the producing kernel (atomic max on the float bits: order
//     independent, so runs stay bitwise reproducible), 3 VALU per element.
// LDS image of a 128 x 32 operand tile: plane (piece p, k-octet g), 2048 B, holds for every row the 8 halves a lane
// feeds to one MFMA (16 B) at 16 * (slot(r) ^ 2g).  The row permutation is chosen against the LDS lane groups of
// gfx950 (MI355X_MICROARCH.md, LDS table): a ds_read_b128 group is {rows 0-3, 12-15 of octet g} + {rows 4-11 of octet
// g^1} -- disjoint 16-byte slots of one 256-byte window; a ds_write_b128 group (8 consecutive lanes = 2 rows x 4
// octets, banks mod 128 B) covers 128 B exactly once; the ds_write_b64 groups of the transposing loaders are 2-way.
#ifndef H3_EXTRA_LDS
#define H3_EXTRA_LDS 0   // diagnostic builds: pad the LDS allocation to force one block per CU
#endif
#ifndef H3_B_DMA
#define H3_B_DMA 0      // 1: pre-split B planes go global -> LDS by buffer_load ... lds (no VGPRs, no ds_write).  Correct, but
                        // measured 20 % SLOWER: with this LDS image the 64 lanes of a transfer fetch 16 B from 64 different
                        // rows (64 cache lines per instruction against 16 on the register path).  Needs a row-major image:
                        // [row][4 x 16 B] with octet g stored in slot g ^ f((row >> 2) & 3), f = {0, 2, 3, 1} -- a transfer
                        // then covers 16 rows x 64 contiguous bytes, 16-byte fragment reads and the k-contiguous stores
                        // stay conflict-free; only the 8-byte stores of the transposing loaders become 4-way.
#endif
#ifndef H3_ABLATE
#define H3_ABLATE 0      // diagnostic builds (-DH3_ABLATE=bits, tools/h3_ablate.py): 1 no K-loop loads, 2 no split/park, 4 no
                        // fragment reads, 8 no epilogue.  Compile-time on purpose: a run-time branch splits scheduling regions.
#endif
#ifdef INR_STAMPS   // diagnostic builds only (tools/build_stamps.sh, tools/h3_stamps.py): 16 x u64 per wave
#define H3_STAMP(slot)                                                                                  \
    do {                                                                                                \
        if (p.stamps && (threadIdx.x & 63) == 0) {                                                      \
            unsigned long long t_;                                                                      \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                  \
            p.stamps[((long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16 + (slot)] = t_; \
        }                                                                                               \
    } while (0)
#else
#define H3_STAMP(slot)
#endif
enum H3Operand { H3_F32_KC = 0, H3_F32_RC = 1, H3_SPLIT_KC = 2 };

__device__ __forceinline__ int h3_slot(int r, int g) { return ((r & ~3) | ((r + (r >> 3)) & 3)) ^ (g << 1); }
__device__ __forceinline__ int h3_slot_inv(int s, int g) {   // the row whose fragment sits in slot s of octet g
    const int u = s ^ (g << 1);
    return (u & ~3) | ((u - (u >> 3)) & 3);
}

struct H3Regs {
    u32x4 q[4];   // raw 16-byte global loads of one operand tile
};

// Operand tiles have ROWS rows x 32 k and are moved by NTH threads; every thread handles (ROWS * 4 / NTH) (row, k-octet)
// pairs of a k-contiguous tile.  ROWS = 128, NTH = 256: two passes; ROWS = 128, NTH = 512: one; ROWS = 256, NTH = 512: two.
template <int MODE, int ROWS, int NTH>
struct H3Mover {
    static constexpr int PASSES = ROWS * 4 / NTH;
    static constexpr int PLANE = ROWS * 16;                 // bytes: one 16-byte slot per row
    static constexpr int TILE = 8 * PLANE;                  // hi/lo x 4 k-octets
    static constexpr int NLOAD = MODE == H3_F32_RC ? 4 : 2 * PASSES;
    static_assert(MODE != H3_F32_RC || (ROWS == 128 && NTH == 256), "transposing loader: 128 rows, 256 threads");
    static_assert(PASSES == 1 || PASSES == 2, "tile / thread count combination");

    // this thread's byte offsets inside the block's SRD window at K-tile 0
    static __device__ __forceinline__ void voffsets(int (&voff)[4], int ld, int tid) {
        if (MODE == H3_F32_KC) {          // rows tid/4 (+NTH/4), floats 8g .. 8g+7
#pragma unroll
            for (int i = 0; i < 4; ++i)
                voff[i] = (((tid >> 2) + (NTH / 4) * (i >> 1)) * ld + (tid & 3) * 8 + (i & 1) * 4) * 4;
        } else if (MODE == H3_F32_RC) {   // k = 4*(tid/32) + i, rows 4*(tid%32) .. +3: 32 consecutive lanes read 512 contiguous bytes
#pragma unroll
            for (int i = 0; i < 4; ++i) voff[i] = ((4 * (tid >> 5) + i) * ld + (tid & 31) * 4) * 4;
        } else {                          // fp16 planes: q[pass] from the hi plane, q[2 + pass] from the lo plane
#pragma unroll
            for (int i = 0; i < 4; ++i) voff[i] = (((tid >> 2) + (NTH / 4) * (i & 1)) * ld + (tid & 3) * 8) * 2;
        }
    }

    static __device__ __forceinline__ void load(H3Regs& r, __amdgpu_buffer_rsrc_t srd, __amdgpu_buffer_rsrc_t srd_lo,
                                                const int (&voff)[4], int soff) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (MODE == H3_SPLIT_KC) {
                if ((i & 1) < PASSES) r.q[i] = __builtin_amdgcn_raw_buffer_load_b128(i >= 2 ? srd_lo : srd, voff[i], soff, 0);
            } else if (MODE == H3_F32_RC || (i >> 1) < PASSES) {
                r.q[i] = __builtin_amdgcn_raw_buffer_load_b128(srd, voff[i], soff, 0);
            }
        }
    }

    // split (if needed) and park one operand tile in its LDS image
    template <bool SCALED>
    static __device__ __forceinline__ void store(char* __restrict__ S, const H3Regs& r, float scale, int tid) {
        if (MODE == H3_F32_KC) {
            const int g = tid & 3;
#pragma unroll
            for (int pass = 0; pass < PASSES; ++pass) {
                const int row = (tid >> 2) + (NTH / 4) * pass;
                const f32x4 x0 = __builtin_bit_cast(f32x4, r.q[2 * pass]), x1 = __builtin_bit_cast(f32x4, r.q[2 * pass + 1]);
                half2v h[4], l[4];
                h3_split2<SCALED>(x0[0], x0[1], scale, h[0], l[0]);
                h3_split2<SCALED>(x0[2], x0[3], scale, h[1], l[1]);
                h3_split2<SCALED>(x1[0], x1[1], scale, h[2], l[2]);
                h3_split2<SCALED>(x1[2], x1[3], scale, h[3], l[3]);
                const int off = h3_slot(row, g) * 16;
                *reinterpret_cast<u32x4*>(S + g * PLANE + off) = __builtin_bit_cast(u32x4, h);
                *reinterpret_cast<u32x4*>(S + (4 + g) * PLANE + off) = __builtin_bit_cast(u32x4, l);
            }
        } else if (MODE == H3_F32_RC) {
            // (the 8-byte stores of 16 consecutive lanes land on 8 slot positions: a 2-way bank conflict, 4 -> 8 LDS
            //  cycles per store.  Giving the low lane bit to the k half removes it, but makes every wave load interleave
            //  two rows, which the FETCH_SIZE counter can no longer be calibrated for; LDS is not what bounds the loop.)
            const int kq = tid >> 5, g = kq >> 1, r0 = (tid & 31) * 4;
            f32x4 m[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) m[i] = __builtin_bit_cast(f32x4, r.q[i]);   // m[k][r]
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                half2v h[2], l[2];
                h3_split2<SCALED>(m[0][rr], m[1][rr], scale, h[0], l[0]);
                h3_split2<SCALED>(m[2][rr], m[3][rr], scale, h[1], l[1]);
                const int off = h3_slot(r0 + rr, g) * 16 + (kq & 1) * 8;
                *reinterpret_cast<unsigned long long*>(S + g * PLANE + off) = __builtin_bit_cast(unsigned long long, h);
                *reinterpret_cast<unsigned long long*>(S + (4 + g) * PLANE + off) = __builtin_bit_cast(unsigned long long, l);
            }
        } else {
            const int g = tid & 3;
#pragma unroll
            for (int pass = 0; pass < PASSES; ++pass) {
                const int off = h3_slot((tid >> 2) + (NTH / 4) * pass, g) * 16;
                *reinterpret_cast<u32x4*>(S + g * PLANE + off) = r.q[pass];
                *reinterpret_cast<u32x4*>(S + (4 + g) * PLANE + off) = r.q[2 + pass];
            }
        }
    }
};

struct H3Main {   // operands that stay live through a whole K-tile
    half8 ah[4], bh[4];
};

// AMODE / BMODE: H3_F32_KC (k-contiguous fp32), H3_F32_RC (row-contiguous fp32), H3_SPLIT_KC (pre-split fp16 planes, B only)
// A_SCALED / B_SCALED: the fp32 operand is multiplied by its power-of-two tensor scale before the split
// NWN: waves along n (2 -> 128 x 128 tile, 256 threads, two blocks per CU; 4 -> 128 x 256 tile, 512 threads, one block
//      per CU: every wave still owns 64 x 64, but an A tile now feeds 256 columns -- 25 % fewer operand bytes through
//      L2 per FLOP and half the A split work; L2 bandwidth is what bounds the K-loop, see DESIGN.md 4)
//
// One K-tile = 48 MFMAs per wave in three blocks that retire operand registers early:
//   X: hi(A) x lo(B)   -- meanwhile tile t+1 (in registers) is split and parked in the other LDS image
//   Y: lo(A) x hi(B)   -- in front of it the A loads of tile t+3 (two raw A sets, swapped by unrolling the loop by two:
//                         at fp16 MFMA speed one K-tile is shorter than an HBM round trip); barrier at the end
//   Z: hi(A) x hi(B)   -- in front of it the B loads of tile t+2 (weights come from L2: one set); meanwhile tile t+1's
//                         lo fragments are read into the registers X and Y freed; its hi fragments follow once Z issued
// The conditional load groups sit BETWEEN the blocks: a branch inside one would split it, and sched_group_barrier only
// orders instructions of one basic block (an earlier version with run-time switches inside the blocks lost all
// interleaving -- and ran at the same speed: the loop is bound by L2 bandwidth, not by issue).
template <int AMODE, int BMODE, bool A_SCALED, bool B_SCALED, int EPI, int NWN>
__global__ void __launch_bounds__(128 * NWN, NWN == 2 ? 2 : 1) gemm_h3_kernel(const GemmParams p) {
    constexpr int NTH = 128 * NWN, BN_ = 64 * NWN, NWAVES = 2 * NWN;
    using MA = H3Mover<AMODE, BM, NTH>;
    using MB = H3Mover<BMODE, BN_, NTH>;
    constexpr int STAGE = MA::TILE + MB::TILE;
    constexpr int EPI_BYTES = NWAVES * 64 * SUB16 * 4;
    constexpr int SMEM_BYTES = ((2 * STAGE > EPI_BYTES) ? 2 * STAGE : EPI_BYTES) + H3_EXTRA_LDS;
    __shared__ __attribute__((aligned(16))) char smem[SMEM_BYTES];
    constexpr bool A_KC = AMODE != H3_F32_RC, B_KC = BMODE != H3_F32_RC;
    constexpr int B_ELT = BMODE == H3_SPLIT_KC ? 2 : 4;
    // instruction counts of one operand's split + park (for the interleave recipe)
    constexpr int A_VALU = (A_SCALED ? 24 : 16) * (AMODE == H3_F32_RC ? 2 : MA::PASSES);
    constexpr int B_VALU = BMODE == H3_SPLIT_KC ? 0 : (B_SCALED ? 24 : 16) * (BMODE == H3_F32_RC ? 2 : MB::PASSES);
    constexpr int A_WR = AMODE == H3_F32_RC ? 8 : 2 * MA::PASSES, B_WR = BMODE == H3_F32_RC ? 8 : 2 * MB::PASSES;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / NWN, wn = wave % NWN;
    const int g = lane >> 4, l16 = lane & 15;
    const TileCoord tc = decode_block(p);
    const int m0 = tc.tile_m * BM, n0 = tc.tile_n * BN_;
    const int k_begin = tc.split * p.k_per_split;
    const int k_end = min(p.K, k_begin + p.k_per_split);
    const int ktiles = (k_end - k_begin + BK - 1) / BK;
    const long long a_first = A_KC ? ((long long)m0 * p.lda + k_begin) : ((long long)k_begin * p.lda + m0);
    const long long b_first = B_KC ? ((long long)n0 * p.ldb + k_begin) : ((long long)k_begin * p.ldb + n0);
    const long long a_span = A_KC ? (long long)BM * p.lda : (long long)(k_end - k_begin) * p.lda;
    const long long b_span = B_KC ? (long long)BN_ * p.ldb : (long long)(k_end - k_begin) * p.ldb;
    const __amdgpu_buffer_rsrc_t srdA = make_srd(p.A + a_first, min(p.a_elems - a_first, a_span) * 4);
    __amdgpu_buffer_rsrc_t srdB, srdBlo;
    if (BMODE == H3_SPLIT_KC) {
        const long long bytes = min(p.b_elems - b_first, b_span) * 2;
        srdB = make_srd(reinterpret_cast<const float*>(p.Bh + b_first), bytes);
        srdBlo = make_srd(reinterpret_cast<const float*>(p.Bl + b_first), bytes);
    } else {
        srdB = make_srd(p.B + b_first, min(p.b_elems - b_first, b_span) * 4);
        srdBlo = srdB;
    }
    const int a_step = (A_KC ? BK : BK * p.lda) * 4;
    const int b_step = (B_KC ? BK : BK * p.ldb) * B_ELT;
    int va[4], vb[4];
    MA::voffsets(va, p.lda, tid);
    MB::voffsets(vb, p.ldb, tid);
    const int ka = p.a_amax ? h3_scale_exp(*p.a_amax) : 0;
    const int kb = p.b_amax ? h3_scale_exp(*p.b_amax) : 0;
    const float sa = h3_pow2(ka), sb = h3_pow2(kb);
    // B by LDS-DMA: the image is 8 * MB::PLANE bytes = 4 one-KB wave transfers per wave; transfer q = 4 * wave + i fills
    // 64 consecutive slots of plane q * 1024 / PLANE, and lane l fetches the row that belongs in its slot
    constexpr bool B_DMA = BMODE == H3_SPLIT_KC && H3_B_DMA != 0;
    int vdma[4];
    if (B_DMA) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = 4 * wave + i, plane = (q * 1024) / MB::PLANE, gq = plane & 3;
            const int slot0 = ((q * 1024) % MB::PLANE) / 16;
            vdma[i] = (h3_slot_inv(slot0 + lane, gq) * p.ldb + gq * 8) * 2;
        }
    }
    auto dma_b = [&](char* stage, int soff) {   // wave-uniform LDS destination, per-lane global source
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = 4 * wave + i;
            const bool lo_plane = (q * 1024) / MB::PLANE >= 4;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(lo_plane ? srdBlo : srdB,
                                                     (__attribute__((address_space(3))) void*)(stage + MA::TILE + q * 1024), 16,
                                                     vdma[i], soff, 0, 0);
        }
    };

    f32x4v acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4v{0.f, 0.f, 0.f, 0.f};
#ifdef INR_STAMPS
    if (p.stamps && lane == 0)
        p.stamps[((long long)blockIdx.x * NWAVES + wave) * 16 + 10] =
            ((unsigned long long)__builtin_amdgcn_s_getreg((32 - 1) << 11 | 0 << 6 | 20) << 32) |
            __builtin_amdgcn_s_getreg((32 - 1) << 11 | 0 << 6 | 4);
#endif
    H3_STAMP(0);

    const int arow = wm * 64 + l16, brow = wn * 64 + l16;
    int oa[4], ob[4];   // byte offsets of this lane's four A / B fragment rows inside a plane
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        oa[i] = g * MA::PLANE + h3_slot(arow + 16 * i, g) * 16;
        ob[i] = MA::TILE + g * MB::PLANE + h3_slot(brow + 16 * i, g) * 16;
    }
    H3Regs ra0, ra1, rb;
    H3Main F;
    half8 al[4], bl[4];

    auto read_hi = [&](const char* S) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            F.ah[i] = *reinterpret_cast<const half8*>(S + oa[i]);
            F.bh[i] = *reinterpret_cast<const half8*>(S + ob[i]);
        }
    };
    auto read_lo = [&](const char* S) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            al[i] = *reinterpret_cast<const half8*>(S + 4 * MA::PLANE + oa[i]);
            bl[i] = *reinterpret_cast<const half8*>(S + 4 * MB::PLANE + ob[i]);
        }
    };
    int a_off = 0, b_off = 0;
    auto load_next_a = [&](H3Regs& ra) {
        a_off += a_step;
        MA::load(ra, srdA, srdA, va, a_off);
    };
    auto load_next_b = [&]() {
        b_off += b_step;
        MB::load(rb, srdB, srdBlo, vb, b_off);
    };
    // K-tile t: operands in F / al / bl; `ra` holds A of tile t+1 (and is refilled with tile t+3), rb holds B of tile
    // t+1 (refilled with tile t+2)
    auto body = [&](H3Regs& ra, int t) {
        char* nS = smem + ((t & 1) ^ 1) * STAGE;
        if (t == 4) H3_STAMP(2);
        if constexpr (B_DMA) {   // tile t+1's B planes straight into the other LDS image (its readers passed barrier t-1)
            b_off += b_step;
            dma_b(nS, b_off);
        }
        if constexpr (!(H3_ABLATE & 2)) {
            MA::template store<A_SCALED>(nS, ra, sa, tid);
            if constexpr (!B_DMA) MB::template store<B_SCALED>(nS + MA::TILE, rb, sb, tid);
        }
        h3_mfma16(acc, F.ah, bl);
        h3_sched<16, A_VALU + (B_DMA ? 0 : B_VALU) + 8, A_WR + (B_DMA ? 0 : B_WR), 0, 0, 0>();
        __builtin_amdgcn_sched_barrier(0);
        if (t == 4) H3_STAMP(3);
        const bool more_a = !(H3_ABLATE & 1) && t + 3 < ktiles;
        if (more_a) load_next_a(ra);
        h3_mfma16(acc, al, F.bh);
        __builtin_amdgcn_sched_barrier(0);
        if (t == 4) H3_STAMP(4);
        if constexpr (B_DMA) {   // vmcnt is in order: the DMA transfers are older than the A loads just issued
            if (more_a) __builtin_amdgcn_s_waitcnt(0x0F70 | MA::NLOAD);
            else __builtin_amdgcn_s_waitcnt(0x0F70);
        }
        __syncthreads();
        if (t == 4) H3_STAMP(5);
        if constexpr (!B_DMA) {
            if (!(H3_ABLATE & 1) && t + 2 < ktiles) load_next_b();
        }
        if constexpr (!(H3_ABLATE & 4)) read_lo(nS);
        h3_mfma16(acc, F.ah, F.bh);
        h3_sched<16, 0, 0, 8, 0, 0>();
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!(H3_ABLATE & 4)) read_hi(nS);
        if (t == 4) H3_STAMP(6);
    };
    auto last = [&]() {
        h3_mfma16(acc, F.ah, bl);
        h3_mfma16(acc, al, F.bh);
        h3_mfma16(acc, F.ah, F.bh);
    };

    if (ktiles > 0) {
        MA::load(ra0, srdA, srdA, va, 0);
        if constexpr (B_DMA) dma_b(smem, 0);
        else MB::load(rb, srdB, srdBlo, vb, 0);
        if (ktiles > 1) load_next_a(ra1);
        MA::template store<A_SCALED>(smem, ra0, sa, tid);
        if constexpr (!B_DMA) {
            MB::template store<B_SCALED>(smem + MA::TILE, rb, sb, tid);
            if (ktiles > 1) load_next_b();
        }
        if (ktiles > 2) load_next_a(ra0);
        if constexpr (B_DMA) {   // tile 0's planes must have landed; up to two A tiles may stay in flight behind them
            if (ktiles > 2) __builtin_amdgcn_s_waitcnt(0x0F70 | (2 * MA::NLOAD));
            else if (ktiles > 1) __builtin_amdgcn_s_waitcnt(0x0F70 | MA::NLOAD);
            else __builtin_amdgcn_s_waitcnt(0x0F70);
        }
    }
    __syncthreads();
    if (ktiles > 0) {
        read_lo(smem);
        read_hi(smem);
    }
    const EpiAddr ea = epi_addr<EPI>(p, m0, n0, wm, wn, lane, tc.split);
    f32x4 mulreg[16];
    H3_STAMP(1);
    // invariant at the top of the unrolled pair (t even): A of tile t+1 in ra1, of tile t+2 in ra0, B of tile t+1 in rb
    int t = 0;
    for (; t + 2 < ktiles; t += 2) {
        body(ra1, t);
        body(ra0, t + 1);
    }
    if (t + 1 < ktiles) {
        body(ra1, t);
        ++t;
    }
    if (EPI == EPI_MUL) {   // the element-wise factor of the epilogue travels under the last K-tile
#pragma unroll
        for (int q = 0; q < 16; ++q) mulreg[q] = buf_load4(ea.srdMul, ea.voff, q * ea.row_step);
    }
    if (t < ktiles) last();
    H3_STAMP(7);

    if constexpr ((H3_ABLATE & 8) != 0) {
        if (acc[0][0][0] == 12345.678f) p.C[0] = acc[1][1][1];
        return;
    }
    __syncthreads();  // operand images are dead: LDS becomes the epilogue staging area
    const float inv_a = h3_pow2(-ka), inv_b = h3_pow2(-kb);   // applied one after the other: 2^-(ka+kb) may underflow
    float* sub = reinterpret_cast<float*>(smem) + wave * (64 * SUB16);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) sub[(i * 16 + 4 * g + r) * SUB16 + j * 16 + l16] = acc[i][j][r] * inv_a * inv_b;
    H3_STAMP(8);
    epilogue_rows<EPI, SUB16>(p, sub, ea, mulreg, n0, wn, lane, tc.tile_m * 2 + wm);
    H3_STAMP(9);
}

// ---- weight split: once per optimizer step -----------------------------------------------------------------------------
// W [out][in] fp32 -> Wh/Wl [out][in] and WhT/WlT [in][out] fp16, scaled by the power of two derived from max|W| (which
// weight_amax_kernel left in *amax).  One block per 64 x 64 tile; the transposed planes go through LDS so that both
// images are written with contiguous 128-byte rows.
struct WeightSplitJob {
    const float* W;
    _Float16 *hi, *lo, *hiT, *loT;
    unsigned* amax;
    int out_f, in_f;
};
struct WeightSplitJobs {
    WeightSplitJob job[8];
};

__global__ void __launch_bounds__(256) INR_PACKED_F32 weight_amax_kernel(const WeightSplitJobs jobs) {
    const WeightSplitJob j = jobs.job[blockIdx.y];
    const int n = j.out_f * j.in_f;
    unsigned m = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) m = max(m, __float_as_uint(j.W[i]) & 0x7fffffffu);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(j.amax, m);
}

__global__ void __launch_bounds__(256) INR_PACKED_F32 weight_split_kernel(const WeightSplitJobs jobs) {
    __shared__ _Float16 th[64][66], tl[64][66];
    const WeightSplitJob j = jobs.job[blockIdx.y];
    const int tiles_i = (j.in_f + 63) / 64, tiles_o = (j.out_f + 63) / 64;
    if ((int)blockIdx.x >= tiles_i * tiles_o) return;
    const int o0 = (blockIdx.x / tiles_i) * 64, i0 = (blockIdx.x % tiles_i) * 64;
    const float s = h3_pow2(h3_scale_exp(*j.amax));
    const int c2 = (threadIdx.x & 31) * 2, r8 = threadIdx.x >> 5;   // column pair, row phase
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
        const int o = o0 + r8 + 8 * rr, c = i0 + c2;
        half2v h = {(_Float16)0.f, (_Float16)0.f}, l = h;
        if (o < j.out_f && c + 1 < j.in_f) {
            const long long at = (long long)o * j.in_f + c;
            h3_split2<true>(j.W[at], j.W[at + 1], s, h, l);
            *reinterpret_cast<half2v*>(j.hi + at) = h;
            *reinterpret_cast<half2v*>(j.lo + at) = l;
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
            const long long at = (long long)c * j.out_f + o;
            *reinterpret_cast<half2v*>(j.hiT + at) = half2v{th[r8 + 8 * rr][c2], th[r8 + 8 * rr][c2 + 1]};
            *reinterpret_cast<half2v*>(j.loT + at) = half2v{tl[r8 + 8 * rr][c2], tl[r8 + 8 * rr][c2 + 1]};
        }
    }
}

// max |x| of a tensor as float bits (atomic max; *out must be zero beforehand)
__global__ void __launch_bounds__(256) INR_PACKED_F32 tensor_amax_kernel(unsigned* __restrict__ out, const float* __restrict__ x, long long n) {
    unsigned m = 0;
    const long long n4 = n >> 2;
    const u32x4* x4 = reinterpret_cast<const u32x4*>(x);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const u32x4 v = x4[i];
        m = max(max(m, v[0] & 0x7fffffffu), max(max(v[1] & 0x7fffffffu, v[2] & 0x7fffffffu), v[3] & 0x7fffffffu));
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) m = max(m, __float_as_uint(x[n4 * 4 + threadIdx.x]) & 0x7fffffffu);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}
