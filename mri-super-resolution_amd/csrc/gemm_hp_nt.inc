// Narrow-tile form of the pre-split (HL32) K-contiguous GEMM: 64 x 128 output tiles, four waves (2 x 2, each 32 x 64), one
// block per tile and per CU, a SIX-stage operand ring.  Included by gemm_hp.hip behind gemm_hp.inc (same operand format, same LDS images, same
// three-product arithmetic, same epilogues).
//
// Why it exists.  The 128 x 256 tiles of gemm_hp_pkd / pkc are what the big fits want (one 8-wave block per CU, 48 MFMAs per
// wave and K-tile), but a launch needs 256 of them to touch every CU once: a fit of a few thousand rows (BASELINE config 1:
// 4,096 rows x 512 columns = 64 wide tiles) ran on a quarter of the chip, 20-28 us per GEMM where the work is worth 2.5 us of
// the machine (profiles/r03_small_n.txt).  Here a tile is a quarter of the wide one: 4,096 x 512 gives 256 tiles.  Per FLOP it
// is the less efficient shape -- 12 fragment reads per 24 MFMAs instead of 16 per 48, one wave per SIMD and block -- which is
// why it takes a launch only as a WHOLE, and only one whose wide tiles would leave a quarter of the CUs idle (hp_kc_choice in
// gemm_hp.hip; handing it the remainder rows of a large launch was measured and dropped, see there).
//
// LDS: stage = A image 64 rows x 128 B (8 KB) + B image 128 rows x 128 B (16 KB); six stages = 144 KB, reused as the
// epilogue staging area (4 waves x 32 rows x 68 floats).  DMA: 24 one-KB transfers per stage, six per wave (two A, four B).
// Why six stages: a K-tile is 24 MFMAs per wave = 384 cycles here (1,536 in the wide kernels), so with the wide kernels' three
// stages a transfer had two iterations = 0.3 us to land and every iteration waited for memory (first version: 12 us per
// forward launch of one tile per CU, 8 of them in the K-loop, where the MFMAs are worth 2.6); five iterations of slack cover
// an L2 / Infinity-Cache round trip.
constexpr int NT_BM = 64, NT_BN = 128, NT_NTH = 256, NT_NSTAGE = 6;
constexpr int NT_A_IMG = NT_BM * 128, NT_B_IMG = NT_BN * 128, NT_STAGE = NT_A_IMG + NT_B_IMG;

__device__ __forceinline__ void nt_mfma8(f32x4v (&acc)[2][4], const half8 (&a)[2], const half8 (&b)[4]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b[j], acc[i][j], 0, 0, 0);
}

// XZY: order of the three MFMA blocks of a K-tile -- hi x lo, hi x hi, lo x hi as in gemm_hp_pkd_kernel (true) or hi x lo,
// lo x hi, hi x hi as in gemm_hp_pkc_kernel / gemm_hp_kernel (false).  fp32 accumulation is order-sensitive in the last bit;
// with the order (and p.fold_bias) of the wide kernel that serves the same K, the rows this kernel takes come out bit for bit
// as that kernel would have produced them: splitting a launch, or re-sampling in other chunk sizes, never changes a value
// (tests/test_gpu_parity.py: chunk invariance).
#ifdef INR_STAMPS   // s_memrealtime (100 MHz, one counter for the whole chip): when does each wave of a small launch do what
#define NT_STAMP(slot)                                                                                  \
    do {                                                                                                \
        if (p.stamps && (threadIdx.x & 63) == 0) {                                                      \
            unsigned long long t_;                                                                      \
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");              \
            p.stamps[((long long)blockIdx.x * 8 + (threadIdx.x >> 6)) * 16 + (slot)] = t_;               \
        }                                                                                               \
    } while (0)
#else
#define NT_STAMP(slot)
#endif

template <int EPI, bool XZY>
__global__ void __launch_bounds__(NT_NTH, 1) INR_PACKED_F32 gemm_hp_nt_kernel(const HpParams p) {
    static_assert(EPI == HPE_SINE || EPI == HPE_SINE_STASH || EPI == HPE_MUL || EPI == HPE_Z, "K-contiguous epilogues only");
    __shared__ __attribute__((aligned(1024))) char smem[NT_NSTAGE * NT_STAGE];
    static_assert(4 * 32 * SUB16 * 4 + 16 <= NT_NSTAGE * NT_STAGE, "epilogue staging fits the operand ring");

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int g = lane >> 4, l16 = lane & 15;
    NT_STAMP(0);

    const int total = p.tiles_m * p.tiles_n;
    int logical = xcd_remap(blockIdx.x, total);
    const int tile_n = logical % p.tiles_n;
    const int tile_m = logical / p.tiles_n;
    const int m0 = tile_m * NT_BM, n0 = tile_n * NT_BN;
    const int ktiles = p.K / HP_BK;

    const __amdgpu_buffer_rsrc_t srdA = hp_srd(p.A + (long long)m0 * p.pitchA, (p.a_rows - m0) * p.pitchA);
    const __amdgpu_buffer_rsrc_t srdB = hp_srd(p.B + (long long)n0 * p.pitchB, (p.b_rows - n0) * p.pitchB);
    int vdma[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int q = wave + 4 * i;   // i < 2: A image (8 transfers), else B image (16)
        const int row = 8 * (i < 2 ? q : q - 8) + (lane >> 3);
        const int c = (lane & 7) ^ hp_f(row);
        vdma[i] = row * (int)(i < 2 ? p.pitchA : p.pitchB) + c * 16;
    }
    int soff = 0;
    auto dma_part = [&](int stage, int part) {   // part 0: the two A transfers, 1 / 2: two B transfers each; part 2 advances
        char* S = smem + stage * NT_STAGE;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if ((i >> 1) != part) continue;
            const int q = wave + 4 * i;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(i < 2 ? srdA : srdB, (__attribute__((address_space(3))) void*)(S + q * 1024),
                                                     16, vdma[i], soff, 0, 0);
        }
        if (part == 2) soff += 128;
    };
    auto dma = [&](int stage) {
        dma_part(stage, 0);
        dma_part(stage, 1);
        dma_part(stage, 2);
    };

    const int fx = (g ^ hp_f(l16)) << 4;
    const int fa_hi = (32 * wm + l16) * 128 + fx, fa_lo = fa_hi ^ 64;
    const int fb_hi = NT_A_IMG + (64 * wn + l16) * 128 + fx, fb_lo = fb_hi ^ 64;

    // (element-wise factor of the input-grad epilogue: fetched first thing, so that it is older than every transfer of the
    //  ring and has landed long before the epilogue -- a load issued there would sit a full memory latency in the open)
    const int ka = hp_scale_exp(p.sa), kb = hp_scale_exp(p.sb);
    const float inv_a = h3_pow2(-ka), inv_b = h3_pow2(-kb);
    const int er = lane >> 3, ec = (lane & 7) * 8;
    const int col_g = n0 + 64 * wn + ec;
    const bool col_ok = col_g < p.N;
    const long long rows_left = p.M - m0;
    const long long win = (rows_left < NT_BM ? rows_left : NT_BM) * (long long)p.N * 4;
    const long long first = (long long)m0 * p.N * 4;
    const int row = 32 * wm + er;
    const int voff32 = col_ok ? (row * p.N + col_g) * 4 : 0x7FFFFF00;
    const int voffhl = col_ok ? row * p.N * 4 + (col_g >> 5) * 128 + (col_g & 31) * 2 : 0x7FFFFF00;
    f32x4 mulreg[8];
    if (EPI == HPE_MUL) {
        const __amdgpu_buffer_rsrc_t srdMul = hp_srd((const char*)p.mul + first, win);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            mulreg[2 * q] = buf_load4(srdMul, voff32 + q * 8 * p.N * 4, 0);
            mulreg[2 * q + 1] = buf_load4(srdMul, voff32 + q * 8 * p.N * 4 + 16, 0);
        }
    }

    // bias through the accumulators (lane holds columns 16 j + lane % 16): bias * 2^(ka + kb), undone by the epilogue's 2^-(ka + kb)
    const bool fold = EPI != HPE_MUL && p.bias && p.fold_bias;
    float bias_s[4] = {0.f, 0.f, 0.f, 0.f};
    if (fold) {
        const float upa = h3_pow2(ka), upb = h3_pow2(kb);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + 64 * wn + 16 * j + l16;
            const float b = p.bias[col < p.N ? col : p.N - 1];
            bias_s[j] = col < p.N ? (b * upa) * upb : 0.f;
        }
    }
    f32x4v acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4v{bias_s[j], bias_s[j], bias_s[j], bias_s[j]};
    half8 ah[2][2], bh[2][4], al[2][2], bl[4];

    // prologue: up to six K-tiles in flight, wait for the first.  (Round 4, s_memrealtime stamps of a 4,096-row forward launch --
    // tools/nt_stamps.py, profiles/r04_small_n.txt: first K-tile visible after 3.0 us, K-loop 6.2 us = 0.39 us per K-tile where the
    // MFMAs take 0.16: the loop runs at the ~61 GB/s a CU receives with every CU asking, epilogue 2.1 us.  A RAMP -- request K-tiles
    // 0 and 1, start on tile 0, let the first iterations request two tiles each until the ring is six deep -- brought the first
    // tile forward to 2.2 us and made the loop 8.0 us: less in flight early means less delivered early, 10.3 us to the end of the
    // K-loop against 9.2.  Dropped.)
#pragma unroll
    for (int st = 0; st < NT_NSTAGE; ++st)
        if (st < ktiles) dma(st);
    {
        const int inflight = ktiles < NT_NSTAGE ? ktiles : NT_NSTAGE;
        switch (inflight) {   // all but the first tile's six transfers may stay in flight (immediates only)
            case 6: __builtin_amdgcn_s_waitcnt(hp_vmcnt(30)); break;
            case 5: __builtin_amdgcn_s_waitcnt(hp_vmcnt(24)); break;
            case 4: __builtin_amdgcn_s_waitcnt(hp_vmcnt(18)); break;
            case 3: __builtin_amdgcn_s_waitcnt(hp_vmcnt(12)); break;
            case 2: __builtin_amdgcn_s_waitcnt(hp_vmcnt(6)); break;
            default: __builtin_amdgcn_s_waitcnt(hp_vmcnt(0)); break;
        }
    }
    __builtin_amdgcn_s_barrier();
    NT_STAMP(1);
    if (ktiles > 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ah[0][i] = *reinterpret_cast<const half8*>(smem + fa_hi + i * 2048);
            al[0][i] = *reinterpret_cast<const half8*>(smem + fa_lo + i * 2048);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bl[j] = *reinterpret_cast<const half8*>(smem + fb_lo + j * 2048);
            bh[0][j] = *reinterpret_cast<const half8*>(smem + fb_hi + j * 2048);
        }
    }

    // One K-tile, as in gemm_hp_kernel: all fragments of tile t are in registers on entry; barrier (tile t+1 visible, stage
    // t % 6 dead); the transfers of tile t+6 spread over the three MFMA blocks, the fragments of tile t+1 read under Y and Z.
    // In flight behind tile t+1 at the wait: tiles t+2 .. t+5 (24 transfers per wave), fewer near the end of K.
    auto body = [&](auto par_c, auto st_c, int t) {
        constexpr int PAR = decltype(par_c)::value, ST = decltype(st_c)::value;
        const char* S1 = smem + ((ST + 1) % NT_NSTAGE) * NT_STAGE;
        const bool more6 = t + NT_NSTAGE < ktiles;
        {
            const int behind = ktiles - (t + 2);   // tiles issued after t+1
            // lgkmcnt(0) always: this wave's fragment reads of stage ST are done
            if (behind >= 4) __builtin_amdgcn_s_waitcnt(hp_vmcnt(24) & 0xF0FF);
            else if (behind == 3) __builtin_amdgcn_s_waitcnt(hp_vmcnt(18) & 0xF0FF);
            else if (behind == 2) __builtin_amdgcn_s_waitcnt(hp_vmcnt(12) & 0xF0FF);
            else if (behind == 1) __builtin_amdgcn_s_waitcnt(hp_vmcnt(6) & 0xF0FF);
            else __builtin_amdgcn_s_waitcnt(hp_vmcnt(0) & 0xF0FF);
        }
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // X: hi x lo
        if (more6) dma_part(ST, 0);
        nt_mfma8(acc, ah[PAR], bl);
        __builtin_amdgcn_sched_barrier(0);
        // second block: lo x hi (or hi x hi); bl is free, the other hi set of A is the landing place of tile t+1
        if (more6) dma_part(ST, 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) bl[j] = *reinterpret_cast<const half8*>(S1 + fb_lo + j * 2048);
#pragma unroll
        for (int i = 0; i < 2; ++i) ah[PAR ^ 1][i] = *reinterpret_cast<const half8*>(S1 + fa_hi + i * 2048);
        if (XZY) nt_mfma8(acc, ah[PAR], bh[PAR]);
        else nt_mfma8(acc, al[PAR], bh[PAR]);
        h3_sched<8, 0, 0, 6, 0, 0>();
        __builtin_amdgcn_sched_barrier(0);
        // third block: hi x hi (or lo x hi)
        if (more6) dma_part(ST, 2);
#pragma unroll
        for (int i = 0; i < 2; ++i) al[PAR ^ 1][i] = *reinterpret_cast<const half8*>(S1 + fa_lo + i * 2048);
#pragma unroll
        for (int j = 0; j < 4; ++j) bh[PAR ^ 1][j] = *reinterpret_cast<const half8*>(S1 + fb_hi + j * 2048);
        if (XZY) nt_mfma8(acc, al[PAR], bh[PAR]);
        else nt_mfma8(acc, ah[PAR], bh[PAR]);
        h3_sched<8, 0, 0, 6, 0, 0>();
        __builtin_amdgcn_sched_barrier(0);
    };
    {
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        using I2 = std::integral_constant<int, 2>;
        using I3 = std::integral_constant<int, 3>;
        using I4 = std::integral_constant<int, 4>;
        using I5 = std::integral_constant<int, 5>;
        int t = 0;
        for (; t + 6 <= ktiles; t += 6) {
            body(I0{}, I0{}, t);
            body(I1{}, I1{}, t + 1);
            body(I0{}, I2{}, t + 2);
            body(I1{}, I3{}, t + 3);
            body(I0{}, I4{}, t + 4);
            body(I1{}, I5{}, t + 5);
        }
        if (t < ktiles) {
            body(I0{}, I0{}, t);
            if (t + 1 < ktiles) {
                body(I1{}, I1{}, t + 1);
                if (t + 2 < ktiles) {
                    body(I0{}, I2{}, t + 2);
                    if (t + 3 < ktiles) {
                        body(I1{}, I3{}, t + 3);
                        if (t + 4 < ktiles) body(I0{}, I4{}, t + 4);
                    }
                }
            }
        }
    }

    NT_STAMP(2);
    // ---- epilogue: the wave's 32 x 64 through the (dead) operand ring, lane's pass q = row 8 q + lane / 8, 8 columns -------------
    const __amdgpu_buffer_rsrc_t srdHL = hp_srd(p.C_hl + first, EPI == HPE_Z ? 0 : win);
    const bool has_c2 = EPI == HPE_SINE_STASH || EPI == HPE_Z;
    const __amdgpu_buffer_rsrc_t srdC2 = hp_srd(has_c2 ? (const char*)p.C2 + first : p.C_hl, has_c2 ? win : 0);
    __syncthreads();   // operand stages are dead
    float* sub = reinterpret_cast<float*>(smem) + wave * (32 * SUB16);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) sub[(i * 16 + 4 * g + r) * SUB16 + j * 16 + l16] = acc[i][j][r] * inv_a * inv_b;
    const float* rd = sub + er * SUB16 + ec;

    if (EPI == HPE_SINE || EPI == HPE_SINE_STASH || EPI == HPE_Z) {
        const bool add_bias = p.bias && col_ok && !fold;   // (x + 0 is not x for x = -0: the folded form adds nothing at all)
        f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
        if (add_bias) {
            b0 = *reinterpret_cast<const f32x4*>(p.bias + col_g);
            b1 = *reinterpret_cast<const f32x4*>(p.bias + col_g + 4);
        }
        auto pre = [&](int q, int half) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(rd + q * 8 * SUB16 + 4 * half);
            return add_bias ? v + (half ? b1 : b0) : v;
        };
        if (EPI == HPE_Z) {   // z + b only (the head step forms sin / cos)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ro = q * 8 * p.N * 4;
                buf_store4(pre(q, 0), srdC2, voff32, ro);
                buf_store4(pre(q, 1), srdC2, voff32 + 16, ro);
            }
            NT_STAMP(3);
            return;
        }
        const float so_act = h3_pow2(hp_scale_exp(p.so));   // scale of the sine outputs' HL32 image
        float zmax = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 z0 = p.omega * pre(q, 0);
            const f32x4 z1 = p.omega * pre(q, 1);
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
        if (__builtin_expect(__any(!(zmax < INR_SINCOS_FAST_LIMIT)), 0)) {   // rare: redo the wave's tile through libm
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {
                float sv[8], cv[8];
#pragma unroll 1
                for (int e = 0; e < 8; ++e) {
                    const float v = rd[q * 8 * SUB16 + e];
                    sincos_f32(p.omega * (add_bias ? v + p.bias[col_g + e] : v), sv[e], cv[e]);
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
        NT_STAMP(3);
        return;
    }

    // HPE_MUL: dz_prev = (dz W) * dact_prev, column sums per 32-row wave block, max |dz_prev|, HL32 image over the bytes of `mul`
    const int ko = hp_scale_exp(p.so);
    const float so = h3_pow2(ko);
    f32x4 cs0 = {0.f, 0.f, 0.f, 0.f}, cs1 = cs0;
    float omax = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
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
    if (p.amax_out) {   // one (conditional) atomic per block
#pragma unroll   // wave_max(), open-coded: through the helper this translation unit's instruction schedule changes
        for (int off = 32; off > 0; off >>= 1) omax = fmaxf(omax, __shfl_xor(omax, off, 64));
        float* red = reinterpret_cast<float*>(smem + 4 * 32 * SUB16 * 4);   // behind the four staging areas
        if (lane == 0) red[wave] = omax;
        __syncthreads();
        if (tid == 0) hp_atomic_max_bits(p.amax_out, fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
    }
    if (p.colsum) {   // 4 rows per lane so far; the 8 lanes sharing a column group are lane ^ 8, ^ 16, ^ 32 (fixed order)
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
    NT_STAMP(3);
}
