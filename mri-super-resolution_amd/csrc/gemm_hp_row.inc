// Row-owning persistent KC kernel (round 5): one block owns 128 rows x ALL 512 columns of the output.
//
// Why it was built (profiles/r05_kloop_rowown_probe_shared_a.txt, tools/kloop_probe.hip V4 against V0, random operands, both AT the 1,400 W
// package cap): the K-loop of a 128 x 512 tile -- 8 waves (2 x 4) of 64 x 128, 128 accumulator registers per lane -- runs the same FLOPs
// in 0.631 ms where the 128 x 256 shape of gemm_hp_pkd_kernel takes 0.702: per MFMA a wave reads 25 % fewer fragment bytes out of LDS
// (24 KB per 96 MFMAs against 16 KB per 48) and the A panel crosses L2 -> LDS once instead of twice.  What it gives up is the second
// accumulator set (128 + 128 registers do not fit beside the fragments), so the epilogue runs IN LINE after a tile's last K-tile.
// MEASURED (profiles/r05_headline_ab.txt): for the ordinary epilogues that costs more than the K-loop gains -- 0.19 ms per launch of epilogue
// with the matrix pipe idle: forward 0.815 against 0.753 ms, input gradient 0.931 against 0.842, step 8.85 against 8.46 ms -- so for those
// (HPE_SINE / SINE_STASH / MUL / Z) the kernel stays selectable (inr_debug_set(27, 1)), tested bit-identical to the deferred-epilogue kernels,
// and is NOT the default.
// What row ownership is ADOPTED for is HPE_HEAD: the last sine layer of a fit step with the head step in its epilogue.  The block holds
// whole rows, so y_n = sum_k sin(omega z_nk) w_k + b is complete inside it: pass 1 takes the sine of every accumulator (leaving the
// argument's reduced fraction of a revolution in the register), sums a row's partials over the sixteen lanes and the four column waves,
// forms the residual and g = dL/dy; pass 2 is the chunk epilogue -- sin and cos of the kept fraction, dz_L = (g w)(omega cos) as HL32, its
// column sums (the layer's bias gradient), sum_n g_n sin (the head's weight gradient), the loss partials, max|dz|.  The z matrix is never
// written, the head step kernel never runs: 2.1 GB and 0.45 ms per step at 128^3 for a last layer that costs 0.25 ms more: -2.1 ... -2.7 %
// per step from 98,304 rows on (profiles/r05_head_fuse_sweep.txt), the default there (inr_debug_set(30, 0): off; key 31: threshold).
//
// LDS: a stage = A image 16 KB (128 rows x 128 B HL32 lines) + B image 64 KB (512 rows) = 80 KB; TWO stages fill the 160 KB.  K-tile t
// computes out of stage t & 1 while t + 1 lands in the other one; its fragments (one register set) are read behind the barrier that ends
// iteration t - 1.  The epilogue's per-wave staging (16 rows x 32 columns fp32, as in the other kernels) lives in the stage the tile's
// last K-tile just left (stage 1: K / 32 is even); the next tile's K-tile 0 lands in stage 0 meanwhile, its K-tile 1 is requested behind
// the barrier that ends the epilogue.
//
// Bits: every accumulator sees the sequence of gemm_hp_pkd_kernel -- bias fold as its start value, per K-tile hi x lo, hi x hi, lo x hi --
// and the epilogue arithmetic is that kernel's chunk code (16 rows x 32 columns through the staging area, the same un-scale, sin / cos,
// split, column-sum order within a wave's 64 rows): a row's value does not depend on which of the kernels took it.
constexpr int HR_BN = 512, HR_A_IMG = 16384, HR_B_IMG = 65536, HR_STAGE = HR_A_IMG + HR_B_IMG;

template <int EPI>
__global__ void __launch_bounds__(HP_NTH, 2) gemm_hp_row_kernel(const HpParams p) {
    __shared__ __attribute__((aligned(1024))) char smem[2 * HR_STAGE];
    static_assert(EPI == HPE_SINE || EPI == HPE_SINE_STASH || EPI == HPE_MUL || EPI == HPE_Z || EPI == HPE_HEAD, "KC epilogues only");

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int g = lane >> 4, l16 = lane & 15;
    const int total = p.tiles_m;          // (tiles_n == 1: the host checks N == 512)
    const int G = gridDim.x;
    const int KT = p.K >> 5;              // even (host: K % 64 == 0)

    auto tile_m0 = [&](int v) {
        const int logical = xcd_remap(v, total);
        return (p.reverse_m ? total - 1 - logical : logical) * HP_BM;
    };
    auto srd_a = [&](int m0) { return hp_srd(p.A + (long long)m0 * p.pitchA, (p.a_rows - m0) * p.pitchA); };
    int vp = blockIdx.x;
    int m0 = tile_m0(vp);
    bool has_next = vp + G < total;
    int m0n = has_next ? tile_m0(vp + G) : m0;
    __amdgpu_buffer_rsrc_t curA = srd_a(m0), nxtA = srd_a(m0n);
    const __amdgpu_buffer_rsrc_t srdB = hp_srd(p.B, p.b_rows * p.pitchB);

    // ---- LDS-DMA: a K-tile is 80 transfers of 1 KB (8 rows x 128 B); wave w issues q = w, w + 8, ..., w + 72 (q < 16: A rows 8 q ..,
    //      else B rows 8 (q - 16) ..): ten per wave
    const int drow = 8 * wave + (lane >> 3);
    const int dslot = ((lane & 7) ^ hp_f(drow)) * 16;
    const int vdmaA = drow * (int)p.pitchA + dslot, vdmaB = drow * (int)p.pitchB + dslot;
    const int pieceA = 64 * (int)p.pitchA, pieceB = 64 * (int)p.pitchB;
    auto dma_ktile = [&](int stage, const __amdgpu_buffer_rsrc_t& sa, int kt) {
        char* S = smem + stage * HR_STAGE;
        const int soff = kt * 128;
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            const int q = wave + 8 * i;
            if (i < 2)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(sa, (__attribute__((address_space(3))) void*)(S + q * 1024), 16, vdmaA,
                                                         soff + i * pieceA, 0, HP_A_AUX);
            else
                __builtin_amdgcn_raw_ptr_buffer_load_lds(srdB, (__attribute__((address_space(3))) void*)(S + q * 1024), 16, vdmaB,
                                                         soff + (i - 2) * pieceB, 0, 0);
        }
    };

    const int fx = (g ^ hp_f(l16)) << 4;
    const int fa_hi = (64 * wm + l16) * 128 + fx, fa_lo = fa_hi ^ 64;
    const int fb_hi = HR_A_IMG + (128 * wn + l16) * 128 + fx, fb_lo = fb_hi ^ 64;

    const int ka = hp_scale_exp(p.sa), kb = hp_scale_exp(p.sb);
    float bias_s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bias_s[j] = 0.f;
    if (EPI != HPE_MUL && p.bias) {
        const float upa = h3_pow2(ka), upb = h3_pow2(kb);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int col = 128 * wn + 16 * j + l16;
            const float b = p.bias[col < p.N ? col : p.N - 1];
            bias_s[j] = col < p.N ? (b * upa) * upb : 0.f;
        }
    }
    // HPE_HEAD: the head weights of this lane's eight accumulator columns (MFMA layout: column 128 wn + 16 j + l16), the head bias
    float hw_j[8];
    float head_b0 = 0.f;
    if constexpr (EPI == HPE_HEAD) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int col = 128 * wn + 16 * j + l16;
            hw_j[j] = col < p.N ? p.head_w[col] : 0.f;
        }
        head_b0 = p.head_b ? p.head_b[0] : 0.f;
    }
    f32x4v acc[4][8];
    auto init_acc = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = f32x4v{bias_s[j], bias_s[j], bias_s[j], bias_s[j]};
    };

    const int er = lane >> 2, ec = (lane & 3) * 8;
    float* const stg = reinterpret_cast<float*>(smem + HR_STAGE + wave * HP_EPI_WAVE);     // (stage 1: see the header)
    const float inv_a = h3_pow2(-ka), inv_b = h3_pow2(-kb);
    const float so = h3_pow2(hp_scale_exp(p.so));
    float omax_run = 0.f;

    // ---- the epilogue of the tile at row m0, in line: sixteen chunks of 16 rows x 32 columns per wave (column block jp outer, row
    //      block i inner -- the order of the deferred kernel, so that the column sums of a wave's 64 rows add up in the same order)
    // LDS of the HPE_HEAD epilogue (all inside stage 1, behind the eight 2 KB chunk areas): per-wave g of its 64 rows, the row partials of the
    // four column waves, the head weights in column order
    float* const g_lds = reinterpret_cast<float*>(smem + HR_STAGE + 8 * HP_EPI_WAVE + wave * 256);
    float* const rp_lds = reinterpret_cast<float*>(smem + HR_STAGE + 8 * HP_EPI_WAVE + 8 * 256);          // [4 (wn)][128 rows]
    float* const hw_lds = reinterpret_cast<float*>(smem + HR_STAGE + 8 * HP_EPI_WAVE + 8 * 256 + 4 * 128 * 4);   // [512]
    float t_row = 0.f, wt_row = 1.f;     // HPE_HEAD: target / loss weight of row m0 + 64 wm + lane, requested before the tile's K-loop
    auto head_prefetch = [&]() {
        if constexpr (EPI == HPE_HEAD) {
            const int row = m0 + 64 * wm + lane;
            const int rr = row < p.M ? row : p.M - 1;
            t_row = p.target[rr];
            wt_row = p.tweight ? p.tweight[rr] : 1.f;
        }
    };
    auto epilogue = [&]() {
        if constexpr (EPI == HPE_HEAD) {
            // ---- pass 1: y_n = sum_k sin(omega z_nk) w_k + b.  In the MFMA layout a lane holds rows 16 i + 4 g + r and columns 16 j + l16:
            //      eight columns per row and lane, the sixteen l16 lanes of a row by xor shuffles, the four column waves through LDS
            hw_lds[tid] = tid < p.N ? p.head_w[tid] : 0.f;
            float part[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int r = 0; r < 4; ++r) part[i][r] = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    // the argument's fraction of a revolution (the reduction of sincos_f32x2_fast, common.h) REPLACES the accumulator: pass 2
                    // takes v_sin / v_cos of it directly -- the same bits as reducing again, a third of the vector work less there
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float xr = p.omega * __builtin_amdgcn_ldexpf(acc[i][j][r], -(ka + kb));
                        const float kr = rintf(xr * INR_INV_2PI_HI);
                        float fr = fmaf(xr, INR_INV_2PI_HI, -kr);
                        fr = fmaf(xr, INR_INV_2PI_LO, fr);
                        acc[i][j][r] = fr;
                        part[i][r] = fmaf(__builtin_amdgcn_sinf(fr), hw_j[j], part[i][r]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = part[i][r];
                    v += __shfl_xor(v, 1, 64);
                    v += __shfl_xor(v, 2, 64);
                    v += __shfl_xor(v, 4, 64);
                    v += __shfl_xor(v, 8, 64);
                    if (l16 == 0) rp_lds[wn * 128 + 64 * wm + 16 * i + 4 * g + r] = v;
                }
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_s_barrier();
            // every wave forms g of its 64 rows (lane <-> row 64 wm + lane; the four waves of a row half compute the same values in the
            // same order); the wn == 0 wave of each half also owns the loss / sum-g partials of the half panel
            {
                const int lr = 64 * wm + lane;
                const float y = ((rp_lds[lr] + rp_lds[128 + lr]) + (rp_lds[256 + lr] + rp_lds[384 + lr])) + head_b0;
                const bool live = m0 + lr < p.M;
                const float res = live ? y - t_row : 0.f;
                const float wr = p.tweight ? wt_row * res : res;
                const float gv = 2.0f * wr * p.inv_count;
                g_lds[lane] = gv;
                if (wn == 0) {
                    float ls = wr * res, gs = gv;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) {
                        ls += __shfl_xor(ls, off, 64);
                        gs += __shfl_xor(gs, off, 64);
                    }
                    if (lane == 0) {
                        p.part_loss[(m0 / HP_BM) * 2 + wm] = ls;
                        p.part_g[(m0 / HP_BM) * 2 + wm] = gs;
                    }
                }
            }
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
        }
        const long long first = (long long)m0 * p.N * 4;
        const long long win = (long long)min(p.M - m0, HP_BM) * p.N * 4;
        const __amdgpu_buffer_rsrc_t srdHL = hp_srd(p.C_hl + first, win);
        const __amdgpu_buffer_rsrc_t srdC2 = hp_srd((const char*)p.C2 + first, p.C2 ? win : 0);
        const __amdgpu_buffer_rsrc_t srdMul = hp_srd((const char*)p.mul + first, p.mul ? win : 0);
        f32x4 mu[3][2];      // HPE_MUL: the element-wise factor of chunk c sits in slot c % 3, requested two chunks ahead
        auto load_mul = [&](auto cc) {
            constexpr int c = decltype(cc)::value, i = c & 3, jp = c >> 2;
            const int row = 64 * wm + 16 * i + er, col = 128 * wn + 32 * jp + ec;
            const int vo = col < p.N ? (row * p.N + col) * 4 : 0x7FFFFF00;
            mu[c % 3][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdMul, vo, 0, HP_MUL_AUX));
            mu[c % 3][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdMul, vo + 16, 0, HP_MUL_AUX));
        };
        if constexpr (EPI == HPE_MUL) {
            load_mul(std::integral_constant<int, 0>{});
            load_mul(std::integral_constant<int, 1>{});
        }
        f32x4 cs0 = {0.f, 0.f, 0.f, 0.f}, cs1 = cs0, cw0 = cs0, cw1 = cs0;
        hp_static_for<0, 4>([&](auto jc) {
            constexpr int jp = decltype(jc)::value;
            hp_static_for<0, 4>([&](auto ic) {
                constexpr int i = decltype(ic)::value, c = 4 * jp + i;
                if constexpr (EPI == HPE_MUL && c + 2 < 16) load_mul(std::integral_constant<int, c + 2>{});
                // park: accumulators -> the wave's staging area (un-scaled by one v_ldexp_f32, as the deferred kernel does)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        stg[(4 * g + r) * 32 + jj * 16 + l16] =
                            EPI == HPE_HEAD ? acc[i][2 * jp + jj][r]      // (already the reduced argument: pass 1)
                            : HP_UNSCALE_LDEXP ? __builtin_amdgcn_ldexpf(acc[i][2 * jp + jj][r], -(ka + kb)) : acc[i][2 * jp + jj][r] * inv_a * inv_b;
                __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the wave's own staging stores have reached the LDS
                __builtin_amdgcn_wave_barrier();
                const f32x4 cv0 = *reinterpret_cast<const f32x4*>(stg + er * 32 + ec);
                const f32x4 cv1 = *reinterpret_cast<const f32x4*>(stg + er * 32 + ec + 4);
                const int row = 64 * wm + 16 * i + er, col = 128 * wn + 32 * jp + ec;
                const bool ok = col < p.N;
                const int vhl = ok ? row * p.N * 4 + (col >> 5) * 128 + (col & 31) * 2 : 0x7FFFFF00;
                const int v32 = ok ? (row * p.N + col) * 4 : 0x7FFFFF00;
                if constexpr (EPI == HPE_MUL) {
                    const f32x4 o0 = hp_mul_sum(cv0, mu[c % 3][0], cs0), o1 = hp_mul_sum(cv1, mu[c % 3][1], cs1);
                    omax_run = fmaxf(omax_run, fmaxf(fmaxf(fmaxf(fabsf(o0[0]), fabsf(o0[1])), fmaxf(fabsf(o0[2]), fabsf(o0[3]))),
                                                     fmaxf(fmaxf(fabsf(o1[0]), fabsf(o1[1])), fmaxf(fabsf(o1[2]), fabsf(o1[3])))));
                    const float ov[8] = {o0[0], o0[1], o0[2], o0[3], o1[0], o1[1], o1[2], o1[3]};
                    u32x4 hi, lo;
                    hp_split8(ov, so, hi, lo);
                    __builtin_amdgcn_raw_buffer_store_b128(hi, srdHL, vhl, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(lo, srdHL, vhl + 64, 0, 0);
                    if constexpr (i == 3) {   // the column block's bias-gradient sums over the wave's 64 rows are complete
                        const long long cbytes = p.colsum ? 2ll * p.tiles_m * p.N * 4 : 0;
                        const __amdgpu_buffer_rsrc_t srdCS = hp_srd(p.colsum ? (const void*)p.colsum : (const void*)p.C_hl, cbytes);
                        const float tot = hp_colsum_fold(cs0, cs1, lane);
                        const int vcs = (lane < 32 && ok) ? (((m0 / HP_BM) * 2 + wm) * p.N + col + hp_colsum_index(lane)) * 4 : 0x7FFFFF00;
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, tot), srdCS, vcs, 0, 0);
                        cs0 = f32x4{0.f, 0.f, 0.f, 0.f};
                        cs1 = cs0;
                    }
                } else if constexpr (EPI == HPE_HEAD) {
                    // ---- pass 2: dz_L = (g w) (omega cos), its column sums, sum_n g_n sin(.)_nk; the arithmetic of hp_head_step_kernel
                    f32x2_t s2[4], c2[4];      // (cv0 / cv1 hold the reduced arguments)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const f32x2_t fr = e < 2 ? f32x2_t{cv0[2 * e], cv0[2 * e + 1]} : f32x2_t{cv1[2 * e - 4], cv1[2 * e - 3]};
                        s2[e] = f32x2_t{__builtin_amdgcn_sinf(fr[0]), __builtin_amdgcn_sinf(fr[1])};
                        c2[e] = f32x2_t{__builtin_amdgcn_cosf(fr[0]), __builtin_amdgcn_cosf(fr[1])};
                    }
                    const float gr = g_lds[16 * i + er];
                    const f32x4 w0 = *reinterpret_cast<const f32x4*>(hw_lds + (col < p.N ? col : 0));
                    const f32x4 w1 = *reinterpret_cast<const f32x4*>(hw_lds + (col < p.N ? col : 0) + 4);
                    float ov[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float we = e < 4 ? w0[e & 3] : w1[e & 3];
                        ov[e] = (gr * we) * (p.omega * c2[e >> 1][e & 1]);
                        omax_run = fmaxf(omax_run, fabsf(ov[e]));
                    }
                    hp_mul_sum(f32x4{ov[0], ov[1], ov[2], ov[3]}, f32x4{1.f, 1.f, 1.f, 1.f}, cs0);
                    hp_mul_sum(f32x4{ov[4], ov[5], ov[6], ov[7]}, f32x4{1.f, 1.f, 1.f, 1.f}, cs1);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        cw0[e] = fmaf(gr, s2[e >> 1][e & 1], cw0[e]);
                        cw1[e] = fmaf(gr, s2[2 + (e >> 1)][e & 1], cw1[e]);
                    }
                    u32x4 hi, lo;
                    hp_split8(ov, so, hi, lo);
                    __builtin_amdgcn_raw_buffer_store_b128(hi, srdHL, vhl, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(lo, srdHL, vhl + 64, 0, 0);
                    if constexpr (i == 3) {   // both column sums over the wave's 64 rows are complete: one slab row per half panel
                        const long long cbytes = 2ll * p.tiles_m * p.N * 4;
                        const __amdgpu_buffer_rsrc_t srdB = hp_srd(p.colsum, cbytes), srdW = hp_srd(p.slab_w, cbytes);
                        const float tb = hp_colsum_fold(cs0, cs1, lane), tw = hp_colsum_fold(cw0, cw1, lane);
                        const int vcs = (lane < 32 && ok) ? (((m0 / HP_BM) * 2 + wm) * p.N + col + hp_colsum_index(lane)) * 4 : 0x7FFFFF00;
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, tb), srdB, vcs, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, tw), srdW, vcs, 0, 0);
                        cs0 = f32x4{0.f, 0.f, 0.f, 0.f};
                        cs1 = cs0;
                        cw0 = cs0;
                        cw1 = cs0;
                    }
                } else if constexpr (EPI == HPE_Z) {
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
                    if constexpr (EPI == HPE_SINE_STASH) {
                        buf_store4(p.omega * f32x4{cvv[0], cvv[1], cvv[2], cvv[3]}, srdC2, v32, 0);
                        buf_store4(p.omega * f32x4{cvv[4], cvv[5], cvv[6], cvv[7]}, srdC2, v32 + 16, 0);
                    }
                }
                __builtin_amdgcn_s_waitcnt(0xC07F);   // the staging reads are done before the next chunk is parked over them
                __builtin_amdgcn_wave_barrier();
            });
        });
    };

    // ---- prologue: K-tiles 0 and 1 of the block's first tile in flight -------------------------------------------------------------
    if (p.stagger > 0) {
        for (int k = ((blockIdx.x >> 3) + blockIdx.x) & 7; k > 0; --k)
            for (int q = 0; q < p.stagger; q += 100) __builtin_amdgcn_s_sleep(100);
    }
    dma_ktile(0, curA, 0);
    dma_ktile(1, curA, 1);
    __builtin_amdgcn_s_waitcnt(hp_vmcnt(10));      // this wave's ten transfers of K-tile 0 have landed (K-tile 1 stays in flight)
    __builtin_amdgcn_s_barrier();

    half8 ah[4], al[4], bh[8], bl[8];
    while (true) {
        init_acc();
        head_prefetch();
        for (int t = 0; t < KT; ++t) {
            const char* S = smem + (t & 1) * HR_STAGE;
#pragma unroll
            for (int i = 0; i < 4; ++i) ah[i] = *reinterpret_cast<const half8*>(S + fa_hi + i * 2048);
#pragma unroll
            for (int j = 0; j < 8; ++j) bl[j] = *reinterpret_cast<const half8*>(S + fb_lo + j * 2048);
#pragma unroll
            for (int j = 0; j < 8; ++j) bh[j] = *reinterpret_cast<const half8*>(S + fb_hi + j * 2048);
#pragma unroll
            for (int i = 0; i < 4; ++i) al[i] = *reinterpret_cast<const half8*>(S + fa_lo + i * 2048);
            // X: hi x lo, Z: hi x hi, Y: lo x hi -- per accumulator the order of the deferred kernel
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
            // K-tile t + 1 (or the next tile's K-tile 0) has landed -- everything this wave requested, stores of the previous epilogue
            // included -- and every wave has read its fragments of stage t & 1: that stage takes K-tile t + 2
            __builtin_amdgcn_s_waitcnt(hp_vmcnt(0) & 0xF0FF);
            __builtin_amdgcn_s_barrier();
            if (t + 2 < KT) dma_ktile(t & 1, curA, t + 2);
            else if (t + 2 == KT && has_next) dma_ktile(0, nxtA, 0);
        }
        epilogue();
        if (!has_next) break;
        __builtin_amdgcn_s_barrier();               // every wave is done with its staging area: stage 1 takes the next tile's K-tile 1
        dma_ktile(1, nxtA, 1);
        m0 = m0n;
        curA = nxtA;
        vp += G;
        has_next = vp + G < total;
        if (has_next) {
            m0n = tile_m0(vp + G);
            nxtA = srd_a(m0n);
        }
    }
    if ((EPI == HPE_MUL || EPI == HPE_HEAD) && p.amax_out) {
        omax_run = wave_max(omax_run);
        if (lane == 0 && (EPI == HPE_MUL || omax_run > 0.f)) hp_atomic_max_bits(p.amax_out, omax_run);
    }
}
