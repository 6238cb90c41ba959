// The split-fp16 number format and its three-product MFMA step -- the one definition behind gemm_h3.inc, the gemm_hp*.inc family
// and the RAMS convolutions (rams_h3.inc, rams_wgrad_h3.inc).
//
// Every fp32 operand element a is represented as hi + lo with hi = fp16(a * s), lo = fp16(a * s - hi), both rounded to nearest,
// for a power-of-two tensor scale s that places max|a| * s in [2^14, 2^15); a product a * b then costs three fp16 MFMAs (hi*lo,
// lo*hi, hi*hi; the lo*lo term, 2^-22 relative, is dropped) with fp32 accumulation.  gemm_h3.inc has the error analysis.
#pragma once
#include "common.h"

namespace inr {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4v __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

constexpr int SUB16 = 68;   // row stride (floats) of a wave's 64-column epilogue stage: the four lane groups hit four bank quarters

// bijective XCD-aware remap: physical block id -> logical id such that logical ids that are close
// together run on the same XCD (blocks are dealt round-robin over the 8 XCDs).
__device__ __forceinline__ int xcd_remap(int pid, int total) {
    const int q = total >> 3, r = total & 7;
    const int xcd = pid & 7, idx = pid >> 3;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t srd, int voff, int soff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(srd, voff, soff, 0);
    return __builtin_bit_cast(f32x4, v);
}
// NOTE: the row offset is folded into the VGPR offset and soffset stays the constant 0.  With an SGPR soffset
// a 16-byte buffer store reads its data registers late, and on gfx950/ROCm 7.2 hipcc let the next VALU
// instruction overwrite them (observed: lanes 12-15 of every 16 stored the FOLLOWING store's second dword).
__device__ __forceinline__ void buf_store4(f32x4 v, __amdgpu_buffer_rsrc_t srd, int voff, int row_off) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), srd, voff + row_off, 0, 0);
}

// exponent k of the power-of-two scale that brings a tensor with max |.| = amax (float bits) to [2^14, 2^15), clamped to
// [kmin, kmax]; 0 (scale 1) for empty / zero / non-finite tensors.  Tensors measured exactly take |k| <= 100.
__device__ __forceinline__ int h3_scale_exp(unsigned amax_bits, int kmax, int kmin) {
    const int e = (int)((amax_bits >> 23) & 0xff);
    if (e == 0 || e == 255) return 0;
    const int k = 14 - (e - 127);
    return k > kmax ? kmax : (k < kmin ? kmin : k);
}
__device__ __forceinline__ int h3_scale_exp(unsigned amax_bits) {
    // = h3_scale_exp(amax_bits, 100, -100), open-coded: through the call gemm_h3_kernel and the RAMS convolutions allocate other registers
    const int e = (int)((amax_bits >> 23) & 0xff);
    if (e == 0 || e == 255) return 0;
    int k = 14 - (e - 127);
    return k > 100 ? 100 : (k < -100 ? -100 : k);
}
__device__ __forceinline__ float h3_pow2(int k) { return __uint_as_float((unsigned)(127 + k) << 23); }

// hi = fp16(x s) and lo = fp16(x s - hi), both rounded TO NEAREST (v_cvt_pk_f16_f32: gfx950 has the packed form, same issue
// cost as v_cvt_pkrtz_f16_f32).  Rounds 1 and 2 truncated (cvt_pkrtz): |x s - hi| < ulp(hi), so lo spent a bit on magnitude
// and hi + lo carried 22 bits with a one-sided error; to nearest the remainder is at most half an ulp of hi, lo keeps 11 bits of
// it and hi + lo = x s to 2^-24 -- fp32's own rounding.  Measured on the late-training state of the config-1 fit (the gradient
// there is a small difference of large terms): the distance from the float64 gradient fell 4x (tools/hp_err_diag.py).  max|x s|
// < 2^15, so rounding up cannot leave fp16's range.
typedef float h3_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ half2v h3_cvt_rn(float a0, float a1) { return __builtin_convertvector(h3_f32x2{a0, a1}, half2v); }

// (Measured and not kept, round 4: v_fma_mixlo_f16 / v_fma_mixhi_f16 by inline asm -- four instructions per pair instead of the six
//  the compiler emits below, the same bits (signature of a 12-step fit identical) -- bought nothing: 8.476 / 8.485 against 8.471 / 8.474
//  ms per step.  The half-register writes are read-modify-write chains with a hazard nop each.)
template <bool SCALED = true>
__device__ __forceinline__ void h3_split2(float v0, float v1, float s, half2v& hi, half2v& lo) {
    if (SCALED) {
        hi = h3_cvt_rn(v0 * s, v1 * s);
        const float r0 = __builtin_fmaf(v0, s, -(float)hi[0]), r1 = __builtin_fmaf(v1, s, -(float)hi[1]);
        lo = h3_cvt_rn(r0, r1);
    } else {   // |v| <= 1 (sine outputs): no scale, one VALU less per element
        hi = h3_cvt_rn(v0, v1);
        const float r0 = v0 - (float)hi[0], r1 = v1 - (float)hi[1];
        lo = h3_cvt_rn(r0, r1);
    }
}

template <int NM, int NV, int NW, int NR, int NG, int I>
__device__ __forceinline__ void h3_sched() {   // NM MFMAs with NV VALU, NW DS writes, NR DS reads, NG VMEM reads spread between
    if constexpr (I < NM) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        constexpr int v = (I + 1) * NV / NM - I * NV / NM;
        if constexpr (v > 0) __builtin_amdgcn_sched_group_barrier(0x002, v, 0);
        constexpr int w = (I + 1) * NW / NM - I * NW / NM;
        if constexpr (w > 0) __builtin_amdgcn_sched_group_barrier(0x200, w, 0);
        constexpr int r = (I + 1) * NR / NM - I * NR / NM;
        if constexpr (r > 0) __builtin_amdgcn_sched_group_barrier(0x100, r, 0);
        constexpr int g = (I + 1) * NG / NM - I * NG / NM;
        if constexpr (g > 0) __builtin_amdgcn_sched_group_barrier(0x020, g, 0);
        h3_sched<NM, NV, NW, NR, NG, I + 1>();
    }
}

// one of the three products of a K-tile on a wave's 64 x 64 sub-tile: 16 v_mfma_f32_16x16x32_f16
__device__ __forceinline__ void h3_mfma16(f32x4v (&acc)[4][4], const half8 (&a)[4], const half8 (&b)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b[j], acc[i][j], 0, 0, 0);
}

}  // namespace inr
