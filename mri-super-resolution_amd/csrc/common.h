// Shared host/device helpers for libinrhip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "inrhip.h"

namespace inr {

// ---- error reporting (thread-local message, see inr_last_error) --------------------------------
void set_error(const char* fmt, ...);

#define INR_REQUIRE(cond, code, ...)             \
    do {                                         \
        if (!(cond)) {                           \
            ::inr::set_error(__VA_ARGS__);       \
            return (code);                       \
        }                                        \
    } while (0)

#define INR_HIP(expr)                                                                   \
    do {                                                                                \
        hipError_t e__ = (expr);                                                        \
        if (e__ != hipSuccess) {                                                        \
            ::inr::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),    \
                             __FILE__, __LINE__);                                       \
            return (int)e__;                                                            \
        }                                                                               \
    } while (0)

// after a kernel launch
#define INR_LAUNCH_CHECK()                                                              \
    do {                                                                                \
        hipError_t e__ = hipGetLastError();                                             \
        if (e__ != hipSuccess) {                                                        \
            ::inr::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e__),\
                             __FILE__, __LINE__);                                       \
            return (int)e__;                                                            \
        }                                                                               \
    } while (0)

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// the workspace of an fp64 image family (rescale, fourier, perceptual, register), which callers count in doubles: present, at
// least `need_bytes` long, 16-byte aligned
static inline int check_ws_doubles(const char* who, const double* workspace, int64_t workspace_doubles, size_t need_bytes) {
    INR_REQUIRE(workspace && workspace_doubles >= 0 && (size_t)workspace_doubles * sizeof(double) >= need_bytes, INR_E_WORKSPACE,
                "%s: workspace too small (%lld doubles, %zu needed)", who, workspace ? (long long)workspace_doubles : 0ll,
                need_bytes / sizeof(double));
    INR_REQUIRE(aligned16(workspace), INR_E_ALIGN, "%s: workspace must be 16-byte aligned", who);
    return 0;
}

// the dense grid `shape` [dim] of an entry point that walks it in chunks (jet.hip, wire_deriv.hip, wire.hip): every axis and the
// row count within 1 .. max_rows.  *total receives the row count
static inline int check_grid_shape(const char* who, const int64_t* shape, int dim, int64_t max_rows, int64_t* total) {
    *total = 1;
    for (int a = 0; a < dim; ++a) {
        INR_REQUIRE(shape[a] >= 1 && shape[a] <= max_rows, INR_E_INVALID, "%s: shape[%d] must be >= 1", who, a);
        *total *= shape[a];
        INR_REQUIRE(*total <= max_rows, INR_E_INVALID, "%s: the grid has too many rows", who);
    }
    return 0;
}

// How every unit hands out its caller-allocated workspace: ONE function `X_view(shape..., base)` per workspace takes the regions
// in order and returns typed pointers plus the total.  The planner is that function with a null base (`take` returns null and
// still advances); the entry point calls it once with the real base and checks `workspace_bytes >= total` before its first launch.
// A region occupies its size rounded up to `align` bytes, the view's granularity.
struct WsCarver {
    char* base;
    size_t align, at = 0;
    WsCarver(void* base_, size_t align_bytes) : base(static_cast<char*>(base_)), align(align_bytes) {}
    template <class T> T* take(size_t count) {
        T* r = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at += round_up(count * sizeof(T), align);
        return r;
    }
    size_t bytes() const { return at; }
};

// ---- per-kernel-class event profiler (bench.py roofline) ---------------------------------------
// gemm_f32.hip and gemm_hp.hip are compiled without packed fp32 VALU instructions (_build.py: SOURCE_FLAGS -- they slow the MFMA kernels' epilogues);
// kernels with no MFMA beside their VALU work switch them back on.  A no-op in translation units built with the default feature set.
#define INR_PACKED_F32 __attribute__((target("packed-fp32-ops")))

// inputs of the split-fp16 GEMM path (gemm_h3.inc); a null pointer / default-constructed value selects the fp32 MFMA
struct H3Args {
    const unsigned* a_amax = nullptr;   // float bits of max|A| (dz operands); null: A unscaled (activations, |A| <= 1)
    const unsigned* b_amax = nullptr;   // amax the pre-split B planes were scaled with
    const _Float16* Bh = nullptr;       // pre-split weight planes, k-contiguous for the GEMM at hand
    const _Float16* Bl = nullptr;
    unsigned* amax_out = nullptr;       // input-grad: receives max|dz_prev|
    int reverse_m = 0;                  // serpentine row-tile order between consecutive kernels (Infinity Cache reuse)
};

// power-of-two scale of an HL32 tensor (gemm_hp.inc) from an a-priori bound: bound = [*meas as float bits] * [*wn] * mul
// (missing factors = 1).  The producer scales by it, every consumer undoes it -- all by evaluating the same expression.
struct HpScale {
    const unsigned* meas = nullptr;   // float bits (an atomic-max slot of a FINISHED kernel), nullable
    const float* wn = nullptr;        // device float, nullable
    float mul = 0.f;                  // 0 = no scale at all
    int kmax = 126;                   // largest exponent of the scale (bounds with `wn`: gradients use the whole range; sine outputs
                                      // stop at 40 so that the folded bias b 2^(ka + kb) stays finite)
};

// The scale slots at the head of a network's split-GEMM region (api.hip: SplitCtx): one 32-bit word each, float bits where the
// getter says `unsigned*` (atomic-max targets and their readers), a float where it says `float*`.  Kernels receive these
// pointers, never an index: this map is the only place that knows the numbers.
struct HpSlots {
    static constexpr int MAX_LAYERS = 8;      // sine layers a region serves
    static constexpr size_t BYTES = 256;      // the slots' share of the region
    unsigned* base = nullptr;
    // rebuilt by every weight preparation (one per optimizer step / forward call)
    unsigned* w_max(int l) const { return base + l; }                                        // max|W_l|
    unsigned* dz_max(int l) const { return base + 8 + l; }                                   // measured max|dz_l|, zeroed there
    float* wnorm(int l) const { return reinterpret_cast<float*>(base + 16 + l); }            // max_j sum_k |W_l[k][j]|
    float* head_bound() const { return reinterpret_cast<float*>(base + 27); }                // a-priori bound of the head's dz
    float* act_bound(int l) const { return reinterpret_cast<float*>(base + 32 + l); }        // a-priori bound of layer l's output
    // measured once per call
    unsigned* x_max() const { return base + 24; }        // max|x| (floor 1)
    unsigned* target_max() const { return base + 25; }   // a fit: max|target| ...
    unsigned* gy_max() const { return base + 25; }       // ... inr_siren_backward_train: max|gy| (the same slot: a workspace serves one of the two)
    unsigned* weight_max() const { return base + 26; }   // max|weight|
};
static_assert(3 * HpSlots::MAX_LAYERS <= 24 && (32 + HpSlots::MAX_LAYERS) * sizeof(unsigned) <= HpSlots::BYTES,
              "the slot map must fit its region");

// one parameter-gradient GEMM of a step (hp_param_grad_multi: all of them in one launch)
struct HpParamGradJob {
    float* slabs;
    int splits;
    const char* dz_hl;
    const char* x_hl;
    int in_f, out_f;
    HpScale sa, sb;
};

// Process-global diagnostic switches behind inr_debug_set (atomics: a read races with nothing, but a switch flipped while
// another thread is enqueueing changes that thread's kernel selection -- diagnostic use only, see include/inrhip.h).
typedef std::atomic<int> tune_int;

// Which kernel family a host launcher picked: counted per process so that a test can assert that the family it means to
// cover is the one that ran (inr_launch_count).  Keep in step with INR_LF_* in include/inrhip.h.
enum LaunchFamily {
    LF_HP_PKD = 0,      // gemm_hp_pkd_kernel   persistent, deferred epilogue (HL32 operands)
    LF_HP_PKC = 1,      // gemm_hp_pkc_kernel   persistent, epilogue in line
    LF_HP_TILE = 2,     // gemm_hp_kernel<HP_KC> one block per tile
    LF_HP_RC = 3,       // gemm_hp_kernel<HP_RC> parameter gradient (row contraction)
    LF_H3 = 4,          // gemm_h3_kernel       split-fp16, operands split in the consumer
    LF_F32_PIPE16 = 5,  // gemm_f32_pipe16_kernel
    LF_F32_PIPE = 6,    // gemm_f32_pipe_kernel
    LF_F32_GENERIC = 7, // gemm_f32_kernel
    LF_SMALL_MULTI = 8, // siren_small_multi_kernel (persistent cooperative)
    LF_SMALL_STEP = 9,  // siren_small step kernel pair
    LF_HP_NARROW = 10,  // gemm_hp_nt_kernel    64 x 128 tiles (launches that cannot fill the chip with wide tiles)
    LF_HP_FUSED_FWD = 11,   // siren_fwd_fused_kernel: all sine layers + head of an inference forward in one launch
    LF_HP_ROW = 12,     // gemm_hp_row_kernel   persistent, one block owns 128 rows x all 512 columns, epilogue in line (round 5)
    LF_SMALL_BATCH = 13,    // siren_small_batch_kernel: several small-network fits in one persistent cooperative launch
    LF_COUNT = 14
};
// The one table behind inr_launch_count, inr_pia_launch_count and inr_jet_launch_count (api.hip).  The SIREN and ERD families sit
// at their public ids; the PIA and jet families, whose public ids start at 0, at internal bases above them that no entry point
// hands out.
enum {
    LF_PIA_BASE = INR_LF_ERD_END,                     // + INR_PIA_LF_*
    LF_JET_BASE = LF_PIA_BASE + INR_PIA_LF_COUNT,     // + INR_JET_LF_*
    LF_TABLE = LF_JET_BASE + INR_JET_LF_COUNT
};
static_assert(LF_COUNT <= INR_LF_ERD_BASE, "the SIREN families must end below the ERD ids");
void count_launch(int family);   // family: an index of that table
#define INR_E_FALLBACK (-100)   // internal: the chosen kernel cannot run on this device, the caller takes its next-best path

// The constants of Adam step number `step` (1-based) as the kernels take them (adam_update below): host-side double bias
// corrections, as torch's _single_tensor_adam does for python-float lr, rounded to fp32 once.
struct AdamConsts {
    float one_minus_b1, b2, one_minus_b2, step_size, bc2_sqrt, eps;
};
static inline AdamConsts adam_consts(long long step, double lr, double b1, double b2, double eps) {
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    return AdamConsts{(float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)(lr / bc1), (float)sqrt(bc2), (float)eps};
}

// ---- deferred gradient reduction of the fused fit (kernels.hip: finalize_kernel) -------------------------------------------
// Every gradient tensor of a step is a fixed-order sum of slab rows its producer left behind (row-split parameter-gradient
// GEMMs, per-tile column sums of the input-gradient epilogues, per-block sums of the head step).  Round 2 reduced each tensor
// right behind its producer -- 9 to 14 launches of ~5 us -- and ran Adam as one more; here the producers only write, and ONE
// launch at the end of the step sums every tensor, finishes the loss and takes the Adam step (two launches when a slab stack is
// tall enough to want a first stage).  No float atomics anywhere: runs stay bitwise reproducible.
constexpr int FIN_MAX_SEG = 20;
constexpr int FIN_GROUP = 32;         // rows per first-stage group
constexpr int FIN_TALL = 4 * FIN_GROUP;   // stacks above this many rows get a first stage
struct FinalizeSeg {
    const float* slab;     // [nslabs][len]
    float* stage1;         // [ceil(nslabs / FIN_GROUP)][len] when nslabs > FIN_TALL, else unused
    long long dst;         // offset of the tensor in the flat parameter / gradient buffers
    long long len;
    int nslabs;
};
struct FinalizeJob {
    FinalizeSeg seg[FIN_MAX_SEG];
    long long first[FIN_MAX_SEG + 1];   // prefix sums of len
    long long s1_first[FIN_MAX_SEG + 1];   // prefix sums of the first-stage blocks per segment (0 for stacks that need none)
    int nseg;
    const float* part_loss;             // [nparts] per-block loss terms (nullable)
    int nparts;
    float loss_scale;
    float* loss_out;
    float* grads;
    float *params, *m, *v;              // params == nullptr: reduce only (inr_siren_loss_grad)
    AdamConsts adam;                    // set by launch_finalize
};
int launch_finalize(FinalizeJob& job, long long adam_step, double lr, double b1, double b2, double eps, hipStream_t st);

enum KernelClass { KC_GEMM_FWD = 0, KC_GEMM_DX = 1, KC_GEMM_DW = 2, KC_OTHER = 3, KC_COUNT = 4 };
bool prof_enabled();
void prof_begin(int kernel_class, hipStream_t s);
void prof_end(int kernel_class, hipStream_t s);

struct ProfScope {
    int kc;
    hipStream_t s;
    bool on;
    ProfScope(int kc_, hipStream_t s_) : kc(kc_), s(s_), on(prof_enabled()) {
        if (on) prof_begin(kc, s);
    }
    ~ProfScope() {
        if (on) prof_end(kc, s);
    }
};

// ---- device math ---------------------------------------------------------------------------------
// sin and cos of one fp32 argument.  On gfx950 the f32 MFMA and the f32 VALU share the same lanes (measured:
// a wave's VALU epilogue does not overlap the co-resident wave's v_mfma_f32_32x32x2_f32 stream), so every VALU
// instruction in a GEMM epilogue costs matrix time.  The argument is therefore reduced to a FRACTION OF A
// REVOLUTION with two FMAs -- f = x/(2*pi) - rint(x/(2*pi)), |f| <= 0.5, single rounding of the exact
// difference plus the 1/(2*pi) tail -- and handed to the transcendental unit (v_sin_f32 / v_cos_f32 take
// revolutions).  6 instructions per element instead of ~24; measured abs error <= 3e-7 for |x| < 2^20
// (hardware sin/cos: 1.4e-7 on [-0.5, 0.5] rev; argument: <= 3e-8 rev).  Larger arguments take the libm path.
#define INR_INV_2PI_HI 1.59154936671257019e-01f
#define INR_INV_2PI_LO 6.42063824329852650e-09f
#define INR_SINCOS_FAST_LIMIT 1048576.0f

typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x2_t sincos_f32_libm(float x) {   // {sin, cos}: the path of arguments beyond the fast limit
    float s, c;
    sincosf(x, &s, &c);
    return f32x2_t{s, c};
}
__device__ __forceinline__ void sincos_f32_fast(float x, float& s, float& c) {   // |x| < INR_SINCOS_FAST_LIMIT
    const float k = rintf(x * INR_INV_2PI_HI);
    float f = fmaf(x, INR_INV_2PI_HI, -k);
    f = fmaf(x, INR_INV_2PI_LO, f);
    s = __builtin_amdgcn_sinf(f);
    c = __builtin_amdgcn_cosf(f);
}
__device__ __forceinline__ void sincos_f32(float x, float& s, float& c) {
    if (__builtin_expect(!(fabsf(x) < INR_SINCOS_FAST_LIMIT), 0)) {
        const f32x2_t r = sincos_f32_libm(x);
        s = r[0];
        c = r[1];
        return;
    }
    sincos_f32_fast(x, s, c);
}
// The same with the libm branch out of line, for kernels with an unrolled MFMA epilogue: inlined there (64 times in the 128-wide
// ERD kernel) it competes with the accumulators for registers and pushed them into scratch memory.
static __device__ __noinline__ f32x2_t sincos_f32_libm_ool(float x) { return sincos_f32_libm(x); }
__device__ __forceinline__ void sincos_f32_ool(float x, float& s, float& c) {
    if (__builtin_expect(!(fabsf(x) < INR_SINCOS_FAST_LIMIT), 0)) {
        const f32x2_t r = sincos_f32_libm_ool(x);
        s = r[0];
        c = r[1];
        return;
    }
    sincos_f32_fast(x, s, c);
}

// Branch-free core of sincos_f32 on float2 (valid for |x| < INR_SINCOS_FAST_LIMIT; callers check that once per
// tile and redo the tile through sincos_f32 otherwise, so the unrolled epilogue carries no libm code).
__device__ __forceinline__ void sincos_f32x2_fast(f32x2_t x, f32x2_t& s, f32x2_t& c) {
    const f32x2_t t = x * INR_INV_2PI_HI;
    const f32x2_t k = f32x2_t{rintf(t[0]), rintf(t[1])};
    f32x2_t f = __builtin_elementwise_fma(x, (f32x2_t)(INR_INV_2PI_HI), -k);
    f = __builtin_elementwise_fma(x, (f32x2_t)(INR_INV_2PI_LO), f);
    s = f32x2_t{__builtin_amdgcn_sinf(f[0]), __builtin_amdgcn_sinf(f[1])};
    c = f32x2_t{__builtin_amdgcn_cosf(f[0]), __builtin_amdgcn_cosf(f[1])};
}

// bit-exact torch.linspace(-1, 1, n)[i] in fp32 (oracle/inr_oracle.py: linspace_pm1)
__device__ __forceinline__ float linspace_pm1(int64_t i, int64_t n) {
    if (n <= 1) return -1.0f;
    const float step = 2.0f / static_cast<float>(n - 1);
    return (i < n / 2) ? fmaf(step, static_cast<float>(i), -1.0f)
                       : fmaf(-step, static_cast<float>(n - 1 - i), 1.0f);
}

// the coordinates of one row of the derivative kernels (jet.hip, wire_deriv.hip; d <= JET_MAX_D axes): the inr_mgrid rule (last axis
// fastest, bit-exact linspace) or the caller's matrix x [.][d]
constexpr int JET_MAX_D = 4;
struct JetGrid {
    long long n[JET_MAX_D];
};
template <bool FROM_GRID>
__device__ __forceinline__ void jet_coords(float* c, const float* __restrict__ x, const JetGrid& g, int d, long long row) {
    if (FROM_GRID) {
        long long rem = row;
#pragma unroll
        for (int a = JET_MAX_D - 1; a >= 0; --a) {
            c[a] = 0.f;
            if (a < d) {
                const long long idx = rem % g.n[a];
                rem /= g.n[a];
                c[a] = linspace_pm1(idx, g.n[a]);
            }
        }
    } else {
#pragma unroll
        for (int a = 0; a < JET_MAX_D; ++a) c[a] = (a < d) ? x[row * d + a] : 0.f;
    }
}

// scipy's 'mirror' boundary (skimage 'reflect'): reflection about the edge samples, period 2n - 2, any number of periods away
__device__ __forceinline__ int mirror_index(int i, int n) {
    if (n <= 1) return 0;
    const int period = 2 * n - 2;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}

// row of accumulator register r (0..15) of a 32 x 32 MFMA tile held by lane half hh = lane >> 5; the column is lane & 31
__device__ __forceinline__ int mfma32_acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// sum / maximum over the 64 lanes of a wave, every lane receives it: xor butterfly, offsets 32 -> 1 (a fixed order -- callers'
// bits depend on it)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = __builtin_elementwise_max(v, (T)__shfl_xor(v, off, 64));
    return v;
}

// sum over a block of 256 threads, every thread receives it: per wave, then the four waves in a fixed order (red: 4 doubles of LDS)
__device__ __forceinline__ double block_sum_f64(double v, double* red /*[4]*/) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return s;
}

// One Adam step of one element in torch's single-tensor formulation: m.lerp_(g, 1 - b1), v = v b2 + (1 - b2) g g,
// p -= step_size * m / (sqrt(v) / bc2_sqrt + eps).  p, m, v: old values in, new out.
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float gi, const AdamConsts& c) {
    const float mi = fmaf(gi - m, c.one_minus_b1, m);
    const float vi = fmaf(c.one_minus_b2 * gi, gi, v * c.b2);
    const float denom = __fsqrt_rn(vi) / c.bc2_sqrt + c.eps;
    m = mi;
    v = vi;
    p = p - c.step_size * (mi / denom);
}

}  // namespace inr
