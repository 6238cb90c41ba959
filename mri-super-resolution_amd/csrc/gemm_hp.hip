// The pre-split fp16 ("HL32", hp_*) GEMM family: every operand already split into hi/lo fp16 halves in HBM (format: split_fp16.h and
// the head of gemm_hp.inc).  This unit holds the family's kernels --
//   gemm_hp.inc      one block per tile, the persistent in-line (pkc) and deferred-epilogue (pkd) kernels, the parameter gradient,
//                    weight preparation, conversions, the head kernels
//   gemm_hp_nt.inc   64 x 128 tiles for launches that cannot fill the chip with wide ones
//   gemm_hp_row.inc  the row-owning 128 x 512 kernel (with the fused head epilogue)
//   gemm_hp_fwd.inc  all layers of an inference forward in one launch
// -- and their host side, hp_kc_choice first: the ONE rule that picks the kernel of a forward or input-gradient launch.
// Compiled without packed fp32 VALU instructions, like gemm_f32.hip (_build.py: SOURCE_FLAGS).
#include "internal.h"
#include "split_fp16.h"

namespace inr {

#include "gemm_hp.inc"
#include "gemm_hp_nt.inc"
#include "gemm_hp_row.inc"
#include "gemm_hp_fwd.inc"

int hp_build_flags() {   // the diagnostic macros of this unit (bit meanings: inr_build_flags)
    int f = 0;
    if (HP_ABLATE != 0) f |= 2;
    if (HP_A_AUX != 2 || HP_MUL_AUX != 0 || HP_RC_A_AUX != 0 || HP_RC_B_AUX != 0 || HP_HEAD_NT != 0 || HP_UNSCALE_LDEXP != 1 || HP_HEAD_PREFETCH != 1 || HP_COLSUM_TRANSPOSED != 1 || HP_DIAG_NO_OMEGA_STASH != 0) f |= 8;     // cache-policy experiments (gemm_hp.inc)
    return f;
}
tune_int g_stamp_class{-1}, g_stamp_nth{0}; // which launch of this family receives g_stamps (class, countdown)
static unsigned long long* hp_stamp_target(int kernel_class) {
    if (!g_stamps || kernel_class != g_stamp_class) return nullptr;
    return g_stamp_nth-- == 0 ? g_stamps : nullptr;
}

tune_int g_hp_stagger{0};  // inr_debug_set(11, n): start phases of the persistent blocks, n * 64 cycles apart (0 = together)
tune_int g_hp_persistent{2}; // inr_debug_set(10, v): 2 persistent walk with the epilogue of tile T under the K-loop of tile T+1
                           // (K = 256 / 512), 1 persistent walk with the epilogue in line, 0 one block per tile
static int hp_num_cus() {
    static int n = 0;
    if (!n) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
        if (n <= 0) n = 256;
    }
    return n;
}
// inr_debug_set(32, v): test-only cap on the grid of the persistent kernels (0 = none, the default), so that small launches walk
// several tiles per block.  Every persistent kernel strides its tiles by gridDim.x and xcd_remap maps [0, tiles) onto itself for any
// grid, so a cap changes which block computes a tile, never what it computes.  (Not applied in hp_row_plan: the family choice
// stays that of the chip.)
tune_int g_hp_grid_cap{0};
static unsigned hp_persistent_grid(long long tiles) {
    long long g = tiles < hp_num_cus() ? tiles : hp_num_cus();
    const int cap = g_hp_grid_cap;
    if (cap > 0 && g > cap) g = cap;
    return (unsigned)g;
}
bool hp_head_ok(int hidden) { return hidden == 128 || hidden == 256 || hidden == 512 || hidden == 1024; }

// per-step weight preparation (gemm_hp.inc): slots.w_max(l) = max|W_l|, slots.dz_max(l) = 0, slots.wnorm(l) = wnorm_l; `part`
// = 8 x HP_PREP_MAXB x 2 words of scratch; head_bound nullable (forward-only callers)
size_t hp_prep_part_bytes() { return (size_t)8 * HP_PREP_MAXB * 2 * sizeof(unsigned); }
int hp_weight_prep(const float* const* W, const int* out_f, const int* in_f, int layers, char* planes, HpSlots slots,
                   unsigned* part, float* head_bound, const float* head_W, const float* head_b, int hidden, const unsigned* tmax,
                   const unsigned* wtmax, float inv_count, float omega, hipStream_t stream, const float* const* bias,
                   const float* layer_omega, float* act_bound, const unsigned* x_amax) {
    INR_REQUIRE(layers >= 1 && layers <= HpSlots::MAX_LAYERS, INR_E_INVALID, "hp_weight_prep: %d layers", layers);
    HpWeightJobs jobs{};
    char* cur = planes;
    int max_tiles = 1, max_sb = 1;
    for (int l = 0; l < layers; ++l) {
        const long long n = (long long)out_f[l] * in_f[l];
        jobs.job[l] = HpWeightJob{W[l], cur, cur + 4 * n, slots.w_max(l), reinterpret_cast<unsigned*>(slots.wnorm(l)), out_f[l], in_f[l], bias ? bias[l] : nullptr,
                                  layer_omega ? layer_omega[l] : 0.f};
        cur += 8 * n;
        const int t = ((out_f[l] + 63) / 64) * ((in_f[l] + 63) / 64);
        if (t > max_tiles) max_tiles = t;
        const int sb = (in_f[l] >> 4) < HP_PREP_MAXB ? (in_f[l] >> 4) : HP_PREP_MAXB;
        if (sb > max_sb) max_sb = sb;
    }
    jobs.layers = layers;
    jobs.part = part;
    jobs.dz_slots = slots.dz_max(0);
    jobs.head_bound = head_bound;
    jobs.head_W = head_W; jobs.head_b = head_b; jobs.hidden = hidden;
    jobs.tmax = tmax; jobs.wtmax = wtmax; jobs.inv_count = inv_count; jobs.omega = omega;
    jobs.act_bound = act_bound; jobs.x_amax = x_amax;
    ProfScope ps(KC_OTHER, stream);
    hipLaunchKernelGGL(hp_weight_stats_kernel, dim3(max_sb, layers), dim3(256), 0, stream, jobs);
    INR_LAUNCH_CHECK();
    hipLaunchKernelGGL(hp_weight_split_kernel, dim3(max_tiles, layers + 1), dim3(256), 0, stream, jobs);
    INR_LAUNCH_CHECK();
    return 0;
}

int hp_convert(char* out, const float* x, long long rows, int cols, HpScale sc, hipStream_t stream) {
    if (rows <= 0) return 0;
    const long long n8 = rows * (cols / 8);
    long long blocks = (n8 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    ProfScope ps(KC_OTHER, stream);
    hipLaunchKernelGGL(hp_convert_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, out, x, rows, cols, sc);
    INR_LAUNCH_CHECK();
    return 0;
}

static int hp_check_grid(const HpParams& p) {
    const long long total = (long long)p.tiles_m * p.tiles_n * p.splits;
    INR_REQUIRE(total > 0 && total < (1ll << 31), INR_E_INVALID, "hp gemm grid out of range (%lld blocks)", total);
    return 0;
}

// ---- the K-contiguous launches (forward, input gradient): one kernel-choice rule, one launcher ---------------------------------------
// may the last sine layer of a fit step stash z only (HPE_Z)?  (deferred-epilogue kernel shapes; debug key 16)
tune_int g_hp_zhead{1};
tune_int g_hp_fused_fwd{0};   // inr_debug_set(19, 1): inference forwards of eligible networks run all layers in one launch (gemm_hp_fwd.inc:
                              // measured SLOWER than the layer-wise launches at hidden = 512 -- 117 against 144 M voxels/s -- so off by default)
tune_int g_hp_narrow_max_tiles{192};   // inr_debug_set(29, v): most wide tiles (per 256 CUs) of a launch that still goes to the narrow kernel
tune_int g_hp_narrow{1};    // inr_debug_set(18, v): 1 = launches with fewer 128-row tiles than two per CU take 64-row tiles (default), 0 = never
// The row-owning kernel (gemm_hp_row.inc): K-contiguous launches of 512 output columns whose 128-row panels number at least
// g_hp_row_min_tiles.  OFF by default (inr_debug_set(27, 1) selects it, key 28 moves the threshold; bit-identical results either way):
// its K-loop is 10 % cheaper than the 128 x 256 shape's (tools/kloop_probe.hip V4 / V0: 0.631 against 0.702 ms at the package cap) but
// it has no registers for a second accumulator set, and the epilogue it therefore runs in line costs 0.19 ms per launch with the
// matrix pipe idle: forward 0.815 against 0.753 ms, input gradient 0.931 against 0.842, step 8.85 against 8.46 ms at 128^3
// (profiles/r05_headline_ab.txt).
tune_int g_hp_row{0};
tune_int g_hp_row_min_tiles{1024};

// Does the deferred-epilogue kernel (gemm_hp_pkd_kernel) serve this K?  Forward K = 256 / 512, input gradient K = 512: its HPE_MUL form
// would spill at K = 256, the in-line epilogue serves that.
static bool hp_deferred_ok(int k, bool forward) { return g_hp_persistent == 2 && (k == 512 || (forward && k == 256)); }
bool hp_z_stash_ok(int in_f) { return g_hp_zhead && hp_deferred_ok(in_f, true); }

// Does a K-contiguous launch go to the 64 x 128 tiles of gemm_hp_nt_kernel?  All of it does when its wide tiles would keep at
// most three quarters of the CUs busy (four narrow tiles per wide one, each a little more than a quarter of its time:
// gemm_hp_nt.inc), otherwise all of it stays wide.
// (Handing the remainder rows of a LARGE launch to the narrow tiles was measured and dropped: these kernels move their bytes at
//  ~3.6 TB/s whatever the tile count, so the round the remainder adds to a few CUs costs ~9 us at 69,632 rows, less than a
//  second launch: 1.39 against 1.34 ms per step.)
static bool hp_row_plan(int64_t n, int width) {
    if (!g_hp_narrow || !g_hp_persistent) return false;
    const long long tiles = (long long)((n + HP_BM - 1) / HP_BM) * ((width + HP_BN - 1) / HP_BN);
    return 256 * tiles <= (long long)g_hp_narrow_max_tiles * hp_num_cus();   // (default 192 per 256 CUs: three quarters of the chip)
}

// The kernel of C[rows][width] = A[rows][K] B[width][K]^T.  The wide family follows from K alone: deferred epilogue where that
// kernel serves K, else the in-line epilogue from three K-tiles on, else one block per tile (debug key 10 takes the persistent
// forms away).  The row-owning kernel (key 27) replaces the deferred one, whose MFMA block order it reproduces bit for bit, and
// the narrow tiles take the order and the bias fold of the wide kernel they stand in for -- read off the SAME branch, which is
// what makes a row's bits independent of the kernel that took it (gemm_hp_nt.inc).
struct HpKcChoice {
    int family;      // LF_HP_ROW, LF_HP_PKD, LF_HP_PKC, LF_HP_TILE or LF_HP_NARROW
    int kt;          // LF_HP_PKD: K-tiles of the launch, 8 or 16 (the kernel's template argument)
    bool xzy;        // LF_HP_NARROW: MFMA block order of the deferred-epilogue kernel
    int fold_bias;   // LF_HP_NARROW: the bias starts the accumulators, as in both persistent kernels
};
static HpKcChoice hp_kc_choice(int64_t rows, int width, int k, bool forward) {
    const bool deferred = hp_deferred_ok(k, forward);
    HpKcChoice c{};
    c.family = deferred ? LF_HP_PKD : (g_hp_persistent && k >= 3 * HP_BK) ? LF_HP_PKC : LF_HP_TILE;
    c.kt = k / HP_BK;
    if (hp_row_plan(rows, width)) {
        c.xzy = deferred;
        c.fold_bias = c.family != LF_HP_TILE;
        c.family = LF_HP_NARROW;
    } else if (deferred && g_hp_row && width == HR_BN && (rows + HP_BM - 1) / HP_BM >= g_hp_row_min_tiles) {
        c.family = LF_HP_ROW;
    }
    return c;
}

// the HpParams fields every K-contiguous launch shares
static HpParams hp_kc_params(char* c_hl, const char* a_hl, const char* b_hl, int64_t rows, int width, int k, HpScale sa, HpScale sb,
                             HpScale so, int kernel_class) {
    HpParams p{};
    p.A = a_hl; p.B = b_hl; p.C_hl = c_hl;
    p.M = (int)rows; p.N = width; p.K = k;
    p.pitchA = (long long)k * 4; p.pitchB = (long long)k * 4;
    p.a_rows = rows; p.b_rows = width;
    p.sa = sa; p.sb = sb; p.so = so;
    p.k_per_split = k; p.splits = 1; p.stagger = g_hp_stagger;
    p.stamps = hp_stamp_target(kernel_class);
    return p;
}

// Grid, launch, family count and launch check of the choice `c`.  Only the kernels the choice rule can ask for exist: no
// gemm_hp_pkd_kernel<HPE_MUL, 8> (it spills), HPE_Z only where the deferred epilogue's block order runs, HPE_HEAD in the
// row-owning kernel alone.  Anything else is an error, not another kernel.
template <int EPI>
static int hp_launch_kc(HpParams p, const HpKcChoice& c, hipStream_t stream) {
    constexpr bool INLINE_EPI = EPI == HPE_SINE || EPI == HPE_SINE_STASH || EPI == HPE_MUL;
    const bool narrow = c.family == LF_HP_NARROW;
    const int bm = narrow ? NT_BM : HP_BM, bn = narrow ? NT_BN : HP_BN;
    p.tiles_m = (int)((p.a_rows + bm - 1) / bm);
    p.tiles_n = c.family == LF_HP_ROW ? 1 : (p.N + bn - 1) / bn;   // (the row-owning block takes all 512 columns)
    if (narrow) p.fold_bias = c.fold_bias;
    if (int rc = hp_check_grid(p)) return rc;
    const long long tiles = (long long)p.tiles_m * p.tiles_n;
    const dim3 grid((unsigned)tiles), pgrid(hp_persistent_grid(tiles)), block(narrow ? NT_NTH : HP_NTH);
    bool served = false;
    if (c.family == LF_HP_ROW) {
        hipLaunchKernelGGL((gemm_hp_row_kernel<EPI>), pgrid, block, 0, stream, p);
        served = true;
    }
    if constexpr (EPI != HPE_HEAD) {
        if (c.family == LF_HP_PKD && c.kt == 16) {
            hipLaunchKernelGGL((gemm_hp_pkd_kernel<EPI, 16>), pgrid, block, 0, stream, p);
            served = true;
        } else if (c.family == LF_HP_NARROW) {
            if (c.xzy) hipLaunchKernelGGL((gemm_hp_nt_kernel<EPI, true>), grid, block, 0, stream, p);
            else hipLaunchKernelGGL((gemm_hp_nt_kernel<EPI, false>), grid, block, 0, stream, p);
            served = true;
        }
        if constexpr (EPI != HPE_MUL) {
            if (c.family == LF_HP_PKD && c.kt == 8) {
                hipLaunchKernelGGL((gemm_hp_pkd_kernel<EPI, 8>), pgrid, block, 0, stream, p);
                served = true;
            }
        }
    }
    if constexpr (INLINE_EPI) {
        if (c.family == LF_HP_PKC) {
            hipLaunchKernelGGL((gemm_hp_pkc_kernel<EPI>), pgrid, block, 0, stream, p);
            served = true;
        } else if (c.family == LF_HP_TILE) {
            hipLaunchKernelGGL((gemm_hp_kernel<HP_KC, EPI>), grid, block, 0, stream, p);
            served = true;
        }
    }
    INR_REQUIRE(served, INR_E_INVALID, "hp gemm: no kernel of family %d for epilogue %d at K = %d", c.family, EPI, p.K);
    INR_LAUNCH_CHECK();
    count_launch(c.family);
    return 0;
}

// act (HL32 [n][out_f]) = sin(omega (x W^T + b)); dact (fp32, nullable) = omega cos(.); z_only: z + b as fp32 into `dact`, nothing else
int hp_sine_forward(char* act_hl, float* dact, const char* x_hl, const char* W_hl, const float* bias, int64_t n, int in_f,
                    int out_f, float omega, HpScale sa, HpScale sb, int reverse_m, hipStream_t stream, bool z_only, HpScale so) {
    HpParams p = hp_kc_params(act_hl, x_hl, W_hl, n, out_f, in_f, sa, sb, so, KC_GEMM_FWD);
    p.C2 = dact; p.bias = bias; p.omega = omega; p.reverse_m = reverse_m;
    if (z_only) INR_REQUIRE(dact && hp_z_stash_ok(in_f), INR_E_INVALID, "hp_sine_forward: z-only stash needs the deferred-epilogue kernel");
    if (n <= 0) return 0;
    const HpKcChoice c = hp_kc_choice(n, out_f, in_f, true);
    ProfScope ps(KC_GEMM_FWD, stream);
    if (z_only) return hp_launch_kc<HPE_Z>(p, c, stream);
    if (dact) return hp_launch_kc<HPE_SINE_STASH>(p, c, stream);
    return hp_launch_kc<HPE_SINE>(p, c, stream);
}

// The last sine layer of a fit step with the head step in its epilogue (gemm_hp_row_kernel<HPE_HEAD>, gemm_hp_row.inc): dz_L (HL32, scale
// `dz_so`) over the bytes of `dact`, per 64-row half panel one row of slab_b (column sums of dz_L = the layer's bias gradient), slab_w
// (sum_n g_n sin(.) = the head's weight gradient), part_loss and part_g; max|dz_L| into `amax_out`.  2 * ceil(n / 128) slab rows.
tune_int g_hp_row_head{1};              // inr_debug_set(30, 0): never (the z-only layer + hp_head_step_kernel instead)
tune_int g_hp_row_head_min_tiles{768};  // inr_debug_set(31, v): fewest 128-row panels of a launch that takes the fused form (98,304 rows:
                                        // measured break-even at ~65-70 k rows, -1.6 % at 98 k, -2.2 % at 139 k, -2.4 % at 524 k: profiles/r05_head_fuse_sweep.txt)
bool hp_row_head_ok(int64_t n, int hidden, int in_f) {
    return g_hp_row_head && hp_deferred_ok(in_f, true) && hidden == HR_BN &&
           (n + HP_BM - 1) / HP_BM >= g_hp_row_head_min_tiles && (n + HP_BM - 1) / HP_BM < (1ll << 30);
}
int hp_row_head_rows(int64_t n) { return 2 * (int)((n + HP_BM - 1) / HP_BM); }
int hp_sine_forward_head(char* dz_hl, const char* x_hl, const char* W_hl, const float* bias, int64_t n, int in_f, int out_f, float omega,
                         HpScale sa, HpScale sb, HpScale dz_so, const float* head_w, const float* head_b, const float* target,
                         const float* weight, int64_t count_total, float* slab_b, float* slab_w, float* part_loss, float* part_g,
                         unsigned* amax_out, hipStream_t stream) {
    INR_REQUIRE(hp_row_head_ok(n, out_f, in_f), INR_E_INVALID, "hp_sine_forward_head: shape not served (n = %lld, %d -> %d)", (long long)n, in_f, out_f);
    HpParams p = hp_kc_params(dz_hl, x_hl, W_hl, n, out_f, in_f, sa, sb, dz_so, KC_GEMM_FWD);
    p.bias = bias; p.omega = omega;
    p.colsum = slab_b; p.slab_w = slab_w; p.part_loss = part_loss; p.part_g = part_g; p.amax_out = amax_out;
    p.head_w = head_w; p.head_b = head_b; p.target = target; p.tweight = weight;
    p.inv_count = (float)(1.0 / (double)(count_total > 0 ? count_total : n));
    ProfScope ps(KC_GEMM_FWD, stream);
    return hp_launch_kc<HPE_HEAD>(p, HpKcChoice{LF_HP_ROW}, stream);   // (hp_row_head_ok is this launch's own rule)
}

// rows of column sums an input-grad launch may write (two per 64-row tile is the finest any of the kernels goes)
int hp_input_grad_max_rows(int64_t n) { return 2 * (int)((n + 63) / 64); }

int hp_input_grad(char* dzprev_hl, const char* dz_hl, const char* WT_hl, const float* mul, int64_t n, int in_f, int out_f,
                  float* colsum_slab, int* colsum_rows, unsigned* amax_out, HpScale sa, HpScale sb, HpScale so,
                  hipStream_t stream) {
    HpParams p = hp_kc_params(dzprev_hl, dz_hl, WT_hl, n, in_f, out_f, sa, sb, so, KC_GEMM_DX);
    p.mul = mul; p.colsum = colsum_slab; p.amax_out = amax_out;
    const HpKcChoice c = hp_kc_choice(n, in_f, out_f, false);
    *colsum_rows = c.family == LF_HP_NARROW ? 2 * (int)((n + NT_BM - 1) / NT_BM) : 2 * (int)((n + HP_BM - 1) / HP_BM);
    if (n <= 0) return 0;
    ProfScope ps(KC_GEMM_DX, stream);
    return hp_launch_kc<HPE_MUL>(p, c, stream);
}

// ---- grid -> Fourier features -> HL32 in one kernel (dense re-sampling) --------------------------------------------------------
// inr_siren_reconstruct built its network input per chunk in four passes: fourier_kernel (1 KB per voxel written at 256
// features), tensor_amax (1 KB read), hp_convert (1 KB read, 1 KB written), then layer 0 reads the HL32 image.  Features are
// sines and cosines, so max|x| <= 1 and the input scale (floor 1.0) is 2^14 whatever the data: here one thread computes
// eight frequencies of a row exactly as fourier_kernel does (same grid rule, same fma order, same sincos) and writes their
// sin and cos octets as HL32 directly -- 1 KB written, 1 KB read per voxel, bit-identical operands.  Needs m % 32 == 0.
struct HlGrid {
    int dim;
    long long n[8];
};
__global__ void __launch_bounds__(256) INR_PACKED_F32 grid_fourier_hl_kernel(char* __restrict__ out, HlGrid g, long long row_begin, long long n_rows,
                                                              const float* __restrict__ B, int m, unsigned* __restrict__ x_amax) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) *x_amax = 0x3f800000u;                       // max(1, max|x|) = 1: what tensor_amax would have found
    const int per_row = m >> 3;
    if (t >= n_rows * per_row) return;
    const long long row = t / per_row;
    const int j0 = (int)(t - row * per_row) * 8;
    const float two_pi = 6.283185307179586f;
    long long rem = row_begin + row;
    float c[8];
#pragma unroll
    for (int a = 7; a >= 0; --a) {
        if (a < g.dim) {
            const long long idx = rem % g.n[a];
            rem /= g.n[a];
            c[a] = linspace_pm1(idx, g.n[a]);
        }
    }
    float sv[8], cv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float proj = 0.f;
#pragma unroll
        for (int a = 0; a < 8; ++a)
            if (a < g.dim) proj = fmaf(two_pi * c[a], B[(j0 + e) * g.dim + a], proj);
        sincos_f32(proj, sv[e], cv[e]);
    }
    const float s = h3_pow2(14);
    u32x4 hi, lo;
    const int cols = 2 * m;
    hp_split8(sv, s, hi, lo);
    char* dst = out + hp_off(row, j0, cols);
    *reinterpret_cast<u32x4*>(dst) = hi;
    *reinterpret_cast<u32x4*>(dst + 64) = lo;
    hp_split8(cv, s, hi, lo);
    dst = out + hp_off(row, m + j0, cols);
    *reinterpret_cast<u32x4*>(dst) = hi;
    *reinterpret_cast<u32x4*>(dst + 64) = lo;
}

bool hp_grid_fourier_ok(int m, int dim) { return m >= 32 && m % 32 == 0 && dim >= 1 && dim <= 8; }
int hp_grid_fourier_hl(char* x_hl, unsigned* x_amax, const int64_t* shape, int dim, int64_t row_begin, int64_t n_rows, const float* B,
                       int m, hipStream_t stream) {
    INR_REQUIRE(hp_grid_fourier_ok(m, dim), INR_E_INVALID, "hp_grid_fourier_hl: m = %d, dim = %d", m, dim);
    if (n_rows == 0) return 0;
    HlGrid g{};
    g.dim = dim;
    for (int a = 0; a < 8; ++a) g.n[a] = a < dim ? shape[a] : 1;
    const long long work = n_rows * (m >> 3);
    ProfScope ps(KC_OTHER, stream);
    hipLaunchKernelGGL(grid_fourier_hl_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, stream, x_hl, g, (long long)row_begin,
                       (long long)n_rows, B, m, x_amax);
    INR_LAUNCH_CHECK();
    return 0;
}

// ---- cross-layer fused forward (gemm_hp_fwd.inc) ---------------------------------------------------------------------------
bool hp_fused_forward_ok(int in_f, int hidden, int n_sine) {
    return g_hp_fused_fwd && (hidden == 512 || hidden == 256) && in_f % 32 == 0 && in_f >= 32 && in_f <= hidden && n_sine >= 1 &&
           n_sine <= FW_MAX_LAYERS;
}
// y [n] = head(sine layers(x)); x_hl: HL32 image of the network input; W_hl[l] / bias[l] / w_amax[l] per sine layer
int hp_fused_forward(float* y, const char* x_hl, const unsigned* x_amax, int64_t n, int in_f, int hidden, int n_sine,
                     const char* const* W_hl, const float* const* bias, const unsigned* const* w_amax, float first_omega,
                     float hidden_omega, const float* head_W, const float* head_b, int use_clamp, float clamp_min,
                     hipStream_t stream) {
    INR_REQUIRE(hp_fused_forward_ok(in_f, hidden, n_sine), INR_E_INVALID, "hp_fused_forward: unsupported network");
    FwParams p{};
    for (int l = 0; l < n_sine; ++l) {
        p.layer[l].W = W_hl[l];
        p.layer[l].bias = bias[l];
        p.layer[l].w_amax = w_amax[l];
        p.layer[l].K = l == 0 ? in_f : hidden;
        p.layer[l].omega = l == 0 ? first_omega : hidden_omega;
    }
    p.n_sine = n_sine; p.H = hidden;
    p.x = x_hl; p.x_amax = x_amax; p.n = n;
    p.head_W = head_W; p.head_b = head_b; p.y = y;
    p.use_clamp = use_clamp; p.clamp_min = clamp_min;
    const long long panels = (n + FW_ROWS - 1) / FW_ROWS;
    const dim3 grid(hp_persistent_grid(panels)), block(FW_NTH);
    ProfScope ps(KC_GEMM_FWD, stream);
    if (hidden == 512) hipLaunchKernelGGL((siren_fwd_fused_kernel<4>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((siren_fwd_fused_kernel<2>), grid, block, 0, stream, p);
    INR_LAUNCH_CHECK();
    count_launch(LF_HP_FUSED_FWD);
    return 0;
}

int hp_param_grad_splits(int64_t n, int in_f, int out_f) {
    const long long tiles = (long long)((out_f + HP_BM - 1) / HP_BM) * ((in_f + HP_BN - 1) / HP_BN);
    const long long ksteps = (n + HP_BK - 1) / HP_BK;
    long long want = (256 + tiles - 1) / tiles;          // one 512-thread block per CU
    const long long max_by_work = (ksteps + 7) / 8;      // at least 8 K-tiles per split
    long long s = want < max_by_work ? want : max_by_work;
    const long long min_by_offset = (n * (long long)(in_f > out_f ? in_f : out_f) * 4 + (1ll << 30) - 1) >> 30;   // 32-bit offsets
    if (s < min_by_offset) s = min_by_offset;
    // fp32 accumulation over one split's rows is a plain running sum: beyond ~16k rows its rounding error (relative to a
    // gradient that is a small mean of large terms) shows at the 1e-5 tier (256^3 volume: 8.8e-5 with 131,072 rows per
    // split) -- keep the register accumulation short and let the fixed-order slab reduction do the rest
    const long long min_by_len = (n + 16383) / 16384;
    if (s < min_by_len) s = min_by_len;
    if (s < 1) s = 1;
    if (s > 4096) s = 4096;
    return (int)s;
}

// slabs[splits][out_f][in_f] = partial dz^T x over row ranges (dz, x: HL32)
static int hp_param_grad_params(HpParams& p, float* slabs, int splits, const char* dz_hl, const char* x_hl, int64_t n, int in_f,
                                int out_f, HpScale sa, HpScale sb) {
    p = HpParams{};
    p.A = dz_hl; p.B = x_hl;
    p.M = out_f; p.N = in_f; p.K = (int)n;
    p.pitchA = (long long)out_f * 4; p.pitchB = (long long)in_f * 4;
    p.a_rows = n; p.b_rows = n;
    p.sa = sa; p.sb = sb;
    p.C2 = slabs;
    p.tiles_m = (out_f + HP_BM - 1) / HP_BM; p.tiles_n = (in_f + HP_BN - 1) / HP_BN; p.splits = splits;
    const long long ksteps = (n + HP_BK - 1) / HP_BK;
    p.k_per_split = (int)((ksteps + splits - 1) / splits) * HP_BK;
    p.slab_stride = (long long)out_f * in_f;
    INR_REQUIRE((long long)p.k_per_split * (p.pitchA > p.pitchB ? p.pitchA : p.pitchB) < (1ll << 31), INR_E_INVALID,
                "hp_param_grad_slabs: row range per split too large for 32-bit offsets");
    return hp_check_grid(p);
}
int hp_param_grad_slabs(float* slabs, int splits, const char* dz_hl, const char* x_hl, int64_t n, int in_f, int out_f,
                        HpScale sa, HpScale sb, hipStream_t stream) {
    HpParams p;
    if (int rc = hp_param_grad_params(p, slabs, splits, dz_hl, x_hl, n, in_f, out_f, sa, sb)) return rc;
    const dim3 grid((unsigned)((long long)p.tiles_m * p.tiles_n * p.splits)), block(HP_NTH);
    p.stamps = hp_stamp_target(KC_GEMM_DW);
    ProfScope ps(KC_GEMM_DW, stream);
    hipLaunchKernelGGL((gemm_hp_kernel<HP_RC, HPE_SLAB>), grid, block, 0, stream, p);
    INR_LAUNCH_CHECK();
    count_launch(LF_HP_RC);
    return 0;
}

// the same GEMMs, `jobs` of them (<= hp_param_grad_multi_max()) in one launch; every job counts as one launch of its family
int hp_param_grad_multi_max() { return HP_MULTI_MAX; }
int hp_param_grad_multi(const HpParamGradJob* jobs, int njobs, int64_t n, hipStream_t stream) {
    INR_REQUIRE(njobs >= 1 && njobs <= HP_MULTI_MAX, INR_E_INVALID, "hp_param_grad_multi: %d jobs (1 .. %d)", njobs, HP_MULTI_MAX);
    HpMultiParams m{};
    long long blocks = 0;
    for (int j = 0; j < njobs; ++j) {
        if (int rc = hp_param_grad_params(m.p[j], jobs[j].slabs, jobs[j].splits, jobs[j].dz_hl, jobs[j].x_hl, n, jobs[j].in_f,
                                          jobs[j].out_f, jobs[j].sa, jobs[j].sb))
            return rc;
        m.first[j] = (int)blocks;
        blocks += (long long)m.p[j].tiles_m * m.p[j].tiles_n * m.p[j].splits;
    }
    m.first[njobs] = (int)blocks;
    m.jobs = njobs;
    INR_REQUIRE(blocks < (1ll << 30), INR_E_INVALID, "hp_param_grad_multi: %lld blocks", blocks);
    ProfScope ps(KC_GEMM_DW, stream);
    hipLaunchKernelGGL(gemm_hp_rc_multi_kernel, dim3((unsigned)blocks), dim3(HP_NTH), 0, stream, m);
    INR_LAUNCH_CHECK();
    for (int j = 0; j < njobs; ++j) count_launch(LF_HP_RC);
    return 0;
}

int hp_head_forward(float* y, const char* a_hl, const float* W, const float* bias, int64_t n, int hidden, int use_clamp,
                    float clamp_min, hipStream_t stream, bool from_z, float omega, HpScale sa) {
    long long blocks = (n + 3) / 4;
    if (blocks > 65536) blocks = 65536;
    const dim3 grid((unsigned)blocks), block(256);
    ProfScope ps(KC_OTHER, stream);
    if (from_z) {
        switch (hidden) {
            case 128: hipLaunchKernelGGL((hp_head_forward_kernel<2, true>), grid, block, 0, stream, y, a_hl, W, bias, n, use_clamp, clamp_min, omega, sa); break;
            case 256: hipLaunchKernelGGL((hp_head_forward_kernel<4, true>), grid, block, 0, stream, y, a_hl, W, bias, n, use_clamp, clamp_min, omega, sa); break;
            case 512: hipLaunchKernelGGL((hp_head_forward_kernel<8, true>), grid, block, 0, stream, y, a_hl, W, bias, n, use_clamp, clamp_min, omega, sa); break;
            case 1024: hipLaunchKernelGGL((hp_head_forward_kernel<16, true>), grid, block, 0, stream, y, a_hl, W, bias, n, use_clamp, clamp_min, omega, sa); break;
            default: INR_REQUIRE(false, INR_E_INVALID, "hp_head_forward: hidden = %d", hidden);
        }
        INR_LAUNCH_CHECK();
        return 0;
    }
    switch (hidden) {
        case 128: hipLaunchKernelGGL((hp_head_forward_kernel<2, false>), grid, block, 0, stream, y, a_hl, W, bias, n, use_clamp, clamp_min, 0.f, sa); break;
        case 256: hipLaunchKernelGGL((hp_head_forward_kernel<4, false>), grid, block, 0, stream, y, a_hl, W, bias, n, use_clamp, clamp_min, 0.f, sa); break;
        case 512: hipLaunchKernelGGL((hp_head_forward_kernel<8, false>), grid, block, 0, stream, y, a_hl, W, bias, n, use_clamp, clamp_min, 0.f, sa); break;
        case 1024: hipLaunchKernelGGL((hp_head_forward_kernel<16, false>), grid, block, 0, stream, y, a_hl, W, bias, n, use_clamp, clamp_min, 0.f, sa); break;
        default: INR_REQUIRE(false, INR_E_INVALID, "hp_head_forward: hidden = %d", hidden);
    }
    INR_LAUNCH_CHECK();
    return 0;
}

// bound of the head's dz for an external dL/dy (the autograd path): gmax = slot holding max|g|
int hp_head_bound_ext(float* head_bound, const unsigned* gmax, const float* head_W, int hidden, float omega, hipStream_t stream) {
    ProfScope ps(KC_OTHER, stream);
    hipLaunchKernelGGL(hp_head_bound_ext_kernel, dim3(1), dim3(256), 0, stream, head_bound, gmax, head_W, hidden, omega);
    INR_LAUNCH_CHECK();
    return 0;
}

// rows per block of the head step: at most 128, fewer when that would leave CUs idle (round 2: 16 blocks at 4,096 rows, 49 us for
// 8 MB).  128, not the 256 of rounds 1-3: at 78 VGPRs six blocks share a CU, and 2,048 blocks on 1,536 slots are 1.33 rounds --
// 4,096 blocks leave a shorter tail (profiles/r04_nt_ab.txt, box 8: 0.542 ms per step outside the GEMMs against 0.551; 64 rows
// 0.546, 344 rows = one block per slot 0.576)
tune_int g_hp_head_min_rows{16};   // inr_debug_set(21, .): fewest rows a block of the head step takes (a multiple of 4)
tune_int g_hp_head_rows{0};        // inr_debug_set(23, .): rows per block of the head step, 0 = the rule below
int hp_head_rows_per_block(int64_t n) {
    if (g_hp_head_rows > 0) return (g_hp_head_rows + 3) / 4 * 4;
    long long r = (n + 1023) / 1024;
    r = (r + 3) / 4 * 4;
    const int lo = g_hp_head_min_rows;
    return (int)(r < lo ? lo : (r > 128 ? 128 : r));
}
int64_t hp_head_blocks(int64_t n) {
    const int rpb = hp_head_rows_per_block(n);
    return (n + rpb - 1) / rpb;
}

// slab_b / slab_w: [blocks][hidden], part_loss / part_g: [blocks], blocks = hp_head_blocks(n)
int hp_head_step(char* dz_hl, float* slab_b, float* slab_w, float* part_loss, float* part_g, const char* a_hl,
                 const float* dact, const float* W, const float* bias, const float* t, const float* wgt, int64_t n, int hidden,
                 int64_t count_total, unsigned* amax_out, HpScale so, hipStream_t stream, bool from_z, float omega,
                 const float* g_ext, HpScale sa) {
    const float inv = (float)(1.0 / (double)(count_total > 0 ? count_total : n));
    const int rpb = hp_head_rows_per_block(n);
    const dim3 grid((unsigned)((n + rpb - 1) / rpb)), block(256);
    ProfScope ps(KC_OTHER, stream);
#define HP_HEAD_STEP(CPL)                                                                                                   \
    do {                                                                                                                    \
        if (from_z && g_ext)                                                                                                \
            hipLaunchKernelGGL((hp_head_step_kernel<CPL, true, true>), grid, block, 0, stream, dz_hl, slab_b, slab_w,        \
                               part_loss, part_g, a_hl, dact, W, bias, t, wgt, n, inv, amax_out, so, rpb, omega, g_ext, sa);  \
        else if (from_z)                                                                                                    \
            hipLaunchKernelGGL((hp_head_step_kernel<CPL, true, false>), grid, block, 0, stream, dz_hl, slab_b, slab_w,       \
                               part_loss, part_g, a_hl, dact, W, bias, t, wgt, n, inv, amax_out, so, rpb, omega, g_ext, sa);  \
        else if (g_ext)                                                                                                     \
            hipLaunchKernelGGL((hp_head_step_kernel<CPL, false, true>), grid, block, 0, stream, dz_hl, slab_b, slab_w,       \
                               part_loss, part_g, a_hl, dact, W, bias, t, wgt, n, inv, amax_out, so, rpb, omega, g_ext, sa);  \
        else                                                                                                                \
            hipLaunchKernelGGL((hp_head_step_kernel<CPL, false, false>), grid, block, 0, stream, dz_hl, slab_b, slab_w,      \
                               part_loss, part_g, a_hl, dact, W, bias, t, wgt, n, inv, amax_out, so, rpb, omega, g_ext, sa);  \
    } while (0)
    switch (hidden) {
        case 128: HP_HEAD_STEP(2); break;
        case 256: HP_HEAD_STEP(4); break;
        case 512: HP_HEAD_STEP(8); break;
        case 1024: HP_HEAD_STEP(16); break;
        default: INR_REQUIRE(false, INR_E_INVALID, "hp_head_step: hidden = %d", hidden);
    }
#undef HP_HEAD_STEP
    INR_LAUNCH_CHECK();
    return 0;
}

}  // namespace inr
