// Spatial derivatives of a fitted WIRE network in forward mode (nn_mri.py:205-221 `gradient` / `divergence` / `laplace` applied to
// the stack of wiretest.ipynb cell 2, whose `detach()` is commented out): what jet.hip does for the SIREN, for the complex-Gabor
// layer.  Everything is real, on the planes [hr | hi] and the block images of wire.hip.  Per row the kernels carry J = 1 + dt + lap
// planes of width 2H -- the value a, one tangent t_i = d a / d x_i per tangent axis i < dt, the Laplacian accumulator q = sum_i
// d^2 a / d x_i^2 -- as [J][chunk][2H] of the workspace.  No stash, no autograd, no float atomics.
//   wired_input_kernel  -- raw coordinates: a = x, t_i = e_i, q = 0, padded to layer 0's K0 with zeros (Fourier features: the jets
//       of jet_fourier_kernel, through jet_launch_fourier; its pitch is K0)
//   wired_layer_kernel<Q, J, LAP> -- one Gabor layer: the Q J GEMMs (plane j) x (image quantity q) on the f32-input MFMA 16x16x4.
//       A block owns 32 rows x 32 units of ALL J planes and ALL Q quantities, a wave 16 x 16 of them (Q J accumulators of four
//       registers: 96 at Q = 4, J = 6), so z = (lin_r, lin_i, orth_r, orth_i) from a, u_i from t_i and r from q of one (row, unit)
//       sit in registers together in the epilogue; u and r never reach memory.  With w = omega, s2 = scale^2 and
//       out = A (cos, sin)(w lin_r) as in wire_gemm_kernel:
//           p_i  = -w u_i[lin_i] - 2 s2 (z . u_i),   g_i = w u_i[lin_r]          (d phi / d x_i = p_i + i g_i, out = exp(phi))
//           t_i' = out (p_i + i g_i)
//           q'   = out (sum_i (p_i + i g_i)^2  - w r[lin_i] - 2 s2 (z . r + sum_i |u_i|^2) + i w r[lin_r])
//       Layer 0 (Q = 2) has lin_i = orth_i = 0.
//   wired_head_kernel   -- a wave per row: y = a . hw + b_r, dy/dx_i = t_i . hw, lap = q . hw, hw = [w_r | -w_i]
// Every row is computed from its own coordinates alone with a fixed summation order, and every multiply-add of the epilogues is
// spelled out (no contraction is left to the compiler): its bits do not depend on the chunk size, on its place in a chunk, on
// which of the other outputs were asked for, or on rows versus grid form.
#include "jet_host.h"

#pragma clang fp contract(off)

namespace inr {

namespace {

constexpr int WD_BM = 32, WD_BN = 32, WD_KB = 32;
constexpr int WD_LDS = WD_KB + 4;       // LDS row pitch in floats (144 B: 16-byte fragment reads, off one bank), as wire.hip / jet.hip
constexpr int WD_THREADS = 256;

// ---- input: raw coordinates.  One thread per (row, column of the K0-wide plane)
template <bool FROM_GRID>
__global__ void __launch_bounds__(256) wired_input_kernel(float* __restrict__ out, long long plane, int K0,
                                                          const float* __restrict__ x, JetGrid g, int d, int dt, int lap,
                                                          long long row_begin, long long n_rows) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows * K0) return;
    const long long row = t / K0;
    const int k = (int)(t - row * K0);
    float c[JET_MAX_D];
    jet_coords<FROM_GRID>(c, x, g, d, FROM_GRID ? row_begin + row : row);
    float v = 0.f;
#pragma unroll
    for (int a = 0; a < JET_MAX_D; ++a)
        if (a == k && a < d) v = c[a];
    float* o = out + row * K0 + k;
    o[0] = v;
    for (int i = 0; i < dt; ++i) o[(1 + i) * plane] = (k == i) ? 1.f : 0.f;
    if (lap) o[(1 + dt) * plane] = 0.f;
}

// ---- one Gabor layer on J planes.  in: [J][.][K] (K a multiple of WD_KB, pad columns zero), img [Q][H][K], pb [Q][H],
// out [J][.][2H].  H is a multiple of WD_BN.
template <int Q, int J, bool LAP>
__global__ void __launch_bounds__(WD_THREADS) wired_layer_kernel(float* __restrict__ out, long long out_plane,
                                                                 const float* __restrict__ in, long long in_plane,
                                                                 const float* __restrict__ img, const float* __restrict__ pb, int K,
                                                                 int H, long long n_rows, float omega, float s2) {
    constexpr int DT = J - 1 - (LAP ? 1 : 0);
    static_assert(DT >= 0 && DT <= JET_MAX_D && (Q == 2 || Q == 4), "J = 1 + tangents + (Laplacian ? 1 : 0)");
    static_assert(WD_BM * WD_KB / 4 == WD_THREADS && WD_BN == WD_BM, "one 16-byte load per thread, plane and quantity");
    __shared__ __attribute__((aligned(16))) float As[J * WD_BM * WD_LDS];
    __shared__ __attribute__((aligned(16))) float Bs[Q * WD_BN * WD_LDS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g4 = lane >> 4, l16 = lane & 15;
    const int wr = wave >> 1, wc = wave & 1;
    const long long row0 = (long long)blockIdx.x * WD_BM;
    const int col0 = blockIdx.y * WD_BN;
    const long long img_plane = (long long)H * K;

    f32x4 acc[Q * J];
#pragma unroll
    for (int a = 0; a < Q * J; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int lr = tid >> 3, c4 = (tid & 7) * 4;      // this thread's (row or unit, first column) of every 32 x 32 tile
    const long long ld_row = row0 + lr;
    const bool row_ok = ld_row < n_rows;
    for (int k0 = 0; k0 < K; k0 += WD_KB) {
        __syncthreads();      // the previous K block's fragment reads are done
#pragma unroll
        for (int j = 0; j < J; ++j) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row_ok) v = *reinterpret_cast<const f32x4*>(in + j * in_plane + ld_row * K + k0 + c4);
            *reinterpret_cast<f32x4*>(As + (j * WD_BM + lr) * WD_LDS + c4) = v;
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(img + q * img_plane + (long long)(col0 + lr) * K + k0 + c4);
            *reinterpret_cast<f32x4*>(Bs + (q * WD_BN + lr) * WD_LDS + c4) = w;
        }
        __syncthreads();
#pragma unroll
        for (int k16 = 0; k16 < WD_KB / 16; ++k16) {
            // lane group g4 supplies columns 16 k16 + 4 g4 + s of both operands in MFMA s: every column once, in a fixed order
            f32x4 fb[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q)
                fb[q] = *reinterpret_cast<const f32x4*>(Bs + (q * WD_BN + wc * 16 + l16) * WD_LDS + 16 * k16 + 4 * g4);
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const f32x4 fa = *reinterpret_cast<const f32x4*>(As + (j * WD_BM + wr * 16 + l16) * WD_LDS + 16 * k16 + 4 * g4);
#pragma unroll
                for (int q = 0; q < Q; ++q)
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        acc[q * J + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[s], fb[q][s], acc[q * J + j], 0, 0, 0);
            }
        }
    }

    // accumulator register r of lane (g4, l16): row 4 g4 + r, column l16 of the wave's 16 x 16 tile
    const int col = col0 + wc * 16 + l16;
    float bq[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) bq[q] = pb[q * H + col];
    const float m2 = -2.f * s2;
    const int W2 = 2 * H;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long row = row0 + wr * 16 + 4 * g4 + r;
        if (row >= n_rows) continue;
        float z[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) z[q] = acc[q * J][r] + bq[q];
        float sq = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) sq = fmaf(z[q], z[q], sq);
        float e = -(s2 * sq);
        if (Q == 4) e = fmaf(-omega, z[1], e);
        const float amp = expf(e);
        float sn, cs;
        sincos_f32_ool(omega * z[0], sn, cs);
        const float o_r = amp * cs, o_i = amp * sn;
        float* o = out + row * W2 + col;
        o[0] = o_r;
        o[H] = o_i;
        float Sr = 0.f, Si = 0.f, uu = 0.f;
#pragma unroll
        for (int i = 0; i < DT; ++i) {
            float u[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) u[q] = acc[q * J + 1 + i][r];
            float zu = 0.f;
#pragma unroll
            for (int q = 0; q < Q; ++q) zu = fmaf(z[q], u[q], zu);
            float p = m2 * zu;
            if (Q == 4) p = fmaf(-omega, u[1], p);
            const float g = omega * u[0];
            o[(1 + i) * out_plane] = fmaf(o_r, p, -(o_i * g));
            o[(1 + i) * out_plane + H] = fmaf(o_r, g, o_i * p);
            if (LAP) {
                Sr = fmaf(p, p, Sr);
                Sr = fmaf(-g, g, Sr);
                Si = fmaf(2.f * p, g, Si);
#pragma unroll
                for (int q = 0; q < Q; ++q) uu = fmaf(u[q], u[q], uu);
            }
        }
        if (LAP) {
            float rq[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) rq[q] = acc[q * J + J - 1][r];
            float zr = uu;
#pragma unroll
            for (int q = 0; q < Q; ++q) zr = fmaf(z[q], rq[q], zr);
            float le = m2 * zr;
            if (Q == 4) le = fmaf(-omega, rq[1], le);
            const float cr = Sr + le;
            const float ci = fmaf(omega, rq[0], Si);
            o[(J - 1) * out_plane] = fmaf(o_r, cr, -(o_i * ci));
            o[(J - 1) * out_plane + H] = fmaf(o_r, ci, o_i * cr);
        }
    }
}

// ---- head: a wave per row, J dot products with hw = [w_r | -w_i] (w interleaved), in the order of wire_head_forward_kernel
__global__ void __launch_bounds__(256) wired_head_kernel(float* __restrict__ y, float* __restrict__ grad, float* __restrict__ lapl,
                                                         const float* __restrict__ in, long long plane,
                                                         const float* __restrict__ w, const float* __restrict__ b, int H, int dt,
                                                         int has_q, long long n_rows) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;      // uniform over the wave
    const int J = 1 + dt + has_q;
    float part[JET_MAX_J];
#pragma unroll
    for (int p = 0; p < JET_MAX_J; ++p) part[p] = 0.f;
    const float* a = in + row * 2 * H;
    for (int k = lane; k < H; k += 64) {
        const float w_r = w[2 * k], w_i = w[2 * k + 1];
#pragma unroll
        for (int p = 0; p < JET_MAX_J; ++p)
            if (p < J) {
                part[p] = fmaf(a[p * plane + k], w_r, part[p]);
                part[p] = fmaf(-a[p * plane + H + k], w_i, part[p]);
            }
    }
#pragma unroll
    for (int p = 0; p < JET_MAX_J; ++p) part[p] = wave_sum(part[p]);
    if (lane != 0) return;
    y[row] = part[0] + b[0];
#pragma unroll
    for (int i = 0; i < JET_MAX_D; ++i)
        if (grad && i < dt) grad[row * dt + i] = part[1 + i];
#pragma unroll
    for (int p = 1; p < JET_MAX_J; ++p)
        if (lapl && p == 1 + dt) lapl[row] = part[p];
}

// ------------------------------------------------------ host ------------------------------------------------------
// the descriptor and the input, before anything else: d coordinate axes, Fourier features (m frequencies) or raw coordinates
int wd_check_desc(const char* who, const inr_wire_desc_t* desc, int d, int m, bool fourier) {
    if (int rc = wire_check_desc(who, desc)) return rc;
    INR_REQUIRE(d >= 1 && d <= JET_MAX_D, INR_E_INVALID, "%s: 1 <= d <= %d coordinate axes (got %d)", who, JET_MAX_D, d);
    if (fourier)
        INR_REQUIRE(m >= 1 && desc->in_features == 2 * m, INR_E_INVALID, "%s: in_features (%d) must equal 2*m (%d)", who,
                    desc->in_features, 2 * m);
    else
        INR_REQUIRE(desc->in_features == d, INR_E_INVALID, "%s: without B in_features (%d) must equal d (%d)", who,
                    desc->in_features, d);
    return 0;
}

// the workspace: the layers' block images and packed biases, the input jets [J][chunk][K0] and two buffers of J planes
// [chunk][2H] that the layers write in turn.  Every region on a 256-byte boundary.  base == null: `total` (in floats) only
struct WdView {
    float *img[WIRE_MAX_LAYERS], *pb[WIRE_MAX_LAYERS];
    float *feats, *buf[2];
    int64_t total;
};
WdView wd_view(const WirePlan& p, int J, int64_t chunk, void* base) {
    WdView v;
    WsCarver c(base, 64 * sizeof(float));
    const size_t H = (size_t)p.H;
    for (int l = 0; l <= p.L; ++l) {
        v.img[l] = c.take<float>(l == 0 ? 2 * H * p.K0 : 8 * H * H);
        v.pb[l] = c.take<float>(4 * H);
    }
    v.feats = c.take<float>((size_t)J * (size_t)chunk * (size_t)p.K0);
    for (int k = 0; k < 2; ++k) v.buf[k] = c.take<float>((size_t)J * (size_t)chunk * 2 * H);
    v.total = (int64_t)(c.bytes() / sizeof(float));
    return v;
}

int wd_launch_layer(bool first, int dt, int lap, hipStream_t st, float* out, long long out_plane, const float* in, long long in_plane,
                    const float* img, const float* pb, int K, int H, long long rows, float omega, float s2) {
    const dim3 grid((unsigned)((rows + WD_BM - 1) / WD_BM), (unsigned)(H / WD_BN));
    const bool served = jet_dispatch(dt, lap, [&](auto j, auto with_lap) {
        constexpr int J = decltype(j)::value;
        constexpr bool LAP = decltype(with_lap)::value;
        if (first)
            hipLaunchKernelGGL((wired_layer_kernel<2, J, LAP>), grid, dim3(WD_THREADS), 0, st, out, out_plane, in, in_plane, img, pb,
                               K, H, rows, omega, s2);
        else
            hipLaunchKernelGGL((wired_layer_kernel<4, J, LAP>), grid, dim3(WD_THREADS), 0, st, out, out_plane, in, in_plane, img, pb,
                               K, H, rows, omega, s2);
    });
    INR_REQUIRE(served, INR_E_INVALID, "wire derivatives: no layer kernel for %d tangents, laplacian %d", dt, lap);
    INR_LAUNCH_CHECK();
    return 0;
}

// the resolved call c on the workspace.  The descriptor has been checked.
int wd_run(const char* who, const inr_wire_desc_t* desc, const float* params, const JetCall& c, void* workspace,
           int64_t workspace_floats) {
    if (c.n == 0) return 0;
    const WirePlan p = wire_plan(desc);
    const WdView v = wd_view(p, c.J, c.chunk, workspace);
    INR_REQUIRE(workspace && workspace_floats >= v.total, INR_E_WORKSPACE, "%s: workspace too small (%lld floats, %lld needed)", who,
                workspace ? (long long)workspace_floats : 0ll, (long long)v.total);
    INR_REQUIRE(aligned16(workspace), INR_E_ALIGN, "%s: workspace must be 16-byte aligned", who);

    hipStream_t st = c.st;
    if (int rc = wire_pack_images(p, v.img, v.pb, params, st)) return rc;
    const int d = c.d, dt = c.dt, has_q = c.has_q;
    const int H = p.H, K0 = p.K0, head = 4 * (p.L + 1);
    const float s2_first = desc->first_scale * desc->first_scale, s2_hidden = desc->hidden_scale * desc->hidden_scale;
    const long long plane = (long long)c.chunk * 2 * H, plane0 = (long long)c.chunk * K0;
    for (int64_t r0 = 0; r0 < c.n; r0 += c.chunk) {
        const long long rows = (c.n - r0 < c.chunk) ? (c.n - r0) : c.chunk;
        const float* xc = c.x ? c.x + r0 * d : nullptr;
        if (c.B) {
            if (int rc = jet_launch_fourier(v.feats, plane0, K0, xc, c.shape, d, dt, has_q, r0, rows, c.B, c.m, st)) return rc;
        } else {
            if (c.x)
                hipLaunchKernelGGL(wired_input_kernel<false>, dim3(jet_blocks(rows * K0)), dim3(256), 0, st, v.feats, plane0, K0, xc,
                                   c.grid, d, dt, has_q, (long long)r0, rows);
            else
                hipLaunchKernelGGL(wired_input_kernel<true>, dim3(jet_blocks(rows * K0)), dim3(256), 0, st, v.feats, plane0, K0, xc,
                                   c.grid, d, dt, has_q, (long long)r0, rows);
            INR_LAUNCH_CHECK();
        }
        const float* in = v.feats;
        for (int l = 0; l <= p.L; ++l) {
            float* out = v.buf[l & 1];
            if (int rc = wd_launch_layer(l == 0, dt, has_q, st, out, plane, in, l == 0 ? plane0 : plane, v.img[l], v.pb[l],
                                         l == 0 ? K0 : 2 * H, H, rows, l == 0 ? desc->first_omega : desc->hidden_omega,
                                         l == 0 ? s2_first : s2_hidden))
                return rc;
            in = out;
        }
        hipLaunchKernelGGL(wired_head_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, c.y + r0,
                           c.grad ? c.grad + r0 * dt : nullptr, c.lap ? c.lap + r0 : nullptr, in, plane, params + p.off[head],
                           params + p.off[head + 1], H, dt, has_q, rows);
        INR_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_wire_derivatives_workspace_floats(const inr_wire_desc_t* desc, int d, int m, int64_t chunk_rows, int want_laplacian) {
    if (chunk_rows < 1 || chunk_rows > JET_MAX_ROWS) {
        set_error("inr_wire_derivatives_workspace_floats: bad chunk_rows %lld", (long long)chunk_rows);
        return 0;
    }
    if (wd_check_desc("inr_wire_derivatives_workspace_floats", desc, d, m, m > 0)) return 0;
    return wd_view(wire_plan(desc), 1 + d + (want_laplacian ? 1 : 0), chunk_rows, nullptr).total;
}

int inr_wire_derivatives(const inr_wire_desc_t* desc, const float* params, const float* x, int64_t n, int d, int d_tangent,
                         const float* B, int m, float* y, float* grad, float* lap, int64_t chunk_rows, void* workspace,
                         int64_t workspace_floats, void* stream) {
    if (int rc = wd_check_desc("inr_wire_derivatives", desc, d, m, B != nullptr)) return rc;
    INR_REQUIRE(params && x && y, INR_E_INVALID, "inr_wire_derivatives: null pointer");
    INR_REQUIRE(n >= 0 && n <= JET_MAX_ROWS, INR_E_INVALID, "inr_wire_derivatives: bad row count %lld", (long long)n);
    JetCall c;
    if (int rc = jet_resolve(c, "inr_wire_derivatives", params, x, nullptr, n, d, d_tangent, B, m, y, grad, lap, chunk_rows, stream))
        return rc;
    return wd_run("inr_wire_derivatives", desc, params, c, workspace, workspace_floats);
}

int inr_wire_derivatives_grid(const inr_wire_desc_t* desc, const float* params, const int64_t* shape, int dim, int d_tangent,
                              const float* B, int m, float* y, float* grad, float* lap, int64_t chunk_rows, void* workspace,
                              int64_t workspace_floats, void* stream) {
    if (int rc = wd_check_desc("inr_wire_derivatives_grid", desc, dim, m, B != nullptr)) return rc;
    INR_REQUIRE(params && shape && y, INR_E_INVALID, "inr_wire_derivatives_grid: null pointer");
    int64_t total;
    if (int rc = check_grid_shape("inr_wire_derivatives_grid", shape, dim, JET_MAX_ROWS, &total)) return rc;
    JetCall c;
    if (int rc = jet_resolve(c, "inr_wire_derivatives_grid", params, nullptr, shape, total, dim, d_tangent, B, m, y, grad, lap,
                             chunk_rows, stream))
        return rc;
    return wd_run("inr_wire_derivatives_grid", desc, params, c, workspace, workspace_floats);
}

}  // extern "C"
