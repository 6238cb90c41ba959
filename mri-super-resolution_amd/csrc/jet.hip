// Spatial derivatives of a fitted SIREN in forward mode (nn_mri.py:205-221 `gradient` / `divergence` / `laplace`, which run two
// torch.autograd.grad passes with create_graph=True): per row and layer the kernels carry J = 1 + dt + lap vectors of the layer's
// width -- the value a, one tangent t_i = d a / d x_i per tangent axis i < dt, and the Laplacian accumulator q = sum_i d^2 a /
// d x_i^2 -- as J planes [J][chunk][width] of the workspace.  No stash, no autograd, no float atomics.
//   jet_fourier_kernel -- the jets of the Fourier features [sin p | cos p], p = 2 pi x B^T (coordinates from the grid rule of
//       inr_mgrid, or from the caller's rows)
//   jet_first_kernel   -- raw coordinates: the first sine layer on the VALU (K = d <= 4; u_i is column i of W_0, r = 0)
//   jet_layer_kernel   -- one sine layer: the J GEMMs [a | t_i | q] W^T on the f32-input MFMA 32x32x2.  A block owns 64 rows x
//       64 columns of ALL J planes, a wave 32 x 32 of them, so that z, every u_i = W t_i and r = W q of one (row, column) sit in
//       registers together in the epilogue:  a' = sin(w z),  t_i' = w cos(w z) u_i,  q' = w cos(w z) r - w^2 sin(w z) sum_i u_i^2.
//       u and r never reach memory.
//   jet_head_kernel    -- a wave per row: y = w.a + b, dy/dx_i = w.t_i, lap = w.q (lane-strided partial sums, xor-shuffle tree).
// Every row is computed from its own coordinates alone with a fixed summation order: its bits do not depend on the chunk size,
// on its place in a chunk, or on which of the other outputs were asked for.
#include "jet_host.h"

#include <vector>

namespace inr {

namespace {

constexpr int JET_BM = 64, JET_BN = 64, JET_KB = 32;
constexpr int JET_LDS = JET_KB + 4;     // LDS row pitch in floats: 144 B keeps the 16-byte fragment reads aligned and off one bank
constexpr int JET_THREADS = 256;
constexpr float JET_TWO_PI = 6.283185307179586f;

// (the d coordinates of one row: jet_coords, common.h)
// ---- input: jets of the Fourier features.  One thread per (row, frequency); planes of `pitch` = 2m rounded up to the GEMM's K block,
// the pad columns zero.  a = [sin p | cos p] with p accumulated exactly as fourier_kernel does.
template <bool FROM_GRID>
__global__ void __launch_bounds__(256) jet_fourier_kernel(float* __restrict__ out, long long plane, int pitch,
                                                          const float* __restrict__ x, JetGrid g, int d, int dt, int lap,
                                                          long long row_begin, long long n_rows,
                                                          const float* __restrict__ B, int m) {
    const int mp = pitch / 2;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows * mp) return;
    const long long row = t / mp;
    const int j = (int)(t - row * mp);
    const int J = 1 + dt + lap;
    float* o = out + row * pitch;
    if (j >= m) {   // pad columns 2m .. pitch - 1, two per thread
        const int c0 = 2 * m + 2 * (j - m);
        for (int p = 0; p < J; ++p) {
            o[p * plane + c0] = 0.f;
            o[p * plane + c0 + 1] = 0.f;
        }
        return;
    }
    float c[JET_MAX_D];
    jet_coords<FROM_GRID>(c, x, g, d, FROM_GRID ? row_begin + row : row);
    float proj = 0.f;
#pragma unroll
    for (int a = 0; a < JET_MAX_D; ++a)
        if (a < d) proj = fmaf(JET_TWO_PI * c[a], B[j * d + a], proj);
    float sn, cs;
    sincos_f32_ool(proj, sn, cs);
    o[j] = sn;
    o[m + j] = cs;
    float nb = 0.f;
#pragma unroll
    for (int i = 0; i < JET_MAX_D; ++i)
        if (i < dt) {
            const float w = JET_TWO_PI * B[j * d + i];
            o[(1 + i) * plane + j] = w * cs;
            o[(1 + i) * plane + m + j] = -(w * sn);
            nb = fmaf(w, w, nb);
        }
    if (lap) {
        o[(1 + dt) * plane + j] = -(nb * sn);
        o[(1 + dt) * plane + m + j] = -(nb * cs);
    }
}

// ---- input: raw coordinates feed the network -- the first sine layer on the VALU.  One thread per (row, hidden unit).
template <bool FROM_GRID>
__global__ void __launch_bounds__(256) jet_first_kernel(float* __restrict__ out, long long plane, const float* __restrict__ x,
                                                        JetGrid g, int d, int dt, int lap, long long row_begin, long long n_rows,
                                                        const float* __restrict__ W0, const float* __restrict__ b0, int H,
                                                        float omega) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows * H) return;
    const long long row = t / H;
    const int h = (int)(t - row * H);
    float c[JET_MAX_D];
    jet_coords<FROM_GRID>(c, x, g, d, FROM_GRID ? row_begin + row : row);
    float z = b0[h];
#pragma unroll
    for (int a = 0; a < JET_MAX_D; ++a)
        if (a < d) z = fmaf(W0[h * d + a], c[a], z);
    float sn, cs;
    sincos_f32_ool(omega * z, sn, cs);
    const float oc = omega * cs;
    float* o = out + row * H + h;
    o[0] = sn;
    float su = 0.f;
#pragma unroll
    for (int i = 0; i < JET_MAX_D; ++i)
        if (i < dt) {
            const float u = W0[h * d + i];
            o[(1 + i) * plane] = oc * u;
            su = fmaf(u, u, su);
        }
    if (lap) o[(1 + dt) * plane] = -((omega * omega * sn) * su);
}

// ---- one sine layer on J planes.  in: [J][.][lda] (lda a multiple of JET_KB, columns K .. lda - 1 zero), W [H][K], out [J][.][H].
template <int J, bool LAP>
__global__ void __launch_bounds__(JET_THREADS) jet_layer_kernel(float* __restrict__ out, long long out_plane,
                                                                const float* __restrict__ in, long long in_plane, int lda,
                                                                const float* __restrict__ W, const float* __restrict__ bias,
                                                                int K, int H, long long n_rows, float omega) {
    constexpr int DT = J - 1 - (LAP ? 1 : 0);
    static_assert(DT >= 0 && DT <= JET_MAX_D, "J = 1 + tangents + (Laplacian ? 1 : 0)");
    __shared__ __attribute__((aligned(16))) float As[J * JET_BM * JET_LDS];
    __shared__ __attribute__((aligned(16))) float Ws[JET_BN * JET_LDS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, l32 = lane & 31;
    const int wr = wave >> 1, wc = wave & 1;
    const long long row0 = (long long)blockIdx.x * JET_BM;
    const int col0 = blockIdx.y * JET_BN;
    const bool w_vec = (K & 3) == 0;      // rows of W are 16-byte aligned (every tensor of the flat buffer starts at one)

    f32x16 acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    for (int k0 = 0; k0 < lda; k0 += JET_KB) {
        __syncthreads();      // the previous K block's fragment reads are done
#pragma unroll
        for (int i = 0; i < (JET_BM * JET_KB / 4) / JET_THREADS; ++i) {
            const int f = tid + JET_THREADS * i;
            const int r = f >> 3, c4 = (f & 7) * 4;
            const long long row = row0 + r;
            const bool ok = row < n_rows;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (ok) v = *reinterpret_cast<const f32x4*>(in + j * in_plane + row * lda + k0 + c4);
                *reinterpret_cast<f32x4*>(As + (j * JET_BM + r) * JET_LDS + c4) = v;
            }
            // the weight tile has the same 64 x 32 shape: the same thread map
            const int col = col0 + r;
            f32x4 w = {0.f, 0.f, 0.f, 0.f};
            if (col < H) {
                const float* src = W + (long long)col * K + k0 + c4;
                if (w_vec && k0 + c4 + 3 < K) {
                    w = *reinterpret_cast<const f32x4*>(src);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (k0 + c4 + e < K) w[e] = src[e];
                }
            }
            *reinterpret_cast<f32x4*>(Ws + r * JET_LDS + c4) = w;
        }
        __syncthreads();
#pragma unroll
        for (int k8 = 0; k8 < JET_KB / 8; ++k8) {
            const f32x4 fb = *reinterpret_cast<const f32x4*>(Ws + (wc * 32 + l32) * JET_LDS + 8 * k8 + 4 * hh);
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const f32x4 fa = *reinterpret_cast<const f32x4*>(As + (j * JET_BM + wr * 32 + l32) * JET_LDS + 8 * k8 + 4 * hh);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s], fb[s], acc[j], 0, 0, 0);
            }
        }
    }

    const int col = col0 + wc * 32 + l32;
    if (col >= H) return;     // uniform over the wave: H is a multiple of 32
    const float bj = bias[col];
    const float o2 = omega * omega;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long row = row0 + wr * 32 + mfma32_acc_row(r, hh);
        if (row >= n_rows) continue;
        float sn, cs;
        sincos_f32_ool(omega * (acc[0][r] + bj), sn, cs);
        const float oc = omega * cs;
        float* o = out + row * H + col;
        o[0] = sn;
        float su = 0.f;
#pragma unroll
        for (int i = 0; i < DT; ++i) {
            const float u = acc[1 + i][r];
            o[(1 + i) * out_plane] = oc * u;
            su = fmaf(u, u, su);
        }
        if (LAP) o[(J - 1) * out_plane] = fmaf(oc, acc[J - 1][r], -((o2 * sn) * su));
    }
}

// ---- head: a wave per row, J dot products with the head's weight row
__global__ void __launch_bounds__(256) jet_head_kernel(float* __restrict__ y, float* __restrict__ grad, float* __restrict__ lapl,
                                                       const float* __restrict__ in, long long plane, const float* __restrict__ w,
                                                       const float* __restrict__ b, int H, int dt, int has_q, long long n_rows) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;      // uniform over the wave
    const int J = 1 + dt + has_q;
    float part[JET_MAX_J];
#pragma unroll
    for (int p = 0; p < JET_MAX_J; ++p) part[p] = 0.f;
    const float* a = in + row * H;
    for (int h = lane; h < H; h += 64) {
        const float wh = w[h];
#pragma unroll
        for (int p = 0; p < JET_MAX_J; ++p)
            if (p < J) part[p] = fmaf(wh, a[p * plane + h], part[p]);
    }
#pragma unroll
    for (int p = 0; p < JET_MAX_J; ++p)
        part[p] = wave_sum(part[p]);
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
struct JetPlan {
    int d = 0, H = 0, S = 0;              // coordinate axes, hidden width, sine layers
    int pitch0 = 0;                       // Fourier features: 2m rounded up to JET_KB; raw coordinates: 0
    int max_pitch = 0;
    Layout L;                             // the flat layout of inr_siren_param_offsets, head last
};

int jet_check_desc(const char* who, const inr_siren_desc_t* d, int dims, int m, bool fourier) {
    INR_REQUIRE(d != nullptr, INR_E_INVALID, "%s: siren descriptor is null", who);
    INR_REQUIRE(d->out_features == 1, INR_E_INVALID, "%s: out_features must be 1 (got %d)", who, d->out_features);
    INR_REQUIRE(dims >= 1 && dims <= JET_MAX_D, INR_E_INVALID, "%s: 1 <= d <= %d coordinate axes (got %d)", who, JET_MAX_D, dims);
    INR_REQUIRE(d->hidden_layers >= 1, INR_E_INVALID, "%s: at least one hidden layer (got %d)", who, d->hidden_layers);
    INR_REQUIRE(d->hidden_features >= 32 && d->hidden_features <= 1024 && d->hidden_features % 32 == 0, INR_E_INVALID,
                "%s: hidden width must be a multiple of 32 up to 1024 (got %d)", who, d->hidden_features);
    if (fourier)
        INR_REQUIRE(m >= 1 && m <= (1 << 20) && d->in_features == 2 * m, INR_E_INVALID,
                    "%s: in_features (%d) must equal 2*m (%d)", who, d->in_features, 2 * m);
    else
        INR_REQUIRE(d->in_features == dims, INR_E_INVALID, "%s: without B in_features (%d) must equal d (%d)", who,
                    d->in_features, dims);
    return 0;
}

JetPlan jet_plan(const inr_siren_desc_t* d, int dims, bool fourier) {
    JetPlan p;
    p.d = dims;
    p.H = d->hidden_features;
    p.S = 1 + d->hidden_layers;
    p.pitch0 = fourier ? (int)round_up((size_t)d->in_features, JET_KB) : 0;
    p.max_pitch = p.pitch0 > p.H ? p.pitch0 : p.H;
    p.L = make_layout(d);
    return p;
}

// the workspace: two buffers of J planes [chunk][max_pitch] that the layers write in turn.  base == null: `total` only
struct JetView { float* buf[2]; size_t total; };
JetView jet_view(const JetPlan& p, int J, int64_t chunk, void* base) {
    JetView v;
    WsCarver c(base, 256);
    for (int k = 0; k < 2; ++k) v.buf[k] = c.take<float>((size_t)J * (size_t)chunk * (size_t)p.max_pitch);
    v.total = c.bytes();
    return v;
}

int jet_launch_layer(int dt, int lap, hipStream_t st, float* out, long long out_plane, const float* in, long long in_plane, int lda,
                     const float* W, const float* bias, int K, int H, long long rows, float omega) {
    const dim3 grid((unsigned)((rows + JET_BM - 1) / JET_BM), (unsigned)((H + JET_BN - 1) / JET_BN));
    const bool served = jet_dispatch(dt, lap, [&](auto j, auto with_lap) {
        hipLaunchKernelGGL((jet_layer_kernel<decltype(j)::value, decltype(with_lap)::value>), grid, dim3(JET_THREADS), 0, st, out,
                           out_plane, in, in_plane, lda, W, bias, K, H, rows, omega);
    });
    INR_REQUIRE(served, INR_E_INVALID, "jet layer: no kernel for %d tangents, laplacian %d", dt, lap);
    INR_LAUNCH_CHECK();
    count_launch(LF_JET_BASE + INR_JET_LF_LAYER);
    return 0;
}

// the resolved call c on the workspace.  The descriptor has been checked.
int jet_run(const char* who, const inr_siren_desc_t* desc, const float* params, const JetCall& c, void* workspace,
            size_t workspace_bytes) {
    if (c.n == 0) return 0;
    const bool fourier = c.B != nullptr;
    const JetPlan p = jet_plan(desc, c.d, fourier);
    const JetView v = jet_view(p, c.J, c.chunk, workspace);
    INR_REQUIRE(workspace && workspace_bytes >= v.total, INR_E_WORKSPACE, "%s: workspace too small (%zu bytes, %zu needed)", who,
                workspace ? workspace_bytes : (size_t)0, v.total);
    INR_REQUIRE(aligned16(workspace), INR_E_ALIGN, "%s: workspace must be 16-byte aligned", who);

    hipStream_t st = c.st;
    float* const* buf = v.buf;
    const int d = c.d, dt = c.dt, has_q = c.has_q;
    const int H = p.H;
    for (int64_t r0 = 0; r0 < c.n; r0 += c.chunk) {
        const long long rows = (c.n - r0 < c.chunk) ? (c.n - r0) : c.chunk;
        const float* xc = c.x ? c.x + r0 * d : nullptr;
        int cur = 0, first_gemm;
        if (fourier) {
            if (int rc = jet_launch_fourier(buf[0], (long long)c.chunk * p.pitch0, p.pitch0, xc, c.shape, d, dt, has_q, r0, rows, c.B,
                                            c.m, st))
                return rc;
            first_gemm = 0;
        } else {
            const long long plane = (long long)c.chunk * H;
            const long long work = rows * H;
            if (c.x)
                hipLaunchKernelGGL(jet_first_kernel<false>, dim3(jet_blocks(work)), dim3(256), 0, st, buf[0], plane, xc, c.grid, d, dt,
                                   has_q, (long long)r0, rows, params + p.L.w_off[0], params + p.L.b_off[0], H, desc->first_omega);
            else
                hipLaunchKernelGGL(jet_first_kernel<true>, dim3(jet_blocks(work)), dim3(256), 0, st, buf[0], plane, xc, c.grid, d, dt,
                                   has_q, (long long)r0, rows, params + p.L.w_off[0], params + p.L.b_off[0], H, desc->first_omega);
            first_gemm = 1;
        }
        INR_LAUNCH_CHECK();
        count_launch(LF_JET_BASE + INR_JET_LF_INPUT);
        for (int l = first_gemm; l < p.S; ++l) {
            const int K = l == 0 ? desc->in_features : H;
            const int lda = l == 0 ? p.pitch0 : H;
            if (int rc = jet_launch_layer(dt, has_q, st, buf[cur ^ 1], (long long)c.chunk * H, buf[cur], (long long)c.chunk * lda, lda,
                                          params + p.L.w_off[l], params + p.L.b_off[l], K, H, rows, layer_omega(desc, l)))
                return rc;
            cur ^= 1;
        }
        hipLaunchKernelGGL(jet_head_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, c.y + r0,
                           c.grad ? c.grad + r0 * dt : nullptr, c.lap ? c.lap + r0 : nullptr, buf[cur], (long long)c.chunk * H,
                           params + p.L.w_off[p.S], params + p.L.b_off[p.S], H, dt, has_q, rows);
        INR_LAUNCH_CHECK();
        count_launch(LF_JET_BASE + INR_JET_LF_HEAD);
    }
    return 0;
}

}  // namespace

// ---- launcher other units may call (internal.h) ----------------------------------------------------------------------------
int jet_launch_fourier(float* out, long long plane, int pitch, const float* x, const int64_t* shape, int d, int dt, int lap,
                       int64_t row_begin, int64_t n_rows, const float* B, int m, hipStream_t st) {
    const JetGrid g = jet_grid(shape, d);
    const dim3 grid(jet_blocks((long long)n_rows * (pitch / 2)));
    if (x)
        hipLaunchKernelGGL(jet_fourier_kernel<false>, grid, dim3(256), 0, st, out, plane, pitch, x, g, d, dt, lap,
                           (long long)row_begin, (long long)n_rows, B, m);
    else
        hipLaunchKernelGGL(jet_fourier_kernel<true>, grid, dim3(256), 0, st, out, plane, pitch, x, g, d, dt, lap,
                           (long long)row_begin, (long long)n_rows, B, m);
    INR_LAUNCH_CHECK();
    return 0;
}

}  // namespace inr

using namespace inr;

extern "C" {

size_t inr_siren_jet_workspace_bytes(const inr_siren_desc_t* desc, int d, int m, int64_t chunk_rows, int want_laplacian) {
    if (chunk_rows < 1 || chunk_rows > JET_MAX_ROWS) return 0;
    if (jet_check_desc("inr_siren_jet_workspace_bytes", desc, d, m, m > 0)) return 0;
    return jet_view(jet_plan(desc, d, m > 0), 1 + d + (want_laplacian ? 1 : 0), chunk_rows, nullptr).total;
}

int inr_siren_jet(const inr_siren_desc_t* desc, const float* params, const float* x, int64_t n, int d, int d_tangent, const float* B,
                  int m, float* y, float* grad, float* lap, int64_t chunk_rows, void* workspace, size_t workspace_bytes,
                  void* stream) {
    if (int rc = jet_check_desc("inr_siren_jet", desc, d, m, B != nullptr)) return rc;
    INR_REQUIRE(params && x && y, INR_E_INVALID, "inr_siren_jet: null pointer");
    INR_REQUIRE(n >= 0 && n <= JET_MAX_ROWS, INR_E_INVALID, "inr_siren_jet: bad row count %lld", (long long)n);
    JetCall c;
    if (int rc = jet_resolve(c, "inr_siren_jet", params, x, nullptr, n, d, d_tangent, B, m, y, grad, lap, chunk_rows, stream)) return rc;
    return jet_run("inr_siren_jet", desc, params, c, workspace, workspace_bytes);
}

int inr_siren_jet_grid(const inr_siren_desc_t* desc, const float* params, const int64_t* shape, int dim, int d_tangent,
                       const float* B, int m, float* y, float* grad, float* lap, int64_t chunk_rows, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (int rc = jet_check_desc("inr_siren_jet_grid", desc, dim, m, B != nullptr)) return rc;
    INR_REQUIRE(params && shape && y, INR_E_INVALID, "inr_siren_jet_grid: null pointer");
    int64_t total;
    if (int rc = check_grid_shape("inr_siren_jet_grid", shape, dim, JET_MAX_ROWS, &total)) return rc;
    JetCall c;
    if (int rc = jet_resolve(c, "inr_siren_jet_grid", params, nullptr, shape, total, dim, d_tangent, B, m, y, grad, lap, chunk_rows,
                             stream))
        return rc;
    return jet_run("inr_siren_jet_grid", desc, params, c, workspace, workspace_bytes);
}

}  // extern "C"
