// Multi-frame TV / Huber super-resolution: K acquisitions of one image, each displaced by a fraction of a pixel, and the prior of
// tvsr.hip:
//   x* = argmin_x 1/2 sum_k sum_i w_ki ((A_k x)_i - y_ki)^2 + lambda sum_j H_alpha(|(grad x)_j|),   A_k = B S_k.
// Images are HR [n][H][W] and LR frames [n][K][h][w], H = f0 h, W = f1 w.  B is the block operator of tvsr.hip (k [f0][f1], sum k = 1).
// S_k is the bilinear translation by the frame's shift s = (s0, s1) in HR pixels, a DEVICE double pair of shifts [n][K][2]: with
// n = floor(s), t = s - n per axis, (S x)[i][j] = sum_{da, db in {0, 1}} wa wb x[i + n0 + da][j + n1 + db], wa = (1 - t0, t0)[da], wb
// likewise.  A_k is therefore ONE weighted sum over the effective kernel ke [f0 + 1][f1 + 1],
//   ke[a][b] = sum_{da, db} (wa wb) k[a - da][b - db]   (taps in ascending (da, db); a tap whose t is exactly 0 is not visited),
//   (A_k x)[i][j] = sum_{a, b} ke[a][b] x[n0 + f0 i + a][n1 + f1 j + b]   (ascending (a, b), over f0 (+ 1 if t0 > 0) rows, columns alike),
// so a zero shift is the block sum of tvsr.hip bit for bit.  A datum (k, i, j) is VALID when that footprint -- rows n0 + f0 i ..
// n0 + f0 i + f0 - 1 (+ 1 if t0 > 0), columns alike -- lies inside the image; an invalid datum has weight 0 whatever `weight` holds, its
// y and weight are never read and its dual variable is 0.  A frame whose shift is not finite or exceeds 2^20 in magnitude is invalid as
// a whole: the test comes BEFORE the conversion to int (mf_geo), so no shift value gives an undefined conversion or an index outside
// the image.  The adjoint is a gather: HR pixel m sums ke[a][b] r[i][j] over the at most 2 x 2 valid LR pixels of every frame with
// m = n + f i + a, frames ascending, then LR rows, then columns.  No atomics anywhere.
//
// Chambolle-Pock with BOTH terms dual, from x = xbar = x0 (default: the block replication of frame 0), p = 0, q = 0:
//   p    <- (p + sigma grad(xbar)) / (1 + sigma alpha / lambda);  p <- p / max(1, |p| / lambda)        (lambda = 0: p = 0)
//   q_k  <- (q_k + sigma (A_k xbar - y_k)) / (1 + sigma / w_k)    for valid data with w_k > 0, else 0
//   x'   <- x - tau (sum_k A_k^T q_k - div p)                     frames in ascending k
//   xbar <- 2 x' - x;  x <- x'
// tau = sigma = 1 / sqrt(8 + K' c), c = (sum |k|) (max |k|) from the host in fp64, K' the number of the image's frames that hold at
// least one valid datum (all K of them unless a frame lies outside the image: such a frame is the zero operator).  |A_k|^2 <=
// |A_k|_1 |A_k|_inf, the row sums of A_k are sum |ke| <= sum |k| and its column sums are <= max |k| (bilinear spreading is a convex
// combination, and one residue class of (f0, f1) meets k once), so |(grad, A_1 .. A_K)|^2 <= 8 + K' c.
//
// LAUNCHES.  Plain launches on the caller's stream: no cooperative launch, no grid barrier, no spin, no host read.
//   init    (thread per element):     writes its own x, xbar, p0, p1 (per HR pixel), q (per LR datum), ke entry and the frame's (n0, n1,
//                                     flags) (per table entry), tau (per image);
//   dual    (thread per HR pixel e AND per LR datum): a pixel thread reads xbar[e], xbar[e + W], xbar[e + 1] -- neighbours' --, reads
//                                     and writes p0[e], p1[e] -- its own; a datum thread reads xbar over its footprint -- others' --,
//                                     reads and writes its own q;
//   primal  (thread per HR pixel e):  gathers q of up to 4 K data and p at e, e - W, e - 1 -- others' --, reads and writes x[e],
//                                     xbar[e] -- its own (the last iteration leaves x' - x in xbar, which nothing differences again);
//   final   (workgroup per part):     reads x across threads, writes the result and the partials of energy, change and the count of
//                                     valid data; finish: one workgroup per image reduces the partials in a fixed order.
// Within a launch a field is either read across threads or written by its owner alone: xbar is read-only in the dual kernel and
// owner-written in the primal one, p and q are owner-written in the dual kernel and read-only in the primal one, x is touched by its
// own thread only; the table and tau are written by init and read-only after it.  STREAM ORDER IS THE BARRIER between launches.
//
// An image's HR pixels followed by its K h w data are cut into "parts" of MF_PART elements; the partials are per PART, and thread t
// of the finish adds partials t, t + 256, ... in ascending order, so the bits of energy and change depend on the shape alone: not on
// the grid (capped at TV_STRIDE_MAX_GRID, or by the test-only inr_debug_set(32, .)), the stream, or the place in a batch.  All arithmetic is
// fp64; the fp32 entry converts at load and rounds once at the store.  The unit is compiled with -ffp-contract=off (_build.py), so
// the two entries, whose kernels differ in their loads and stores only, agree bit for bit.
//
// The block kernel with its check and the size refusals are tv_block.h's (TvBlock carries c beside |k|^2); the Huber function, the
// floor division, the grids, the refusals of the scalar parameters and the finish kernel are tv_shared.h's, which tv_block.h includes.
#include "tv_block.h"

namespace inr {
namespace {

constexpr int MF_THREADS = 256;
constexpr int MF_MAX_FACTOR = INR_TVSR_MAX_FACTOR;
constexpr int MF_MAX_FRAMES = INR_TVMF_MAX_FRAMES;
constexpr int MF_PART = 4 * MF_THREADS;                                  // elements of a part: four per thread
constexpr int MF_KE_MAX = (MF_MAX_FACTOR + 1) * (MF_MAX_FACTOR + 1);
constexpr double MF_MAX_SHIFT = 1048576.0;                               // 2^20 HR pixels

struct MfShape {
    int H, W, h, w, f0, f1, K;
    int parts;   // per image: ceil((H W + K h w) / MF_PART)
};

// one frame's geometry; flags: 1 the shift is usable, 2 t0 > 0, 4 t1 > 0
struct MfGeo {
    int n0, n1, flags;
    double t0, t1;
};

// THE conversion of a shift: the range test first (false for NaN and the infinities), then floor of a value within +-2^20
__device__ __forceinline__ MfGeo mf_geo(const double* shift) {
    const double s0 = shift[0], s1 = shift[1];
    const bool ok = fabs(s0) <= MF_MAX_SHIFT && fabs(s1) <= MF_MAX_SHIFT;
    const double c0 = ok ? s0 : 0.0, c1 = ok ? s1 : 0.0;
    const double fl0 = floor(c0), fl1 = floor(c1);
    MfGeo g;
    g.n0 = (int)fl0;
    g.n1 = (int)fl1;
    g.t0 = c0 - fl0;
    g.t1 = c1 - fl1;
    g.flags = (ok ? 1 : 0) | (g.t0 > 0.0 ? 2 : 0) | (g.t1 > 0.0 ? 4 : 0);
    return g;
}

// ke[a][b] from the block kernel ks [f0][f1]
__device__ __forceinline__ double mf_ke(const double* ks, int f0, int f1, const MfGeo& g, int a, int b) {
    double acc = 0.0;
    for (int da = 0; da <= ((g.flags >> 1) & 1); ++da) {
        const int aa = a - da;
        if (aa < 0 || aa >= f0) continue;
        const double wa = da ? g.t0 : 1.0 - g.t0;
        for (int db = 0; db <= ((g.flags >> 2) & 1); ++db) {
            const int bb = b - db;
            if (bb < 0 || bb >= f1) continue;
            const double wb = db ? g.t1 : 1.0 - g.t1;
            acc += (wa * wb) * ks[aa * f1 + bb];
        }
    }
    return acc;
}

// LR index i of an axis: its footprint n + f i .. n + f i + e - 1 inside 0 .. N - 1
__device__ __forceinline__ bool mf_inside(int n, int e, int f, int i, int N) {
    const int r = n + f * i;
    return r >= 0 && r + e <= N;
}
// some i of 0 .. cnt - 1 is inside
__device__ __forceinline__ bool mf_axis_live(int n, int e, int f, int cnt, int N) {
    const int i = n >= 0 ? 0 : (-n + f - 1) / f;
    return i < cnt && n + f * i + e <= N;
}
__device__ __forceinline__ bool mf_frame_live(const MfGeo& g, const MfShape& s) {
    return (g.flags & 1) && mf_axis_live(g.n0, s.f0 + ((g.flags >> 1) & 1), s.f0, s.h, s.H) &&
           mf_axis_live(g.n1, s.f1 + ((g.flags >> 2) & 1), s.f1, s.w, s.W);
}
__device__ __forceinline__ bool mf_valid(const MfShape& s, int n0, int n1, int flags, int i, int j) {
    return (flags & 1) && mf_inside(n0, s.f0 + ((flags >> 1) & 1), s.f0, i, s.H) && mf_inside(n1, s.f1 + ((flags >> 2) & 1), s.f1, j, s.W);
}

// (A_k x)[i][j] of a VALID datum; kek [f0 + 1][f1 + 1] of the frame, x one image
__device__ __forceinline__ double mf_apply(const double* x, const double* kek, const MfShape& s, int n0, int n1, int flags, int i, int j) {
    const int ea = s.f0 + ((flags >> 1) & 1), eb = s.f1 + ((flags >> 2) & 1), es = s.f1 + 1;
    double acc = 0.0;
    for (int a = 0; a < ea; ++a) {
        const double* row = x + (size_t)(n0 + s.f0 * i + a) * s.W + (n1 + s.f1 * j);
        for (int b = 0; b < eb; ++b) acc += kek[a * es + b] * row[b];
    }
    return acc;
}

// sum_k (A_k^T r_k)[mi][mj]: r [K][h][w] of one image, geo [K][4], ke [K][(f0 + 1)(f1 + 1)]
__device__ __forceinline__ double mf_gather(const double* r, const int* geo, const double* ke, const MfShape& s, int mi, int mj) {
    const int es = s.f1 + 1, ke_size = (s.f0 + 1) * es;
    const size_t hw = (size_t)s.h * s.w;
    double g = 0.0;
    for (int k = 0; k < s.K; ++k) {
        const int n0 = geo[4 * k], n1 = geo[4 * k + 1], flags = geo[4 * k + 2];
        if (!(flags & 1)) continue;
        const int ea = s.f0 + ((flags >> 1) & 1), eb = s.f1 + ((flags >> 2) & 1);
        const int ih = tv_floordiv(mi - n0, s.f0), ah = mi - n0 - ih * s.f0;   // the last LR row that reaches mi, 0 <= ah < f0
        const int jh = tv_floordiv(mj - n1, s.f1), bh = mj - n1 - jh * s.f1;
        const double* kek = ke + (size_t)k * ke_size;
        const double* rk = r + (size_t)k * hw;
        for (int di = ah + s.f0 < ea ? -1 : 0; di <= 0; ++di) {               // the row before reaches mi with its extra tap row only
            const int i = ih + di, a = ah - di * s.f0;
            if (i < 0 || i >= s.h || !mf_inside(n0, ea, s.f0, i, s.H)) continue;
            for (int dj = bh + s.f1 < eb ? -1 : 0; dj <= 0; ++dj) {
                const int j = jh + dj, b = bh - dj * s.f1;
                if (j < 0 || j >= s.w || !mf_inside(n1, eb, s.f1, j, s.W)) continue;
                g += kek[a * es + b] * rk[(size_t)i * s.w + j];
            }
        }
    }
    return g;
}

// the workspace: the state x | xbar | p0 | p1 of every image, q [n][K][h][w], the table ke [n][K][(f0 + 1)(f1 + 1)] and geo [n][K][4],
// tau [n], and the partials [n][parts] of energy, change and the count of valid data.  base == null: `total` only
struct MfView {
    double *state, *q, *ke, *tau, *epart, *chpart, *vpart;
    int* geo;
    size_t total;
};
MfView mf_view(int n, const MfShape& s, void* base) {
    MfView v;
    WsCarver c(base, 16);
    const size_t nn = (size_t)(n > 0 ? n : 1), HW = (size_t)s.H * s.W, hw = (size_t)s.h * s.w;
    v.state = c.take<double>(nn * 4 * HW);
    v.q = c.take<double>(nn * s.K * hw);
    v.ke = c.take<double>(nn * s.K * (size_t)((s.f0 + 1) * (s.f1 + 1)));
    v.tau = c.take<double>(nn);
    v.epart = c.take<double>(nn * s.parts);
    v.chpart = c.take<double>(nn * s.parts);
    v.vpart = c.take<double>(nn * s.parts);
    v.geo = c.take<int>(nn * s.K * 4);
    v.total = c.bytes();
    return v;
}

template <typename T>
__global__ void __launch_bounds__(MF_THREADS) mf_init_kernel(MfView v, const T* y, const T* x0, const double* shifts, long long n, MfShape s,
                                                             TvBlock kb) {
    __shared__ double ks[MF_MAX_FACTOR * MF_MAX_FACTOR];
    if ((int)threadIdx.x < s.f0 * s.f1) ks[threadIdx.x] = kb.k[threadIdx.x];
    __syncthreads();
    const long long HW = (long long)s.H * s.W, hw = (long long)s.h * s.w, Khw = s.K * hw;
    const int es = s.f1 + 1, ke_size = (s.f0 + 1) * es;
    const long long n_pix = n * HW, n_dat = n * Khw, n_tab = n * s.K * ke_size, total = n_pix + n_dat + n_tab + n;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        if (t < n_pix) {
            const long long img = t / HW;
            const int e = (int)(t - img * HW), i = e / s.W, j = e - i * s.W;
            const double val = x0 ? (double)x0[t] : (double)y[img * Khw + (long long)(i / s.f0) * s.w + j / s.f1];   // frame 0
            double* x = v.state + img * 4 * HW;
            x[e] = val;
            x[HW + e] = val;
            x[2 * HW + e] = 0.0;
            x[3 * HW + e] = 0.0;
        } else if (t < n_pix + n_dat) {
            v.q[t - n_pix] = 0.0;
        } else if (t < n_pix + n_dat + n_tab) {
            const long long u = t - n_pix - n_dat, frame = u / ke_size;
            const int idx = (int)(u - frame * ke_size), a = idx / es, b = idx - a * es;
            const MfGeo g = mf_geo(shifts + 2 * frame);
            v.ke[u] = mf_ke(ks, s.f0, s.f1, g, a, b);
            if (idx == 0) {
                int* geo = v.geo + 4 * frame;
                geo[0] = g.n0;
                geo[1] = g.n1;
                geo[2] = g.flags;
                geo[3] = 0;
            }
        } else {
            const long long img = t - n_pix - n_dat - n_tab;
            int live = 0;
            for (int k = 0; k < s.K; ++k) live += mf_frame_live(mf_geo(shifts + 2 * (img * s.K + k)), s) ? 1 : 0;
            v.tau[img] = 1.0 / sqrt(8.0 + (double)live * kb.c);
        }
    }
}

// threads begin .. n H W - 1 are HR pixels (begin = n H W where lambda = 0), the rest LR data
template <typename T>
__global__ void __launch_bounds__(MF_THREADS) mf_dual_kernel(MfView v, const T* y, const T* weight, long long n, MfShape s, double lam,
                                                             double alpha, long long begin) {
    const long long HW = (long long)s.H * s.W, hw = (long long)s.h * s.w, Khw = s.K * hw;
    const int ke_size = (s.f0 + 1) * (s.f1 + 1);
    const long long n_pix = n * HW, total = n_pix + n * Khw;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = begin + (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        if (t < n_pix) {
            const long long img = t / HW;
            const int e = (int)(t - img * HW), i = e / s.W, j = e - i * s.W;
            const double sigma = v.tau[img], den = 1.0 + sigma * alpha / lam;
            const double* xbar = v.state + img * 4 * HW + HW;
            double* p0 = v.state + img * 4 * HW + 2 * HW;
            double* p1 = p0 + HW;
            const double xb = xbar[e];
            const double g0 = i + 1 < s.H ? xbar[e + s.W] - xb : 0.0;
            const double g1 = j + 1 < s.W ? xbar[e + 1] - xb : 0.0;
            double q0 = (p0[e] + sigma * g0) / den;
            double q1 = (p1[e] + sigma * g1) / den;
            const double nrm = sqrt(q0 * q0 + q1 * q1) / lam;
            if (nrm > 1.0) {
                q0 /= nrm;
                q1 /= nrm;
            }
            p0[e] = q0;
            p1[e] = q1;
        } else {
            const long long u = t - n_pix, img = u / Khw, frame = u / hw;
            const int l = (int)(u - frame * hw), i = l / s.w, j = l - i * s.w;
            const int* geo = v.geo + 4 * frame;
            const int n0 = geo[0], n1 = geo[1], flags = geo[2];
            double qn = 0.0;
            if (mf_valid(s, n0, n1, flags, i, j)) {
                const double wv = weight ? (double)weight[u] : 1.0;
                if (wv > 0.0) {
                    const double sigma = v.tau[img];
                    const double ax = mf_apply(v.state + img * 4 * HW + HW, v.ke + frame * ke_size, s, n0, n1, flags, i, j);
                    qn = (v.q[u] + sigma * (ax - (double)y[u])) / (1.0 + sigma / wv);
                }
            }
            v.q[u] = qn;
        }
    }
}

__global__ void __launch_bounds__(MF_THREADS) mf_primal_kernel(MfView v, long long n, MfShape s, int last) {
    const long long HW = (long long)s.H * s.W, Khw = (long long)s.K * s.h * s.w, total = n * HW;
    const int ke_size = (s.f0 + 1) * (s.f1 + 1);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const long long img = t / HW;
        const int e = (int)(t - img * HW), i = e / s.W, j = e - i * s.W;
        double* x = v.state + img * 4 * HW;
        double* xbar = x + HW;
        const double* p0 = xbar + HW;
        const double* p1 = p0 + HW;
        const double g = mf_gather(v.q + img * Khw, v.geo + img * s.K * 4, v.ke + img * s.K * ke_size, s, i, j);
        double d = 0.0;
        if (i + 1 < s.H) d += p0[e];
        if (i > 0) d -= p0[e - s.W];
        if (j + 1 < s.W) d += p1[e];
        if (j > 0) d -= p1[e - 1];
        const double xo = x[e];
        const double xn = xo - v.tau[img] * (g - d);
        xbar[e] = last ? xn - xo : 2.0 * xn - xo;
        x[e] = xn;
    }
}

// element u of an image: an HR pixel below H W (its prior term, its change, the result), a datum above (its data term)
template <typename T>
__global__ void __launch_bounds__(MF_THREADS) mf_final_kernel(T* out, MfView v, const T* y, const T* weight, long long n, MfShape s, double lam,
                                                              double alpha, int n_iter) {
    __shared__ double red[MF_THREADS / 64];
    const int tid = threadIdx.x;
    const long long HW = (long long)s.H * s.W, hw = (long long)s.h * s.w, Khw = s.K * hw;
    const int ke_size = (s.f0 + 1) * (s.f1 + 1);
    for (long long item = blockIdx.x; item < n * s.parts; item += gridDim.x) {
        const long long img = item / s.parts;
        const int part = (int)(item - img * s.parts);
        const double* x = v.state + img * 4 * HW;
        const double* diff = x + HW;   // x' - x of the last iteration
        double en = 0.0, reg = 0.0, ch = 0.0, cnt = 0.0;
        for (int r = 0; r < MF_PART / MF_THREADS; ++r) {
            const long long u = (long long)part * MF_PART + r * MF_THREADS + tid;
            if (u < HW) {
                const int e = (int)u, i = e / s.W, j = e - i * s.W;
                const double xe = x[e];
                out[img * HW + e] = (T)xe;
                if (lam > 0.0) {
                    const double g0 = i + 1 < s.H ? x[e + s.W] - xe : 0.0;
                    const double g1 = j + 1 < s.W ? x[e + 1] - xe : 0.0;
                    reg += tv_huber(sqrt(g0 * g0 + g1 * g1), alpha);
                }
                if (n_iter > 0) ch = fmax(ch, fabs(diff[e]));
            } else if (u < HW + Khw) {
                const long long d = img * Khw + (u - HW), frame = d / hw;
                const int l = (int)(d - frame * hw), i = l / s.w, j = l - i * s.w;
                const int* geo = v.geo + 4 * frame;
                const int n0 = geo[0], n1 = geo[1], flags = geo[2];
                if (mf_valid(s, n0, n1, flags, i, j)) {
                    cnt += 1.0;
                    const double wv = weight ? (double)weight[d] : 1.0;
                    if (wv > 0.0) {
                        const double res = mf_apply(x, v.ke + frame * ke_size, s, n0, n1, flags, i, j) - (double)y[d];
                        en += 0.5 * wv * res * res;
                    }
                }
            }
        }
        if (lam > 0.0) en += lam * reg;
        en = block_sum_f64(en, red);
        cnt = block_sum_f64(cnt, red);
        ch = block_max_f64(ch, red);   // ends with a barrier: red is free for the next item
        if (tid == 0) {
            v.epart[item] = en;
            v.vpart[item] = cnt;
            v.chpart[item] = ch;
        }
    }
}

// out [n][K][h][w] = (A_k in [n][H][W])_k, 0 at an invalid datum; valid [n][K][h][w] bytes or null.  One workgroup per frame forms the
// frame's ke in LDS
__global__ void __launch_bounds__(MF_THREADS) mf_apply_kernel(double* __restrict__ out, unsigned char* __restrict__ valid,
                                                              const double* __restrict__ in, const double* __restrict__ shifts, long long n,
                                                              MfShape s, TvBlock kb) {
    __shared__ double ks[MF_MAX_FACTOR * MF_MAX_FACTOR];
    __shared__ double kes[MF_KE_MAX];
    const int tid = threadIdx.x;
    if (tid < s.f0 * s.f1) ks[tid] = kb.k[tid];
    __syncthreads();
    const long long HW = (long long)s.H * s.W, hw = (long long)s.h * s.w;
    const int es = s.f1 + 1, ke_size = (s.f0 + 1) * es;
    for (long long frame = blockIdx.x; frame < n * s.K; frame += gridDim.x) {
        const MfGeo g = mf_geo(shifts + 2 * frame);
        if (tid < ke_size) kes[tid] = mf_ke(ks, s.f0, s.f1, g, tid / es, tid % es);
        __syncthreads();
        const double* x = in + (frame / s.K) * HW;
        for (long long l = tid; l < hw; l += MF_THREADS) {
            const int i = (int)(l / s.w), j = (int)(l - (long long)i * s.w);
            const bool ok = mf_valid(s, g.n0, g.n1, g.flags, i, j);
            out[frame * hw + l] = ok ? mf_apply(x, kes, s, g.n0, g.n1, g.flags, i, j) : 0.0;
            if (valid) valid[frame * hw + l] = ok ? 1 : 0;
        }
        __syncthreads();   // kes is free for the next frame
    }
}

// out [n][H][W] = sum_k A_k^T in [n][K][h][w]: one workgroup per 256 HR pixels of an image forms the image's table in LDS
__global__ void __launch_bounds__(MF_THREADS) mf_adjoint_kernel(double* __restrict__ out, const double* __restrict__ in,
                                                                const double* __restrict__ shifts, long long n, MfShape s, TvBlock kb,
                                                                int chunks) {
    __shared__ double ks[MF_MAX_FACTOR * MF_MAX_FACTOR];
    __shared__ double kes[MF_MAX_FRAMES * MF_KE_MAX];
    __shared__ int geos[MF_MAX_FRAMES * 4];
    const int tid = threadIdx.x;
    if (tid < s.f0 * s.f1) ks[tid] = kb.k[tid];
    __syncthreads();
    const long long HW = (long long)s.H * s.W, Khw = (long long)s.K * s.h * s.w;
    const int es = s.f1 + 1, ke_size = (s.f0 + 1) * es;
    for (long long item = blockIdx.x; item < n * chunks; item += gridDim.x) {
        const long long img = item / chunks;
        const int chunk = (int)(item - img * chunks);
        for (int t = tid; t < s.K * ke_size; t += MF_THREADS) {
            const int k = t / ke_size, idx = t - k * ke_size;
            const MfGeo g = mf_geo(shifts + 2 * (img * s.K + k));
            kes[t] = mf_ke(ks, s.f0, s.f1, g, idx / es, idx % es);
            if (idx == 0) {
                geos[4 * k] = g.n0;
                geos[4 * k + 1] = g.n1;
                geos[4 * k + 2] = g.flags;
                geos[4 * k + 3] = 0;
            }
        }
        __syncthreads();
        const long long e = (long long)chunk * MF_THREADS + tid;
        if (e < HW) out[img * HW + e] = mf_gather(in + img * Khw, geos, kes, s, (int)(e / s.W), (int)(e % s.W));
        __syncthreads();   // the table is free for the next item
    }
}

int mf_shape_check(const char* who, int n, int K, int H, int W, int f0, int f1, MfShape* s) {
    // n_images, then the frame count, then tv_block.h's refusals of the factors and the sizes: the order callers have always seen
    INR_REQUIRE(n >= 0, INR_E_INVALID, "%s: bad sizes (n_images = %d)", who, n);
    INR_REQUIRE(K >= 1 && K <= MF_MAX_FRAMES, INR_E_INVALID, "%s: frames per image are 1 .. %d (got %d)", who, MF_MAX_FRAMES, K);
    TvShape b;
    if (int rc = tv_shape_check(who, n, H, W, f0, f1, &b)) return rc;
    MfShape v{H, W, b.h, b.w, f0, f1, K, 0};
    v.parts = (int)(((long long)H * W + (long long)K * v.h * v.w + MF_PART - 1) / MF_PART);   // <= 65 * 2^20 / 1,024
    *s = v;
    return 0;
}

template <typename T>
int mf_solve(const char* who, T* out, double* energy, double* change, double* valid_fraction, const T* y, const double* shifts,
             const T* weight, const T* x0, int n, int K, int H, int W, int f0, int f1, const double* kernel, double lam, double alpha,
             int n_iter, double* workspace, int64_t workspace_doubles, hipStream_t st) {
    INR_REQUIRE(out && y, INR_E_INVALID, "%s: null pointer", who);
    INR_REQUIRE(shifts, INR_E_INVALID, "%s: null pointer (shifts)", who);
    MfShape s;
    TvBlock kb;
    if (int rc = mf_shape_check(who, n, K, H, W, f0, f1, &s)) return rc;
    if (int rc = tv_params_check(who, lam, alpha, n_iter, INR_TVSR3D_MAX_ITER)) return rc;
    if (int rc = tv_block_check(who, kernel, f0, f1, &kb)) return rc;
    if (int rc = check_ws_doubles(who, workspace, workspace_doubles, mf_view(n, s, nullptr).total)) return rc;
    if (n == 0) return 0;
    const MfView v = mf_view(n, s, workspace);
    const long long pixels = (long long)n * H * W, data = (long long)n * K * s.h * s.w;
    const long long table = (long long)n * K * (f0 + 1) * (f1 + 1), items = (long long)n * s.parts;
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL((mf_init_kernel<T>), dim3(tv_thread_grid(pixels + data + table + n, MF_THREADS)), dim3(MF_THREADS), 0, st, v, y, x0, shifts,
                       (long long)n, s, kb);
    INR_LAUNCH_CHECK();
    const long long begin = lam > 0.0 ? 0 : pixels;
    for (int it = 0; it < n_iter; ++it) {
        hipLaunchKernelGGL((mf_dual_kernel<T>), dim3(tv_thread_grid(pixels + data - begin, MF_THREADS)), dim3(MF_THREADS), 0, st, v, y, weight,
                           (long long)n, s, lam, alpha, begin);
        INR_LAUNCH_CHECK();
        hipLaunchKernelGGL(mf_primal_kernel, dim3(tv_thread_grid(pixels, MF_THREADS)), dim3(MF_THREADS), 0, st, v, (long long)n, s,
                           (int)(it + 1 == n_iter));
        INR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((mf_final_kernel<T>), dim3(tv_grid(items)), dim3(MF_THREADS), 0, st, out, v, y, weight, (long long)n, s, lam, alpha,
                       n_iter);
    INR_LAUNCH_CHECK();
    return tv_finish<MF_THREADS>(energy, change, valid_fraction, v.epart, s.parts, v.chpart, s.parts, v.vpart, (double)s.K * s.h * s.w, n, st);
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_tvmf_workspace_doubles(int n_images, int n_frames, int height, int width, int f0, int f1) {
    MfShape s;
    if (mf_shape_check("inr_tvmf_workspace_doubles", n_images, n_frames, height, width, f0, f1, &s)) return 0;
    return (int64_t)((mf_view(n_images, s, nullptr).total + sizeof(double) - 1) / sizeof(double));
}

int inr_tvmf_solve2d(double* out, double* energy, double* change, double* valid_fraction, const double* y, const double* shifts,
                     const double* weight, const double* x0, int n_images, int n_frames, int height, int width, int f0, int f1,
                     const double* kernel, double lambda, double alpha, int n_iter, double* workspace, int64_t workspace_doubles,
                     void* stream) {
    return mf_solve("inr_tvmf_solve2d", out, energy, change, valid_fraction, y, shifts, weight, x0, n_images, n_frames, height, width, f0,
                    f1, kernel, lambda, alpha, n_iter, workspace, workspace_doubles, (hipStream_t)stream);
}

int inr_tvmf_solve2d_f32(float* out, double* energy, double* change, double* valid_fraction, const float* y, const double* shifts,
                         const float* weight, const float* x0, int n_images, int n_frames, int height, int width, int f0, int f1,
                         const double* kernel, double lambda, double alpha, int n_iter, double* workspace, int64_t workspace_doubles,
                         void* stream) {
    return mf_solve("inr_tvmf_solve2d_f32", out, energy, change, valid_fraction, y, shifts, weight, x0, n_images, n_frames, height, width,
                    f0, f1, kernel, lambda, alpha, n_iter, workspace, workspace_doubles, (hipStream_t)stream);
}

int inr_frame_apply2d(double* out, unsigned char* valid, const double* in, const double* shifts, int n_images, int n_frames, int height,
                      int width, int f0, int f1, const double* kernel, void* stream) {
    INR_REQUIRE(out && in, INR_E_INVALID, "inr_frame_apply2d: null pointer");
    INR_REQUIRE(shifts, INR_E_INVALID, "inr_frame_apply2d: null pointer (shifts)");
    MfShape s;
    TvBlock kb;
    if (int rc = mf_shape_check("inr_frame_apply2d", n_images, n_frames, height, width, f0, f1, &s)) return rc;
    if (int rc = tv_block_check("inr_frame_apply2d", kernel, f0, f1, &kb)) return rc;
    if (n_images == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL(mf_apply_kernel, dim3(tv_grid((long long)n_images * n_frames)), dim3(MF_THREADS), 0, st, out, valid, in, shifts,
                       (long long)n_images, s, kb);
    INR_LAUNCH_CHECK();
    return 0;
}

int inr_frame_adjoint2d(double* out, const double* in, const double* shifts, int n_images, int n_frames, int height, int width, int f0,
                        int f1, const double* kernel, void* stream) {
    INR_REQUIRE(out && in, INR_E_INVALID, "inr_frame_adjoint2d: null pointer");
    INR_REQUIRE(shifts, INR_E_INVALID, "inr_frame_adjoint2d: null pointer (shifts)");
    MfShape s;
    TvBlock kb;
    if (int rc = mf_shape_check("inr_frame_adjoint2d", n_images, n_frames, height, width, f0, f1, &s)) return rc;
    if (int rc = tv_block_check("inr_frame_adjoint2d", kernel, f0, f1, &kb)) return rc;
    if (n_images == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(KC_OTHER, st);
    const int chunks = (height * width + MF_THREADS - 1) / MF_THREADS;
    hipLaunchKernelGGL(mf_adjoint_kernel, dim3(tv_grid((long long)n_images * chunks)), dim3(MF_THREADS), 0, st, out, in, shifts,
                       (long long)n_images, s, kb, chunks);
    INR_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
