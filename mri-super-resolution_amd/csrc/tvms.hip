// Multi-stack 3-D TV / Huber reconstruction with general slice profiles: S stacks of thick slices of one volume -- any orientation,
// overlapping or gapped profiles, whole-voxel offsets -- and the 3-D prior of tvsr3d.hip:
//   x* = argmin_x 1/2 sum_s sum_i w_si ((A_s x)_i - y_si)^2 + lambda sum_j H_alpha(sqrt((g1 d1 x)_j^2 + (g2 d2 x)_j^2 + (g0 d0 x)_j^2))
// The volume is HR [n][D][H][W] (slice, row, column).  Stack s has per axis a spacing f_a (1 .. 8), a tap count L_a (1 .. 16), an offset
// o_a (|o_a| <= 2^20 HR voxels, may be negative), an extent n_a (1 .. 2048) and taps k_a [L_a] summing to 1:
//   (A_s x)[l][i][j] = sum_{a, b, c} k[a][b][c] x[o_0 + f_0 l + a][o_1 + f_1 i + b][o_2 + f_2 j + c],  k[a][b][c] = (k_1[b] * k_2[c]) * k_0[a],
// the terms added in ascending (a, b, c): the table and the order of tvsr3d.hip, so a stack with L = f, o = 0, n = N / f is its block
// operator bit for bit (the unit is compiled with -ffp-contract=off, _build.py).  The product is formed where it is used: tables of
// 8 x 16^3 doubles fit neither the kernel arguments nor LDS.  The data y, weight and the dual q are [n][M], M = sum_s n_0 n_1 n_2, the
// stacks in order.  A datum is VALID when its footprint lies inside the volume on every axis, 0 <= o + f i and o + f i + L <= N; the HOST
// turns that into one index range lo .. hi per stack and axis (ms_stack_ranges), and every kernel tests lo <= i <= hi BEFORE it forms an
// address.  An invalid datum has weight 0 whatever `weight` holds, its y and weight are never read and its dual variable is 0.  With
// |o| <= 2^20, f <= 8, i < 2048 and L <= 16 every o + f i + L fits an int.  The adjoint is a gather: HR voxel m sums k[a][b][c] r[l][i][j]
// over the valid data whose footprint holds m -- stacks ascending, then l, i, j ascending, per axis the indices
// floordiv(m - o - L + 1 + f - 1, f) .. floordiv(m - o, f) cut to lo .. hi, at most ceil(L / f) of them.  No atomics anywhere.
//
// Chambolle-Pock with BOTH terms dual, from x = xbar = x0, p = 0, q = 0:
//   p    <- (p + sigma g d(xbar)) / (1 + sigma alpha / lambda);  p <- p / max(1, |p| / lambda)     (prior off: p = 0)
//   q_s  <- (q_s + sigma (A_s xbar - y_s)) / (1 + sigma / w_s)    for valid data with w_s > 0, else 0
//   x'   <- x - tau (sum_s A_s^T q_s - div p);  xbar <- 2 x' - x;  x <- x'
// with the differences, the gradient weights, the combining order (row, column, then slice) and the "axes longer than 1" rule of
// tvsr3d.hip.  tau = sigma = 1 / sqrt(4 sum_a g_a^2 + sum_{s live} c_s), formed on the HOST in fp64 (the geometry is the host's): the
// first sum over the axes longer than 1 in the order (1, 2, 0); c_s = prod_a (sum_t |k_a[t]|) (max_{r < f_a} sum_{t = r mod f_a} |k_a[t]|)
// bounds |A_s|^2 by |A_s|_1 |A_s|_inf (A_s is a Kronecker product of three banded matrices whose row sums are sum |k_a| and whose
// column sums are the residue-class sums); a stack is LIVE when it holds a valid datum.  The default x0 is the normalised
// back-projection (sum_s A_s^T y_s) / (sum_s A_s^T 1) over the usable data -- valid and w > 0 --, 0 where no usable datum reaches.
//
// LAUNCHES.  Plain launches on the caller's stream: no cooperative launch, no grid barrier, no spin, no host read.
//   init    (thread per element):     writes its own x, xbar (from x0, where given), p0, p1, p2 (per HR voxel) and q (per datum);
//   backproject (thread per HR voxel, only without x0): gathers y and weight -- the caller's, read-only --, writes its own x, xbar;
//   dual    (thread per HR voxel e AND per datum): a voxel thread (none where the prior is off) reads xbar[e], xbar[e + W], xbar[e + 1],
//                                     xbar[e + HW] -- neighbours' --, reads and writes p0[e], p1[e], p2[e] -- its own; a datum thread
//                                     reads xbar over its footprint -- others' --, reads and writes its own q;
//   primal  (thread per HR voxel e):  gathers q of every stack and p at e, e - W, e - 1, e - HW -- others' --, reads and writes x[e],
//                                     xbar[e] -- its own (the last iteration leaves x' - x in xbar, which nothing differences again);
//   final   (workgroup per part):     reads x across threads, writes the result and the partials of energy, change and the count of
//                                     valid data; finish: one workgroup per volume reduces the partials in a fixed order.
// Within a launch a field is either read across threads or written by its owner alone: xbar is read-only in the dual kernel and
// owner-written in the primal one, p and q are owner-written in the dual kernel and read-only in the primal one, x is touched by its
// own thread only.  STREAM ORDER IS THE BARRIER between launches.  The stack table (geometry, ranges, taps) travels by value in the
// kernel arguments and every workgroup copies it to LDS before use.
//
// Consecutive datum threads take consecutive j, the fastest LR index, so the reads of xbar are contiguous whenever f_2 = 1.  A
// volume's HR voxels followed by its M data are cut into "parts" of MS_PART elements; the partials are per PART, and thread t of the
// finish adds partials t, t + 256, ... in ascending order, so the bits of energy and change depend on the shape alone: not on the
// grid (capped at TV_STRIDE_MAX_GRID, or by the test-only inr_debug_set(32, .)), the stream, or the place in a batch.  All arithmetic is
// fp64; the fp32 entry converts at load and rounds once at the store.
//
// The Huber function, the floor division, the grids, the refusals of the scalar parameters and the gradient weights, the step setup
// of the prior and the finish kernel are tv_shared.h's.
#include "tv_shared.h"

namespace inr {
namespace {

constexpr int MS_THREADS = 256;
constexpr int MS_MAX_STACKS = INR_TVMS_MAX_STACKS;
constexpr int MS_MAX_TAPS = INR_TVMS_MAX_TAPS;
constexpr int MS_MAX_FACTOR = INR_TVSR_MAX_FACTOR;
constexpr int MS_MAX_SIDE = INR_TVSR_MAX_SIDE;
constexpr int MS_MAX_EXTENT = 2048;
constexpr int MS_MAX_OFFSET = 1 << 20;
constexpr int MS_PART = 4 * MS_THREADS;   // elements of a part: four per thread

// one stack: the caller's geometry, the valid index range lo .. hi per axis (empty: hi < lo; lo is cut to n and hi to -1, which keeps
// an empty range empty and both within a short) and whether all three hold an index.  Packed: the table travels in kernel arguments
struct MsStack {
    long long base;   // of the stack's data within a row of M
    int o[3];
    short n[3], lo[3], hi[3];
    unsigned char f[3], L[3];
    unsigned char live, pad;
};

// the stacks of one call, by value in the kernel arguments (3.4 KiB); workgroups keep their copy of it in LDS
struct MsTable {
    MsStack g[MS_MAX_STACKS];
    double k[MS_MAX_STACKS][3][MS_MAX_TAPS];
};
typedef MsTable MsLds;
static_assert(sizeof(MsTable) <= 3584, "the stack table must leave room for the other kernel arguments");

struct MsShape {
    int D, H, W, S;
    long long M;       // data per volume
    long long parts;   // per volume: ceil((D H W + M) / MS_PART)
};

struct MsStep {
    double g0, g1, g2, tau, lam, alpha;   // lam: 0 where the prior is off
};

// the table in LDS: every thread of the workgroup calls this before its first use
__device__ __forceinline__ void ms_stage(MsLds* lds, const MsTable& tab, int S) {
    for (int t = threadIdx.x; t < S * 3 * MS_MAX_TAPS; t += blockDim.x) (&lds->k[0][0][0])[t] = (&tab.k[0][0][0])[t];
    for (int t = threadIdx.x; t < S; t += blockDim.x) lds->g[t] = tab.g[t];
    __syncthreads();
}

// datum u of a volume's row of M -> its stack and LR indices
struct MsDatum {
    int s, l, i, j;
};
__device__ __forceinline__ MsDatum ms_datum(const MsLds* t, int S, long long u) {
    MsDatum d;
    d.s = 0;
    for (int s = 1; s < S; ++s)
        if (u >= t->g[s].base) d.s = s;
    const MsStack& g = t->g[d.s];
    const long long local = u - g.base, plane = (long long)g.n[1] * g.n[2];
    d.l = (int)(local / plane);
    const int r = (int)(local - d.l * plane);
    d.i = r / g.n[2];
    d.j = r - d.i * g.n[2];
    return d;
}

__device__ __forceinline__ bool ms_valid(const MsStack& g, const MsDatum& d) {
    return d.l >= g.lo[0] && d.l <= g.hi[0] && d.i >= g.lo[1] && d.i <= g.hi[1] && d.j >= g.lo[2] && d.j <= g.hi[2];
}

// (A_s x) of a VALID datum; x one volume
__device__ __forceinline__ double ms_apply(const double* x, const MsLds* t, const MsShape& sh, const MsDatum& d) {
    const MsStack& g = t->g[d.s];
    const double *k0 = t->k[d.s][0], *k1 = t->k[d.s][1], *k2 = t->k[d.s][2];
    const int z0 = g.o[0] + g.f[0] * d.l, i0 = g.o[1] + g.f[1] * d.i, j0 = g.o[2] + g.f[2] * d.j;
    double acc = 0.0;
    for (int a = 0; a < g.L[0]; ++a)
        for (int b = 0; b < g.L[1]; ++b) {
            const double* row = x + ((long long)(z0 + a) * sh.H + (i0 + b)) * sh.W + j0;
            for (int c = 0; c < g.L[2]; ++c) acc += ((k1[b] * k2[c]) * k0[a]) * row[c];
        }
    return acc;
}

// the LR indices of axis a whose footprint holds HR coordinate m, cut to the valid ones
__device__ __forceinline__ void ms_reach(const MsStack& g, int a, int m, int* first, int* last) {
    const int u = m - g.o[a], f = g.f[a], L = g.L[a];
    *first = max(tv_floordiv(u - L + 1 + f - 1, f), (int)g.lo[a]);
    *last = min(tv_floordiv(u, f), (int)g.hi[a]);
}

// sum_s (A_s^T r_s) at HR voxel (z, i, j): val(u) is r at datum u of the volume's row
template <typename F>
__device__ __forceinline__ double ms_gather(const MsLds* t, int S, int z, int i, int j, F val) {
    double acc = 0.0;
    for (int s = 0; s < S; ++s) {
        const MsStack& g = t->g[s];
        if (!g.live) continue;
        int l0, l1, i0, i1, j0, j1;
        ms_reach(g, 0, z, &l0, &l1);
        ms_reach(g, 1, i, &i0, &i1);
        ms_reach(g, 2, j, &j0, &j1);
        const double *k0 = t->k[s][0], *k1 = t->k[s][1], *k2 = t->k[s][2];
        for (int l = l0; l <= l1; ++l) {
            const int a = z - g.o[0] - g.f[0] * l;
            for (int ii = i0; ii <= i1; ++ii) {
                const int b = i - g.o[1] - g.f[1] * ii;
                for (int jj = j0; jj <= j1; ++jj) {
                    const int c = j - g.o[2] - g.f[2] * jj;
                    acc += ((k1[b] * k2[c]) * k0[a]) * val(g.base + ((long long)l * g.n[1] + ii) * g.n[2] + jj);
                }
            }
        }
    }
    return acc;
}

// the workspace: the state x | xbar | p0 | p1 | p2 of every volume, q [n][M], and the partials [n][parts] of energy, change and the
// count of valid data.  base == null: `total` only
struct MsView {
    double *state, *q, *epart, *chpart, *vpart;
    size_t total;
};
MsView ms_view(int n, const MsShape& s, void* base) {
    MsView v;
    WsCarver c(base, 16);
    const size_t nn = (size_t)(n > 0 ? n : 1), DHW = (size_t)s.D * s.H * s.W;
    v.state = c.take<double>(nn * 5 * DHW);
    v.q = c.take<double>(nn * (size_t)s.M);
    v.epart = c.take<double>(nn * (size_t)s.parts);
    v.chpart = c.take<double>(nn * (size_t)s.parts);
    v.vpart = c.take<double>(nn * (size_t)s.parts);
    v.total = c.bytes();
    return v;
}

// voxel e of a volume -> (z, i, j)
__device__ __forceinline__ void ms_voxel(const MsShape& s, int e, int* z, int* i, int* j) {
    const int HW = s.H * s.W;
    *z = e / HW;
    const int r = e - *z * HW;
    *i = r / s.W;
    *j = r - *i * s.W;
}

template <typename T>
__global__ void __launch_bounds__(MS_THREADS) ms_init_kernel(MsView v, const T* x0, long long n, MsShape s) {
    const long long DHW = (long long)s.D * s.H * s.W, n_vox = n * DHW, total = n_vox + n * s.M;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        if (t < n_vox) {
            const long long img = t / DHW, e = t - img * DHW;
            double* x = v.state + img * 5 * DHW;
            if (x0) {
                const double val = (double)x0[t];
                x[e] = val;
                x[DHW + e] = val;
            }
            x[2 * DHW + e] = 0.0;
            x[3 * DHW + e] = 0.0;
            x[4 * DHW + e] = 0.0;
        } else {
            v.q[t - n_vox] = 0.0;
        }
    }
}

// x = xbar = (sum_s A_s^T y_s) / (sum_s A_s^T 1) over the usable data, 0 where the denominator is not > 0
template <typename T>
__global__ void __launch_bounds__(MS_THREADS) ms_backproject_kernel(MsView v, const T* y, const T* weight, long long n, MsShape s,
                                                                    MsTable tab) {
    __shared__ MsLds lds;
    ms_stage(&lds, tab, s.S);
    const long long DHW = (long long)s.D * s.H * s.W, total = n * DHW;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const long long img = t / DHW;
        const int e = (int)(t - img * DHW);
        int z, i, j;
        ms_voxel(s, e, &z, &i, &j);
        const T* yi = y + img * s.M;
        const T* wi = weight ? weight + img * s.M : nullptr;
        const double num = ms_gather(&lds, s.S, z, i, j, [&](long long u) { return !wi || (double)wi[u] > 0.0 ? (double)yi[u] : 0.0; });
        const double den = ms_gather(&lds, s.S, z, i, j, [&](long long u) { return !wi || (double)wi[u] > 0.0 ? 1.0 : 0.0; });
        const double val = den > 0.0 ? num / den : 0.0;
        double* x = v.state + img * 5 * DHW;
        x[e] = val;
        x[DHW + e] = val;
    }
}

// threads begin .. n D H W - 1 are HR voxels (begin = n D H W where the prior is off), the rest data
template <typename T>
__global__ void __launch_bounds__(MS_THREADS) ms_dual_kernel(MsView v, const T* y, const T* weight, long long n, MsShape s, MsTable tab,
                                                             MsStep c, long long begin) {
    __shared__ MsLds lds;
    ms_stage(&lds, tab, s.S);
    const long long HW = (long long)s.H * s.W, DHW = HW * s.D, n_vox = n * DHW, total = n_vox + n * s.M;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const double sigma = c.tau;
    for (long long t = begin + (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        if (t < n_vox) {
            const long long img = t / DHW;
            const int e = (int)(t - img * DHW);
            int z, i, j;
            ms_voxel(s, e, &z, &i, &j);
            const double den = 1.0 + sigma * c.alpha / c.lam;
            const double* xbar = v.state + img * 5 * DHW + DHW;
            double* p0 = v.state + img * 5 * DHW + 2 * DHW;
            double* p1 = p0 + DHW;
            double* p2 = p1 + DHW;
            const double xb = xbar[e];
            const double d1 = i + 1 < s.H ? xbar[e + s.W] - xb : 0.0;
            const double d2 = j + 1 < s.W ? xbar[e + 1] - xb : 0.0;
            const double d0 = z + 1 < s.D ? xbar[e + HW] - xb : 0.0;
            double q1 = (p1[e] + sigma * (c.g1 * d1)) / den;
            double q2 = (p2[e] + sigma * (c.g2 * d2)) / den;
            double q0 = (p0[e] + sigma * (c.g0 * d0)) / den;
            const double nrm = sqrt((q1 * q1 + q2 * q2) + q0 * q0) / c.lam;
            if (nrm > 1.0) {
                q1 /= nrm;
                q2 /= nrm;
                q0 /= nrm;
            }
            p1[e] = q1;
            p2[e] = q2;
            p0[e] = q0;
        } else {
            const long long ua = t - n_vox, img = ua / s.M, u = ua - img * s.M;
            const MsDatum d = ms_datum(&lds, s.S, u);
            double qn = 0.0;
            if (ms_valid(lds.g[d.s], d)) {
                const double wv = weight ? (double)weight[ua] : 1.0;
                if (wv > 0.0) {
                    const double ax = ms_apply(v.state + img * 5 * DHW + DHW, &lds, s, d);
                    qn = (v.q[ua] + sigma * (ax - (double)y[ua])) / (1.0 + sigma / wv);
                }
            }
            v.q[ua] = qn;
        }
    }
}

__global__ void __launch_bounds__(MS_THREADS) ms_primal_kernel(MsView v, long long n, MsShape s, MsTable tab, MsStep c, int last) {
    __shared__ MsLds lds;
    ms_stage(&lds, tab, s.S);
    const long long HW = (long long)s.H * s.W, DHW = HW * s.D, total = n * DHW;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const long long img = t / DHW;
        const int e = (int)(t - img * DHW);
        int z, i, j;
        ms_voxel(s, e, &z, &i, &j);
        double* x = v.state + img * 5 * DHW;
        double* xbar = x + DHW;
        const double* p0 = xbar + DHW;
        const double* p1 = p0 + DHW;
        const double* p2 = p1 + DHW;
        const double* q = v.q + img * s.M;
        const double g = ms_gather(&lds, s.S, z, i, j, [&](long long u) { return q[u]; });
        double dv = 0.0;
        if (c.lam > 0.0) {
            if (i + 1 < s.H) dv += c.g1 * p1[e];
            if (i > 0) dv -= c.g1 * p1[e - s.W];
            if (j + 1 < s.W) dv += c.g2 * p2[e];
            if (j > 0) dv -= c.g2 * p2[e - 1];
            if (z + 1 < s.D) dv += c.g0 * p0[e];
            if (z > 0) dv -= c.g0 * p0[e - HW];
        }
        const double xo = x[e];
        const double xn = xo - c.tau * (g - dv);
        xbar[e] = last ? xn - xo : 2.0 * xn - xo;
        x[e] = xn;
    }
}

// element u of a volume: an HR voxel below D H W (its prior term, its change, the result), a datum above (its data term)
template <typename T>
__global__ void __launch_bounds__(MS_THREADS) ms_final_kernel(T* out, MsView v, const T* y, const T* weight, long long n, MsShape s,
                                                              MsTable tab, MsStep c, int n_iter) {
    __shared__ MsLds lds;
    __shared__ double red[MS_THREADS / 64];
    ms_stage(&lds, tab, s.S);
    const int tid = threadIdx.x;
    const long long HW = (long long)s.H * s.W, DHW = HW * s.D;
    for (long long item = blockIdx.x; item < n * s.parts; item += gridDim.x) {
        const long long img = item / s.parts, part = item - img * s.parts;
        const double* x = v.state + img * 5 * DHW;
        const double* diff = x + DHW;   // x' - x of the last iteration
        double en = 0.0, reg = 0.0, ch = 0.0, cnt = 0.0;
        for (int r = 0; r < MS_PART / MS_THREADS; ++r) {
            const long long u = part * MS_PART + r * MS_THREADS + tid;
            if (u < DHW) {
                const int e = (int)u;
                int z, i, j;
                ms_voxel(s, e, &z, &i, &j);
                const double xe = x[e];
                out[img * DHW + e] = (T)xe;
                if (c.lam > 0.0) {
                    const double d1 = i + 1 < s.H ? x[e + s.W] - xe : 0.0;
                    const double d2 = j + 1 < s.W ? x[e + 1] - xe : 0.0;
                    const double d0 = z + 1 < s.D ? x[e + HW] - xe : 0.0;
                    const double t1 = c.g1 * d1, t2 = c.g2 * d2, t0 = c.g0 * d0;
                    reg += tv_huber(sqrt((t1 * t1 + t2 * t2) + t0 * t0), c.alpha);
                }
                if (n_iter > 0) ch = fmax(ch, fabs(diff[e]));
            } else if (u < DHW + s.M) {
                const long long du = u - DHW, ua = img * s.M + du;
                const MsDatum d = ms_datum(&lds, s.S, du);
                if (ms_valid(lds.g[d.s], d)) {
                    cnt += 1.0;
                    const double wv = weight ? (double)weight[ua] : 1.0;
                    if (wv > 0.0) {
                        const double res = ms_apply(x, &lds, s, d) - (double)y[ua];
                        en += 0.5 * wv * res * res;
                    }
                }
            }
        }
        if (c.lam > 0.0) en += c.lam * reg;
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

// out [n][M] = (A_s in [n][D][H][W])_s, 0 at an invalid datum; valid [n][M] bytes or null.  One thread per datum
__global__ void __launch_bounds__(MS_THREADS) ms_apply_kernel(double* __restrict__ out, unsigned char* __restrict__ valid,
                                                              const double* __restrict__ in, long long n, MsShape s, MsTable tab) {
    __shared__ MsLds lds;
    ms_stage(&lds, tab, s.S);
    const long long DHW = (long long)s.D * s.H * s.W, total = n * s.M;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const long long img = t / s.M;
        const MsDatum d = ms_datum(&lds, s.S, t - img * s.M);
        const bool ok = ms_valid(lds.g[d.s], d);
        out[t] = ok ? ms_apply(in + img * DHW, &lds, s, d) : 0.0;
        if (valid) valid[t] = ok ? 1 : 0;
    }
}

// out [n][D][H][W] = sum_s A_s^T in [n][M]: one thread per HR voxel
__global__ void __launch_bounds__(MS_THREADS) ms_adjoint_kernel(double* __restrict__ out, const double* __restrict__ in, long long n,
                                                                MsShape s, MsTable tab) {
    __shared__ MsLds lds;
    ms_stage(&lds, tab, s.S);
    const long long DHW = (long long)s.D * s.H * s.W, total = n * DHW;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const long long img = t / DHW;
        int z, i, j;
        ms_voxel(s, (int)(t - img * DHW), &z, &i, &j);
        const double* r = in + img * s.M;
        out[t] = ms_gather(&lds, s.S, z, i, j, [&](long long u) { return r[u]; });
    }
}

// the valid index range of every axis of a stack and its liveness: 0 <= o + f i and o + f i + L <= N, 0 <= i < n
void ms_stack_ranges(MsStack* g, const int N[3]) {
    g->live = 1;
    for (int a = 0; a < 3; ++a) {
        const int f = g->f[a], n = g->n[a];
        const int lo = g->o[a] >= 0 ? 0 : (-g->o[a] + f - 1) / f;
        const int top = tv_floordiv(N[a] - (int)g->L[a] - g->o[a], f);
        const int hi = top < n - 1 ? top : n - 1;
        g->lo[a] = (short)(lo < n ? lo : n);
        g->hi[a] = (short)(hi > -1 ? hi : -1);
        if (hi < lo) g->live = 0;
    }
}

// the sizes and the geometry [S][12] = (f0, f1, f2, L0, L1, L2, o0, o1, o2, n0, n1, n2) of one call; tab may be null
int ms_shape_check(const char* who, int n, int D, int H, int W, int S, const int* geometry, MsShape* s, MsTable* tab) {
    INR_REQUIRE(geometry, INR_E_INVALID, "%s: null pointer (geometry)", who);
    INR_REQUIRE(n >= 0, INR_E_INVALID, "%s: bad sizes (n_volumes = %d)", who, n);
    INR_REQUIRE(S >= 1 && S <= MS_MAX_STACKS, INR_E_INVALID, "%s: stacks per volume are 1 .. %d (got %d)", who, MS_MAX_STACKS, S);
    for (int k = 0; k < S; ++k) {
        const int* g = geometry + 12 * k;
        for (int a = 0; a < 3; ++a) {
            INR_REQUIRE(g[a] >= 1 && g[a] <= MS_MAX_FACTOR, INR_E_INVALID, "%s: spacings are 1 .. %d per axis (stack %d, f%d = %d)", who,
                        MS_MAX_FACTOR, k, a, g[a]);
            INR_REQUIRE(g[3 + a] >= 1 && g[3 + a] <= MS_MAX_TAPS, INR_E_INVALID, "%s: tap counts are 1 .. %d per axis (stack %d, L%d = %d)",
                        who, MS_MAX_TAPS, k, a, g[3 + a]);
            INR_REQUIRE(g[6 + a] >= -MS_MAX_OFFSET && g[6 + a] <= MS_MAX_OFFSET, INR_E_INVALID,
                        "%s: offsets are within +-%d HR voxels (stack %d, o%d = %d)", who, MS_MAX_OFFSET, k, a, g[6 + a]);
            INR_REQUIRE(g[9 + a] >= 1 && g[9 + a] <= MS_MAX_EXTENT, INR_E_INVALID, "%s: LR extents are 1 .. %d per axis (stack %d, n%d = %d)",
                        who, MS_MAX_EXTENT, k, a, g[9 + a]);
        }
    }
    INR_REQUIRE(D >= 1 && H >= 1 && W >= 1 && D <= MS_MAX_SIDE && H <= MS_MAX_SIDE && W <= MS_MAX_SIDE, INR_E_INVALID,
                "%s: bad sizes (HR volumes of 1 .. %d samples per axis, got %d x %d x %d)", who, MS_MAX_SIDE, D, H, W);
    MsShape v{D, H, W, S, 0, 0};
    const int N[3] = {D, H, W};
    for (int k = 0; k < S; ++k) {
        const int* g = geometry + 12 * k;
        if (tab) {
            MsStack* st = &tab->g[k];
            for (int a = 0; a < 3; ++a)
                st->f[a] = (unsigned char)g[a], st->L[a] = (unsigned char)g[3 + a], st->o[a] = g[6 + a], st->n[a] = (short)g[9 + a];
            st->pad = 0;
            st->base = v.M;
            ms_stack_ranges(st, N);
        }
        v.M += (long long)g[9] * g[10] * g[11];   // <= 8 * 2^33
    }
    v.parts = ((long long)D * H * W + v.M + MS_PART - 1) / MS_PART;
    *s = v;
    return 0;
}

// the caller's HOST taps, per stack k0 | k1 | k2: finite, each summing to 1.  csum: sum over the live stacks of
// c_s = prod_a (sum_t |k_a[t]|) (max_r sum_{t = r mod f_a} |k_a[t]|), stacks ascending, axes (0, 1, 2)
int ms_taps_check(const char* who, const double* taps, const MsShape& s, MsTable* tab, double* csum) {
    INR_REQUIRE(taps, INR_E_INVALID, "%s: null pointer (taps)", who);
    const double* k = taps;
    double total = 0.0;
    for (int st = 0; st < s.S; ++st) {
        const MsStack& g = tab->g[st];
        double c = 1.0;
        for (int a = 0; a < 3; ++a) {
            double sum = 0.0, l1 = 0.0, top = 0.0;
            for (int t = 0; t < MS_MAX_TAPS; ++t) tab->k[st][a][t] = 0.0;
            for (int t = 0; t < g.L[a]; ++t) {
                INR_REQUIRE(std::isfinite(k[t]), INR_E_INVALID, "%s: the taps must be finite (stack %d, k%d[%d] is %g)", who, st, a, t, k[t]);
                tab->k[st][a][t] = k[t];
                sum += k[t];
                l1 += std::fabs(k[t]);
            }
            INR_REQUIRE(std::isfinite(sum) && std::fabs(sum - 1.0) <= 1e-9, INR_E_INVALID,
                        "%s: the taps of every axis must sum to 1 (stack %d, k%d sums to %.17g)", who, st, a, sum);
            for (int r = 0; r < g.f[a]; ++r) {
                double cls = 0.0;
                for (int t = r; t < g.L[a]; t += g.f[a]) cls += std::fabs(k[t]);
                top = std::fmax(top, cls);
            }
            c = c * (l1 * top);
            k += g.L[a];
        }
        if (g.live) total += c;
    }
    *csum = total;
    return 0;
}

template <typename T>
int ms_solve(const char* who, T* out, double* energy, double* change, double* valid_fraction, const T* y, const T* weight, const T* x0,
             int n, int D, int H, int W, int S, const int* geometry, const double* taps, const double* grad_weights, double lam,
             double alpha, int n_iter, double* workspace, int64_t workspace_doubles, hipStream_t st) {
    INR_REQUIRE(out && y, INR_E_INVALID, "%s: null pointer", who);
    INR_REQUIRE(grad_weights, INR_E_INVALID, "%s: null pointer (grad_weights)", who);
    MsShape s;
    MsTable tab;
    double csum = 0.0;
    if (int rc = ms_shape_check(who, n, D, H, W, S, geometry, &s, &tab)) return rc;
    if (int rc = tv_params_check(who, lam, alpha, n_iter, INR_TVSR3D_MAX_ITER)) return rc;
    if (int rc = tv_grad_weights_check(who, grad_weights)) return rc;
    if (int rc = ms_taps_check(who, taps, s, &tab, &csum)) return rc;
    if (int rc = check_ws_doubles(who, workspace, workspace_doubles, ms_view(n, s, nullptr).total)) return rc;
    if (n == 0) return 0;
    MsStep c;
    c.g0 = grad_weights[0], c.g1 = grad_weights[1], c.g2 = grad_weights[2];
    const double gsum = tv_grad_weight_sum(grad_weights, D, H, W);
    c.lam = gsum > 0.0 ? lam : 0.0;
    const double bound = 4.0 * gsum + csum;
    c.tau = bound > 0.0 ? 1.0 / std::sqrt(bound) : 1.0 / std::sqrt(8.0);
    c.alpha = alpha;
    const MsView v = ms_view(n, s, workspace);
    const long long voxels = (long long)n * D * H * W, data = (long long)n * s.M, items = (long long)n * s.parts;
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL((ms_init_kernel<T>), dim3(tv_thread_grid(voxels + data, MS_THREADS)), dim3(MS_THREADS), 0, st, v, x0, (long long)n, s);
    INR_LAUNCH_CHECK();
    if (!x0) {
        hipLaunchKernelGGL((ms_backproject_kernel<T>), dim3(tv_thread_grid(voxels, MS_THREADS)), dim3(MS_THREADS), 0, st, v, y, weight, (long long)n, s,
                           tab);
        INR_LAUNCH_CHECK();
    }
    const long long begin = c.lam > 0.0 ? 0 : voxels;
    for (int it = 0; it < n_iter; ++it) {
        hipLaunchKernelGGL((ms_dual_kernel<T>), dim3(tv_thread_grid(voxels + data - begin, MS_THREADS)), dim3(MS_THREADS), 0, st, v, y, weight,
                           (long long)n, s, tab, c, begin);
        INR_LAUNCH_CHECK();
        hipLaunchKernelGGL(ms_primal_kernel, dim3(tv_thread_grid(voxels, MS_THREADS)), dim3(MS_THREADS), 0, st, v, (long long)n, s, tab, c,
                           (int)(it + 1 == n_iter));
        INR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((ms_final_kernel<T>), dim3(tv_grid(items)), dim3(MS_THREADS), 0, st, out, v, y, weight, (long long)n, s, tab, c,
                       n_iter);
    INR_LAUNCH_CHECK();
    return tv_finish<MS_THREADS>(energy, change, valid_fraction, v.epart, s.parts, v.chpart, s.parts, v.vpart, (double)s.M, n, st);
}

int ms_operator(const char* who, bool adjoint, double* out, unsigned char* valid, const double* in, int n, int D, int H, int W, int S,
                const int* geometry, const double* taps, hipStream_t st) {
    INR_REQUIRE(out && in, INR_E_INVALID, "%s: null pointer", who);
    MsShape s;
    MsTable tab;
    double csum = 0.0;
    if (int rc = ms_shape_check(who, n, D, H, W, S, geometry, &s, &tab)) return rc;
    if (int rc = ms_taps_check(who, taps, s, &tab, &csum)) return rc;
    if (n == 0) return 0;
    ProfScope ps(KC_OTHER, st);
    if (adjoint)
        hipLaunchKernelGGL(ms_adjoint_kernel, dim3(tv_thread_grid((long long)n * D * H * W, MS_THREADS)), dim3(MS_THREADS), 0, st, out, in, (long long)n,
                           s, tab);
    else
        hipLaunchKernelGGL(ms_apply_kernel, dim3(tv_thread_grid((long long)n * s.M, MS_THREADS)), dim3(MS_THREADS), 0, st, out, valid, in, (long long)n,
                           s, tab);
    INR_LAUNCH_CHECK();
    return 0;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int inr_tvms_apply(double* out, unsigned char* valid, const double* in, int n_volumes, int depth, int height, int width, int n_stacks,
                   const int* geometry, const double* taps, void* stream) {
    return ms_operator("inr_tvms_apply", false, out, valid, in, n_volumes, depth, height, width, n_stacks, geometry, taps,
                       (hipStream_t)stream);
}

int inr_tvms_adjoint(double* out, const double* in, int n_volumes, int depth, int height, int width, int n_stacks, const int* geometry,
                     const double* taps, void* stream) {
    return ms_operator("inr_tvms_adjoint", true, out, nullptr, in, n_volumes, depth, height, width, n_stacks, geometry, taps,
                       (hipStream_t)stream);
}

int64_t inr_tvms_workspace_doubles(int n_volumes, int depth, int height, int width, int n_stacks, const int* geometry) {
    MsShape s;
    if (ms_shape_check("inr_tvms_workspace_doubles", n_volumes, depth, height, width, n_stacks, geometry, &s, nullptr)) return 0;
    return (int64_t)((ms_view(n_volumes, s, nullptr).total + sizeof(double) - 1) / sizeof(double));
}

int inr_tvms_solve(double* out, double* energy, double* change, double* valid_fraction, const double* y, const double* weight,
                   const double* x0, int n_volumes, int depth, int height, int width, int n_stacks, const int* geometry,
                   const double* taps, const double* grad_weights, double lambda, double alpha, int n_iter, double* workspace,
                   int64_t workspace_doubles, void* stream) {
    return ms_solve("inr_tvms_solve", out, energy, change, valid_fraction, y, weight, x0, n_volumes, depth, height, width, n_stacks,
                    geometry, taps, grad_weights, lambda, alpha, n_iter, workspace, workspace_doubles, (hipStream_t)stream);
}

int inr_tvms_solve_f32(float* out, double* energy, double* change, double* valid_fraction, const float* y, const float* weight,
                       const float* x0, int n_volumes, int depth, int height, int width, int n_stacks, const int* geometry,
                       const double* taps, const double* grad_weights, double lambda, double alpha, int n_iter, double* workspace,
                       int64_t workspace_doubles, void* stream) {
    return ms_solve("inr_tvms_solve_f32", out, energy, change, valid_fraction, y, weight, x0, n_volumes, depth, height, width, n_stacks,
                    geometry, taps, grad_weights, lambda, alpha, n_iter, workspace, workspace_doubles, (hipStream_t)stream);
}

}  // extern "C"
