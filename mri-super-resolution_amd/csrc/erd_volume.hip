// Whole-volume AutoERD with the ERD-weighted direction means and ADC maps of implicit-neural-representations/david.py:44-91.
// One thread owns one pixel and does everything for it in one launch:
//
//   clustering  the n acquisition values are split in two exactly as auto_erd_kernel (metrics.hip) splits them -- scipy's
//               nearest-neighbour-chain walk, the cut at the last of the stably sorted merges, rules 1 and 2 -- but without the
//               n x n distance matrix.  For a 1-D sample the complete-linkage distance of clusters A and B is
//               max(max A, max B) - min(min A, min B): the clusters the walk forms are intervals that do not interleave, rounding
//               is monotone, so the largest rounded |x_i - x_j| over A x B is the rounded difference of the extreme pair, which is
//               the entry the Lance-Williams update D[i][hi] = fmax(D[i][lo], D[i][hi]) would hold, bit for bit (DESIGN.md 4h;
//               tests/test_erd_volume_cpu.py checks the identity against the sklearn fixtures).  A live cluster is its (min, max).
//   the cut     scipy sorts the merges by distance (stable) and sklearn unites all but the last of that list.  The last of a
//               stable sort is the LAST-FOUND merge among those of the largest distance, and leaving one merge (lo, hi) out of a
//               union-find over all of them leaves exactly two components: the points slot lo held when it was merged, and the
//               rest.  So the walk keeps a membership mask per live slot and remembers the mask of slot lo at the latest merge
//               whose distance is >= every earlier one: no merge list, no sort, no union-find.
//   reductions  per group of acquisitions three sequential fp64 sums (david.py:62-78), the two means and their ADC maps
//               (david.py:80-85), optionally the ADC of every acquisition (david.py:68-69).
//
// Layouts: lanes are pixels, so every global array is a stack of planes ([n][P] in, [n][P] and [G][P] out) and a wave's loads and
// stores are contiguous.  The per-pixel state lives in dynamic LDS laid out [slot][lane]: a lane only ever touches its own column,
// whichever slot its data-dependent index selects, so the bank of an access depends on the lane alone and a wave's access is
// conflict-free for 4- and 8-byte words (bank = (slot * 64 * w + lane * w) / 4 mod 64).  21 n bytes per pixel: cmin, cmax (fp64),
// the membership masks (u32) and the chain (u8); 1,344 n bytes per 64-pixel block, 43,008 B at n = 32.  No scratch, no atomics.
// This unit is compiled with -ffp-contract=off (_build.py SOURCE_FLAGS): value * accept is rounded before it is added, as NumPy
// does, and the ADC stays a division, an addition, a log, a division and a multiplication.
#include <math.h>

#include "internal.h"

namespace inr {
namespace {

constexpr int EV_MAXN = 32, EV_MAXG = INR_ERD_VOLUME_MAX_GROUPS, EV_LANES = 64;
constexpr double EV_EPS = 1e-7;   // david.py:28

struct EvGroups {
    int n;
    int size[EV_MAXG];
};

size_t ev_lds_bytes(int n) { return (size_t)EV_LANES * (size_t)n * (2 * sizeof(double) + sizeof(unsigned) + 1); }

// david.py:68-69, 82-85: -log(v / (b0 + eps) + eps) / b, then *= 1000 (ONE factor 1000; master.py's calc_adc has two)
__device__ __forceinline__ double ev_adc(double v, double b0_eps, double b) {
    const double ratio = v / b0_eps;
    const double arg = ratio + EV_EPS;
    const double neg_log = -log(arg);
    const double q = neg_log / b;
    return q * 1000.0;
}

// erd_numpy_sum of metrics.hip (numpy's pairwise summation of a short contiguous float64 array) on a column of the LDS image:
// element i is a[i * EV_LANES].  r[] is only ever indexed by unrolled constants, so it stays in registers.
__device__ double ev_numpy_sum(const double* a, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += a[i * EV_LANES];
        return r;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j * EV_LANES];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += a[(i + j) * EV_LANES];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i * EV_LANES];
    return res;
}

__global__ void __launch_bounds__(EV_LANES)
erd_volume_kernel(double* __restrict__ accept, double* __restrict__ direction_mean, double* __restrict__ accepted_mean,
                  double* __restrict__ direction_adc, double* __restrict__ accepted_adc, double* __restrict__ adc,
                  const double* __restrict__ values, const double* __restrict__ b0, const double* __restrict__ erd_map,
                  const double* __restrict__ accept_in, int64_t npix, int n, EvGroups groups, double b, int rule, double majority) {
    extern __shared__ double ev_lds[];
    const int lane = threadIdx.x;
    const int64_t pix = (int64_t)blockIdx.x * EV_LANES + lane;
    if (pix >= npix) return;   // (no barrier anywhere: a lane's columns are its own)
    double* cmin = ev_lds + lane;                                                    // [n][64]
    double* cmax = cmin + n * EV_LANES;                                              // [n][64]
    unsigned* member = reinterpret_cast<unsigned*>(ev_lds + 2 * n * EV_LANES) + lane;   // [n][64]
    unsigned char* chain = reinterpret_cast<unsigned char*>(ev_lds) + (size_t)n * EV_LANES * 20 + lane;   // [n][64]
    const unsigned full = n == 32 ? 0xffffffffu : (1u << n) - 1u;

    unsigned reject = 0;   // bit i: acquisition i is rejected
    bool finite = true;
    if (rule != 0) {
        for (int i = 0; i < n; ++i) {
            const double v = values[(int64_t)i * npix + pix];
            finite = finite && isfinite(v);
            cmin[i * EV_LANES] = v;
            cmax[i * EV_LANES] = v;
            member[i * EV_LANES] = 1u << i;
        }
    }
    // A pixel with a non-finite value is not clustered and keeps every acquisition (sklearn refuses such input).
    if (rule != 0 && finite) {
        unsigned alive = full, cut = 0;
        double cut_dist = -INFINITY;
        int chain_len = 0;
        bool ok = true;
        for (int k = 0; k < n - 1 && ok; ++k) {
            if (chain_len == 0) {
                chain[0] = (unsigned char)(__ffs((int)alive) - 1);
                chain_len = 1;
            }
            int a, bb;
            double cur;
            // The walk terminates for finite input: a step appends bb only when dist(a, bb) is STRICTLY below dist(a, previous
            // element) (the previous element wins ties), so the distances between neighbours decrease strictly along the chain,
            // no cluster can appear in it twice, and it holds at most one entry per live cluster: after fewer than `live` steps
            // the nearest neighbour is the previous element.  All comparisons are between finite numbers or +inf (the extent of
            // two finite values can overflow), never NaN, so "strictly below" is a strict order.
            while (true) {
                a = chain[(chain_len - 1) * EV_LANES];
                const double amin = cmin[a * EV_LANES], amax = cmax[a * EV_LANES];
                if (chain_len > 1) {
                    bb = chain[(chain_len - 2) * EV_LANES];
                    cur = fmax(amax, cmax[bb * EV_LANES]) - fmin(amin, cmin[bb * EV_LANES]);
                } else {
                    bb = -1;
                    cur = INFINITY;
                }
                for (unsigned m = alive & ~(1u << a); m; m &= m - 1) {   // live slots in rising order, as scipy scans them
                    const int i = __ffs((int)m) - 1;
                    const double d = fmax(amax, cmax[i * EV_LANES]) - fmin(amin, cmin[i * EV_LANES]);
                    if (d < cur) {
                        cur = d;
                        bb = i;
                    }
                }
                // No neighbour found (every extent overflowed to +inf): there is no index to step to.  The pixel is left
                // unclustered and keeps everything.
                if (bb < 0) {
                    ok = false;
                    break;
                }
                if (chain_len > 1 && bb == chain[(chain_len - 2) * EV_LANES]) break;
                if (chain_len >= n) {   // cannot happen (see above); the chain's column has n entries and is never written past them
                    ok = false;
                    break;
                }
                chain[chain_len * EV_LANES] = (unsigned char)bb;
                ++chain_len;
            }
            if (!ok) break;
            chain_len -= 2;
            const int lo = a < bb ? a : bb, hi = a < bb ? bb : a;
            const unsigned mlo = member[lo * EV_LANES];
            if (cur >= cut_dist) {   // the last of the stably sorted merges so far
                cut_dist = cur;
                cut = mlo;
            }
            member[hi * EV_LANES] |= mlo;
            cmin[hi * EV_LANES] = fmin(cmin[lo * EV_LANES], cmin[hi * EV_LANES]);
            cmax[hi * EV_LANES] = fmax(cmax[lo * EV_LANES], cmax[hi * EV_LANES]);
            alive &= ~(1u << lo);
        }
        if (ok) {
            const unsigned c0 = cut, c1 = full & ~cut;   // the two clusters
            const int n0 = __popc(c0), n1 = n - n0;
            bool drop0 = false, drop1 = false;
            if (rule == 1) {
                if ((double)n0 >= majority) drop1 = true;
                if ((double)n1 >= majority) drop0 = true;
            } else if (!erd_map || erd_map[pix] > 0.0) {
                // the clusters' values, gathered in acquisition order into the (now free) cmin / cmax columns
                int k0 = 0, k1 = 0;
                for (int i = 0; i < n; ++i) {
                    const double v = values[(int64_t)i * npix + pix];
                    if ((c0 >> i) & 1u) cmin[(k0++) * EV_LANES] = v;
                    else cmax[(k1++) * EV_LANES] = v;
                }
                const double m0 = ev_numpy_sum(cmin, n0) / (double)n0, m1 = ev_numpy_sum(cmax, n1) / (double)n1;
                if (m0 > m1) drop1 = true;
                if (m1 > m0) drop0 = true;
            }
            reject = (drop0 ? c0 : 0u) | (drop1 ? c1 : 0u);
        }
    }
    if (accept)
        for (int i = 0; i < n; ++i) {
            const int64_t at = (int64_t)i * npix + pix;
            accept[at] = rule == 0 ? (accept_in ? accept_in[at] : 1.0) : (((reject >> i) & 1u) ? 0.0 : 1.0);
        }

    const bool want_adc = direction_adc || accepted_adc || adc;
    const double b0_eps = want_adc ? b0[pix] + EV_EPS : 0.0;
    if (direction_mean || accepted_mean || direction_adc || accepted_adc) {
        int first = 0;
        for (int g = 0; g < groups.n; ++g) {
            double sum_image = 0.0, sum_accepted = 0.0, sum_accepts = 0.0;
            for (int i = first; i < first + groups.size[g]; ++i) {
                const int64_t at = (int64_t)i * npix + pix;
                const double v = values[at];
                const double w = rule == 0 ? (accept_in ? accept_in[at] : 1.0) : (((reject >> i) & 1u) ? 0.0 : 1.0);
                sum_image += v;
                sum_accepted += v * w;
                sum_accepts += w;
            }
            first += groups.size[g];
            const double dmean = sum_image / (double)groups.size[g];
            const double amean = sum_accepted / sum_accepts;   // 0 / 0 = NaN where the whole group is rejected, as in NumPy
            const int64_t at = (int64_t)g * npix + pix;
            if (direction_mean) direction_mean[at] = dmean;
            if (accepted_mean) accepted_mean[at] = amean;
            if (direction_adc) direction_adc[at] = ev_adc(dmean, b0_eps, b);
            if (accepted_adc) accepted_adc[at] = ev_adc(amean, b0_eps, b);
        }
    }
    if (adc)
        for (int i = 0; i < n; ++i) {
            const int64_t at = (int64_t)i * npix + pix;
            adc[at] = ev_adc(values[at], b0_eps, b);
        }
}

// host only: no device is touched
int erd_volume_check(int n, const int* group_sizes, int n_groups, double b, int rule) {
    INR_REQUIRE(n >= 2 && n <= EV_MAXN, INR_E_INVALID, "inr_auto_erd_volume: 2 <= acquisitions <= %d (got %d)", EV_MAXN, n);
    INR_REQUIRE(rule >= 0 && rule <= 2, INR_E_INVALID,
                "inr_auto_erd_volume: rule must be 0 (no clustering), 1 (majority voting) or 2 (intensity-cognisant)");
    INR_REQUIRE(n_groups >= 1 && n_groups <= EV_MAXG, INR_E_INVALID, "inr_auto_erd_volume: 1 <= groups <= %d (got %d)", EV_MAXG, n_groups);
    INR_REQUIRE(group_sizes != nullptr, INR_E_INVALID, "inr_auto_erd_volume: null pointer (group_sizes)");
    long long total = 0;
    for (int g = 0; g < n_groups; ++g) {
        INR_REQUIRE(group_sizes[g] >= 1, INR_E_INVALID, "inr_auto_erd_volume: group %d has size %d (< 1)", g, group_sizes[g]);
        total += group_sizes[g];
    }
    INR_REQUIRE(total == n, INR_E_INVALID, "inr_auto_erd_volume: the group sizes sum to %lld, not to the %d acquisitions", total, n);
    INR_REQUIRE(b != 0.0 && b == b, INR_E_INVALID, "inr_auto_erd_volume: b must not be 0");
    return 0;
}

int launch_erd_volume(double* accept, double* direction_mean, double* accepted_mean, double* direction_adc, double* accepted_adc,
                      double* adc, const double* values, const double* b0, const double* erd_map, const double* accept_in, int64_t npix,
                      int n, const int* group_sizes, int n_groups, double b, int rule, hipStream_t st) {
    if (int rc = erd_volume_check(n, group_sizes, n_groups, b, rule)) return rc;
    if (npix == 0) return 0;
    EvGroups groups{};
    groups.n = n_groups;
    for (int g = 0; g < n_groups; ++g) groups.size[g] = group_sizes[g];
    const double majority = (2.0 / 3.0) * (double)n;   // david.py:54, evaluated as Python does
    ProfScope ps(KC_OTHER, st);
    hipLaunchKernelGGL(erd_volume_kernel, dim3((unsigned)((npix + EV_LANES - 1) / EV_LANES)), dim3(EV_LANES), ev_lds_bytes(n), st, accept,
                       direction_mean, accepted_mean, direction_adc, accepted_adc, adc, values, b0, erd_map, accept_in, npix, n, groups, b,
                       rule, majority);
    INR_LAUNCH_CHECK();
    return 0;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int inr_auto_erd_volume(double* accept, double* direction_mean, double* accepted_mean, double* direction_adc, double* accepted_adc,
                   double* adc, const double* values, const double* b0, const double* erd_map, const double* accept_in,
                   int64_t n_pixels, int n_acquisitions, const int* group_sizes, int n_groups, double b, int rule, void* stream) {
    INR_REQUIRE(values != nullptr, INR_E_INVALID, "inr_auto_erd_volume: null pointer (values)");
    INR_REQUIRE(b0 != nullptr || !(direction_adc || accepted_adc || adc), INR_E_INVALID,
                "inr_auto_erd_volume: null pointer (b0, which the ADC outputs need)");
    INR_REQUIRE(n_pixels >= 0 && n_pixels < (1ll << 37), INR_E_INVALID, "inr_auto_erd_volume: bad pixel count");
    if (int rc = erd_volume_check(n_acquisitions, group_sizes, n_groups, b, rule)) return rc;
    INR_REQUIRE(rule == 0 || accept_in == nullptr, INR_E_INVALID,
                "inr_auto_erd_volume: accept_in supplies the weights of rule 0; rules 1 and 2 compute them");
    return launch_erd_volume(accept, direction_mean, accepted_mean, direction_adc, accepted_adc, adc, values, b0, erd_map, accept_in,
                             n_pixels, n_acquisitions, group_sizes, n_groups, b, rule, (hipStream_t)stream);
}

}  // extern "C"
