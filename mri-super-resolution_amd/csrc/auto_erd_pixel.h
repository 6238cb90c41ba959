// The per-pixel body of auto_erd_kernel (metrics.hip), in a header that also compiles without the HIP compiler: the same text runs
// in the kernel and in tools/auto_erd_host.cpp, a stand-alone host program that tests/test_metrics_edges_cpu.py builds with
// -fsanitize=address,undefined and compares with oracle/erd_oracle.py.
//
// One pixel: the n acquisition values (a 1-D sample) are split in two by complete-linkage agglomeration exactly as
// sklearn.cluster.AgglomerativeClustering(n_clusters=2, linkage='complete') does it -- scipy's nearest-neighbour-chain walk
// (scipy/cluster/_hierarchy.pyx: nn_chain, ties resolved by scan order and by preferring the previous chain element), a STABLE
// sort of the merges by distance, the tree cut at its last merge -- then one of the reference's two rejection rules.  Intensities
// are often integer-valued, so equal distances are the rule, not the exception: every tie falls as it does in scipy
// (oracle/erd_oracle.py restates the same steps in NumPy and is pinned against sklearn itself: tests/golden/erd.npz).
// float64 throughout (scipy converts to double); n <= ERD_MAXN values live in private arrays.
//
// Pixels that are not clustered.  A pixel keeps every acquisition (all accept entries 1) when
//   * one of its n values is not finite (sklearn refuses such input), or
//   * its largest pairwise distance, max - min, overflows to +inf.
// erd_volume.hip has the same two rules, the second one implicitly: it starts the walk on such a pixel, but the last merge joins
// the two remaining clusters at the largest pairwise distance, the chain is empty or one long by then (a chain of two would hold
// two clusters at a distance strictly below +inf, and only two are left), the walk therefore looks for a distance strictly below
// +inf, finds none, and the kernel leaves the pixel unclustered -- at that merge if not at an earlier one.  Both kernels thus keep
// everything exactly where max - min is +inf, and tests/test_gpu_metrics_edges.py compares them on such pixels.
//
// Termination.  Past the guard every D[i][j] is a finite number (an absolute difference of finite values that is at most max - min,
// or an fmax of two such).  A chain of length 1 starts from cur = +inf with at least one other live cluster (k < n - 1 merges have
// been made, n - k >= 2 clusters live), whose finite distance is strictly below +inf: b becomes a valid index.  A longer chain
// starts from b = its previous element.  So b is never negative when it is used.  A step appends b only when D[a][b] is STRICTLY
// below D[a][previous element] (the previous element wins ties), so the distances between neighbours decrease strictly along the
// chain, no cluster appears in it twice, it holds at most one entry per live cluster, and after fewer than n steps the nearest
// neighbour is the previous element.  (The part of a chain that a merge leaves behind keeps this order: complete linkage only
// ever raises the distances to the merged cluster, and the distances among the clusters that stay are untouched.)  The two `return`s inside the walk are therefore unreachable; they are there so that a
// mistake in this argument ends in "keep everything" and not in an index outside the private arrays.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define INR_ERD_HD __host__ __device__
#else
#define INR_ERD_HD
#endif

namespace inr {

constexpr int ERD_MAXN = 32;

// numpy's pairwise summation as np.mean runs it on a short contiguous float64 array (n < 8: plain loop; else eight partial sums)
INR_ERD_HD inline double erd_numpy_sum(const double* a, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

// accept[0..n) <- 1 = keep / 0 = reject for the n values of one pixel (2 <= n <= ERD_MAXN, rule 1 or 2, majority = (2/3) n;
// erd_positive: the pixel's ERD-map entry is positive, or there is no map)
INR_ERD_HD inline void auto_erd_pixel(float* accept, const double* values, int n, int rule, double majority, bool erd_positive) {
    double x[ERD_MAXN], D[ERD_MAXN][ERD_MAXN], md[ERD_MAXN];
    int size[ERD_MAXN], chain[ERD_MAXN], mlo[ERD_MAXN], mhi[ERD_MAXN], order[ERD_MAXN], parent[ERD_MAXN];
    for (int i = 0; i < n; ++i) accept[i] = 1.f;
    bool finite = true;
    double lo_v = INFINITY, hi_v = -INFINITY;
    for (int i = 0; i < n; ++i) {
        x[i] = values[i];
        finite = finite && isfinite(x[i]);
        lo_v = fmin(lo_v, x[i]);
        hi_v = fmax(hi_v, x[i]);
    }
    if (!finite || !isfinite(hi_v - lo_v)) return;   // not clustered: keeps every acquisition
    for (int i = 0; i < n; ++i) {
        size[i] = 1;
        for (int j = 0; j < n; ++j) D[i][j] = fabs(x[i] - x[j]);
    }
    int chain_len = 0;
    for (int k = 0; k < n - 1; ++k) {
        if (chain_len == 0) {
            chain_len = 1;
            for (int i = 0; i < n; ++i)
                if (size[i] > 0) {
                    chain[0] = i;
                    break;
                }
        }
        int a, b;
        double cur;
        while (true) {
            a = chain[chain_len - 1];
            if (chain_len > 1) {
                b = chain[chain_len - 2];
                cur = D[a][b];
            } else {
                b = -1;
                cur = INFINITY;
            }
            for (int i = 0; i < n; ++i) {
                if (size[i] == 0 || i == a) continue;
                if (D[a][i] < cur) {
                    cur = D[a][i];
                    b = i;
                }
            }
            if (b < 0) return;                      // unreachable (see above)
            if (chain_len > 1 && b == chain[chain_len - 2]) break;
            if (chain_len >= n) return;             // unreachable (see above)
            chain[chain_len++] = b;
        }
        chain_len -= 2;
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        mlo[k] = lo;
        mhi[k] = hi;
        md[k] = cur;
        size[hi] += size[lo];
        size[lo] = 0;
        for (int i = 0; i < n; ++i) {
            if (size[i] == 0 || i == hi) continue;
            const double d = fmax(D[i][lo], D[i][hi]);
            D[i][hi] = d;
            D[hi][i] = d;
        }
    }
    // stable sort of the n - 1 merges by distance (insertion sort keeps equal keys in order)
    for (int k = 0; k < n - 1; ++k) {
        int j = k;
        while (j > 0 && md[order[j - 1]] > md[k]) {
            order[j] = order[j - 1];
            --j;
        }
        order[j] = k;
    }
    for (int i = 0; i < n; ++i) parent[i] = i;
    auto find = [&](int i) {
        while (parent[i] != i) i = parent[i];
        return i;
    };
    for (int q = 0; q < n - 2; ++q) {
        const int k = order[q];
        parent[find(mlo[k])] = find(mhi[k]);
    }
    const int root = find(0);
    // the two clusters: in0 = with point 0, the rest
    double g0[ERD_MAXN], g1[ERD_MAXN];
    int n0 = 0, n1 = 0;
    bool in0[ERD_MAXN];
    for (int i = 0; i < n; ++i) {
        in0[i] = find(i) == root;
        if (in0[i]) g0[n0++] = x[i];
        else g1[n1++] = x[i];
    }
    bool drop0 = false, drop1 = false;      // reject cluster 0 / cluster 1
    if (rule == 1) {
        if ((double)n0 >= majority) drop1 = true;
        if ((double)n1 >= majority) drop0 = true;
    } else if (erd_positive) {
        const double m0 = erd_numpy_sum(g0, n0) / (double)n0, m1 = erd_numpy_sum(g1, n1) / (double)n1;
        if (m0 > m1) drop1 = true;
        if (m1 > m0) drop0 = true;
    }
    for (int i = 0; i < n; ++i) accept[i] = (in0[i] ? drop0 : drop1) ? 0.f : 1.f;
}

}  // namespace inr
