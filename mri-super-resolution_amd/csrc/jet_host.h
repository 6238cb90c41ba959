// The host code that the two derivative units, jet.hip (SIREN) and wire_deriv.hip (WIRE), share -- and nothing either of them does
// alone: the limits, the resolved call, the step from the run-time (tangents, Laplacian) to the kernels' compile-time (J, LAP).
// Private to those two units: no other file includes it.  What depends on the network -- descriptor checks, the workspace view and
// its refusals, the launches -- stays in the units.
#pragma once
#include <type_traits>

#include "internal.h"

namespace inr {
namespace {

constexpr int JET_MAX_J = JET_MAX_D + 2;      // the value, up to JET_MAX_D tangents, the Laplacian accumulator
constexpr int64_t JET_MAX_ROWS = (1ll << 31) - 256;

inline unsigned jet_blocks(long long work) { return (unsigned)((work + 255) / 256); }

// the kernels' grid argument: the d axes of `shape`, the rest 1 (all 1 for a call on rows, shape == null)
inline JetGrid jet_grid(const int64_t* shape, int d) {
    JetGrid g;
    for (int a = 0; a < JET_MAX_D; ++a) g.n[a] = (shape && a < d) ? shape[a] : 1;
    return g;
}

// one derivative call, resolved: rows x [n][d] (x != null) or the grid `shape` [d] of n rows, evaluated `chunk` rows at a time on
// J = 1 + dt + has_q planes
struct JetCall {
    const float* x;
    const int64_t* shape;
    int64_t n, chunk;
    int d, dt, has_q, J;
    const float* B;
    int m;
    float *y, *grad, *lap;
    JetGrid grid;
    hipStream_t st;
};

// the refusals every derivative entry point makes after its own, then the call.  n == 0 is a success with nothing to do: the caller
// returns before it looks at the workspace
inline int jet_resolve(JetCall& c, const char* who, const float* params, const float* x, const int64_t* shape, int64_t n, int d,
                       int d_tangent, const float* B, int m, float* y, float* grad, float* lap, int64_t chunk_rows, void* stream) {
    INR_REQUIRE(d_tangent >= 1 && d_tangent <= d, INR_E_INVALID, "%s: 1 <= d_tangent <= d (got %d, d = %d)", who, d_tangent, d);
    INR_REQUIRE(chunk_rows >= 1 && chunk_rows <= JET_MAX_ROWS, INR_E_INVALID, "%s: bad chunk_rows %lld", who, (long long)chunk_rows);
    INR_REQUIRE(aligned16(params), INR_E_ALIGN, "%s: params must be 16-byte aligned", who);
    // with neither derivative asked for only the value plane is carried; a Laplacian needs the tangents too
    const int dt = (grad || lap) ? d_tangent : 0;
    const int has_q = lap ? 1 : 0;
    c = JetCall{x, shape, n, chunk_rows < n ? chunk_rows : n, d, dt, has_q, 1 + dt + has_q, B, m, y, grad, lap, jet_grid(shape, d),
                (hipStream_t)stream};
    return 0;
}

// f(std::integral_constant<int, J>, std::bool_constant<LAP>) for the J = 1 + dt + lap planes of `dt` tangents with (lap = 1) or
// without the Laplacian; false where no kernel is built for the pair
template <int DT, int LAP, class F>
inline void jet_call_as(F& f) {
    f(std::integral_constant<int, 1 + DT + LAP>{}, std::bool_constant<LAP != 0>{});
}
template <class F>
inline bool jet_dispatch(int dt, int lap, F f) {
    switch (2 * dt + lap) {
        case 0: jet_call_as<0, 0>(f); return true;
        case 2: jet_call_as<1, 0>(f); return true;
        case 3: jet_call_as<1, 1>(f); return true;
        case 4: jet_call_as<2, 0>(f); return true;
        case 5: jet_call_as<2, 1>(f); return true;
        case 6: jet_call_as<3, 0>(f); return true;
        case 7: jet_call_as<3, 1>(f); return true;
        case 8: jet_call_as<4, 0>(f); return true;
        case 9: jet_call_as<4, 1>(f); return true;
        default: return false;
    }
}

}  // namespace
}  // namespace inr
