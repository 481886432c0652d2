// minsnap_knots.h -- launch interface of the open-chain solve with per-knot derivative constraints
// (minsnap_knots.hip, csp_minsnap_solve_knots_batch).  Internal; the public boundary is
// include/csp_minsnap.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace csp {

// Orders 2..5, uniform or ragged, f64 storage or f32 storage with f64 arithmetic, zero-velocity penalty.  One lane per
// trajectory, workgroups of 64.  Trajectory b owns knots (waypoints) seg0 + b .. seg0 + b + S_b.
struct KnotsArgs {
    const void *wp;                // [B][S+1][3] (or ragged concatenation)
    const void *times;             // [B][S]
    const uint8_t *mask;           // [knots]: bit r set = derivative r+1 of the knot is fixed
    const void *values;            // [knots][o-1][3], storage type
    void *coeffs;                  // [B][S][3][2o] (trajectory-major)
    double *cost;                  // [B] or null
    int32_t *status;               // [B] or null
    const int64_t *seg_off;        // ragged prefix sums or null
    void *ws;                      // f64 [(Smax+1)][(o-1)^2 + 3(o-1)][B]: W_k, z_k per knot 0..S
    const double *vw_per;          // [B] or null
    double vel_zero_weight;
    int64_t B;
    int S;                         // uniform S (ignored when seg_off != null)
    int Smax;                      // knots the workspace holds per trajectory, less one: a longer ragged trajectory is skipped
    int order;
};
inline size_t knots_ws_entries(int order) { const int n = order - 1; return (size_t)(n * n + 3 * n); }
hipError_t launch_knots(const KnotsArgs &a, bool f32, hipStream_t st);

}  // namespace csp
