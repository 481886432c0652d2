// minsnap_knots_timeopt.h -- launch interface of the segment-time optimiser under per-knot derivative constraints
// (minsnap_knots_timeopt.hip, csp_minsnap_optimize_times_knots_batch).  Internal; the public boundary is
// include/csp_minsnap.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace csp {

// Orders 2..5, uniform or ragged, f64 storage or f32 storage with f64 arithmetic, zero-velocity penalty.  One lane per
// trajectory, workgroups of 64.  Trajectory b owns knots (waypoints) seg0 + b .. seg0 + b + S_b.
struct KnotsTimeOptArgs {
    const void *wp;                // [B][S+1][3] (or ragged concatenation)
    const void *times;             // [B][S]: the input times
    const uint8_t *mask;           // [knots]: bit r set = derivative r+1 of the knot is fixed
    const void *values;            // [knots][o-1][3], storage type
    void *times_out;               // [B][S] (the layout of times)
    double *objective;             // [B][2] initial, final objective, or null
    int32_t *iterations;           // [B] or null
    int32_t *status;               // [B] or null
    const int64_t *seg_off;        // ragged prefix sums or null
    void *ws;                      // f64 [(Smax+1)][(o-1)^2 + 3(o-1)][B]: W_k, z_k per knot (knots 0..S-1 are stored)
    double *vec;                   // f64 [4][Smax][B] current / trial times and their gradients
    const double *vw_per;          // [B] or null
    double vel_zero_weight;
    double time_weight, min_time, tol;
    int64_t B;
    int S;                         // uniform S (ignored when seg_off != null)
    int Smax;                      // segments the workspace holds per trajectory: a longer ragged trajectory is skipped
    int order;
    int mode;                      // CSP_TIMEOPT_*_V (minsnap_launch.h)
    int max_iters;
};
hipError_t launch_knots_timeopt(const KnotsTimeOptArgs &a, bool f32, hipStream_t st);

}  // namespace csp
