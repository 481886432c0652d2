// minsnap_periodic_timeopt.h -- launch interface of the lap-time optimiser of the periodic (closed-loop) solve
// (minsnap_periodic_timeopt.hip, csp_minsnap_optimize_times_periodic_batch).  Internal; the public boundary
// is include/csp_minsnap.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace csp {

// Orders 2..5, uniform or ragged, f64 storage or f32 storage with f64 arithmetic, zero-velocity penalty.  One lane per
// loop, workgroups of 64.  Trajectory b owns waypoints AND times seg0 .. seg0 + S_b - 1 (the periodic solve's layout: no
// closing waypoint, no +b offset).
struct PeriodicTimeOptArgs {
    const void *wp;                // [B][S][3] (or ragged concatenation)
    const void *times;             // [B][S]: the input times
    void *times_out;               // [B][S] (the layout of times)
    double *objective;             // [B][2] initial, final objective, or null
    int32_t *iterations;           // [B] or null
    int32_t *status;               // [B] or null
    const int64_t *seg_off;        // ragged prefix sums or null
    void *ws;                      // f64 [(Smax-1)][2(o-1)^2 + 3(o-1)][B]: W_k, V_k, z_k of knots 1..S-1 (minsnap_periodic.hip's)
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
hipError_t launch_periodic_timeopt(const PeriodicTimeOptArgs &a, bool f32, hipStream_t st);

// The offsets the coefficient launch of a ragged device call reads: out[0..B] = seg_off[0..B] when every S_b <= Smax.
// launch_periodic has no length guard (a lane longer than the workspace was sized for writes past it) and an offsets
// table cannot leave one trajectory out without moving its neighbours, so with a longer trajectory in the batch every
// entry is seg_off[0]: all lanes see S = 0 and the launch writes nothing.  One workgroup, no atomics.
hipError_t launch_periodic_coeff_offsets(const int64_t *seg_off, int64_t *out, int64_t B, int Smax, hipStream_t st);

}  // namespace csp
