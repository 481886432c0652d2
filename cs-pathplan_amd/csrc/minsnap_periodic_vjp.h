// minsnap_periodic_vjp.h -- launch interface of the periodic solve's reverse mode (minsnap_periodic_vjp.hip), between
// the C-ABI (minsnap_capi.hip) and the kernel.  Internal; the public boundary is include/csp_minsnap.h.
#pragma once
#include "minsnap_launch.h"

namespace csp {

// Scope, mapping and layouts of launch_periodic (minsnap_launch.h).  The J_bar terms are compiled in when `grad_cost`
// is non-null; each of the two outputs may be null.
struct PeriodicVjpArgs {
    const void *wp;                // [B][S][3] (or ragged concatenation)
    const void *times;             // [B][S]
    const void *grad_coeffs;       // [B][S][3][2o]
    const double *grad_cost;       // [B] or null
    void *grad_wp;                 // layout of wp, or null
    void *grad_times;              // layout of times, or null
    int32_t *status;               // [B] or null
    const int64_t *seg_off;        // ragged prefix sums or null
    void *ws;                      // f64 [(Smax-1)][2(o-1)^2 + 6(o-1)][B]: W, V, z (3 primal + 3 adjoint) per knot 1..S-1
    const double *vw_per;          // [B] or null
    double vel_zero_weight;
    int64_t B;
    int S;                         // uniform S (ignored when seg_off != null)
    int order;
};
inline size_t periodic_vjp_ws_entries(int order) { const int n = order - 1; return (size_t)(2 * n * n + 6 * n); }
hipError_t launch_periodic_vjp(const PeriodicVjpArgs &a, bool f32, hipStream_t st);

}  // namespace csp
