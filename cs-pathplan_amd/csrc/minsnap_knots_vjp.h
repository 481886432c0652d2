// minsnap_knots_vjp.h -- launch interface of the knot-constrained solve's reverse mode (minsnap_knots_vjp.hip,
// csp_minsnap_solve_knots_batch_vjp).  Internal; the public boundary is include/csp_minsnap.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace csp {

// Scope, mapping and layouts of launch_knots (minsnap_knots.h).  The instantiation follows from which cotangents are
// given: grad_coeffs alone, both, or grad_cost alone (three right-hand-side columns, grad_coeffs never read).  Each of
// the three outputs may be null.
struct KnotsVjpArgs {
    const void *wp;                // [B][S+1][3] (or ragged concatenation)
    const void *times;             // [B][S]
    const uint8_t *mask;           // [knots]: bit r set = derivative r+1 of the knot is fixed
    const void *values;            // [knots][o-1][3], storage type
    const void *grad_coeffs;       // [B][S][3][2o] (trajectory-major) or null
    const double *grad_cost;       // [B] or null
    void *grad_wp;                 // layout of wp, or null
    void *grad_times;              // layout of times, or null
    void *grad_values;             // layout of values, or null
    int32_t *status;               // [B] or null
    const int64_t *seg_off;        // ragged prefix sums or null
    void *ws;                      // f64 [(Smax+1)][(o-1)^2 + c(o-1)][B], c = 6 with grad_coeffs and 3 without: W_k, z_k
    const double *vw_per;          // [B] or null
    double vel_zero_weight;
    int64_t B;
    int S;                         // uniform S (ignored when seg_off != null)
    int Smax;                      // knots the workspace holds per trajectory, less one: a longer ragged trajectory is skipped
    int order;
};
inline size_t knots_vjp_ws_entries(int order, bool pbar) { const int n = order - 1; return (size_t)(n * n + (pbar ? 6 : 3) * n); }
hipError_t launch_knots_vjp(const KnotsVjpArgs &a, bool f32, hipStream_t st);

}  // namespace csp
