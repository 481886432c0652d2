// minsnap_cost_vjp.h -- launch interface of the open-chain solve's reverse mode with a cost cotangent
// (minsnap_cost_vjp.hip), between the C-ABI (minsnap_capi.hip) and the kernel.  Internal; the public
// boundary is include/csp_minsnap.h.  Its args struct extends VjpArgs; it lives here and not beside it because
// minsnap_launch.h's bytes are part of the headline kernel's source hash (bench.py), which a reverse-mode entry should
// not move.
#pragma once
#include "minsnap_launch.h"

namespace csp {

// The VJP's scope, mapping and layouts (VjpArgs).  grad_cost is never null here: without it the call is launch_vjp.
// grad_coeffs null: the cost-only kernel, three right-hand-side columns, `ws` f64 [(Smax-1)][(o-1)^2 + 3(o-1)][B]
// (timeopt_ws_entries); otherwise six columns and the workspace of VjpArgs.
struct CostVjpArgs : VjpArgs {
    const double *grad_cost;       // [B]
};
hipError_t launch_cost_vjp(const CostVjpArgs &a, bool f32, hipStream_t st);

// Second pass of a shared bc's gradient, defined in minsnap_vjp.hip beside its kernel: one wave sums the [12][nblk] f64
// partials in a fixed order into grad_bc [4][3] of the storage type.
hipError_t launch_vjp_bc_reduce(const double *part, int64_t nblk, void *grad_bc, bool f32, hipStream_t st);

}  // namespace csp
