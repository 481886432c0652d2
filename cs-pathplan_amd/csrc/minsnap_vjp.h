// minsnap_vjp.h -- launch interface of the open-chain solve's reverse mode (minsnap_vjp.hip), between
// the C-ABI (minsnap_capi.hip) and the kernel.  Internal; the public boundary is include/csp_minsnap.h.  Its args struct
// extends VjpArgs; it lives here and not beside it because minsnap_launch.h's bytes are part of the headline kernel's
// source hash (bench.py), which a reverse-mode entry should not move.
#pragma once
#include "minsnap_launch.h"

namespace csp {

// The VJP's scope, mapping and layouts (VjpArgs), with a cotangent of the snap cost beside the one of the coefficients;
// either may be null, not both.  grad_coeffs null: the cost-only kernel, three right-hand-side columns, `ws` f64
// [(Smax-1)][(o-1)^2 + 3(o-1)][B] (timeopt_ws_entries); otherwise six columns and the workspace of VjpArgs.
struct CostVjpArgs : VjpArgs {
    const double *grad_cost;       // [B] or null
};
hipError_t launch_vjp(const CostVjpArgs &a, bool f32, hipStream_t st);

}  // namespace csp
