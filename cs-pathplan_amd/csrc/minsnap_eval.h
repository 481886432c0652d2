// minsnap_eval.h -- launch interface of the trajectory evaluation kernels (minsnap_eval.hip), between the C-ABI
// (minsnap_capi.hip) and the kernels.  Internal; the public boundary and the contract are in include/csp_minsnap.h
// (csp_minsnap_eval_batch, csp_minsnap_eval_batch_vjp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "minsnap_eval_plan.h"

namespace csp {

// Forward when grad_out is null (writes out / seg_index), reverse otherwise (writes the grad_* that are non-null).
// All floating arrays are in the storage type; the arithmetic is fp64.
struct EvalArgs {
    const void *times;        // [B][S] (or ragged concatenation)
    const void *coeffs;       // [B][S][3][2o], records 16-byte (fp64) / 8-byte (fp32) aligned
    const void *query;        // [B][Q]
    const void *grad_out;     // reverse: [B][Q][D][3]
    void *out;                // forward: [B][Q][D][3]
    int32_t *seg_index;       // forward: [B][Q] or null
    void *grad_coeffs;        // reverse: layout of coeffs, or null
    void *grad_times;         // reverse: layout of times, or null
    void *grad_query;         // reverse: [B][Q], or null
    int32_t *status;          // [B] or null
    const int64_t *seg_off;   // ragged prefix sums or null
    int64_t B, Q;
    int S;                    // uniform S (ignored when seg_off != null)
    int Smax;                 // S, or the ragged batch's max_segments
    int order, D;
};
hipError_t launch_eval(const EvalArgs &a, bool f32, hipStream_t st);
hipError_t launch_eval_vjp(const EvalArgs &a, bool f32, hipStream_t st);

}  // namespace csp
