// minsnap_fixed_o4d.hip -- instantiates the write-through flavour of the persistent order-4 kernel
// (minsnap_fixed_impl.h: minsnap_fixed_persistent_wt_kernel) for the even segment counts, whose records leave as
// paired whole-line bursts.  launch_s (minsnap_fixed_o4a/b/c.hip) calls it for launches whose coefficients exceed the
// chip's aggregate L2 and fit the Infinity Cache (plan_fixed in minsnap_fixed_plan.h).
#include "minsnap_fixed_impl.h"

#ifdef CSP_STAMPS
extern "C" int csp_debug_read_stamps_wt(unsigned long long *host, size_t n) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(csp_g_stamps), n * sizeof(unsigned long long));
}
#endif

namespace csp {
namespace fixedk {

template <int S>
static void launch_wt(const GenericArgs &f, int n_slices, unsigned grid, hipStream_t st) {
    if (f.status) hipLaunchKernelGGL((minsnap_fixed_persistent_wt_kernel<4, S, true, SP_WT>), dim3(grid), dim3(128), 0, st, f, n_slices);
    else hipLaunchKernelGGL((minsnap_fixed_persistent_wt_kernel<4, S, false, SP_WT>), dim3(grid), dim3(128), 0, st, f, n_slices);
}

hipError_t launch_persistent_wt_o4(const GenericArgs &f, int n_slices, unsigned grid, hipStream_t st) {
    switch (f.S) {
        case 4: launch_wt<4>(f, n_slices, grid, st); break;
        case 6: launch_wt<6>(f, n_slices, grid, st); break;
        case 8: launch_wt<8>(f, n_slices, grid, st); break;
        case 10: launch_wt<10>(f, n_slices, grid, st); break;
        case 12: launch_wt<12>(f, n_slices, grid, st); break;
        case 14: launch_wt<14>(f, n_slices, grid, st); break;
        case 16: launch_wt<16>(f, n_slices, grid, st); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace fixedk
}  // namespace csp
