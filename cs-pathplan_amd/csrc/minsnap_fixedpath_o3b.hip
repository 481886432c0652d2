// minsnap_fixedpath_o3b.hip -- instantiates the register-resident path-penalty kernels
// (minsnap_fixed_path_impl.h) for derivative order 3, S = 12..16 segments.
#include "minsnap_fixed_path_impl.h"

namespace csp {

hipError_t launch_fixedpath_o3b(const GenericArgs &a, hipStream_t st) {
    switch (a.S) {
        case 12: return fixedk::launch_path_s<3, 12>(a, st);
        case 13: return fixedk::launch_path_s<3, 13>(a, st);
        case 14: return fixedk::launch_path_s<3, 14>(a, st);
        case 15: return fixedk::launch_path_s<3, 15>(a, st);
        case 16: return fixedk::launch_path_s<3, 16>(a, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace csp
