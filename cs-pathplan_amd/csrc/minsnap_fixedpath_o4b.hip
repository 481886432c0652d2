// minsnap_fixedpath_o4b.hip -- instantiates the register-resident path-penalty kernels
// (minsnap_fixed_path_impl.h) for derivative order 4, S = 14..16 segments (10..13: minsnap_fixedpath_o4c.hip).
#include "minsnap_fixed_path_impl.h"

namespace csp {

hipError_t launch_fixedpath_o4b(const GenericArgs &a, hipStream_t st) {
    switch (a.S) {
        case 14: return fixedk::launch_path_s<4, 14>(a, st);
        case 15: return fixedk::launch_path_s<4, 15>(a, st);
        case 16: return fixedk::launch_path_s<4, 16>(a, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace csp
