// minsnap_fixed_o4c.hip -- instantiates the register-resident fixed-size kernels
// (minsnap_fixed_impl.h) for derivative order 4 (polynomial degree 7), S = 10..13 segments.
#include "minsnap_fixed_impl.h"

namespace csp {

hipError_t launch_fixed_o4c(const GenericArgs &a, int cus, hipStream_t st) {
    switch (a.S) {
        case 10: return fixedk::launch_s<4, 10, true>(a, cus, st);
        case 11: return fixedk::launch_s<4, 11, true>(a, cus, st);
        case 12: return fixedk::launch_s<4, 12, true>(a, cus, st);
        case 13: return fixedk::launch_s<4, 13, true>(a, cus, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace csp
