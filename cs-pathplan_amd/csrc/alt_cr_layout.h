// alt_cr_layout.h -- where each problem of a cyclic-reduction altitude call keeps its data in the caller's workspace
// (alt.hip: alt_optimize_cr_kernel, alt_global_smooth_cr_kernel).  Plain C++ on purpose: tests/test_alt.py compiles it on
// the CPU (cs-pathplan_amd/host/alt_cr_layout_check.cpp) and checks that no region reaches into its neighbour's or past
// the end of the workspace, for every problem length.
//
// Problem b of n samples starting at sample o owns the doubles [14 o + CR_PAD b, 14 (o + n) + CR_PAD (b + 1)):
//     x      2 N2 + 2   the solution (N2 = ceil(n / 2) block rows of two samples)
//     store  13 N2      the block rows, when they do not fit in LDS
//     act    n          the active flags of the global smooth
// 15 N2 + 2 + n doubles in all, which is 14 n + 4 for n = 1 and at most 14 n for n >= 2: the CR_PAD doubles per problem
// cover the one-sample problem.  A cyclic-reduction call has at most CR_MAX_BATCH problems, so the pads fit in the
// 4096 bytes of slack that csp_alt_workspace_bytes adds to 14 doubles per sample.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define CSP_ALT_HD __host__ __device__
#else
#define CSP_ALT_HD
#endif

namespace csp {
namespace alt {

constexpr int64_t CR_MAX_BATCH = 64;   // problems per cyclic-reduction call (alt.hip: use_cr)
constexpr int64_t CR_PAD = 8;          // doubles per problem beyond 14 per sample

// offsets in doubles from the workspace's start
struct CrRegion {
    int64_t x, store, act, end;
};

CSP_ALT_HD inline CrRegion cr_region(int64_t o, int64_t b, int64_t n) {
    const int64_t N2 = (n + 1) / 2, start = o * 14 + b * CR_PAD;
    CrRegion r;
    r.x = start;
    r.store = r.x + 2 * N2 + 2;
    r.act = r.store + 13 * N2;
    r.end = r.act + n;
    return r;
}

// the public size (include/csp_alt.h): 4 doubles per sample for the recurrence kernels, 14 per sample + slack for the
// cyclic-reduction ones
inline size_t workspace_bytes(int64_t total_points) { return total_points > 0 ? (size_t)total_points * 14 * 8 + 4096 : 0; }

}  // namespace alt
}  // namespace csp
