// minsnap_eval_plan.h -- tile sizes and LDS bytes of the trajectory evaluation kernels (minsnap_eval.hip), in plain C++:
// the launcher executes these plans and cs-pathplan_amd/host/eval_plan_check.cpp prints them on a CPU
// (tests/test_eval_plan.py).  No HIP in this file.
//
// Both kernels give a workgroup of EVAL_THREADS lanes a tile of `tb` consecutive trajectories.  Their prefix sums of
// the segment times live in LDS, one row of smax + 1 doubles per trajectory.
//   forward: one lane per (trajectory, query) of the tile; nothing else is kept in LDS.
//   reverse: the tile's segments are numbered f = tl * smax + j and cut into blocks of EVAL_BLOCK_SEGS; one lane per
//            (segment of the block, axis) owns that record's accumulators in registers.  Queries pass through LDS in
//            tiles of `qt` per trajectory: local time, the query's term of grad_times and its segment key.
#pragma once
#include <cstddef>
#include <cstdint>

namespace csp {
namespace evalk {

constexpr int EVAL_THREADS = 256;
constexpr int EVAL_BLOCK_SEGS = 85;          // 85 segments x 3 axes = 255 record lanes
constexpr int EVAL_MAX_SEGMENTS = 1024;
constexpr int EVAL_MAX_DERIVS = 5;
constexpr int EVAL_QUERY_SLOTS = 2048;       // reverse: queries of a tile held in LDS at once (all trajectories together)
constexpr int EVAL_FWD_TILE_SEGS = 1024;     // forward: tb * smax stays at or below this
constexpr size_t EVAL_LDS_LIMIT = 163840;    // what one CU has

struct EvalPlan {
    int tb;            // trajectories per workgroup
    int qt;            // reverse only: queries per trajectory and LDS tile (0: forward, or no query)
    int blocks;        // reverse only: segment blocks per tile
    size_t lds_bytes;  // dynamic LDS of the launch
    int64_t grid;      // workgroups
};

inline bool eval_supported(int order, int smax) { return order >= 2 && order <= 5 && smax >= 1 && smax <= EVAL_MAX_SEGMENTS; }

// LDS layout, in this order (every array starts on a multiple of 8 bytes):
//   double  cum[tb][smax + 1]
//   int64   seg_base[tb]        first record of the trajectory
//   int32   nseg[tb], bad[tb], stat[tb]   (+ 4 bytes of padding when tb is odd)
// reverse adds
//   double  seg_sum[tb][smax], hi_sum[tb]
//   double  tau[tb * qt], gt[tb * qt];  int32 key[tb * qt]
inline size_t eval_lds_common(int tb, int smax) {
    const size_t ints = ((size_t)3 * tb + 1) / 2 * 2;
    return (size_t)tb * (smax + 1) * 8 + (size_t)tb * 8 + ints * 4;
}

inline EvalPlan plan_eval_forward(int smax, int64_t B) {
    EvalPlan p{};
    int tb = EVAL_FWD_TILE_SEGS / smax;
    p.tb = tb < 1 ? 1 : (tb > 64 ? 64 : tb);
    p.qt = 0;
    p.blocks = 0;
    p.lds_bytes = eval_lds_common(p.tb, smax);
    p.grid = (B + p.tb - 1) / p.tb;
    return p;
}

inline EvalPlan plan_eval_vjp(int smax, int64_t Q, int64_t B) {
    EvalPlan p{};
    int tb = EVAL_BLOCK_SEGS / smax;
    p.tb = tb < 1 ? 1 : (tb > 64 ? 64 : tb);
    const int64_t cap = EVAL_QUERY_SLOTS / p.tb;
    p.qt = (int)(Q < cap ? Q : cap);
    p.blocks = (p.tb * smax + EVAL_BLOCK_SEGS - 1) / EVAL_BLOCK_SEGS;
    const size_t slots = (((size_t)p.tb * p.qt) + 1) / 2 * 2;
    p.lds_bytes = eval_lds_common(p.tb, smax) + ((size_t)p.tb * smax + p.tb) * 8 + slots * 20;
    p.grid = (B + p.tb - 1) / p.tb;
    return p;
}

}  // namespace evalk
}  // namespace csp
