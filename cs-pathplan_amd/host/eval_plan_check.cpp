// eval_plan_check.cpp -- prints the launch plans of the trajectory evaluation kernels (cs-pathplan_amd/csrc/minsnap_eval_plan.h)
// as key=value pairs: the same functions launch_eval / launch_eval_vjp execute, driven on a CPU by tests/test_eval_plan.py.
// usage: eval_plan_check plan  smax Q B     one shape: the forward and the reverse plan
//        eval_plan_check sweep              every smax in 1..1024 against every Q in 0..4200 and a few huge ones: the
//                                           extremes of the tile sizes and of the LDS bytes (the plans do not depend on
//                                           the order: no array in LDS is sized by it)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/minsnap_eval_plan.h"

using namespace csp::evalk;

int main(int argc, char **argv) {
    if (argc == 5 && std::strcmp(argv[1], "plan") == 0) {
        const int smax = std::atoi(argv[2]);
        const long long Q = std::atoll(argv[3]), B = std::atoll(argv[4]);
        const EvalPlan f = plan_eval_forward(smax, B), v = plan_eval_vjp(smax, Q, B);
        std::printf("fwd_tb=%d fwd_lds=%zu fwd_grid=%lld vjp_tb=%d vjp_qt=%d vjp_blocks=%d vjp_lds=%zu vjp_grid=%lld\n", f.tb,
                    f.lds_bytes, (long long)f.grid, v.tb, v.qt, v.blocks, v.lds_bytes, (long long)v.grid);
        return 0;
    }
    if (argc == 2 && std::strcmp(argv[1], "sweep") == 0) {
        size_t max_lds = 0;
        int min_tb = 1 << 30, min_qt = 1 << 30, max_slots = 0, max_record_lanes = 0, bad = 0;
        const long long huge[] = {65536, 1LL << 31, (1LL << 31) + 1, 1LL << 40, 9223372036854775807LL};
        for (int order = 2; order <= 5; ++order) {
            for (int smax = 1; smax <= EVAL_MAX_SEGMENTS; ++smax) {
                if (!eval_supported(order, smax)) ++bad;
                const EvalPlan f = plan_eval_forward(smax, 65);
                if (f.lds_bytes > max_lds) max_lds = f.lds_bytes;
                if (f.tb < min_tb) min_tb = f.tb;
                if (f.grid * f.tb < 65) ++bad;
                for (long long qi = 0; qi <= 4200 + 5; ++qi) {
                    const long long Q = qi <= 4200 ? qi : huge[qi - 4201];
                    const EvalPlan v = plan_eval_vjp(smax, Q, 65);
                    if (v.lds_bytes > max_lds) max_lds = v.lds_bytes;
                    if (v.tb < min_tb) min_tb = v.tb;
                    if (Q > 0 && v.qt < min_qt) min_qt = v.qt;
                    if (v.tb * v.qt > max_slots) max_slots = v.tb * v.qt;
                    if (v.qt > Q || (Q > 0 && v.qt < 1) || v.grid * v.tb < 65) ++bad;
                    // every segment of the tile has a record lane in some block, and a block fits the workgroup
                    if (v.blocks * EVAL_BLOCK_SEGS < v.tb * smax) ++bad;
                    const int lanes = 3 * (v.tb * smax < EVAL_BLOCK_SEGS ? v.tb * smax : EVAL_BLOCK_SEGS);
                    if (lanes > max_record_lanes) max_record_lanes = lanes;
                }
            }
        }
        std::printf("max_lds=%zu min_tb=%d min_qt=%d max_slots=%d max_record_lanes=%d threads=%d bad=%d\n", max_lds, min_tb, min_qt,
                    max_slots, max_record_lanes, EVAL_THREADS, bad);
        return 0;
    }
    return 2;
}
