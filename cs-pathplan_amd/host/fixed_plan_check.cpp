// fixed_plan_check.cpp -- prints the launch plan of the fixed-size solve kernels (cs-pathplan_amd/csrc/minsnap_fixed_plan.h)
// for one shape, as one line of key=value pairs: the same functions launch_s / launch_path_s execute, driven on a CPU by
// tests/test_fixed_plan.py.  The five override strings are CSP_SLICE_W, CSP_AXIS_LANES, CSP_NT_STORES, CSP_STORE_POLICY and
// CSP_PATH_STAGGER in that order; "-" stands for an unset variable (nothing is read from the environment).
// usage: fixed_plan_check solve order S B cus flags  w axis nt policy stagger     flags: letters of "spbvm" or "-"
//                                                      (segment-major, persistent, bc per trajectory, weight per trajectory, multi)
//        fixed_plan_check path  order S B              w axis nt policy stagger
//        fixed_plan_check env                          w axis nt policy stagger
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/minsnap_fixed_plan.h"

using namespace csp::fixedk;

static const char *opt(const char *s) { return std::strcmp(s, "-") == 0 ? nullptr : s; }
static const char *store_name(int sp) { return sp == SP_WT ? "wt" : sp == SP_NT ? "nt" : sp == SP_PLAIN ? "plain" : "?"; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const bool solve = std::strcmp(argv[1], "solve") == 0, path = std::strcmp(argv[1], "path") == 0, envonly = std::strcmp(argv[1], "env") == 0;
    const int first_env = solve ? 7 : path ? 5 : 2;
    if (!(solve || path || envonly) || argc != first_env + 5) return 2;
    char **e = argv + first_env;
    const FixedEnv env = parse_fixed_env(opt(e[0]), opt(e[1]), opt(e[2]), opt(e[3]), opt(e[4]));
    if (envonly) {
        std::printf("slice_w=%d axis_lanes=%d nt=%d policy=%s stagger=%d\n", env.slice_w, (int)env.axis_lanes, env.nt,
                    env.policy < 0 ? "unset" : store_name(env.policy), env.stagger);
        return 0;
    }
    const int order = std::atoi(argv[2]), S = std::atoi(argv[3]);
    const long long B = std::atoll(argv[4]);
    if (path) {
        const PathPlan p = plan_fixed_path(order, S, B, env);
        std::printf("grid=%lld nt=%d stagger=%d\n", (long long)p.grid, (int)p.nt, p.stagger);
        return 0;
    }
    const char *fl = argv[6];
    const auto has = [&](char c) { return std::strchr(fl, c) != nullptr; };
    const FixedPlan p = plan_fixed({order, S, B, std::atoi(argv[5]), has('s'), has('p'), has('b'), has('v'), has('m')}, env);
    switch (p.path) {
        case FP_REFUSED: std::printf("path=refused\n"); break;
        case FP_MULTI: std::printf("path=multi slice_w=%d store=plain\n", p.slice_w); break;
        case FP_NARROW: std::printf("path=narrow slice_w=%d axis_lanes=%d grid=%lld store=plain\n", p.slice_w, (int)p.axis_lanes, (long long)p.grid); break;
        case FP_WHOLE:
            std::printf("path=whole n_full=%lld rem=%d grid=%lld body=%s store=%s\n", (long long)p.n_full, p.rem, (long long)p.grid,
                        p.body == FB_PERSISTENT_WT ? "persistent_wt" : p.body == FB_PERSISTENT ? "persistent" : "slice", store_name(p.store));
            break;
    }
    return 0;
}
