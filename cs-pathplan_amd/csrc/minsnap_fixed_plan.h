// minsnap_fixed_plan.h -- which variant a launch of the register-resident fixed-size kernels takes (minsnap_fixed_impl.h,
// minsnap_fixed_path_impl.h): slice width, lane mapping, grid, kernel body and store flavour, from the launch's shape and
// five environment overrides.  Plain C++17 without HIP: the launchers (launch_s, launch_path_s) only execute a plan, and
// host/fixed_plan_check.cpp drives the same functions from tests/test_fixed_plan.py on a CPU.  Every threshold of these
// launchers lives here, next to the measurement that set it.
#pragma once
#include <cstdint>
#include <cstdlib>

namespace csp {
namespace fixedk {

// Store policy of a full-slice kernel's coefficient stores, a compile-time property of the instantiation: ordinary,
// non-temporal, or (values >= 16) write-through with that value as the buffer store's cache bits.
constexpr int SP_PLAIN = 0, SP_NT = 1, SP_WT = 16;

// ---- the overrides (tuning and A/B runs) -----------------------------------------------------------------------------
struct FixedEnv {
    int slice_w = 0;          // CSP_SLICE_W: 8, 16, 32 or 64 (even: 16-byte pieces stay aligned); anything else = 0 = unset
    bool axis_lanes = true;   // CSP_AXIS_LANES: off only when the first character is '0'
    int nt = -1;              // CSP_NT_STORES: unset -1, first character '0' -> 0, anything else 1
    int policy = -1;          // CSP_STORE_POLICY: unset -1, else by first character 'w' SP_WT, 'n' SP_NT, anything else SP_PLAIN
    int stagger = -1;         // CSP_PATH_STAGGER: atoi; used when >= 0
};
inline FixedEnv parse_fixed_env(const char *slice_w, const char *axis_lanes, const char *nt, const char *policy, const char *stagger) {
    FixedEnv e;
    const int w = slice_w ? std::atoi(slice_w) : 0;
    if (w == 8 || w == 16 || w == 32 || w == 64) e.slice_w = w;
    e.axis_lanes = !(axis_lanes && axis_lanes[0] == '0');
    if (nt) e.nt = nt[0] == '0' ? 0 : 1;
    if (policy) e.policy = policy[0] == 'w' ? SP_WT : (policy[0] == 'n' ? SP_NT : SP_PLAIN);
    if (stagger) e.stagger = std::atoi(stagger);
    return e;
}
// read once per process, at the first launch (tools and tests set the variables in child processes for that reason)
inline const FixedEnv &fixed_env() {
    static const FixedEnv e = parse_fixed_env(std::getenv("CSP_SLICE_W"), std::getenv("CSP_AXIS_LANES"), std::getenv("CSP_NT_STORES"),
                                              std::getenv("CSP_STORE_POLICY"), std::getenv("CSP_PATH_STAGGER"));
    return e;
}

// ---- shape predicates and thresholds ---------------------------------------------------------------------------------
// Trajectories start on 128-byte lines (records of 48 * O bytes): what the whole-line rings (LineGeom) need.
constexpr bool starts_on_lines(int O, int S) { return (S * 48 * O) % 128 == 0; }
// Paired order-4 records, whose every store instruction writes whole lines: the shapes that have a write-through kernel.
constexpr bool wt_shape(int O, int S) { return O == 4 && S >= 4 && S % 2 == 0; }
// Dense residency of the path kernel (order 2, S >= 8): under 40 KB of LDS and 256 registers, so that FOUR workgroups
// share a CU.
constexpr bool path_dense(int O, int S) { return O == 2 && S >= 8; }
// segment-major output ([S][B][3][2o]) is instantiated for order 4 only
constexpr bool seg_major_order(int O) { return O == 4; }
// Coefficients a launch writes, from the WHOLE batch (tail included).
inline double coeff_bytes(int O, int S, int64_t B) { return (double)B * S * 6 * O * 8.0; }
// The chip's aggregate L2 (8 x 4 MiB): up to here stores stay ordinary whatever a sweep says -- a
// following kernel (the sampler after a plan) still finds those lines in L2.
constexpr double L2_BYTES = 32.0 * 1024 * 1024;
// The Infinity Cache: above it non-temporal stores win -- B = 524288, order 4, S = 16: 348 us against 378 us (67.9 % against
// 62.5 % of HBM peak); at B = 65536, whose 201 MB the cache absorbs, the ordinary store is the faster one (42.5 us against
// 46.1 us).  Between the two sizes write-through wins where it exists (sweep in DESIGN.md 5.1.2; crossover between 192
// and 288 MiB).
constexpr double INFINITY_CACHE_BYTES = 256.0 * 1024 * 1024;
// Path kernels: non-temporal stores FROM this size on.  Measured at order 4, S = 16 (tools/path_nt_ab.py; three boxes):
// B = 16384 / 32768 / 65536 / 98304 / 131072 / 262144 / 524288: 40.7 / 45.1 / 93-95 / 145 / 188 / 368 / 723 us against 44.1 /
// 49.3 / 95.5-97.6 / 163 / 214 / 419 / 817 us with ordinary stores, and WRITE_SIZE 1.013x the coefficients instead of 1.083x:
// unlike the unpenalised kernel this one computes for most of its time and gains from lines that leave whole.  Launches
// that write less keep ordinary stores: nothing measurable to gain (B = 8192: 40.2 against 40.6 us; one order-4 flight
// through the host C-ABI: 1167-1186 us either way), and the reader that follows a small solve (the sampler) then finds
// the coefficients in the cache.
constexpr double PATH_NT_FROM_BYTES = 48.0 * 1024 * 1024;

// ---- the unpenalised kernels (launch_s) ------------------------------------------------------------------------------
struct FixedShape {
    int order, S;
    int64_t B;          // ignored by a multi-batch launch
    int cus;
    bool seg_major, persistent, bc_per_traj, vw_per;
    bool multi;         // csp_minsnap_solve_multi: many batches in one grid
};
enum FixedPath {
    FP_REFUSED,   // segment-major output at an order that has no such instantiation
    FP_MULTI,     // every batch cut into slices of 64, one workgroup per slice, all of them in one grid (taken from the table)
    FP_NARROW,    // one launch of slices of slice_w < 64 trajectories
    FP_WHOLE      // n_full slices of 64 (body, store, grid) plus one workgroup for the last rem trajectories
};
enum FixedBody { FB_SLICE, FB_PERSISTENT, FB_PERSISTENT_WT };   // one workgroup per slice / persistent / persistent, write-through
struct FixedPlan {
    FixedPath path = FP_WHOLE;
    int slice_w = 64;           // FP_MULTI, FP_NARROW: trajectories per workgroup
    bool axis_lanes = false;    // FP_NARROW: three lanes per trajectory, one per axis (fixed_body NAX = 1)
    int64_t grid = 0;           // FP_NARROW: its workgroups; FP_WHOLE: those of the whole-slice launch
    int64_t n_full = 0;         // FP_WHOLE
    int rem = 0;                // FP_WHOLE: trajectories of the tail (ordinary stores, like FP_MULTI and FP_NARROW)
    FixedBody body = FB_SLICE;  // FP_WHOLE: kernel of the whole slices ...
    int store = SP_PLAIN;       // ... and its store flavour
};

inline FixedPlan plan_fixed(const FixedShape &s, const FixedEnv &env) {
    FixedPlan p;
    if (s.multi) { p.path = FP_MULTI; return p; }
    // Trajectories per workgroup.  A small batch is latency-bound -- a lone wave's instruction stream is the run time -- so
    // what helps is fewer instructions per lane, not more workgroups: with the three-lanes-per-trajectory mapping (order 4)
    // batches of B <= 32 * CUs trajectories run as slices of 16 (measured, B = 4096, S = 8: 8.2 us one lane per trajectory in
    // slices of 64, 7.9 us in slices of 16, 6.1 us with three lanes per trajectory; B = 8192: 9.3 -> 8.8 us).  Everything
    // else keeps 64.  A forced width is honoured at every order, but never under segment-major.
    const bool axis_ok = s.order == 4 && !s.seg_major && env.axis_lanes;
    const int w = env.slice_w ? env.slice_w : (axis_ok && s.B <= 32 * (int64_t)s.cus) ? 16 : 64;
    if (w < 64 && !s.seg_major) {
        p.path = FP_NARROW;
        p.slice_w = w;
        p.axis_lanes = axis_ok && w <= 16;
        p.grid = (s.B + w - 1) / w;
        return p;
    }
    if (s.seg_major && !seg_major_order(s.order)) { p.path = FP_REFUSED; return p; }
    p.n_full = s.B / 64;
    p.rem = (int)(s.B % 64);
    // The persistent kernel reads boundary conditions and weight once, before its slice loop: per-trajectory ones take the
    // one-workgroup-per-slice kernel.  Persistent grid: two workgroups per CU.
    const bool persistent = s.persistent && !s.bc_per_traj && !s.vw_per;
    p.body = persistent ? FB_PERSISTENT : FB_SLICE;
    p.grid = persistent && 2 * (int64_t)s.cus < p.n_full ? 2 * (int64_t)s.cus : p.n_full;
    const double bytes = coeff_bytes(s.order, s.S, s.B);
    const int by_size = bytes > INFINITY_CACHE_BYTES ? SP_NT : SP_PLAIN;
    const int by_nt_env = env.nt >= 0 ? (env.nt ? SP_NT : SP_PLAIN) : by_size;
    if (wt_shape(s.order, s.S) && !s.seg_major) {
        // Three-way rule, for the shapes with a write-through kernel alone: CSP_STORE_POLICY, then CSP_NT_STORES, then
        // write-through between the L2 and the Infinity Cache.  Write-through (chosen or forced) that meets the
        // one-workgroup-per-slice kernel stores ordinarily.
        p.store = env.policy >= 0 ? env.policy : (env.nt < 0 && bytes > L2_BYTES && bytes <= INFINITY_CACHE_BYTES) ? SP_WT : by_nt_env;
        if (p.store == SP_WT) {
            if (persistent) p.body = FB_PERSISTENT_WT;
            else p.store = SP_PLAIN;
        }
    } else if (s.order == 4 || starts_on_lines(s.order, s.S)) {
        // Non-temporal stores need lines that leave whole: order 4 (paired 192-byte records) and every order whose
        // trajectories start on 128-byte lines (LineRing).  Order-4 segment-major and odd S keep the rule although they
        // have no whole lines.
        p.store = by_nt_env;
    } else {
        // Record-at-a-time stores of 96- / 144- / 240-byte records share lines between instructions, which the L2 merges for
        // ordinary stores and not for non-temporal ones (B = 524288: 261 / 392 / 312 us ordinary against 499 / 841 / 404 us
        // non-temporal): only CSP_NT_STORES=1 asks for them.
        p.store = env.nt == 1 ? SP_NT : SP_PLAIN;
    }
    return p;
}

// ---- the path-penalty kernels (launch_path_s): one workgroup per slice of 64 ------------------------------------------
struct PathPlan {
    int64_t grid;
    bool nt;       // non-temporal coefficient stores
    int stagger;   // GenericArgs::stagger
};
inline PathPlan plan_fixed_path(int order, int S, int64_t B, const FixedEnv &env) {
    PathPlan p;
    p.grid = (B + 63) / 64;
    // Whole lines leave at order 4 and wherever the trajectories start on lines (LineRing; the dense order-2 variant's
    // HalfRing included).  Without them orders 2 and 3 LOSE with non-temporal stores at every size (B = 524288: 503 against
    // 306 us, 876 against 620 us): a non-temporal partial line is not merged on the way out.
    const bool whole_lines = order == 4 || starts_on_lines(order, S);
    p.nt = env.nt >= 0 ? env.nt != 0 : whole_lines && coeff_bytes(order, S, B) >= PATH_NT_FROM_BYTES;
    // Start delay between the workgroups that share a CU, so that one's store phase meets the other's compute.  Measured at
    // B = 65536, S = 16 (tools/path_bench.py, CSP_PATH_STAGGER = 0 / 1 / 2 / 3 / 4 / 6): order 3 58.4 / 57.3 / 57.7 / 61.0 / 65.5 /
    // 76.7 us, order 4 86.4 / 85.0 / 86.8 / 84.0 / 86.2 / 95.7 us -- a 2-3 % effect; scaled with the sweep length.  Dense order-2
    // variant (the four workgroups of a CU start stagger x S x 64 clocks apart), CSP_PATH_STAGGER = 0 / 2 / 3 / 4 / 5 / 6 / 8:
    // 33.2 / 30.6 / 30.2 / 30.3 / 30.3 / 30.8 / 32.1 us.
    p.stagger = env.stagger >= 0 ? env.stagger : path_dense(order, S) ? 4 : order == 3 ? (S + 8) / 16 : order == 4 ? (3 * S + 8) / 16 : 0;
    return p;
}

}  // namespace fixedk
}  // namespace csp
