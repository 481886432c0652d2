/*
 * csp_minsnap.h -- C-ABI of the MI355X-native batched minimum-snap solver.
 *
 * This is the drop-in boundary for ONE hot path of MEZHANGYUE/CS-PathPlan: the closed-form
 * minimum-snap QP behind `TrajectoryGeneratorTool` (reference interface:
 * math_util/minimum_snap.hpp:36-63; implementation math_util/minimum_snap.cpp:22-649).
 * The reference is a C++ class with Eigen types in its signatures; a C++ shim with the same
 * class surface (cs-pathplan_amd/host/math_util/minimum_snap.hpp) forwards to the entry points below, so
 * `UavPathPlanner::Minisnap_3D/Minisnap_EN` (uavPathPlanning.cpp:4401-4474) compile unchanged.
 * See INTEGRATION.md for the binding a reference maintainer would add.
 *
 * Conventions shared by every entry point
 *   - plain pointers and sizes only; caller owns every buffer; nothing throws across the ABI;
 *   - return value: CSP_OK (0) or a negative csp_status; per-trajectory problems are reported
 *     through the optional `status` array, never by aborting the batch;
 *   - silent: nothing is printed (the reference prints inside the solver);
 *   - thread-safe for distinct streams; no global mutable state besides the lazily built
 *     constant tables and the pool of staging arenas host-memory calls borrow from (mutex-protected);
 *   - the compute path is HIP on gfx950 only.  There is NO CPU fallback: without a usable
 *     device the calls return CSP_ERR_NO_DEVICE.
 *
 * Data layout (all row-major, contiguous; device pointers 16-byte aligned -- hipMalloc and torch
 * allocations are -- or pass CSP_FLAG_FORCE_GENERIC)
 *   waypoints : [B][S+1][3]   positions (reference `Path`, W x 3, minimum_snap.hpp:47)
 *   times     : [B][S]        segment durations (reference `Time`, minimum_snap.hpp:50)
 *   bc        : [B or 1][4][3] rows = start vel, end vel, start acc, end acc
 *                             (reference `Vel` 2x3 and `Acc` 2x3, minimum_snap.hpp:48-49)
 *   coeffs    : [B][S][3][2*order]  polynomial coefficients per segment and axis, HIGHEST power
 *               first, local time t in [0, T_seg] -- the row-major image of the reference's
 *               PolyCoeff (S x 3*p_num1d, minimum_snap.cpp:220-223, :626-648)
 *   ragged batches (num_segments == 0): trajectories are concatenated; trajectory b owns
 *               segments seg_offsets[b] .. seg_offsets[b+1]-1 of `times`/`coeffs` and waypoints
 *               seg_offsets[b]+b .. seg_offsets[b+1]+b of `waypoints`.
 *
 * Accuracy and the spread of segment times.  The problem's conditioning grows with
 * R = max T / min T inside one trajectory like R^(2*order-1).  Measured per coefficient power against a 40-digit solve,
 * fp64: with R <= 16 every open-chain entry point stays within 1e-9 up to order 4 and 4e-8 at order 5 (a plain fp64 CPU
 * solver: 7e-10 / 2e-7); with R = 256 on constant-speed legs 2e-10 at order 3 and 8e-7 at order 4 (CPU: 6e-10 / 1e-6).  A
 * trajectory whose short segments sit between long ones with no boundary derivative beside them is worse for every fp64
 * method (2e-5 at order 5, R = 16), and order 5 with R in the hundreds is outside what fp64 can solve, by any method.
 * The periodic solve pins no derivative at all and loses more: with R = 16 up to 5e-9 at order 4 and 1e-5 at order 5
 * (coefficients, cost and time gradient alike); keep R <= 4 there for order 5 (1e-8), or use orders <= 3 (3e-12).
 * The gradient, cost and knot-constraint entries (error of a gradient: its largest error over its
 * largest entry per trajectory, the time gradient also weighted by T): with R <= 16 the open-chain reverse mode stays within
 * 3e-14 / 2e-13 / 2e-10 / 1e-8 at orders 2 / 3 / 4 / 5, the cost within 5e-10 and its time gradient within 2e-9 at order 5
 * (2e-12 / 9e-12 at order 4), the knot-constrained coefficients within 3e-9 at order 4 and 5e-6 at order 5 -- all within
 * 1.3 x a careful plain fp64 CPU solve.  With R = 256 on constant-speed legs the reverse mode and the cost entry, which
 * form their right-hand sides from the legs, reach 2e-9 at order 3 and 3e-7 at order 4 (gradients, within 7 x the CPU
 * solve) and 1e-10 / 7e-8 (the cost's time gradient).  The periodic reverse mode follows the
 * periodic solve: 3e-9 up to order 4, 4e-5 at order 5 with R = 16.
 */
#ifndef CSP_MINSNAP_H_
#define CSP_MINSNAP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSP_MINSNAP_ABI_VERSION 1u

typedef enum csp_status {
    CSP_OK = 0,
    CSP_ERR_INVALID_ARG = -1, /* null pointer, bad order/segment count, bad abi_version      */
    CSP_ERR_UNSUPPORTED = -2, /* order outside 1..5 (the reference's int arithmetic overflows
                                 from order 6, minimum_snap.cpp:321-323)                      */
    CSP_ERR_WORKSPACE = -3,   /* workspace missing or smaller than csp_minsnap_workspace_bytes */
    CSP_ERR_HIP = -4,         /* a HIP runtime call failed; see csp_minsnap_last_hip_error    */
    CSP_ERR_NO_DEVICE = -5    /* no gfx950 device visible -- there is no CPU fallback         */
} csp_status;

enum { CSP_DTYPE_F64 = 0, CSP_DTYPE_F32 = 1 };
enum { CSP_MEM_HOST = 0, CSP_MEM_DEVICE = 1 };

/* flags */
#define CSP_FLAG_FORCE_GENERIC 0x1u /* never dispatch the register-resident fixed-size kernel */
#define CSP_FLAG_SEGMENT_MAJOR 0x2u /* uniform batches only: coeffs laid out [S][B][3][2*order]
                                       (segment-major) instead of [B][S][3][2*order]; each
                                       (segment, trajectory) record keeps the reference's row
                                       content (3*p_num1d values, highest power first) */

#define CSP_FLAG_F32_ARITH 0x8u      /* CSP_DTYPE_F32 only: compute in fp32 too.  By default fp32 is
                                       the STORAGE type and the arithmetic is fp64 (pure fp32 loses
                                       3..5 digits at order 4..5) */
#define CSP_FLAG_LONG_SEGMENTS 0x10u /* csp_minsnap_sample_batch with device memory: segments hold hundreds of
                                       0.1-s candidates each (long legs): sample with one wave per trajectory.
                                       Host-memory calls decide this themselves from the times. */
#define CSP_FLAG_SPAN 0x20u          /* 16 < S <= 256: use the 16-segments-per-lane kernel (the default beyond 256
                                       segments) instead of the 4-segments-per-lane one (A/B testing) */
#define CSP_FLAG_NO_PERSISTENT 0x4u  /* fixed kernel: one workgroup per 64 trajectories instead of
                                       persistent workgroups with LDS-DMA prefetch (A/B testing) */

/* per-trajectory status bits written to `status` */
#define CSP_TRAJ_OK 0
#define CSP_TRAJ_NONFINITE 1   /* a coefficient is inf/NaN (the reference would return it silently).  The register-resident
                                  kernels (uniform S <= 16, with or without the path penalty) test the highest-power and
                                  the constant coefficient of every record -- every input and unknown of the segment
                                  enters the former, the latter is the start waypoint --, so an inf/NaN that ARISES in a
                                  middle coefficient alone (finite inputs of magnitude >~ 1e300) is not flagged there; the
                                  chunked, span and generic kernels test every stored coefficient                       */
#define CSP_TRAJ_NOT_SPD 2     /* a pivot of the free-derivative Hessian R_PP was <= 0              */
#define CSP_TRAJ_SKIPPED 4     /* csp_minsnap_solve_mixed (and a device-memory csp_minsnap_eval_batch[_vjp] given a ragged length outside
                                  0..max_segments): the trajectory was NOT solved (its order is outside 2..5
                                  or its segment count outside 1..min(256, max_segments)); its coefficient block is left untouched (zero-filled with CSP_MEM_HOST) */
#define CSP_TRAJ_NOT_CONVERGED 8 /* csp_minsnap_optimize_times[_knots|_periodic]_batch only: the stopping rule was not met (max_iters reached, or
                                  no decrease within rounding); the times returned are the last accepted ones          */

typedef struct csp_minsnap_desc {
    uint32_t abi_version;       /* CSP_MINSNAP_ABI_VERSION                                       */
    uint32_t dtype;             /* CSP_DTYPE_F64 | CSP_DTYPE_F32: STORAGE type of waypoints/times/bc/coeffs */
    int32_t order;              /* derivative order d_order (reference `order`): 4 = min-snap,
                                   polynomial degree 2*order-1 (minimum_snap.cpp:237-238)         */
    int32_t num_segments;       /* uniform S >= 1, or 0 for a ragged batch                         */
    int64_t batch;              /* B >= 0                                                          */
    const int64_t *seg_offsets; /* ragged only: [B+1] prefix sums, same memory space as the data   */
    int32_t max_segments;       /* ragged only: max_b S_b (sizes the workspace)                    */
    uint32_t bc_per_trajectory; /* 0: bc is [1][4][3] shared by the batch; 1: [B][4][3]            */
    double path_weight;         /* reference `path_weight` (minimum_snap.cpp:233, :347-469)        */
    double vel_zero_weight;     /* reference `vel_zero_weight` (:234, :473-509)                    */
    const double *vel_zero_weight_per_traj; /* optional [B] (always f64) overriding the scalar;
                                   used by the batched re-solve loop (minimum_snap.cpp:80-90)      */
    uint32_t mem_space;         /* CSP_MEM_HOST: pointers are host memory, the call stages through
                                   the device and is synchronous; CSP_MEM_DEVICE: device pointers,
                                   the call only enqueues work on `hip_stream`                     */
    int32_t device_id;          /* HIP device ordinal; -1 = current device                         */
    uint32_t flags;
    uint32_t reserved;
} csp_minsnap_desc;

/* Replaces TrajectoryGeneratorTool::SolveQPClosedForm (math_util/minimum_snap.hpp:45-53,
 * minimum_snap.cpp:227-649) for a batch of independent trajectories.
 *   max_dev : optional [B] f64, the reference's *max_deviation out-parameter per trajectory
 *   status  : optional [B] i32, CSP_TRAJ_* bits
 *   workspace / workspace_bytes : device scratch of at least csp_minsnap_workspace_bytes(desc)
 *             bytes (CSP_MEM_DEVICE); may be NULL/0 with CSP_MEM_HOST (carved from the cached arena)
 *   hip_stream : hipStream_t (NULL = default stream) */
int csp_minsnap_solve_batch(const csp_minsnap_desc *desc, const void *waypoints, const void *times,
                            const void *bc, void *coeffs, double *max_dev, int32_t *status,
                            void *workspace, size_t workspace_bytes, void *hip_stream);

/* Device scratch bytes the call above needs for `desc` (0 when the fixed-size kernel serves it). */
size_t csp_minsnap_workspace_bytes(const csp_minsnap_desc *desc);

/* Reverse mode of csp_minsnap_solve_batch: the vector-Jacobian product.  Given grad_coeffs = dL/dcoeffs, writes
 * dL/dwaypoints, dL/dtimes and dL/dbc.  The primal is re-solved from waypoints / times / bc in the
 * same block-LDL^T sweep that solves the adjoint system (the forward's coefficients are not read), one lane per
 * trajectory, the factors in `workspace`.  Results are deterministic run to run (no atomics).
 *   desc          : as for csp_minsnap_solve_batch; orders 2..5, uniform or ragged, CSP_DTYPE_F64 or CSP_DTYPE_F32
 *                   (fp32 storage, fp64 arithmetic), vel_zero_weight(_per_traj).  CSP_ERR_UNSUPPORTED for
 *                   path_weight != 0, order 1, CSP_FLAG_SEGMENT_MAJOR and CSP_FLAG_F32_ARITH.  Gradients with respect
 *                   to the weights are not computed.
 *   grad_coeffs   : [B][S][3][2*order] (trajectory-major, the layout of `coeffs`); 16-byte aligned (fp64) / 8-byte (fp32)
 *   grad_waypoints: optional out, the layout of `waypoints`
 *   grad_times    : optional out, the layout of `times`
 *   grad_bc       : optional out, the shape of `bc`: [B][4][3] per trajectory, or [1][4][3] summed over the batch
 *                   (in a fixed order).  Rows the order does not use (acceleration at order 2) are zero.
 *   status        : optional [B] i32: CSP_TRAJ_NOT_SPD (a pivot <= 0), CSP_TRAJ_NONFINITE (a gradient this trajectory
 *                   writes is inf/NaN)
 *   workspace     : device scratch of csp_minsnap_vjp_workspace_bytes(desc) bytes (CSP_MEM_DEVICE, 8-byte aligned);
 *                   may be NULL/0 with CSP_MEM_HOST.  With o = order, Smax = num_segments (uniform) or max_segments
 *                   (ragged):
 *                     round_up_256((Smax - 1) * ((o-1)^2 + 6(o-1)) * B * 8)
 *                       + (bc_per_trajectory ? 0 : 12 * ceil(B / 64) * 8)
 * CSP_MEM_HOST: staged through the cached arena, synchronous.  CSP_MEM_DEVICE: asynchronous on `hip_stream`. */
int csp_minsnap_solve_batch_vjp(const csp_minsnap_desc *desc, const void *waypoints, const void *times,
                                const void *bc, const void *grad_coeffs, void *grad_waypoints,
                                void *grad_times, void *grad_bc, int32_t *status,
                                void *workspace, size_t workspace_bytes, void *hip_stream);
/* Device scratch bytes csp_minsnap_solve_batch_vjp needs for `desc` (formula above; 0 for an invalid or unsupported
 * descriptor). */
size_t csp_minsnap_vjp_workspace_bytes(const csp_minsnap_desc *desc);

/* Reverse mode of (coeffs, J) = csp_minsnap_solve_batch + csp_minsnap_cost_batch: csp_minsnap_solve_batch_vjp with a
 * second cotangent grad_cost = dL/dJ.  J is the snap cost of csp_minsnap_cost_batch at the optimum; by
 * the envelope theorem its part of the gradients needs no adjoint solve:
 *   dJ/dwaypoints, dJ/dbc = 2 (K d) at the fixed slots      (+ 2 w v at the two boundary velocities)
 *   dJ/dtimes             = csp_minsnap_cost_batch's grad_times
 * so with grad_coeffs NULL the call is the cost kernel's three-column sweep plus a few products per segment, and
 * grad_coeffs is never read.  With both cotangents it is the VJP's six-column sweep with the J terms added in the back
 * substitution.  Deterministic run to run (no atomics).
 *   desc          : the scope and CSP_ERR_UNSUPPORTED cases of csp_minsnap_solve_batch_vjp
 *   grad_coeffs   : [B][S][3][2*order] as for csp_minsnap_solve_batch_vjp, or NULL (no cotangent on the coefficients)
 *   grad_cost     : [B] f64 (whatever the storage type), or NULL: then the call IS csp_minsnap_solve_batch_vjp (same
 *                   kernel, same bits).  Both NULL: CSP_ERR_INVALID_ARG.
 *   grad_waypoints, grad_times, grad_bc : optional outs as for csp_minsnap_solve_batch_vjp; all three NULL:
 *                   CSP_ERR_INVALID_ARG
 *   status        : optional [B] i32: CSP_TRAJ_NOT_SPD (a pivot <= 0), CSP_TRAJ_NONFINITE (a gradient this trajectory
 *                   writes is inf/NaN, e.g. from an infinite grad_cost entry)
 *   workspace     : device scratch of csp_minsnap_cost_vjp_workspace_bytes(desc, grad_coeffs != NULL) bytes
 *                   (CSP_MEM_DEVICE, 8-byte aligned); may be NULL/0 with CSP_MEM_HOST.  With o = order, Smax =
 *                   num_segments (uniform) or max_segments (ragged), c = 6 with grad_coeffs and 3 without:
 *                     round_up_256((Smax - 1) * ((o-1)^2 + c(o-1)) * B * 8)
 *                       + (bc_per_trajectory ? 0 : 12 * ceil(B / 64) * 8)
 *                   (c = 6 is csp_minsnap_vjp_workspace_bytes, c = 3 the factors of csp_minsnap_cost_workspace_bytes;
 *                   the second term holds the per-workgroup partials of a shared bc's gradient and is only written
 *                   when grad_bc is asked for)
 * Every argument check (workspace size and alignment of a device-memory call included) comes back before a device is
 * looked for.  CSP_MEM_HOST: staged through the cached arena, synchronous.  CSP_MEM_DEVICE: asynchronous on
 * `hip_stream`. */
int csp_minsnap_solve_batch_cost_vjp(const csp_minsnap_desc *desc, const void *waypoints, const void *times,
                                     const void *bc, const void *grad_coeffs, const double *grad_cost,
                                     void *grad_waypoints, void *grad_times, void *grad_bc, int32_t *status,
                                     void *workspace, size_t workspace_bytes, void *hip_stream);
/* Device scratch bytes csp_minsnap_solve_batch_cost_vjp needs for `desc`, with (non-zero) or without (0) a grad_coeffs
 * cotangent (formula above; 0 for an invalid or unsupported descriptor). */
size_t csp_minsnap_cost_vjp_workspace_bytes(const csp_minsnap_desc *desc, int with_grad_coeffs);

/* The cost the solve minimises and its gradient with respect to the segment times:
 *   J(T)    = sum_axes sum_j [ integral_0^T_j (p_j^(order))^2 dt + w (v_j(0)^2 + v_j(T_j)^2) ]   at the solve's optimum
 *   dJ/dT_j = (1/T_j) sum_axes sum_ab (deriv_a + deriv_b + 1 - 2 order) Qt_ab(T_j) d_a d_b   (envelope theorem: the
 *             optimum's endpoint derivatives d are held fixed, no adjoint solve; the w term does not depend on T)
 * One lane per trajectory: the solve's block-LDL^T sweep and back substitution, no coefficients.
 *   desc       : the scope of csp_minsnap_solve_batch_vjp (orders 2..5, uniform or ragged, fp64 storage or fp32 storage
 *                with fp64 arithmetic, shared or per-trajectory bc and vel_zero_weight).  CSP_ERR_UNSUPPORTED for
 *                path_weight != 0, order 1, CSP_FLAG_SEGMENT_MAJOR and CSP_FLAG_F32_ARITH.
 *   cost       : out, [B] f64
 *   grad_times : optional out, the layout and storage type of `times`
 *   status     : optional [B] i32: CSP_TRAJ_NOT_SPD, CSP_TRAJ_NONFINITE (J or a gradient is inf/NaN)
 *   workspace  : device scratch of csp_minsnap_cost_workspace_bytes(desc) bytes (CSP_MEM_DEVICE, 8-byte aligned); may be
 *                NULL/0 with CSP_MEM_HOST.  With o = order, Smax = num_segments (uniform) or max_segments (ragged):
 *                  round_up_256((Smax - 1) * ((o-1)^2 + 3(o-1)) * B * 8)
 * CSP_MEM_HOST: staged through the cached arena, synchronous.  CSP_MEM_DEVICE: asynchronous on `hip_stream`. */
int csp_minsnap_cost_batch(const csp_minsnap_desc *desc, const void *waypoints, const void *times, const void *bc,
                           double *cost, void *grad_times, int32_t *status, void *workspace, size_t workspace_bytes,
                           void *hip_stream);
/* Device scratch bytes csp_minsnap_cost_batch needs (formula above; 0 for an invalid or unsupported descriptor). */
size_t csp_minsnap_cost_workspace_bytes(const csp_minsnap_desc *desc);

/* segment-time optimisation modes */
#define CSP_TIMEOPT_FIXED_TOTAL 0u  /* minimise J subject to sum_j T_j = sum_j T_j^in, T_j >= min_time */
#define CSP_TIMEOPT_TIME_PENALTY 1u /* minimise J + time_weight * sum_j T_j, T_j >= min_time          */

typedef struct csp_minsnap_timeopt_params {
    uint32_t abi_version;       /* CSP_MINSNAP_ABI_VERSION                                          */
    uint32_t mode;              /* CSP_TIMEOPT_FIXED_TOTAL | CSP_TIMEOPT_TIME_PENALTY                */
    double time_weight;         /* rho > 0, CSP_TIMEOPT_TIME_PENALTY only                           */
    double min_time;            /* t_min > 0                                                        */
    double tol;                 /* >= 0: stop when max_j |x_j - P(x_j - g_j)| <= tol (scaled, below)  */
    int32_t max_iters;          /* >= 0 accepted iterations at most                                 */
    uint32_t reserved;
} csp_minsnap_timeopt_params;

/* Segment-time optimisation: per trajectory, the times that minimise the snap cost J (fixed total) or J + rho sum T
 * (time penalty), starting from times_in, in ONE launch.  Spectral projected gradient: Barzilai-Borwein
 * steps with monotone Armijo backtracking, in the scaled variables x = T / mean(T_start) and objective / its initial value,
 * with an exact projection (Michelot's algorithm for the fixed total, a clip for the time penalty).  The start is
 * times_in, projected onto the feasible set when an entry is below min_time.  Every evaluation is a full pass of
 * csp_minsnap_cost_batch's kernel (the trial's gradient is the next iteration's).
 *   Stopping rule: max_j |x_j - P(x_j - g^_j)| <= tol, g^ the scaled gradient; otherwise CSP_TRAJ_NOT_CONVERGED after
 *   max_iters accepted iterations (max_iters = 0 returns the start).  The objective never increases: final <= initial
 *   bit for bit from the kernel's own evaluations.  The bounds hold exactly; the fixed total holds to 1e-12 relative
 *   (with fp32 storage, to the rounding of the returned times).  Lanes of a wave take different numbers of iterations
 *   and the wave runs until its slowest lane is done.
 *   desc        : the scope of csp_minsnap_cost_batch (same CSP_ERR_UNSUPPORTED cases)
 *   prm         : CSP_ERR_INVALID_ARG for NULL, a bad abi_version or mode, time_weight <= 0 with the time penalty,
 *                 min_time <= 0, tol < 0, max_iters < 0, and (CSP_MEM_HOST) sum_j T_j^in < S * min_time with the fixed
 *                 total.  With CSP_MEM_DEVICE the last check is per trajectory on the device: such a trajectory is
 *                 returned unchanged with CSP_TRAJ_NOT_CONVERGED, iterations 0 and NaN objectives.
 *   times_in    : an entry below min_time (zero and negative ones included) is not an error: the start is the
 *                 projection.  A trajectory with an inf / NaN time has no projection and is returned unchanged with
 *                 CSP_TRAJ_NONFINITE, iterations 0 and NaN objectives.  S = 1 with the fixed total has nothing to
 *                 optimise: times_out = times_in bit for bit, final objective = initial objective, iterations 0.
 *   times_out   : out, the layout of times_in
 *   coeffs      : optional out, csp_minsnap_solve_batch(times_out) -- computed by that call's own dispatch, so bit-equal
 *                 to a separate solve
 *   objective   : optional out, [B][2] f64: initial (at the start) and final objective (J, plus rho sum T)
 *   iterations  : optional out, [B] i32 accepted iterations
 *   status      : optional out, [B] i32: CSP_TRAJ_NOT_SPD / CSP_TRAJ_NONFINITE (the solve failed at the start, e.g. an
 *                 inf / NaN waypoint or bc: the trajectory stops there, times_out = the start, iterations 0),
 *                 CSP_TRAJ_NOT_CONVERGED.  A bad trajectory does not change any output of another one.
 *   workspace   : device scratch of csp_minsnap_timeopt_workspace_bytes(desc) bytes (CSP_MEM_DEVICE, 8-byte aligned);
 *                 may be NULL/0 with CSP_MEM_HOST:
 *                   round_up_256((Smax - 1) * ((o-1)^2 + 3(o-1)) * B * 8) + 4 * Smax * B * 8
 * CSP_MEM_HOST: staged through the cached arena, synchronous.  CSP_MEM_DEVICE: asynchronous on `hip_stream`. */
int csp_minsnap_optimize_times_batch(const csp_minsnap_desc *desc, const csp_minsnap_timeopt_params *prm,
                                     const void *waypoints, const void *times_in, const void *bc, void *times_out,
                                     void *coeffs, double *objective, int32_t *iterations, int32_t *status,
                                     void *workspace, size_t workspace_bytes, void *hip_stream);
/* Device scratch bytes csp_minsnap_optimize_times_batch needs (formula above; 0 for an invalid or unsupported
 * descriptor). */
size_t csp_minsnap_timeopt_workspace_bytes(const csp_minsnap_desc *desc);

/* The periodic (closed-loop) minimum-snap solve: S >= 1 segments around a loop, segment j from
 * waypoint P_j to P_{(j+1) mod S} in time T_j.  Every knot is interior, the wrap P_{S-1} -> P_0 included: derivatives
 * 1..order-1 are continuous around the whole loop, and there are no boundary conditions.  One lane per trajectory, a
 * bordered block-LDL^T sweep (knot 0 is the border), the factors in `workspace`.  Results are deterministic run to run.
 *   desc       : the scope of csp_minsnap_solve_batch_vjp (orders 2..5, uniform or ragged, CSP_DTYPE_F64 or CSP_DTYPE_F32
 *                with fp64 arithmetic, vel_zero_weight scalar or per trajectory).  CSP_ERR_UNSUPPORTED for order 1 or
 *                6+, path_weight != 0, CSP_FLAG_SEGMENT_MAJOR and CSP_FLAG_F32_ARITH.  bc_per_trajectory is ignored.
 *   waypoints  : [B][S][3], the S distinct loop points (no repeated closing point)
 *   times      : [B][S]
 *   RAGGED LAYOUT (num_segments == 0): trajectory b owns waypoints AND times seg_offsets[b] .. seg_offsets[b+1]-1, i.e.
 *                waypoints is [seg_offsets[B]][3].  This differs from the open chain, whose waypoints are offset by +b.
 *                A trajectory with S_b = 0 gets cost 0 and status 0; nothing else is written for it.
 *   coeffs     : out, [B][S][3][2*order], the record format of csp_minsnap_solve_batch; 16-byte aligned (fp64) / 8-byte
 *                (fp32).  Bit-identical whether or not cost / grad_times are requested.
 *   cost       : optional out, [B] f64: the snap cost J of csp_minsnap_cost_batch (w term included) at the solution
 *   grad_times : optional out, dJ/dT_j by the envelope theorem, the layout and storage type of `times`
 *   status     : optional out, [B] i32: CSP_TRAJ_NOT_SPD (a pivot <= 0, the border's Schur complement included: only
 *                non-positive or non-finite times cause it), CSP_TRAJ_NONFINITE (a stored coefficient, J or a gradient
 *                is inf/NaN)
 *   workspace  : device scratch of csp_minsnap_periodic_workspace_bytes(desc) bytes (CSP_MEM_DEVICE, 8-byte aligned);
 *                may be NULL/0 with CSP_MEM_HOST.  With o = order, Smax = num_segments (uniform) or max_segments (ragged):
 *                  round_up_256((Smax - 1) * (2(o-1)^2 + 3(o-1)) * B * 8)
 * Arguments are checked before a device is looked for.
 * CSP_MEM_HOST: staged through the cached arena, synchronous.  CSP_MEM_DEVICE: asynchronous on `hip_stream`. */
int csp_minsnap_solve_periodic_batch(const csp_minsnap_desc *desc, const void *waypoints, const void *times, void *coeffs,
                                     double *cost, void *grad_times, int32_t *status, void *workspace,
                                     size_t workspace_bytes, void *hip_stream);
/* Device scratch bytes csp_minsnap_solve_periodic_batch needs (formula above; 0 for an invalid or unsupported
 * descriptor). */
size_t csp_minsnap_periodic_workspace_bytes(const csp_minsnap_desc *desc);

/* Reverse mode of csp_minsnap_solve_periodic_batch: given grad_coeffs = dL/dcoeffs and, optionally,
 * grad_cost = dL/dcost for a scalar L of that call's coefficients and cost, writes dL/dwaypoints and dL/dtimes.  The
 * adjoint system is the forward's block-cyclic matrix, shared by the three axes; the primal is re-solved from waypoints
 * and times in the same sweep (the forward's coefficients are not an input).  One lane per trajectory, no atomics, every
 * sum in a fixed order: two calls give identical bits, whichever outputs are asked for.
 *   desc           : the scope, layouts (RAGGED LAYOUT included) and CSP_ERR_UNSUPPORTED cases of
 *                    csp_minsnap_solve_periodic_batch; bc_per_trajectory is ignored
 *   waypoints      : [B][S][3]
 *   times          : [B][S]
 *   grad_coeffs    : [B][S][3][2*order], the layout of coeffs; 16-byte aligned (fp64) / 8-byte (fp32)
 *   grad_cost      : optional, [B] f64; NULL means 0 (its terms are then not computed)
 *   grad_waypoints : optional out, the layout and storage type of `waypoints`
 *   grad_times     : optional out, the layout and storage type of `times`; with grad_cost it includes
 *                    grad_cost * dJ/dT_j, the forward's grad_times.  CSP_ERR_INVALID_ARG when both outputs are NULL.
 *                    S = 1: grad_waypoints = sum of grad_coeffs at power 0 per axis, grad_times = 0.
 *                    A trajectory with S_b = 0 gets status 0; nothing else is written for it.
 *   status         : optional out, [B] i32: CSP_TRAJ_NOT_SPD (a pivot <= 0, the border's Schur complement included),
 *                    CSP_TRAJ_NONFINITE (a gradient written for the trajectory is inf/NaN).  A bad trajectory does not
 *                    change any output of another one.
 *   workspace      : device scratch of csp_minsnap_periodic_vjp_workspace_bytes(desc) bytes (CSP_MEM_DEVICE, 8-byte
 *                    aligned); may be NULL/0 with CSP_MEM_HOST.  With o = order, Smax = num_segments (uniform) or
 *                    max_segments (ragged):
 *                      round_up_256((Smax - 1) * (2(o-1)^2 + 6(o-1)) * B * 8)
 * Arguments are checked before a device is looked for.
 * CSP_MEM_HOST: staged through the cached arena, synchronous.  CSP_MEM_DEVICE: asynchronous on `hip_stream`. */
int csp_minsnap_solve_periodic_batch_vjp(const csp_minsnap_desc *desc, const void *waypoints, const void *times,
                                         const void *grad_coeffs, const double *grad_cost, void *grad_waypoints,
                                         void *grad_times, int32_t *status, void *workspace, size_t workspace_bytes,
                                         void *hip_stream);
/* Device scratch bytes csp_minsnap_solve_periodic_batch_vjp needs (formula above; 0 for an invalid or unsupported
 * descriptor). */
size_t csp_minsnap_periodic_vjp_workspace_bytes(const csp_minsnap_desc *desc);

/* The open-chain minimum-snap solve with PER-KNOT derivative constraints: positions are fixed at every
 * waypoint as in csp_minsnap_solve_batch, and every derivative 1..order-1 of every knot (waypoint) is either fixed to a
 * given value or free, chosen by the solve.  Free ends, a velocity pinned at an interior waypoint, "come to rest at
 * waypoint k" are masks.  There is no bc argument: the standard problem of csp_minsnap_solve_batch is the mask with all
 * order-1 bits set at both end knots (values: velocity and acceleration from bc, higher rows zero) and 0 at every
 * interior knot.  One lane per trajectory, one block-LDL^T sweep over the S+1 knots shared by the three axes, the factors
 * in `workspace`; no atomics, results bit-identical run to run.
 *   desc        : the scope of csp_minsnap_cost_batch (orders 2..5, any S >= 1, uniform or ragged, CSP_DTYPE_F64 or
 *                 CSP_DTYPE_F32 with fp64 arithmetic, vel_zero_weight scalar or per trajectory).  CSP_ERR_UNSUPPORTED for
 *                 order 1 or 6+, path_weight != 0, CSP_FLAG_SEGMENT_MAJOR and CSP_FLAG_F32_ARITH.  bc_per_trajectory is
 *                 ignored.
 *   waypoints   : [B][S+1][3]; the knots of trajectory b.  Ragged: knot k of trajectory b is row seg_offsets[b] + b + k
 *   times       : [B][S]
 *   knot_mask   : [B][S+1] u8, the knots' layout (ragged: index seg_offsets[b] + b + k).  Bit r (r = 0 .. order-2) set:
 *                 derivative r+1 at that knot is fixed to knot_values[knot][r][0..2]; clear: it is free.  The three axes
 *                 share a knot's mask.  Bits from order-1 upward are ignored.
 *   knot_values : [knots][order-1][3] in the storage type of desc->dtype.  An entry whose mask bit is clear is never
 *                 used: NaN or inf there reaches no output.
 *   coeffs      : out, [B][S][3][2*order], the record format and trajectory-major layout of csp_minsnap_solve_batch (so
 *                 csp_minsnap_eval_batch and csp_minsnap_sample_batch read it unchanged); 16-byte aligned (fp64) / 8-byte
 *                 (fp32)
 *   cost        : optional out, [B] f64: J at the optimum with the definition of csp_minsnap_cost_batch, the
 *                 vel_zero_weight term included.  The coefficients are the same bits with or without it.
 *   status      : optional out, [B] i32.  CSP_TRAJ_NOT_SPD: a pivot <= 0, a segment time that is not > 0 (its Hessian
 *                 block is not positive semi-definite even where pinned neighbours leave every pivot positive), or a
 *                 trajectory whose constraint count -- its
 *                 S+1 positions plus the set mask bits below order-1, summed over its knots -- is below the order: a
 *                 non-zero polynomial of degree < order then costs nothing and the minimiser is not unique.  That case
 *                 is decided by the count before the sweep; coefficients and cost are NaN.  CSP_TRAJ_NONFINITE: a stored
 *                 coefficient or J is inf/NaN.  A ragged trajectory with S_b = 0 gets cost 0 and status 0; nothing else
 *                 is written for it.  A ragged trajectory longer than max_segments (CSP_MEM_DEVICE; CSP_MEM_HOST:
 *                 CSP_ERR_INVALID_ARG) gets CSP_TRAJ_SKIPPED and a NaN cost, its coefficients are not written.  A bad
 *                 trajectory does not change any output of another one.
 *   workspace   : device scratch of csp_minsnap_knots_workspace_bytes(desc) bytes (CSP_MEM_DEVICE, 8-byte aligned); may
 *                 be NULL/0 with CSP_MEM_HOST.  With o = order, Smax = num_segments (uniform) or max_segments (ragged):
 *                   round_up_256((Smax + 1) * ((o-1)^2 + 3(o-1)) * B * 8)
 * Arguments (NULL waypoints / times / knot_mask / knot_values / coeffs, workspace size and alignment and the alignment of
 * coeffs of a device call) are checked before a device is looked for.
 * CSP_MEM_HOST: staged through the cached arena, synchronous.  CSP_MEM_DEVICE: asynchronous on `hip_stream`. */
int csp_minsnap_solve_knots_batch(const csp_minsnap_desc *desc, const void *waypoints, const void *times,
                                  const uint8_t *knot_mask, const void *knot_values, void *coeffs, double *cost,
                                  int32_t *status, void *workspace, size_t workspace_bytes, void *hip_stream);
/* Device scratch bytes csp_minsnap_solve_knots_batch needs (formula above; 0 for an invalid or unsupported descriptor). */
size_t csp_minsnap_knots_workspace_bytes(const csp_minsnap_desc *desc);

/* Reverse mode of csp_minsnap_solve_knots_batch: given grad_coeffs = dL/dcoeffs and / or grad_cost =
 * dL/dcost for a scalar L of that call's coefficients and cost, writes dL/dwaypoints, dL/dtimes and dL/dknot_values.  The
 * adjoint system is the forward's masked block-tridiagonal matrix, shared by the three axes; the primal is re-solved
 * from the inputs in the same sweep (the forward's coefficients are not an input).  One lane per trajectory, every
 * output written once by its owner, no atomics: two calls give identical bits, and an output's bits do not depend on
 * which other outputs are asked for.  There is no gradient for the mask or the weights.
 *   desc             : the scope, layouts (RAGGED LAYOUT included) and CSP_ERR_UNSUPPORTED cases of
 *                      csp_minsnap_solve_knots_batch; bc_per_trajectory is ignored
 *   waypoints, times, knot_mask, knot_values : the forward's inputs (a value whose mask bit is clear is never used, mask
 *                      bits from order-1 upward are ignored)
 *   grad_coeffs      : optional, [B][S][3][2*order], the layout and storage type of coeffs; 16-byte aligned (fp64) /
 *                      8-byte (fp32) for a device call.  NULL: its terms are not computed, the adjoint columns are not run
 *                      and the workspace is the smaller one
 *   grad_cost        : optional, [B] f64; NULL means 0 (its terms are then not computed).  CSP_ERR_INVALID_ARG when both
 *                      cotangents are NULL.
 *   grad_waypoints   : optional out, the layout and storage type of `waypoints`
 *   grad_times       : optional out, the layout and storage type of `times`
 *   grad_knot_values : optional out, the layout and storage type of `knot_values`.  The entry of a slot whose mask bit is
 *                      clear is exactly 0.0, whatever knot_values holds there.  CSP_ERR_INVALID_ARG when all three outputs
 *                      are NULL.
 *   status           : optional out, [B] i32, the forward's rules in the forward's order.  S_b = 0: status 0, zeros in the
 *                      trajectory's one knot row of grad_waypoints and grad_knot_values.  A ragged trajectory longer than
 *                      max_segments (CSP_MEM_DEVICE; CSP_MEM_HOST: CSP_ERR_INVALID_ARG): CSP_TRAJ_SKIPPED, every gradient
 *                      row it owns is NaN, the workspace is not touched for it.  A constraint count below the order:
 *                      CSP_TRAJ_NOT_SPD, decided before the sweep, every gradient row it owns is NaN.  A segment time that
 *                      is not > 0 or a pivot <= 0: CSP_TRAJ_NOT_SPD.  A written gradient that is inf/NaN:
 *                      CSP_TRAJ_NONFINITE.  A bad trajectory does not change any output of another one.
 *   workspace        : device scratch of csp_minsnap_knots_vjp_workspace_bytes(desc, grad_coeffs != NULL) bytes
 *                      (CSP_MEM_DEVICE, 8-byte aligned); may be NULL/0 with CSP_MEM_HOST.  With o = order, Smax =
 *                      num_segments (uniform) or max_segments (ragged), c = 6 with grad_coeffs and 3 without:
 *                        round_up_256((Smax + 1) * ((o-1)^2 + c(o-1)) * B * 8)
 * Arguments (NULL inputs, both cotangents or all outputs NULL, workspace size and alignment, the alignment of grad_coeffs
 * of a device call, ragged host offsets outside 0..max_segments) are checked before a device is looked for.
 * CSP_MEM_HOST: staged through the cached arena, synchronous.  CSP_MEM_DEVICE: asynchronous on `hip_stream`. */
int csp_minsnap_solve_knots_batch_vjp(const csp_minsnap_desc *desc, const void *waypoints, const void *times,
                                      const uint8_t *knot_mask, const void *knot_values, const void *grad_coeffs,
                                      const double *grad_cost, void *grad_waypoints, void *grad_times,
                                      void *grad_knot_values, int32_t *status, void *workspace, size_t workspace_bytes,
                                      void *hip_stream);
/* Device scratch bytes csp_minsnap_solve_knots_batch_vjp needs (formula above; 0 for an invalid or unsupported
 * descriptor). */
size_t csp_minsnap_knots_vjp_workspace_bytes(const csp_minsnap_desc *desc, int with_grad_coeffs);

/* Segment-time optimisation under PER-KNOT derivative constraints: csp_minsnap_optimize_times_batch for
 * the problem of csp_minsnap_solve_knots_batch.  Per trajectory, the times that minimise the snap cost J of the partition
 * the mask describes (fixed total) or J + rho sum T (time penalty), starting from times_in, in ONE launch: the same
 * spectral projected gradient loop, constants, scaling, projection and stopping rule as csp_minsnap_optimize_times_batch
 * (one copy of the loop serves both kernels), every evaluation a masked block-LDL^T sweep over the S+1 knots with the cost
 * and its envelope-theorem time gradient from the back substitution.  No atomics, every output written once by its owner:
 * two calls give identical bits.
 *   desc        : the scope, layouts (ragged: knot k of trajectory b is row seg_offsets[b] + b + k) and
 *                 CSP_ERR_UNSUPPORTED cases of csp_minsnap_solve_knots_batch (order 1 or 6+, path_weight != 0,
 *                 CSP_FLAG_SEGMENT_MAJOR, CSP_FLAG_F32_ARITH); bc_per_trajectory is ignored
 *   prm         : the rules of csp_minsnap_optimize_times_batch: CSP_ERR_INVALID_ARG for NULL, a bad abi_version or
 *                 mode, time_weight <= 0 with the time penalty, min_time <= 0, tol < 0, max_iters < 0, and (CSP_MEM_HOST)
 *                 sum_j T_j^in < S * min_time with the fixed total.  With CSP_MEM_DEVICE the last check is per trajectory
 *                 on the device: such a trajectory is returned unchanged with CSP_TRAJ_NOT_CONVERGED, iterations 0 and
 *                 NaN objectives.
 *   waypoints, knot_mask, knot_values : as csp_minsnap_solve_knots_batch.  A value whose mask bit is clear is never
 *                 used: NaN or inf there reaches no output.  Mask bits from order-1 upward are ignored.
 *   times_in    : [B][S]; an entry below min_time is not an error, the start is the projection
 *   times_out   : out, the layout of times_in
 *   coeffs      : optional out, csp_minsnap_solve_knots_batch(times_out) -- launched by that entry's own dispatch, so
 *                 bit-equal to a separate call; 16-byte aligned (fp64) / 8-byte (fp32) for a device call
 *   objective   : optional out, [B][2] f64: initial (at the start) and final objective (J, plus rho sum T)
 *   iterations  : optional out, [B] i32 accepted iterations
 *   status      : optional out, [B] i32.  Per trajectory, in this order:
 *                 - S_b = 0 (ragged): status 0, objectives 0, iterations 0; nothing else is written for it.
 *                 - a ragged trajectory longer than max_segments (CSP_MEM_DEVICE; CSP_MEM_HOST: CSP_ERR_INVALID_ARG):
 *                   CSP_TRAJ_SKIPPED, times_out = times_in, NaN objectives, iterations 0; coeffs are not written.
 *                 - a constraint count (S+1 positions plus the set mask bits below order-1) below the order:
 *                   CSP_TRAJ_NOT_SPD, decided before anything is evaluated; times_out = times_in, iterations 0, NaN
 *                   objectives; coeffs are the knots solve's own NaN coefficients.
 *                 - otherwise the rules of csp_minsnap_optimize_times_batch: an inf / NaN time gives CSP_TRAJ_NONFINITE
 *                   and the trajectory is returned unchanged (iterations 0, NaN objectives); a solve that fails at the
 *                   start (CSP_TRAJ_NOT_SPD / CSP_TRAJ_NONFINITE, e.g. an inf / NaN waypoint or pinned value) stops the
 *                   trajectory there: times_out = the start, iterations 0; CSP_TRAJ_NOT_CONVERGED after max_iters
 *                   accepted iterations (max_iters = 0 returns the start) or 30 backtracks without a decrease.  S = 1
 *                   with the fixed total: times_out = times_in bit for bit.
 *                 A bad trajectory does not change any output of another one.
 *   workspace   : device scratch of csp_minsnap_knots_timeopt_workspace_bytes(desc) bytes (CSP_MEM_DEVICE, 8-byte
 *                 aligned); may be NULL/0 with CSP_MEM_HOST.  With o = order, Smax = num_segments (uniform) or
 *                 max_segments (ragged):
 *                   round_up_256((Smax + 1) * ((o-1)^2 + 3(o-1)) * B * 8) + 4 * Smax * B * 8
 *                 (the knots solve's factor region, reused by the coefficient launch, then the optimiser's four vectors).
 *                 No slot is read before the same launch wrote it: stale contents change no output.
 * Arguments (NULL prm / waypoints / times_in / knot_mask / knot_values / times_out, the parameter rules, workspace size and
 * alignment and the alignment of coeffs of a device call, ragged host offsets outside 0..max_segments, an infeasible host
 * fixed total) are checked before a device is looked for.
 * CSP_MEM_HOST: staged through the cached arena, synchronous.  CSP_MEM_DEVICE: asynchronous on `hip_stream`. */
int csp_minsnap_optimize_times_knots_batch(const csp_minsnap_desc *desc, const csp_minsnap_timeopt_params *prm,
                                           const void *waypoints, const void *times_in, const uint8_t *knot_mask,
                                           const void *knot_values, void *times_out, void *coeffs, double *objective,
                                           int32_t *iterations, int32_t *status, void *workspace, size_t workspace_bytes,
                                           void *hip_stream);
/* Device scratch bytes csp_minsnap_optimize_times_knots_batch needs (formula above; 0 for an invalid or unsupported
 * descriptor). */
size_t csp_minsnap_knots_timeopt_workspace_bytes(const csp_minsnap_desc *desc);

/* Lap-time optimisation of the PERIODIC (closed-loop) solve: csp_minsnap_optimize_times_batch for the
 * problem of csp_minsnap_solve_periodic_batch.  Per loop, the segment times that minimise the snap cost J of the closed
 * spline (fixed total: the lap time is kept) or J + rho sum T (time penalty), starting from times_in, in ONE launch: the
 * same spectral projected gradient loop, constants, scaling, projection and stopping rule as
 * csp_minsnap_optimize_times_batch (one copy of the loop serves all three kernels), every evaluation a bordered
 * block-LDL^T sweep around the loop with the cost and its envelope-theorem time gradient from the back substitution.
 * No atomics, every output written once by its owner: two calls give identical bits.
 *   desc        : the scope, layouts (RAGGED LAYOUT: trajectory b owns waypoints AND times seg_offsets[b] ..
 *                 seg_offsets[b+1]-1, no +b offset) and CSP_ERR_UNSUPPORTED cases of csp_minsnap_solve_periodic_batch
 *                 (order 1 or 6+, path_weight != 0, CSP_FLAG_SEGMENT_MAJOR, CSP_FLAG_F32_ARITH); bc_per_trajectory is
 *                 ignored; vel_zero_weight is honoured, scalar or per trajectory
 *   prm         : the rules of csp_minsnap_optimize_times_batch: CSP_ERR_INVALID_ARG for NULL, a bad abi_version or
 *                 mode, time_weight <= 0 with the time penalty, min_time <= 0, tol < 0, max_iters < 0, and (CSP_MEM_HOST)
 *                 sum_j T_j^in < S * min_time with the fixed total.  With CSP_MEM_DEVICE the last check is per trajectory
 *                 on the device: such a trajectory is returned unchanged with CSP_TRAJ_NOT_CONVERGED, iterations 0 and
 *                 NaN objectives.
 *   waypoints   : [B][S][3], the S distinct loop points (no repeated closing point)
 *   times_in    : [B][S]; an entry below min_time is not an error, the start is the projection
 *   times_out   : out, the layout of times_in
 *   coeffs      : optional out, csp_minsnap_solve_periodic_batch(times_out) -- launched by that entry's own dispatch, so
 *                 bit-equal to a separate call; 16-byte aligned (fp64) / 8-byte (fp32) for a device call
 *   objective   : optional out, [B][2] f64: initial (at the start) and final objective (J, plus rho sum T)
 *   iterations  : optional out, [B] i32 accepted iterations
 *   status      : optional out, [B] i32.  Per trajectory, in this order:
 *                 - S_b = 0 (ragged): status 0, objectives 0, iterations 0; nothing else is written for it.
 *                 - a ragged trajectory longer than max_segments (CSP_MEM_DEVICE; CSP_MEM_HOST: CSP_ERR_INVALID_ARG):
 *                   CSP_TRAJ_SKIPPED, times_out = times_in, NaN objectives, iterations 0; coeffs are not written.  The
 *                   periodic solve has no length guard of its own and a table of offsets cannot leave one trajectory
 *                   out, so the coefficient launch of such a batch writes NO trajectory's coefficients: the descriptor
 *                   was wrong for the batch, every other output of every other trajectory is as without it.
 *                 - an inf / NaN time: CSP_TRAJ_NONFINITE, the trajectory is returned unchanged (iterations 0, NaN
 *                   objectives).
 *                 - an infeasible fixed total (CSP_MEM_DEVICE): CSP_TRAJ_NOT_CONVERGED, returned unchanged, NaN
 *                   objectives, iterations 0.
 *                 - a solve that fails at the start (CSP_TRAJ_NOT_SPD / CSP_TRAJ_NONFINITE, e.g. an inf / NaN waypoint):
 *                   the trajectory stops there, times_out = the start, iterations 0.  CSP_TRAJ_NOT_SPD: a pivot <= 0,
 *                   the border's Schur complement included, or a time that is not > 0; CSP_TRAJ_NONFINITE: J or a
 *                   gradient is inf/NaN.
 *                 - CSP_TRAJ_NOT_CONVERGED after max_iters accepted iterations (max_iters = 0 returns the start) or 30
 *                   backtracks without a decrease.
 *                 - S = 1 with the fixed total has nothing to optimise: times_out = times_in bit for bit, final
 *                   objective = initial objective (J = 0 for one knot, whatever w), iterations 0.  S = 1 with the time
 *                   penalty is a real problem: J = 0 for every T, so the time runs to min_time (a converged trajectory
 *                   that moved returns min_time itself, final objective time_weight * min_time).
 *                 A bad trajectory does not change any output of another one.
 *   workspace   : device scratch of csp_minsnap_periodic_timeopt_workspace_bytes(desc) bytes (CSP_MEM_DEVICE, 8-byte
 *                 aligned); may be NULL/0 with CSP_MEM_HOST.  With o = order, Smax = num_segments (uniform) or
 *                 max_segments (ragged):
 *                   round_up_256((Smax - 1) * (2(o-1)^2 + 3(o-1)) * B * 8) + 4 * Smax * B * 8
 *                 (the periodic solve's factor region, reused by the coefficient launch, then the optimiser's four
 *                 vectors).  No slot is read before the same launch wrote it: stale contents change no output.
 * Arguments (NULL prm / waypoints / times_in / times_out, the parameter rules, workspace size and alignment and the
 * alignment of coeffs of a device call, ragged host offsets outside 0..max_segments, an infeasible host fixed total) are
 * checked before a device is looked for.
 * CSP_MEM_HOST: staged through the cached arena, synchronous.  CSP_MEM_DEVICE: asynchronous on `hip_stream`. */
int csp_minsnap_optimize_times_periodic_batch(const csp_minsnap_desc *desc, const csp_minsnap_timeopt_params *prm,
                                              const void *waypoints, const void *times_in, void *times_out, void *coeffs,
                                              double *objective, int32_t *iterations, int32_t *status, void *workspace,
                                              size_t workspace_bytes, void *hip_stream);
/* Device scratch bytes csp_minsnap_optimize_times_periodic_batch needs (formula above; 0 for an invalid or unsupported
 * descriptor, and for B = 0). */
size_t csp_minsnap_periodic_timeopt_workspace_bytes(const csp_minsnap_desc *desc);

/* The same solve spread over `ngpu` devices of this node from ONE process (the reference planner
 * is a single C++ process).  Trajectories are independent
 * (minimum_snap.cpp has no cross-trajectory term), so the batch is cut into `ngpu` contiguous shards, shard g on the
 * g-th gfx950 device; no collective other than the scatter of inputs and the gather of results.  Synchronous.
 * ngpu <= 0 uses every gfx950 device; ngpu greater than the device count is CSP_ERR_INVALID_ARG.
 *   CSP_MEM_HOST   : every shard is staged from / to the caller's host memory by a host thread of its own through that
 *                    device's cached arena (page-locked halves, DMA overlapped with the host copy); desc->device_id is
 *                    ignored.  PCIe-bound (1.3-1.55e7 solves/s measured on one device).
 *   CSP_MEM_DEVICE : the batch is RESIDENT on a root device (desc->device_id, or the current one), uniform batches only
 *                    (ragged: CSP_ERR_UNSUPPORTED).  Inputs are scattered and coefficients gathered over RCCL / xGMI from
 *                    that root -- single-process communicators (ncclCommInitAll, cached), grouped ncclSend / ncclRecv,
 *                    one compute and one communication stream per device; every shard is cut into chunks (4; at least
 *                    4096 trajectories each; CSP_SHARD_CHUNKS overrides) and the gather of chunk i overlaps the solve of
 *                    chunk i+1.  The root's own shard is solved in place.  The call first synchronises the root device
 *                    (it takes no stream).
 * The span-versus-chunked kernel choice is made ONCE from the whole batch and pinned for the shards / chunks; within the
 * fixed-size kernels the narrow small-batch variants are bit-equal with the wide ones (tests), so results equal
 * csp_minsnap_solve_batch on one device bit for bit.  UNVERIFIED ON MORE THAN ONE GPU: the development boxes have one
 * device -- what runs there is ngpu = 1 (both forms), the chunk / peer schedule over a recording transport on the CPU
 * (tests/test_shard_schedule.py), and tests that run only where two devices exist. */
int csp_minsnap_solve_batch_sharded(const csp_minsnap_desc *desc, const void *waypoints, const void *times,
                                    const void *bc, void *coeffs, double *max_dev, int32_t *status, int ngpu);

/* n INDEPENDENT uniform batches of one shape (same order, segment count, dtype, weights, flags: `desc`; desc->batch is
 * ignored) with their own buffers, in ONE call -- and, for the shapes of the register-resident fixed-size kernels without
 * the path penalty, in ONE kernel launch: a launch costs ~3 us of dispatch / first-load / end-of-kernel latency around the
 * 3 us of work of a 4096-trajectory batch (BASELINE config 2), so a planner that solves many small batches per tick pays
 * mostly launches.  The workgroups find their (batch, slice) in a table passed as a kernel argument (no upload).
 * The reference solves one flight per call (TrajectoryGeneratorTool::SolveQPClosedForm, math_util/minimum_snap.hpp:45-53).
 *   batches[k]            : trajectories of batch k
 *   waypoints/times/bc/coeffs[k] : batch k's buffers, layouts as csp_minsnap_solve_batch (bc [1][4][3] or [B_k][4][3])
 *   status                : NULL, or n pointers to [B_k] int32 arrays (all or none)
 * CSP_MEM_DEVICE only (CSP_ERR_UNSUPPORTED otherwise, as for ragged descriptors and per-trajectory weights); other shapes
 * are served by one ordinary launch per batch when they need no workspace.  Results equal csp_minsnap_solve_batch's per
 * batch bit for bit.  Asynchronous on `hip_stream`. */
int csp_minsnap_solve_multi(const csp_minsnap_desc *desc, int n, const int64_t *batches, const void *const *waypoints,
                            const void *const *times, const void *const *bc, void *const *coeffs, int32_t *const *status,
                            void *hip_stream);

/* Mixed-ORDER ragged batches in ONE call (BASELINE config 5: per-trajectory segment count AND derivative order).  The
 * reference solves one flight per call with one `order` (TrajectoryGeneratorTool::SolveQPClosedForm,
 * math_util/minimum_snap.hpp:45-53); a planner that batches flights of different smoothness classes would otherwise have to
 * sort them by order itself.  Here the bucketing by (order, length class) runs on the device and the solve reads the inputs
 * and writes the coefficients IN THE CALLER'S ORDER -- nothing is gathered or un-permuted:
 *   desc        : dtype, batch, seg_offsets ([B+1], ragged layout as above), max_segments (<= 256), bc_per_trajectory,
 *                 vel_zero_weight(_per_traj), mem_space, device_id as for csp_minsnap_solve_batch; desc->order and
 *                 num_segments are ignored; path_weight must be 0 and CSP_FLAG_F32_ARITH is not offered (CSP_ERR_UNSUPPORTED)
 *   orders      : [B] int32, derivative order of every trajectory, 2..5 (same memory space as the data)
 *   coeffs      : trajectory b's block [S_b][3][2*order_b] starts at element coeff_offsets[b] = sum_{k<b} E_k, concatenated in
 *                 caller order, where E_k = 6*order_k*S_k rounded up to a whole number of 16-byte pieces (fp32 storage: a
 *                 multiple of 4 elements, i.e. 2 floats of padding after a block of odd order AND odd segment count; fp64:
 *                 no padding ever) -- every block starts 16-byte aligned.  The caller sizes the array (sum_b E_b <= the
 *                 tight sum + 2*B elements), e.g. from its own host copy of the shapes
 *   coeff_offsets_out : optional [B+1] int64, the offsets above (computed on the device); [B] = the total
 *   status      : optional [B] int32 CSP_TRAJ_* bits; trajectories outside the served range get CSP_TRAJ_SKIPPED
 *   workspace   : >= csp_minsnap_mixed_workspace_bytes(desc) bytes of device memory (CSP_MEM_DEVICE); NULL/0 with CSP_MEM_HOST
 *                 (it holds the bucketing tables and the checkpoint slots of the solve below: up to 0.2 MB per persistent
 *                 workgroup at max_segments = 64, 103 MB from B = 16384 on; less for shorter trajectories)
 * Trajectories of up to 64 segments are solved by a sequential twisted block-LDL^T sweep, two lanes per trajectory, in
 * blocks of segments whose factors are recomputed from checkpoints (cs-pathplan_amd/csrc/minsnap_twist_impl.h: the arithmetic
 * of the register-resident fixed-size kernels), every order in ONE persistent launch; longer ones (65..256 segments) by
 * csp_minsnap_solve_batch's workspace-free chunked kernel, one launch per order.  A trajectory longer than
 * desc->max_segments is reported CSP_TRAJ_SKIPPED.
 * CSP_MEM_DEVICE: asynchronous on `hip_stream`.  CSP_MEM_HOST: staged through the cached arena, synchronous. */
int csp_minsnap_solve_mixed(const csp_minsnap_desc *desc, const int32_t *orders, const void *waypoints, const void *times,
                            const void *bc, void *coeffs, int64_t *coeff_offsets_out, int32_t *status,
                            void *workspace, size_t workspace_bytes, void *hip_stream);
size_t csp_minsnap_mixed_workspace_bytes(const csp_minsnap_desc *desc);

/* Replaces the time-allocation step of TrajectoryGeneratorTool::GenerateTrajectoryMatrix
 * (minimum_snap.cpp:59-72): T_i = max(|p_{i+1}-p_i| / V_avg, min_time_s), or min_time_s when
 * V_avg <= 1e-6.  Every operation is rounded on its own in the storage type (no fused multiply-add): with fp64 storage the
 * times are bit for bit the reference's.  Same layouts / descriptor as the solve (path/vel weights ignored). */
int csp_minsnap_time_alloc_batch(const csp_minsnap_desc *desc, const void *waypoints, double v_avg,
                                 double min_time_s, void *times, void *hip_stream);

/* Replaces the solver half of TrajectoryGeneratorTool::GenerateTrajectoryMatrix
 * (minimum_snap.cpp:59-90) for a batch: time allocation (as csp_minsnap_time_alloc_batch) followed
 * by the re-solve loop -- solve; while max_deviation > 0.2 and fewer than 10 increases:
 * vel_zero_weight <- (w < 1e-6 ? 0.01 : 2w), solve again -- tracked per trajectory on the device
 * (no host round trip: converged trajectories are skipped by the later passes).
 *   times      : out, [B][S] (same layout rules as the solve)
 *   coeffs     : out
 *   max_dev    : out, optional [B] f64 (final deviation metric)
 *   vel_zero_weight_out : optional [B] f64, the weight the final solve used.  max_dev, vel_zero_weight_out and
 *                iterations are LIVE LOOP STATE during the call (the passes read and update them in place); with
 *                CSP_MEM_DEVICE vel_zero_weight_out may alias desc->vel_zero_weight_per_traj (weights updated in place)
 *   iterations : optional [B] i32, number of weight increases (reference `iter`)
 *   workspace  : >= csp_minsnap_plan_workspace_bytes(desc) bytes (device); NULL/0 with CSP_MEM_HOST */
int csp_minsnap_plan_batch(const csp_minsnap_desc *desc, const void *waypoints, double v_avg, double min_time_s,
                           const void *bc, void *times, void *coeffs, double *max_dev,
                           double *vel_zero_weight_out, int32_t *iterations, int32_t *status,
                           void *workspace, size_t workspace_bytes, void *hip_stream);
size_t csp_minsnap_plan_workspace_bytes(const csp_minsnap_desc *desc);

/* Replaces the sampling half of GenerateTrajectoryMatrix (minimum_snap.cpp:97-205): evaluates each
 * trajectory at dt = min(0.1, T_seg/10), keeps a point whenever it is >= sample_distance away from
 * the previously kept one, appends the end point, and computes the two statistics the reference
 * prints (max climb/descent rate, min turn radius).
 *   samples : out, [B][capacity][3] (storage dtype); trajectory b uses the first counts[b] rows; the rows from
 *             min(counts[b], capacity) on are left as they were (every sampler; CSP_MEM_DEVICE)
 *   counts  : out, [B] i32 -- the TRUE number of samples; rows beyond `capacity` are dropped, so
 *             counts[b] > capacity tells the caller to retry with a larger capacity
 *   stats   : optional out, [B][2] f64 = {max climb rate, min turn radius} */
int csp_minsnap_sample_batch(const csp_minsnap_desc *desc, const void *times, const void *coeffs,
                             double sample_distance, int64_t capacity, void *samples, int32_t *counts,
                             double *stats, void *hip_stream);

/* Replaces the WHOLE of TrajectoryGeneratorTool::GenerateTrajectoryMatrix (minimum_snap.cpp:22-206) for a batch:
 * csp_minsnap_plan_batch followed by csp_minsnap_sample_batch with the times and coefficients left on the device.
 * Results are bit for bit those of the two calls.  A CSP_MEM_HOST caller -- the reference's own call pattern, one
 * flight per call (uavPathPlanning.cpp:4423, :4461) -- pays ONE upload, ONE download and ONE synchronisation (a
 * second round only when the re-solve loop had to raise somebody's weight).
 *   capacity : rows of `samples` per trajectory (csp_minsnap_sample_capacity gives a sufficient value)
 *   times, coeffs : optional outputs with CSP_MEM_HOST; REQUIRED (device buffers, they are the intermediates) with
 *                   CSP_MEM_DEVICE
 *   workspace : >= csp_minsnap_plan_workspace_bytes(desc) bytes (device); NULL/0 with CSP_MEM_HOST
 * Everything else as in the two calls it stands for. */
int csp_minsnap_generate_batch(const csp_minsnap_desc *desc, const void *waypoints, double v_avg, double min_time_s,
                               const void *bc, double sample_distance, int64_t capacity, void *samples,
                               int32_t *counts, double *stats, void *times, void *coeffs, double *max_dev,
                               double *vel_zero_weight_out, int32_t *iterations, int32_t *status,
                               void *workspace, size_t workspace_bytes, void *hip_stream);

/* Position and its derivatives of every trajectory at arbitrary query times.  Works on any
 * coefficient array in csp_minsnap_solve_batch's trajectory-major layout: the open-chain solve's, the periodic solve's
 * (reduce t modulo the lap time first: there is no wrap-around here), a plan's.  Workspace-free.
 *   desc       : dtype, order 2..5, batch, num_segments 1..1024 or a ragged batch (seg_offsets, max_segments <= 1024),
 *                mem_space, device_id.  CSP_ERR_UNSUPPORTED for order 1, more than 1024 segments,
 *                CSP_FLAG_SEGMENT_MAJOR and CSP_FLAG_F32_ARITH.  The weights and bc_per_trajectory are ignored.
 *   times      : [B][S] segment durations T (ragged: concatenated, as for the solve)
 *   coeffs     : [B][S][3][M], M = 2*order, highest power first (c_k * tau^(M-1-k)); 16-byte aligned (fp64) / 8-byte
 *                (fp32), as the solve writes them
 *   query      : [B][num_queries] global times t, measured from the trajectory's start; num_queries >= 0 is the same
 *                for every trajectory
 *   num_derivs : D in 1..5: position, velocity, acceleration, jerk, snap
 *   out        : [B][num_queries][D][3]
 *   seg_index  : optional [B][num_queries] i32, the segment j of every query
 *   status     : optional [B] i32 CSP_TRAJ_* bits
 * Every floating array is in the storage type desc->dtype; all arithmetic is fp64 (fp32 inputs convert exactly, outputs
 * are rounded once when stored).  Per trajectory of S segments and per query t:
 *   1. cum[0] = 0, cum[j+1] = cum[j] + T[j]: the left-to-right fp64 running sum, every addition rounded once.
 *   2. t_c = min(max(t, 0), cum[S]).  t < 0 is "clamped low", t > cum[S] "clamped high"; t == cum[S] is in range.
 *   3. j = the largest index with cum[j] <= t_c, at most S-1: a query on a knot belongs to the LATER segment, and a
 *      zero-length segment is never selected unless it is the last one and t_c = cum[S].
 *   4. tau = t_c - cum[j], one fp64 subtraction.
 *   5. out[q][d][a] = sum_k c[j][a][k] * ff(p,d) * tau^(p-d), p = M-1-k, ff(p,d) = p(p-1)...(p-d+1) (0 for p < d),
 *      0^0 = 1.  At tau = 0 the position is c[j][a][M-1] bit for bit (derivative d: ff(d,d) * c[j][a][M-1-d]).
 *   6. seg_index[q] = j.
 * Bad inputs are handled values, they never fault and never touch another trajectory's outputs:
 *   - a query that is inf or NaN: its out rows are NaN and its seg_index is -1; the status is not changed;
 *   - a trajectory with a T that is negative, inf or NaN: CSP_TRAJ_NONFINITE, all its out rows NaN, seg_index -1;
 *   - a ragged trajectory with S_b = 0: status 0, out rows NaN, seg_index -1 (CSP_MEM_DEVICE: a length outside
 *     0..max_segments is treated the same way and reported as CSP_TRAJ_SKIPPED; CSP_MEM_HOST: CSP_ERR_INVALID_ARG);
 *   - CSP_TRAJ_NONFINITE is also set when a value stored for a finite query of a good trajectory is inf or NaN (NaN
 *     coefficients, for instance).
 * CSP_ERR_INVALID_ARG: num_derivs outside 1..5, num_queries < 0, a null times / coeffs, a null query / out with
 * num_queries > 0, misaligned coeffs (CSP_MEM_DEVICE).  batch == 0 or num_queries == 0: CSP_OK, nothing is launched.
 * Every argument check comes back before a device is looked for.
 * CSP_MEM_HOST: staged through the cached arena, synchronous, the same bits as the device form.  CSP_MEM_DEVICE:
 * asynchronous on `hip_stream`. */
int csp_minsnap_eval_batch(const csp_minsnap_desc *desc, const void *times, const void *coeffs, const void *query,
                           int64_t num_queries, int32_t num_derivs, void *out, int32_t *seg_index, int32_t *status,
                           void *hip_stream);

/* Reverse mode of csp_minsnap_eval_batch: given grad_out = dL/dout [B][num_queries][D][3], the vector-Jacobian products
 * with respect to the coefficients, the segment times and the query times.  With tau_q, j_q of rules 1-4 above and
 *   g_tau[q] = sum_{d,a} grad_out[q][d][a] * x_a^(d+1)(tau_q)          (derivatives up to order D)
 *   grad_coeffs[j][a][k] = sum_{q: j_q = j} sum_d grad_out[q][d][a] * ff(p,d) * tau_q^(p-d), in ascending q.  EVERY record
 *                  of the trajectory is written, zeros where no query falls: the caller pre-zeroes nothing.
 *   grad_query[q] = g_tau[q] for a query in range, 0 for a clamped one.
 *   grad_times[i] = - sum_{q in range, j_q > i} g_tau[q], plus sum_{q clamped high} g_tau[q] for i = S-1 only (a
 *                  clamped-high query has tau = T[S-1] in exact arithmetic, so it moves grad_times[S-1] alone; a
 *                  clamped-low one depends on no T).  Formed as per-segment sums in ascending q, then a suffix sum
 *                  over the segments.
 * This is the EXPLICIT dependence on `times` through tau only; the dependence of the coefficients on the times is
 * csp_minsnap_solve_batch_vjp's, and the two add.  No atomics: two calls give identical bits, and each output has the
 * same bits whichever of the others are asked for.
 *   grad_coeffs : optional out, the layout and alignment of `coeffs`
 *   grad_times  : optional out, the layout of `times`
 *   grad_query  : optional out, [B][num_queries]; all three NULL: CSP_ERR_INVALID_ARG
 *   status      : optional [B] i32
 * Bad inputs: an inf / NaN query contributes nothing to grad_coeffs and grad_times, its grad_query is NaN; a trajectory
 * with a negative, inf or NaN T gets CSP_TRAJ_NONFINITE and NaN in all its grad_coeffs, grad_times and grad_query rows;
 * a ragged trajectory with S_b = 0 gets status 0 and zeros in its grad_query rows (it has no other rows);
 * CSP_TRAJ_NONFINITE is also set when a gradient stored for a good trajectory (grad_query of a finite query) is inf/NaN.
 * Scope, CSP_ERR_UNSUPPORTED and CSP_ERR_INVALID_ARG cases as above (grad_out takes the place of out; a misaligned
 * grad_coeffs counts like misaligned coeffs).  batch == 0: CSP_OK.  num_queries == 0 still writes zero grad_coeffs and
 * grad_times.  CSP_MEM_HOST: staged, synchronous, the device form's bits.  CSP_MEM_DEVICE: asynchronous on `hip_stream`. */
int csp_minsnap_eval_batch_vjp(const csp_minsnap_desc *desc, const void *times, const void *coeffs, const void *query,
                               int64_t num_queries, int32_t num_derivs, const void *grad_out, void *grad_coeffs,
                               void *grad_times, void *grad_query, int32_t *status, void *hip_stream);

/* Upper bound of the samples any trajectory of the batch can produce (every candidate of the sampling loop,
 * minimum_snap.cpp:126-161, plus the first and the last point), from HOST-resident waypoints: a `capacity` that
 * csp_minsnap_generate_batch / csp_minsnap_sample_batch cannot overflow.  -1 for an invalid descriptor. */
int64_t csp_minsnap_sample_capacity(const csp_minsnap_desc *desc, const void *waypoints_host, double v_avg,
                                    double min_time_s);

/* Name of the kernel csp_minsnap_solve_batch would dispatch for `desc` ("fixed_o4_s16_f64",
 * "generic_o4_f64", ...); NULL for an invalid descriptor.  For tests and profiles. */
const char *csp_minsnap_kernel_name(const csp_minsnap_desc *desc);

/* Number of visible HIP devices whose architecture is gfx950 (0 => every solve call fails). */
int csp_minsnap_device_count(void);

/* Process-lifetime notes: the library keeps helper threads (staging copies), cached arenas, streams and RCCL communicators
 * alive once used -- do not dlclose() it or fork() after the first call; HIP device ordinals up to 63 are supported.
 * An idle arena keeps at most 512 MB of device memory (CSP_ARENA_KEEP_MB), larger ones are freed when the call returns. */
/* CSP_MEM_HOST calls stage through per-device arenas (one device allocation + 16 MB of page-locked memory each) that are
 * cached between calls, so that the reference's call pattern -- one flight per call, uavPathPlanning.cpp:4423/:4461 -- does
 * not pay hipMalloc/hipFree every time.  This frees the arenas no call is using (optional; e.g. before a long idle phase). */
void csp_minsnap_release_cached_memory(void);

const char *csp_minsnap_version(void);
const char *csp_minsnap_strerror(int status);
const char *csp_minsnap_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif /* CSP_MINSNAP_H_ */
