// minsnap_knots_timeopt.hip -- the segment-time optimiser under per-knot derivative constraints (orders 2..5, uniform or
// ragged, fp64 storage or fp32 storage with fp64 arithmetic, zero-velocity penalty).  DESIGN.md §23.
//
// Three existing pieces joined: the masked block-LDL^T sweep over all S + 1 knots of minsnap_knots.hip (its pinning rule,
// unchanged), the per-segment quadratic form of minsnap_timeopt.hip's cost_pass (cost and envelope-theorem gradient from
// one product u = QT dh), and the spectral projected gradient loop of minsnap_spg.h, which both optimisers instantiate.
//
//   J(T)    = sum_axes sum_j d_j^T Qt^w_j(T_j) d_j,    d_j = segment j's endpoint derivatives at the optimum of the
//                                                      partition the mask describes,
//   dJ/dT_j = (1/T_j) sum_axes sum_ab (deriv_a + deriv_b + 1 - 2o) Qt_ab(T_j) d_a d_b.
// The envelope theorem holds under any partition: a pinned derivative does not depend on T, a free one sits at the
// optimum, where dJ/d(free) = 0; either way only the explicit dependence of Qt on T_j is left.
//
// Layout as both parents: one lane per trajectory, workgroups of one wave, W_k and z_k of knots 0..S-1 in a
// [knot][entry][trajectory] workspace (knot S's stay in registers), both sweeps software-pipelined one knot ahead (a
// knot's mask and values travel with its waypoint), the optimiser's vectors [buffer][segment][trajectory] behind the
// factors.  No coefficients are recovered here: the C-ABI launches the knots solve at the returned times.
#include "minsnap_device.h"
#include "minsnap_launch.h"
#include "minsnap_knots_timeopt.h"
#include "minsnap_mixed.h"   // CSP_TRAJ_SKIPPED_BIT
#include "minsnap_spg.h"

namespace csp {

namespace {

template <typename IO>
__device__ __forceinline__ void ktload3(const IO *p, const double (&org)[3], double (&v)[3]) {
    v[0] = double(p[0]) - org[0]; v[1] = double(p[1]) - org[1]; v[2] = double(p[2]) - org[2];
}

// mask and pinned values of one knot; a free derivative's entry is replaced by 0 with a select, never by arithmetic,
// so that whatever the caller left there (NaN, inf) goes nowhere
template <int N, typename IO>
__device__ __forceinline__ void ktload_pins(const uint8_t *mk, const IO *kv, unsigned &m, double (&pv)[N][3]) {
    m = (unsigned)mk[0] & ((1u << N) - 1u);
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double v = double(kv[r * 3 + ax]);
            pv[r][ax] = ((m >> r) & 1u) ? v : 0.0;
        }
}

// One evaluation at the times tm[j * ts], j < S, of the problem the mask describes: returns J and writes dJ/dT_j to
// g[j * gs].  The count rule is the caller's (it does not depend on the times).  Status bits as the knots solve:
// NOT_SPD for a pivot <= 0 or a time that is not > 0, NONFINITE when J or a gradient is inf/NaN.
template <int O, typename IO, typename TT, typename GT>
__device__ int knots_cost_pass(const IO *wp, const TT *tm, int64_t ts, const uint8_t *mk, const IO *kv, double vw,
                               double *ws, int64_t B, int S, GT *g, int64_t gs, double &J) {
    constexpr int N = O - 1;
    constexpr int M = 2 * O;
    constexpr int E = N * N + 3 * N;
    int status = 0;
    const double org[3] = {double(wp[0]), double(wp[1]), double(wp[2])};

    // ---- forward sweep over knots 0..S
    double z[N][3];   // after the sweep: z_S = x_S
    {
        double W[N][N];
        SegBlocks<O, double> left, right;
#pragma unroll
        for (int r = 0; r < N; ++r) {
#pragma unroll
            for (int c = 0; c < N; ++c) { W[r][c] = 0.0; left.ee[r][c] = 0.0; left.se[r][c] = 0.0; }
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) z[r][ax] = 0.0;
            left.ep1[r] = 0.0;
        }
        double Pp[3] = {0.0, 0.0, 0.0}, Pc[3] = {0.0, 0.0, 0.0}, Pn[3], Pnn[3] = {0.0, 0.0, 0.0};
        ktload3<IO>(wp + 3, org, Pn);
        double Tn = double(tm[0]), Tnn = 1.0;
        unsigned mp = 0, mc, mn, mnn = 0;
        double pvp[N][3], pvc[N][3], pvn[N][3], pvnn[N][3];
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { pvp[r][ax] = 0.0; pvnn[r][ax] = 0.0; }
        ktload_pins<N, IO>(mk, kv, mc, pvc);
        ktload_pins<N, IO>(mk + 1, kv + 3 * N, mn, pvn);
        for (int k = 0; k <= S; ++k) {
            if (k + 2 <= S) {   // prefetch knot k+2 (waypoint, mask, values) and time k+1
                ktload3<IO>(wp + 3 * (k + 2), org, Pnn);
                ktload_pins<N, IO>(mk + (k + 2), kv + (int64_t)(k + 2) * (3 * N), mnn, pvnn);
                Tnn = double(tm[(int64_t)(k + 1) * ts]);
            } else {            // past the last knot: no segment, nothing pinned
                Tnn = 1.0;
                mnn = 0;
#pragma unroll
                for (int r = 0; r < N; ++r)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) pvnn[r][ax] = 0.0;
            }
            seg_blocks<O, double, false>(Tn, vw, 0.0, 0, Pc, Pn, right);   // segment k: knot k -> knot k+1
            // Qt(T) of a time <= 0 (or NaN) is not positive semi-definite, yet the pivots of the masked system may all
            // come out positive (pinned neighbours, a positive block beside it): flagged from the time itself
            if (!(Tn > 0.0)) status |= CSP_TRAJ_NOT_SPD_BIT;
            if (k == S) {   // the last knot has no segment to its right (Tn = 1 there)
#pragma unroll
                for (int r = 0; r < N; ++r) {
#pragma unroll
                    for (int c = 0; c < N; ++c) { right.ss[r][c] = 0.0; right.se[r][c] = 0.0; }
                    right.sp1[r] = 0.0;
                }
            }
            double A[N][N], Bm[N][N + 3], Lse[N][N];
#pragma unroll
            for (int j = 0; j < N; ++j)
#pragma unroll
                for (int r = 0; r < N; ++r)   // C_{k-1} without row j of a pinned j (knot k-1), column r of a pinned r
                    Lse[j][r] = (((mp >> j) | (mc >> r)) & 1u) ? 0.0 : left.se[j][r];
#pragma unroll
            for (int r = 0; r < N; ++r) {
                const bool pr = (mc >> r) & 1u;
#pragma unroll
                for (int c = 0; c < N; ++c) {
                    const bool pc = (mc >> c) & 1u;
                    double v = left.ee[r][c] + right.ss[r][c];
#pragma unroll
                    for (int j = 0; j < N; ++j) v = fma_<double>(-Lse[j][r], W[j][c], v);
                    A[r][c] = (pr || pc) ? (r == c ? 1.0 : 0.0) : v;
                    Bm[r][c] = (pr || ((mn >> c) & 1u)) ? 0.0 : right.se[r][c];
                }
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    // Qt annihilates constants (ep0 = -ep1, sp0 = -sp1): the two legs, not four nearly opposite
                    // products of the waypoints, which lose |P| / |leg| digits.  The first
                    // knot has no left leg (ep1 = 0 there), the last no right one (sp1 = 0).
                    double v = left.ep1[r] * (Pc[ax] - Pp[ax]);
                    v = fma_<double>(right.sp1[r], Pn[ax] - Pc[ax], v);
                    // the pinned unknowns of knots k-1, k, k+1 (pv is 0 for a free one)
#pragma unroll
                    for (int c = 0; c < N; ++c) {
                        v = fma_<double>(left.se[c][r], pvp[c][ax], v);
                        v = fma_<double>(left.ee[r][c] + right.ss[r][c], pvc[c][ax], v);
                        v = fma_<double>(right.se[r][c], pvn[c][ax], v);
                    }
#pragma unroll
                    for (int j = 0; j < N; ++j) v = fma_<double>(Lse[j][r], z[j][ax], v);
                    Bm[r][N + ax] = pr ? pvc[r][ax] : -v;
                }
            }
            const double piv = spd_solve<N, N + 3, double>(A, Bm);
            if (!(piv > 0.0)) status |= CSP_TRAJ_NOT_SPD_BIT;
#pragma unroll
            for (int r = 0; r < N; ++r) {
#pragma unroll
                for (int c = 0; c < N; ++c) W[r][c] = Bm[r][c];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) z[r][ax] = Bm[r][N + ax];
            }
            if (k < S) {   // knot S's factors stay in registers: W_S = 0, z_S = x_S
                double *wk = ws + (int64_t)k * E * B;
#pragma unroll
                for (int r = 0; r < N; ++r) {
#pragma unroll
                    for (int c = 0; c < N; ++c) wk[(int64_t)(r * N + c) * B] = W[r][c];
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) wk[(int64_t)(N * N + r * 3 + ax) * B] = z[r][ax];
                }
            }
            left = right;
            Tn = Tnn;
            mp = mc; mc = mn; mn = mnn;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { Pp[ax] = Pc[ax]; Pc[ax] = Pn[ax]; Pn[ax] = Pnn[ax]; }
#pragma unroll
            for (int r = 0; r < N; ++r)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) { pvp[r][ax] = pvc[r][ax]; pvc[r][ax] = pvn[r][ax]; pvn[r][ax] = pvnn[r][ax]; }
        }
    }

    // ---- back substitution over segments S-1..0; per segment the cost and the time gradient (cost_pass's form)
    double xn[N][3];   // the end knot of segment k
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) xn[r][ax] = z[r][ax];
    double nanacc = 0.0, Jacc = 0.0;
    double Tk = double(tm[(int64_t)(S - 1) * ts]), P0[3], P1[3], wz[E];
    ktload3<IO>(wp + 3 * (S - 1), org, P0);
    ktload3<IO>(wp + 3 * S, org, P1);
    {
        const double *wk = ws + (int64_t)(S - 1) * E * B;
#pragma unroll
        for (int e = 0; e < E; ++e) wz[e] = wk[(int64_t)e * B];
    }
    for (int k = S - 1; k >= 0; --k) {
        double Tp = 1.0, Pm[3] = {0.0, 0.0, 0.0}, wzp[E];
        if (k >= 1) {   // prefetch segment k-1: its time, start waypoint and the factors of knot k-1
            Tp = double(tm[(int64_t)(k - 1) * ts]);
            ktload3<IO>(wp + 3 * (k - 1), org, Pm);
            const double *wk = ws + (int64_t)(k - 1) * E * B;
#pragma unroll
            for (int e = 0; e < E; ++e) wzp[e] = wk[(int64_t)e * B];
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) wzp[e] = 0.0;
        }
        double xk[N][3];
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                double v = wz[N * N + r * 3 + ax];
#pragma unroll
                for (int c = 0; c < N; ++c) v = fma_<double>(-wz[r * N + c], xn[c][ax], v);
                xk[r][ax] = v;
            }
        double tp[O];
        tp[0] = 1.0;
#pragma unroll
        for (int e = 1; e < O; ++e) tp[e] = tp[e - 1] * Tk;
        const double it = fast_rcp(Tk);
        double s0 = 0.0, s1 = 0.0, vel = 0.0;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            double dh[M];
            dh[0] = 0.0;              // the segment's start as origin: Qt annihilates constants, and the quadratic
            dh[O] = P1[ax] - P0[ax];  // form then sums smaller terms
#pragma unroll
            for (int r = 0; r < N; ++r) { dh[r + 1] = xk[r][ax] * tp[r + 1]; dh[O + r + 1] = xn[r][ax] * tp[r + 1]; }
            vel = fma_<double>(xk[0][ax], xk[0][ax], vel);
            vel = fma_<double>(xn[0][ax], xn[0][ax], vel);
#pragma unroll
            for (int aa = 0; aa < M; ++aa) {
                double u = 0.0;
#pragma unroll
                for (int bb = 0; bb < M; ++bb) {
                    constexpr double zero = 0.0;
                    if (Tab<O>::QT(aa, bb) != zero) u = fma_<double>(Tab<O>::QT(aa, bb), dh[bb], u);
                }
                s0 = fma_<double>(dh[aa], u, s0);
                if (aa % O) s1 = fma_<double>(double(aa % O) * dh[aa], u, s1);
            }
        }
        double ipw = it;   // T^(1-2o)
#pragma unroll
        for (int e = 2; e < M; ++e) ipw *= it;
        Jacc += fma_<double>(vw, vel, ipw * s0);
        const double gk = -(ipw * it) * fma_<double>(double(M - 1), s0, -2.0 * s1);
        g[(int64_t)k * gs] = GT(gk);
        nanacc = fma_<double>(double(GT(gk)), 0.0, nanacc);
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) xn[r][ax] = xk[r][ax];
        Tk = Tp;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { P1[ax] = P0[ax]; P0[ax] = Pm[ax]; }
#pragma unroll
        for (int e = 0; e < E; ++e) wz[e] = wzp[e];
    }
    nanacc = fma_<double>(Jacc, 0.0, nanacc);
    if (!(nanacc == 0.0)) status |= CSP_TRAJ_NONFINITE_BIT;
    J = Jacc;
    return status;
}

}  // namespace

// csp_minsnap_optimize_times_knots_batch: the spectral projected gradient loop of minsnap_spg.h over knots_cost_pass.
template <int O, typename IO>
__global__ void __launch_bounds__(64) minsnap_knots_timeopt_kernel(KnotsTimeOptArgs a) {
    constexpr int N = O - 1;
    constexpr unsigned FULL = (1u << N) - 1u;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    int64_t seg0;
    int S;
    if (a.seg_off) { seg0 = a.seg_off[b]; S = (int)(a.seg_off[b + 1] - seg0); }
    else { seg0 = b * (int64_t)a.S; S = a.S; }
    const IO *tin = (const IO *)a.times + seg0;
    IO *tout = (IO *)a.times_out + seg0;
    const uint8_t *mk = a.mask + (seg0 + b);                     // [S+1]
    const IO *kv = (const IO *)a.values + (seg0 + b) * (3 * N);  // [S+1][N][3]
    const int64_t B = a.B;
    const int64_t plane = (int64_t)a.Smax * B;
    double *Tb[2] = {a.vec + b, a.vec + plane + b};              // times, [segment][trajectory]
    double *Gb[2] = {a.vec + 2 * plane + b, a.vec + 3 * plane + b};   // dJ/dT at those times
    const bool ft = a.mode == CSP_TIMEOPT_FIXED_TOTAL_V;
    const double lo = a.min_time, rho = ft ? 0.0 : a.time_weight;

    int status = 0, iters = 0;
    double f0 = 0.0, f = 0.0;
    if (S >= 1) {
        // Stopped before anything is evaluated, the times left as they came: a ragged length the workspace was not sized
        // for (device memory: the host could not check it); the count rule of the knots solve -- with fewer constraints
        // than the order the minimiser is not unique, whatever the times; then the optimiser's own start rules.
        int stop = 0;
        double C = 0.0;
        if (S > a.Smax) {
            stop = CSP_TRAJ_SKIPPED_BIT;
        } else {
            if (S + 1 < O) {
                int count = S + 1;
                for (int k = 0; k <= S; ++k) count += __builtin_popcount((unsigned)mk[k] & FULL);
                if (count < O) stop = CSP_TRAJ_NOT_SPD_BIT;
            }
            if (!stop) stop = spg_start<IO>(tin, S, ft, lo, Tb[0], B, C);
        }
        if (stop) {
            for (int j = 0; j < S; ++j) tout[j] = tin[j];
            if (a.objective) { a.objective[2 * b] = __builtin_nan(""); a.objective[2 * b + 1] = __builtin_nan(""); }
            if (a.iterations) a.iterations[b] = 0;
            if (a.status) a.status[b] = stop;
            return;
        }
        const double vw = a.vw_per ? a.vw_per[b] : a.vel_zero_weight;
        const IO *wp = (const IO *)a.wp + (seg0 + b) * 3;
        double *ws = (double *)a.ws + b;
        const SpgResult r = spg_minimise(
            [&](int eb, double &J) { return knots_cost_pass<O, IO, double, double>(wp, Tb[eb], B, mk, kv, vw, ws, B, S, Gb[eb], B, J); },
            Tb, Gb, B, S, ft, C, lo, rho, a.tol, a.max_iters);
        status = r.status; iters = r.iters; f0 = r.f0; f = r.f;
        for (int j = 0; j < S; ++j) tout[j] = IO(Tb[r.cur][(int64_t)j * B]);
    }
    if (a.objective) { a.objective[2 * b] = f0; a.objective[2 * b + 1] = f; }
    if (a.iterations) a.iterations[b] = iters;
    if (a.status) a.status[b] = status;
}

template <int O, typename IO> static hipError_t launch_o(const KnotsTimeOptArgs &a, hipStream_t st) {
    const unsigned blocks = (unsigned)((a.B + 63) / 64);
    hipLaunchKernelGGL((minsnap_knots_timeopt_kernel<O, IO>), dim3(blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

template <typename IO> static hipError_t launch_io(const KnotsTimeOptArgs &a, hipStream_t st) {
    switch (a.order) {
        case 2: return launch_o<2, IO>(a, st);
        case 3: return launch_o<3, IO>(a, st);
        case 4: return launch_o<4, IO>(a, st);
        case 5: return launch_o<5, IO>(a, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_knots_timeopt(const KnotsTimeOptArgs &a, bool f32, hipStream_t st) {
    if (a.B == 0) return hipSuccess;
    return f32 ? launch_io<float>(a, st) : launch_io<double>(a, st);
}

}  // namespace csp
