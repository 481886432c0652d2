// minsnap_timeopt.hip -- the snap cost J(T) that csp_minsnap_solve_batch minimises, its gradient with respect to the
// segment times, and a per-trajectory optimiser of the times (orders 2..5, uniform or ragged, fp64 storage or fp32
// storage with fp64 arithmetic, zero-velocity penalty).  DESIGN.md §12.
//
//   J(T)      = sum_axes sum_j d_j^T Qt^w_j(T_j) d_j
//   dJ/dT_j   = (1/T_j) sum_axes sum_ab (deriv_a + deriv_b + 1 - 2o) Qt_ab(T_j) d_a d_b      (envelope theorem)
// d_j are segment j's endpoint derivatives at the optimum.  With dh_a = T^deriv_a d_a, Qt_ab(T) d_a d_b =
// QT_ab T^(1-2o) dh_a dh_b, so per segment and axis one product u = QT dh gives both sums:
//   d^T Qt d = T^(1-2o) dh.u      and      T dJ/dT = -T^(1-2o) [ (2o-1) dh.u - 2 sum_a deriv_a dh_a u_a ].
// The +w velocity diagonal does not depend on T and only enters J.
//
// Layout as minsnap_generic.hip: one lane per trajectory, workgroups of one wave, the block-LDL^T factors in a
// [waypoint][entry][trajectory] workspace.  One evaluation ("pass") is the forward sweep and the back substitution;
// coefficients are not recovered.  The optimiser runs the whole spectral projected gradient loop per lane inside one
// launch; its vectors (current and trial times, their gradients) live in the workspace, [buffer][segment][trajectory].
// There is no separate cost-only pass for the line search: a Barzilai-Borwein trial is usually accepted, and the full
// pass at the trial already holds the gradient the next iteration needs, where a cost-only trial would need a second
// pass after every acceptance.
#include "minsnap_device.h"
#include "minsnap_launch.h"
#include "minsnap_spg.h"

namespace csp {

namespace {

// a waypoint relative to the trajectory's first one (J and the free derivatives do not depend on a translation; the
// right-hand sides then cancel less)
template <typename IO>
__device__ __forceinline__ void tload3(const IO *p, const double (&org)[3], double (&v)[3]) {
    v[0] = double(p[0]) - org[0]; v[1] = double(p[1]) - org[1]; v[2] = double(p[2]) - org[2];
}

// One evaluation at the times tm[j * ts], j < S: returns J and writes dJ/dT_j to g[j * gs] (when g is non-null).
// Status bits as the solve: NOT_SPD for a pivot <= 0, NONFINITE when J or a gradient is inf/NaN.
template <int O, typename IO, typename TT, typename GT>
__device__ int cost_pass(const IO *wp, const TT *tm, int64_t ts, const double (&x0)[O - 1][3], const double (&xS)[O - 1][3],
                         double vw, double *ws, int64_t B, int S, GT *g, int64_t gs, double &J) {
    constexpr int N = O - 1;
    constexpr int M = 2 * O;
    constexpr int E = N * N + 3 * N;
    int status = 0;
    const double org[3] = {double(wp[0]), double(wp[1]), double(wp[2])};

    if (S > 1) {
        double W[N][N], z[N][3];
#pragma unroll
        for (int r = 0; r < N; ++r) {
#pragma unroll
            for (int c = 0; c < N; ++c) W[r][c] = 0.0;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) z[r][ax] = x0[r][ax];
        }
        double Pp[3], Pc[3], Pn[3], Pnn[3] = {0.0, 0.0, 0.0};
        tload3<IO>(wp, org, Pp);
        tload3<IO>(wp + 3, org, Pc);
        tload3<IO>(wp + 6, org, Pn);
        double Tn = double(tm[ts]), Tnn = 1.0;
        SegBlocks<O, double> left, right;
        seg_blocks<O, double, false>(double(tm[0]), vw, 0.0, 0, Pp, Pc, left);
        for (int k = 1; k < S; ++k) {
            if (k + 1 < S) {  // prefetch waypoint k+2 and time k+1
                tload3<IO>(wp + 3 * (k + 2), org, Pnn);
                Tnn = double(tm[(int64_t)(k + 1) * ts]);
            }
            seg_blocks<O, double, false>(Tn, vw, 0.0, 0, Pc, Pn, right);
            double A[N][N], Bm[N][N + 3];
#pragma unroll
            for (int r = 0; r < N; ++r) {
#pragma unroll
                for (int c = 0; c < N; ++c) {
                    double v = left.ee[r][c] + right.ss[r][c];
#pragma unroll
                    for (int j = 0; j < N; ++j) v = fma_<double>(-left.se[j][r], W[j][c], v);
                    A[r][c] = v;
                    Bm[r][c] = right.se[r][c];
                }
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    // Qt annihilates constants (ep0 = -ep1, sp0 = -sp1): the two legs, not four nearly opposite
                    // products of the waypoints, which lose |P| / |leg| digits
                    double v = left.ep1[r] * (Pc[ax] - Pp[ax]);
                    v = fma_<double>(right.sp1[r], Pn[ax] - Pc[ax], v);
#pragma unroll
                    for (int j = 0; j < N; ++j) v = fma_<double>(left.se[j][r], z[j][ax], v);
                    Bm[r][N + ax] = -v;
                }
            }
            const double piv = spd_solve<N, N + 3, double>(A, Bm);
            if (!(piv > 0.0)) status |= CSP_TRAJ_NOT_SPD_BIT;
            double *wk = ws + (int64_t)(k - 1) * E * B;
#pragma unroll
            for (int r = 0; r < N; ++r) {
#pragma unroll
                for (int c = 0; c < N; ++c) { W[r][c] = Bm[r][c]; wk[(int64_t)(r * N + c) * B] = W[r][c]; }
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) { z[r][ax] = Bm[r][N + ax]; wk[(int64_t)(N * N + r * 3 + ax) * B] = z[r][ax]; }
            }
            left = right;
            Tn = Tnn;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { Pp[ax] = Pc[ax]; Pc[ax] = Pn[ax]; Pn[ax] = Pnn[ax]; }
        }
    }

    // back substitution; per segment the cost and the time gradient
    double xn[N][3];
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) xn[r][ax] = xS[r][ax];
    double nanacc = 0.0, Jacc = 0.0;
    double Tk = double(tm[(int64_t)(S - 1) * ts]), P0[3], P1[3], wz[E];
    tload3<IO>(wp + 3 * (S - 1), org, P0);
    tload3<IO>(wp + 3 * S, org, P1);
    if (S > 1) {
        const double *wk = ws + (int64_t)(S - 2) * E * B;
#pragma unroll
        for (int e = 0; e < E; ++e) wz[e] = wk[(int64_t)e * B];
    }
    for (int k = S - 1; k >= 0; --k) {
        double Tp = 1.0, Pm[3] = {0.0, 0.0, 0.0}, wzp[E];
        if (k >= 1) {  // prefetch segment k-1: its time, start waypoint and factors
            Tp = double(tm[(int64_t)(k - 1) * ts]);
            tload3<IO>(wp + 3 * (k - 1), org, Pm);
            if (k >= 2) {
                const double *wk = ws + (int64_t)(k - 2) * E * B;
#pragma unroll
                for (int e = 0; e < E; ++e) wzp[e] = wk[(int64_t)e * B];
            }
        }
        double xk[N][3];
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                if (k == 0) { xk[r][ax] = x0[r][ax]; continue; }
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
        if (g) {
            const double gk = -(ipw * it) * fma_<double>(double(M - 1), s0, -2.0 * s1);
            g[(int64_t)k * gs] = GT(gk);
            nanacc = fma_<double>(double(GT(gk)), 0.0, nanacc);
        }
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

template <int O, typename IO>
__device__ __forceinline__ void load_bc(const TimeOptArgs &a, int64_t b, double (&x0)[O - 1][3], double (&xS)[O - 1][3]) {
    const IO *bc = (const IO *)a.bc + (a.bc_per_traj ? b * 12 : 0);
#pragma unroll
    for (int r = 0; r < O - 1; ++r)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            x0[r][ax] = r == 0 ? double(bc[0 * 3 + ax]) : r == 1 ? double(bc[2 * 3 + ax]) : 0.0;
            xS[r][ax] = r == 0 ? double(bc[1 * 3 + ax]) : r == 1 ? double(bc[3 * 3 + ax]) : 0.0;
        }
}

}  // namespace

// csp_minsnap_cost_batch: J and (optionally) dJ/dT at the given times, one lane per trajectory.
template <int O, typename IO>
__global__ void __launch_bounds__(64) minsnap_cost_kernel(TimeOptArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    int64_t seg0;
    int S;
    if (a.seg_off) { seg0 = a.seg_off[b]; S = (int)(a.seg_off[b + 1] - seg0); }
    else { seg0 = b * (int64_t)a.S; S = a.S; }
    int status = 0;
    double J = 0.0;
    if (S >= 1) {
        double x0[O - 1][3], xS[O - 1][3];
        load_bc<O, IO>(a, b, x0, xS);
        const double vw = a.vw_per ? a.vw_per[b] : a.vel_zero_weight;
        status = cost_pass<O, IO, IO, IO>((const IO *)a.wp + (seg0 + b) * 3, (const IO *)a.times + seg0, 1, x0, xS, vw,
                                          (double *)a.ws + b, a.B, S, a.grad ? (IO *)a.grad + seg0 : (IO *)nullptr, 1, J);
    }
    a.cost[b] = J;
    if (a.status) a.status[b] = status;
}

// csp_minsnap_optimize_times_batch: the spectral projected gradient loop of minsnap_spg.h (shared with the optimiser under
// per-knot constraints, minsnap_knots_timeopt.hip) over cost_pass.
template <int O, typename IO>
__global__ void __launch_bounds__(64) minsnap_timeopt_kernel(TimeOptArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    int64_t seg0;
    int S;
    if (a.seg_off) { seg0 = a.seg_off[b]; S = (int)(a.seg_off[b + 1] - seg0); }
    else { seg0 = b * (int64_t)a.S; S = a.S; }
    const IO *tin = (const IO *)a.times + seg0;
    IO *tout = (IO *)a.times_out + seg0;
    const int64_t B = a.B;
    const int64_t plane = (int64_t)a.Smax * B;
    double *Tb[2] = {a.vec + b, a.vec + plane + b};              // times, [segment][trajectory]
    double *Gb[2] = {a.vec + 2 * plane + b, a.vec + 3 * plane + b};   // dJ/dT at those times
    const bool ft = a.mode == CSP_TIMEOPT_FIXED_TOTAL_V;
    const double lo = a.min_time, rho = ft ? 0.0 : a.time_weight;

    int status = 0, iters = 0;
    double f0 = 0.0, f = 0.0;
    if (S >= 1) {
        double C;
        const int stop = spg_start<IO>(tin, S, ft, lo, Tb[0], B, C);
        if (stop) {
            // the times are left as they came and nothing was evaluated
            for (int j = 0; j < S; ++j) tout[j] = tin[j];
            if (a.objective) { a.objective[2 * b] = __builtin_nan(""); a.objective[2 * b + 1] = __builtin_nan(""); }
            if (a.iterations) a.iterations[b] = 0;
            if (a.status) a.status[b] = stop;
            return;
        }
        double x0[O - 1][3], xS[O - 1][3];
        load_bc<O, IO>(a, b, x0, xS);
        const double vw = a.vw_per ? a.vw_per[b] : a.vel_zero_weight;
        const IO *wp = (const IO *)a.wp + (seg0 + b) * 3;
        double *ws = (double *)a.ws + b;
        const SpgResult r = spg_minimise(
            [&](int eb, double &J) { return cost_pass<O, IO, double, double>(wp, Tb[eb], B, x0, xS, vw, ws, B, S, Gb[eb], B, J); },
            Tb, Gb, B, S, ft, C, lo, rho, a.tol, a.max_iters);
        status = r.status; iters = r.iters; f0 = r.f0; f = r.f;
        for (int j = 0; j < S; ++j) tout[j] = IO(Tb[r.cur][(int64_t)j * B]);
    }
    if (a.objective) { a.objective[2 * b] = f0; a.objective[2 * b + 1] = f; }
    if (a.iterations) a.iterations[b] = iters;
    if (a.status) a.status[b] = status;
}

template <int O, typename IO> static hipError_t launch_o(const TimeOptArgs &a, bool opt, hipStream_t st) {
    const unsigned blocks = (unsigned)((a.B + 63) / 64);
    if (opt) hipLaunchKernelGGL((minsnap_timeopt_kernel<O, IO>), dim3(blocks), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((minsnap_cost_kernel<O, IO>), dim3(blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

template <typename IO> static hipError_t launch_io(const TimeOptArgs &a, bool opt, hipStream_t st) {
    switch (a.order) {
        case 2: return launch_o<2, IO>(a, opt, st);
        case 3: return launch_o<3, IO>(a, opt, st);
        case 4: return launch_o<4, IO>(a, opt, st);
        case 5: return launch_o<5, IO>(a, opt, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_cost(const TimeOptArgs &a, bool f32, hipStream_t st) {
    if (a.B == 0) return hipSuccess;
    return f32 ? launch_io<float>(a, false, st) : launch_io<double>(a, false, st);
}

hipError_t launch_timeopt(const TimeOptArgs &a, bool f32, hipStream_t st) {
    if (a.B == 0) return hipSuccess;
    return f32 ? launch_io<float>(a, true, st) : launch_io<double>(a, true, st);
}

}  // namespace csp
