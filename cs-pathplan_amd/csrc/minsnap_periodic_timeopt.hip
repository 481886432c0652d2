// minsnap_periodic_timeopt.hip -- the lap-time optimiser of the periodic (closed-loop) solve (orders 2..5, uniform or
// ragged, fp64 storage or fp32 storage with fp64 arithmetic, zero-velocity penalty).  DESIGN.md §24.
//
// Three existing pieces joined: the bordered block-LDL^T sweep of minsnap_periodic.hip (knot 0 is the border, knots
// 1..S-1 are swept carrying W_k, V_k, z_k), the per-segment quadratic form of minsnap_timeopt.hip's cost_pass (cost and
// envelope-theorem gradient from the sums s0 and s1, evaluated here through the segment's monomial coefficients), and
// the spectral projected gradient loop of minsnap_spg.h.
//
//   J(T)    = sum_axes sum_j d_j^T Qt^w_j(T_j) d_j,    d_j = segment j's endpoint derivatives at the loop's optimum,
//   dJ/dT_j = (1/T_j) sum_axes sum_ab (deriv_a + deriv_b + 1 - 2o) Qt_ab(T_j) d_a d_b.
// The envelope theorem holds on the loop: every derivative of every knot is free and sits at the optimum, where
// dJ/d(free) = 0, and the positions do not depend on T; only the explicit dependence of Qt on T_j is left.
//
// Layout as the parent: one lane per loop, workgroups of one wave, W_k, V_k, z_k of knots 1..S-1 in a
// [knot][entry][trajectory] workspace, both sweeps software-pipelined one knot ahead, the optimiser's vectors
// [buffer][segment][trajectory] behind the factors.  No coefficients are recovered here: the C-ABI launches the periodic
// solve at the returned times.
#include "minsnap_device.h"
#include "minsnap_launch.h"
#include "minsnap_periodic_timeopt.h"
#include "minsnap_mixed.h"   // CSP_TRAJ_SKIPPED_BIT
#include "minsnap_spg.h"

namespace csp {

namespace {

template <typename IO>
__device__ __forceinline__ void ptload3(const IO *p, double (&v)[3]) {
    v[0] = double(p[0]); v[1] = double(p[1]); v[2] = double(p[2]);
}

// Q(1) of one segment over its top o monomial coefficients, highest power first (row i is power 2o-1-i):
// int_0^1 (t^p)^(o) (t^q)^(o) dt = p!/(p-o)! q!/(q-o)! / (p + q - 2o + 1), an integer for orders 2..5 (the division is
// exact, cs-pathplan_amd/tablegen.py q_unit).  Tab<O>::QT is G^T Q G with Tab<O>::G.
template <int O> __device__ constexpr double mono_q(int i, int l) {
    const int p = 2 * O - 1 - i, q = 2 * O - 1 - l;
    double f = 1.0;
    for (int j = 0; j < O; ++j) f *= double((p - j) * (q - j));
    return f / double(p + q - 2 * O + 1);
}

// One evaluation of the loop wp[0..S-1] at the times tm[j * ts], j < S: returns J and writes dJ/dT_j to g[j * gs].
// Status bits as the periodic solve: NOT_SPD for a pivot <= 0 (the border's Schur complement included) or a time that is
// not > 0, NONFINITE when J or a gradient is inf/NaN.
template <int O, typename IO, typename TT, typename GT>
__device__ int periodic_cost_pass(const IO *wp, const TT *tm, int64_t ts, double vw, double *ws, int64_t B, int S, GT *g,
                                  int64_t gs, double &J) {
    constexpr int N = O - 1;
    constexpr int M = 2 * O;
    constexpr int E = 2 * N * N + 3 * N;   // W, V, z per knot
    int status = 0;

    // ---- forward sweep over knots 1..S-1; Sig / r0 accumulate the border's Schur complement and right-hand side.
    // Right-hand sides from the legs: Qt annihilates constants (ep0 = -ep1, sp0 = -sp1), so knot k's is
    // -(ep1_{k-1} (P_k - P_{k-1}) + sp1_k (P_{k+1} - P_k)), not four nearly opposite products.
    double Sig[N][N], r0[N][3];
    {
        double P0[3], P1[3];
        ptload3<IO>(wp, P0);
        ptload3<IO>(wp + 3 * (S > 1 ? 1 : 0), P1);
        const double T0 = double(tm[0]);
        if (!(T0 > 0.0)) status |= CSP_TRAJ_NOT_SPD_BIT;
        SegBlocks<O, double> left;
        seg_blocks<O, double, false>(T0, vw, 0.0, 0, P0, P1, left);
        // knot 0's own terms from segment 0 (its start)
#pragma unroll
        for (int r = 0; r < N; ++r) {
#pragma unroll
            for (int c = 0; c < N; ++c) Sig[r][c] = left.ss[r][c];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) r0[r][ax] = -(left.sp1[r] * (P1[ax] - P0[ax]));
        }
        if (S == 1) {
            // one knot: segment 0 also ends there and couples the knot to itself; both legs are 0
#pragma unroll
            for (int r = 0; r < N; ++r)
#pragma unroll
                for (int c = 0; c < N; ++c) Sig[r][c] += left.ee[r][c] + (left.se[r][c] + left.se[c][r]);
        } else {
            double W[N][N], V[N][N], z[N][3];
            double Pp[3], Pc[3], Pn[3], Pnn[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { Pp[ax] = P0[ax]; Pc[ax] = P1[ax]; }
            ptload3<IO>(wp + 3 * (2 % S), Pn);
            double Tn = double(tm[ts]), Tnn = 1.0;
            SegBlocks<O, double> right;
            for (int k = 1; k < S; ++k) {
                if (k + 1 < S) {   // prefetch waypoint k+2 (mod S) and time k+1
                    const int kn = k + 2 >= S ? k + 2 - S : k + 2;
                    ptload3<IO>(wp + 3 * kn, Pnn);
                    Tnn = double(tm[(int64_t)(k + 1) * ts]);
                }
                seg_blocks<O, double, false>(Tn, vw, 0.0, 0, Pc, Pn, right);   // segment k: knot k -> knot k+1 (mod S)
                if (!(Tn > 0.0)) status |= CSP_TRAJ_NOT_SPD_BIT;
                const bool last = k == S - 1;
                double A[N][N], G[N][N], Bm[N][2 * N + 3];
#pragma unroll
                for (int r = 0; r < N; ++r) {
#pragma unroll
                    for (int c = 0; c < N; ++c) {
                        double v = left.ee[r][c] + right.ss[r][c];
                        double gg = k == 1 ? left.se[c][r] : 0.0;
                        if (k > 1) {
#pragma unroll
                            for (int j = 0; j < N; ++j) {
                                v = fma_<double>(-left.se[j][r], W[j][c], v);
                                gg = fma_<double>(-left.se[j][r], V[j][c], gg);
                            }
                        }
                        if (last) gg += right.se[r][c];   // the corner C_{S-1} (S = 2: C_0^T + C_1)
                        A[r][c] = v;
                        G[r][c] = gg;
                        Bm[r][c] = last ? 0.0 : right.se[r][c];
                        Bm[r][N + c] = gg;
                    }
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        double v = left.ep1[r] * (Pc[ax] - Pp[ax]);
                        v = fma_<double>(right.sp1[r], Pn[ax] - Pc[ax], v);
                        if (k > 1) {
#pragma unroll
                            for (int j = 0; j < N; ++j) v = fma_<double>(left.se[j][r], z[j][ax], v);
                        }
                        Bm[r][2 * N + ax] = -v;
                    }
                }
                const double piv = spd_solve<N, 2 * N + 3, double>(A, Bm);
                if (!(piv > 0.0)) status |= CSP_TRAJ_NOT_SPD_BIT;
                double *wk = ws + (int64_t)(k - 1) * E * B;
#pragma unroll
                for (int r = 0; r < N; ++r) {
#pragma unroll
                    for (int c = 0; c < N; ++c) {
                        W[r][c] = Bm[r][c];
                        V[r][c] = Bm[r][N + c];
                        if (!last) wk[(int64_t)(r * N + c) * B] = W[r][c];   // W_{S-1} = 0 is never read
                        wk[(int64_t)(N * N + r * N + c) * B] = V[r][c];
                    }
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        z[r][ax] = Bm[r][2 * N + ax];
                        wk[(int64_t)(2 * N * N + r * 3 + ax) * B] = z[r][ax];
                    }
                }
                // border: Sig -= G^T V_k, r0 -= G^T z_k
#pragma unroll
                for (int r = 0; r < N; ++r) {
#pragma unroll
                    for (int c = 0; c < N; ++c) {
                        double v = Sig[r][c];
#pragma unroll
                        for (int j = 0; j < N; ++j) v = fma_<double>(-G[j][r], V[j][c], v);
                        Sig[r][c] = v;
                    }
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        double v = r0[r][ax];
#pragma unroll
                        for (int j = 0; j < N; ++j) v = fma_<double>(-G[j][r], z[j][ax], v);
                        r0[r][ax] = v;
                    }
                }
                left = right;
                Tn = Tnn;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) { Pp[ax] = Pc[ax]; Pc[ax] = Pn[ax]; Pn[ax] = Pnn[ax]; }
            }
            // knot 0's terms from segment S-1 (its end): left is segment S-1, Pp = P_{S-1}, Pc = P_0 -- the wrap leg
#pragma unroll
            for (int r = 0; r < N; ++r) {
#pragma unroll
                for (int c = 0; c < N; ++c) Sig[r][c] += left.ee[r][c];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) r0[r][ax] = fma_<double>(-left.ep1[r], Pc[ax] - Pp[ax], r0[r][ax]);
            }
        }
    }
    const double piv0 = spd_solve<N, 3, double>(Sig, r0);
    if (!(piv0 > 0.0)) status |= CSP_TRAJ_NOT_SPD_BIT;
    double x0[N][3];
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) x0[r][ax] = r0[r][ax];

    // ---- back substitution over segments S-1..0; per segment the cost and the time gradient (cost_pass's form)
    double xn[N][3];   // the end knot of segment k: knot 0 for k = S-1
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) xn[r][ax] = x0[r][ax];
    double nanacc = 0.0, Jacc = 0.0;
    double Tk = double(tm[(int64_t)(S - 1) * ts]), P0[3], P1[3], wz[E];
    ptload3<IO>(wp + 3 * (S - 1), P0);
    ptload3<IO>(wp, P1);
    if (S > 1) {   // knot S-1: its W was never stored and is 0
        const double *wk = ws + (int64_t)(S - 2) * E * B;
#pragma unroll
        for (int e = 0; e < E; ++e) wz[e] = e < N * N ? 0.0 : wk[(int64_t)e * B];
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) wz[e] = 0.0;
    }
    for (int k = S - 1; k >= 0; --k) {
        double Tp = 1.0, Pm[3] = {0.0, 0.0, 0.0}, wzp[E];
        if (k >= 2) {   // prefetch the factors of knot k-1
            const double *wk = ws + (int64_t)(k - 2) * E * B;
#pragma unroll
            for (int e = 0; e < E; ++e) wzp[e] = wk[(int64_t)e * B];
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) wzp[e] = 0.0;
        }
        if (k >= 1) {   // prefetch segment k-1: its time and start waypoint
            Tp = double(tm[(int64_t)(k - 1) * ts]);
            ptload3<IO>(wp + 3 * (k - 1), Pm);
        }
        double xk[N][3];
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                if (k == 0) { xk[r][ax] = x0[r][ax]; continue; }
                double v = wz[2 * N * N + r * 3 + ax];
#pragma unroll
                for (int c = 0; c < N; ++c) {
                    v = fma_<double>(-wz[r * N + c], xn[c][ax], v);
                    v = fma_<double>(-wz[N * N + r * N + c], x0[c][ax], v);
                }
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
            // s0 = dh^T QT dh and s1 = sum_a deriv_a dh_a (QT dh)_a, through QT = G^T Q G: c = G dh are the segment's top
            // o monomial coefficients in t / T, cd = G (deriv * dh), v = Q c, s0 = c . v, s1 = cd . v.  Near the optimum a
            // short segment is close to a polynomial of degree < o (its share of J is ~T_j of the total while its terms
            // grow as T_j^(1-2o)): dh^T QT dh then cancels to 1e-5 of J at order 5, c . Q c to 1e-10.
            double c[O], cd[O];
#pragma unroll
            for (int i = 0; i < O; ++i) {
                double ci = 0.0, di = 0.0;
#pragma unroll
                for (int aa = 1; aa < M; ++aa) {
                    constexpr double zero = 0.0;
                    if (Tab<O>::G(i, aa) != zero) {
                        ci = fma_<double>(Tab<O>::G(i, aa), dh[aa], ci);
                        if (aa % O) di = fma_<double>(Tab<O>::G(i, aa) * double(aa % O), dh[aa], di);
                    }
                }
                c[i] = ci;
                cd[i] = di;
            }
#pragma unroll
            for (int i = 0; i < O; ++i) {
                double v = 0.0;
#pragma unroll
                for (int l = 0; l < O; ++l) v = fma_<double>(mono_q<O>(i, l), c[l], v);
                s0 = fma_<double>(c[i], v, s0);
                s1 = fma_<double>(cd[i], v, s1);
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

// csp_minsnap_optimize_times_periodic_batch: the spectral projected gradient loop of minsnap_spg.h over
// periodic_cost_pass.
template <int O, typename IO>
__global__ void __launch_bounds__(64) minsnap_periodic_timeopt_kernel(PeriodicTimeOptArgs a) {
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
        // Stopped before anything is evaluated, the times left as they came: a ragged length the workspace was not sized
        // for (device memory: the host could not check it), then the optimiser's own start rules.
        int stop = 0;
        double C = 0.0;
        if (S > a.Smax) stop = CSP_TRAJ_SKIPPED_BIT;
        else stop = spg_start<IO>(tin, S, ft, lo, Tb[0], B, C);
        if (stop) {
            for (int j = 0; j < S; ++j) tout[j] = tin[j];
            if (a.objective) { a.objective[2 * b] = __builtin_nan(""); a.objective[2 * b + 1] = __builtin_nan(""); }
            if (a.iterations) a.iterations[b] = 0;
            if (a.status) a.status[b] = stop;
            return;
        }
        const double vw = a.vw_per ? a.vw_per[b] : a.vel_zero_weight;
        const IO *wp = (const IO *)a.wp + seg0 * 3;   // [S][3], no closing point
        double *ws = (double *)a.ws + b;
        const SpgResult r = spg_minimise(
            [&](int eb, double &J) { return periodic_cost_pass<O, IO, double, double>(wp, Tb[eb], B, vw, ws, B, S, Gb[eb], B, J); },
            Tb, Gb, B, S, ft, C, lo, rho, a.tol, a.max_iters);
        status = r.status; iters = r.iters; f0 = r.f0; f = r.f;
        if (S == 1 && !ft && status == 0 && iters > 0) {
            // One knot: J = 0 for every T (x_0 = 0), the objective is rho T and its minimiser is the bound itself.  The
            // loop has converged onto it up to the rounding of its trial point T + lambda (lo - T); the bound is returned.
            Tb[r.cur][0] = lo;
            f = rho * lo;
        }
        for (int j = 0; j < S; ++j) tout[j] = IO(Tb[r.cur][(int64_t)j * B]);
    }
    if (a.objective) { a.objective[2 * b] = f0; a.objective[2 * b + 1] = f; }
    if (a.iterations) a.iterations[b] = iters;
    if (a.status) a.status[b] = status;
}

template <int O, typename IO> static hipError_t launch_o(const PeriodicTimeOptArgs &a, hipStream_t st) {
    const unsigned blocks = (unsigned)((a.B + 63) / 64);
    hipLaunchKernelGGL((minsnap_periodic_timeopt_kernel<O, IO>), dim3(blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

template <typename IO> static hipError_t launch_io(const PeriodicTimeOptArgs &a, hipStream_t st) {
    switch (a.order) {
        case 2: return launch_o<2, IO>(a, st);
        case 3: return launch_o<3, IO>(a, st);
        case 4: return launch_o<4, IO>(a, st);
        case 5: return launch_o<5, IO>(a, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_periodic_timeopt(const PeriodicTimeOptArgs &a, bool f32, hipStream_t st) {
    if (a.B == 0) return hipSuccess;
    return f32 ? launch_io<float>(a, st) : launch_io<double>(a, st);
}

// One workgroup walks the B + 1 offsets twice: is any trajectory longer than Smax, then the table (see the header).
__global__ void __launch_bounds__(1024) periodic_coeff_offsets_kernel(const int64_t *seg_off, int64_t *out, int64_t B, int Smax) {
    int longer = 0;
    for (int64_t b = threadIdx.x; b < B; b += blockDim.x) longer |= (seg_off[b + 1] - seg_off[b] > (int64_t)Smax) ? 1 : 0;
    const bool none = __syncthreads_or(longer) == 0;
    const int64_t first = seg_off[0];
    for (int64_t i = threadIdx.x; i <= B; i += blockDim.x) out[i] = none ? seg_off[i] : first;
}

hipError_t launch_periodic_coeff_offsets(const int64_t *seg_off, int64_t *out, int64_t B, int Smax, hipStream_t st) {
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(periodic_coeff_offsets_kernel, dim3(1), dim3(1024), 0, st, seg_off, out, B, Smax);
    return hipGetLastError();
}

}  // namespace csp
