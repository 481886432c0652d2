// minsnap_vjp.hip -- reverse mode of the open-chain solve: the vector-Jacobian product of
// (coeffs, J) = (csp_minsnap_solve_batch, csp_minsnap_cost_batch), orders 2..5, uniform or ragged, fp64 storage or fp32
// storage with fp64 arithmetic, zero-velocity penalty.  One kernel, a compile-time flag per cotangent.
//
// PBAR: given p_bar = dL/dcoeffs, per axis
//   d_bar_j = M(T_j)^-T p_bar_j                          (endpoint-derivative space, no inverse at run time)
//   K_ff lambda = d_bar_free                             (the forward's R_PP, shared by the three axes)
//   grad at a fixed slot  = d_bar_F - sum_j (Qt^w_j lambda~_j)_F
//   T_bar_j = (1/T_j) [ sum_a deriv_a d_a d_bar_a - sum_i pow_i p_i p_bar_i
//                       - sum_ab (1-2o+deriv_a+deriv_b) lambda~_a Qt_ab d_b ]
// The primal is re-solved in the same factorisation (6 right-hand sides: 3 primal, 3 adjoint) instead of being rebuilt
// from the forward's coefficients, which may be fp32 and lose digits at large T (cond(M)).  p_bar is read
// twice: once forwards (free slots of d_bar for the adjoint right-hand side) and once in the back substitution (T_bar
// and the fixed-slot gradients).  Storing what the back pass needs would cost as many workspace bytes, written and
// read, as the one extra read.
//
// JBAR: given J_bar = dL/dJ.  Per axis J = d^T K d with K = sum_j P_j^T Qt^w_j P_j and (K d)_free = 0 at the optimum, so
// (envelope theorem, no adjoint solve for the J part):
//   grad at a fixed slot  = d_bar_F - sum_j (Qt^w_j (lambda~_j - 2 J_bar d_j))_F
//   T_bar_j               = [the T_bar_j above] + J_bar dJ/dT_j                   (dJ/dT_j as minsnap_timeopt.hip)
// lambda~ is zero at the fixed slots, so the +w diagonal enters through the J_bar part only, and only at the two
// boundary velocities: +2 J_bar w v.  Per segment one product u = QT dh gives J's time gradient and the fixed-slot
// gradients.
//
// JBAR without PBAR (grad_coeffs null, never read): d_bar = 0 and lambda = 0.  The cost kernel's sweep -- three primal
// right-hand sides, (o-1)^2 + 3(o-1) workspace entries per knot.
//
// Mapping as minsnap_generic.hip / minsnap_timeopt.hip: one lane per trajectory, workgroups of one wave, the block-LDL^T
// factors in a coalesced [waypoint][entry][trajectory] workspace, the next step's inputs requested one step ahead, loops
// over the segments only.  A shared bc's gradient is reduced over the batch in a fixed order (in-wave tree into
// [12][blocks] partials, then one small kernel over them), so results are bit-identical run to run; no atomics.
#include "minsnap_device.h"
#include "minsnap_vjp.h"
#include "minsnap_vjp_device.h"

namespace csp {

using namespace vjpk;   // minsnap_vjp_device.h: vload3, load_rec, dbar_axis, powers, wave_sum

template <int O, typename IO, bool PBAR, bool JBAR>
__global__ void __launch_bounds__(64) minsnap_vjp_kernel(CostVjpArgs a) {
    static_assert(PBAR || JBAR, "a cotangent of the coefficients, of the cost, or both");
    typedef double R;
    constexpr int N = O - 1;
    constexpr int M = 2 * O;
    constexpr int NC = PBAR ? 6 : 3;        // right-hand-side columns: 3 primal (+ 3 adjoint)
    constexpr int E = N * N + NC * N;       // workspace entries per interior waypoint: W (N x N), z (N x NC)
    constexpr int A2 = N >= 2 ? 2 : 1;      // the acceleration slot (an index that exists at order 2, where it is unused)
    // Without JBAR the kernel keeps the statements of the p_bar-only kernel it replaces -- bc held in registers across
    // both loops, the primal and the adjoint column in one fma loop, the end's bc gradient in gbc -- so that its listing
    // and its time stay that kernel's (order 4, fp64: the same instructions but for two kernarg offsets and one register
    // pair).  Order 5 reads bc where it is used, as with JBAR: holding it there spills 116 B instead of
    // 28 and measured 420.8 against 377.1 us (C3) and 944.3 against 744.5 us (ragged),
    // profiles/r06_vjp_merge/speed_rounds_hold_bc_at_order5.jsonl.
    constexpr bool HOLD_BC = !JBAR && O < 5;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t seg0 = 0;
    int S = 0;
    if (b < a.B) {
        if (a.seg_off) { seg0 = a.seg_off[b]; S = (int)(a.seg_off[b + 1] - seg0); }
        else { seg0 = b * (int64_t)a.S; S = a.S; }
    }
    R gbc[4][3];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) gbc[r][ax] = R(0);
    // The end's bc gradient is known after the back substitution's first step and needed after its last.  With JBAR it
    // waits in the lane's own LDS slots, not in 12 registers across the loop (which cost the order-4 cost-only kernel its
    // second wave).  Without JBAR it stays in gbc (no LDS is allocated then): behind the store's branch the compiler no
    // longer fuses d_bar's multiply into the end velocity's subtraction, and grad_bc and grad_times lost their last bit
    // against the earlier kernel in 75 of the 272 fp64 p_bar-only calls of profiles/r06_vjp_merge/bit_equality.txt's grid.
    __shared__ R end_bc[6][64];
    int status = 0;
    if (b < a.B && S < 1) {   // an empty ragged trajectory: its one waypoint (and its bc) get zero gradients
        if (a.grad_wp) {
            IO *gwp = (IO *)a.grad_wp + (seg0 + b) * 3;
            gwp[0] = IO(0); gwp[1] = IO(0); gwp[2] = IO(0);
        }
        if (a.grad_bc && a.bc_per_traj)
            for (int e = 0; e < 12; ++e) ((IO *)a.grad_bc)[b * 12 + e] = IO(0);
    }
    if (S >= 1) {
        const IO *wp = (const IO *)a.wp + (seg0 + b) * 3;
        const IO *tm = (const IO *)a.times + seg0;
        const IO *gco = PBAR ? (const IO *)a.grad_coeffs + seg0 * 3 * M : nullptr;
        IO *gwp = a.grad_wp ? (IO *)a.grad_wp + (seg0 + b) * 3 : nullptr;
        IO *gtm = a.grad_times ? (IO *)a.grad_times + seg0 : nullptr;
        const IO *bc = (const IO *)a.bc + (a.bc_per_traj ? b * 12 : 0);
        R jb = R(0);
        if constexpr (JBAR) jb = a.grad_cost[b];
        const R jb2 = R(2) * jb;
        // fixed boundary derivatives at the start (end = 0) or the end (end = 1): velocity (order >= 2), acceleration
        // (order >= 3), higher ones zero
        auto read_bc = [&](int end, R (&x)[N][3]) {
#pragma unroll
            for (int r = 0; r < N; ++r)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) x[r][ax] = r == 0 ? R(bc[end * 3 + ax]) : r == 1 ? R(bc[(2 + end) * 3 + ax]) : R(0);
        };
        // Read where they are used (the sweep's first step, the back substitution's first and last), or, HOLD_BC, held
        // in registers across both loops as the p_bar-only kernel always held them.
        R held[2][N][3];
        if constexpr (HOLD_BC) { read_bc(0, held[0]); read_bc(1, held[1]); }
        auto load_bc = [&](int end, R (&x)[N][3]) {
            if constexpr (!HOLD_BC) read_bc(end, x);
            else {
#pragma unroll
                for (int r = 0; r < N; ++r)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) x[r][ax] = held[end][r][ax];
            }
        };
        R *ws = (R *)a.ws + b;
        const R vw = (R)(a.vw_per ? a.vw_per[b] : a.vel_zero_weight);

        // ---- forward sweep: block-LDL^T of R_PP with 3 primal (and, PBAR, 3 adjoint) right-hand sides ----
        if (S > 1) {
            R W[N][N], z[N][NC], x0[N][3];
            load_bc(0, x0);
#pragma unroll
            for (int r = 0; r < N; ++r) {
#pragma unroll
                for (int c = 0; c < N; ++c) W[r][c] = R(0);
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    z[r][ax] = x0[r][ax];
                    if (PBAR) z[r][NC - 3 + ax] = R(0);
                }
            }
            R Pp[3], Pc[3], Pn[3], Pnn[3] = {R(0), R(0), R(0)};
            vload3<IO, R>(wp, Pp);
            vload3<IO, R>(wp + 3, Pc);
            vload3<IO, R>(wp + 6, Pn);
            R Tn = R(tm[1]), Tnn = R(1);
            R pbn[3][M], pbnn[3][M];
            // segment 0: the end part of its d_bar is the left contribution of waypoint 1
            R dend[N][3];
            if (PBAR) {
                R pb0[3][M], tp[O], ip[M];
                load_rec<O, IO, R>(gco, pb0);
                load_rec<O, IO, R>(gco + 3 * M, pbn);
                const R T0 = R(tm[0]);
                powers<O, R>(T0, tp, ip);
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    R db[M];
                    dbar_axis<O, O + 1, M, R>(pb0[ax], tp, ip, db);
#pragma unroll
                    for (int r = 0; r < N; ++r) dend[r][ax] = db[O + 1 + r];
                }
            }
            SegBlocks<O, R> left, right;
            seg_blocks<O, R, false>(R(tm[0]), vw, R(0), 0, Pp, Pc, left);
            for (int k = 1; k < S; ++k) {
                if (k + 1 < S) {  // prefetch waypoint k+2, time k+1 (and p_bar of segment k+1)
                    vload3<IO, R>(wp + 3 * (k + 2), Pnn);
                    Tnn = R(tm[k + 1]);
                    if (PBAR) load_rec<O, IO, R>(gco + (int64_t)(k + 1) * 3 * M, pbnn);
                }
                seg_blocks<O, R, false>(Tn, vw, R(0), 0, Pc, Pn, right);
                R dstart[N][3], dnext[N][3];
                if (PBAR) {
                    R tp[O], ip[M];
                    powers<O, R>(Tn, tp, ip);
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        R db[M];
                        dbar_axis<O, 1, O, R>(pbn[ax], tp, ip, db);
                        dbar_axis<O, O + 1, M, R>(pbn[ax], tp, ip, db);
#pragma unroll
                        for (int r = 0; r < N; ++r) { dstart[r][ax] = db[1 + r]; dnext[r][ax] = db[O + 1 + r]; }
                    }
                }
                R A[N][N], Bm[N][N + NC];
#pragma unroll
                for (int r = 0; r < N; ++r) {
#pragma unroll
                    for (int c = 0; c < N; ++c) {
                        R v = left.ee[r][c] + right.ss[r][c];
#pragma unroll
                        for (int j = 0; j < N; ++j) v = fma_<R>(-left.se[j][r], W[j][c], v);
                        A[r][c] = v;
                        Bm[r][c] = right.se[r][c];
                    }
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        // Qt annihilates constants (ep0 = -ep1, sp0 = -sp1): the two legs, not four nearly opposite
                        // products of the waypoints themselves, which lose |P| / |leg| digits
                        R v = left.ep1[r] * (Pc[ax] - Pp[ax]);
                        v = fma_<R>(right.sp1[r], Pn[ax] - Pc[ax], v);
                        if constexpr (JBAR) {
#pragma unroll
                            for (int j = 0; j < N; ++j) v = fma_<R>(left.se[j][r], z[j][ax], v);
                            Bm[r][N + ax] = -v;
                            if (PBAR) {
                                R u = dend[r][ax] + dstart[r][ax];
#pragma unroll
                                for (int j = 0; j < N; ++j) u = fma_<R>(-left.se[j][r], z[j][NC - 3 + ax], u);
                                Bm[r][N + NC - 3 + ax] = u;
                            }
                        } else {   // both columns in one loop, the p_bar-only kernel's statement order
                            R u = dend[r][ax] + dstart[r][ax];
#pragma unroll
                            for (int j = 0; j < N; ++j) {
                                v = fma_<R>(left.se[j][r], z[j][ax], v);
                                u = fma_<R>(-left.se[j][r], z[j][3 + ax], u);
                            }
                            Bm[r][N + ax] = -v;
                            Bm[r][N + 3 + ax] = u;
                        }
                    }
                }
                const R piv = spd_solve<N, N + NC, R>(A, Bm);
                if (!(piv > R(0))) status |= CSP_TRAJ_NOT_SPD_BIT;
                R *wk = ws + (int64_t)(k - 1) * E * a.B;
#pragma unroll
                for (int r = 0; r < N; ++r) {
#pragma unroll
                    for (int c = 0; c < N; ++c) { W[r][c] = Bm[r][c]; wk[(int64_t)(r * N + c) * a.B] = W[r][c]; }
#pragma unroll
                    for (int c = 0; c < NC; ++c) { z[r][c] = Bm[r][N + c]; wk[(int64_t)(N * N + r * NC + c) * a.B] = z[r][c]; }
                    if (PBAR) {
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) dend[r][ax] = dnext[r][ax];
                    }
                }
                left = right;
                Tn = Tnn;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    Pp[ax] = Pc[ax]; Pc[ax] = Pn[ax]; Pn[ax] = Pnn[ax];
                    if (PBAR) {
#pragma unroll
                        for (int i = 0; i < M; ++i) pbn[ax][i] = pbnn[ax][i];
                    }
                }
            }
        }

        // ---- back substitution: x (and lambda) per waypoint, then per segment T_bar and the fixed-slot gradients ----
        R xn[N][3], ln[N][3];
        load_bc(1, xn);
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) ln[r][ax] = R(0);
        R nanacc = R(0);
        R carry[3] = {R(0), R(0), R(0)};   // start-of-segment part of waypoint k+1's gradient (segment k+1)
        R Tk = R(tm[S - 1]), P0[3], P1[3], wz[E], pb[3][M];
        // positions enter as P1 - P0 only
        vload3<IO, R>(wp + 3 * (S - 1), P0);
        vload3<IO, R>(wp + 3 * S, P1);
        if (PBAR) load_rec<O, IO, R>(gco + (int64_t)(S - 1) * 3 * M, pb);
        if (S > 1) {
            const R *wk = ws + (int64_t)(S - 2) * E * a.B;
#pragma unroll
            for (int e = 0; e < E; ++e) wz[e] = wk[(int64_t)e * a.B];
        }
        for (int k = S - 1; k >= 0; --k) {
            R Tp = R(1), Pm[3] = {R(0), R(0), R(0)}, wzp[E], pbp[3][M];
            if (k >= 1) {  // prefetch segment k-1: time, start waypoint, (p_bar) and factors
                Tp = R(tm[k - 1]);
                vload3<IO, R>(wp + 3 * (k - 1), Pm);
                if (PBAR) load_rec<O, IO, R>(gco + (int64_t)(k - 1) * 3 * M, pbp);
                if (k >= 2) {
                    const R *wk = ws + (int64_t)(k - 2) * E * a.B;
#pragma unroll
                    for (int e = 0; e < E; ++e) wzp[e] = wk[(int64_t)e * a.B];
                }
            }
            R xk[N][3], lk[N][3];
            if constexpr (!HOLD_BC) {
                if (k == 0) load_bc(0, xk);
            }
#pragma unroll
            for (int r = 0; r < N; ++r)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    if constexpr (!JBAR) {   // the p_bar-only kernel's statements, x and lambda in one loop
                        if (k == 0) {
                            if constexpr (HOLD_BC) xk[r][ax] = held[0][r][ax];
                            lk[r][ax] = R(0);
                            continue;
                        }
                        R v = wz[N * N + r * 6 + ax], u = wz[N * N + r * 6 + 3 + ax];
#pragma unroll
                        for (int c = 0; c < N; ++c) {
                            v = fma_<R>(-wz[r * N + c], xn[c][ax], v);
                            u = fma_<R>(-wz[r * N + c], ln[c][ax], u);
                        }
                        xk[r][ax] = v;
                        lk[r][ax] = u;
                        continue;
                    }
                    lk[r][ax] = R(0);
                    if (k == 0) continue;
                    R v = wz[N * N + r * NC + ax];
#pragma unroll
                    for (int c = 0; c < N; ++c) v = fma_<R>(-wz[r * N + c], xn[c][ax], v);
                    xk[r][ax] = v;
                    if (PBAR) {
                        R u = wz[N * N + r * NC + NC - 3 + ax];
#pragma unroll
                        for (int c = 0; c < N; ++c) u = fma_<R>(-wz[r * N + c], ln[c][ax], u);
                        lk[r][ax] = u;
                    }
                }
            R tp[O], ip[M];
            powers<O, R>(Tk, tp, ip);
            const R ipw = ip[M - 1];   // T^(1-2o)
            R tsum = R(0), s0 = R(0), s1 = R(0), gs[3], ge[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                R gv0, gv1, ga0 = R(0), ga1 = R(0);   // start / end velocity slot, acceleration slots (order >= 3)
                if constexpr (JBAR) {
                    // J part: u = QT dh with dh_a = T^deriv_a d_a, the segment's start as origin (Qt annihilates
                    // constants): (Qt d)_a = T^(1-2o) T^deriv_a u_a,  d^T Qt d = T^(1-2o) dh.u
                    R dh[M], u[M];
                    dh[0] = R(0);
                    dh[O] = P1[ax] - P0[ax];
#pragma unroll
                    for (int r = 0; r < N; ++r) { dh[r + 1] = xk[r][ax] * tp[r + 1]; dh[O + r + 1] = xn[r][ax] * tp[r + 1]; }
#pragma unroll
                    for (int aa = 0; aa < M; ++aa) {
                        R v = R(0);
#pragma unroll
                        for (int bb = 0; bb < M; ++bb) {
                            constexpr double zero = 0.0;
                            if (Tab<O>::QT(aa, bb) != zero) v = fma_<R>(Tab<O>::QT(aa, bb), dh[bb], v);
                        }
                        u[aa] = v;
                        s0 = fma_<R>(dh[aa], v, s0);
                        if (aa % O) s1 = fma_<R>(R(aa % O) * dh[aa], v, s1);
                    }
                    const R js = jb2 * ipw;
                    gs[ax] = js * u[0];
                    ge[ax] = js * u[O];
                    gv0 = jb2 * fma_<R>(ipw * tp[1], u[1], vw * xk[0][ax]);
                    gv1 = jb2 * fma_<R>(ipw * tp[1], u[O + 1], vw * xn[0][ax]);
                    if (N >= 2) { ga0 = js * tp[A2] * u[A2]; ga1 = js * tp[A2] * u[O + A2]; }
                }
                if (PBAR) {
                    R d[M], c[M], db[M], lt[M];
                    // the segment's start as origin: positions carry weight zero in every term below but the Qt
                    // products, which annihilate constants, and only the constant coefficient of c depends on it
                    d[0] = R(0);
                    d[O] = P1[ax] - P0[ax];
                    lt[0] = R(0);
                    lt[O] = R(0);
#pragma unroll
                    for (int r = 0; r < N; ++r) {
                        d[r + 1] = xk[r][ax]; d[O + r + 1] = xn[r][ax];
                        lt[r + 1] = lk[r][ax]; lt[O + r + 1] = ln[r][ax];
                    }
                    recover_axis<O, R>(d, tp, ip, c);
                    dbar_axis<O, 0, M, R>(pb[ax], tp, ip, db);
                    // (Qt lambda~) at the fixed slots: both positions, and the bc slots of the first / last segment.
                    // lambda~ is zero at every fixed slot, so the +w diagonal never enters.
                    R q[M];
#pragma unroll
                    for (int aa = 0; aa < M; ++aa) {
                        R v = R(0);
#pragma unroll
                        for (int bb = 0; bb < M; ++bb) {
                            if (bb % O == 0) continue;
                            v = fma_<R>(R(Tab<O>::QT(aa, bb)) * ip[M - 1 - aa % O - bb % O], lt[bb], v);
                        }
                        q[aa] = v;
                    }
                    R t = R(0);
#pragma unroll
                    for (int aa = 0; aa < M; ++aa) {
                        t = fma_<R>(R(aa % O) * d[aa], db[aa], t);
                        t = fma_<R>(-R(M - 1 - aa) * c[aa], pb[ax][aa], t);
                    }
                    // sum_ab (1-2o+deriv_a+deriv_b) lambda~_a Qt_ab d_b over the free slots a
#pragma unroll
                    for (int aa = 0; aa < M; ++aa) {
                        if (aa % O == 0) continue;
                        R v = R(0);
#pragma unroll
                        for (int bb = 0; bb < M; ++bb)
                            v = fma_<R>(R(1 - 2 * O + aa % O + bb % O) * R(Tab<O>::QT(aa, bb)) * ip[M - 1 - aa % O - bb % O], d[bb], v);
                        t = fma_<R>(-lt[aa], v, t);
                    }
                    tsum += t;
                    if constexpr (JBAR) {   // joins the J part
                        gs[ax] += db[0] - q[0];
                        ge[ax] += db[O] - q[O];
                        gv0 += db[1] - q[1];
                        gv1 += db[O + 1] - q[O + 1];
                        if (N >= 2) { ga0 += db[A2] - q[A2]; ga1 += db[O + A2] - q[O + A2]; }
                    } else {                // is the gradient: assigned, not added to a zero (which would lose a -0)
                        gs[ax] = db[0] - q[0];
                        ge[ax] = db[O] - q[O];
                        gv0 = db[1] - q[1];
                        gv1 = db[O + 1] - q[O + 1];
                        if (N >= 2) { ga0 = db[A2] - q[A2]; ga1 = db[O + A2] - q[O + A2]; }
                    }
                }
                if (k == 0) { gbc[0][ax] = gv0; gbc[2][ax] = ga0; }
                if (k == S - 1) {
                    if constexpr (JBAR) { end_bc[ax][threadIdx.x] = gv1; end_bc[3 + ax][threadIdx.x] = ga1; }
                    else { gbc[1][ax] = gv1; gbc[3][ax] = ga1; }
                }
            }
            if (gtm) {
                R g;
                if constexpr (JBAR) {
                    // J_bar dJ/dT_j = -J_bar T^(-2o) [ (2o-1) dh.u - 2 sum_a deriv_a dh_a u_a ]
                    g = jb * (-(ipw * ip[1]) * fma_<R>(R(M - 1), s0, R(-2) * s1));
                    if (PBAR) g = fma_<R>(tsum, ip[1], g);
                } else {
                    g = tsum * ip[1];
                }
                gtm[k] = IO(g);
                nanacc = fma_<R>(R(IO(g)), R(0), nanacc);
            }
            if (gwp) {
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const IO g = IO(carry[ax] + ge[ax]);
                    gwp[3 * (k + 1) + ax] = g;
                    nanacc = fma_<R>(R(g), R(0), nanacc);
                }
            }
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) carry[ax] = gs[ax];
#pragma unroll
            for (int r = 0; r < N; ++r)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) { xn[r][ax] = xk[r][ax]; ln[r][ax] = lk[r][ax]; }
            Tk = Tp;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                P1[ax] = P0[ax]; P0[ax] = Pm[ax];
                if (PBAR) {
#pragma unroll
                    for (int i = 0; i < M; ++i) pb[ax][i] = pbp[ax][i];
                }
            }
#pragma unroll
            for (int e = 0; e < E; ++e) wz[e] = wzp[e];
        }
        if (gwp) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const IO g = IO(carry[ax]);
                gwp[ax] = g;
                nanacc = fma_<R>(R(g), R(0), nanacc);
            }
        }
        if (a.grad_bc) {
            if constexpr (JBAR) {
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) { gbc[1][ax] = end_bc[ax][threadIdx.x]; gbc[3][ax] = end_bc[3 + ax][threadIdx.x]; }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) nanacc = fma_<R>(gbc[r][ax], R(0), nanacc);
            if (a.bc_per_traj) {
                IO *gb = (IO *)a.grad_bc + b * 12;
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) gb[r * 3 + ax] = IO(gbc[r][ax]);
            }
        }
        if (!(nanacc == R(0))) status |= CSP_TRAJ_NONFINITE_BIT;
    }
    if (b < a.B && a.status) a.status[b] = status;
    // shared bc: this workgroup's sum in a fixed order (the whole wave takes part, idle lanes add zeros)
    if (a.grad_bc && !a.bc_per_traj) {
        R *part = (R *)a.bc_part;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const double s = wave_sum((double)gbc[r][ax]);
                if (threadIdx.x == 0) part[(int64_t)(r * 3 + ax) * gridDim.x + blockIdx.x] = R(s);
            }
    }
}

// Second pass of the shared-bc reduction: one wave sums the per-workgroup partials of each of the 12 entries in a
// fixed order (strided per lane, then an in-wave tree).
template <typename IO, typename R>
__global__ void __launch_bounds__(64) minsnap_vjp_bc_reduce(const R *part, int64_t nblk, IO *grad_bc) {
    for (int e = 0; e < 12; ++e) {
        double s = 0.0;
        for (int64_t i = threadIdx.x; i < nblk; i += 64) s += (double)part[(int64_t)e * nblk + i];
        s = wave_sum(s);
        if (threadIdx.x == 0) grad_bc[e] = IO(s);
    }
}

// the instantiation follows from which cotangents are given (the C-ABI refuses a call with neither)
template <int O, typename IO> static hipError_t launch_vjp_o(const CostVjpArgs &a, hipStream_t st) {
    const int64_t blocks = vjp_blocks(a.B);
    const dim3 grid((unsigned)blocks), wave(64);
    if (!a.grad_cost) hipLaunchKernelGGL((minsnap_vjp_kernel<O, IO, true, false>), grid, wave, 0, st, a);
    else if (a.grad_coeffs) hipLaunchKernelGGL((minsnap_vjp_kernel<O, IO, true, true>), grid, wave, 0, st, a);
    else hipLaunchKernelGGL((minsnap_vjp_kernel<O, IO, false, true>), grid, wave, 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.grad_bc || a.bc_per_traj) return e;
    hipLaunchKernelGGL((minsnap_vjp_bc_reduce<IO, double>), dim3(1), wave, 0, st, (const double *)a.bc_part, blocks,
                       (IO *)a.grad_bc);
    return hipGetLastError();
}

template <typename IO> static hipError_t launch_vjp_r(const CostVjpArgs &a, hipStream_t st) {
    switch (a.order) {
        case 2: return launch_vjp_o<2, IO>(a, st);
        case 3: return launch_vjp_o<3, IO>(a, st);
        case 4: return launch_vjp_o<4, IO>(a, st);
        case 5: return launch_vjp_o<5, IO>(a, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_vjp(const CostVjpArgs &a, bool f32, hipStream_t st) {
    if (a.B == 0) return hipSuccess;
    return f32 ? launch_vjp_r<float>(a, st) : launch_vjp_r<double>(a, st);
}

hipError_t launch_vjp(const VjpArgs &v, bool f32, hipStream_t st) {
    CostVjpArgs a;
    static_cast<VjpArgs &>(a) = v;
    a.grad_cost = nullptr;
    return launch_vjp(a, f32, st);
}

}  // namespace csp
