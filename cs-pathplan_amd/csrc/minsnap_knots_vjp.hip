// minsnap_knots_vjp.hip -- reverse mode of the open-chain solve with per-knot derivative constraints: the vector-Jacobian
// product of (coeffs, J) = csp_minsnap_solve_knots_batch, orders 2..5, uniform or ragged, fp64 storage or fp32 storage
// with fp64 arithmetic, zero-velocity penalty.  One kernel, a compile-time flag per cotangent.  DESIGN.md §22.
//
// The unknowns are all knot derivatives x_k (k = 0..S); a mask bit pins one to a value.  Given p_bar = dL/dcoeffs and
// J_bar = dL/dJ, per axis
//   d_bar_j = M(T_j)^-T p_bar_j, scattered to the knots (end part of segment k-1 + start part of segment k)
//   R_ff lambda_f = d_bar_f, lambda_F = 0        the forward's masked block-tridiagonal matrix (minsnap_knots.hip) with
//                                                three more right-hand-side columns: d_bar at a free slot, 0 at a pinned
//                                                one, none of the primal's pin-coupling terms
//   u = Qt^w_j lambda~_j,  e = 2 J_bar Qt^w_j d_j   per segment (lambda~: lambda at the segment's slots, 0 at positions
//                                                and pins; the e part is the envelope theorem, no adjoint solve)
//   a position slot adds d_bar - u + e to the waypoint's gradient, a pinned derivative slot to its value's gradient;
//   a free slot's value gradient is 0.0 by a select on the mask bit
//   T_bar_j = (1/T_j) [ sum_a deriv_a d_a d_bar_a - sum_a (T^deriv_a d_a) (G^T diag(pow T^-pow) p_bar)_a
//                       - sum_ab (1-2o+deriv_a+deriv_b) lambda~_a Qt_ab d_b ] + J_bar dJ/dT_j
// The second term of T_bar is sum_i pow_i p_i p_bar_i with the coefficient recovery folded into the cotangent, so the
// cancelling recovery (double-double in the forward) is not needed here.  lambda~ is zero at every pinned slot, so the +w
// diagonal enters through the J_bar part only.
//
// Layout as minsnap_knots.hip / minsnap_vjp.hip: one lane per trajectory, workgroups of one wave, W_k and z_k in a
// [knot][entry][trajectory] workspace, both sweeps software-pipelined one knot ahead, the primal re-solved in the same
// sweep.  Masks are data: every use is a select on a mask bit with static indexing.  Every output has one owner: a
// knot's gradient is the end part of segment k-1 plus the start part carried from segment k, written once.  No atomics.
#include "minsnap_device.h"
#include "minsnap_launch.h"
#include "minsnap_knots_vjp.h"
#include "minsnap_mixed.h"   // CSP_TRAJ_SKIPPED_BIT
#include "minsnap_vjp_device.h"

namespace csp {

using namespace vjpk;   // vload3, load_rec, powers

namespace {

// mask and pinned values of one knot; a free derivative's entry is replaced by 0 with a select, never by arithmetic
template <int N, typename IO>
__device__ __forceinline__ void load_pins(const uint8_t *mk, const IO *kv, unsigned &m, double (&pv)[N][3]) {
    m = (unsigned)mk[0] & ((1u << N) - 1u);
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double v = double(kv[r * 3 + ax]);
            pv[r][ax] = ((m >> r) & 1u) ? v : 0.0;
        }
}

// d_bar[a] = T^deriv_a sum_i G[i][a] T^-pow_i p_bar[i] and gp[a] = sum_i G[i][a] pow_i T^-pow_i p_bar[i], all slots
template <int O, typename R>
__device__ __forceinline__ void dbar_pow_axis(const R (&pb)[2 * O], const R (&tp)[O], const R (&ip)[2 * O], R (&db)[2 * O],
                                              R (&gp)[2 * O]) {
    constexpr int M = 2 * O;
    R ph[M], pw[M];
#pragma unroll
    for (int i = 0; i < M; ++i) { ph[i] = pb[i] * ip[M - 1 - i]; pw[i] = R(M - 1 - i) * ph[i]; }
#pragma unroll
    for (int a = 0; a < M; ++a) {
        R acc = R(0), acp = R(0);
#pragma unroll
        for (int i = 0; i < M; ++i) {
            constexpr double zero = 0.0;
            if (Tab<O>::G(i, a) != zero) {
                acc = fma_<R>(R(Tab<O>::G(i, a)), ph[i], acc);
                if (i != M - 1) acp = fma_<R>(R(Tab<O>::G(i, a)), pw[i], acp);
            }
        }
        db[a] = acc * tp[a % O];
        gp[a] = acp;
    }
}

}  // namespace

template <int O, typename IO, bool PBAR, bool JBAR>
__global__ void __launch_bounds__(64) minsnap_knots_vjp_kernel(KnotsVjpArgs a) {
    static_assert(PBAR || JBAR, "a cotangent of the coefficients, of the cost, or both");
    typedef double R;
    constexpr int N = O - 1;
    constexpr int M = 2 * O;
    constexpr int NC = PBAR ? 6 : 3;        // right-hand-side columns: 3 primal (+ 3 adjoint)
    constexpr int E = N * N + NC * N;       // W, z per knot
    constexpr unsigned FULL = (1u << N) - 1u;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    int64_t seg0;
    int S;
    if (a.seg_off) { seg0 = a.seg_off[b]; S = (int)(a.seg_off[b + 1] - seg0); }
    else { seg0 = b * (int64_t)a.S; S = a.S; }
    IO *gwp = a.grad_wp ? (IO *)a.grad_wp + (seg0 + b) * 3 : nullptr;            // [S+1][3]
    IO *gtm = a.grad_times ? (IO *)a.grad_times + seg0 : nullptr;               // [S]
    IO *gkv = a.grad_values ? (IO *)a.grad_values + (seg0 + b) * (3 * N) : nullptr;   // [S+1][N][3]
    // every gradient row of `knots` knots and `segs` segments gets v (the lanes that are not solved)
    auto fill = [&](IO v, int knots, int segs) {
        for (int k = 0; k < knots; ++k) {
            if (gwp) { gwp[3 * k] = v; gwp[3 * k + 1] = v; gwp[3 * k + 2] = v; }
            if (gkv)
                for (int e = 0; e < 3 * N; ++e) gkv[(int64_t)k * (3 * N) + e] = v;
        }
        if (gtm)
            for (int k = 0; k < segs; ++k) gtm[k] = v;
    };
    if (S < 1) {   // an empty ragged trajectory: its one knot gets zero gradients
        fill(IO(0), 1, 0);
        if (a.status) a.status[b] = 0;
        return;
    }
    if (S > a.Smax) {   // a ragged length the workspace was not sized for (device memory: the host could not check it)
        fill(IO(__builtin_nan("")), S + 1, S);
        if (a.status) a.status[b] = CSP_TRAJ_SKIPPED_BIT;
        return;
    }
    const IO *wp = (const IO *)a.wp + (seg0 + b) * 3;            // [S+1][3]
    const IO *tm = (const IO *)a.times + seg0;
    const uint8_t *mk = a.mask + (seg0 + b);                     // [S+1]
    const IO *kv = (const IO *)a.values + (seg0 + b) * (3 * N);  // [S+1][N][3]
    const IO *gco = PBAR ? (const IO *)a.grad_coeffs + seg0 * 3 * M : nullptr;
    const int64_t B = a.B;
    R *ws = (R *)a.ws + b;
    const R vw = a.vw_per ? a.vw_per[b] : a.vel_zero_weight;
    R jb = R(0);
    if constexpr (JBAR) jb = a.grad_cost[b];
    const R jb2 = R(2) * jb;

    // the forward's count rule, decided before the sweep (minsnap_knots.hip)
    if (S + 1 < O) {
        int count = S + 1;
        for (int k = 0; k <= S; ++k) count += __builtin_popcount((unsigned)mk[k] & FULL);
        if (count < O) {
            fill(IO(__builtin_nan("")), S + 1, S);
            if (a.status) a.status[b] = CSP_TRAJ_NOT_SPD_BIT;
            return;
        }
    }

    int status = 0;

    // ---- forward sweep over knots 0..S: the forward's masked block-LDL^T with 3 primal (and, PBAR, 3 adjoint) columns
    R z[N][NC];   // after the sweep: z_S = (x_S, lambda_S)
    {
        R W[N][N];
        SegBlocks<O, R> left, right;
#pragma unroll
        for (int r = 0; r < N; ++r) {
#pragma unroll
            for (int c = 0; c < N; ++c) { W[r][c] = R(0); left.ee[r][c] = R(0); left.se[r][c] = R(0); }
#pragma unroll
            for (int c = 0; c < NC; ++c) z[r][c] = R(0);
            left.ep1[r] = R(0);
        }
        R Pp[3], Pc[3], Pn[3], Pnn[3] = {R(0), R(0), R(0)};
        vload3<IO, R>(wp, Pc);
        vload3<IO, R>(wp + 3, Pn);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) Pp[ax] = Pc[ax];
        R Tn = R(tm[0]), Tnn = R(1);
        unsigned mp = 0, mc, mn, mnn = 0;
        R pvp[N][3], pvc[N][3], pvn[N][3], pvnn[N][3];
        R dend[N][3];   // the end part of segment k-1's d_bar: the left contribution of knot k
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { pvp[r][ax] = R(0); pvnn[r][ax] = R(0); dend[r][ax] = R(0); }
        load_pins<N, IO>(mk, kv, mc, pvc);
        load_pins<N, IO>(mk + 1, kv + 3 * N, mn, pvn);
        R pbn[3][M], pbnn[3][M];
        if (PBAR) {
            load_rec<O, IO, R>(gco, pbn);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                for (int i = 0; i < M; ++i) pbnn[ax][i] = R(0);
        }
        for (int k = 0; k <= S; ++k) {
            if (k + 2 <= S) {   // prefetch knot k+2 (waypoint, mask, values), time k+1 (and p_bar of segment k+1)
                vload3<IO, R>(wp + 3 * (k + 2), Pnn);
                load_pins<N, IO>(mk + (k + 2), kv + (int64_t)(k + 2) * (3 * N), mnn, pvnn);
                Tnn = R(tm[k + 1]);
                if (PBAR) load_rec<O, IO, R>(gco + (int64_t)(k + 1) * 3 * M, pbnn);
            } else {            // past the last knot: no segment, nothing pinned
                Tnn = R(1);
                mnn = 0;
#pragma unroll
                for (int r = 0; r < N; ++r)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) pvnn[r][ax] = R(0);
            }
            seg_blocks<O, R, false>(Tn, vw, R(0), 0, Pc, Pn, right);   // segment k: knot k -> knot k+1
            if (!(Tn > R(0))) status |= CSP_TRAJ_NOT_SPD_BIT;          // as the forward: flagged from the time itself
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
            if (k == S) {   // the last knot has no segment to its right (Tn = 1 there)
#pragma unroll
                for (int r = 0; r < N; ++r) {
#pragma unroll
                    for (int c = 0; c < N; ++c) { right.ss[r][c] = R(0); right.se[r][c] = R(0); }
                    right.sp1[r] = R(0);
                    if (PBAR) {
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) dstart[r][ax] = R(0);
                    }
                }
            }
            R A[N][N], Bm[N][N + NC], Lse[N][N];
#pragma unroll
            for (int j = 0; j < N; ++j)
#pragma unroll
                for (int r = 0; r < N; ++r)   // C_{k-1} without row j of a pinned j (knot k-1), column r of a pinned r
                    Lse[j][r] = (((mp >> j) | (mc >> r)) & 1u) ? R(0) : left.se[j][r];
#pragma unroll
            for (int r = 0; r < N; ++r) {
                const bool pr = (mc >> r) & 1u;
#pragma unroll
                for (int c = 0; c < N; ++c) {
                    const bool pc = (mc >> c) & 1u;
                    R v = left.ee[r][c] + right.ss[r][c];
#pragma unroll
                    for (int j = 0; j < N; ++j) v = fma_<R>(-Lse[j][r], W[j][c], v);
                    A[r][c] = (pr || pc) ? (r == c ? R(1) : R(0)) : v;
                    Bm[r][c] = (pr || ((mn >> c) & 1u)) ? R(0) : right.se[r][c];
                }
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    // Qt annihilates constants (ep0 = -ep1, sp0 = -sp1): the two legs, not four nearly opposite products
                    R v = left.ep1[r] * (Pc[ax] - Pp[ax]);
                    v = fma_<R>(right.sp1[r], Pn[ax] - Pc[ax], v);
                    // the pinned unknowns of knots k-1, k, k+1 (pv is 0 for a free one)
#pragma unroll
                    for (int c = 0; c < N; ++c) {
                        v = fma_<R>(left.se[c][r], pvp[c][ax], v);
                        v = fma_<R>(left.ee[r][c] + right.ss[r][c], pvc[c][ax], v);
                        v = fma_<R>(right.se[r][c], pvn[c][ax], v);
                    }
#pragma unroll
                    for (int j = 0; j < N; ++j) v = fma_<R>(Lse[j][r], z[j][ax], v);
                    Bm[r][N + ax] = pr ? pvc[r][ax] : -v;
                    if (PBAR) {   // the adjoint column: d_bar at a free slot, 0 at a pinned one, no pin coupling
                        R u = dend[r][ax] + dstart[r][ax];
#pragma unroll
                        for (int j = 0; j < N; ++j) u = fma_<R>(-Lse[j][r], z[j][NC - 3 + ax], u);
                        Bm[r][N + NC - 3 + ax] = pr ? R(0) : u;
                    }
                }
            }
            const R piv = spd_solve<N, N + NC, R>(A, Bm);
            if (!(piv > R(0))) status |= CSP_TRAJ_NOT_SPD_BIT;
#pragma unroll
            for (int r = 0; r < N; ++r) {
#pragma unroll
                for (int c = 0; c < N; ++c) W[r][c] = Bm[r][c];
#pragma unroll
                for (int c = 0; c < NC; ++c) z[r][c] = Bm[r][N + c];
            }
            if (k < S) {   // knot S's factors stay in registers: W_S = 0, z_S = (x_S, lambda_S)
                R *wk = ws + (int64_t)k * E * B;
#pragma unroll
                for (int r = 0; r < N; ++r) {
#pragma unroll
                    for (int c = 0; c < N; ++c) wk[(int64_t)(r * N + c) * B] = W[r][c];
#pragma unroll
                    for (int c = 0; c < NC; ++c) wk[(int64_t)(N * N + r * NC + c) * B] = z[r][c];
                }
            }
            left = right;
            Tn = Tnn;
            mp = mc; mc = mn; mn = mnn;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                Pp[ax] = Pc[ax]; Pc[ax] = Pn[ax]; Pn[ax] = Pnn[ax];
                if (PBAR) {
#pragma unroll
                    for (int i = 0; i < M; ++i) pbn[ax][i] = pbnn[ax][i];
                }
            }
#pragma unroll
            for (int r = 0; r < N; ++r)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    pvp[r][ax] = pvc[r][ax]; pvc[r][ax] = pvn[r][ax]; pvn[r][ax] = pvnn[r][ax];
                    if (PBAR) dend[r][ax] = dnext[r][ax];
                }
        }
    }

    // ---- back substitution over segments S-1..0: x (and lambda) per knot, then per segment T_bar and the slot gradients
    R xn[N][3], ln[N][3];   // the end knot of segment k
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { xn[r][ax] = z[r][ax]; ln[r][ax] = PBAR ? z[r][NC - 3 + ax] : R(0); }
    R nanacc = R(0);
    R carryP[3] = {R(0), R(0), R(0)}, carryD[N][3];   // start-of-segment part of knot k+1's gradients (segment k+1)
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) carryD[r][ax] = R(0);
    R Tk = R(tm[S - 1]), P0[3], P1[3], wz[E], pb[3][M];
    unsigned mkn = (unsigned)mk[S] & FULL, mkc = (unsigned)mk[S - 1] & FULL;   // masks of knot k+1 and knot k
    vload3<IO, R>(wp + 3 * (S - 1), P0);
    vload3<IO, R>(wp + 3 * S, P1);
    if (PBAR) load_rec<O, IO, R>(gco + (int64_t)(S - 1) * 3 * M, pb);
    {
        const R *wk = ws + (int64_t)(S - 1) * E * B;
#pragma unroll
        for (int e = 0; e < E; ++e) wz[e] = wk[(int64_t)e * B];
    }
    for (int k = S - 1; k >= 0; --k) {
        R Tp = R(1), Pm[3] = {R(0), R(0), R(0)}, wzp[E], pbp[3][M];
        unsigned mkp = 0;
        if (k >= 1) {   // prefetch segment k-1: its time, start waypoint, mask, (p_bar) and the factors of knot k-1
            Tp = R(tm[k - 1]);
            vload3<IO, R>(wp + 3 * (k - 1), Pm);
            mkp = (unsigned)mk[k - 1] & FULL;
            if (PBAR) load_rec<O, IO, R>(gco + (int64_t)(k - 1) * 3 * M, pbp);
            const R *wk = ws + (int64_t)(k - 1) * E * B;
#pragma unroll
            for (int e = 0; e < E; ++e) wzp[e] = wk[(int64_t)e * B];
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) wzp[e] = R(0);
            if (PBAR) {
#pragma unroll
                for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                    for (int i = 0; i < M; ++i) pbp[ax][i] = R(0);
            }
        }
        R xk[N][3], lk[N][3];
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                R v = wz[N * N + r * NC + ax];
#pragma unroll
                for (int c = 0; c < N; ++c) v = fma_<R>(-wz[r * N + c], xn[c][ax], v);
                xk[r][ax] = v;
                lk[r][ax] = R(0);
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
        R tsum = R(0), s0 = R(0), s1 = R(0);
        R gsP[3], geP[3], gsD[N][3], geD[N][3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            // dh_a = T^deriv_a d_a with the segment's start as origin: positions carry weight zero in every term but the
            // Qt products, which annihilate constants
            R d[M], dh[M], g[M];
            d[0] = R(0);
            d[O] = P1[ax] - P0[ax];
#pragma unroll
            for (int r = 0; r < N; ++r) { d[r + 1] = xk[r][ax]; d[O + r + 1] = xn[r][ax]; }
#pragma unroll
            for (int aa = 0; aa < M; ++aa) dh[aa] = d[aa] * tp[aa % O];
            if constexpr (JBAR) {
                // e = 2 J_bar Qt^w d: u = QT dh, (Qt d)_a = T^(1-2o) T^deriv_a u_a, d^T Qt d = T^(1-2o) dh.u
                R u[M];
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
#pragma unroll
                for (int aa = 0; aa < M; ++aa) g[aa] = js * tp[aa % O] * u[aa];
                g[1] = jb2 * fma_<R>(ipw * tp[1], u[1], vw * xk[0][ax]);
                g[O + 1] = jb2 * fma_<R>(ipw * tp[1], u[O + 1], vw * xn[0][ax]);
            }
            if (PBAR) {
                R db[M], gp[M], lt[M];
                lt[0] = R(0);
                lt[O] = R(0);
#pragma unroll
                for (int r = 0; r < N; ++r) { lt[r + 1] = lk[r][ax]; lt[O + r + 1] = ln[r][ax]; }
                dbar_pow_axis<O, R>(pb[ax], tp, ip, db, gp);
                // u = Qt lambda~ (lambda~ is zero at positions and pins, so the +w diagonal never enters)
                R t = R(0);
#pragma unroll
                for (int aa = 0; aa < M; ++aa) {
                    R v = R(0);
#pragma unroll
                    for (int bb = 0; bb < M; ++bb) {
                        if (bb % O == 0) continue;
                        v = fma_<R>(R(Tab<O>::QT(aa, bb)) * ip[M - 1 - aa % O - bb % O], lt[bb], v);
                    }
                    if constexpr (JBAR) g[aa] += db[aa] - v;
                    else g[aa] = db[aa] - v;
                    t = fma_<R>(R(aa % O) * d[aa], db[aa], t);
                    t = fma_<R>(-dh[aa], gp[aa], t);
                }
                // sum_ab (1-2o+deriv_a+deriv_b) lambda~_a Qt_ab d_b over the derivative slots a
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
            }
            gsP[ax] = g[0];
            geP[ax] = g[O];
#pragma unroll
            for (int r = 0; r < N; ++r) { gsD[r][ax] = g[r + 1]; geD[r][ax] = g[O + r + 1]; }
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
                const IO g = IO(carryP[ax] + geP[ax]);
                gwp[3 * (k + 1) + ax] = g;
                nanacc = fma_<R>(R(g), R(0), nanacc);
            }
        }
        if (gkv) {   // knot k+1: a pinned slot's gradient, 0.0 at a free slot
            IO *dst = gkv + (int64_t)(k + 1) * (3 * N);
#pragma unroll
            for (int r = 0; r < N; ++r)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const IO g = ((mkn >> r) & 1u) ? IO(carryD[r][ax] + geD[r][ax]) : IO(0);
                    dst[r * 3 + ax] = g;
                    nanacc = fma_<R>(R(g), R(0), nanacc);
                }
        }
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) carryP[ax] = gsP[ax];
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                carryD[r][ax] = gsD[r][ax];
                xn[r][ax] = xk[r][ax];
                ln[r][ax] = lk[r][ax];
            }
        Tk = Tp;
        mkn = mkc; mkc = mkp;
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
    // knot 0: the start part of segment 0 alone
    if (gwp) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const IO g = IO(carryP[ax]);
            gwp[ax] = g;
            nanacc = fma_<R>(R(g), R(0), nanacc);
        }
    }
    if (gkv) {
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const IO g = ((mkn >> r) & 1u) ? IO(carryD[r][ax]) : IO(0);
                gkv[r * 3 + ax] = g;
                nanacc = fma_<R>(R(g), R(0), nanacc);
            }
    }
    if (!(nanacc == R(0))) status |= CSP_TRAJ_NONFINITE_BIT;
    if (a.status) a.status[b] = status;
}

// the instantiation follows from which cotangents are given (the C-ABI refuses a call with neither)
template <int O, typename IO> static hipError_t launch_o(const KnotsVjpArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)((a.B + 63) / 64)), wave(64);
    if (!a.grad_cost) hipLaunchKernelGGL((minsnap_knots_vjp_kernel<O, IO, true, false>), grid, wave, 0, st, a);
    else if (a.grad_coeffs) hipLaunchKernelGGL((minsnap_knots_vjp_kernel<O, IO, true, true>), grid, wave, 0, st, a);
    else hipLaunchKernelGGL((minsnap_knots_vjp_kernel<O, IO, false, true>), grid, wave, 0, st, a);
    return hipGetLastError();
}

template <typename IO> static hipError_t launch_io(const KnotsVjpArgs &a, hipStream_t st) {
    switch (a.order) {
        case 2: return launch_o<2, IO>(a, st);
        case 3: return launch_o<3, IO>(a, st);
        case 4: return launch_o<4, IO>(a, st);
        case 5: return launch_o<5, IO>(a, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_knots_vjp(const KnotsVjpArgs &a, bool f32, hipStream_t st) {
    if (a.B == 0) return hipSuccess;
    return f32 ? launch_io<float>(a, st) : launch_io<double>(a, st);
}

}  // namespace csp
