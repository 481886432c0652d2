// minsnap_knots.hip -- the open-chain minimum-snap solve with per-knot derivative constraints (orders 2..5, uniform or
// ragged, fp64 storage or fp32 storage with fp64 arithmetic, zero-velocity penalty).  DESIGN.md §20.
//
// Knot k = 0..S (the waypoints) owns the N = o-1 derivatives x_k, shared by the end of segment k-1 and the start of
// segment k.  Over ALL of them the Hessian is block-tridiagonal:
//   D_k = Qt_{k-1}[ee] + Qt_k[ss]  (k = 0: [ss] alone, k = S: [ee] alone),   C_k = Qt_k[se] couples knot k to knot k+1,
//   y_k = -(Qt_{k-1}[e,pos] + Qt_k[s,pos]) P   (waypoints measured from the trajectory's first one).
// A mask bit pins an unknown i of knot k to a value v: every other row of knots k-1, k, k+1 loses (its coupling to
// i) * v from its right-hand side, row and column i of D_k become the identity row with right-hand side v, column i
// of C_{k-1} and row i of C_k become zero.  What is left is a principal submatrix of the SPD Hessian bordered by
// identity rows: the block-LDL^T sweep of minsnap_generic.hip runs over it unchanged and without pivoting,
//   S_k = D_k - C_{k-1}^T W_{k-1},  W_k = S_k^-1 C_k,  z_k = S_k^-1 (y_k - C_{k-1}^T z_{k-1}),   x_k = z_k - W_k x_{k+1},
// with W_{-1} = 0 and C_S = 0, so the end knots are ordinary knots.  The masks are data: every use is a select on a mask
// bit with static indexing, the arrays stay in registers.  The three axes share a knot's mask and so one factorisation.
//
// Layout as minsnap_generic.hip: one lane per trajectory, workgroups of one wave, W_k and z_k in a
// [knot][entry][trajectory] workspace, both sweeps software-pipelined one knot ahead (a knot's mask and values travel
// with its waypoint).  The back substitution recovers the coefficients with the segment's start as origin, in
// double-double arithmetic (see there: the polynomial must reproduce its own end derivatives), and, when the cost is
// asked for, sums the per-segment quadratic form of minsnap_timeopt.hip's cost_pass; the coefficients are
// computed by the same instructions either way.
#include "minsnap_device.h"
#include "minsnap_launch.h"
#include "minsnap_knots.h"
#include "minsnap_mixed.h"   // CSP_TRAJ_SKIPPED_BIT

namespace csp {

namespace {

template <typename IO>
__device__ __forceinline__ void kload3(const IO *p, const double (&org)[3], double (&v)[3]) {
    v[0] = double(p[0]) - org[0]; v[1] = double(p[1]) - org[1]; v[2] = double(p[2]) - org[2];
}

// mask and pinned values of one knot; a free derivative's entry is replaced by 0 with a select, never by arithmetic,
// so that whatever the caller left there (NaN, inf) goes nowhere
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

template <int M, typename IO> __device__ __forceinline__ void store_row(IO *dst, const IO (&q)[M]) {
    typedef IO vec2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int i = 0; i < M; i += 2) {
        vec2 v;
        v.x = q[i];
        v.y = q[i + 1];
        *reinterpret_cast<vec2 *>(dst + i) = v;
    }
}

// Double-double pieces of the coefficient recovery (error-free transformations; this file is compiled without
// floating-point contraction, so a product that feeds a sum stays a rounded product).
struct dd { double h, l; };
__device__ __forceinline__ dd two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd two_prod(double a, double b) {
    const double p = a * b;
    return {p, __builtin_fma(a, b, -p)};
}
__device__ __forceinline__ dd dd_mul(dd x, double b) {
    const dd p = two_prod(x.h, b);
    const double l = __builtin_fma(x.l, b, p.l), s = p.h + l;
    return {s, l - (s - p.h)};
}
// G * (o-1)! is a table of integers (every entry of M(1)^-1 is an integer over the factorial of its derivative;
// tests/test_knots_math.py): exact in a double where 1/6 is not
template <int O> __device__ __forceinline__ constexpr double g_int(int i, int a) {
    constexpr double f = O == 2 ? 1.0 : O == 3 ? 2.0 : O == 4 ? 6.0 : 24.0;
    const double v = Tab<O>::G(i, a) * f;
    return double((long long)(v < 0.0 ? v - 0.5 : v + 0.5));
}

}  // namespace

template <int O, typename IO>
__global__ void __launch_bounds__(64) minsnap_knots_kernel(KnotsArgs a) {
    constexpr int N = O - 1;
    constexpr int M = 2 * O;
    constexpr int E = N * N + 3 * N;   // W, z per knot
    constexpr unsigned FULL = (1u << N) - 1u;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    int64_t seg0;
    int S;
    if (a.seg_off) { seg0 = a.seg_off[b]; S = (int)(a.seg_off[b + 1] - seg0); }
    else { seg0 = b * (int64_t)a.S; S = a.S; }
    if (S < 1) {
        if (a.cost) a.cost[b] = 0.0;
        if (a.status) a.status[b] = 0;
        return;
    }
    if (S > a.Smax) {   // a ragged length the workspace was not sized for (device memory: the host could not check it)
        if (a.cost) a.cost[b] = __builtin_nan("");
        if (a.status) a.status[b] = CSP_TRAJ_SKIPPED_BIT;
        return;
    }
    const IO *wp = (const IO *)a.wp + (seg0 + b) * 3;            // [S+1][3]
    const IO *tm = (const IO *)a.times + seg0;
    const uint8_t *mk = a.mask + (seg0 + b);                     // [S+1]
    const IO *kv = (const IO *)a.values + (seg0 + b) * (3 * N);  // [S+1][N][3]
    IO *co = (IO *)a.coeffs + seg0 * 3 * M;
    const int64_t B = a.B;
    double *ws = (double *)a.ws + b;
    const double vw = a.vw_per ? a.vw_per[b] : a.vel_zero_weight;

    // the count rule: with fewer constraints than the order a non-zero polynomial of degree < order costs nothing and
    // the minimiser is not unique.  Decided here, not by a pivot; S + 1 >= order needs no look at the masks.
    if (S + 1 < O) {
        int count = S + 1;
        for (int k = 0; k <= S; ++k) count += __builtin_popcount((unsigned)mk[k] & FULL);
        if (count < O) {
            IO q[M];
#pragma unroll
            for (int i = 0; i < M; ++i) q[i] = IO(__builtin_nan(""));
            for (int k = 0; k < S; ++k)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) store_row<M, IO>(co + ((int64_t)k * 3 + ax) * M, q);
            if (a.cost) a.cost[b] = __builtin_nan("");
            if (a.status) a.status[b] = CSP_TRAJ_NOT_SPD_BIT;
            return;
        }
    }

    const double org[3] = {double(wp[0]), double(wp[1]), double(wp[2])};
    int status = 0;

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
            left.ep0[r] = 0.0;
            left.ep1[r] = 0.0;
        }
        double Pp[3] = {0.0, 0.0, 0.0}, Pc[3] = {0.0, 0.0, 0.0}, Pn[3], Pnn[3] = {0.0, 0.0, 0.0};
        kload3<IO>(wp + 3, org, Pn);
        double Tn = double(tm[0]), Tnn = 1.0;
        unsigned mp = 0, mc, mn, mnn = 0;
        double pvp[N][3], pvc[N][3], pvn[N][3], pvnn[N][3];
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { pvp[r][ax] = 0.0; pvnn[r][ax] = 0.0; }
        load_pins<N, IO>(mk, kv, mc, pvc);
        load_pins<N, IO>(mk + 1, kv + 3 * N, mn, pvn);
        for (int k = 0; k <= S; ++k) {
            if (k + 2 <= S) {   // prefetch knot k+2 (waypoint, mask, values) and time k+1
                kload3<IO>(wp + 3 * (k + 2), org, Pnn);
                load_pins<N, IO>(mk + (k + 2), kv + (int64_t)(k + 2) * (3 * N), mnn, pvnn);
                Tnn = double(tm[k + 1]);
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
                    right.sp0[r] = 0.0;
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
                    double v = left.ep0[r] * Pp[ax];
                    v = fma_<double>(left.ep1[r], Pc[ax], v);
                    v = fma_<double>(right.sp0[r], Pc[ax], v);
                    v = fma_<double>(right.sp1[r], Pn[ax], v);
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
            double *wk = ws + (int64_t)k * E * B;
#pragma unroll
            for (int r = 0; r < N; ++r) {
#pragma unroll
                for (int c = 0; c < N; ++c) W[r][c] = Bm[r][c];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) z[r][ax] = Bm[r][N + ax];
            }
            if (k < S) {   // knot S's factors stay in registers: W_S = 0, z_S = x_S
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

    // ---- back substitution over segments S-1..0 fused with coefficient recovery (and the cost)
    const bool want_cost = a.cost != nullptr;
    double xn[N][3];   // the end knot of segment k
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) xn[r][ax] = z[r][ax];
    double nanacc = 0.0, Jacc = 0.0;
    double Tk = double(tm[S - 1]), P0[3], P1[3], wz[E];
    P0[0] = double(wp[3 * (S - 1)]); P0[1] = double(wp[3 * (S - 1) + 1]); P0[2] = double(wp[3 * (S - 1) + 2]);
    P1[0] = double(wp[3 * S]); P1[1] = double(wp[3 * S + 1]); P1[2] = double(wp[3 * S + 2]);
    {
        const double *wk = ws + (int64_t)(S - 1) * E * B;
#pragma unroll
        for (int e = 0; e < E; ++e) wz[e] = wk[(int64_t)e * B];
    }
    for (int k = S - 1; k >= 0; --k) {
        double Tp = 1.0, Pm[3] = {0.0, 0.0, 0.0}, wzp[E];
        if (k >= 1) {   // prefetch segment k-1: its time, start waypoint and the factors of knot k-1
            Tp = double(tm[k - 1]);
            Pm[0] = double(wp[3 * (k - 1)]); Pm[1] = double(wp[3 * (k - 1) + 1]); Pm[2] = double(wp[3 * (k - 1) + 2]);
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
        // The recovery c = diag(T^-p) G diag(T^a) d cancels: on a smooth trajectory |G| |d| is tens of times |G d|, and
        // in plain fp64 the polynomial then misses its own end derivatives -- a pinned value at the last knot -- by that
        // factor times the rounding unit.  So the powers of T and the scaled derivatives are kept as double-double
        // pairs, the sums run over the integer table G (o-1)! with error-free products and sums, and one division
        // with a correction step rounds each coefficient once: every stored coefficient is within about an ulp of the
        // exact coefficient of the Hermite interpolant of (x_k, x_{k+1}, T).
        constexpr double FACT = O == 2 ? 1.0 : O == 3 ? 2.0 : O == 4 ? 6.0 : 24.0;
        dd tpd[M];
        tpd[0] = {1.0, 0.0};
#pragma unroll
        for (int e = 1; e < M; ++e) tpd[e] = dd_mul(tpd[e - 1], Tk);
        dd den[M];      // the denominators (o-1)! T^e
        double ip[M];   // and their reciprocals, for the division
        const double it = fast_rcp(Tk);
#pragma unroll
        for (int e = 0; e < M; ++e) { den[e] = dd_mul(tpd[e], FACT); ip[e] = fast_rcp(den[e].h); }
        double s0 = 0.0, vel = 0.0;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            // endpoint derivatives scaled by T^deriv, the segment's start as origin
            dd dhd[M];
            double dh[M];
            dhd[0] = {0.0, 0.0};
            dhd[O] = two_sum(P1[ax], -P0[ax]);
#pragma unroll
            for (int r = 0; r < N; ++r) { dhd[r + 1] = dd_mul(tpd[r + 1], xk[r][ax]); dhd[O + r + 1] = dd_mul(tpd[r + 1], xn[r][ax]); }
#pragma unroll
            for (int aa = 0; aa < M; ++aa) dh[aa] = dhd[aa].h;
            IO q[M];
#pragma unroll
            for (int i = 0; i < M - 1; ++i) {
                double sh = 0.0, sl = 0.0;
#pragma unroll
                for (int aa = 1; aa < M; ++aa) {
                    const double gi = g_int<O>(i, aa);
                    if (gi != 0.0) {
                        const dd p = two_prod(gi, dhd[aa].h);
                        const dd t = two_sum(sh, p.h);
                        sh = t.h;
                        sl += t.l + p.l;
                        sl = __builtin_fma(gi, dhd[aa].l, sl);
                    }
                }
                // (sh + sl) / ((o-1)! T^p): a quotient from the reciprocal, then its residual against the denominator
                const int e = M - 1 - i;
                const double q0 = (sh + sl) * ip[e];
                const dd pq = two_prod(q0, den[e].h);
                const double res = ((sh - pq.h) - pq.l) + sl - q0 * den[e].l;
                const double c = q0 + res * ip[e];
                q[i] = IO(c);
                nanacc = fma_<double>(double(q[i]), 0.0, nanacc);
            }
            q[M - 1] = IO(P0[ax]);   // p(0) = P_k, copied through
            nanacc = fma_<double>(double(q[M - 1]), 0.0, nanacc);
            store_row<M, IO>(co + ((int64_t)k * 3 + ax) * M, q);
            if (want_cost) {
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
                }
            }
        }
        if (want_cost) {
            double ipw = it;   // T^(1-2o)
#pragma unroll
            for (int e = 2; e < M; ++e) ipw *= it;
            Jacc += fma_<double>(vw, vel, ipw * s0);
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
    if (want_cost) {
        nanacc = fma_<double>(Jacc, 0.0, nanacc);
        a.cost[b] = Jacc;
    }
    if (!(nanacc == 0.0)) status |= CSP_TRAJ_NONFINITE_BIT;
    if (a.status) a.status[b] = status;
}

template <int O, typename IO> static hipError_t launch_o(const KnotsArgs &a, hipStream_t st) {
    const unsigned blocks = (unsigned)((a.B + 63) / 64);
    hipLaunchKernelGGL((minsnap_knots_kernel<O, IO>), dim3(blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

template <typename IO> static hipError_t launch_io(const KnotsArgs &a, hipStream_t st) {
    switch (a.order) {
        case 2: return launch_o<2, IO>(a, st);
        case 3: return launch_o<3, IO>(a, st);
        case 4: return launch_o<4, IO>(a, st);
        case 5: return launch_o<5, IO>(a, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_knots(const KnotsArgs &a, bool f32, hipStream_t st) {
    if (a.B == 0) return hipSuccess;
    return f32 ? launch_io<float>(a, st) : launch_io<double>(a, st);
}

}  // namespace csp
