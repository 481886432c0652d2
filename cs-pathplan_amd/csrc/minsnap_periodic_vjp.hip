// minsnap_periodic_vjp.hip -- reverse mode of the periodic (closed-loop) solve: the vector-Jacobian product of
// csp_minsnap_solve_periodic_batch (orders 2..5, uniform or ragged, fp64 storage or fp32 storage with fp64 arithmetic,
// zero-velocity penalty).  DESIGN.md §15.
//
// Given p_bar = dL/dcoeffs and (JBAR) J_bar = dL/dcost, per axis:
//   d_bar_j = M(T_j)^-T p_bar_j                          (endpoint-derivative space, no inverse at run time)
//   R_PP lambda = d_bar_free                             (the forward's block-cyclic matrix, shared by the three axes)
//   dL/dP_k = d_bar_pos(k) - sum_j (Qt_j mu_j)_pos(k),   mu_j = lambda~_j - 2 J_bar d_j   (lambda~ zero at positions)
//   T_bar_j = (1/T_j) [ sum_a deriv_a d_a d_bar_a - sum_i pow_i p_i p_bar_i
//                       + sum_ab (1-2o+deriv_a+deriv_b) (J_bar d_a - lambda~_a) Qt_ab d_b ]
// The J_bar terms are the envelope-theorem gradient of J = d^T K d ((K d)_free = 0 at the optimum).
//
// The sweep is minsnap_periodic.hip's bordered block-LDL^T (knot 0 the border) with three adjoint right-hand sides
// next to the three primal ones: one spd_solve per knot of 2N+6 columns (W, V, z, z_lambda), the border's Schur
// complement and its two right-hand sides in registers.  The primal is re-solved from waypoints and times instead of
// being rebuilt from the forward's coefficients (minsnap_vjp.hip).  p_bar is read twice: forwards for
// the free slots of d_bar (segment k's start part feeds knot k, its end part knot k+1; segment S-1's end part wraps to
// knot 0) and in the back substitution for T_bar and the position slots.  Positions are measured from the loop's first
// waypoint in the sweep and from the segment's start in the back substitution: every quantity here is invariant under
// a translation (the rows of Qt sum to zero over the two position slots).
// One lane per trajectory, no cross-lane operation, no atomics, every sum in a fixed order: two calls give identical
// bits, and a lane's arithmetic never depends on its neighbours.  Every loop runs over the segments only.
//
// load_rec / dbar_axis / powers repeat the helpers of the same names in minsnap_vjp_device.h.
#include "minsnap_device.h"
#include "minsnap_periodic_vjp.h"

namespace csp {

namespace {

template <typename IO>
__device__ __forceinline__ void pload3(const IO *p, const double (&org)[3], double (&v)[3]) {
    v[0] = double(p[0]) - org[0]; v[1] = double(p[1]) - org[1]; v[2] = double(p[2]) - org[2];
}

template <typename IO>
__device__ __forceinline__ void rload3(const IO *p, double (&v)[3]) {
    v[0] = double(p[0]); v[1] = double(p[1]); v[2] = double(p[2]);
}

// One segment's p_bar record [3][2O] as 16-byte (f64) or 8-byte (f32) vector loads: record bases are multiples of
// 2O*sizeof(IO) bytes from a 16-byte (f64) / 8-byte (f32) aligned array (checked by the C-ABI).
template <int O, typename IO>
__device__ __forceinline__ void load_rec(const IO *src, double (&q)[3][2 * O]) {
    typedef IO vec2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
#pragma unroll
        for (int i = 0; i < 2 * O; i += 2) {
            const vec2 v = *reinterpret_cast<const vec2 *>(src + ax * 2 * O + i);
            q[ax][i] = double(v.x);
            q[ax][i + 1] = double(v.y);
        }
}

// d_bar[a] = T^deriv_a sum_i G[i][a] T^-pow_i p_bar[i]  (= M(T)^-T p_bar), for the slots a in [A0, A1)
template <int O, int A0, int A1>
__device__ __forceinline__ void dbar_axis(const double (&pb)[2 * O], const double (&tp)[O], const double (&ip)[2 * O],
                                          double (&db)[2 * O]) {
    constexpr int M = 2 * O;
    double ph[M];
#pragma unroll
    for (int i = 0; i < M; ++i) ph[i] = pb[i] * ip[M - 1 - i];
#pragma unroll
    for (int a = A0; a < A1; ++a) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < M; ++i) {
            constexpr double zero = 0.0;
            if (Tab<O>::G(i, a) != zero) acc = fma_<double>(Tab<O>::G(i, a), ph[i], acc);
        }
        db[a] = acc * tp[a % O];
    }
}

template <int O> __device__ __forceinline__ void powers(double T, double (&tp)[O], double (&ip)[2 * O]) {
    tp[0] = 1.0;
#pragma unroll
    for (int e = 1; e < O; ++e) tp[e] = tp[e - 1] * T;
    ip[0] = 1.0;
    ip[1] = fast_rcp(T);
#pragma unroll
    for (int e = 2; e < 2 * O; ++e) ip[e] = ip[e - 1] * ip[1];
}

// The free slots of one segment's d_bar, all three axes: start part (slots 1..o-1) and end part (o+1..2o-1)
template <int O>
__device__ __forceinline__ void dbar_free(const double (&pb)[3][2 * O], double T, double (&ds)[O - 1][3], double (&de)[O - 1][3]) {
    constexpr int N = O - 1;
    constexpr int M = 2 * O;
    double tp[O], ip[M];
    powers<O>(T, tp, ip);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        double db[M];
        dbar_axis<O, 1, O>(pb[ax], tp, ip, db);
        dbar_axis<O, O + 1, M>(pb[ax], tp, ip, db);
#pragma unroll
        for (int r = 0; r < N; ++r) { ds[r][ax] = db[1 + r]; de[r][ax] = db[O + 1 + r]; }
    }
}

}  // namespace

template <int O, typename IO, bool JBAR>
__global__ void __launch_bounds__(64) minsnap_periodic_vjp_kernel(PeriodicVjpArgs a) {
    constexpr int N = O - 1;
    constexpr int M = 2 * O;
    constexpr int E = 2 * N * N + 6 * N;   // W, V, z (3 primal + 3 adjoint columns) per knot
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    int64_t seg0;
    int S;
    if (a.seg_off) { seg0 = a.seg_off[b]; S = (int)(a.seg_off[b + 1] - seg0); }
    else { seg0 = b * (int64_t)a.S; S = a.S; }
    if (S < 1) {   // an empty loop owns no waypoint and no time
        if (a.status) a.status[b] = 0;
        return;
    }
    const IO *wp = (const IO *)a.wp + seg0 * 3;   // [S][3], no closing point
    const IO *tm = (const IO *)a.times + seg0;
    const IO *gco = (const IO *)a.grad_coeffs + seg0 * 3 * M;
    IO *gwp = a.grad_wp ? (IO *)a.grad_wp + seg0 * 3 : (IO *)nullptr;
    IO *gtm = a.grad_times ? (IO *)a.grad_times + seg0 : (IO *)nullptr;
    const int64_t B = a.B;
    double *ws = (double *)a.ws + b;
    const double vw = a.vw_per ? a.vw_per[b] : a.vel_zero_weight;
    const double jb = JBAR ? a.grad_cost[b] : 0.0;
    const double org[3] = {double(wp[0]), double(wp[1]), double(wp[2])};
    int status = 0;

    // ---- forward sweep over knots 1..S-1; Sig / r0 accumulate the border's Schur complement and its right-hand sides
    // (columns 0..2 primal, 3..5 adjoint)
    double Sig[N][N], r0[N][6];
    {
        double P0[3], P1[3];
        pload3<IO>(wp, org, P0);
        pload3<IO>(wp + 3 * (S > 1 ? 1 : 0), org, P1);
        const double T0 = double(tm[0]);
        SegBlocks<O, double> left;
        seg_blocks<O, double, false>(T0, vw, 0.0, 0, P0, P1, left);
        // segment 0's d_bar: its start part is knot 0's, its end part goes to knot 1 (S = 1: to knot 0 again)
        double dend[N][3];
        {
            double pb[3][M], ds[N][3];
            load_rec<O, IO>(gco, pb);
            dbar_free<O>(pb, T0, ds, dend);
#pragma unroll
            for (int r = 0; r < N; ++r)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) r0[r][3 + ax] = ds[r][ax];
        }
        // knot 0's own terms from segment 0 (its start)
#pragma unroll
        for (int r = 0; r < N; ++r) {
#pragma unroll
            for (int c = 0; c < N; ++c) Sig[r][c] = left.ss[r][c];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) r0[r][ax] = -fma_<double>(left.sp0[r], P0[ax], left.sp1[r] * P1[ax]);
        }
        if (S == 1) {
            // one knot: segment 0 also ends there and couples the knot to itself
#pragma unroll
            for (int r = 0; r < N; ++r) {
#pragma unroll
                for (int c = 0; c < N; ++c) Sig[r][c] += left.ee[r][c] + (left.se[r][c] + left.se[c][r]);
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) r0[r][3 + ax] += dend[r][ax];
            }
        } else {
            double W[N][N], V[N][N], z[N][6];
            double Pp[3], Pc[3], Pn[3], Pnn[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { Pp[ax] = P0[ax]; Pc[ax] = P1[ax]; }
            pload3<IO>(wp + 3 * (2 % S), org, Pn);
            double Tn = double(tm[1]), Tnn = 1.0;
            SegBlocks<O, double> right;
            for (int k = 1; k < S; ++k) {
                if (k + 1 < S) {   // prefetch waypoint k+2 (mod S) and time k+1
                    const int kn = k + 2 >= S ? k + 2 - S : k + 2;
                    pload3<IO>(wp + 3 * kn, org, Pnn);
                    Tnn = double(tm[k + 1]);
                }
                double pb[3][M];   // segment k's p_bar: asked for here, used after the blocks are built
                load_rec<O, IO>(gco + (int64_t)k * 3 * M, pb);
                seg_blocks<O, double, false>(Tn, vw, 0.0, 0, Pc, Pn, right);   // segment k: knot k -> knot k+1 (mod S)
                const bool last = k == S - 1;
                double A[N][N], G[N][N], Bm[N][2 * N + 6];
#pragma unroll
                for (int r = 0; r < N; ++r) {
#pragma unroll
                    for (int c = 0; c < N; ++c) {
                        double v = left.ee[r][c] + right.ss[r][c];
                        double g = k == 1 ? left.se[c][r] : 0.0;
                        if (k > 1) {
#pragma unroll
                            for (int j = 0; j < N; ++j) {
                                v = fma_<double>(-left.se[j][r], W[j][c], v);
                                g = fma_<double>(-left.se[j][r], V[j][c], g);
                            }
                        }
                        if (last) g += right.se[r][c];   // the corner C_{S-1} (S = 2: C_0^T + C_1)
                        A[r][c] = v;
                        G[r][c] = g;
                        Bm[r][c] = last ? 0.0 : right.se[r][c];
                        Bm[r][N + c] = g;
                    }
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        double v = left.ep0[r] * Pp[ax];
                        v = fma_<double>(left.ep1[r], Pc[ax], v);
                        v = fma_<double>(right.sp0[r], Pc[ax], v);
                        v = fma_<double>(right.sp1[r], Pn[ax], v);
                        if (k > 1) {
#pragma unroll
                            for (int j = 0; j < N; ++j) v = fma_<double>(left.se[j][r], z[j][ax], v);
                        }
                        Bm[r][2 * N + ax] = -v;
                    }
                }
                double dstart[N][3], dnext[N][3];
                dbar_free<O>(pb, Tn, dstart, dnext);
#pragma unroll
                for (int r = 0; r < N; ++r)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        double u = dend[r][ax] + dstart[r][ax];
                        if (k > 1) {
#pragma unroll
                            for (int j = 0; j < N; ++j) u = fma_<double>(-left.se[j][r], z[j][3 + ax], u);
                        }
                        Bm[r][2 * N + 3 + ax] = u;
                    }
                const double piv = spd_solve<N, 2 * N + 6, double>(A, Bm);
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
                    for (int c = 0; c < 6; ++c) {
                        z[r][c] = Bm[r][2 * N + c];
                        wk[(int64_t)(2 * N * N + r * 6 + c) * B] = z[r][c];
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
                    for (int c = 0; c < 6; ++c) {
                        double v = r0[r][c];
#pragma unroll
                        for (int j = 0; j < N; ++j) v = fma_<double>(-G[j][r], z[j][c], v);
                        r0[r][c] = v;
                    }
                }
                left = right;
                Tn = Tnn;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) { Pp[ax] = Pc[ax]; Pc[ax] = Pn[ax]; Pn[ax] = Pnn[ax]; }
#pragma unroll
                for (int r = 0; r < N; ++r)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) dend[r][ax] = dnext[r][ax];
            }
            // knot 0's terms from segment S-1 (its end): left is segment S-1, Pp = P_{S-1}, Pc = P_0, dend its end part
#pragma unroll
            for (int r = 0; r < N; ++r) {
#pragma unroll
                for (int c = 0; c < N; ++c) Sig[r][c] += left.ee[r][c];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    r0[r][ax] -= fma_<double>(left.ep0[r], Pp[ax], left.ep1[r] * Pc[ax]);
                    r0[r][3 + ax] += dend[r][ax];
                }
            }
        }
    }
    const double piv0 = spd_solve<N, 6, double>(Sig, r0);   // r0 becomes knot 0's x (0..2) and lambda (3..5)
    if (!(piv0 > 0.0)) status |= CSP_TRAJ_NOT_SPD_BIT;

    // ---- back substitution: x and lambda per knot, then per segment T_bar and its two position-slot parts
    double xn[N][6];   // the end knot of segment k: knot 0 for k = S-1
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) xn[r][c] = r0[r][c];
    double nanacc = 0.0;
    double carry[3] = {0.0, 0.0, 0.0};   // the start part of knot k+1's gradient (segment k+1)
    double g0e[3] = {0.0, 0.0, 0.0};     // the end part of knot 0's gradient (segment S-1), kept until knot 0 closes
    double Tk = double(tm[S - 1]), P0[3], P1[3], wz[E];
    rload3<IO>(wp + 3 * (S - 1), P0);
    rload3<IO>(wp, P1);
    if (S > 1) {
        const double *wk = ws + (int64_t)(S - 2) * E * B;
#pragma unroll
        for (int e = 0; e < E; ++e) wz[e] = e < N * N ? 0.0 : wk[(int64_t)e * B];
    }
    for (int k = S - 1; k >= 0; --k) {
        double Tp = 1.0, Pm[3] = {0.0, 0.0, 0.0}, wzp[E];
        if (k >= 1) {   // prefetch segment k-1: its time, start waypoint and the factors of knot k-1
            Tp = double(tm[k - 1]);
            rload3<IO>(wp + 3 * (k - 1), Pm);
            if (k >= 2) {
                const double *wk = ws + (int64_t)(k - 2) * E * B;
#pragma unroll
                for (int e = 0; e < E; ++e) wzp[e] = wk[(int64_t)e * B];
            }
        }
        double pb[3][M];
        load_rec<O, IO>(gco + (int64_t)k * 3 * M, pb);
        double xk[N][6];
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int c6 = 0; c6 < 6; ++c6) {
                if (k == 0) { xk[r][c6] = r0[r][c6]; continue; }
                double v = wz[2 * N * N + r * 6 + c6];
#pragma unroll
                for (int c = 0; c < N; ++c) {
                    v = fma_<double>(-wz[r * N + c], xn[c][c6], v);
                    v = fma_<double>(-wz[N * N + r * N + c], r0[c][c6], v);
                }
                xk[r][c6] = v;
            }
        double tp[O], ip[M];
        powers<O>(Tk, tp, ip);
        double tsum = 0.0, gs[3], ge[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            // endpoint derivatives with the segment's start as origin, lambda~ (zero at the position slots) and
            // mu = lambda~ - 2 J_bar d
            double d[M], c[M], db[M], lt[M], mu[M];
            d[0] = 0.0;
            d[O] = P1[ax] - P0[ax];
            lt[0] = 0.0;
            lt[O] = 0.0;
#pragma unroll
            for (int r = 0; r < N; ++r) {
                d[r + 1] = xk[r][ax]; d[O + r + 1] = xn[r][ax];
                lt[r + 1] = xk[r][3 + ax]; lt[O + r + 1] = xn[r][3 + ax];
            }
#pragma unroll
            for (int aa = 0; aa < M; ++aa) mu[aa] = JBAR ? fma_<double>(-2.0 * jb, d[aa], lt[aa]) : lt[aa];
            recover_axis<O, double>(d, tp, ip, c);
            dbar_axis<O, 0, M>(pb[ax], tp, ip, db);
            // (Qt mu) at the two position slots; the +w diagonal sits on velocity slots and never enters
            double q[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int aa = h * O;
                double v = 0.0;
#pragma unroll
                for (int bb = 1; bb < M; ++bb) {
                    if (!JBAR && bb == O) continue;   // mu[0] = 0 always, mu[O] = 0 without J_bar
                    v = fma_<double>(Tab<O>::QT(aa, bb) * ip[M - 1 - bb % O], mu[bb], v);
                }
                q[h] = v;
            }
            double t = 0.0;
#pragma unroll
            for (int aa = 0; aa < M; ++aa) {
                t = fma_<double>(double(aa % O) * d[aa], db[aa], t);
                t = fma_<double>(-double(M - 1 - aa) * c[aa], pb[ax][aa], t);
            }
            // sum_ab (1-2o+deriv_a+deriv_b) (J_bar d_a - lambda~_a) Qt_ab d_b; d[0] = 0, and without J_bar only the
            // free slots a carry a factor
#pragma unroll
            for (int aa = 1; aa < M; ++aa) {
                if (!JBAR && aa == O) continue;
                double v = 0.0;
#pragma unroll
                for (int bb = 1; bb < M; ++bb)
                    v = fma_<double>(double(1 - 2 * O + aa % O + bb % O) * Tab<O>::QT(aa, bb) * ip[M - 1 - aa % O - bb % O], d[bb], v);
                t = fma_<double>(JBAR ? fma_<double>(jb, d[aa], -lt[aa]) : -lt[aa], v, t);
            }
            tsum += t;
            gs[ax] = db[0] - q[0];
            ge[ax] = db[O] - q[1];
        }
        if (gtm) {
            const double g = tsum * ip[1];
            gtm[k] = IO(g);
            nanacc = fma_<double>(double(IO(g)), 0.0, nanacc);
        }
        // knot k+1 = segment k+1's start part + segment k's end part, written once; segment S-1 ends at knot 0
        if (k == S - 1) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) g0e[ax] = ge[ax];
        } else if (gwp) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const IO g = IO(carry[ax] + ge[ax]);
                gwp[3 * (k + 1) + ax] = g;
                nanacc = fma_<double>(double(g), 0.0, nanacc);
            }
        }
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) carry[ax] = gs[ax];
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int c6 = 0; c6 < 6; ++c6) xn[r][c6] = xk[r][c6];
        Tk = Tp;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { P1[ax] = P0[ax]; P0[ax] = Pm[ax]; }
#pragma unroll
        for (int e = 0; e < E; ++e) wz[e] = wzp[e];
    }
    if (gwp) {   // knot 0 closes last: segment 0's start part + segment S-1's end part
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const IO g = IO(carry[ax] + g0e[ax]);
            gwp[ax] = g;
            nanacc = fma_<double>(double(g), 0.0, nanacc);
        }
    }
    if (!(nanacc == 0.0)) status |= CSP_TRAJ_NONFINITE_BIT;
    if (a.status) a.status[b] = status;
}

template <int O, typename IO> static hipError_t launch_o(const PeriodicVjpArgs &a, hipStream_t st) {
    const unsigned blocks = (unsigned)((a.B + 63) / 64);
    if (a.grad_cost) hipLaunchKernelGGL((minsnap_periodic_vjp_kernel<O, IO, true>), dim3(blocks), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((minsnap_periodic_vjp_kernel<O, IO, false>), dim3(blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

template <typename IO> static hipError_t launch_io(const PeriodicVjpArgs &a, hipStream_t st) {
    switch (a.order) {
        case 2: return launch_o<2, IO>(a, st);
        case 3: return launch_o<3, IO>(a, st);
        case 4: return launch_o<4, IO>(a, st);
        case 5: return launch_o<5, IO>(a, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_periodic_vjp(const PeriodicVjpArgs &a, bool f32, hipStream_t st) {
    if (a.B == 0) return hipSuccess;
    return f32 ? launch_io<float>(a, st) : launch_io<double>(a, st);
}

}  // namespace csp
