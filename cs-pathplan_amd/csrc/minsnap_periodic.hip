// minsnap_periodic.hip -- the periodic (closed-loop) minimum-snap solve: S segments around a loop, every knot interior,
// the wrap P_{S-1} -> P_0 included, no boundary conditions (orders 2..5, uniform or ragged, fp64 storage or fp32
// storage with fp64 arithmetic, zero-velocity penalty).  DESIGN.md §13.
//
// Knot k owns the N = o-1 free derivatives x_k, shared by the end of segment k-1 (mod S) and the start of segment k.
// The free-derivative Hessian is block-CYCLIC-tridiagonal:
//   D_k = Qt_{k-1}[ee] + Qt_k[ss],   C_k = Qt_k[se] couples knot k to knot k+1 (mod S; C_{S-1} is the corner).
// Bordered block-LDL^T with knot 0 as the border: knots 1..S-1 are swept as in minsnap_generic.hip
//   S_k = D_k - C_{k-1}^T W_{k-1},  W_k = S_k^-1 C_k,  z_k = S_k^-1 (y_k - C_{k-1}^T z_{k-1}),
// carrying the border column G_k (G_1 = C_0^T, G_k = -C_{k-1}^T V_{k-1}, plus the corner C_{S-1} at the last knot),
// V_k = S_k^-1 G_k.  The border's Schur complement  Sigma = D_0 - sum_k G_k^T V_k  and right-hand side
// y_0 - sum_k G_k^T z_k  give x_0; back substitution  x_k = z_k - W_k x_{k+1} - V_k x_0  (W_{S-1} = 0).
// S = 1 is the single knot with the block ss + ee + se + se^T and a zero right-hand side: x_0 = 0 exactly.
//
// Layout as minsnap_generic.hip: one lane per trajectory, workgroups of one wave, the factors W_k, V_k, z_k in a
// [knot][entry][trajectory] workspace, both sweeps software-pipelined one knot ahead.  With COST the back substitution
// also sums the snap cost J and writes dJ/dT (the per-segment formula of minsnap_timeopt.hip's cost_pass); the
// coefficients are computed by the same instructions either way.
#include "minsnap_device.h"
#include "minsnap_launch.h"

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

}  // namespace

template <int O, typename IO, bool COST>
__global__ void __launch_bounds__(64) minsnap_periodic_kernel(PeriodicArgs a) {
    constexpr int N = O - 1;
    constexpr int M = 2 * O;
    constexpr int E = 2 * N * N + 3 * N;   // W, V, z per knot
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    int64_t seg0;
    int S;
    if (a.seg_off) { seg0 = a.seg_off[b]; S = (int)(a.seg_off[b + 1] - seg0); }
    else { seg0 = b * (int64_t)a.S; S = a.S; }
    if (S < 1) {
        if (COST && a.cost) a.cost[b] = 0.0;
        if (a.status) a.status[b] = 0;
        return;
    }
    const IO *wp = (const IO *)a.wp + seg0 * 3;   // [S][3], no closing point
    const IO *tm = (const IO *)a.times + seg0;
    IO *co = (IO *)a.coeffs + seg0 * 3 * M;
    const int64_t B = a.B;
    double *ws = (double *)a.ws + b;
    const double vw = a.vw_per ? a.vw_per[b] : a.vel_zero_weight;
    const double org[3] = {double(wp[0]), double(wp[1]), double(wp[2])};
    int status = 0;

    // ---- forward sweep over knots 1..S-1; Sig / r0 accumulate the border's Schur complement and right-hand side
    double Sig[N][N], r0[N][3];
    {
        double P0[3], P1[3];
        pload3<IO>(wp, org, P0);
        pload3<IO>(wp + 3 * (S > 1 ? 1 : 0), org, P1);
        SegBlocks<O, double> left;
        seg_blocks<O, double, false>(double(tm[0]), vw, 0.0, 0, P0, P1, left);
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
            for (int r = 0; r < N; ++r)
#pragma unroll
                for (int c = 0; c < N; ++c) Sig[r][c] += left.ee[r][c] + (left.se[r][c] + left.se[c][r]);
        } else {
            double W[N][N], V[N][N], z[N][3];
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
                seg_blocks<O, double, false>(Tn, vw, 0.0, 0, Pc, Pn, right);   // segment k: knot k -> knot k+1 (mod S)
                const bool last = k == S - 1;
                double A[N][N], G[N][N], Bm[N][2 * N + 3];
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
            // knot 0's terms from segment S-1 (its end): left is segment S-1, Pp = P_{S-1}, Pc = P_0
#pragma unroll
            for (int r = 0; r < N; ++r) {
#pragma unroll
                for (int c = 0; c < N; ++c) Sig[r][c] += left.ee[r][c];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) r0[r][ax] -= fma_<double>(left.ep0[r], Pp[ax], left.ep1[r] * Pc[ax]);
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

    // ---- back substitution fused with coefficient recovery (and with COST, the cost and the time gradient)
    double xn[N][3];   // the end knot of segment k: knot 0 for k = S-1
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) xn[r][ax] = x0[r][ax];
    double nanacc = 0.0, Jacc = 0.0;
    double Tk = double(tm[S - 1]), P0[3], P1[3], wz[E];
    rload3<IO>(wp + 3 * (S - 1), P0);
    rload3<IO>(wp, P1);
    if (S > 1) {
        const double *wk = ws + (int64_t)(S - 2) * E * B;
#pragma unroll
        for (int e = 0; e < E; ++e) wz[e] = e < N * N ? 0.0 : wk[(int64_t)e * B];
    }
    IO *gout = COST && a.grad ? (IO *)a.grad + seg0 : (IO *)nullptr;
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
        double tp[O], ip[M];
        tp[0] = 1.0;
#pragma unroll
        for (int e = 1; e < O; ++e) tp[e] = tp[e - 1] * Tk;
        ip[0] = 1.0;
        ip[1] = fast_rcp(Tk);
#pragma unroll
        for (int e = 2; e < M; ++e) ip[e] = ip[e - 1] * ip[1];
        double s0 = 0.0, s1 = 0.0, vel = 0.0;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            // endpoint derivatives scaled by T^deriv, the segment's start as origin (c = diag(T^-pow) G dh)
            double dh[M];
            dh[0] = 0.0;
            dh[O] = P1[ax] - P0[ax];
#pragma unroll
            for (int r = 0; r < N; ++r) { dh[r + 1] = xk[r][ax] * tp[r + 1]; dh[O + r + 1] = xn[r][ax] * tp[r + 1]; }
            IO q[M];
#pragma unroll
            for (int i = 0; i < M - 1; ++i) {
                double acc = 0.0;
#pragma unroll
                for (int aa = 1; aa < M; ++aa) {
                    constexpr double zero = 0.0;
                    if (Tab<O>::G(i, aa) != zero) acc = fma_<double>(Tab<O>::G(i, aa), dh[aa], acc);
                }
                q[i] = IO(acc * ip[M - 1 - i]);
                nanacc = fma_<double>(double(q[i]), 0.0, nanacc);
            }
            q[M - 1] = IO(P0[ax]);   // p(0) = P_k, copied through
            nanacc = fma_<double>(double(q[M - 1]), 0.0, nanacc);
            store_row<M, IO>(co + ((int64_t)k * 3 + ax) * M, q);
            if (COST) {
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
        }
        if (COST) {
            const double ipw = ip[M - 1];   // T^(1-2o)
            Jacc += fma_<double>(vw, vel, ipw * s0);
            if (gout) {
                const double gk = -(ipw * ip[1]) * fma_<double>(double(M - 1), s0, -2.0 * s1);
                gout[k] = IO(gk);
                nanacc = fma_<double>(double(IO(gk)), 0.0, nanacc);
            }
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
    if (COST) {
        nanacc = fma_<double>(Jacc, 0.0, nanacc);
        if (a.cost) a.cost[b] = Jacc;
    }
    if (!(nanacc == 0.0)) status |= CSP_TRAJ_NONFINITE_BIT;
    if (a.status) a.status[b] = status;
}

template <int O, typename IO> static hipError_t launch_o(const PeriodicArgs &a, hipStream_t st) {
    const unsigned blocks = (unsigned)((a.B + 63) / 64);
    if (a.cost || a.grad) hipLaunchKernelGGL((minsnap_periodic_kernel<O, IO, true>), dim3(blocks), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((minsnap_periodic_kernel<O, IO, false>), dim3(blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

template <typename IO> static hipError_t launch_io(const PeriodicArgs &a, hipStream_t st) {
    switch (a.order) {
        case 2: return launch_o<2, IO>(a, st);
        case 3: return launch_o<3, IO>(a, st);
        case 4: return launch_o<4, IO>(a, st);
        case 5: return launch_o<5, IO>(a, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_periodic(const PeriodicArgs &a, bool f32, hipStream_t st) {
    if (a.B == 0) return hipSuccess;
    return f32 ? launch_io<float>(a, st) : launch_io<double>(a, st);
}

}  // namespace csp
