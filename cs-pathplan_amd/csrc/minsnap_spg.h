// minsnap_spg.h -- the per-lane spectral projected gradient loop of the segment-time optimisers, written
// once over the "pass" that evaluates the cost and its time gradient: minsnap_timeopt.hip instantiates it with cost_pass
// (the standard partition), minsnap_knots_timeopt.hip with the masked pass (per-knot derivative constraints, §23),
// minsnap_periodic_timeopt.hip with the periodic pass (closed loops, §24).
//
// The iterate and the trial point live in the workspace, [buffer][segment][trajectory]: Tb[c][j * B] is time j of buffer
// c, Gb[c][j * B] the cost's gradient there.  Everything is done in T with exact bounds; the scaled variables
// x = T / tau (tau = the start's mean time) and f / f0 only set the step: in T the step is  T - tau * alpha * g^,
// g^ = (tau / f0) grad f,  and the projection onto the scaled set is the projection onto {sum T = C, T >= t_min} scaled
// by tau.
#pragma once
#include "minsnap_device.h"
#include "minsnap_launch.h"

namespace csp {

// Euclidean projection onto {sum_j y_j = C, y_j >= lo} (fixed_total) or {y_j >= lo} (clip): y_j = max(v_j - theta, lo).
// theta by Michelot's algorithm, written over theta alone: the active set {v_j - theta > lo} only shrinks while theta
// grows, so a pass whose count does not change ends it (at most S + 1 passes).  v(j) is recomputed per pass.
template <typename F>
__device__ double proj_theta(F v, int S, bool fixed_total, double C, double lo) {
    if (!fixed_total) return 0.0;
    double sum = 0.0;
    for (int j = 0; j < S; ++j) sum += v(j);
    double theta = (sum - C) / double(S);
    int n = S;
    for (int pass = 0; pass <= S; ++pass) {
        double s = 0.0;
        int m = 0;
        for (int j = 0; j < S; ++j) {
            const double vj = v(j);
            if (vj - theta > lo) { s += vj; ++m; }
        }
        if (m == n || m == 0) break;
        n = m;
        theta = (s - C + double(S - n) * lo) / double(n);
    }
    return theta;
}

// The start: the input's projection (the input itself when it is feasible), written to T0[j * B]; C = the input's total.
// Returns 0, or the status the trajectory stops with before anything is evaluated (nothing is written then):
// NONFINITE for an inf / NaN time -- the total has no projection (Michelot's theta would be NaN and every entry would
// come back as min_time) -- and NOT_CONVERGED for an infeasible fixed total (device memory: the C-ABI could not check it
// on the host).
template <typename IO>
__device__ __forceinline__ int spg_start(const IO *tin, int S, bool ft, double lo, double *T0, int64_t B, double &C) {
    C = 0.0;
    bool feasible = true;
    for (int j = 0; j < S; ++j) {
        const double t = double(tin[j]);
        C += t;
        feasible = feasible && t >= lo;
    }
    const bool nonfinite = !(fabs(C) <= 1.7976931348623157e308);
    if (nonfinite) return CSP_TRAJ_NONFINITE_BIT;
    if (ft && C < double(S) * lo) return CSP_TRAJ_NOT_CONVERGED_BIT;
    const double Ct = C;
    const double th0 = feasible ? 0.0 : proj_theta([&](int j) { return double(tin[j]); }, S, ft, Ct, lo);
    for (int j = 0; j < S; ++j) {
        const double t = double(tin[j]);
        T0[(int64_t)j * B] = feasible ? t : fmax(t - th0, lo);
    }
    return 0;
}

struct SpgResult {
    int status, iters, cur;   // cur: the buffer of the accepted iterate
    double f0, f;             // objective (cost + rho sum T) at the start and at the accepted iterate
};

// Spectral projected gradient: Barzilai-Borwein step, monotone Armijo backtracking with a safeguarded quadratic step.
// pass(eb, J) evaluates buffer eb: it reads Tb[eb], writes the cost's gradient to Gb[eb] and the cost to J, and returns
// the solve's status bits (non-zero: the point cannot be taken).  One evaluation site: every turn of the loop evaluates
// the buffer `eb` (the start, Tb[0], then trial points) and then decides what to do next.
template <typename Pass>
__device__ __forceinline__ SpgResult spg_minimise(Pass pass, double *const (&Tb)[2], double *const (&Gb)[2], int64_t B, int S,
                                                  bool ft, double C, double lo, double rho, double tol, int max_iters) {
    constexpr double kArmijo = 1e-4, kAlphaMin = 1e-10, kAlphaMax = 1e4;
    constexpr int kMaxBacktrack = 30;
    int status = 0, iters = 0;
    double f0 = 0.0, f = 0.0;

    int cur = 0;                 // buffer of the accepted iterate
    bool first = true;
    double tau = 1.0, k = 1.0, alpha = 1.0, lam = 1.0, thd = 0.0, gd = 0.0, fs = 1.0;
    // tau * alpha * g^_j = step * grad f_j
    auto pg_measure = [&](int c) {   // max_j |T_j - P(T_j - tau g^_j)| / tau
        const double st = tau * k;
        const double th = proj_theta([&](int j) { return Tb[c][(int64_t)j * B] - st * (Gb[c][(int64_t)j * B] + rho); },
                                     S, ft, C, lo);
        double m = 0.0;
        for (int j = 0; j < S; ++j) {
            const double t = Tb[c][(int64_t)j * B];
            m = fmax(m, fabs(t - fmax(t - st * (Gb[c][(int64_t)j * B] + rho) - th, lo)));
        }
        return m / tau;
    };
    // direction d = P(T - tau alpha g^) - T (its theta kept in thd), gd = grad f . d; then the trial T + lam d
    auto direction = [&]() {
        const double st = tau * alpha * k;
        thd = proj_theta([&](int j) { return Tb[cur][(int64_t)j * B] - st * (Gb[cur][(int64_t)j * B] + rho); }, S, ft, C, lo);
        gd = 0.0;
        for (int j = 0; j < S; ++j) {
            const double t = Tb[cur][(int64_t)j * B], gj = Gb[cur][(int64_t)j * B] + rho;
            gd = fma_<double>(gj, fmax(t - st * gj - thd, lo) - t, gd);
        }
    };
    auto trial = [&]() {
        const double st = tau * alpha * k;
        double *tt = Tb[cur ^ 1];
        for (int j = 0; j < S; ++j) {
            const double t = Tb[cur][(int64_t)j * B], gj = Gb[cur][(int64_t)j * B] + rho;
            tt[(int64_t)j * B] = fma_<double>(lam, fmax(t - st * gj - thd, lo) - t, t);
        }
        // T + lam d is feasible in exact arithmetic; the projection removes the rounding (sum drift, bounds)
        const double th = proj_theta([&](int j) { return tt[(int64_t)j * B]; }, S, ft, C, lo);
        for (int j = 0; j < S; ++j) tt[(int64_t)j * B] = fmax(tt[(int64_t)j * B] - th, lo);
    };

    int eb = 0, backtracks = 0;
    while (true) {
        double J = 0.0;
        const int st = pass(eb, J);
        double sumT = 0.0;
        if (rho != 0.0)
            for (int j = 0; j < S; ++j) sumT += Tb[eb][(int64_t)j * B];
        const double fe = fma_<double>(rho, sumT, J);
        if (st) {
            if (first) {   // the start itself: the trajectory stops there
                status |= st;
                f0 = f = fe;
                break;
            }
            // a trial point the solve cannot take (extreme times after a long step): rejected like a failed
            // Armijo test, with a tenth of the step
            if (++backtracks > kMaxBacktrack) {
                status |= CSP_TRAJ_NOT_CONVERGED_BIT;
                break;
            }
            lam *= 0.1;
            trial();
            continue;
        }
        bool accept;
        if (first) {
            first = false;
            accept = false;
            f0 = f = fe;
            fs = f0 > 0.0 ? f0 : 1.0;
            tau = 0.0;
            for (int j = 0; j < S; ++j) tau += Tb[0][(int64_t)j * B];
            tau /= double(S);
            k = tau / fs;
            const double pg = pg_measure(cur);
            if (pg <= tol || iters >= max_iters) { if (pg > tol) status |= CSP_TRAJ_NOT_CONVERGED_BIT; break; }
            alpha = fmin(kAlphaMax, fmax(kAlphaMin, 1.0 / pg));
        } else {
            accept = fe <= f && fe <= fma_<double>(kArmijo * lam, gd, f);
            if (!accept) {   // backtrack: minimiser of the quadratic through f, gd and fe, kept in [0.1, 0.5] lam
                if (++backtracks > kMaxBacktrack) {
                    status |= CSP_TRAJ_NOT_CONVERGED_BIT;   // no decrease within rounding: stop at the accepted point
                    break;
                }
                const double lt = -0.5 * lam * lam * gd / (fe - f - lam * gd);
                lam = (lt >= 0.1 * lam && lt <= 0.5 * lam) ? lt : 0.5 * lam;
                trial();
                continue;
            }
        }
        if (accept) {
            // Barzilai-Borwein step from s = (T+ - T) / tau and y = g^+ - g^
            const int nx = cur ^ 1;
            double ss = 0.0, sy = 0.0;
            for (int j = 0; j < S; ++j) {
                const double s = (Tb[nx][(int64_t)j * B] - Tb[cur][(int64_t)j * B]) / tau;
                ss = fma_<double>(s, s, ss);
                sy = fma_<double>(s, k * (Gb[nx][(int64_t)j * B] - Gb[cur][(int64_t)j * B]), sy);
            }
            cur = nx;
            f = fe;
            ++iters;
            const double pg = pg_measure(cur);
            // no positive curvature along s: the start's rule, a step of unit length in the scaled variables
            alpha = fmin(kAlphaMax, fmax(kAlphaMin, sy > 0.0 ? ss / sy : 1.0 / pg));
            if (pg <= tol) break;
            if (iters >= max_iters) { status |= CSP_TRAJ_NOT_CONVERGED_BIT; break; }
        }
        direction();
        lam = 1.0;
        backtracks = 0;
        trial();
        eb = cur ^ 1;
    }
    return SpgResult{status, iters, cur, f0, f};
}

}  // namespace csp
