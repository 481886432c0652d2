"""Multi-precision reference adjoint of the knot-constrained minimum-snap solve (csp_minsnap_solve_knots_batch_vjp,
DESIGN.md §22).

TEST INFRASTRUCTURE ONLY.  Independent of the HIP kernels: written from the math, with the dense assembly of
tests/knots_ref.solve (no block recursion).  For L = sum p_bar . coeffs + J_bar J of one trajectory, per axis:

    d_bar_j = diag(T^da) G^T diag(T^-pow) p_bar_j, scattered to the knots' derivative slots
    R_ff lambda_f = d_bar_f, lambda_F = 0                        (R: the Hessian over all knot derivatives)
    u = Qt^w_j lambda~_j,  e = 2 J_bar Qt^w_j d_j                (lambda~: lambda at the segment's slots, 0 at positions
                                                                  and pins)
    a position slot adds d_bar - u + e to dL/dP of its knot, a pinned slot to dL/dvalues[knot][r]; a free slot's is 0
    T_bar_j = (1/T_j) [ sum_a da d_a d_bar_a - sum_i pow_i p_i p_bar_i - sum_ab (1-2o+da+db) lambda~_a Qt_ab d_b
                        + J_bar sum_ab (1-2o+da+db) Qt_ab d_a d_b ]          (summed over the axes, Qt without w)

    adjoint(order, path, time, mask, values, pbar=None, jbar=0.0, vel_zero_weight=0, dps=40)
        -> Adjoint(waypoints [S+1,3], times [S], values [S+1,o-1,3])
    adjoints(order, path, time, mask, values, cotangents, vel_zero_weight=0, dps=40)
        -> [Adjoint, ...] for a list of (pbar or None, jbar): one assembly and one primal solve shared by all of them

dps=None runs the same code in Python floats: that run is e_cpu64.
"""
import collections
import contextlib

import numpy as np

from tests import knots_ref, spread_ref

Adjoint = collections.namedtuple("Adjoint", "waypoints times values")


def adjoint(order, path, time, mask, values, pbar=None, jbar=0.0, vel_zero_weight=0.0, dps=40):
    return adjoints(order, path, time, mask, values, [(pbar, jbar)], vel_zero_weight, dps)[0]


def adjoints(order, path, time, mask, values, cotangents, vel_zero_weight=0.0, dps=40):
    o = int(order)
    m, n = 2 * o, o - 1
    path = np.asarray(path, dtype=np.float64)
    time = np.asarray(time, dtype=np.float64)
    S = len(time)
    assert o >= 2 and S >= 1 and path.shape == (S + 1, 3)
    mask = np.asarray(mask).astype(np.int64).reshape(S + 1)
    values = np.asarray(values, dtype=np.float64).reshape(S + 1, n, 3)
    if knots_ref.constraint_count(o, mask) < o:
        raise knots_ref.Underdetermined("%d constraints, order %d" % (knots_ref.constraint_count(o, mask), o))
    G1, Q1 = spread_ref.unit_tables(o)
    if dps is None:
        ctx, num = contextlib.nullcontext(), float
    else:
        import mpmath
        ctx, num = mpmath.workdps(int(dps)), mpmath.mpf
    with ctx:
        zero = num(0)
        G = [[num(v) for v in row] for row in G1]
        Qu = [[num(v) for v in row] for row in Q1]
        w = num(float(vel_zero_weight))
        T = [num(float(t)) for t in time]
        P = [[num(float(path[k, ax])) for ax in range(3)] for k in range(S + 1)]
        NN = (S + 1) * n
        R = [[zero] * NN for _ in range(NN)]
        g = [[zero] * NN for _ in range(3)]
        Qs, Qw = [], []

        def var(j, a):
            side, r = divmod(a, o)
            return None if r == 0 else (j + side) * n + r - 1

        for j in range(S):
            q = [[Qu[a][b] * T[j] ** (1 - 2 * o + a % o + b % o) for b in range(m)] for a in range(m)]
            qw = [list(row) for row in q]
            qw[1][1] += w
            qw[o + 1][o + 1] += w
            Qs.append(q)
            Qw.append(qw)
            for a in range(m):
                va = var(j, a)
                if va is None:
                    continue
                for b in range(m):
                    vb = var(j, b)
                    if vb is None:
                        for ax in range(3):
                            g[ax][va] += qw[a][b] * P[j + b // o][ax]
                    else:
                        R[va][vb] += qw[a][b]
        fixed = [k * n + r for k in range(S + 1) for r in range(n) if (mask[k] >> r) & 1]
        isfixed = set(fixed)
        free = [i for i in range(NN) if i not in isfixed]
        A = [[R[i][j] for j in free] for i in free]
        x = [[zero] * NN for _ in range(3)]
        for ax in range(3):
            for i in fixed:
                x[ax][i] = num(float(values[i // n, i % n, ax]))
        if free:
            rhs = [[-(g[ax][i] + sum((R[i][j] * x[ax][j] for j in fixed if abs(i - j) < 2 * n), zero)) for i in free]
                   for ax in range(3)]
            sol = knots_ref._band_solve(A, rhs, len(free), 2 * n - 1)
            for ax in range(3):
                for i, v in zip(free, sol[ax]):
                    x[ax][i] = v
        out = []
        for pbar, jbar in cotangents:
            jb = num(float(jbar))
            if pbar is not None:
                pbar = np.asarray(pbar, dtype=np.float64).reshape(S, 3, m)
            # d_bar per segment and scattered to the knots
            dbs = [[[zero] * m for _ in range(3)] for _ in range(S)]
            dbar = [[zero] * NN for _ in range(3)]
            if pbar is not None:
                for j in range(S):
                    for ax in range(3):
                        pb = [num(float(pbar[j, ax, i])) for i in range(m)]
                        for a in range(m):
                            dbs[j][ax][a] = T[j] ** (a % o) * sum(G[i][a] * pb[i] / T[j] ** (m - 1 - i) for i in range(m))
                            va = var(j, a)
                            if va is not None:
                                dbar[ax][va] += dbs[j][ax][a]
            lam = [[zero] * NN for _ in range(3)]
            if free and pbar is not None:
                sol = knots_ref._band_solve(A, [[dbar[ax][i] for i in free] for ax in range(3)], len(free), 2 * n - 1)
                for ax in range(3):
                    for i, v in zip(free, sol[ax]):
                        lam[ax][i] = v
            gwp = [[zero] * 3 for _ in range(S + 1)]
            gkv = [[zero] * 3 for _ in range(NN)]
            gt = [zero] * S
            for j in range(S):
                t = zero
                for ax in range(3):
                    d = [P[j + a // o][ax] if a % o == 0 else x[ax][var(j, a)] for a in range(m)]
                    lt = [zero if a % o == 0 else lam[ax][var(j, a)] for a in range(m)]
                    for a in range(m):
                        u = sum(Qw[j][a][b] * lt[b] for b in range(m))
                        e = 2 * jb * sum(Qw[j][a][b] * d[b] for b in range(m))
                        v = dbs[j][ax][a] - u + e
                        va = var(j, a)
                        if va is None:
                            gwp[j + a // o][ax] += v
                        elif va in isfixed:
                            gkv[va][ax] += v
                    if pbar is not None:
                        p = [sum(G[i][a] * T[j] ** (a % o) * d[a] for a in range(m)) / T[j] ** (m - 1 - i) for i in range(m)]
                        t += sum((a % o) * d[a] * dbs[j][ax][a] for a in range(m))
                        t -= sum((m - 1 - i) * p[i] * num(float(pbar[j, ax, i])) for i in range(m))
                    for a in range(m):
                        for b in range(m):
                            c = (1 - 2 * o + a % o + b % o) * Qs[j][a][b] * d[b]
                            t += (jb * d[a] - lt[a]) * c
                gt[j] = t / T[j]
            out.append(Adjoint(np.array([[float(v) for v in row] for row in gwp]), np.array([float(v) for v in gt]),
                               np.array([[float(v) for v in row] for row in gkv]).reshape(S + 1, n, 3)))
        return out
