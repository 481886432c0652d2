"""Dense numpy restatement of the snap cost and its time gradient under per-knot derivative constraints, and of the
segment-time optimiser over it, one trajectory at a time.

TEST INFRASTRUCTURE ONLY.  Independent of the HIP kernels: tests/timeopt_ref.py with an arbitrary fixed / free partition.
The free set is the unmasked derivatives 1..o-1 of every knot 0..S (timeopt_ref frees the interior knots alone); the
segment matrices are the scaling-law tables of timeopt_ref._scaled_tables, the free block is solved with
numpy.linalg.solve, the gradient is the envelope formula written over the dense Qt with the segment's start as origin,
and the optimiser is §12's algorithm with timeopt_ref's projection, measure and constants.
"""
import numpy as np

from tests import knots_ref
from tests.timeopt_ref import ALPHA_MAX, ALPHA_MIN, ARMIJO, MAX_BACKTRACK, NOT_CONVERGED, _scaled_tables, pg_measure, project


def endpoint_derivatives(order, path, time, mask, values, w=0.0):
    """Returns (D [S, 2o, 3] per-segment endpoint derivatives at the optimum of the masked problem, tables per segment).
    A value whose mask bit is clear is never read.  Raises knots_ref.Underdetermined below the constraint count."""
    o = int(order)
    n = o - 1
    path = np.asarray(path, dtype=np.float64)
    path = path - path[0]   # J does not depend on a translation; centring removes cancellation in d^T Qt d
    T = np.asarray(time, dtype=np.float64)
    S = len(T)
    mask = np.asarray(mask).astype(np.int64).reshape(S + 1)
    values = np.asarray(values, dtype=np.float64).reshape(S + 1, n, 3)
    if knots_ref.constraint_count(o, mask) < o:
        raise knots_ref.Underdetermined("%d constraints, order %d" % (knots_ref.constraint_count(o, mask), o))
    V = (S + 1) * o
    seg = [np.r_[j * o:(j + 2) * o] for j in range(S)]
    tabs = [_scaled_tables(o, T[j], w) for j in range(S)]
    K = np.zeros((V, V))
    for j in range(S):
        K[np.ix_(seg[j], seg[j])] += tabs[j][3]
    pinned = lambda k, r: bool((mask[k] >> (r - 1)) & 1)
    free = np.array([k * o + r for k in range(S + 1) for r in range(1, o) if not pinned(k, r)], dtype=int)
    fixed = np.setdiff1d(np.arange(V), free)
    D = np.zeros((V, 3))
    for k in range(S + 1):
        D[k * o] = path[k]
        for r in range(1, o):
            if pinned(k, r):
                D[k * o + r] = values[k, r - 1]
    if len(free):
        D[free] = -np.linalg.solve(K[np.ix_(free, free)], K[np.ix_(free, fixed)] @ D[fixed])
    return np.stack([D[seg[j]] for j in range(S)]), tabs


def cost_grad(order, path, time, mask, values, w=0.0):
    """J = sum_j sum_axes d_j^T Qt^w_j d_j and the envelope gradient dJ/dT_j: pinned derivatives do not depend on T, free
    ones are at the optimum, and the w term does not depend on T."""
    o = int(order)
    T = np.asarray(time, dtype=np.float64)
    d, tabs = endpoint_derivatives(o, path, T, mask, values, w)
    deriv = np.array([a % o for a in range(2 * o)], dtype=np.float64)
    expo = 1 - 2 * o + deriv[:, None] + deriv[None, :]
    J = 0.0
    g = np.zeros(len(T))
    for j in range(len(T)):
        Qt, Qw = tabs[j][2], tabs[j][3]
        dj = d[j].copy()
        dj[[0, o]] -= dj[0]   # the segment's start position as origin (Qt annihilates constants): less cancellation
        J += np.einsum("ax,ab,bx->", dj, Qw, dj)
        g[j] = np.einsum("ax,ab,bx->", dj, expo * Qt, dj) / T[j]
    return J, g


def _objective(order, path, T, mask, values, w, rho):
    J, g = cost_grad(order, path, T, mask, values, w)
    return J + rho * T.sum(), g + rho


def optimize(order, path, time, mask, values, w=0.0, mode="fixed_total", rho=0.0, min_time=0.01, tol=1e-6, max_iters=100):
    """The kernel's optimiser (timeopt_ref.optimize over the masked objective).  Returns dict(times, f0, f, iterations,
    status)."""
    T = np.asarray(time, dtype=np.float64).copy()
    ft = mode == "fixed_total"
    rho = 0.0 if ft else float(rho)
    total = T.sum() if ft else None
    if np.any(T < min_time):
        T = project(T, min_time, total)
    f, gf = _objective(order, path, T, mask, values, w, rho)
    f0 = f
    fs = f0 if f0 > 0 else 1.0
    tau = T.mean()
    k = tau / fs
    pg = pg_measure(T, gf, tau, fs, min_time, total)
    it = 0
    if pg <= tol:
        return dict(times=T, f0=f0, f=f, iterations=0, status=0)
    if max_iters == 0:
        return dict(times=T, f0=f0, f=f, iterations=0, status=NOT_CONVERGED)
    alpha = min(ALPHA_MAX, max(ALPHA_MIN, 1.0 / pg))
    while True:
        P = project(T - tau * alpha * k * gf, min_time, total)
        d = P - T
        gd = float(gf @ d)
        lam, bt = 1.0, 0
        while True:
            Tt = project(T + lam * d, min_time, total)
            try:
                fe, ge = _objective(order, path, Tt, mask, values, w, rho)
                failed = not (np.isfinite(fe) and np.all(np.isfinite(ge)))
            except np.linalg.LinAlgError:
                failed = True
            if not failed and fe <= f and fe <= f + ARMIJO * lam * gd:
                break
            bt += 1
            if bt > MAX_BACKTRACK:
                return dict(times=T, f0=f0, f=f, iterations=it, status=NOT_CONVERGED)
            if failed:   # a trial point the solve cannot take (extreme times after a long step): a tenth of the step
                lam *= 0.1
                continue
            lt = -0.5 * lam * lam * gd / (fe - f - lam * gd)
            lam = lt if 0.1 * lam <= lt <= 0.5 * lam else 0.5 * lam
        s = (Tt - T) / tau
        y = k * (ge - gf)
        ss, sy = float(s @ s), float(s @ y)
        T, f, gf = Tt, fe, ge
        it += 1
        pg = pg_measure(T, gf, tau, fs, min_time, total)
        alpha = min(ALPHA_MAX, max(ALPHA_MIN, ss / sy if sy > 0 else 1.0 / pg))
        if pg <= tol:
            return dict(times=T, f0=f0, f=f, iterations=it, status=0)
        if it >= max_iters:
            return dict(times=T, f0=f0, f=f, iterations=it, status=NOT_CONVERGED)
