"""Dense numpy restatement of the snap cost, its time gradient and the segment-time optimiser, one
trajectory at a time.

TEST INFRASTRUCTURE ONLY.  Independent of the HIP kernel: the endpoint derivatives come from the dense system of
tests/vjp_ref.py (Qt = M^-T Q M^-1 by dense inverses, the free block solved with numpy.linalg.solve), the gradient is the
envelope formula written over the dense Qt, and the optimiser is the kernel's algorithm (spectral projected gradient,
Barzilai-Borwein step, monotone Armijo backtracking, Michelot projection) with the same constants.
"""
import numpy as np

from tests.vjp_ref import _seg_tables

_UNIT = {}


def _scaled_tables(o, T, w):
    """(None, None, Qt(T), Qt^w(T)) from the dense Qt(1) (cached) by the scaling law Qt_ab(T) = Qt_ab(1) T^(1-2o+da+db)
    (DESIGN.md §2): the dense inverse of M(T) at every T would add ~1e-9 relative noise to J at order 4, more than the
    line search can tolerate near the optimum."""
    if o not in _UNIT:
        deriv = np.array([a % o for a in range(2 * o)], dtype=np.float64)
        _UNIT[o] = (_seg_tables(o, 1.0, 0.0)[2], 1 - 2 * o + deriv[:, None] + deriv[None, :])
    Q1, expo = _UNIT[o]
    Qt = Q1 * float(T) ** expo
    Qw = Qt.copy()
    Qw[1, 1] += w
    Qw[o + 1, o + 1] += w
    return None, None, Qt, Qw

ARMIJO, ALPHA_MIN, ALPHA_MAX, MAX_BACKTRACK = 1e-4, 1e-10, 1e4, 30
NOT_CONVERGED = 8


def endpoint_derivatives(order, path, time, bc, w=0.0):
    """Returns (D [S, 2o, 3] per-segment endpoint derivatives at the optimum, tables per segment)."""
    o = int(order)
    path = np.asarray(path, dtype=np.float64)
    path = path - path[0]   # J does not depend on a translation; centring removes cancellation in d^T Qt d
    T = np.asarray(time, dtype=np.float64)
    bc = np.asarray(bc, dtype=np.float64).reshape(4, 3)
    S = len(T)
    V = (S + 1) * o
    seg = [np.r_[j * o:(j + 2) * o] for j in range(S)]
    tabs = [_scaled_tables(o, T[j], w) for j in range(S)]
    K = np.zeros((V, V))
    for j in range(S):
        K[np.ix_(seg[j], seg[j])] += tabs[j][3]
    free = np.array([k * o + r for k in range(1, S) for r in range(1, o)], dtype=int)
    fixed = np.setdiff1d(np.arange(V), free)
    D = np.zeros((V, 3))
    for k in range(S + 1):
        D[k * o] = path[k]
    if o >= 2:
        D[1], D[S * o + 1] = bc[0], bc[1]
    if o >= 3:
        D[2], D[S * o + 2] = bc[2], bc[3]
    if len(free):
        D[free] = -np.linalg.solve(K[np.ix_(free, free)], K[np.ix_(free, fixed)] @ D[fixed])
    return np.stack([D[seg[j]] for j in range(S)]), tabs


def cost_grad(order, path, time, bc, w=0.0):
    """J = sum_j sum_axes d_j^T Qt^w_j d_j and the envelope gradient dJ/dT_j (the w term does not depend on T)."""
    o = int(order)
    T = np.asarray(time, dtype=np.float64)
    d, tabs = endpoint_derivatives(o, path, T, bc, w)
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


def cost_from_coeffs(order, coeffs, time, w=0.0):
    """sum_j sum_axes [ int_0^T_j (p^(o))^2 dt + w (v(0)^2 + v(T_j)^2) ] by exact polynomial integration of coefficients
    [S, 3, 2o] (highest power first)."""
    o = int(order)
    J = 0.0
    for j, Tj in enumerate(np.asarray(time, dtype=np.float64)):
        for ax in range(3):
            c = np.asarray(coeffs[j][ax], dtype=np.float64)
            po = np.polyder(c, o)
            J += np.polyval(np.polyint(np.polymul(po, po)), Tj)
            v = np.polyder(c, 1)
            J += w * (np.polyval(v, 0.0) ** 2 + np.polyval(v, Tj) ** 2)
    return J


def project(v, lo, total=None):
    """Euclidean projection onto {sum y = total, y >= lo} (Michelot's algorithm over theta) or, total=None, {y >= lo}."""
    v = np.asarray(v, dtype=np.float64)
    if total is None:
        return np.maximum(v, lo)
    S = len(v)
    theta = (v.sum() - total) / S
    n = S
    for _ in range(S + 1):
        act = v - theta > lo
        m = int(act.sum())
        if m == n or m == 0:
            break
        n = m
        theta = (v[act].sum() - total + (S - n) * lo) / n
    return np.maximum(v - theta, lo)


def _objective(order, path, T, bc, w, rho):
    J, g = cost_grad(order, path, T, bc, w)
    return J + rho * T.sum(), g + rho


def pg_measure(T, gf, tau, fs, lo, total):
    """max_j |x_j - P(x_j - g^_j)| in the scaled variables x = T / tau, g^ = (tau / fs) grad f."""
    T = np.asarray(T, dtype=np.float64)
    return np.max(np.abs(T - project(T - tau * (tau / fs) * gf, lo, total))) / tau


def optimize(order, path, time, bc, w=0.0, mode="fixed_total", rho=0.0, min_time=0.01, tol=1e-6, max_iters=100):
    """The kernel's optimiser.  Returns dict(times, f0, f, iterations, status)."""
    T = np.asarray(time, dtype=np.float64).copy()
    ft = mode == "fixed_total"
    rho = 0.0 if ft else float(rho)
    total = T.sum() if ft else None
    if np.any(T < min_time):
        T = project(T, min_time, total)
    f, gf = _objective(order, path, T, bc, w, rho)
    f0 = f
    fs = f0 if f0 > 0 else 1.0
    tau = T.mean()
    k = tau / fs
    pg = pg_measure(T, gf, tau, fs, min_time, total)
    it, status = 0, 0
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
            fe, ge = _objective(order, path, Tt, bc, w, rho)
            if fe <= f and fe <= f + ARMIJO * lam * gd:
                break
            bt += 1
            if bt > MAX_BACKTRACK:
                return dict(times=T, f0=f0, f=f, iterations=it, status=NOT_CONVERGED)
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


def batch_apply(fn, seg_offsets, waypoints, times, bc, w):
    """Calls fn(b, path, time, bc_b, w_b) per trajectory of a ragged (concatenated) batch; returns the list of results."""
    seg_offsets = np.asarray(seg_offsets)
    B = len(seg_offsets) - 1
    bc = np.asarray(bc, dtype=np.float64).reshape(-1, 4, 3)
    wv = np.broadcast_to(np.asarray(w, dtype=np.float64), (B,))
    out = []
    for b in range(B):
        s0, s1 = int(seg_offsets[b]), int(seg_offsets[b + 1])
        out.append(fn(b, waypoints[s0 + b:s1 + b + 1], times[s0:s1], bc[b if bc.shape[0] > 1 else 0], float(wv[b])))
    return out
