"""Dense restatement of the periodic (closed-loop) minimum-snap QP, one loop at a time.

TEST INFRASTRUCTURE ONLY.  Independent of the HIP kernel and of tablegen.py: the unknowns are every segment's monomial
coefficients, the Hessian of integral (p^(o))^2 is written in closed form (plus w (v(0)^2 + v(T)^2)), and the
constraints p_j(0) = P_j, p_j(T_j) = P_{j+1 mod S}, p_j^(r)(T_j) = p_{j+1 mod S}^(r)(0) (r = 1..o-1) go into one KKT
system, solved densely.  The same code runs in numpy fp64 and in mpmath at any precision.

    [2H  A^T] [c]   [0]        J = c^T H c,
    [A   0  ] [l] = [b]        dJ/dT_j = c^T (dH/dT_j) c + l^T (dA/dT_j) c        (envelope theorem)

Coefficients come back in the kernel's record format: [S][3][2o], highest power first.
"""
import contextlib
import math

import numpy as np


def _fall(i, k):
    """i (i-1) ... (i-k+1): the k-th derivative factor of t^i."""
    r = 1
    for j in range(k):
        r *= i - j
    return r


class _Num:
    """Scalars and a dense solve, in numpy fp64 (dps None) or in mpmath (inside _Num.ctx(dps))."""

    def __init__(self, dps=None):
        self.mp = None
        if dps is not None:
            import mpmath
            self.mp = mpmath.mp

    @staticmethod
    def ctx(dps):
        if dps is None:
            return contextlib.nullcontext()
        import mpmath
        return mpmath.workdps(int(dps))

    def num(self, x):
        return self.mp.mpf(x) if self.mp else float(x)

    def zeros(self, n, m):
        return self.mp.zeros(n, m) if self.mp else np.zeros((n, m))

    def solve(self, K, R):
        if not self.mp:
            return np.linalg.solve(K, R)
        # Gaussian elimination with partial pivoting on rows held as lists, all right-hand sides at once, zeros skipped
        # (the KKT matrix is sparse): the same dense system at the same precision as mpmath's lu_solve per column, at a
        # fraction of its time
        n, nr = R.rows, R.cols
        rows = [[K[i, j] for j in range(n)] + [R[i, a] for a in range(nr)] for i in range(n)]
        for c in range(n):
            p = max(range(c, n), key=lambda r: abs(rows[r][c]))
            rows[c], rows[p] = rows[p], rows[c]
            piv = rows[c]
            inv = 1 / piv[c]
            nz = [k for k in range(c + 1, n + nr) if piv[k] != 0]
            for r in range(c + 1, n):
                rr = rows[r]
                if rr[c] != 0:
                    f = rr[c] * inv
                    for k in nz:
                        rr[k] -= f * piv[k]
        X = self.mp.zeros(n, nr)
        for a in range(nr):
            x = [None] * n
            for r in range(n - 1, -1, -1):
                rr = rows[r]
                s = rr[n + a]
                for k in range(r + 1, n):
                    if rr[k] != 0:
                        s -= rr[k] * x[k]
                x[r] = s / rr[r]
                X[r, a] = x[r]
        return X


def _kkt(o, path, T, w, nm):
    m = 2 * o
    S = len(T)
    n = S * m
    nc = S * (o + 1)
    K = nm.zeros(n + nc, n + nc)
    R = nm.zeros(n + nc, 3)
    for j in range(S):
        base = j * m
        # Hessian of integral_0^T (p^(o))^2 (times 2), coefficient i ascending: p = sum c_i t^i
        for i in range(o, m):
            for k in range(o, m):
                e = i + k - 2 * o + 1
                K[base + i, base + k] += 2 * _fall(i, o) * _fall(k, o) * T[j] ** e / e
        # w (v(0)^2 + v(T)^2)
        if w != 0:
            for i in range(1, m):
                for k in range(1, m):
                    v = i * k * T[j] ** (i + k - 2)
                    if i == 1 and k == 1:
                        v += 1
                    K[base + i, base + k] += 2 * w * v
    row = n
    for j in range(S):
        base, nxt = j * m, ((j + 1) % S) * m
        K[row, base] = 1                      # p_j(0) = P_j
        for ax in range(3):
            R[row, ax] = path[j][ax]
        row += 1
        for i in range(m):                    # p_j(T_j) = P_{j+1}
            K[row, base + i] = T[j] ** i
        for ax in range(3):
            R[row, ax] = path[(j + 1) % S][ax]
        row += 1
        for r in range(1, o):                 # p_j^(r)(T_j) - p_{j+1}^(r)(0) = 0
            for i in range(r, m):
                K[row, base + i] += _fall(i, r) * T[j] ** (i - r)
            K[row, nxt + r] -= math.factorial(r)
            row += 1
    for a in range(n, n + nc):
        for b in range(n):
            K[b, a] = K[a, b]
    return K, R


def solve(order, path, time, w=0.0, dps=None, raw=False):
    """Returns (coeffs [S,3,2o] highest power first, J, dJ/dT [S]) as float64.  path [S,3], time [S].  dps: mpmath digits
    (None = numpy fp64).  raw: keep the numbers of the solve (mpmath under dps) in object arrays, for checks that need
    more than a double."""
    o = int(order)
    m = 2 * o
    S = len(time)
    path = np.asarray(path, dtype=np.float64)
    org = path[0].copy()
    with _Num.ctx(dps):
        nm = _Num(dps)
        # positions from the first waypoint: J and the derivatives do not depend on a translation
        P = [[nm.num(path[j][ax]) - nm.num(org[ax]) for ax in range(3)] for j in range(S)]
        T = [nm.num(t) for t in np.asarray(time, dtype=np.float64)]
        w_ = nm.num(w)
        K, R = _kkt(o, P, T, w_, nm)
        X = nm.solve(K, R)
        n = S * m
        c = [[[X[j * m + i, ax] for i in range(m)] for ax in range(3)] for j in range(S)]
        lam = [[X[n + q, ax] for ax in range(3)] for q in range(S * (o + 1))]

        def deriv(cc, k, t):
            return sum(_fall(i, k) * cc[i] * t ** (i - k) for i in range(k, m))

        J = nm.num(0)
        g = [nm.num(0) for _ in range(S)]
        for j in range(S):
            q0 = j * (o + 1)
            for ax in range(3):
                cc = c[j][ax]
                for i in range(o, m):
                    for k in range(o, m):
                        e = i + k - 2 * o + 1
                        J += _fall(i, o) * _fall(k, o) * T[j] ** e / e * cc[i] * cc[k]
                vT = deriv(cc, 1, T[j])
                J += w_ * (cc[1] * cc[1] + vT * vT)
                # dH/dT: (p^(o)(T))^2 + 2 w v(T) a(T); dA/dT on the rows at t = T_j: d/dT p^(r)(T) = p^(r+1)(T)
                po = deriv(cc, o, T[j])
                gj = po * po + 2 * w_ * vT * deriv(cc, 2, T[j])
                for r in range(0, o):
                    gj += lam[q0 + 1 + r][ax] * deriv(cc, r + 1, T[j])
                g[j] += gj
        if raw:
            co = np.array([[[c[j][ax][m - 1 - i] if i < m - 1 else nm.num(path[j][ax]) for i in range(m)] for ax in range(3)]
                           for j in range(S)], dtype=object)
            return co, J, np.array(g, dtype=object)
        coeffs = np.zeros((S, 3, m))
        for j in range(S):
            for ax in range(3):
                for i in range(1, m):
                    coeffs[j, ax, m - 1 - i] = float(c[j][ax][i])
                coeffs[j, ax, m - 1] = path[j][ax]   # p_j(0) = P_j (the constraint holds exactly)
        return coeffs, float(J), np.array([float(x) for x in g])


def solve_batch(order, waypoints, times, w=0.0, seg_offsets=None, dps=None):
    """Loops of a uniform ([B,S,3], [B,S]) or ragged ([sum S_b,3], [sum S_b] + seg_offsets) batch; w scalar or [B].
    Returns (coeffs in the layout of the kernel's output, cost [B], grad in the layout of times)."""
    waypoints = np.asarray(waypoints, dtype=np.float64)
    times = np.asarray(times, dtype=np.float64)
    m = 2 * int(order)
    if seg_offsets is None:
        B = times.shape[0]
        loops = [(waypoints[b], times[b]) for b in range(B)]
    else:
        off = np.asarray(seg_offsets)
        B = len(off) - 1
        loops = [(waypoints[off[b]:off[b + 1]], times[off[b]:off[b + 1]]) for b in range(B)]
    ws = np.broadcast_to(np.asarray(w, dtype=np.float64), (B,))
    co, J, G = [], np.zeros(B), []
    for b, (p, t) in enumerate(loops):
        if len(t) == 0:
            co.append(np.zeros((0, 3, m)))
            G.append(np.zeros(0))
            continue
        c, J[b], g = solve(order, p, t, ws[b], dps)
        co.append(c)
        G.append(g)
    if seg_offsets is None:
        return np.stack(co), J, np.stack(G)
    return np.concatenate(co), J, np.concatenate(G)


def eval_deriv(row, k, t):
    """k-th derivative at t of one record (highest power first)."""
    c = np.asarray(row, dtype=np.float64)[::-1]
    return sum(_fall(i, k) * c[i] * t ** (i - k) for i in range(k, len(c)))


def unrolled_middle_lap(order, path, time, laps):
    """The reference's open chain over `laps` repeats of the loop plus the closing point, from rest
    (oracle.numpy_ref.solve_qp_closed_form); returns the middle lap's records [S,3,2o]."""
    from oracle.numpy_ref import solve_qp_closed_form
    path = np.asarray(path, dtype=np.float64)
    S = len(time)
    o = int(order)
    chain = np.concatenate([np.tile(path, (laps, 1)), path[:1]])
    tt = np.tile(np.asarray(time, dtype=np.float64), laps)
    z = np.zeros((2, 3))
    co, _ = solve_qp_closed_form(o, chain, z, z, tt)
    mid = laps // 2
    return co.reshape(laps * S, 3, 2 * o)[mid * S:(mid + 1) * S]
