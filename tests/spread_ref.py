"""Multi-precision reference for the open-chain minimum-snap solve, and the unequal-time input patterns.

TEST INFRASTRUCTURE ONLY.  Independent of the HIP kernels, of cs-pathplan_amd/tablegen.py and of oracle/: written from
the math of DESIGN.md §2.  Per segment, d = [derivatives 0..o-1 at t = 0 ; derivatives 0..o-1 at t = T] and the cost
is d^T Qt(T) d with

    Qt_ab(T) = Qt_ab(1) T^(1 - 2o + da + db),        Qt(1) = M(1)^-T Q(1) M(1)^-1        (da = a mod o),

plus w on the two velocity diagonals (the zero-velocity penalty).  Interior knot k owns the o-1 free derivatives shared
by segment k-1's end and segment k's start, so the normal equations are block-tridiagonal with (o-1)x(o-1) blocks: one
forward elimination, one back substitution, three right-hand sides.  The coefficients are recovered as
p = M(T)^-1 d = diag(T^-pow) M(1)^-1 diag(T^da) d.  The unit tables Qt(1) and M(1)^-1 are computed once per order at
60 digits; everything else runs at `dps` digits (40 by default; dps=None is plain Python floats through the same code).
O(S) per trajectory.  tests/test_spread_ref.py ties it to the 60-digit KKT (no block elimination) and to fixture F8.

Coefficients come back as [S, 3, 2o], highest power first, rounded to double.

The patterns (`spread_times`, `spread_batch`, `spread_loops`) draw segment times whose largest ratio inside one
trajectory is R, scaled so that their geometric mean is about 1:
    log   T = exp(U(-ln R / 2, ln R / 2))
    alt   T alternates between 1/sqrt(R) and sqrt(R), each times U(0.9, 1.1)
    ramp  T_j = R^(j/(S-1) - 1/2) (every other trajectory descending)
    dist  log-uniform times of ratio R with the waypoints re-laid at constant speed: unit random directions, step
          length 5 T_j -- what time allocation at v_avg = 5 gives for legs of unequal length
"""
import contextlib

import numpy as np

_UNIT = {}
UNIT_DPS = 60


def _ff(a, k):
    r = 1
    for q in range(k):
        r *= a - q
    return r


def _inverse(A, n, one):
    """Gauss-Jordan with partial pivoting on a list-of-lists matrix (mpmath scalars)."""
    A = [list(A[i]) + [one if i == j else 0 * one for j in range(n)] for i in range(n)]
    for c in range(n):
        p = max(range(c, n), key=lambda r: abs(A[r][c]))
        A[c], A[p] = A[p], A[c]
        inv = one / A[c][c]
        A[c] = [v * inv for v in A[c]]
        for r in range(n):
            if r != c and A[r][c] != 0:
                f = A[r][c]
                A[r] = [x - f * y for x, y in zip(A[r], A[c])]
    return [row[n:] for row in A]


def unit_tables(order):
    """(G = M(1)^-1, Qt(1)) as lists of mpmath numbers at UNIT_DPS digits; coefficient index i is power 2o-1-i."""
    o = int(order)
    if o in _UNIT:
        return _UNIT[o]
    import mpmath
    m = 2 * o
    with mpmath.workdps(UNIT_DPS):
        one = mpmath.mpf(1)
        M = [[0 * one] * m for _ in range(m)]
        Q = [[0 * one] * m for _ in range(m)]
        for i in range(m):
            pw = m - 1 - i
            for r in range(o):
                if pw == r:
                    M[r][i] = one * _ff(pw, r)           # p^(r)(0)
                if pw >= r:
                    M[o + r][i] = one * _ff(pw, r)       # p^(r)(1)
            for l in range(m):
                pl = m - 1 - l
                if pw >= o and pl >= o:
                    Q[i][l] = one * (_ff(pw, o) * _ff(pl, o)) / (pw + pl - 2 * o + 1)
        G = _inverse(M, m, one)
        QG = [[sum(Q[i][k] * G[k][b] for k in range(m)) for b in range(m)] for i in range(m)]
        Qt = [[sum(G[k][a] * QG[k][b] for k in range(m)) for b in range(m)] for a in range(m)]
        _UNIT[o] = (G, Qt)
    return _UNIT[o]


def _spd_solve(A, cols, n):
    """A^-1 [cols] for a symmetric positive definite n x n list matrix by elimination without pivoting; cols is a list
    of right-hand-side columns (each a list of n)."""
    A = [list(r) for r in A]
    cols = [list(c) for c in cols]
    for c in range(n):
        inv = 1 / A[c][c]
        for r in range(c + 1, n):
            f = A[r][c] * inv
            if f == 0:
                continue
            for k in range(c, n):
                A[r][k] -= f * A[c][k]
            for col in cols:
                col[r] -= f * col[c]
    for col in cols:
        for r in range(n - 1, -1, -1):
            s = col[r]
            for k in range(r + 1, n):
                s -= A[r][k] * col[k]
            col[r] = s / A[r][r]
    return cols


def _cofactor3_solve(A, cols, n):
    """A^-1 [cols] for n = 3 by the cofactor (adjugate / determinant) inverse, the way the register-resident and the
    multi-lane kernels invert their 3 x 3 pivots at order 4 (SmallSpd<3>: one reciprocal, a short dependency chain)."""
    a, b, c, d, e, f = A[0][0], A[1][0], A[1][1], A[2][0], A[2][1], A[2][2]
    c00, c10, c20 = c * f - e * e, d * e - b * f, b * e - c * d
    c11, c21, c22 = a * f - d * d, b * d - a * e, a * c - b * b
    rd = 1 / (a * c00 + b * c10 + d * c20)
    inv = [[c00 * rd, c10 * rd, c20 * rd], [c10 * rd, c11 * rd, c21 * rd], [c20 * rd, c21 * rd, c22 * rd]]
    return [[sum(inv[r][k] * col[k] for k in range(3)) for r in range(3)] for col in cols]


def solve(order, path, time, bc=None, vel_zero_weight=0.0, dps=40, meet=None, cofactor3=False):
    """One trajectory: path [S+1,3], time [S], bc [4,3] (rows start vel, end vel, start acc, end acc; None = zeros).
    Returns coefficients [S,3,2o], highest power first, as float64.  meet: the knot at which a left-to-right and a
    right-to-left sweep meet (a twisted elimination; None: one sweep, left to right); cofactor3: at order 4 invert the
    3 x 3 pivots by cofactors instead of elimination.  Both give the same answer at 40 digits and another rounding with
    dps=None, which is what they are for: plain fp64 doing a kernel's own math."""
    spd = _cofactor3_solve if (cofactor3 and int(order) == 4) else _spd_solve
    o = int(order)
    m, n = 2 * o, int(order) - 1
    path = np.asarray(path, dtype=np.float64)
    time = np.asarray(time, dtype=np.float64)
    S = len(time)
    assert path.shape == (S + 1, 3)
    bc = np.zeros((4, 3)) if bc is None else np.asarray(bc, dtype=np.float64).reshape(4, 3)
    G1, Q1 = unit_tables(o)
    if dps is None:
        ctx, num = contextlib.nullcontext(), float
    else:
        import mpmath
        ctx, num = mpmath.workdps(int(dps)), mpmath.mpf
    with ctx:
        G = [[num(v) for v in row] for row in G1]
        Qu = [[num(v) for v in row] for row in Q1]
        w = num(float(vel_zero_weight))
        zero, one = num(0), num(1)
        T = [num(float(t)) for t in time]
        P = [[num(float(path[k, ax])) for ax in range(3)] for k in range(S + 1)]
        # d[j][a][ax]: the known entries; the free ones (None) are filled after the solve
        d = [[None] * m for _ in range(S)]
        for j in range(S):
            d[j][0], d[j][o] = P[j], P[j + 1]
        for r in range(1, o):
            d[0][r] = [num(float(bc[0 if r == 1 else 2, ax])) if r <= 2 else zero for ax in range(3)]
            d[S - 1][o + r] = [num(float(bc[1 if r == 1 else 3, ax])) if r <= 2 else zero for ax in range(3)]
        Tp = []     # Tp[j][e + 2o - 1] = T_j^e, e = -(2o-1) .. 2o-1
        for j in range(S):
            inv = one / T[j]
            neg, pos = [one], [one]
            for _ in range(m - 1):
                neg.append(neg[-1] * inv)
                pos.append(pos[-1] * T[j])
            Tp.append(neg[:0:-1] + pos)
        off = m - 1

        def qw(j):
            q = [[Qu[a][b] * Tp[j][off + 1 - 2 * o + a % o + b % o] for b in range(m)] for a in range(m)]
            if o >= 2:
                q[1][1] += w
                q[o + 1][o + 1] += w
            return q

        if n > 0 and S > 1:
            Bk = [[[zero] * n for _ in range(n)] for _ in range(S)]      # index k = 1..S-1
            Ck = [None] * S
            yk = [[[zero] * n for _ in range(3)] for _ in range(S)]
            for j in range(S):
                q = qw(j)
                fixed = [a for a in range(m) if d[j][a] is not None]
                for side, k in ((0, j), (o, j + 1)):     # this segment's start belongs to knot j, its end to knot j+1
                    if k < 1 or k > S - 1:
                        continue
                    for r in range(n):
                        row = q[side + 1 + r]
                        for s in range(n):
                            Bk[k][r][s] += row[side + 1 + s]
                        for ax in range(3):
                            acc = zero
                            for a in fixed:
                                acc += row[a] * d[j][a][ax]
                            yk[k][ax][r] -= acc
                if 1 <= j <= S - 2:
                    Ck[j] = [[q[1 + r][o + 1 + s] for s in range(n)] for r in range(n)]     # couples knot j with knot j+1
            # knots 1 .. mk-1 are eliminated left to right, knots S-1 .. mk+1 right to left, and knot mk -- where the two
            # sweeps meet -- takes the Schur carries of both sides (mk = S-1: the plain one-sided sweep)
            mk = S - 1 if meet is None else min(max(int(meet), 1), S - 1)
            W, z = [None] * (S + 1), [None] * (S + 1)

            def carry(Sk, yk_, C, tr):
                """S^-1 [y, C-columns]; C couples towards the next knot of the sweep (tr: use C^T)."""
                cols = [[C[s][r] for r in range(n)] for s in range(n)] if tr else [[C[r][s] for r in range(n)] for s in range(n)]
                sol = spd(Sk, list(yk_) + cols, n)
                return sol[:3], sol[3:]

            Sk = Bk[1]
            for k in range(1, mk):              # forward: row k+1 loses C_k^T S_k^-1 [C_k, y_k]
                z[k], W[k] = carry(Sk, yk[k], Ck[k], False)
                C = Ck[k]
                Sk = [[Bk[k + 1][r][s] - sum(C[q_][r] * W[k][s][q_] for q_ in range(n)) for s in range(n)] for r in range(n)]
                for ax in range(3):
                    for r in range(n):
                        yk[k + 1][ax][r] -= sum(C[q_][r] * z[k][ax][q_] for q_ in range(n))
            Sm = Sk if mk > 1 else Bk[1]
            if mk < S - 1:
                Sk = Bk[S - 1]
                for k in range(S - 1, mk, -1):  # backward: row k-1 loses C_{k-1} S_k^-1 [C_{k-1}^T, y_k]
                    C = Ck[k - 1]
                    z[k], W[k] = carry(Sk, yk[k], C, True)
                    nxt = Sm if k - 1 == mk else Bk[k - 1]
                    Sk = [[nxt[r][s] - sum(C[r][q_] * W[k][s][q_] for q_ in range(n)) for s in range(n)] for r in range(n)]
                    for ax in range(3):
                        for r in range(n):
                            yk[k - 1][ax][r] -= sum(C[r][q_] * z[k][ax][q_] for q_ in range(n))
                Sm = Sk
            x = [None] * (S + 1)
            x[mk] = spd(Sm, list(yk[mk]), n)
            for k in range(mk - 1, 0, -1):
                x[k] = [[z[k][ax][r] - sum(W[k][s][r] * x[k + 1][ax][s] for s in range(n)) for r in range(n)] for ax in range(3)]
            for k in range(mk + 1, S):
                x[k] = [[z[k][ax][r] - sum(W[k][s][r] * x[k - 1][ax][s] for s in range(n)) for r in range(n)] for ax in range(3)]
            for k in range(1, S):
                for r in range(n):
                    v = [x[k][ax][r] for ax in range(3)]
                    d[k - 1][o + 1 + r] = v
                    d[k][1 + r] = v
        out = np.zeros((S, 3, m))
        for j in range(S):
            for ax in range(3):
                sc = [Tp[j][off + a % o] * d[j][a][ax] for a in range(m)]
                for i in range(m - 1):
                    out[j, ax, i] = float(Tp[j][off - (m - 1 - i)] * sum(G[i][a] * sc[a] for a in range(m)))
                out[j, ax, m - 1] = path[j, ax]
    return out


def solve_batch(order, waypoints, times, bc=None, vel_zero_weight=0.0, dps=40):
    """Uniform batch [B,S+1,3] / [B,S]; bc [4,3], [1,4,3] or [B,4,3]; vel_zero_weight scalar or [B].  -> [B,S,3,2o]."""
    waypoints, times = np.asarray(waypoints, dtype=np.float64), np.asarray(times, dtype=np.float64)
    B = times.shape[0]
    bc = np.zeros((1, 4, 3)) if bc is None else np.asarray(bc, dtype=np.float64).reshape(-1, 4, 3)
    vw = np.broadcast_to(np.asarray(vel_zero_weight, dtype=np.float64), (B,))
    return np.stack([solve(order, waypoints[b], times[b], bc[b if bc.shape[0] > 1 else 0], float(vw[b]), dps) for b in range(B)])


# ------------------------------------------------------------------------------------------------------------ the patterns

PATTERNS = {"log16": ("log", 16.0), "alt16": ("alt", 16.0), "ramp16": ("ramp", 16.0), "dist16": ("dist", 16.0),
            "dist256": ("dist", 256.0)}
SPEED = 5.0


def _rng(kind, R, S, seed):
    return np.random.Generator(np.random.Philox(key=[20261019 + int(seed), (int(S) << 20) | (int(R) << 4) | "lard".index(kind[0])]))


def _times(kind, R, B, S, g):
    h = 0.5 * np.log(R)
    if kind in ("log", "dist"):
        return np.exp(g.uniform(-h, h, size=(B, S)))
    if kind == "alt":
        sign = np.where(np.arange(S) % 2 == 0, -1.0, 1.0)                 # every trajectory starts on a short segment
        return np.exp(sign * h)[None, :] * g.uniform(0.9, 1.1, size=(B, S))
    if kind == "ramp":
        e = np.linspace(-0.5, 0.5, S) if S > 1 else np.zeros(1)
        t = np.tile(np.asarray(R) ** e, (B, 1))
        t[1::2] = t[1::2, ::-1]
        return t
    raise ValueError(kind)


def spread_times(kind, R, B, S, seed):
    """Segment times [B,S] of pattern `kind` ('log', 'alt', 'ramp', 'dist') with ratio R."""
    return _times(kind, float(R), B, S, _rng(kind, R, S, seed))


def _walk(B, S, g):
    p0 = g.uniform(-10.0, 10.0, size=(B, 1, 3))
    return np.concatenate([p0, p0 + np.cumsum(g.normal(0.0, 1.0, size=(B, S, 3)), axis=1)], axis=1)


def relay_constant_speed(times, g, speed=SPEED):
    """Waypoints [B,S+1,3] whose leg j has length speed * T_j in a uniformly random direction."""
    B, S = times.shape
    u = g.normal(size=(B, S, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    p0 = g.uniform(-10.0, 10.0, size=(B, 1, 3))
    return np.concatenate([p0, p0 + np.cumsum(u * (speed * times)[..., None], axis=1)], axis=1)


def spread_batch(name, B, S, seed):
    """(waypoints [B,S+1,3], times [B,S]) of the named pattern (PATTERNS): the random walk of tests/synth.py under the
    log / alt / ramp times, constant-speed legs under the dist ones.  Deterministic in (name, S, seed); B <= 8 distinct
    trajectories (the tests tile them over their batches), and row b does not depend on B."""
    kind, R = PATTERNS[name]
    g = _rng(kind, R, S, seed)
    rows = 8
    assert B <= rows, B
    tm = _times(kind, R, rows, S, g)
    wp = relay_constant_speed(tm, g) if kind == "dist" else _walk(rows, S, g)
    return wp[:B], tm[:B]


def spread_loops(name, B, S, seed):
    """Closed loops for the periodic solve: (waypoints [B,S,3] without the closing point, times [B,S]).  Under `dist`
    the closing leg's time is its length / speed, kept inside the range of the other legs' times so that the ratio
    stays at most R (from three segments on: the two legs of a two-segment loop are equally long, and equal times
    would be no spread at all)."""
    kind, R = PATTERNS[name]
    wp, tm = spread_batch(name, B, S, seed + 500)
    wp, tm = wp[:, :S].copy(), tm.copy()
    if kind == "dist" and S > 2:
        close = np.linalg.norm(wp[:, 0] - wp[:, S - 1], axis=1) / SPEED
        tm[:, S - 1] = np.clip(close, tm[:, :S - 1].min(axis=1), tm[:, :S - 1].max(axis=1))
    return wp, tm


def tile(K, B):
    """Index of the distinct trajectory that batch row b carries: K distinct ones tiled over B rows."""
    return np.arange(B) % K


# ------------------------------------------------------- the periodic solve in its free-derivative form, plain fp64


def solve_loop_reduced(order, path, time, vel_zero_weight=0.0):
    """The closed loop the way the periodic kernel poses it, in numpy fp64: the unknowns are the o-1 free derivatives of
    every knot, the block-cyclic system is assembled from Qt(T) by the scaling law and solved by a Cholesky
    factorisation with knot 0 last (the kernel's bordered elimination order), the coefficients recovered per segment.
    "Plain fp64 loops doing the same math": under unequal times this system, once its blocks are summed in fp64, has
    lost digits that the dense KKT in the polynomial coefficients (tests/periodic_ref.py) keeps.
    path [S,3] (no closing point), time [S] -> (coeffs [S,3,2o] highest power first, J, dJ/dT [S])."""
    o = int(order)
    n, m = o - 1, 2 * o
    path, time = np.asarray(path, dtype=np.float64), np.asarray(time, dtype=np.float64)
    S, w = len(time), float(vel_zero_weight)
    G1, Q1 = unit_tables(o)
    G = np.array([[float(v) for v in row] for row in G1])
    Qu = np.array([[float(v) for v in row] for row in Q1])
    da = np.arange(m) % o
    expo = 1 - 2 * o + da[:, None] + da[None, :]
    fs, fe = np.r_[1:o], np.r_[o + 1:m]
    A, y, Qs = np.zeros((S * n, S * n)), np.zeros((S * n, 3)), []
    for j in range(S):
        Q = Qu * time[j] ** expo
        Qs.append(Q.copy())
        Q[1, 1] += w
        Q[o + 1, o + 1] += w
        i0, i1 = np.r_[j * n:(j + 1) * n], np.r_[((j + 1) % S) * n:((j + 1) % S + 1) * n]
        A[np.ix_(i0, i0)] += Q[np.ix_(fs, fs)]
        A[np.ix_(i1, i1)] += Q[np.ix_(fe, fe)]
        A[np.ix_(i0, i1)] += Q[np.ix_(fs, fe)]
        A[np.ix_(i1, i0)] += Q[np.ix_(fe, fs)]
        dP = path[(j + 1) % S] - path[j]          # Qt[., start position] = -Qt[., end position]
        np.add.at(y, i0, -np.outer(Q[fs, o], dP))
        np.add.at(y, i1, -np.outer(Q[fe, o], dP))
    perm = np.r_[n:S * n, 0:n]
    L = np.linalg.cholesky(A[np.ix_(perm, perm)])
    x = np.zeros_like(y)
    x[perm] = np.linalg.solve(L.T, np.linalg.solve(L, y[perm]))
    out, J, g = np.zeros((S, 3, m)), 0.0, np.zeros(S)
    pw = (m - 1 - np.arange(m)).astype(np.float64)
    for j in range(S):
        T = time[j]
        d = np.zeros((m, 3))
        d[o] = path[(j + 1) % S] - path[j]        # positions from the segment's start
        d[fs], d[fe] = x[j * n:(j + 1) * n], x[((j + 1) % S) * n:((j + 1) % S + 1) * n]
        out[j] = ((T ** -pw)[:, None] * (G @ ((T ** da.astype(np.float64))[:, None] * d))).T
        out[j, :, m - 1] = path[j]
        J += np.einsum("ax,ab,bx->", d, Qs[j], d) + w * float(np.sum(d[1] ** 2 + d[o + 1] ** 2))
        g[j] = np.einsum("ax,ab,bx->", d, expo * Qs[j], d) / T
    return out, J, g
