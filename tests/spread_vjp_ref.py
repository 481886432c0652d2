"""Multi-precision reverse mode of the minimum-snap solves: the cost J, dJ/dT and the gradients of
L = <pbar, coeffs> + jbar J with respect to waypoints, times and bc, for one open chain or one closed loop.

TEST INFRASTRUCTURE ONLY.  Independent of the HIP kernels, of the kernels' Python package, of oracle/ and of the fp64 numpy
restatements (tests/vjp_ref.py, tests/cost_vjp_ref.py, tests/periodic_vjp_ref.py): written from the math of DESIGN.md
§11.1 / §12.1 / §15.1 / §18.1, no numpy.linalg.  All arithmetic is mpmath at `dps` digits (40 by default); dps=None runs
the same code in Python floats -- that run is e_cpu64, plain fp64 doing this math.  The unit tables G = M(1)^-1 and Qt(1)
come from tests/spread_ref.unit_tables.

Open chain.  D holds derivative r = 0..o-1 of every knot k = 0..S (slot k o + r); segment j sees d_j = [D of knot j ; D
of knot j+1], its cost is d_j^T Qt^w(T_j) d_j with Qt_ab(T) = Qt_ab(1) T^(1-2o+da+db) (da = a mod o) plus w on the two
velocity diagonals, and its coefficients are p_j = diag(T^-pow) G diag(T^da) d_j.  With K = sum_j P_j^T Qt^w_j P_j the
free slots (derivatives 1..o-1 of the interior knots) solve K_ff D_f = -K_fF D_F: an SPD band system of half-width 2o-3,
ASSEMBLED and eliminated inside the band without pivoting.  The adjoint is one more set of columns of the same
elimination:

    Dbar = sum_j P_j^T M_j^-T pbar_j,   K_ff lam_f = Dbar_f,   dL/dD_F = (Dbar - K lam)_F,
    dL/dT_j = [ sum_a da d_a dbar_a - sum_i pow_i p_i pbar_i - lam_j^T (expo o Qt_j) d_j ] / T_j      (summed over the axes),
    dJ/dD_F = 2 (K D)_F,   dJ/dT_j = d_j^T (expo o Qt_j) d_j / T_j      (the envelope: K_f. D = 0).

Every product Qt d is formed with the positions taken from the segment's own start (Qt annihilates constants), so that
the dps=None run does not lose digits to the offset of the path -- e_cpu64 is a yardstick and should be a careful one.

Closed loop.  tests/periodic_ref.py's KKT system in the monomial coefficients, [2H A^T; A 0] [c; l] = [0; b], is
symmetric, so with cbar = pbar + 2 jbar H c the adjoint is K Y = [cbar; 0] -- three more columns of the elimination
periodic_ref._Num.solve does -- and for a parameter th of the matrix or the right-hand side

    dL/dth = Y^T (dR/dth - dK/dth X) + jbar c^T dH/dth c.

`raw=True` keeps mpmath numbers (numpy object arrays) for checks that need more than a double.
"""
import collections
import contextlib

import numpy as np

from tests import periodic_ref, spread_ref

Adjoint = collections.namedtuple("Adjoint", "coeffs cost cost_grad_times waypoints times bc cost_waypoints cost_times cost_bc")
Adjoint.__doc__ = """coeffs [S,3,2o] (highest power first), cost J, cost_grad_times dJ/dT [S]; waypoints / times / bc: the
gradients of <pbar, coeffs> ([S+1,3] -- [S,3] for a loop --, [S], [4,3]; with a leading axis when pbar has one);
cost_waypoints / cost_times / cost_bc: jbar times the gradients of J.  A loop has no bc: None."""


def _ctx(dps):
    if dps is None:
        return contextlib.nullcontext(), float
    import mpmath
    return mpmath.workdps(int(dps)), mpmath.mpf


def _band_ldl_solve(A, cols, bw):
    """A^-1 [cols] for a symmetric positive definite band matrix (|i - j| <= bw), rows as lists, no pivoting."""
    n = len(A)
    A = [list(r) for r in A]
    cols = [list(c) for c in cols]
    for c in range(n):
        piv = A[c]
        inv = 1 / piv[c]
        hi = min(n, c + bw + 1)
        for r in range(c + 1, hi):
            f = A[r][c] * inv
            if f == 0:
                continue
            row = A[r]
            for k in range(c, hi):
                row[k] -= f * piv[k]
            for col in cols:
                col[r] -= f * col[c]
    for col in cols:
        for r in range(n - 1, -1, -1):
            s = col[r]
            row = A[r]
            for k in range(r + 1, min(n, r + bw + 1)):
                s -= row[k] * col[k]
            col[r] = s / row[r]
    return cols


def _out(x, raw):
    a = np.array(x, dtype=object)
    return a if raw else a.astype(np.float64)


def open_chain(order, path, time, bc=None, w=0.0, pbar=None, jbar=1.0, dps=40, raw=False, origin="segment"):
    """One open-chain trajectory: path [S+1,3], time [S], bc [4,3] (rows start vel, end vel, start acc, end acc; None =
    zeros), w the velocity-zero weight, pbar [S,3,2o] or [k,S,3,2o] (k cotangents at once; None: zeros), jbar a scalar.
    origin: where the positions inside the products Qt d are measured from -- "segment" (the segment's own start, the
    careful form, which is also what the reverse-mode kernel does: it forms its right-hand sides from the legs), "first"
    (the trajectory's first waypoint, as the cost kernel of minsnap_timeopt.hip takes them) or "none" (as they are, the
    four-product form of the forward kernels).  All three are the same numbers at 40 digits; with dps=None the last two
    are plain fp64 doing that math, e_same
    of tests/grad_spread_cases.py.  Returns an Adjoint."""
    o = int(order)
    m, n = 2 * o, o - 1
    path = np.asarray(path, dtype=np.float64)
    time = np.asarray(time, dtype=np.float64)
    S = len(time)
    assert o >= 2 and S >= 1 and path.shape == (S + 1, 3) and origin in ("segment", "first", "none")
    bc = np.zeros((4, 3)) if bc is None else np.asarray(bc, dtype=np.float64).reshape(4, 3)
    pb = np.zeros((S, 3, m)) if pbar is None else np.asarray(pbar, dtype=np.float64)
    stacked = pb.ndim == 4
    pb = pb.reshape(-1, S, 3, m)
    nk = pb.shape[0]
    G1, Q1 = spread_ref.unit_tables(o)
    ctx, num = _ctx(dps)
    with ctx:
        zero, one = num(0), num(1)
        G = [[num(v) for v in row] for row in G1]
        Qu = [[num(v) for v in row] for row in Q1]
        wn, jb = num(float(w)), num(float(jbar))
        T = [num(float(t)) for t in time]
        P = [[num(float(path[k, ax])) for ax in range(3)] for k in range(S + 1)]
        da = [a % o for a in range(m)]
        pw = [m - 1 - i for i in range(m)]
        V = (S + 1) * o
        slot = lambda j, a: (j + a // o) * o + a % o
        Tpow, Qt, Qw = [], [], []
        for j in range(S):
            inv = one / T[j]
            tp = {0: one}
            for e in range(1, m):
                tp[e] = tp[e - 1] * T[j]
                tp[-e] = tp[1 - e] * inv
            Tpow.append(tp)
            q = [[Qu[a][b] * tp[1 - 2 * o + da[a] + da[b]] for b in range(m)] for a in range(m)]
            Qt.append(q)
            qw = [list(r) for r in q]
            qw[1][1] += wn
            qw[o + 1][o + 1] += wn
            Qw.append(qw)
        # the known slots
        D = [[None] * V for _ in range(3)]
        for ax in range(3):
            for k in range(S + 1):
                D[ax][k * o] = P[k][ax]
            for r in range(1, o):
                D[ax][r] = num(float(bc[0 if r == 1 else 2, ax])) if r <= 2 else zero
                D[ax][S * o + r] = num(float(bc[1 if r == 1 else 3, ax])) if r <= 2 else zero
        free = [k * o + r for k in range(1, S) for r in range(1, o)]
        pos = {s: i for i, s in enumerate(free)}
        nf = len(free)

        def local(ax, j, known_only=False):
            """d_j of one axis with the positions taken from the segment's start."""
            d = []
            for a in range(m):
                v = D[ax][slot(j, a)]
                if da[a] == 0:
                    v = v - (P[j][ax] if origin == "segment" else P[0][ax] if origin == "first" else zero)
                elif known_only and slot(j, a) in pos:
                    v = zero
                d.append(v)
            return d

        # dbar_j = M_j^-T pbar_j per cotangent and axis; Dbar its scatter
        Minv = [[[Tpow[j][-pw[i]] * G[i][a] * Tpow[j][da[a]] for a in range(m)] for i in range(m)] for j in range(S)]
        pbn = [[[[num(float(pb[c, j, ax, i])) for i in range(m)] for ax in range(3)] for j in range(S)] for c in range(nk)]
        dbar = [[[[sum((Minv[j][i][a] * pbn[c][j][ax][i] for i in range(m)), zero) for a in range(m)] for ax in range(3)]
                 for j in range(S)] for c in range(nk)]
        Dbar = [[[zero] * V for _ in range(3)] for _ in range(nk)]
        for c in range(nk):
            for j in range(S):
                for ax in range(3):
                    for a in range(m):
                        Dbar[c][ax][slot(j, a)] += dbar[c][j][ax][a]
        lam = [[[zero] * V for _ in range(3)] for _ in range(nk)]
        if nf:
            A = [[zero] * nf for _ in range(nf)]
            rhs = [[zero] * nf for _ in range(3)]
            for j in range(S):
                for a in range(m):
                    ia = pos.get(slot(j, a))
                    if ia is None:
                        continue
                    for b in range(m):
                        ib = pos.get(slot(j, b))
                        if ib is not None:
                            A[ia][ib] += Qw[j][a][b]
                for ax in range(3):
                    d = local(ax, j, known_only=True)
                    for a in range(m):
                        ia = pos.get(slot(j, a))
                        if ia is not None:
                            rhs[ax][ia] -= sum((Qw[j][a][b] * d[b] for b in range(m)), zero)
            cols = rhs + [[Dbar[c][ax][s] for s in free] for c in range(nk) for ax in range(3)]
            sol = _band_ldl_solve(A, cols, 2 * n - 1)
            for ax in range(3):
                for s, v in zip(free, sol[ax]):
                    D[ax][s] = v
            for c in range(nk):
                for ax in range(3):
                    for s, v in zip(free, sol[3 + 3 * c + ax]):
                        lam[c][ax][s] = v
        # coefficients, cost, K D, K lam, the time gradients
        coeffs = [[[None] * m for _ in range(3)] for _ in range(S)]
        J = zero
        gJ = [zero] * S
        KD = [[zero] * V for _ in range(3)]
        Klam = [[[zero] * V for _ in range(3)] for _ in range(nk)]
        gT = [[zero] * S for _ in range(nk)]
        for j in range(S):
            expoQ = [[(1 - 2 * o + da[a] + da[b]) * Qt[j][a][b] for b in range(m)] for a in range(m)]
            for ax in range(3):
                d = local(ax, j)
                full = [D[ax][slot(j, a)] for a in range(m)]
                for i in range(m):
                    coeffs[j][ax][i] = sum((Minv[j][i][a] * full[a] for a in range(m)), zero)
                qd = [sum((Qw[j][a][b] * d[b] for b in range(m)), zero) for a in range(m)]
                ed = [sum((expoQ[a][b] * d[b] for b in range(m)), zero) for a in range(m)]
                J += sum((d[a] * qd[a] for a in range(m)), zero)
                gJ[j] += sum((d[a] * ed[a] for a in range(m)), zero)
                for a in range(m):
                    KD[ax][slot(j, a)] += qd[a]
                for c in range(nk):
                    lj = [lam[c][ax][slot(j, a)] for a in range(m)]
                    for a in range(m):
                        Klam[c][ax][slot(j, a)] += sum((Qw[j][a][b] * lj[b] for b in range(m)), zero)
                    t = sum((da[a] * full[a] * dbar[c][j][ax][a] for a in range(m)), zero)
                    t -= sum((pw[i] * coeffs[j][ax][i] * pbn[c][j][ax][i] for i in range(m)), zero)
                    t -= sum((lj[a] * ed[a] for a in range(m)), zero)
                    gT[c][j] += t
            gJ[j] = gJ[j] / T[j]
            for c in range(nk):
                gT[c][j] = gT[c][j] / T[j]
            for ax in range(3):
                coeffs[j][ax][m - 1] = P[j][ax]      # p_j(0) = P_j exactly

        def fixed_part(F):
            """(waypoints [S+1,3], bc [4,3]) of a field over the slots."""
            gw = [[F[ax][k * o] for ax in range(3)] for k in range(S + 1)]
            gb = [[zero] * 3 for _ in range(4)]
            for ax in range(3):
                gb[0][ax], gb[1][ax] = F[ax][1], F[ax][S * o + 1]
                if o >= 3:
                    gb[2][ax], gb[3][ax] = F[ax][2], F[ax][S * o + 2]
            return gw, gb

        Lw, Lb = [], []
        for c in range(nk):
            gw, gb = fixed_part([[Dbar[c][ax][s] - Klam[c][ax][s] for s in range(V)] for ax in range(3)])
            Lw.append(gw)
            Lb.append(gb)
        Jw, Jbc = fixed_part([[2 * jb * KD[ax][s] for s in range(V)] for ax in range(3)])
        Jt = [jb * g for g in gJ]
        if not stacked:
            Lw, Lb, gT = Lw[0], Lb[0], gT[0]
        res = Adjoint(_out(coeffs, raw), J if raw else float(J), _out(gJ, raw), _out(Lw, raw), _out(gT, raw), _out(Lb, raw),
                      _out(Jw, raw), _out(Jt, raw), _out(Jbc, raw))
    return res


# ------------------------------------------------------------------------------------------------------------ closed loops


def _pivot_solve(rows, n, nr):
    """Gaussian elimination with partial pivoting on augmented rows (lists of n + nr scalars), zeros skipped; returns the
    nr solution columns.  The same code for Python floats and mpmath numbers."""
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
    X = []
    for a in range(nr):
        x = [None] * n
        for r in range(n - 1, -1, -1):
            rr = rows[r]
            s = rr[n + a]
            for k in range(r + 1, n):
                if rr[k] != 0:
                    s -= rr[k] * x[k]
            x[r] = s / rr[r]
        X.append(x)
    return X


def loop(order, path, time, w=0.0, pbar=None, jbar=1.0, dps=40, raw=False):
    """One closed loop: path [S,3] (no closing point), time [S], pbar [S,3,2o] or [k,S,3,2o], jbar a scalar.  Returns an
    Adjoint (bc and cost_bc None).  The coefficients, J and dJ/dT are periodic_ref.solve's, recomputed here because the
    multipliers are needed; the J part comes from the envelope (dJ/db = -l, dJ/dT as in periodic_ref), the pbar part
    from the transposed solve."""
    o = int(order)
    m = 2 * o
    path = np.asarray(path, dtype=np.float64)
    time = np.asarray(time, dtype=np.float64)
    S = len(time)
    assert o >= 2 and S >= 1 and path.shape == (S, 3)
    pb = np.zeros((S, 3, m)) if pbar is None else np.asarray(pbar, dtype=np.float64)
    stacked = pb.ndim == 4
    pb = pb.reshape(-1, S, 3, m)
    nk = pb.shape[0]
    fall = periodic_ref._fall
    ctx, num = _ctx(dps)
    with ctx:
        nm = periodic_ref._Num(dps)
        zero = num(0)
        jb, wn = num(float(jbar)), num(float(w))
        # positions from the first waypoint (J, the derivatives and every gradient but the constant terms' are
        # translation invariant; the constant terms are the waypoints themselves)
        P = [[num(float(path[j, ax])) - num(float(path[0, ax])) for ax in range(3)] for j in range(S)]
        T = [num(float(t)) for t in time]
        K, R = periodic_ref._kkt(o, P, T, wn, nm)
        n, nc = S * m, S * (o + 1)
        N = n + nc
        rows = [[num(K[a, b]) if K[a, b] != 0 else zero for b in range(N)] + [num(R[a, ax]) for ax in range(3)] for a in range(N)]
        for c in range(nk):
            for ax in range(3):
                for j in range(S):
                    for i in range(m):
                        rows[j * m + i].append(num(float(pb[c, j, ax, m - 1 - i])))
                for a in range(n, N):
                    rows[a].append(zero)
        sol = _pivot_solve(rows, N, 3 + 3 * nk)
        X, Y = sol[:3], [sol[3 + 3 * c:6 + 3 * c] for c in range(nk)]

        def deriv(cc, k, t):
            return sum((fall(i, k) * cc[i] * t ** (i - k) for i in range(k, m)), zero)

        J = zero
        gJ = [zero] * S
        gT = [[zero] * S for _ in range(nk)]
        Jw = [[zero] * 3 for _ in range(S)]
        Lw = [[[zero] * 3 for _ in range(S)] for _ in range(nk)]
        coeffs = [[[None] * m for _ in range(3)] for _ in range(S)]
        for j in range(S):
            base, q0, nx = j * m, n + j * (o + 1), (j + 1) % S
            Tj = T[j]
            # d/dT_j of the KKT matrix, upper triangle plus constraint rows, as (row, column, value) with row != column
            # entries standing for both (a, b) and (b, a)
            dK = []
            for i in range(o, m):
                for k in range(o, m):
                    e = i + k - 2 * o + 1
                    dK.append((base + i, base + k, 2 * fall(i, o) * fall(k, o) * Tj ** (e - 1), False))
            if w != 0:
                for i in range(1, m):
                    for k in range(1, m):
                        if i + k > 2:
                            dK.append((base + i, base + k, 2 * wn * i * k * (i + k - 2) * Tj ** (i + k - 3), False))
            for i in range(1, m):
                dK.append((q0 + 1, base + i, i * Tj ** (i - 1), True))
            for r in range(1, o):
                for i in range(r + 1, m):
                    dK.append((q0 + 1 + r, base + i, fall(i, r) * (i - r) * Tj ** (i - r - 1), True))
            for ax in range(3):
                x = X[ax]
                cc = [x[base + i] for i in range(m)]
                for i in range(m):
                    coeffs[j][ax][m - 1 - i] = cc[i]
                coeffs[j][ax][m - 1] = num(float(path[j, ax]))
                for i in range(o, m):
                    for k in range(o, m):
                        e = i + k - 2 * o + 1
                        J += fall(i, o) * fall(k, o) * Tj ** e / e * cc[i] * cc[k]
                vT = deriv(cc, 1, Tj)
                J += wn * (cc[1] * cc[1] + vT * vT)
                po = deriv(cc, o, Tj)
                g = po * po + 2 * wn * vT * deriv(cc, 2, Tj)
                for r in range(o):
                    g += x[q0 + 1 + r] * deriv(cc, r + 1, Tj)
                gJ[j] += g
                # dJ/db = -l on the two position rows that carry waypoint j: p_j(0) = P_j and p_{j-1}(T) = P_j
                Jw[j][ax] -= x[q0]
                Jw[nx][ax] -= x[q0 + 1]
                for c in range(nk):
                    y = Y[c][ax]
                    Lw[c][j][ax] += y[q0]
                    Lw[c][nx][ax] += y[q0 + 1]
                    t = zero
                    for a, b, v, both in dK:
                        t += y[a] * v * x[b]
                        if both:
                            t += y[b] * v * x[a]
                    gT[c][j] -= t
        Jw = [[jb * v for v in r] for r in Jw]
        Jt = [jb * g for g in gJ]
        if not stacked:
            Lw, gT = Lw[0], gT[0]
        res = Adjoint(_out(coeffs, raw), J if raw else float(J), _out(gJ, raw), _out(Lw, raw), _out(gT, raw), None,
                      _out(Jw, raw), _out(Jt, raw), None)
    return res
