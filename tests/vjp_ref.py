"""Dense numpy restatement of the solve's reverse mode, one trajectory at a time.

TEST INFRASTRUCTURE ONLY.  Independent of the HIP kernel: M(T) and Q(T) are built from monomials
(oracle/numpy_ref.py, the reference's construction), Qt = M^-T Q M^-1 by dense inverses, the global
matrix K = sum_j P_j^T Qt^w_j P_j assembled densely and the free block solved with numpy.linalg.solve.
"""
import numpy as np

from oracle.numpy_ref import build_M, build_Q


def _seg_tables(o, T, w):
    M = build_M(o, np.array([T]))
    Minv = np.linalg.inv(M)
    Qt = Minv.T @ build_Q(o, np.array([T])) @ Minv
    Qt = 0.5 * (Qt + Qt.T)
    Qw = Qt.copy()
    Qw[1, 1] += w
    Qw[o + 1, o + 1] += w
    return M, Minv, Qt, Qw


def adjoint(order, path, time, bc, pbar, w=0.0):
    """path [S+1,3], time [S], bc [4,3] (rows v0, v1, a0, a1), pbar [S,3,2o] = dL/dcoeffs.
    Returns dict(coeffs [S,3,2o], waypoints [S+1,3], times [S], bc [4,3])."""
    o = int(order)
    m = 2 * o
    path = np.asarray(path, dtype=np.float64)
    T = np.asarray(time, dtype=np.float64)
    bc = np.asarray(bc, dtype=np.float64).reshape(4, 3)
    pbar = np.asarray(pbar, dtype=np.float64).reshape(len(T), 3, m)
    S = len(T)
    V = (S + 1) * o                       # global slots: waypoint k, derivative r -> k*o + r
    seg = [np.r_[j * o:(j + 1) * o, (j + 1) * o:(j + 2) * o] for j in range(S)]
    tabs = [_seg_tables(o, T[j], w) for j in range(S)]
    K = np.zeros((V, V))
    for j in range(S):
        K[np.ix_(seg[j], seg[j])] += tabs[j][3]
    free = np.array([k * o + r for k in range(1, S) for r in range(1, o)], dtype=int)
    fixed = np.setdiff1d(np.arange(V), free)
    D = np.zeros((V, 3))                  # fixed values: positions, bc vel/acc at the ends, zeros above
    for k in range(S + 1):
        D[k * o] = path[k]
    if o >= 2:
        D[1], D[S * o + 1] = bc[0], bc[1]
    if o >= 3:
        D[2], D[S * o + 2] = bc[2], bc[3]
    if len(free):
        D[free] = -np.linalg.solve(K[np.ix_(free, free)], K[np.ix_(free, fixed)] @ D[fixed])
    coeffs = np.zeros((S, 3, m))
    Dbar = np.zeros((V, 3))
    dbar_seg = []
    for j in range(S):
        Minv = tabs[j][1]
        coeffs[j] = (Minv @ D[seg[j]]).T
        db = Minv.T @ pbar[j].T            # [m,3]
        dbar_seg.append(db)
        Dbar[seg[j]] += db
    lam = np.zeros((V, 3))
    if len(free):
        lam[free] = np.linalg.solve(K[np.ix_(free, free)], Dbar[free])
    G = Dbar - K @ lam                     # valid at the fixed slots
    deriv = np.array([a % o for a in range(m)], dtype=np.float64)
    pw = np.array([m - 1 - i for i in range(m)], dtype=np.float64)
    expo = 1 - 2 * o + deriv[:, None] + deriv[None, :]
    gt = np.zeros(S)
    for j in range(S):
        d, lt, Qt = D[seg[j]], lam[seg[j]], tabs[j][2]
        t = np.sum(deriv[:, None] * d * dbar_seg[j]) - np.sum(pw[None, :] * coeffs[j] * pbar[j])
        t -= np.einsum("ax,ab,bx->", lt, expo * Qt, d)
        gt[j] = t / T[j]
    gwp = np.stack([G[k * o] for k in range(S + 1)])
    gbc = np.zeros((4, 3))
    if o >= 2:
        gbc[0], gbc[1] = G[1], G[S * o + 1]
    if o >= 3:
        gbc[2], gbc[3] = G[2], G[S * o + 2]
    return dict(coeffs=coeffs, waypoints=gwp, times=gt, bc=gbc)


def adjoint_batch(order, waypoints, times, bc, pbar, w=0.0, seg_offsets=None):
    """Batched wrapper: uniform [B,S+1,3] / [B,S] / pbar [B,S,3,2o], or ragged (concatenated, seg_offsets [B+1]).
    bc [1 or B,4,3]; w scalar or [B].  Returns (gwp, gt, gbc_per_traj [B,4,3]) in the input layouts."""
    m = 2 * order
    if seg_offsets is None:
        B, S = np.asarray(times).shape
        seg_offsets = np.arange(B + 1) * S
        waypoints = np.asarray(waypoints).reshape(-1, 3)
        times = np.asarray(times).reshape(-1)
        pbar = np.asarray(pbar).reshape(-1, 3, m)
        uniform = (B, S)
    else:
        uniform = None
    seg_offsets = np.asarray(seg_offsets)
    B = len(seg_offsets) - 1
    bc = np.asarray(bc, dtype=np.float64).reshape(-1, 4, 3)
    wv = np.broadcast_to(np.asarray(w, dtype=np.float64), (B,))
    gwp = np.zeros((len(waypoints), 3))
    gt = np.zeros(len(times))
    gbc = np.zeros((B, 4, 3))
    for b in range(B):
        s0, s1 = int(seg_offsets[b]), int(seg_offsets[b + 1])
        if s1 == s0:
            continue
        r = adjoint(order, waypoints[s0 + b:s1 + b + 1], times[s0:s1], bc[b if bc.shape[0] > 1 else 0], pbar[s0:s1], wv[b])
        gwp[s0 + b:s1 + b + 1] = r["waypoints"]
        gt[s0:s1] = r["times"]
        gbc[b] = r["bc"]
    if uniform is not None:
        B, S = uniform
        return gwp.reshape(B, S + 1, 3), gt.reshape(B, S), gbc
    return gwp, gt, gbc


def oracle_directional(oracle_mod, order, path, time, bc, pbar, w=0.0):
    """Directional derivatives of L = <pbar, coeffs> from the 80-bit oracle, along every coordinate.
    Waypoints and bc enter linearly: a central difference with step 1 is exact up to rounding.  Times: central
    differences at h_j = 1e-3 T_j and h_j / 2, Richardson-extrapolated (error O(h^4)).
    Returns (d/dwaypoints [S+1,3], d/dbc [4,3], d/dtimes [S])."""
    path, time = np.asarray(path, dtype=np.float64), np.asarray(time, dtype=np.float64)
    bc = np.asarray(bc, dtype=np.float64).reshape(4, 3)
    S = len(time)

    def loss(wp, tm, bcs):
        c, _ = oracle_mod.solve_batch(order, wp, tm, bcs, vel_zero_weight=w, long_double=True)
        return np.einsum("nsxi,sxi->n", c, pbar)
    n_wp = (S + 1) * 3
    E = np.eye(n_wp + 12)
    wp = np.concatenate([path[None] + E[:, :n_wp].reshape(-1, S + 1, 3), path[None] - E[:, :n_wp].reshape(-1, S + 1, 3)])
    bcs = np.concatenate([bc[None] + E[:, n_wp:].reshape(-1, 4, 3), bc[None] - E[:, n_wp:].reshape(-1, 4, 3)])
    L = loss(wp, np.repeat(time[None], len(wp), 0), bcs)
    fd = 0.5 * (L[:len(E)] - L[len(E):])
    h = 1e-3 * time
    tms = np.concatenate([time[None] + sgn * f * np.diag(h) for f in (1.0, 0.5) for sgn in (1, -1)])
    L = loss(np.repeat(path[None], len(tms), 0), tms, np.repeat(bc[None], len(tms), 0)).reshape(4, S)
    d1 = (L[0] - L[1]) / (2 * h)
    d2 = (L[2] - L[3]) / h
    return fd[:n_wp].reshape(S + 1, 3), fd[n_wp:].reshape(4, 3), (4 * d2 - d1) / 3


def rel_err_rows(got, ref):
    """Per-row (trajectory) max-abs error over max-abs reference; max over rows."""
    got = np.asarray(got, dtype=np.float64).reshape(np.asarray(ref).shape[0], -1)
    ref = np.asarray(ref, dtype=np.float64).reshape(got.shape)
    den = np.max(np.abs(ref), axis=1)
    den[den == 0] = 1.0
    return float(np.max(np.max(np.abs(got - ref), axis=1) / den))
