"""Dense numpy restatement of the open-chain solve's reverse mode with a cotangent of the snap cost, one
trajectory at a time.

TEST INFRASTRUCTURE ONLY.  Independent of the HIP kernel: the p_bar part is tests/vjp_ref.adjoint, the J_bar part is
2 (K d) at the fixed slots over the dense tables of tests/timeopt_ref.py and its envelope gradient cost_grad.
"""
import numpy as np

from oracle.numpy_ref import build_M, build_Q
from tests.timeopt_ref import cost_from_coeffs, cost_grad, endpoint_derivatives
from tests.vjp_ref import adjoint


def cost_adjoint(order, path, time, bc, w=0.0):
    """Gradients of J alone.  Returns dict(cost, waypoints [S+1,3], times [S], bc [4,3])."""
    o = int(order)
    T = np.asarray(time, dtype=np.float64)
    S = len(T)
    d, tabs = endpoint_derivatives(o, path, T, bc, w)
    J, gt = cost_grad(o, path, T, bc, w)
    gwp, gbc = np.zeros((S + 1, 3)), np.zeros((4, 3))
    for j in range(S):
        dj = d[j].copy()
        dj[[0, o]] -= dj[0]               # Qt annihilates constants; the w diagonal sits on velocities only
        q = 2.0 * tabs[j][3] @ dj         # 2 Qt^w_j d_j, [2o,3]
        gwp[j] += q[0]
        gwp[j + 1] += q[o]
        if j == 0:
            gbc[0] = q[1]
            if o >= 3:
                gbc[2] = q[2]
        if j == S - 1:
            gbc[1] = q[o + 1]
            if o >= 3:
                gbc[3] = q[o + 2]
    return dict(cost=J, waypoints=gwp, times=gt, bc=gbc)


def cost_vjp(order, path, time, bc, pbar, jbar, w=0.0):
    """Gradients of L = <pbar, coeffs> + jbar * J; pbar may be None.  Returns dict(waypoints, times, bc)."""
    cj = cost_adjoint(order, path, time, bc, w)
    out = {k: float(jbar) * cj[k] for k in ("waypoints", "times", "bc")}
    if pbar is not None:
        r = adjoint(order, path, time, bc, pbar, w)
        for k in out:
            out[k] = out[k] + r[k]
    return out


def cost_coeff_cotangent(order, coeffs, time, w=0.0):
    """J written over the monomial coefficients, J = sum c^T (Q + w V) c: returns (p_bar = dJ/dcoeffs = 2 (Q + w V) c
    [S,3,2o], the explicit time derivative at fixed coefficients p^(o)(T)^2 + 2 w v(T) a(T) summed over the axes [S])."""
    o = int(order)
    coeffs = np.asarray(coeffs, dtype=np.float64)
    pbar, explicit = np.zeros_like(coeffs), np.zeros(len(time))
    for j, T in enumerate(np.asarray(time, dtype=np.float64)):
        M = build_M(o, np.array([T]))
        V = np.outer(M[1], M[1]) + np.outer(M[o + 1], M[o + 1])    # v(0)^2 + v(T)^2 in coefficient space
        QV = build_Q(o, np.array([T])) + w * V
        for ax in range(3):
            c = coeffs[j, ax]
            pbar[j, ax] = 2.0 * QV @ c
            explicit[j] += (np.polyval(np.polyder(c, o), T) ** 2
                            + 2.0 * w * np.polyval(np.polyder(c, 1), T) * np.polyval(np.polyder(c, 2), T))
    return pbar, explicit


def cost_vjp_batch(order, waypoints, times, bc, pbar, jbar, w=0.0, seg_offsets=None):
    """Batched wrapper in the layouts of tests/vjp_ref.adjoint_batch: uniform [B,S+1,3] / [B,S] / pbar [B,S,3,2o] (or None),
    or ragged (concatenated, seg_offsets [B+1]).  bc [1 or B,4,3]; jbar [B]; w scalar or [B].  An empty trajectory gets zeros.
    Returns (gwp, gt, gbc_per_traj [B,4,3])."""
    m = 2 * order
    uniform = None
    if seg_offsets is None:
        B, S = np.asarray(times).shape
        uniform = (B, S)
        seg_offsets = np.arange(B + 1) * S
        waypoints = np.asarray(waypoints).reshape(-1, 3)
        times = np.asarray(times).reshape(-1)
    if pbar is not None:
        pbar = np.asarray(pbar, dtype=np.float64).reshape(-1, 3, m)
    seg_offsets = np.asarray(seg_offsets)
    B = len(seg_offsets) - 1
    bc = np.asarray(bc, dtype=np.float64).reshape(-1, 4, 3)
    wv = np.broadcast_to(np.asarray(w, dtype=np.float64), (B,))
    jbar = np.broadcast_to(np.asarray(jbar, dtype=np.float64), (B,))
    gwp, gt, gbc = np.zeros((len(waypoints), 3)), np.zeros(len(times)), np.zeros((B, 4, 3))
    for b in range(B):
        s0, s1 = int(seg_offsets[b]), int(seg_offsets[b + 1])
        if s1 == s0:
            continue
        r = cost_vjp(order, waypoints[s0 + b:s1 + b + 1], times[s0:s1], bc[b if bc.shape[0] > 1 else 0],
                     None if pbar is None else pbar[s0:s1], jbar[b], wv[b])
        gwp[s0 + b:s1 + b + 1], gt[s0:s1], gbc[b] = r["waypoints"], r["times"], r["bc"]
    if uniform is not None:
        return gwp.reshape(uniform[0], uniform[1] + 1, 3), gt.reshape(uniform), gbc
    return gwp, gt, gbc


def oracle_cost(oracle_mod, order, wp, tm, bcs, w):
    """J of every trajectory of a uniform batch from the 80-bit oracle's coefficients (exact polynomial integration)."""
    c, _ = oracle_mod.solve_batch(order, wp, tm, bcs, vel_zero_weight=w, long_double=True)
    return np.array([cost_from_coeffs(order, c[n], tm[n], w) for n in range(len(c))])


def oracle_cost_directional(oracle_mod, order, path, time, bc, w=0.0):
    """Derivatives of the oracle's J along every coordinate.  J is quadratic in (waypoints, bc): a central difference
    with step 1 is exact up to rounding.  Times: central differences at h_j = 1e-3 T_j and h_j / 2, Richardson-extrapolated.
    J does not depend on a translation, so the path is centred first (less cancellation in the differences).
    Returns (d/dwaypoints [S+1,3], d/dbc [4,3], d/dtimes [S])."""
    path, time = np.asarray(path, dtype=np.float64), np.asarray(time, dtype=np.float64)
    path = path - path[0]
    bc = np.asarray(bc, dtype=np.float64).reshape(4, 3)
    S = len(time)
    n_wp = (S + 1) * 3
    E = np.eye(n_wp + 12)
    wp = np.concatenate([path[None] + E[:, :n_wp].reshape(-1, S + 1, 3), path[None] - E[:, :n_wp].reshape(-1, S + 1, 3)])
    bcs = np.concatenate([bc[None] + E[:, n_wp:].reshape(-1, 4, 3), bc[None] - E[:, n_wp:].reshape(-1, 4, 3)])
    Jv = oracle_cost(oracle_mod, order, wp, np.repeat(time[None], len(wp), 0), bcs, w)
    fd = 0.5 * (Jv[:len(E)] - Jv[len(E):])
    h = 1e-3 * time
    tms = np.concatenate([time[None] + sgn * f * np.diag(h) for f in (1.0, 0.5) for sgn in (1, -1)])
    Jt = oracle_cost(oracle_mod, order, np.repeat(path[None], len(tms), 0), tms, np.repeat(bc[None], len(tms), 0), w).reshape(4, S)
    d1 = (Jt[0] - Jt[1]) / (2 * h)
    d2 = (Jt[2] - Jt[3]) / h
    return fd[:n_wp].reshape(S + 1, 3), fd[n_wp:].reshape(4, 3), (4 * d2 - d1) / 3
