"""Dense numpy restatement of the periodic solve's reverse mode, one loop at a time.

TEST INFRASTRUCTURE ONLY.  Independent of the HIP kernel: the per-segment tables come from tests/vjp_ref._seg_tables
(M and Q from monomials, Qt = M^-T Q M^-1 by dense inverses), the global matrix K = sum_j P_j^T Qt^w_j P_j is assembled
with cyclic selection matrices (knot k, derivative r -> slot k*o + r; segment j ends at knot (j+1) mod S) and the free
block is solved with numpy.linalg.solve.  `directional` differentiates tests/periodic_ref.solve -- the KKT system in
the monomial coefficients, in mpmath -- and shares nothing with the adjoint but the problem statement.
"""
import numpy as np

from tests import periodic_ref
from tests.vjp_ref import _seg_tables


def _select(o, S, j):
    """P_j [2o, S*o]: segment j's endpoint slots out of the loop's."""
    P = np.zeros((2 * o, S * o))
    for r in range(o):
        P[r, j * o + r] = 1.0
        P[o + r, ((j + 1) % S) * o + r] = 1.0
    return P


def adjoint(order, path, time, pbar, jbar=0.0, w=0.0):
    """path [S,3] (no closing point), time [S], pbar [S,3,2o] = dL/dcoeffs, jbar = dL/dcost.
    Returns dict(coeffs [S,3,2o], cost, waypoints [S,3], times [S])."""
    o = int(order)
    m = 2 * o
    path = np.asarray(path, dtype=np.float64)
    T = np.asarray(time, dtype=np.float64)
    S = len(T)
    pbar = np.asarray(pbar, dtype=np.float64).reshape(S, 3, m)
    V = S * o
    sel = [_select(o, S, j) for j in range(S)]
    tabs = [_seg_tables(o, T[j], w) for j in range(S)]
    K = np.zeros((V, V))
    for j in range(S):
        K += sel[j].T @ tabs[j][3] @ sel[j]
    pos = np.arange(S) * o
    free = np.setdiff1d(np.arange(V), pos)
    # positions from the first waypoint, as the kernel and periodic_ref measure them (K annihilates a translation)
    D = np.zeros((V, 3))
    D[pos] = path - path[0]
    D[free] = -np.linalg.solve(K[np.ix_(free, free)], K[np.ix_(free, pos)] @ D[pos])
    cost = float(np.sum(D * (K @ D)))
    coeffs = np.zeros((S, 3, m))
    Dbar = np.zeros((V, 3))
    dbar_seg = []
    for j in range(S):
        Minv = tabs[j][1]
        coeffs[j] = (Minv @ (sel[j] @ D)).T
        db = Minv.T @ pbar[j].T            # [m,3]
        dbar_seg.append(db)
        Dbar += sel[j].T @ db
    lam = np.zeros((V, 3))
    lam[free] = np.linalg.solve(K[np.ix_(free, free)], Dbar[free])
    G = Dbar - K @ lam + 2.0 * jbar * (K @ D)      # valid at the position slots
    deriv = np.array([a % o for a in range(m)], dtype=np.float64)
    pw = np.array([m - 1 - i for i in range(m)], dtype=np.float64)
    expo = 1 - 2 * o + deriv[:, None] + deriv[None, :]
    gt = np.zeros(S)
    for j in range(S):
        d, lt, Qt = sel[j] @ D, sel[j] @ lam, tabs[j][2]
        t = np.sum(deriv[:, None] * d * dbar_seg[j]) - np.sum(pw[None, :] * coeffs[j] * pbar[j])
        t -= np.einsum("ax,ab,bx->", lt, expo * Qt, d)
        t += jbar * np.einsum("ax,ab,bx->", d, expo * Qt, d)
        gt[j] = t / T[j]
    coeffs[:, :, m - 1] = path            # p_j(0) = P_j, copied through
    return dict(coeffs=coeffs, cost=cost, waypoints=G[pos], times=gt)


def adjoint_batch(order, waypoints, times, pbar, jbar=None, w=0.0, seg_offsets=None):
    """Batched wrapper: uniform [B,S,3] / [B,S] / pbar [B,S,3,2o], or ragged (waypoints, times and pbar concatenated, all
    split by seg_offsets [B+1]; an empty loop contributes nothing).  jbar None or [B]; w scalar or [B].
    Returns (gwp, gt) in the input layouts."""
    m = 2 * order
    if seg_offsets is None:
        B, S = np.asarray(times).shape
        seg_offsets = np.arange(B + 1) * S
        uniform = (B, S)
    else:
        uniform = None
    waypoints = np.asarray(waypoints, dtype=np.float64).reshape(-1, 3)
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    pbar = np.asarray(pbar, dtype=np.float64).reshape(-1, 3, m)
    seg_offsets = np.asarray(seg_offsets)
    B = len(seg_offsets) - 1
    wv = np.broadcast_to(np.asarray(w, dtype=np.float64), (B,))
    jv = np.zeros(B) if jbar is None else np.broadcast_to(np.asarray(jbar, dtype=np.float64), (B,))
    gwp = np.zeros((len(waypoints), 3))
    gt = np.zeros(len(times))
    for b in range(B):
        s0, s1 = int(seg_offsets[b]), int(seg_offsets[b + 1])
        if s1 == s0:
            continue
        r = adjoint(order, waypoints[s0:s1], times[s0:s1], pbar[s0:s1], jv[b], wv[b])
        gwp[s0:s1] = r["waypoints"]
        gt[s0:s1] = r["times"]
    if uniform is not None:
        B, S = uniform
        return gwp.reshape(B, S, 3), gt.reshape(B, S)
    return gwp, gt


def directional_parts(order, path, time, pbar, w=0.0, dps=30):
    """Directional derivatives of <pbar, coeffs> and of J from periodic_ref.solve along every coordinate, at `dps` mpmath
    digits (None = numpy fp64).  Both are at most quadratic in the waypoints: a central difference with step 1 is exact
    up to rounding.  Times: central differences at h_j = 1e-3 T_j and h_j / 2, Richardson-extrapolated (error O(h^4)).
    Returns dict(wp_p [S,3], wp_J [S,3], t_p [S], t_J [S])."""
    path, time = np.asarray(path, dtype=np.float64), np.asarray(time, dtype=np.float64)
    S = len(time)
    pbar = np.asarray(pbar, dtype=np.float64).reshape(S, 3, 2 * order)

    def diff(p1, t1, p0, t0):
        # differenced coefficient by coefficient: what does not move (the constant coefficients along a time) cancels exactly
        c1, J1, _ = periodic_ref.solve(order, p1, t1, w, dps)
        c0, J0, _ = periodic_ref.solve(order, p0, t0, w, dps)
        return np.array([float(np.sum((c1 - c0) * pbar)), J1 - J0])
    gwp = np.zeros((S, 3, 2))
    for k in range(S):
        for ax in range(3):
            e = np.zeros((S, 3))
            e[k, ax] = 1.0
            gwp[k, ax] = 0.5 * diff(path + e, time, path - e, time)
    gt = np.zeros((S, 2))
    for j in range(S):
        h = 1e-3 * time[j]
        e = np.zeros(S)
        e[j] = h
        d1 = diff(path, time + e, path, time - e) / (2 * h)
        d2 = diff(path, time + 0.5 * e, path, time - 0.5 * e) / h
        gt[j] = (4 * d2 - d1) / 3
    return dict(wp_p=gwp[..., 0], wp_J=gwp[..., 1], t_p=gt[:, 0], t_J=gt[:, 1])


def directional(order, path, time, pbar, jbar=0.0, w=0.0, dps=30):
    """Directional derivatives of L = <pbar, coeffs> + jbar * J: (d/dwaypoints [S,3], d/dtimes [S])."""
    d = directional_parts(order, path, time, pbar, w, dps)
    return d["wp_p"] + jbar * d["wp_J"], d["t_p"] + jbar * d["t_J"]


# ---- recorded 30-digit derivatives (tests/golden/periodic_vjp_dir30.json) ----
# The 30-digit KKT solves take up to half a minute per loop (order 5, S = 3): they are recorded once,
#     python -m tests.periodic_vjp_ref
# and the tests read the record; tests/test_periodic_vjp_math.py recomputes the cheapest loops and compares.

GOLDEN = "periodic_vjp_dir30.json"
GOLDEN_ORDERS, GOLDEN_S, GOLDEN_W = (2, 3, 4, 5), (1, 2, 3), (0.0, 0.3)


def golden_inputs(order, S):
    """The recorded loops: (path [S,3], time [S], pbar [S,3,2o])."""
    from tests import synth
    wp, tm = synth.make_batch(1, S, config_id=3, offset=10 * order + S)
    pbar = np.random.default_rng(order * 7 + S).normal(size=(S, 3, 2 * order))
    return wp[0][:S].copy(), tm[0].copy(), pbar


def golden_cases():
    """Every recorded case as dict(order, S, w, path, time, pbar, wp_p, wp_J, t_p, t_J) of float64 arrays."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)) as f:
        rows = json.load(f)["cases"]
    keys = ("path", "time", "pbar", "wp_p", "wp_J", "t_p", "t_J")
    return [dict(c, **{k: np.array([float.fromhex(x) for x in c[k]]).reshape(c[k + "_shape"]) for k in keys}) for c in rows]


def _record():
    import json
    import os
    rows = []
    for order in GOLDEN_ORDERS:
        for S in GOLDEN_S:
            path, time, pbar = golden_inputs(order, S)
            for w in GOLDEN_W:
                c = dict(order=order, S=S, w=w, path=path, time=time, pbar=pbar, **directional_parts(order, path, time, pbar, w, 30))
                row = dict(order=order, S=S, w=w)
                for k, v in c.items():
                    if isinstance(v, np.ndarray):
                        row[k] = [float(x).hex() for x in v.ravel()]
                        row[k + "_shape"] = list(v.shape)
                rows.append(row)
                print(order, S, w, flush=True)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)
    with open(out, "w") as f:
        json.dump(dict(what="30-digit directional derivatives of tests/periodic_ref.solve (tests/periodic_vjp_ref.py)",
                       dps=30, cases=rows), f, indent=0)
    print(out)


if __name__ == "__main__":
    _record()
