"""High-precision reference of the two altitude programmes (TEST INFRASTRUCTURE ONLY): the pentadiagonal systems of
include/csp_alt.h assembled by the triplet rules of oracle/alt_oracle.c and tests/test_alt.py::_np_hessian, solved by
an O(n) banded LDL^T in mpmath at DPS digits.  Inputs are taken as the fp64 numbers they are; everything after that --
edge lengths, weights, sums, the factorisation -- is done at DPS digits, so the result is the exact solution of the
problem the fp64 codes are asked to solve, to ~DPS - log10(cond) digits (cond <= ~1e25 for the stiffest case used).

    optimize(xyz, elev, ls, lf, sd, mcr)  -> z [n] fp64 (rounded from mpmath)
    global_smooth(zin, xyz, ls, mcr)      -> (z [n] fp64, solves, margin)

`margin` is the smallest |z_i - (zin_i - 1e-3)| over the samples not yet active in any of the solves: how far the
active-set decisions were from a tie.  A test that compares solve counts uses only cases whose margin is far above the
error of the code under test.
"""
import mpmath as mp
import numpy as np

DPS = 60


def _bands(xyz, ls, mcr):
    """(diag, e = H[i][i-1], f = H[i][i-2]) of lambda L^T L + the climb-rate first differences, as mpf lists."""
    n = len(xyz)
    ls, mcr = mp.mpf(float(ls)), mp.mpf(float(mcr))
    d, e, f = [mp.mpf(0)] * n, [mp.mpf(0)] * n, [mp.mpf(0)] * n
    if n >= 3 and ls > 0:
        for i in range(1, n - 1):           # ls * outer([1, -2, 1]) on rows i-1 .. i+1
            d[i - 1] += ls; d[i] += 4 * ls; d[i + 1] += ls
            e[i] -= 2 * ls; e[i + 1] -= 2 * ls
            f[i + 1] += ls
    if mcr > 0:
        for i in range(n - 1):
            dx = mp.mpf(float(xyz[i + 1][0])) - mp.mpf(float(xyz[i][0]))
            dy = mp.mpf(float(xyz[i + 1][1])) - mp.mpf(float(xyz[i][1]))
            dist = mp.sqrt(dx * dx + dy * dy)
            if dist <= mp.mpf(1e-9) or dist * mcr <= mp.mpf(1e-12):   # the early-outs of edge_w; finite inputs only
                continue
            w = 1 / (dist * mcr) ** 2
            d[i] += w; d[i + 1] += w; e[i + 1] -= w
    return d, e, f


def _solve(d, e, f, r):
    """Banded LDL^T of the pentadiagonal SPD matrix (d, e, f) and the solve with right side r; all mpf lists."""
    n = len(d)
    D, l1, l2, y = [None] * n, [mp.mpf(0)] * n, [mp.mpf(0)] * n, [None] * n
    for i in range(n):
        if i >= 2:
            l2[i] = f[i] / D[i - 2]
        if i >= 1:
            l1[i] = (e[i] - (l2[i] * l1[i - 1] * D[i - 2] if i >= 2 else 0)) / D[i - 1]
        D[i] = d[i] - (l1[i] ** 2 * D[i - 1] if i >= 1 else 0) - (l2[i] ** 2 * D[i - 2] if i >= 2 else 0)
        y[i] = r[i] - (l1[i] * y[i - 1] if i >= 1 else 0) - (l2[i] * y[i - 2] if i >= 2 else 0)
    z = [None] * n
    for i in range(n - 1, -1, -1):
        z[i] = y[i] / D[i] - (l1[i + 1] * z[i + 1] if i + 1 < n else 0) - (l2[i + 2] * z[i + 2] if i + 2 < n else 0)
    return z


def optimize_mp(xyz, elev, ls, lf, sd, mcr):
    """optimizeHeights as a list of mpf."""
    with mp.workdps(DPS):
        n = len(elev)
        if n == 0:
            return []
        d, e, f = _bands(xyz, ls, mcr)
        lf, sd = mp.mpf(float(lf)), mp.mpf(float(sd))
        r = [mp.mpf(0)] * n
        floor = [None] * n
        for i in range(n):
            if not np.isnan(elev[i]):
                floor[i] = mp.mpf(float(elev[i])) + sd
                d[i] += lf
                r[i] = lf * max(mp.mpf(float(xyz[i][2])), floor[i])
            d[i] += mp.mpf(1e-8)
        z = _solve(d, e, f, r)
        return [zi if fl is None else max(zi, fl) for zi, fl in zip(z, floor)]


def optimize(xyz, elev, ls=1.0, lf=0.0, sd=50.0, mcr=2.0):
    return np.array([float(v) for v in optimize_mp(xyz, elev, ls, lf, sd, mcr)], dtype=np.float64)


def global_smooth_mp(zin, xyz, ls, mcr):
    """optimizeHeightsGlobalSmooth: (list of mpf, solves, smallest margin to the activation threshold)."""
    with mp.workdps(DPS):
        n = len(zin)
        if n == 0:
            return [], 0, mp.inf
        d0, e, f = _bands(xyz, ls, mcr)
        zi = [mp.mpf(float(v)) for v in zin]
        big, pen, thr = mp.mpf(1e10), mp.mpf(1e8), mp.mpf(1e-3)
        active = [False] * n
        margin, solves, z = mp.inf, 0, None
        for _ in range(10):
            d, r = list(d0), [mp.mpf(0)] * n
            d[0] += big; r[0] += big * zi[0]
            d[n - 1] += big; r[n - 1] += big * zi[n - 1]
            for i in range(1, n - 1):
                if active[i]:
                    d[i] += pen; r[i] += pen * zi[i]
            for i in range(n):
                d[i] += mp.mpf(1e-8)
            z = _solve(d, e, f, r)
            solves += 1
            new = False
            for i in range(n):
                if not active[i]:
                    margin = min(margin, abs(z[i] - (zi[i] - thr)))
                    if z[i] < zi[i] - thr:
                        active[i] = new = True
            if not new:
                break
        return [max(a, b) for a, b in zip(z, zi)], solves, margin


def global_smooth(zin, xyz, ls=1.0, mcr=2.0):
    z, solves, margin = global_smooth_mp(zin, xyz, ls, mcr)
    return np.array([float(v) for v in z], dtype=np.float64), solves, float(margin)


def rel_err(got, ref):
    """max-abs over max-abs, the figure every altitude gate uses (0 for empty problems)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), np.finfo(np.float64).tiny))
