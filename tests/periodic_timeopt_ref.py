"""Dense numpy restatement of the lap-time optimiser of the periodic (closed-loop) solve, one loop at a
time.

TEST INFRASTRUCTURE ONLY.  Independent of the HIP kernels: the objective is tests/periodic_ref.py's dense KKT system in
the monomial basis (J from the coefficients, dJ/dT from the multipliers), the optimiser is §12's algorithm with
tests/timeopt_ref.py's projection, measure and constants.
"""
import numpy as np

from tests import periodic_ref
from tests.timeopt_ref import ALPHA_MAX, ALPHA_MIN, ARMIJO, MAX_BACKTRACK, NOT_CONVERGED, pg_measure, project


def cost_grad(order, path, time, w=0.0):
    """(J, dJ/dT [S]) of the loop path [S,3] at the times time [S]."""
    _, J, g = periodic_ref.solve(order, path, time, w)
    return J, g


def _objective(order, path, T, w, rho):
    J, g = cost_grad(order, path, T, w)
    return J + rho * T.sum(), g + rho


def optimize(order, path, time, w=0.0, mode="fixed_total", rho=0.0, min_time=0.01, tol=1e-6, max_iters=100):
    """The kernel's optimiser (timeopt_ref.optimize over the periodic objective).  Returns dict(times, f0, f, iterations,
    status)."""
    T = np.asarray(time, dtype=np.float64).copy()
    ft = mode == "fixed_total"
    rho = 0.0 if ft else float(rho)
    total = T.sum() if ft else None
    if np.any(T < min_time):
        T = project(T, min_time, total)
    f, gf = _objective(order, path, T, w, rho)
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
                fe, ge = _objective(order, path, Tt, w, rho)
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
        # (pg = 0: the kernel's 1 / pg is inf and the clamp returns ALPHA_MAX)
        alpha = min(ALPHA_MAX, max(ALPHA_MIN, ss / sy if sy > 0 else (1.0 / pg if pg > 0 else ALPHA_MAX)))
        if pg <= tol:
            return dict(times=T, f0=f0, f=f, iterations=it, status=0)
        if it >= max_iters:
            return dict(times=T, f0=f0, f=f, iterations=it, status=NOT_CONVERGED)


# ------------------------------------------------------------------------------------ the inputs both test files share

def make_loop(order, S, row, seed=0):
    """(path [S,3], time [S]) of one loop, a function of its arguments alone: points around a wobbly circle of radius 3..6
    in angular order, plus a far offset (the solve must not depend on it), times U(0.5, 2)."""
    rng = np.random.default_rng([order, S, row, seed, 20261021])
    th = np.sort(rng.uniform(0.0, 2.0 * np.pi, S))
    r = rng.uniform(3.0, 6.0, S)
    path = np.stack([r * np.cos(th), r * np.sin(th), rng.normal(size=S)], axis=1) + 5.0 * rng.normal(size=3)
    time = rng.uniform(0.5, 2.0, S)
    return path, time


def hexagon(radius=4.0):
    th = np.arange(6) * (np.pi / 3.0)
    return np.stack([radius * np.cos(th), radius * np.sin(th), np.zeros(6)], axis=1)


def there_and_back(length=5.0):
    return np.array([[0.0, 0.0, 0.0], [length, 1.0, -0.5]])


# Where the optimiser stops inside the tolerance depends on the start, and the closed-form gates are set by the stopping
# measure (tol 1e-6), not by the arithmetic.  The starts of the closed-form cases are U(0.5, 2) draws whose seed was picked
# on the CPU, with optimize() above and nothing else, so that this reference ends well inside the gates at every order:
# fixed total (seed 2) times within 4.8e-7 of equal and J within 6.3e-11; time penalty (seed 5) within 2.7e-6 of t* at
# orders 2-4 and 1.5e-5 at order 5.  Seeds 0..7 range up to 1.5e-5 / 1.5e-8 and 2.3e-4.
CLOSED_FORM_SEED = {"fixed_total": 2, "time_penalty": 5}


def closed_form_start(order, S, mode):
    return np.random.default_rng([order, S, CLOSED_FORM_SEED[mode], 20261021]).uniform(0.5, 2.0, S)


def penalty_weight(order, cases, w=0.0):
    """rho of the time-penalty runs: the median of J / sum T over the first eight loops at the start, S = 1 skipped
    (J = 0 there); 1 for a batch of S = 1 loops."""
    wv = np.broadcast_to(np.asarray(w, dtype=np.float64), (len(cases),))
    v = [cost_grad(order, p, t, wv[b])[0] / t.sum() for b, (p, t) in enumerate(cases[:8]) if len(t) > 1]
    return float(np.median(v)) if v else 1.0
