"""csp_minsnap_optimize_times_knots_batch on the MI355X: the standard mask against the existing optimiser,
closed forms the standard partition cannot satisfy, invariants against the dense reference tests/knots_timeopt_ref.py,
the start's cost against the 40-digit tests/knots_ref.py, edges, determinism and memory (tests/guarded.py).

Batches mix the mask patterns lane by lane (trajectory b has PATTERNS[b % 5], "free_end" where the pattern does not apply
to the order or the length), so the lanes of a wave solve different partitions and take different numbers of iterations.
Times U(0.5, 2) (spread <= 4), waypoints random walks of step ~2, pinned values N(0, 0.5).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import guarded, knots_ref, knots_timeopt_ref
from tests.test_gpu_timeopt import GATE_J
from tests.timeopt_ref import NOT_CONVERGED, pg_measure

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NONFINITE, NOT_SPD, SKIPPED = 1, 2, 4
ORDERS = (2, 3, 4, 5)
PATTERNS = ("free_end", "both_free", "vel_mid", "rest_mid", "random")
B = 70
# min_time 0.5 (exact in fp32 too, so T >= min_time can be asked bit for bit): a free end drives its last segment to the
# bound, and with a smaller bound the optimum has times 20 apart, where the dense reference's own J is off by 1e-3 at
# order 5 against the 40-digit tests/knots_ref.py (1e-11 at the start's spread of 4) and could not gate anything
TMIN, TOL, MAX_ITERS = 0.5, 1e-6, 300
# final objective against the reference optimiser's, and J against the reference's at the returned times: the project's
# gates between kernel and reference optimiser (tests/test_gpu_timeopt.py)
GATE_F = {2: 2e-7, 3: 2e-7, 4: 2e-7, 5: 1e-6}
GATE_JT = {2: 1e-8, 3: 1e-8, 4: 1e-8, 5: 1e-6}
# uniform S -> the mode it runs in (S = 1 with the fixed total has nothing to optimise)
MODE = {1: "time_penalty", 2: "fixed_total", 3: "time_penalty", 6: "fixed_total"}
# (order, S) -> seed, picked on the CPU so that the reference optimiser (knots_timeopt_ref.optimize, tol 1e-6, 300
# iterations) converges on at least 7/8 of the batch; its share is written beside the seed.  S = 0 is the ragged batch.
SEEDS = {
    (2, 1): 0,   # 70/70
    (2, 2): 0,   # 70/70
    (2, 3): 0,   # 70/70
    (2, 6): 0,   # 70/70
    (2, 0): 0,   # 40/40
    (3, 1): 0,   # 70/70
    (3, 2): 0,   # 67/70
    (3, 3): 0,   # 70/70
    (3, 6): 0,   # 69/70
    (3, 0): 0,   # 40/40
    (4, 1): 0,   # 70/70
    (4, 2): 0,   # 69/70
    (4, 3): 0,   # 70/70
    (4, 6): 0,   # 67/70
    (4, 0): 0,   # 38/40
    (5, 1): 0,   # 70/70
    (5, 2): 0,   # 68/70
    (5, 3): 0,   # 69/70
    (5, 6): 3,   # 62/70 (seeds 0, 1, 2, 4, 5, 6: 60, 55, 53, 61, 59, 57)
    (5, 0): 0,   # 35/40
}
RAGGED_B = 40


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


# ----------------------------------------------------------------------------------------------------------------- inputs

def applicable(order, S, pattern):
    if pattern == "both_free":
        return order <= 3 and S >= 2   # the count (S + 1 positions) must reach the order
    if pattern in ("vel_mid", "rest_mid"):
        return S >= 2
    return True


def well_posed(order, time, mask):
    """The minimiser is unique iff no non-zero polynomial of degree < order vanishes at every knot together with its
    pinned derivatives (it would cost nothing).  The constraint count >= order is necessary, not sufficient: at order 5
    with S = 1, snap pinned at both knots is one condition on a quartic, not two, and the Hessian of the free
    derivatives is singular (CSP_TRAJ_NOT_SPD from a pivot).  Checked as the rank of the conditions on the o coefficients,
    with the knots' times scaled to [0, 1]."""
    o = int(order)
    tk = np.concatenate([[0.0], np.cumsum(time)]) / np.sum(time)
    rows = []
    for k, t in enumerate(tk):
        for r in range(o):
            if r == 0 or (int(mask[k]) >> (r - 1)) & 1:
                rows.append([np.prod(np.arange(i, i - r, -1)) * t ** (i - r) if i >= r else 0.0 for i in range(o)])
    return np.linalg.matrix_rank(np.array(rows), tol=1e-9) == o


def make_case(order, S, pattern, row, seed=0):
    """(path [S+1,3], time [S], mask [S+1], values [S+1,o-1,3]) of one trajectory, a function of its arguments alone."""
    n = order - 1
    full = (1 << n) - 1
    if not applicable(order, S, pattern):
        pattern = "free_end"
    rng = np.random.default_rng([order, S, PATTERNS.index(pattern), row, seed, 20261021])
    path = np.cumsum(rng.normal(size=(S + 1, 3)) * 2, axis=0)
    time = rng.uniform(0.5, 2.0, S)
    values = rng.normal(size=(S + 1, n, 3)) * 0.5
    values[0, 2:] = values[S, 2:] = 0.0
    mask = np.zeros(S + 1, dtype=np.uint8)
    mask[0] = mask[S] = full
    mid = (S + 1) // 2 if S >= 2 else 0
    if pattern == "free_end":
        mask[S] = 0
    elif pattern == "both_free":
        mask[0] = mask[S] = 0
    elif pattern == "vel_mid":
        mask[mid] |= 1
    elif pattern == "rest_mid":
        mask[mid] = full
        values[mid] = 0.0
    elif pattern == "random":
        mask[:] = rng.integers(0, full + 1, size=S + 1)
        if not well_posed(order, time, mask):   # (contains the count rule) a full first knot always is: Taylor's polynomial
            mask[0] = full
    return path, time, mask, values


def uniform_cases(order, S, rows=B, seed=None):
    seed = SEEDS[(order, S)] if seed is None else seed
    return [make_case(order, S, PATTERNS[b % len(PATTERNS)], b, seed) for b in range(rows)]


def ragged_cases(order, seed=None):
    seed = SEEDS[(order, 0)] if seed is None else seed
    lens = np.random.default_rng([order, seed, 77]).integers(1, 10, size=RAGGED_B)
    return [make_case(order, int(s), PATTERNS[b % len(PATTERNS)], b, seed) for b, s in enumerate(lens)]


def ragged_weights(order):
    return np.random.default_rng(order).uniform(0.0, 0.3, size=RAGGED_B)


def stack(cases):
    return tuple(np.ascontiguousarray(np.stack([c[i] for c in cases])) for i in range(4))


def concat(cases):
    off = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])]).astype(np.int64)
    return tuple(np.ascontiguousarray(np.concatenate([c[i] for c in cases])) for i in range(4)) + (off,)


def penalty_weight(order, cases, w=0.0):
    """rho of the time-penalty runs: the median of J / sum T over the first eight trajectories at the start (reference)."""
    wv = np.broadcast_to(np.asarray(w, dtype=np.float64), (len(cases),))
    return float(np.median([knots_timeopt_ref.cost_grad(order, p, t, m, v, wv[b])[0] / t.sum()
                            for b, (p, t, m, v) in enumerate(cases[:8])]))


def check_batch(order, cases, r, mode, rho, w=0.0, f32=False, check_ref=4, tmin=TMIN, tol=TOL):
    """The invariants of tests/test_gpu_timeopt.py's _invariants, per trajectory, against knots_timeopt_ref.  With fp32
    storage the reference sees the inputs as the kernel does (rounded to fp32), the returned times are rounded to fp32,
    so the fixed total holds to 1e-6, J at the returned times to (2o-1) 2^-23 (J ~ T^(1-2o) and every time moved by up to
    2^-24 relative), and the stationarity measure is not asked of the rounded times."""
    T, obj, it, st = (_host(x) for x in (r.times, r.objective, r.iterations, r.status))
    T = T.reshape(-1).astype(np.float64)
    wv = np.broadcast_to(np.asarray(w, dtype=np.float64), (len(cases),))
    rd = (lambda a: np.asarray(a).astype(np.float32).astype(np.float64)) if f32 else (lambda a: np.asarray(a, dtype=np.float64))
    gate_jt = max(GATE_JT[order], (2 * order - 1) * 2.0 ** -23) if f32 else GATE_JT[order]
    pos = nconv = 0
    for b, (p, t, m, v) in enumerate(cases):
        p, t, v = rd(p), rd(t), rd(v)
        tb = T[pos:pos + len(t)]
        pos += len(t)
        assert st[b] & ~NOT_CONVERGED == 0, (b, st[b])
        assert obj[b, 1] <= obj[b, 0], (b, obj[b])
        assert tb.min() >= tmin, (b, tb.min())
        if mode == "fixed_total":
            assert abs(tb.sum() - t.sum()) <= (1e-6 if f32 else 1e-12) * t.sum(), (b, tb.sum(), t.sum())
        J, g = knots_timeopt_ref.cost_grad(order, p, tb, m, v, wv[b])
        pen = rho if mode == "time_penalty" else 0.0
        f = J + pen * tb.sum()
        # With a constraint count <= order and zero weight a polynomial of degree < order meets every constraint: J is
        # exactly zero, whatever the times, and a relative gate divides by rounding noise.  It is scaled by
        # L^2 / T_min^(2o-1) (L the longest leg) there, as in tests/test_gpu_knots.py.
        scale = abs(f)
        if knots_ref.constraint_count(order, m) <= order and wv[b] == 0.0:
            scale = pen * tb.sum() + np.max(np.linalg.norm(np.diff(p, axis=0), axis=1)) ** 2 / tb.min() ** (2 * order - 1)
        assert abs(f - obj[b, 1]) <= gate_jt * scale, (b, f, obj[b, 1])
        if st[b] == 0:
            nconv += 1
            if not f32 and (scale == abs(f) or pen):   # (J identically zero: its gradient is rounding noise over a noise f0)
                # the reference's gradient has its own rounding: a 2x margin on the measure
                pg = pg_measure(tb, g + pen, t.mean(), obj[b, 0], tmin,
                                t.sum() if mode == "fixed_total" else None)
                assert pg <= 2 * tol, (b, pg)
        if b < check_ref:
            ref = knots_timeopt_ref.optimize(order, p, t, m, v, wv[b], mode, rho, tmin, tol, 500)
            assert abs(ref["f"] - obj[b, 1]) <= GATE_F[order] * (scale if scale != abs(f) else ref["f"]), (b, ref["f"], obj[b, 1])
    return nconv


def check_cap(order, nconv, total, tag):
    """NOT_CONVERGED on at most 1/4 of a batch (3/8 at order 5): a condition of the issue, not a measurement."""
    print("%s: converged %d / %d" % (tag, nconv, total))
    allowed = total * 3 // 8 if order == 5 else total // 4
    assert total - nconv <= allowed, (tag, nconv, total)


# ------------------------------------------------------------------- 1. the standard mask against the existing optimiser

@pytest.mark.parametrize("mode", ["fixed_total", "time_penalty"])
@pytest.mark.parametrize("order", ORDERS)
def test_standard_mask_meets_the_existing_optimiser(csp, order, mode):
    Bn, S = 8, 6
    cs = [make_case(order, S, "free_end", b, 100 + order) for b in range(Bn)]
    wp, tm = stack(cs)[:2]
    bc = np.random.default_rng(order).normal(size=(Bn, 4, 3)) * 0.5
    mk, kv = csp.knots_from_bc(bc, S, order)
    c0 = csp.snap_cost_batch(wp, tm, bc, order=order)
    rho = float(np.median(c0.cost / tm.sum(axis=1))) if mode == "time_penalty" else 0.0
    kw = dict(order=order, mode=mode, time_weight=rho, min_time=TMIN, tol=TOL, max_iters=MAX_ITERS)
    old = csp.optimize_times_batch(wp, tm, bc, **kw)
    new = csp.optimize_times_knots_batch(wp, tm, mk, kv, **kw)
    assert not (new.status & ~NOT_CONVERGED).any(), new.status
    start = c0.cost + rho * tm.sum(axis=1)
    e0 = np.max(np.abs(new.objective[:, 0] - start) / np.abs(c0.cost))
    both = (old.status == 0) & (new.status == 0)
    ef = np.max(np.abs(new.objective[both, 1] - old.objective[both, 1]) / old.objective[both, 1]) if both.any() else 0.0
    print("o%d %s: start %.2e  final %.2e on %d lanes" % (order, mode, e0, ef, both.sum()))
    assert e0 <= GATE_J[order], e0
    assert both.sum() >= 1 and ef <= GATE_F[order], ef
    # the coefficients are the knots solve's at the returned times
    ref = csp.solve_knots_batch(wp, new.times, mk, kv, order=order)
    assert np.array_equal(new.coeffs, ref.coeffs)


# ---------------------------------------------------------- 2. closed forms that the standard partition cannot satisfy

def _rest_stop(order, Bn=3):
    n = order - 1
    rng = np.random.default_rng(order)
    wp = np.cumsum(rng.normal(size=(Bn, 3, 3)) * rng.uniform(0.5, 4.0, size=(Bn, 3, 1)), axis=1)
    mk = np.full((Bn, 3), (1 << n) - 1, dtype=np.uint8)
    kv = np.zeros((Bn, 3, n, 3))
    return wp, mk, kv


@pytest.mark.parametrize("order", ORDERS)
def test_rest_stop_fixed_total_closed_form(csp, order):
    """Every bit set with zero values at all three knots: each side is an independent rest-to-rest segment with
    J_j = a_j T_j^(1-2o), a_j ~ |dP_j|^2, so at the optimum T_0 / T_1 = (|dP_0| / |dP_1|)^(1/o)."""
    wp, mk, kv = _rest_stop(order)
    tm = np.tile([[0.8, 1.7]], (len(wp), 1))
    r = csp.optimize_times_knots_batch(wp, tm, mk, kv, order=order, min_time=1e-3, tol=1e-9, max_iters=MAX_ITERS)
    # a lane may stop at the rounding floor of J before the measure reaches 1e-9 (NOT_CONVERGED); the gate is on the times
    assert not (r.status & ~NOT_CONVERGED).any(), r.status
    leg = np.linalg.norm(np.diff(wp, axis=1), axis=2)
    ratio = (leg[:, 0] / leg[:, 1]) ** (1.0 / order)
    want = np.stack([2.5 * ratio / (1 + ratio), 2.5 / (1 + ratio)], axis=1)
    err = np.max(np.abs(r.times - want) / want)
    print("o%d rest stop, fixed total: %.2e" % (order, err))
    assert err < 1e-7, (r.times, want)


@pytest.mark.parametrize("order", ORDERS)
def test_rest_stop_time_penalty_closed_form(csp, order):
    """The same masks with the time penalty: T_j* = ((2o-1) a_j / rho)^(1/(2o)), a_j from the knots solve's cost of each
    one-segment piece at unit time."""
    wp, mk, kv = _rest_stop(order)
    Bn = len(wp)
    one = np.ones((Bn, 1))
    a = np.stack([csp.solve_knots_batch(wp[:, j:j + 2], one, mk[:, :2], kv[:, :2], order=order, want_cost=True).cost
                  for j in range(2)], axis=1)
    rho = 0.5 * float(a.min())
    r = csp.optimize_times_knots_batch(wp, np.ones((Bn, 2)), mk, kv, order=order, mode="time_penalty", time_weight=rho,
                                       min_time=1e-3, tol=1e-9, max_iters=MAX_ITERS)
    # a lane may stop at the rounding floor of J before the measure reaches 1e-9 (NOT_CONVERGED); the gate is on the times
    assert not (r.status & ~NOT_CONVERGED).any(), r.status
    want = ((2 * order - 1) * a / rho) ** (1.0 / (2 * order))
    err = np.max(np.abs(r.times - want) / want)
    print("o%d rest stop, time penalty: %.2e" % (order, err))
    assert err < 1e-7, (r.times, want)


@pytest.mark.parametrize("order", ORDERS)
def test_free_end_time_penalty_closed_form(csp, order):
    """S = 1, the start fully pinned at rest, the end free: J is still homogeneous of degree 1 - 2o, so
    T* = ((2o-1) J(1) / rho)^(1/(2o))."""
    n = order - 1
    wp = np.cumsum(np.random.default_rng(order).normal(size=(3, 2, 3)) * 2, axis=1)
    mk = np.tile(np.array([[(1 << n) - 1, 0]], dtype=np.uint8), (3, 1))
    kv = np.zeros((3, 2, n, 3))
    one = np.ones((3, 1))
    J1 = csp.solve_knots_batch(wp, one, mk, kv, order=order, want_cost=True).cost
    rho = 0.5 * float(J1.min())
    r = csp.optimize_times_knots_batch(wp, one, mk, kv, order=order, mode="time_penalty", time_weight=rho, min_time=1e-3,
                                       tol=1e-9, max_iters=MAX_ITERS)
    # a lane may stop at the rounding floor of J before the measure reaches 1e-9 (NOT_CONVERGED); the gate is on the times
    assert not (r.status & ~NOT_CONVERGED).any(), r.status
    want = ((2 * order - 1) * J1 / rho) ** (1.0 / (2 * order))
    err = np.max(np.abs(r.times[:, 0] - want) / want)
    print("o%d free end, time penalty: %.2e" % (order, err))
    assert err < 1e-7, (r.times[:, 0], want)


# ------------------------------------------------------------------------------------------- 3. invariants and reference

@pytest.mark.parametrize("S", [1, 2, 3, 6])
@pytest.mark.parametrize("order", ORDERS)
def test_invariants_uniform(csp, order, S):
    cases = uniform_cases(order, S)
    wp, tm, mk, kv = stack(cases)
    mode = MODE[S]
    rho = penalty_weight(order, cases) if mode == "time_penalty" else 0.0
    r = csp.optimize_times_knots_batch(_dev(wp), _dev(tm), _dev(mk), _dev(kv), order=order, mode=mode, time_weight=rho,
                                       min_time=TMIN, tol=TOL, max_iters=MAX_ITERS)
    torch.cuda.synchronize()
    nconv = check_batch(order, cases, r, mode, rho)
    check_cap(order, nconv, B, "o%d S%d %s" % (order, S, mode))


@pytest.mark.parametrize("order", ORDERS)
def test_invariants_ragged_device_and_host_f32(csp, order):
    cases = ragged_cases(order)
    wp, tm, mk, kv, off = concat(cases)
    w = ragged_weights(order)
    r = csp.optimize_times_knots_batch(_dev(wp), _dev(tm), _dev(mk), _dev(kv), order=order, min_time=TMIN, tol=TOL,
                                       max_iters=MAX_ITERS, seg_offsets=_dev(off), vel_zero_weight_per_traj=_dev(w))
    torch.cuda.synchronize()
    nconv = check_batch(order, cases, r, "fixed_total", 0.0, w)
    check_cap(order, nconv, RAGGED_B, "o%d ragged device" % order)
    # fp32 storage, host memory: fp64 arithmetic, the returned times rounded to fp32
    f = np.float32
    r32 = csp.optimize_times_knots_batch(wp.astype(f), tm.astype(f), mk, kv.astype(f), order=order, min_time=TMIN, tol=TOL,
                                         max_iters=MAX_ITERS, seg_offsets=off, vel_zero_weight_per_traj=w)
    assert r32.times.dtype == f and r32.coeffs.dtype == f
    nconv = check_batch(order, cases, r32, "fixed_total", 0.0, w, f32=True)
    check_cap(order, nconv, RAGGED_B, "o%d ragged host fp32" % order)


# --------------------------------------------------------------- 4. cost and gradient of the pass against what exists

@functools.lru_cache(maxsize=None)
def _reference_costs(order):
    """40-digit J of ten trajectories (the five patterns at S = 3 and at S = 6); computed once, never changed."""
    out = []
    for S in (3, 6):
        for i, pat in enumerate(PATTERNS):
            c = make_case(order, S, pat, i, 400)
            out.append((c, knots_ref.solve(order, *c).cost))
    return tuple(out)


@pytest.mark.parametrize("order", ORDERS)
def test_start_cost_against_the_40_digit_reference(csp, order):
    """objective[:, 0] against knots_ref's J: at most 4x the error of solve_knots_batch(want_cost=True).cost on the same
    inputs (another summation order of the same quadratic form), floor 64 ulp.  Both are the worst over the order's ten
    trajectories."""
    e_new = e_old = 0.0
    for S in (3, 6):
        sel = [(c, J) for c, J in _reference_costs(order) if len(c[1]) == S]
        wp, tm, mk, kv = stack([c for c, _ in sel])
        Jr = np.array([J for _, J in sel])
        r = csp.optimize_times_knots_batch(wp, tm, mk, kv, order=order, min_time=1e-3, max_iters=0, want_coeffs=False)
        k = csp.solve_knots_batch(wp, tm, mk, kv, order=order, want_cost=True)
        assert not (r.status & ~NOT_CONVERGED).any() and not k.status.any()
        assert np.array_equal(r.times, tm) and np.array_equal(r.objective[:, 0], r.objective[:, 1])
        e_new = max(e_new, float(np.max(np.abs(r.objective[:, 0] - Jr) / Jr)))
        e_old = max(e_old, float(np.max(np.abs(k.cost - Jr) / Jr)))
    print("o%d start cost vs 40 digits: optimiser %.2e  knots solve %.2e" % (order, e_new, e_old))
    assert e_new <= max(4 * e_old, 64 * 2.0 ** -52), (e_new, e_old)


@pytest.mark.parametrize("order", ORDERS)
def test_one_iteration_strictly_decreases(csp, order):
    cases = uniform_cases(order, 6, seed=500)
    wp, tm, mk, kv = stack(cases)
    r = csp.optimize_times_knots_batch(wp, tm, mk, kv, order=order, min_time=TMIN, tol=1e-12, max_iters=1, want_coeffs=False)
    assert np.all(r.status == NOT_CONVERGED) and np.all(r.iterations == 1)
    assert np.all(r.objective[:, 1] < r.objective[:, 0])


# ------------------------------------------------------------------------------------------------------------- 5. edges

def test_max_iters_zero_returns_the_start(csp):
    wp, tm, mk, kv = stack(uniform_cases(4, 6, seed=600))
    r = csp.optimize_times_knots_batch(wp, tm, mk, kv, order=4, min_time=TMIN, max_iters=0)
    assert np.array_equal(r.times, tm)
    assert np.all(r.status == NOT_CONVERGED) and not r.iterations.any()
    assert np.array_equal(r.objective[:, 0], r.objective[:, 1])


@pytest.mark.parametrize("order", ORDERS)
def test_single_segment_fixed_total_is_bit_identical(csp, order):
    wp, tm, mk, kv = stack(uniform_cases(order, 1, seed=700))
    r = csp.optimize_times_knots_batch(_dev(wp), _dev(tm), _dev(mk), _dev(kv), order=order, min_time=TMIN)
    torch.cuda.synchronize()
    assert _host(r.times).tobytes() == tm.tobytes()
    assert not _host(r.status).any() and not _host(r.iterations).any()
    obj = _host(r.objective)
    assert np.array_equal(obj[:, 0], obj[:, 1])


@pytest.mark.parametrize("order", (3, 4, 5))
def test_count_rule_lanes(csp, order):
    """S = 1: two positions.  A lane with fewer than order - 2 mask bits has no unique minimiser: CSP_TRAJ_NOT_SPD from the
    count, times_out = times_in, iterations 0, NaN objectives, the knots solve's NaN coefficients; the lanes beside it
    have the bits of a run without it."""
    wp, tm, mk, kv = stack(uniform_cases(order, 1, seed=800))
    bad = [3, 64, 69]
    mk2 = mk.copy()
    mk2[bad, :] = 0
    kw = dict(order=order, mode="time_penalty", time_weight=5.0, min_time=TMIN, max_iters=50)
    good = csp.optimize_times_knots_batch(_dev(wp), _dev(tm), _dev(mk), _dev(kv), **kw)
    r = csp.optimize_times_knots_batch(_dev(wp), _dev(tm), _dev(mk2), _dev(kv), **kw)
    torch.cuda.synchronize()
    k = csp.solve_knots_batch(_dev(wp), r.times, _dev(mk2), _dev(kv), order=order)
    torch.cuda.synchronize()
    assert torch.equal(r.coeffs.view(torch.int64), k.coeffs.view(torch.int64))
    keep = np.setdiff1d(np.arange(B), bad)
    for name in ("times", "coeffs", "objective", "iterations", "status"):
        a, g = _host(getattr(r, name)), _host(getattr(good, name))
        assert a[keep].tobytes() == g[keep].tobytes(), name
    for b in bad:
        assert _host(r.status)[b] == NOT_SPD and _host(r.iterations)[b] == 0
        assert np.isnan(_host(r.objective)[b]).all() and np.isnan(_host(r.coeffs)[b]).all()
        assert _host(r.times)[b].tobytes() == tm[b].tobytes()


@pytest.mark.parametrize("order", ORDERS)
def test_ragged_edges_on_the_device(csp, order):
    """A ragged device batch with max_segments = 5 (the workspace, guard-banded, sized for 5): a 9-segment member is
    CSP_TRAJ_SKIPPED with its times copied through, NaN objectives and iterations 0; S_b = 0 gets status 0, objectives 0
    and iterations 0; every other trajectory has the bits of the call with max_segments = 9."""
    n = order - 1
    lens = (3, 0, 9, 5, 1, 0, 2)
    cases = [make_case(order, s, PATTERNS[b % 5], b, 900) if s else
             (np.ones((1, 3)), np.zeros(0), np.array([0xFF], np.uint8), np.full((1, n, 3), np.nan)) for b, s in enumerate(lens)]
    wp, tm, mk, kv, off = concat(cases)
    host = dict(waypoints=wp, times=tm, knot_mask=mk, knot_values=kv, seg_offsets=off, vw=np.zeros(len(lens)))
    full = _guarded_call(csp, order, host, None, 9, 0xFF, False)
    short = _guarded_call(csp, order, host, None, 5, 0xFF, False)
    M = 2 * order
    for i, s in enumerate(lens):
        sl = slice(off[i], off[i + 1])
        if s > 5:
            assert short["status"][i] == SKIPPED and short["iterations"][i] == 0 and np.isnan(short["objective"][i]).all()
            assert short["times"][sl].tobytes() == tm[sl].tobytes()
            assert (short["coeffs"].reshape(-1, 3 * M)[sl].view(np.uint8) == 0xFF).all(), "coefficients of a skipped trajectory"
        else:
            for k in ("times", "objective", "iterations", "status"):
                a, b = ((x[k].reshape(len(lens), -1)[i] if k != "times" else x[k][sl]) for x in (short, full))
                assert a.tobytes() == b.tobytes(), (i, k)
            assert short["coeffs"].reshape(-1, 3 * M)[sl].tobytes() == full["coeffs"].reshape(-1, 3 * M)[sl].tobytes()
        if s == 0:
            assert short["status"][i] == 0 and short["iterations"][i] == 0 and not short["objective"][i].any()


@pytest.mark.parametrize("order", ORDERS)
def test_bad_lanes_change_no_other_lane(csp, order):
    """An inf time: CSP_TRAJ_NONFINITE, returned unchanged.  A NaN waypoint: the trajectory stops at the start with
    CSP_TRAJ_NONFINITE, times = the start, iterations 0.  NaN / inf in values whose mask bit is clear: no output changes.
    Every other lane of the wave has the bits of the run without them."""
    cases = uniform_cases(order, 3, seed=1000)
    wp, tm, mk, kv = stack(cases)
    kw = dict(order=order, min_time=TMIN, max_iters=60)
    good = csp.optimize_times_knots_batch(_dev(wp), _dev(tm), _dev(mk), _dev(kv), **kw)
    wp2, tm2, kv2 = wp.copy(), tm.copy(), kv.copy()
    tm2[5, 1] = np.inf
    wp2[9, 2, 1] = np.nan
    free = ((mk[:, :, None] >> np.arange(order - 1)) & 1) == 0
    kv2[free] = np.where(np.arange(free.sum()) % 2 == 0, np.nan, np.inf)[:, None]
    r = csp.optimize_times_knots_batch(_dev(wp2), _dev(tm2), _dev(mk), _dev(kv2), **kw)
    torch.cuda.synchronize()
    keep = np.setdiff1d(np.arange(B), [5, 9])
    for name in ("times", "coeffs", "objective", "iterations", "status"):
        a, g = _host(getattr(r, name)), _host(getattr(good, name))
        assert a[keep].tobytes() == g[keep].tobytes(), name
    st, it, T, obj = _host(r.status), _host(r.iterations), _host(r.times), _host(r.objective)
    assert st[5] == NONFINITE and it[5] == 0 and T[5].tobytes() == tm2[5].tobytes() and np.isnan(obj[5]).all()
    assert st[9] & NONFINITE and it[9] == 0 and T[9].tobytes() == tm[9].tobytes()


def test_empty_batch(csp):
    wp, tm, mk, kv = np.zeros((0, 5, 3)), np.zeros((0, 4)), np.zeros((0, 5), np.uint8), np.zeros((0, 5, 3, 3))
    assert csp.optimize_times_knots_batch(wp, tm, mk, kv).times.shape == (0, 4)
    r = csp.optimize_times_knots_batch(_dev(wp), _dev(tm), _dev(mk), _dev(kv))
    torch.cuda.synchronize()
    assert r.times.shape == (0, 4) and r.coeffs.shape == (0, 4, 3, 8)


# ------------------------------------------------------------------------- 6. determinism and the coefficient contract

@pytest.mark.parametrize("order", (3, 4, 5))
def test_deterministic_and_coeffs_are_the_knots_solve(csp, order):
    S = 6
    wp, tm, mk, kv = stack(uniform_cases(order, S, seed=1100))
    d = [_dev(x) for x in (wp, tm, mk, kv)]
    kw = dict(order=order, min_time=TMIN, max_iters=50)
    r1 = csp.optimize_times_knots_batch(*d, **kw)
    r2 = csp.optimize_times_knots_batch(*d, **kw)
    torch.cuda.synchronize()
    ref = csp.solve_knots_batch(d[0], r1.times, d[2], d[3], order=order)
    torch.cuda.synchronize()
    assert torch.equal(r1.coeffs, ref.coeffs)
    names = ("times", "coeffs", "objective", "iterations", "status")
    for nm in names:
        assert torch.equal(getattr(r1, nm), getattr(r2, nm)), nm
    rh = csp.optimize_times_knots_batch(wp, tm, mk, kv, **kw)
    for nm in names:
        assert getattr(rh, nm).tobytes() == _host(getattr(r1, nm)).tobytes(), nm


# ------------------------------------------------------------------------------------------------------------ 7. memory

def _guarded_call(csp, order, host, uniform_S, max_segments, fill, f32, mode="fixed_total", rho=0.0, max_iters=40):
    """One device-memory call through the raw C-ABI with every array in a guard-banded buffer of exactly its documented
    size; workspace and outputs start as `fill` bytes.  Checks the return code, every band, and that no input changed."""
    Bn = host["vw"].shape[0]
    total = host["times"].size
    elt = 4 if f32 else 8
    n = order - 1
    ins = {k: guarded.carve_from(v, DEV, name=k) for k, v in host.items()}
    outs = {"times": guarded.Guarded(total * elt, DEV, name="times_out").fill(fill),
            "coeffs": guarded.Guarded(total * 3 * 2 * order * elt, DEV, name="coeffs").fill(fill),
            "objective": guarded.Guarded(Bn * 16, DEV, name="objective").fill(fill),
            "iterations": guarded.Guarded(Bn * 4, DEV, name="iterations").fill(fill),
            "status": guarded.Guarded(Bn * 4, DEV, name="status").fill(fill)}
    ragged = uniform_S is None
    desc = csp.make_desc(order, Bn, 0 if ragged else uniform_S, csp.DTYPE_F32 if f32 else csp.DTYPE_F64, 0.0, 0.0, csp.MEM_DEVICE,
                         False, ins["seg_offsets"].data_ptr() if ragged else None, max_segments if ragged else 0, ins["vw"].data_ptr())
    need = csp.knots_timeopt_workspace_bytes(desc)
    smax = max_segments if ragged else uniform_S
    assert need == ((smax + 1) * (n * n + 3 * n) * Bn * 8 + 255) // 256 * 256 + 4 * smax * Bn * 8
    ws = guarded.Guarded(need, DEV, name="workspace").fill(fill)
    prm = csp.make_timeopt_params(csp.TIMEOPT_FIXED_TOTAL if mode == "fixed_total" else csp.TIMEOPT_TIME_PENALTY, rho, TMIN,
                                  TOL, max_iters)
    rc = csp.raw_lib().csp_minsnap_optimize_times_knots_batch(
        ctypes.byref(desc), ctypes.byref(prm), ins["waypoints"].data_ptr(), ins["times"].data_ptr(),
        ins["knot_mask"].data_ptr(), ins["knot_values"].data_ptr(), outs["times"].data_ptr(), outs["coeffs"].data_ptr(),
        outs["objective"].data_ptr(), outs["iterations"].data_ptr(), outs["status"].data_ptr(), ws.data_ptr(), need,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, csp.strerror(rc))
    torch.cuda.synchronize()
    for g in [ws] + list(ins.values()) + list(outs.values()):
        g.check()
    for k, g in ins.items():
        assert g.bytes().tobytes() == np.ascontiguousarray(host[k]).tobytes(), (k, "an input changed")
    fl = np.float32 if f32 else np.float64
    return dict(times=outs["times"].numpy(fl), coeffs=outs["coeffs"].numpy(fl), objective=outs["objective"].numpy(np.float64, (-1, 2)),
                iterations=outs["iterations"].numpy(np.int32), status=outs["status"].numpy(np.int32))


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("order", ORDERS)
def test_guard_bands_and_stale_workspace_uniform(csp, order, f32):
    """The workspace carved at exactly knots_timeopt_workspace_bytes, every output at exactly its size, the inputs guarded:
    no band is touched, no input changes, and a 0x00-filled and a 0xFF-filled start give the same bits."""
    fl = np.float32 if f32 else np.float64
    for S in (1, 2, 6):
        wp, tm, mk, kv = stack(uniform_cases(order, S, seed=1200))
        host = dict(waypoints=wp.astype(fl), times=tm.astype(fl), knot_mask=mk, knot_values=kv.astype(fl), vw=np.zeros(B))
        mode, rho = ("time_penalty", 5.0) if S == 1 else ("fixed_total", 0.0)
        a = _guarded_call(csp, order, host, S, None, 0x00, f32, mode, rho)
        b = _guarded_call(csp, order, host, S, None, 0xFF, f32, mode, rho)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (S, k, "differs between a 0x00 and a 0xFF start")
        assert not (a["status"] & ~NOT_CONVERGED).any()


@pytest.mark.parametrize("order", ORDERS)
def test_guard_bands_and_stale_workspace_ragged(csp, order):
    cases = ragged_cases(order, seed=1300)
    wp, tm, mk, kv, off = concat(cases)
    host = dict(waypoints=wp, times=tm, knot_mask=mk, knot_values=kv, seg_offsets=off, vw=ragged_weights(order))
    a = _guarded_call(csp, order, host, None, 9, 0x00, False)
    b = _guarded_call(csp, order, host, None, 9, 0xFF, False)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (k, "differs between a 0x00 and a 0xFF start")
    assert not (a["status"] & ~NOT_CONVERGED).any()
