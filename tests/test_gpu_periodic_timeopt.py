"""csp_minsnap_optimize_times_periodic_batch on the MI355X: invariants per loop against the dense
reference tests/periodic_timeopt_ref.py, the start's and the final cost against tests/periodic_ref.py and the periodic
solve's own cost, symmetric closed forms, edges, bad lanes, determinism and memory (tests/guarded.py).

Loops are ref.make_loop's: points around a wobbly circle in angular order, far from the origin, times U(0.5, 2).
Settings min_time 0.1, tol 1e-6, 300 iterations.  B = 70 is one full wave and a partial one.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import guarded
from tests import periodic_timeopt_ref as ref
from tests.test_gpu_knots_timeopt import GATE_F
from tests.test_gpu_periodic import GATE_J
from tests.timeopt_ref import NOT_CONVERGED, pg_measure, project

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NONFINITE, NOT_SPD, SKIPPED = 1, 2, 4
ORDERS = (2, 3, 4, 5)
B = 70
RAGGED_B = 40
TMIN, TOL, MAX_ITERS = 0.1, 1e-6, 300
# uniform S -> the mode it runs in (S = 1 with the fixed total has nothing to optimise)
MODE = {1: "time_penalty", 2: "fixed_total", 3: "time_penalty", 6: "fixed_total"}
ULP64 = 64 * 2.0 ** -52
_FINAL_COST = {}   # order -> {batch tag: (e_new, e_old)}, filled by the invariant tests, read by test_final_cost_per_order


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


# ----------------------------------------------------------------------------------------------------------------- inputs

def uniform_cases(order, S, rows=B, seed=0):
    return [ref.make_loop(order, S, b, seed) for b in range(rows)]


def ragged_cases(order, seed=0):
    lens = np.random.default_rng([order, seed, 77]).integers(1, 10, size=RAGGED_B)
    return [ref.make_loop(order, int(s), b, seed) for b, s in enumerate(lens)]


def ragged_weights(order):
    return np.random.default_rng(order).uniform(0.0, 0.3, size=RAGGED_B)


def stack(cases):
    return tuple(np.ascontiguousarray(np.stack([c[i] for c in cases])) for i in range(2))


def concat(cases):
    off = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])]).astype(np.int64)
    return tuple(np.ascontiguousarray(np.concatenate([c[i] for c in cases])) for i in range(2)) + (off,)


@functools.lru_cache(maxsize=None)
def _ref_optimum(order, S, row, seed, mode, rho, w, f32):
    """The reference optimiser's final objective of one loop; computed once per loop, never changed."""
    p, t = ref.make_loop(order, S, row, seed)
    if f32:
        p, t = (a.astype(np.float32).astype(np.float64) for a in (p, t))
    return ref.optimize(order, p, t, w, mode, rho, TMIN, TOL, MAX_ITERS)["f"]


def check_batch(csp, order, cases, r, parent0, parentT, mode, rho, w=0.0, f32=False, check_ref=4, seed=0, tag=""):
    """Per loop: no status bit but NOT_CONVERGED, final <= initial, T >= min_time, the fixed total, the start objective
    against the reference (GATE_J) and the periodic solve's own cost (2 GATE_J), stationarity of converged fp64 lanes from
    the reference gradient (2 tol), the final objective of the first `check_ref` loops against the reference optimiser's
    (GATE_F).  parent0 / parentT: solve_periodic_batch's cost at the start and at the returned times.  Returns (converged
    count, e_new, e_old): the worst deviation from the reference at the returned times of the optimiser's final objective
    and of the periodic solve's own cost there, which test_final_cost_per_order gates."""
    T, obj, st = (_host(x) for x in (r.times, r.objective, r.status))
    T = T.reshape(-1).astype(np.float64)
    wv = np.broadcast_to(np.asarray(w, dtype=np.float64), (len(cases),))
    rd = (lambda a: np.asarray(a).astype(np.float32).astype(np.float64)) if f32 else (lambda a: np.asarray(a, dtype=np.float64))
    pen = rho if mode == "time_penalty" else 0.0
    pos = nconv = 0
    e_new = e_old = e_start = 0.0
    for b, (p, t) in enumerate(cases):
        p, t = rd(p), rd(t)
        S = len(t)
        tb = T[pos:pos + S]
        pos += S
        assert st[b] & ~NOT_CONVERGED == 0, (b, st[b])
        assert obj[b, 1] <= obj[b, 0], (b, obj[b])
        assert tb.min() >= TMIN, (b, tb.min())
        total = t.sum() if mode == "fixed_total" else None
        if total is not None:
            assert abs(tb.sum() - total) <= (1e-6 if f32 else 1e-12) * total, (b, tb.sum(), total)
        J0, _ = ref.cost_grad(order, p, t, wv[b])
        f0 = J0 + pen * t.sum()
        J, g = ref.cost_grad(order, p, tb, wv[b])
        f = J + pen * tb.sum()
        if S == 1:   # one knot: J = 0 exactly, the objective is the penalty alone
            assert abs(J0) <= 1e-20 and abs(J) <= 1e-20
            assert obj[b, 0] == pen * t.sum() and abs(obj[b, 1] - pen * tb.sum()) <= (2.0 ** -23 if f32 else 0.0) * pen * tb.sum()
        else:
            e_start = max(e_start, abs(obj[b, 0] - f0) / f0)
            assert abs(obj[b, 0] - f0) <= GATE_J[order] * f0, (b, obj[b, 0], f0)
            assert abs(obj[b, 0] - (parent0[b] + pen * t.sum())) <= 2 * GATE_J[order] * f0, (b, obj[b, 0], parent0[b])
            e_new = max(e_new, abs(obj[b, 1] - f) / f)
            e_old = max(e_old, abs(parentT[b] + pen * tb.sum() - f) / f)
        if st[b] == 0:
            nconv += 1
            if not f32:   # the reference's gradient has its own rounding: a 2x margin on the measure
                pg = pg_measure(tb, g + pen, t.mean(), obj[b, 0] if obj[b, 0] > 0 else 1.0, TMIN, total)
                assert pg <= 2 * TOL, (b, pg)
        if b < check_ref:
            fr = _ref_optimum(order, S, b, seed, mode, float(rho), float(wv[b]), f32)
            assert abs(fr - obj[b, 1]) <= GATE_F[order] * fr, (b, fr, obj[b, 1])
    print("%s: start vs reference %.2e; at the returned times optimiser %.2e, periodic solve %.2e; converged %d / %d"
          % (tag, e_start, e_new, e_old, nconv, len(cases)))
    return nconv, e_new, e_old


def check_cap(order, nconv, total, tag):
    """NOT_CONVERGED on at most 1/4 of a batch (3/8 at order 5): a condition of the issue, not a measurement."""
    allowed = total * 3 // 8 if order == 5 else total // 4
    assert total - nconv <= allowed, (tag, nconv, total)


# ------------------------------------------------------------------------------------------- 1, 2. invariants and costs

@pytest.mark.parametrize("S", [1, 2, 3, 6])
@pytest.mark.parametrize("order", ORDERS)
def test_invariants_uniform(csp, order, S):
    cases = uniform_cases(order, S)
    wp, tm = stack(cases)
    mode = MODE[S]
    rho = ref.penalty_weight(order, cases) if mode == "time_penalty" else 0.0
    d_wp, d_tm = _dev(wp), _dev(tm)
    r = csp.optimize_times_periodic_batch(d_wp, d_tm, order=order, mode=mode, time_weight=rho, min_time=TMIN, tol=TOL,
                                          max_iters=MAX_ITERS)
    p0 = csp.solve_periodic_batch(d_wp, d_tm, order=order, want_cost=True)
    pT = csp.solve_periodic_batch(d_wp, r.times, order=order, want_cost=True)
    torch.cuda.synchronize()
    assert torch.equal(r.coeffs, pT.coeffs)
    tag = "o%d S%d %s" % (order, S, mode)
    nconv, e_new, e_old = check_batch(csp, order, cases, r, _host(p0.cost), _host(pT.cost), mode, rho, tag=tag)
    _FINAL_COST.setdefault(order, {})[tag] = (e_new, e_old)
    check_cap(order, nconv, B, tag)
    if S == 1:   # J = 0 for every T: the time runs to the bound, exactly
        assert np.all(_host(r.times) == TMIN) and np.all(_host(r.objective)[:, 1] == rho * TMIN)
        assert not _host(r.status).any()
    if S == 3:
        # homogeneity at an interior optimum (w = 0): J has degree 1 - 2o in the times, so (2o-1) J = rho sum T there
        T, obj, st = _host(r.times), _host(r.objective), _host(r.status)
        sel = (st == 0) & (T.min(axis=1) > TMIN)
        J = obj[:, 1] - rho * T.sum(axis=1)
        h = np.abs((2 * order - 1) * J - rho * T.sum(axis=1)) / obj[:, 1]
        print("%s: homogeneity %.2e on %d lanes" % (tag, h[sel].max(), sel.sum()))
        assert sel.sum() >= B // 2 and h[sel].max() <= (1e-3 if order == 5 else 1e-4)


@pytest.mark.parametrize("mode", ["fixed_total", "time_penalty"])
@pytest.mark.parametrize("order", ORDERS)
def test_invariants_ragged_device_and_host_f32(csp, order, mode):
    cases = ragged_cases(order)
    wp, tm, off = concat(cases)
    w = ragged_weights(order)
    rho = ref.penalty_weight(order, cases, w) if mode == "time_penalty" else 0.0
    kw = dict(order=order, mode=mode, time_weight=rho, min_time=TMIN, tol=TOL, max_iters=MAX_ITERS)
    d = dict(seg_offsets=_dev(off), vel_zero_weight_per_traj=_dev(w))
    r = csp.optimize_times_periodic_batch(_dev(wp), _dev(tm), **kw, **d)
    p0 = csp.solve_periodic_batch(_dev(wp), _dev(tm), order=order, want_cost=True, **d)
    pT = csp.solve_periodic_batch(_dev(wp), r.times, order=order, want_cost=True, **d)
    torch.cuda.synchronize()
    tag = "o%d ragged device %s" % (order, mode)
    nconv, e_new, e_old = check_batch(csp, order, cases, r, _host(p0.cost), _host(pT.cost), mode, rho, w, tag=tag)
    _FINAL_COST.setdefault(order, {})[tag] = (e_new, e_old)
    check_cap(order, nconv, RAGGED_B, tag)
    # fp32 storage, host memory: fp64 arithmetic, the returned times rounded to fp32
    f = np.float32
    h = dict(seg_offsets=off, vel_zero_weight_per_traj=w)
    r32 = csp.optimize_times_periodic_batch(wp.astype(f), tm.astype(f), **kw, **h)
    assert r32.times.dtype == f and r32.coeffs.dtype == f
    p0 = csp.solve_periodic_batch(wp.astype(f), tm.astype(f), order=order, want_cost=True, **h)
    pT = csp.solve_periodic_batch(wp.astype(f), r32.times, order=order, want_cost=True, **h)
    assert np.array_equal(r32.coeffs, pT.coeffs)
    tag = "o%d ragged host fp32 %s" % (order, mode)
    nconv, e_new, e_old = check_batch(csp, order, cases, r32, p0.cost, pT.cost, mode, rho, w, f32=True, tag=tag)
    check_cap(order, nconv, RAGGED_B, tag)
    # the objective is the kernel's evaluation at the fp64 iterate, the reference sees the times rounded to fp32: J moves
    # by (2o-1) 2^-24 per time
    assert e_new <= max(4 * e_old, (2 * order - 1) * 2.0 ** -23), (tag, e_new, e_old)


@pytest.mark.parametrize("order", ORDERS)
def test_final_cost_per_order(csp, order):
    """J at the returned times, where the optimum's spread of times reaches 16: the optimiser's final objective against
    the reference there, at most 4x the deviation of solve_periodic_batch's own cost at those same times (a second,
    differently ordered summation of the same quantities; floor 64 ulp).  Both are the worst over the order's fp64
    batches above -- uniform S = 2, 3, 6 and the two ragged device batches -- which those tests measured; a batch that has
    not run yet (this test selected alone) is run here.  Measured, optimiser / periodic solve at orders 2..5: 6.2e-15 /
    6.2e-15, 1.6e-13 / 3.5e-13, 1.1e-11 / 2.1e-10, 1.0e-9 / 7.4e-6.  The worst lane of a single batch is the rounding
    noise of one summation order against another (each kernel is the closer one on some lanes), which is why the two
    are compared per order and not per batch."""
    want = ["o%d S%d %s" % (order, S, MODE[S]) for S in (2, 3, 6)] + ["o%d ragged device %s" % (order, m)
                                                                      for m in ("fixed_total", "time_penalty")]
    have = _FINAL_COST.setdefault(order, {})
    for S in (2, 3, 6):
        if want[(2, 3, 6).index(S)] not in have:
            test_invariants_uniform(csp, order, S)
    for m in ("fixed_total", "time_penalty"):
        if "o%d ragged device %s" % (order, m) not in have:
            test_invariants_ragged_device_and_host_f32(csp, order, m)
    e_new = max(have[k][0] for k in want)
    e_old = max(have[k][1] for k in want)
    print("o%d final cost against the reference: optimiser %.2e, periodic solve %.2e" % (order, e_new, e_old))
    assert e_new <= max(4 * e_old, ULP64), (order, e_new, e_old, have)


# ------------------------------------------------------------------------------------------------------- 3. closed forms

@pytest.mark.parametrize("order", ORDERS)
def test_symmetric_loops_return_to_equal_times(csp, order):
    """S = 2 there-and-back and the regular hexagon with the fixed total: equal times within 1e-5 relative, the final J
    within 1e-9 of J at equal times (the stopping measure, not the arithmetic, sets both)."""
    for name, path in (("there-and-back", ref.there_and_back()), ("hexagon", ref.hexagon())):
        S = len(path)
        t0 = ref.closed_form_start(order, S, "fixed_total")
        mean = t0.sum() / S
        wp = np.stack([path, path])
        tm = np.stack([t0, np.full(S, mean)])   # the second lane starts at the optimum
        r = csp.optimize_times_periodic_batch(_dev(wp), _dev(tm), order=order, min_time=TMIN, tol=TOL, max_iters=MAX_ITERS,
                                              want_coeffs=False)
        torch.cuda.synchronize()
        T, obj, st, it = (_host(x) for x in (r.times, r.objective, r.status, r.iterations))
        assert not st.any(), st
        assert it[1] == 0 and T[1].tobytes() == tm[1].tobytes()
        Jeq = obj[1, 0]
        et, ej = np.max(np.abs(T[0] - mean)) / mean, abs(obj[0, 1] - Jeq) / Jeq
        print("o%d %s: times %.2e  J %.2e  (%d iterations)" % (order, name, et, ej, it[0]))
        assert et <= 1e-5 and ej <= 1e-9


@pytest.mark.parametrize("order", ORDERS)
def test_hexagon_time_penalty_closed_form(csp, order):
    """Equal times t on the hexagon: J(t) = J(1) t^(1-2o), so every time is t* = ((2o-1) J(1) / (rho S))^(1/2o)."""
    path, S = ref.hexagon(), 6
    J1 = float(csp.solve_periodic_batch(path[None], np.ones((1, S)), order=order, want_cost=True).cost[0])
    rho = J1 / S
    t0 = ref.closed_form_start(order, S, "time_penalty")
    r = csp.optimize_times_periodic_batch(path[None], t0[None], order=order, mode="time_penalty", time_weight=rho,
                                          min_time=TMIN, tol=TOL, max_iters=MAX_ITERS, want_coeffs=False)
    assert not (r.status & ~NOT_CONVERGED).any(), r.status
    want = ((2 * order - 1) * J1 / (rho * S)) ** (1.0 / (2 * order))
    err = np.max(np.abs(r.times - want)) / want
    print("o%d hexagon, time penalty: %.2e  (%d iterations, status %d)" % (order, err, r.iterations[0], r.status[0]))
    assert err <= (1e-3 if order == 5 else 1e-4), (r.times, want)


# ------------------------------------------------------------------------------------------------------------- 4. edges

@pytest.mark.parametrize("order", ORDERS)
def test_single_segment_fixed_total_is_bit_identical(csp, order):
    wp, tm = stack(uniform_cases(order, 1, seed=700))
    r = csp.optimize_times_periodic_batch(_dev(wp), _dev(tm), order=order, min_time=TMIN, vel_zero_weight=0.2)
    torch.cuda.synchronize()
    assert _host(r.times).tobytes() == tm.tobytes()
    assert not _host(r.status).any() and not _host(r.iterations).any()
    assert not _host(r.objective).any()   # J = 0 for one knot, whatever w


def test_max_iters_zero_returns_the_start(csp):
    wp, tm = stack(uniform_cases(4, 6, seed=600))
    r = csp.optimize_times_periodic_batch(wp, tm, order=4, min_time=TMIN, max_iters=0)
    assert np.array_equal(r.times, tm)
    assert np.all(r.status == NOT_CONVERGED) and not r.iterations.any()
    assert np.array_equal(r.objective[:, 0], r.objective[:, 1])
    # a start that is already stationary (the hexagon at equal times) is converged, not cut off
    r = csp.optimize_times_periodic_batch(ref.hexagon()[None], np.full((1, 6), 1.25), order=4, min_time=TMIN, max_iters=0)
    assert r.status[0] == 0 and r.iterations[0] == 0 and np.all(r.times == 1.25)


@pytest.mark.parametrize("order", ORDERS)
def test_one_iteration_strictly_decreases(csp, order):
    wp, tm = stack(uniform_cases(order, 6, seed=500))
    r = csp.optimize_times_periodic_batch(wp, tm, order=order, min_time=TMIN, tol=1e-12, max_iters=1, want_coeffs=False)
    assert np.all(r.status == NOT_CONVERGED) and np.all(r.iterations == 1)
    assert np.all(r.objective[:, 1] < r.objective[:, 0])


def test_coincident_waypoints_and_projected_start(csp):
    """Every waypoint the same point: J = 0 for all times, the gradient is 0 and the start -- the projection of an input
    with an entry below min_time -- is stationary: returned with objectives 0, status 0, iterations 0.  On a real loop
    the same input starts from the same projection (max_iters = 0 returns it)."""
    tm = np.array([[0.9, 0.02, 1.4, 0.7, -0.3]])
    want = project(tm[0], TMIN, tm[0].sum())
    assert want.min() == TMIN and abs(want.sum() - tm[0].sum()) < 1e-15
    wp = np.tile(np.array([[3.0, -2.0, 7.5]]), (1, 5, 1))
    r = csp.optimize_times_periodic_batch(wp, tm, order=4, min_time=TMIN)
    assert r.status[0] == 0 and r.iterations[0] == 0 and not r.objective.any()
    assert np.max(np.abs(r.times[0] - want)) <= 4 * 2.0 ** -52 and r.times.min() == TMIN
    path = ref.make_loop(4, 5, 0, seed=800)[0]
    r = csp.optimize_times_periodic_batch(path[None], tm, order=4, min_time=TMIN, max_iters=0)
    assert r.status[0] == NOT_CONVERGED and np.max(np.abs(r.times[0] - want)) <= 4 * 2.0 ** -52
    J = csp.solve_periodic_batch(path[None], r.times, order=4, want_cost=True).cost[0]
    assert abs(r.objective[0, 0] - J) <= 2 * GATE_J[4] * J


def test_empty_batch(csp):
    wp, tm = np.zeros((0, 4, 3)), np.zeros((0, 4))
    assert csp.optimize_times_periodic_batch(wp, tm).times.shape == (0, 4)
    r = csp.optimize_times_periodic_batch(_dev(wp), _dev(tm))
    torch.cuda.synchronize()
    assert r.times.shape == (0, 4) and r.coeffs.shape == (0, 4, 3, 8)


# ------------------------------------------------------------------------------------------------------------ 8. memory

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
    need = csp.periodic_timeopt_workspace_bytes(desc)
    smax = max_segments if ragged else uniform_S
    assert need == ((smax - 1) * (2 * n * n + 3 * n) * Bn * 8 + 255) // 256 * 256 + 4 * smax * Bn * 8
    ws = guarded.Guarded(need, DEV, name="workspace").fill(fill)
    prm = csp.make_timeopt_params(csp.TIMEOPT_FIXED_TOTAL if mode == "fixed_total" else csp.TIMEOPT_TIME_PENALTY, rho, TMIN,
                                  TOL, max_iters)
    rc = csp.raw_lib().csp_minsnap_optimize_times_periodic_batch(
        ctypes.byref(desc), ctypes.byref(prm), ins["waypoints"].data_ptr(), ins["times"].data_ptr(), outs["times"].data_ptr(),
        outs["coeffs"].data_ptr(), outs["objective"].data_ptr(), outs["iterations"].data_ptr(), outs["status"].data_ptr(),
        ws.data_ptr(), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, csp.strerror(rc))
    torch.cuda.synchronize()
    for g in [ws] + list(ins.values()) + list(outs.values()):
        g.check()
    for k, g in ins.items():
        assert g.bytes().tobytes() == np.ascontiguousarray(host[k]).tobytes(), (k, "an input changed")
    fl = np.float32 if f32 else np.float64
    return dict(times=outs["times"].numpy(fl), coeffs=outs["coeffs"].numpy(fl), objective=outs["objective"].numpy(np.float64, (-1, 2)),
                iterations=outs["iterations"].numpy(np.int32), status=outs["status"].numpy(np.int32))


class _HostBand:
    """A numpy payload between two pattern bands (the host-memory counterpart of guarded.Guarded)."""
    BAND = 4096

    def __init__(self, nbytes, fill):
        self.n = int(nbytes)
        self.buf = np.full(self.n + 2 * self.BAND, guarded.PATTERN, dtype=np.uint8)
        self.buf[self.BAND:self.BAND + self.n] = fill

    def ptr(self):
        return self.buf.ctypes.data + self.BAND

    def view(self, dtype, shape=(-1,)):
        return self.buf[self.BAND:self.BAND + self.n].view(dtype).reshape(shape).copy()

    def check(self):
        assert (self.buf[:self.BAND] == guarded.PATTERN).all() and (self.buf[self.BAND + self.n:] == guarded.PATTERN).all()


def _host_call(csp, order, host, uniform_S, max_segments, fill, f32, mode="fixed_total", rho=0.0, max_iters=40):
    """The same call with host memory (no workspace: staged), every output between two bands."""
    Bn = host["vw"].shape[0]
    total = host["times"].size
    elt = 4 if f32 else 8
    ins = {k: np.ascontiguousarray(v).copy() for k, v in host.items()}
    outs = {"times": _HostBand(total * elt, fill), "coeffs": _HostBand(total * 3 * 2 * order * elt, fill),
            "objective": _HostBand(Bn * 16, fill), "iterations": _HostBand(Bn * 4, fill), "status": _HostBand(Bn * 4, fill)}
    ragged = uniform_S is None
    desc = csp.make_desc(order, Bn, 0 if ragged else uniform_S, csp.DTYPE_F32 if f32 else csp.DTYPE_F64, 0.0, 0.0, csp.MEM_HOST,
                         False, ins["seg_offsets"].ctypes.data if ragged else None, max_segments if ragged else 0,
                         ins["vw"].ctypes.data)
    prm = csp.make_timeopt_params(csp.TIMEOPT_FIXED_TOTAL if mode == "fixed_total" else csp.TIMEOPT_TIME_PENALTY, rho, TMIN,
                                  TOL, max_iters)
    rc = csp.raw_lib().csp_minsnap_optimize_times_periodic_batch(
        ctypes.byref(desc), ctypes.byref(prm), ins["waypoints"].ctypes.data, ins["times"].ctypes.data, outs["times"].ptr(),
        outs["coeffs"].ptr(), outs["objective"].ptr(), outs["iterations"].ptr(), outs["status"].ptr(), None, 0, None)
    assert rc == 0, (rc, csp.strerror(rc))
    for g in outs.values():
        g.check()
    for k, v in ins.items():
        assert v.tobytes() == np.ascontiguousarray(host[k]).tobytes(), (k, "an input changed")
    fl = np.float32 if f32 else np.float64
    return dict(times=outs["times"].view(fl), coeffs=outs["coeffs"].view(fl), objective=outs["objective"].view(np.float64, (-1, 2)),
                iterations=outs["iterations"].view(np.int32), status=outs["status"].view(np.int32))


def _same_over_fills(csp, order, host, uniform_S, max_segments, f32, mode="fixed_total", rho=0.0):
    """0xFF bytes are NaN in every float slot, 0x3F bytes stale finite numbers (4.8e-4 as a double): both as the start of
    the workspace and of every output, device and host memory; every output has the same bits in all four calls."""
    runs = [_guarded_call(csp, order, host, uniform_S, max_segments, fill, f32, mode, rho) for fill in (0xFF, 0x3F)]
    runs += [_host_call(csp, order, host, uniform_S, max_segments, fill, f32, mode, rho) for fill in (0xFF, 0x3F)]
    for other in runs[1:]:
        for k in runs[0]:
            assert runs[0][k].tobytes() == other[k].tobytes(), (uniform_S, k, "differs between fills or memory spaces")
    assert not (runs[0]["status"] & ~NOT_CONVERGED).any()
    return runs[0]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("order", ORDERS)
def test_guard_bands_and_stale_workspace_uniform(csp, order, f32):
    fl = np.float32 if f32 else np.float64
    for S in (1, 2, 6):
        wp, tm = stack(uniform_cases(order, S, seed=1200))
        host = dict(waypoints=wp.astype(fl), times=tm.astype(fl), vw=np.zeros(B))
        mode, rho = ("time_penalty", 5.0) if S == 1 else ("fixed_total", 0.0)
        _same_over_fills(csp, order, host, S, None, f32, mode, rho)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("order", ORDERS)
def test_guard_bands_and_stale_workspace_ragged(csp, order, f32):
    fl = np.float32 if f32 else np.float64
    wp, tm, off = concat(ragged_cases(order, seed=1300))
    host = dict(waypoints=wp.astype(fl), times=tm.astype(fl), seg_offsets=off, vw=ragged_weights(order))
    _same_over_fills(csp, order, host, None, 9, f32)


# ------------------------------------------------------------------------------------------- 5. ragged edges on the device

@pytest.mark.parametrize("order", ORDERS)
def test_ragged_edges_on_the_device(csp, order):
    """A ragged device batch with max_segments = 5 (the workspace, guard-banded, sized for 5): the 9-segment loop is
    CSP_TRAJ_SKIPPED with its times copied through, NaN objectives and iterations 0, and the coefficient launch of such a
    batch writes nothing (no band is touched, every coefficient byte is the fill); S_b = 0 gets status 0, objectives 0 and
    iterations 0; a loop whose fixed total is infeasible is returned unchanged with CSP_TRAJ_NOT_CONVERGED, NaN objectives
    and iterations 0; every other output of every other loop has the bits of the call with max_segments = 9."""
    lens = (3, 0, 9, 5, 1, 0, 2, 4)
    cases = [ref.make_loop(order, s, b, 900) if s else (np.zeros((0, 3)), np.zeros(0)) for b, s in enumerate(lens)]
    cases[7] = (cases[7][0], np.array([0.01, 0.2, 0.05, 0.02]))   # sum 0.28 < 4 * 0.1
    wp, tm, off = concat(cases)
    host = dict(waypoints=wp, times=tm, seg_offsets=off, vw=np.zeros(len(lens)))
    full = _guarded_call(csp, order, host, None, 9, 0xFF, False)
    short = _guarded_call(csp, order, host, None, 5, 0xFF, False)
    M = 2 * order
    assert (short["coeffs"].view(np.uint8) == 0xFF).all(), "coefficients written although a loop was skipped"
    solo = csp.solve_periodic_batch(_dev(wp), _dev(full["times"]), order=order, seg_offsets=_dev(off), max_segments=9)
    torch.cuda.synchronize()
    assert np.array_equal(full["coeffs"].reshape(-1, 3, M), _host(solo.coeffs))
    for i, s in enumerate(lens):
        sl = slice(off[i], off[i + 1])
        if s > 5:
            assert short["status"][i] == SKIPPED and short["iterations"][i] == 0 and np.isnan(short["objective"][i]).all()
            assert short["times"][sl].tobytes() == tm[sl].tobytes()
            assert full["status"][i] & ~NOT_CONVERGED == 0
        else:
            for k in ("times", "objective", "iterations", "status"):
                a, b = ((x[k].reshape(len(lens), -1)[i] if k != "times" else x[k][sl]) for x in (short, full))
                assert a.tobytes() == b.tobytes(), (i, k)
        if s == 0:
            assert short["status"][i] == 0 and short["iterations"][i] == 0 and not short["objective"][i].any()
    assert full["status"][7] == NOT_CONVERGED and full["iterations"][7] == 0 and np.isnan(full["objective"][7]).all()
    assert full["times"][off[7]:off[8]].tobytes() == tm[off[7]:off[8]].tobytes()


# ------------------------------------------------------------------------------------------------------- 6. bad lanes

@pytest.mark.parametrize("order", ORDERS)
def test_bad_lanes_change_no_other_lane(csp, order):
    """A NaN time: CSP_TRAJ_NONFINITE, returned unchanged, NaN objectives.  An inf waypoint: the loop stops at the start
    with CSP_TRAJ_NONFINITE, times = the start, iterations 0.  A zero time is below min_time, not an error: the start is
    the projection and the loop is optimised.  Every other lane has the bits of the run without them."""
    wp, tm = stack(uniform_cases(order, 3, seed=1000))
    kw = dict(order=order, min_time=TMIN, max_iters=60)
    good = csp.optimize_times_periodic_batch(_dev(wp), _dev(tm), **kw)
    wp2, tm2 = wp.copy(), tm.copy()
    tm2[5, 1] = np.nan
    wp2[9, 2, 1] = np.inf
    tm2[66, 0] = 0.0
    r = csp.optimize_times_periodic_batch(_dev(wp2), _dev(tm2), **kw)
    torch.cuda.synchronize()
    keep = np.setdiff1d(np.arange(B), [5, 9, 66])
    for name in ("times", "coeffs", "objective", "iterations", "status"):
        a, g = _host(getattr(r, name)), _host(getattr(good, name))
        assert a[keep].tobytes() == g[keep].tobytes(), name
    st, it, T, obj = _host(r.status), _host(r.iterations), _host(r.times), _host(r.objective)
    assert st[5] == NONFINITE and it[5] == 0 and T[5].tobytes() == tm2[5].tobytes() and np.isnan(obj[5]).all()
    assert st[9] & NONFINITE and it[9] == 0 and T[9].tobytes() == tm[9].tobytes()
    assert st[66] & ~NOT_CONVERGED == 0 and T[66].min() >= TMIN and abs(T[66].sum() - tm2[66].sum()) <= 1e-12 * tm2[66].sum()
    assert obj[66, 1] <= obj[66, 0] and np.isfinite(obj[66]).all()


# --------------------------------------------------------------------------------- 7. determinism and the coefficients

@pytest.mark.parametrize("order", (3, 4, 5))
def test_deterministic_and_coeffs_are_the_periodic_solve(csp, order):
    wp, tm = stack(uniform_cases(order, 6, seed=1100))
    d = [_dev(x) for x in (wp, tm)]
    kw = dict(order=order, min_time=TMIN, max_iters=50, vel_zero_weight=0.1)
    r1 = csp.optimize_times_periodic_batch(*d, **kw)
    r2 = csp.optimize_times_periodic_batch(*d, **kw)
    torch.cuda.synchronize()
    solo = csp.solve_periodic_batch(d[0], r1.times, order=order, vel_zero_weight=0.1)
    torch.cuda.synchronize()
    assert torch.equal(r1.coeffs, solo.coeffs)
    names = ("times", "coeffs", "objective", "iterations", "status")
    for nm in names:
        assert torch.equal(getattr(r1, nm), getattr(r2, nm)), nm
    rh = csp.optimize_times_periodic_batch(wp, tm, **kw)
    for nm in names:
        assert getattr(rh, nm).tobytes() == _host(getattr(r1, nm)).tobytes(), nm
