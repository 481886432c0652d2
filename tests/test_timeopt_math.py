"""CPU checks of the segment-time optimisation: the numpy restatement (tests/timeopt_ref.py) of the cost
and its envelope gradient against the 80-bit oracle, the reference optimiser against scipy's SLSQP, and the C-ABI surface
of csp_minsnap_cost_batch / csp_minsnap_optimize_times_batch without a device."""
import ctypes

import numpy as np
import pytest

from tests import synth
from tests.conftest import load_cases
from tests.timeopt_ref import cost_from_coeffs, cost_grad, optimize, project


def _oracle_cost(oracle_mod, order, path, time, bc, w):
    c, _ = oracle_mod.solve_batch(order, np.asarray(path)[None], np.asarray(time)[None], np.asarray(bc)[None],
                                  vel_zero_weight=w, long_double=True)
    return cost_from_coeffs(order, c[0], time, w)


def _richardson(oracle_mod, order, path, time, bc, w):
    """dJ/dT_j by central differences of the oracle's cost at h = 1e-3 T_j and h / 2, Richardson-extrapolated."""
    time = np.asarray(time, dtype=np.float64)
    g = np.zeros(len(time))
    for j in range(len(time)):
        h = 1e-3 * time[j]
        vals = []
        for f in (1.0, 0.5):
            e = np.zeros(len(time))
            e[j] = f * h
            vals.append((_oracle_cost(oracle_mod, order, path, time + e, bc, w)
                         - _oracle_cost(oracle_mod, order, path, time - e, bc, w)) / (2 * f * h))
        g[j] = (4 * vals[1] - vals[0]) / 3
    return g


@pytest.mark.parametrize("order", [2, 3, 4, 5])
@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("w", [0.0, 0.3])
def test_cost_and_gradient_match_oracle(oracle_mod, order, S, w):
    wp, tm = synth.make_batch(1, S, config_id=3, offset=order)
    bc = np.random.default_rng(10 * order + S).normal(size=(4, 3))
    J, g = cost_grad(order, wp[0], tm[0], bc, w)
    Jo = _oracle_cost(oracle_mod, order, wp[0], tm[0], bc, w)
    assert abs(J - Jo) <= 1e-9 * abs(Jo), (J, Jo)
    fd = _richardson(oracle_mod, order, wp[0], tm[0], bc, w)
    err = np.max(np.abs(g - fd)) / np.max(np.abs(fd))
    # measured: <= 6e-10 at orders 2..4, 2e-8 at order 5 (the dense fp64 inverses of M, as tests/test_vjp_math.py)
    assert err < (1e-6 if order == 5 else 1e-8), err


def test_cost_and_gradient_golden_f3(oracle_mod):
    cases = load_cases("F3_wellscaled.json")
    assert cases
    for c in cases:
        J, g = cost_grad(c["order"], c["path"], c["time"], c["bc"])
        Jo = cost_from_coeffs(c["order"], c["coeff"], c["time"])
        assert abs(J - Jo) <= 1e-8 * abs(Jo), (J, Jo)
        fd = _richardson(oracle_mod, c["order"], c["path"], c["time"], c["bc"], 0.0)
        assert np.max(np.abs(g - fd)) / np.max(np.abs(fd)) < 1e-7


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_euler_identity_zero_bc(order):
    """With zero bc and w = 0, J is homogeneous of degree 1 - 2o in T: sum_j T_j dJ/dT_j = (1 - 2o) J."""
    wp, tm = synth.make_batch(1, 6, config_id=3, offset=11 * order)
    J, g = cost_grad(order, wp[0], tm[0], np.zeros((4, 3)))
    assert abs(tm[0] @ g - (1 - 2 * order) * J) <= 1e-9 * abs(J)


def test_projection():
    rng = np.random.default_rng(5)
    for _ in range(200):
        S = int(rng.integers(1, 12))
        v = rng.normal(size=S) * rng.uniform(0.1, 10)
        lo = 0.1
        total = lo * S + rng.uniform(0, 5)
        y = project(v, lo, total)
        assert abs(y.sum() - total) <= 1e-12 * total and y.min() >= lo
        # KKT: y_j = max(v_j - theta, lo) with one theta
        act = y > lo
        if act.any():
            th = v[act] - y[act]
            assert np.ptp(th) < 1e-12 * (1 + np.abs(th).max())
            assert np.all(v[~act] - th[0] <= lo + 1e-12)


@pytest.mark.parametrize("order,S", [(3, 4), (4, 8), (4, 16), (5, 4), (5, 16)])
def test_reference_optimiser_reaches_slsqp(order, S):
    opt = pytest.importorskip("scipy.optimize")
    wp, tm = synth.make_batch(1, S, config_id=3, offset=31 * order + S)
    bc = np.random.default_rng(order).normal(size=(4, 3)) * 0.5
    lo, total = 0.05, tm[0].sum()
    r = optimize(order, wp[0], tm[0], bc, mode="fixed_total", min_time=lo, tol=1e-6, max_iters=500)
    assert r["status"] == 0 and r["f"] <= r["f0"]
    assert abs(r["times"].sum() - total) <= 1e-12 * total and r["times"].min() >= lo
    # SLSQP in the same scaled variables (unscaled, it stops on "inequality constraints incompatible" at order 5)
    tau, f0 = total / S, r["f0"]
    fun = lambda x: cost_grad(order, wp[0], tau * x, bc)[0] / f0
    jac = lambda x: cost_grad(order, wp[0], tau * x, bc)[1] * tau / f0
    s = opt.minimize(fun, tm[0] / tau, jac=jac, method="SLSQP", bounds=[(lo / tau, None)] * S,
                     constraints=[{"type": "eq", "fun": lambda x: x.sum() - S, "jac": lambda x: np.ones(S)}],
                     options=dict(ftol=1e-16, maxiter=1000))
    assert s.success, s
    s.fun *= f0
    # tol = 1e-6 in the scaled measure: measured 1e-12 .. 8e-9 relative, 7.6e-8 at order 5, S = 16 (ill-conditioned)
    assert abs(r["f"] - s.fun) <= 2e-7 * s.fun, (r["f"], s.fun)


def test_reference_optimiser_time_penalty_closed_form():
    """S = 1, zero bc: J(T) = J(1) T^(1-2o), so J + rho T is minimal at T* = ((2o-1) J(1) / rho)^(1/(2o))."""
    wp, _ = synth.make_batch(1, 1, config_id=3)
    for order in (2, 3, 4, 5):
        J1 = cost_grad(order, wp[0], [1.0], np.zeros((4, 3)))[0]
        rho = 0.5 * J1
        r = optimize(order, wp[0], [1.0], np.zeros((4, 3)), mode="time_penalty", rho=rho, min_time=1e-3, tol=1e-10)
        Ts = ((2 * order - 1) * J1 / rho) ** (1.0 / (2 * order))
        assert r["status"] == 0 and abs(r["times"][0] - Ts) <= 1e-8 * Ts, (order, r, Ts)


def test_timeopt_symbols_exported(csp):
    for name in ("csp_minsnap_cost_batch", "csp_minsnap_cost_workspace_bytes", "csp_minsnap_optimize_times_batch",
                 "csp_minsnap_timeopt_workspace_bytes"):
        assert name in csp.EXPORTED_SYMBOLS
        assert getattr(ctypes.CDLL(csp.LIB_PATH), name)
    assert callable(csp.snap_cost_batch) and callable(csp.optimize_times_batch)


def _factors(order, smax, B):
    n = order - 1
    return (max(smax - 1, 0) * (n * n + 3 * n) * B * 8 + 255) // 256 * 256


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_workspace_formulas(csp, order):
    for S, B, per in [(16, 65536, False), (1, 100, False), (7, 3, True), (40, 129, False), (2, 1, True)]:
        d = csp.make_desc(order, B, S, bc_per_trajectory=per)
        assert csp.cost_workspace_bytes(d) == _factors(order, S, B), (S, B)
        assert csp.timeopt_workspace_bytes(d) == _factors(order, S, B) + 4 * S * B * 8, (S, B)
        # the coefficients' solve runs in the factor region
        assert csp.workspace_bytes(d) <= _factors(order, S, B)
    off = np.array([0, 3, 3, 10], dtype=np.int64)
    d = csp.make_desc(order, 3, 0, seg_offsets_ptr=off.ctypes.data, max_segments=7)
    assert csp.cost_workspace_bytes(d) == _factors(order, 7, 3)
    assert csp.timeopt_workspace_bytes(d) == _factors(order, 7, 3) + 4 * 7 * 3 * 8
    for bad in (csp.make_desc(1, 10, 4), csp.make_desc(4, 10, 4, path_weight=0.1), csp.make_desc(6, 10, 4),
                csp.make_desc(4, 10, 4, flags=csp.FLAG_SEGMENT_MAJOR)):
        assert csp.cost_workspace_bytes(bad) == 0 and csp.timeopt_workspace_bytes(bad) == 0


def _cost_args(wp, tm, bc, cost):
    return (wp.ctypes.data, tm.ctypes.data, bc.ctypes.data, cost.ctypes.data, None, None, None, 0, None)


def test_cost_codes(csp):
    """Argument checks come before the device check, so these hold on any machine."""
    f = csp.raw_lib().csp_minsnap_cost_batch
    wp, tm, bc, cost = np.zeros((2, 4, 3)), np.ones((2, 3)), np.zeros((1, 4, 3)), np.zeros(2)
    a = _cost_args(wp, tm, bc, cost)
    assert f(csp.make_desc(4, 2, 3, path_weight=0.5), *a) == -2
    assert f(csp.make_desc(1, 2, 3), *a) == -2
    assert f(csp.make_desc(4, 2, 3, flags=csp.FLAG_SEGMENT_MAJOR), *a) == -2
    assert f(csp.make_desc(4, 2, 3, dtype=csp.DTYPE_F32, flags=csp.FLAG_F32_ARITH), *a) == -2
    assert f(csp.make_desc(0, 2, 3), *a) == -1
    assert f(None, *a) == -1
    assert f(csp.make_desc(4, 2, 3), wp.ctypes.data, tm.ctypes.data, bc.ctypes.data, None, None, None, None, 0, None) == -1
    assert f(csp.make_desc(4, 0, 3), None, None, None, None, None, None, None, 0, None) == 0
    if csp.device_count() == 0:
        assert f(csp.make_desc(4, 2, 3), *a) == -5


def test_optimize_codes(csp):
    f = csp.raw_lib().csp_minsnap_optimize_times_batch
    wp, tm, bc, out = np.zeros((2, 4, 3)), np.ones((2, 3)), np.zeros((1, 4, 3)), np.zeros((2, 3))
    P = csp.make_timeopt_params

    def call(desc, prm, times=tm):
        return f(desc, None if prm is None else ctypes.byref(prm), wp.ctypes.data, times.ctypes.data, bc.ctypes.data,
                 out.ctypes.data, None, None, None, None, None, 0, None)
    d = csp.make_desc(4, 2, 3)
    assert call(csp.make_desc(4, 2, 3, path_weight=0.5), P()) == -2
    assert call(csp.make_desc(1, 2, 3), P()) == -2
    assert call(csp.make_desc(4, 2, 3, flags=csp.FLAG_SEGMENT_MAJOR), P()) == -2
    assert call(csp.make_desc(4, 2, 3, dtype=csp.DTYPE_F32, flags=csp.FLAG_F32_ARITH), P()) == -2
    assert call(d, None) == -1
    assert call(d, P(mode=csp.TIMEOPT_TIME_PENALTY, time_weight=0.0)) == -1
    assert call(d, P(mode=csp.TIMEOPT_TIME_PENALTY, time_weight=-1.0)) == -1
    assert call(d, P(min_time=0.0)) == -1
    assert call(d, P(min_time=-1.0)) == -1
    assert call(d, P(max_iters=-1)) == -1
    assert call(d, P(tol=-1.0)) == -1
    assert call(d, P(mode=7)) == -1
    bad = P()
    bad.abi_version = 2
    assert call(d, bad) == -1
    # sum T_in = 3 < S * min_time = 3 * 1.5 (the time penalty has no such limit)
    assert call(d, P(min_time=1.5)) == -1
    assert call(csp.make_desc(4, 0, 3), P()) == 0
    if csp.device_count() == 0:
        assert call(d, P()) == -5
        assert call(d, P(mode=csp.TIMEOPT_TIME_PENALTY, time_weight=1.0, min_time=1.5)) == -5
        with pytest.raises(csp.CspError) as e:
            csp.optimize_times_batch(wp, tm)
        assert e.value.code == -5
        with pytest.raises(csp.CspError) as e:
            csp.snap_cost_batch(wp, tm)
        assert e.value.code == -5
