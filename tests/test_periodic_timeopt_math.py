"""CPU checks of the lap-time optimisation of the periodic solve: the C-ABI surface of
csp_minsnap_optimize_times_periodic_batch without a device (every check comes before a device is looked for), and the
dense reference tests/periodic_timeopt_ref.py itself -- its gradient against central differences of J, Euler's identity
and the two symmetric closed forms the GPU tests hold the kernel to."""
import ctypes

import numpy as np
import pytest

from tests import periodic_timeopt_ref as ref

OK, INVALID_ARG, UNSUPPORTED, WORKSPACE, NO_DEVICE = 0, -1, -2, -3, -5
ORDERS = (2, 3, 4, 5)


# --------------------------------------------------------------------------------------------------------------- the C-ABI

def test_symbols_exported(csp):
    for name in ("csp_minsnap_optimize_times_periodic_batch", "csp_minsnap_periodic_timeopt_workspace_bytes"):
        assert name in csp.EXPORTED_SYMBOLS
        assert getattr(ctypes.CDLL(csp.LIB_PATH), name)
    assert callable(csp.optimize_times_periodic_batch) and callable(csp.periodic_timeopt_workspace_bytes)


def test_workspace_bytes_formula(csp):
    up = lambda v: (v + 255) // 256 * 256
    for order in ORDERS:
        n = order - 1
        for S, B in ((1, 1), (3, 4), (6, 70), (16, 65536), (9, 129)):
            want = up((S - 1) * (2 * n * n + 3 * n) * B * 8) + 4 * S * B * 8
            off = np.zeros(B + 1, dtype=np.int64)
            assert csp.periodic_timeopt_workspace_bytes(csp.make_desc(order, B, S)) == want
            assert csp.periodic_timeopt_workspace_bytes(csp.make_desc(order, B, 0, seg_offsets_ptr=off.ctypes.data,
                                                                      max_segments=S)) == want
            assert csp.periodic_timeopt_workspace_bytes(csp.make_desc(order, B, S, dtype=csp.DTYPE_F32)) == want
            # the coefficient launch runs in the factor region
            assert csp.periodic_workspace_bytes(csp.make_desc(order, B, S)) == want - 4 * S * B * 8
        assert csp.periodic_timeopt_workspace_bytes(csp.make_desc(order, 0, 6)) == 0
    bad_abi = csp.make_desc(4, 4, 3)
    bad_abi.abi_version = 99
    for bad in (csp.make_desc(1, 4, 3), csp.make_desc(6, 4, 3), csp.make_desc(4, 4, 3, path_weight=0.5),
                csp.make_desc(4, 4, 3, flags=csp.FLAG_SEGMENT_MAJOR),
                csp.make_desc(4, 4, 3, dtype=csp.DTYPE_F32, flags=csp.FLAG_F32_ARITH), bad_abi,
                csp.make_desc(4, 4, 0, max_segments=3)):   # ragged without offsets
        assert csp.periodic_timeopt_workspace_bytes(bad) == 0


def _p(a):
    return None if a is None else (a if isinstance(a, int) else a.ctypes.data)


def _call(csp, desc, prm, wp, tm, tout, co=None, ws=None, ws_bytes=0):
    return csp.raw_lib().csp_minsnap_optimize_times_periodic_batch(
        None if desc is None else ctypes.byref(desc), None if prm is None else ctypes.byref(prm), _p(wp), _p(tm), _p(tout),
        _p(co), None, None, None, _p(ws), ws_bytes, None)


def test_every_return_code_comes_back_without_a_device(csp):
    B, S, order = 4, 3, 4
    wp, tm = np.zeros((B, S, 3)), np.ones((B, S))
    tout = np.zeros_like(tm)
    P = csp.make_timeopt_params
    call = lambda d, prm, times=tm: _call(csp, d, prm, wp, times, tout)
    unsupported = {"order 1": csp.make_desc(1, B, S),
                   "order 6": csp.make_desc(6, B, S),
                   "path penalty": csp.make_desc(order, B, S, path_weight=0.5),
                   "segment major": csp.make_desc(order, B, S, flags=csp.FLAG_SEGMENT_MAJOR),
                   "f32 arithmetic": csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, flags=csp.FLAG_F32_ARITH)}
    for name, d in unsupported.items():
        assert call(d, P()) == UNSUPPORTED, name
    host = csp.make_desc(order, B, S)
    # the three required pointers, the parameters and the descriptor
    assert _call(csp, None, P(), wp, tm, tout) == INVALID_ARG
    assert _call(csp, host, None, wp, tm, tout) == INVALID_ARG
    assert _call(csp, host, P(), None, tm, tout) == INVALID_ARG
    assert _call(csp, host, P(), wp, None, tout) == INVALID_ARG
    assert _call(csp, host, P(), wp, tm, None) == INVALID_ARG
    # the descriptor's and the parameters' rules
    bad = csp.make_desc(order, B, S)
    bad.abi_version = 99
    assert call(bad, P()) == INVALID_ARG
    badp = P()
    badp.abi_version = 2
    assert call(host, badp) == INVALID_ARG
    assert call(host, P(mode=7)) == INVALID_ARG
    assert call(host, P(min_time=0.0)) == INVALID_ARG
    assert call(host, P(min_time=-1.0)) == INVALID_ARG
    assert call(host, P(tol=-1.0)) == INVALID_ARG
    assert call(host, P(max_iters=-1)) == INVALID_ARG
    assert call(host, P(mode=csp.TIMEOPT_TIME_PENALTY, time_weight=0.0)) == INVALID_ARG
    assert call(host, P(mode=csp.TIMEOPT_TIME_PENALTY, time_weight=-1.0)) == INVALID_ARG
    # a host fixed total below S * min_time: sum T_in = 3 < 3 * 1.5, in one trajectory of the batch
    assert call(host, P(min_time=1.5)) == INVALID_ARG
    short = tm.copy()
    short[2] = 0.1
    assert call(host, P(min_time=0.2), short) == INVALID_ARG
    # ragged host call: offsets outside 0..max_segments (a negative length, a length above max_segments)
    for off in ([0, 3, 2, 8, 12], [0, 3, 10, 11, 12]):
        off = np.array(off, dtype=np.int64)
        rag = csp.make_desc(order, B, 0, seg_offsets_ptr=off.ctypes.data, max_segments=6)
        assert _call(csp, rag, P(), np.zeros((12, 3)), np.ones(12), np.zeros(12)) == INVALID_ARG
    # device-memory form, from the pointers' values alone: a missing, short or misaligned workspace is CSP_ERR_WORKSPACE
    # (the periodic solve's own size is short: the optimiser's vectors come on top), a misaligned coeffs
    # CSP_ERR_INVALID_ARG
    dev = csp.make_desc(order, B, S, mem_space=csp.MEM_DEVICE)
    dev32 = csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, mem_space=csp.MEM_DEVICE)
    need = csp.periodic_timeopt_workspace_bytes(dev)
    a = (4096,) * 3
    for code in (_call(csp, dev, P(), *a, ws=None, ws_bytes=0), _call(csp, dev, P(), *a, ws=8192, ws_bytes=need - 1),
                 _call(csp, dev, P(), *a, ws=8192, ws_bytes=csp.periodic_workspace_bytes(dev)),
                 _call(csp, dev, P(), *a, ws=8196, ws_bytes=need)):
        assert code == WORKSPACE
    assert _call(csp, dev, P(), *a, co=4104, ws=8192, ws_bytes=need) == INVALID_ARG
    assert _call(csp, dev32, P(), *a, co=4100, ws=8192, ws_bytes=need) == INVALID_ARG
    # nothing to do: CSP_OK, with or without a device
    assert _call(csp, csp.make_desc(order, 0, S), P(), None, None, None) == OK
    if csp.device_count() == 0:   # everything in order: only now is a device looked for
        assert call(host, P()) == NO_DEVICE
        assert call(host, P(mode=csp.TIMEOPT_TIME_PENALTY, time_weight=1.0, min_time=1.5)) == NO_DEVICE
        assert _call(csp, dev, P(), *a, co=4096, ws=8192, ws_bytes=need) == NO_DEVICE
        with pytest.raises(csp.CspError) as e:
            csp.optimize_times_periodic_batch(wp, tm, order=order)
        assert e.value.code == NO_DEVICE
    with pytest.raises(ValueError):
        csp.optimize_times_periodic_batch(wp, tm, order=order, mode="fastest")


# ------------------------------------------------------------------------------------------------------ the reference

# Central differences of the dense fp64 J with step h = 1e-4 T_j.  Two error terms, both relative to |dJ/dT_j| ~
# (2o-1) J / T_j: truncation h^2 J''' / 6 ~ (1e-8 / 6) 2o (2o+1) <= 1.9e-7, and the noise of J itself over the step,
# eps_J / (1e-4 (2o-1)), with eps_J the dense KKT's own error (up to 1.3e-10 at order 5 against 40
# digits, 3e-11 / 5e-13 / 3e-15 below) <= 1.5e-7.  Unequal times put most of J into the shortest segment, so one entry's
# share of the gradient is up to ~30x below the largest: the gate is on the error over max_j |dJ/dT_j|, 10x the sum.
GATE_FD = 4e-6


@pytest.mark.parametrize("w", [0.0, 0.3])
@pytest.mark.parametrize("S", [2, 3, 6])
@pytest.mark.parametrize("order", ORDERS)
def test_reference_gradient_against_central_differences(order, S, w):
    path, time = ref.make_loop(order, S, 0, seed=40)
    J, g = ref.cost_grad(order, path, time, w)
    fd = np.zeros(S)
    for j in range(S):
        h = 1e-4 * time[j]
        tp, tm = time.copy(), time.copy()
        tp[j] += h
        tm[j] -= h
        fd[j] = (ref.cost_grad(order, path, tp, w)[0] - ref.cost_grad(order, path, tm, w)[0]) / (2 * h)
    err = np.max(np.abs(fd - g)) / np.max(np.abs(g))
    print("o%d S%d w%.1f: gradient vs central differences %.2e" % (order, S, w, err))
    assert err <= GATE_FD, (err, g, fd)


@pytest.mark.parametrize("S", [1, 2, 3, 6, 9])
@pytest.mark.parametrize("order", ORDERS)
def test_reference_eulers_identity(order, S):
    """J is homogeneous of degree 1 - 2o in the times at w = 0 (scale every T by c: the optimal loop is the same curve
    run c times slower, its o-th derivative c^-o times smaller over c times the time): sum_j T_j dJ/dT_j = (1 - 2o) J.
    Gate: the sum of the project's gates on this reference's J and on its gradient (tests/test_gpu_periodic.py's GATE_J
    + GATE_G: 3e-14 + 5e-14, 5e-12 + 4e-12, 3e-10 + 6e-10, 1e-8 + 1e-8), the two quantities the identity joins."""
    path, time = ref.make_loop(order, S, 1, seed=41)
    J, g = ref.cost_grad(order, path, time)
    gate = {2: 8e-14, 3: 9e-12, 4: 9e-10, 5: 2e-8}[order]
    if S == 1:
        assert abs(J) <= 1e-20 and np.all(np.abs(g) <= 1e-20)
        return
    err = abs(time @ g - (1 - 2 * order) * J) / ((2 * order - 1) * J)
    print("o%d S%d: Euler %.2e" % (order, S, err))
    assert err <= gate, err


@pytest.mark.parametrize("order", ORDERS)
def test_reference_fixed_total_returns_to_equal_times(order):
    """S = 2 there-and-back and a regular hexagon are symmetric under the cyclic shift of the segments, and J is convex
    along the fixed total there: the optimum has equal times.  Measured with tol 1e-6 from the starts of
    ref.closed_form_start: equal within 4.8e-7 relative, final J within 6.3e-11 of J at equal times; gated with the
    margin the GPU test uses (the stopping measure, not the arithmetic, sets them)."""
    for name, path in (("there-and-back", ref.there_and_back()), ("hexagon", ref.hexagon())):
        S = len(path)
        t0 = ref.closed_form_start(order, S, "fixed_total")
        r = ref.optimize(order, path, t0, 0.0, "fixed_total", 0.0, 0.1, 1e-6, 300)
        mean = t0.sum() / S
        Jeq = ref.cost_grad(order, path, np.full(S, mean))[0]
        et = np.max(np.abs(r["times"] - mean)) / mean
        ej = abs(r["f"] - Jeq) / Jeq
        print("o%d %s: times %.2e  J %.2e  (%d iterations, status %d)" % (order, name, et, ej, r["iterations"], r["status"]))
        assert r["status"] == 0
        assert et <= 1e-5 and ej <= 1e-9 and r["f"] >= Jeq * (1 - 1e-9)


@pytest.mark.parametrize("order", ORDERS)
def test_reference_time_penalty_closed_form_on_the_hexagon(order):
    """Equal times t on the hexagon: J(t) = J(1) t^(1-2o), so J + rho S t is stationary at
    t* = ((2o-1) J(1) / (rho S))^(1/2o); with rho = J(1) / S that is (2o-1)^(1/2o).  Measured from
    ref.closed_form_start: within 2.7e-6 at orders 2-4, 1.5e-5 at order 5.  Gates as the GPU test's: 1e-4 / 1e-3."""
    path = ref.hexagon()
    S = 6
    J1 = ref.cost_grad(order, path, np.ones(S))[0]
    rho = J1 / S
    t0 = ref.closed_form_start(order, S, "time_penalty")
    r = ref.optimize(order, path, t0, 0.0, "time_penalty", rho, 0.1, 1e-6, 300)
    want = ((2 * order - 1) * J1 / (rho * S)) ** (1.0 / (2 * order))
    err = np.max(np.abs(r["times"] - want)) / want
    print("o%d hexagon, time penalty: %.2e  (%d iterations, status %d)" % (order, err, r["iterations"], r["status"]))
    assert err <= (1e-3 if order == 5 else 1e-4), (r["times"], want)
    # homogeneity at the optimum: (2o-1) J = rho sum T
    T = r["times"]
    J = ref.cost_grad(order, path, T)[0]
    assert abs((2 * order - 1) * J - rho * T.sum()) <= (1e-3 if order == 5 else 1e-4) * r["f"]
