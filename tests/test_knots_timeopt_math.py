"""CPU checks of the segment-time optimisation under per-knot derivative constraints: the dense numpy
restatement tests/knots_timeopt_ref.py against the two references that exist (tests/timeopt_ref.py on the standard
partition, the 40-digit adjoint tests/knots_vjp_ref.py on three other partitions), Euler's identity, and the C-ABI
surface of csp_minsnap_optimize_times_knots_batch without a device (every check comes before a device is looked for)."""
import ctypes

import numpy as np
import pytest

from tests import knots_ref, knots_timeopt_ref, knots_vjp_ref, synth, timeopt_ref

OK, INVALID_ARG, UNSUPPORTED, WORKSPACE, NO_DEVICE = 0, -1, -2, -3, -5
ORDERS = (2, 3, 4, 5)
# Two fp64 dense solves of one system, and a dense fp64 solve against 40 digits.  Measured on the CPU (printed by the
# tests): on the standard mask J and the gradient come out bit-equal (the free set has the same order, so the two are
# the same arithmetic); against the 40-digit adjoint J and the gradient are <= 1.2e-11 at order 5, <= 1e-13 at order 4
# and <= 3.1e-15 below.  1e-10 holds at every order, so no order needs the 4x-measured rule.
GATE = 1e-10


def _problem(order, S, seed):
    wp, tm = synth.make_batch(1, S, config_id=3, offset=seed)
    bc = np.random.default_rng(seed).normal(size=(4, 3)) * 0.5
    return wp[0], tm[0], bc


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("S", [1, 2, 6])
@pytest.mark.parametrize("w", [0.0, 0.3])
def test_standard_mask_is_the_existing_reference(order, S, w):
    path, time, bc = _problem(order, S, 7 * order + S)
    mask, values = knots_ref.standard_problem(order, S, bc)
    J, g = knots_timeopt_ref.cost_grad(order, path, time, mask, values, w)
    Jr, gr = timeopt_ref.cost_grad(order, path, time, bc, w)
    ej, eg = abs(J - Jr) / abs(Jr), np.max(np.abs(g - gr)) / np.max(np.abs(gr))
    print("o%d S%d w%.1f: J %.2e grad %.2e" % (order, S, w, ej, eg))
    assert ej <= GATE and eg <= GATE, (ej, eg)


def _masks_s3(order):
    """free end; an interior velocity pin with a non-zero value; an interior full pin (non-zero values)."""
    n = order - 1
    full = (1 << n) - 1
    std = np.array([full, 0, 0, full], dtype=np.uint8)
    free_end, vel_pin, full_pin = std.copy(), std.copy(), std.copy()
    free_end[3] = 0
    vel_pin[1] = 1
    full_pin[2] = full
    return dict(free_end=free_end, vel_pin=vel_pin, full_pin=full_pin)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["free_end", "vel_pin", "full_pin"])
def test_gradient_is_the_adjoint_of_the_cost(order, name):
    path, time, _ = _problem(order, 3, 13 * order)
    rng = np.random.default_rng(order)
    values = rng.normal(size=(4, order - 1, 3))
    values[0, 2:] = values[3, 2:] = 0.0
    mask = _masks_s3(order)[name]
    for w in (0.0, 0.3):
        J, g = knots_timeopt_ref.cost_grad(order, path, time, mask, values, w)
        ref = knots_ref.solve(order, path, time, mask, values, vel_zero_weight=w)
        gr = np.asarray(knots_vjp_ref.adjoint(order, path, time, mask, values, pbar=None, jbar=1.0, vel_zero_weight=w).times,
                        dtype=np.float64).reshape(-1)
        ej, eg = abs(J - ref.cost) / abs(ref.cost), np.max(np.abs(g - gr)) / np.max(np.abs(gr))
        print("o%d %s w%.1f: J %.2e grad %.2e" % (order, name, w, ej, eg))
        assert ej <= GATE and eg <= GATE, (ej, eg)


@pytest.mark.parametrize("order", ORDERS)
def test_euler_identity_zero_pins(order):
    """Zero pinned values and w = 0: J is homogeneous of degree 1 - 2o in T under any mask."""
    path, time, _ = _problem(order, 5, 3 * order)
    n = order - 1
    rng = np.random.default_rng(order)
    mask = rng.integers(0, 1 << n, size=6).astype(np.uint8)
    mask[0] |= 1   # at least one pin keeps the example away from the trivial minimiser
    J, g = knots_timeopt_ref.cost_grad(order, path, time, mask, np.zeros((6, n, 3)))
    assert abs(time @ g - (1 - 2 * order) * J) <= 1e-9 * abs(J)


def test_unmasked_values_are_never_read():
    path, time, bc = _problem(4, 4, 1)
    mask, values = knots_ref.standard_problem(4, 4, bc)
    J, g = knots_timeopt_ref.cost_grad(4, path, time, mask, values)
    values[1:4] = np.nan
    J2, g2 = knots_timeopt_ref.cost_grad(4, path, time, mask, values)
    assert J == J2 and np.array_equal(g, g2)


def test_reference_optimiser_standard_mask_is_the_existing_one():
    for order, mode, rho in ((3, "fixed_total", 0.0), (4, "time_penalty", 40.0)):
        path, time, bc = _problem(order, 5, 50 + order)
        mask, values = knots_ref.standard_problem(order, 5, bc)
        a = knots_timeopt_ref.optimize(order, path, time, mask, values, 0.1, mode, rho, 0.05, 1e-6, 300)
        b = timeopt_ref.optimize(order, path, time, bc, 0.1, mode, rho, 0.05, 1e-6, 300)
        assert a["status"] == b["status"] == 0
        assert abs(a["f"] - b["f"]) <= 2e-7 * b["f"] and abs(a["f0"] - b["f0"]) <= 1e-10 * b["f0"]


# --------------------------------------------------------------------------------------------------------------- the C-ABI

def test_symbols_exported(csp):
    for name in ("csp_minsnap_optimize_times_knots_batch", "csp_minsnap_knots_timeopt_workspace_bytes"):
        assert name in csp.EXPORTED_SYMBOLS
        assert getattr(ctypes.CDLL(csp.LIB_PATH), name)
    assert callable(csp.optimize_times_knots_batch) and callable(csp.knots_timeopt_workspace_bytes)


def test_workspace_bytes_formula(csp):
    up = lambda v: (v + 255) // 256 * 256
    for order in ORDERS:
        n = order - 1
        for S, B in ((1, 1), (3, 4), (6, 70), (16, 65536), (9, 129)):
            want = up((S + 1) * (n * n + 3 * n) * B * 8) + 4 * S * B * 8
            off = np.zeros(B + 1, dtype=np.int64)
            assert csp.knots_timeopt_workspace_bytes(csp.make_desc(order, B, S)) == want
            assert csp.knots_timeopt_workspace_bytes(csp.make_desc(order, B, 0, seg_offsets_ptr=off.ctypes.data,
                                                                   max_segments=S)) == want
            assert csp.knots_timeopt_workspace_bytes(csp.make_desc(order, B, S, dtype=csp.DTYPE_F32)) == want
            # the coefficient launch runs in the factor region
            assert csp.knots_workspace_bytes(csp.make_desc(order, B, S)) == want - 4 * S * B * 8
    for bad in (csp.make_desc(1, 4, 3), csp.make_desc(6, 4, 3), csp.make_desc(4, 4, 3, path_weight=0.5),
                csp.make_desc(4, 4, 3, flags=csp.FLAG_SEGMENT_MAJOR),
                csp.make_desc(4, 4, 3, dtype=csp.DTYPE_F32, flags=csp.FLAG_F32_ARITH)):
        assert csp.knots_timeopt_workspace_bytes(bad) == 0


def _p(a):
    return None if a is None else (a if isinstance(a, int) else a.ctypes.data)


def _call(csp, desc, prm, wp, tm, mk, kv, tout, co=None, ws=None, ws_bytes=0):
    return csp.raw_lib().csp_minsnap_optimize_times_knots_batch(
        None if desc is None else ctypes.byref(desc), None if prm is None else ctypes.byref(prm), _p(wp), _p(tm), _p(mk),
        _p(kv), _p(tout), _p(co), None, None, None, _p(ws), ws_bytes, None)


def test_every_return_code_comes_back_without_a_device(csp):
    B, S, order = 4, 3, 4
    n = order - 1
    wp, tm = np.zeros((B, S + 1, 3)), np.ones((B, S))
    mk, kv = np.zeros((B, S + 1), np.uint8), np.zeros((B, S + 1, n, 3))
    mk[:, 0] = mk[:, S] = 7
    tout = np.zeros_like(tm)
    P = csp.make_timeopt_params
    call = lambda d, prm, times=tm: _call(csp, d, prm, wp, times, mk, kv, tout)
    unsupported = {"order 1": csp.make_desc(1, B, S),
                   "order 6": csp.make_desc(6, B, S),
                   "path penalty": csp.make_desc(order, B, S, path_weight=0.5),
                   "segment major": csp.make_desc(order, B, S, flags=csp.FLAG_SEGMENT_MAJOR),
                   "f32 arithmetic": csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, flags=csp.FLAG_F32_ARITH)}
    for name, d in unsupported.items():
        assert call(d, P()) == UNSUPPORTED, name
    host = csp.make_desc(order, B, S)
    # the six required pointers (and the descriptor)
    assert _call(csp, None, P(), wp, tm, mk, kv, tout) == INVALID_ARG
    assert _call(csp, host, None, wp, tm, mk, kv, tout) == INVALID_ARG
    assert _call(csp, host, P(), None, tm, mk, kv, tout) == INVALID_ARG
    assert _call(csp, host, P(), wp, None, mk, kv, tout) == INVALID_ARG
    assert _call(csp, host, P(), wp, tm, None, kv, tout) == INVALID_ARG
    assert _call(csp, host, P(), wp, tm, mk, None, tout) == INVALID_ARG
    assert _call(csp, host, P(), wp, tm, mk, kv, None) == INVALID_ARG
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
    # ragged host call: offsets outside 0..max_segments
    off = np.array([0, 3, 2, 8, 12], dtype=np.int64)
    rag = csp.make_desc(order, B, 0, seg_offsets_ptr=off.ctypes.data, max_segments=6)
    assert _call(csp, rag, P(), np.zeros((16, 3)), np.ones(12), np.zeros(16, np.uint8), np.zeros((16, n, 3)),
                 np.zeros(12)) == INVALID_ARG
    off = np.array([0, 3, 10, 11, 12], dtype=np.int64)
    rag = csp.make_desc(order, B, 0, seg_offsets_ptr=off.ctypes.data, max_segments=6)
    assert _call(csp, rag, P(), np.zeros((16, 3)), np.ones(12), np.zeros(16, np.uint8), np.zeros((16, n, 3)),
                 np.zeros(12)) == INVALID_ARG
    # device-memory form, from the pointers' values alone, through the C-ABI's one device-argument check: a short or
    # misaligned workspace is refused with that check's code for a workspace (CSP_ERR_WORKSPACE, as at every other
    # entry), a misaligned coeffs with CSP_ERR_INVALID_ARG
    dev = csp.make_desc(order, B, S, mem_space=csp.MEM_DEVICE)
    dev32 = csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, mem_space=csp.MEM_DEVICE)
    need = csp.knots_timeopt_workspace_bytes(dev)
    a = (4096,) * 5
    for code in (_call(csp, dev, P(), *a, ws=None, ws_bytes=0), _call(csp, dev, P(), *a, ws=8192, ws_bytes=need - 1),
                 _call(csp, dev, P(), *a, ws=8192, ws_bytes=csp.knots_workspace_bytes(dev)),
                 _call(csp, dev, P(), *a, ws=8196, ws_bytes=need)):
        assert code == WORKSPACE
    assert _call(csp, dev, P(), *a, co=4104, ws=8192, ws_bytes=need) == INVALID_ARG
    assert _call(csp, dev32, P(), *a, co=4100, ws=8192, ws_bytes=need) == INVALID_ARG
    # nothing to do: CSP_OK, with or without a device
    assert _call(csp, csp.make_desc(order, 0, S), P(), None, None, None, None, None) == OK
    if csp.device_count() == 0:   # everything in order: only now is a device looked for
        assert call(host, P()) == NO_DEVICE
        assert call(host, P(mode=csp.TIMEOPT_TIME_PENALTY, time_weight=1.0, min_time=1.5)) == NO_DEVICE
        assert _call(csp, dev, P(), *a, co=4096, ws=8192, ws_bytes=need) == NO_DEVICE
        with pytest.raises(csp.CspError) as e:
            csp.optimize_times_knots_batch(wp, tm, mk, kv, order=order)
        assert e.value.code == NO_DEVICE
    with pytest.raises(ValueError):
        csp.optimize_times_knots_batch(wp, tm, mk, kv, order=order, mode="fastest")
    with pytest.raises(ValueError):
        csp.optimize_times_knots_batch(wp, tm, mk[:, :-1], kv, order=order)
