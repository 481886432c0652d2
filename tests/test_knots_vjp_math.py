"""CPU tests of the knot-constrained solve's reverse mode (csp_minsnap_solve_knots_batch_vjp): the
reference adjoint tests/knots_vjp_ref.py against directional derivatives of tests/knots_ref.py and against the open
chain's adjoint, exact zeros at free slots, the C-ABI's argument checks (every one of them comes back with no device
present), the workspace formula and the exported symbols."""
import ctypes

import numpy as np
import pytest

from tests import knots_ref, knots_vjp_ref
from tests.cost_vjp_ref import cost_vjp
from tests.test_gpu_knots import PATTERNS, make_case
from tests.test_gpu_vjp import GATE_NUMPY
from tests.vjp_ref import rel_err_rows

OK, INVALID_ARG, UNSUPPORTED, WORKSPACE, NO_DEVICE = 0, -1, -2, -3, -5
ORDERS = (2, 3, 4, 5)
SEGMENTS = (1, 2, 3, 5)
FD_GATE = 1e-12
FD_DPS = 50
H = 2.0 ** -16


def _case(order, S, pattern):
    """One trajectory of test_gpu_knots.make_case with times on multiples of 2^-10 (T +- h is then an exact double) and
    cotangents; row S % 3 so that both weights 0 and 0.3 occur."""
    path, time, mask, values, w = make_case(order, S, pattern, S % 3)
    time = np.round(time * 1024.0) / 1024.0
    rng = np.random.default_rng([order, S, PATTERNS.index(pattern), 7])
    return path, time, mask, values, w, rng.normal(size=(S, 3, 2 * order)), float(rng.normal())


def _loss(order, path, time, mask, values, w, pbar, jbar):
    import mpmath
    s = knots_ref.solve(order, path, time, mask, values, vel_zero_weight=w, dps=FD_DPS, raw=True)
    with mpmath.workdps(FD_DPS):
        L = mpmath.mpf(float(jbar)) * s.cost
        for j in range(len(time)):
            for ax in range(3):
                for i in range(2 * order):
                    L += mpmath.mpf(float(pbar[j, ax, i])) * s.coeffs[j][ax][i]
        return L


def _directional(order, path, time, mask, values, w, pbar, jbar):
    """(dL/dwaypoints, dL/dtimes, dL/dvalues at the pinned slots) by differences of knots_ref.solve.  L is a quadratic in
    waypoints and values: a central difference with step 1 is exact.  Times: central differences at h and h/2,
    Richardson-extrapolated (truncation h^4, about 5e-20 of the scale)."""
    import mpmath
    S, n = len(time), order - 1
    f = lambda p, t, v: _loss(order, p, t, mask, v, w, pbar, jbar)
    with mpmath.workdps(FD_DPS):
        gwp, gkv, gt = np.zeros((S + 1, 3)), np.zeros((S + 1, n, 3)), np.zeros(S)
        for k in range(S + 1):
            for ax in range(3):
                e = np.zeros_like(path)
                e[k, ax] = 1.0
                gwp[k, ax] = float((f(path + e, time, values) - f(path - e, time, values)) / 2)
                for r in range(n):
                    if (mask[k] >> r) & 1:
                        e = np.zeros_like(values)
                        e[k, r, ax] = 1.0
                        gkv[k, r, ax] = float((f(path, time, values + e) - f(path, time, values - e)) / 2)
        for j in range(S):
            e = np.zeros(S)
            e[j] = H
            d1 = (f(path, time + e, values) - f(path, time - e, values)) / (2 * mpmath.mpf(H))
            d2 = (f(path, time + e / 2, values) - f(path, time - e / 2, values)) / mpmath.mpf(H)
            gt[j] = float((4 * d2 - d1) / 3)
    return gwp, gt, gkv


@pytest.mark.parametrize("order", ORDERS)
def test_reference_adjoint_meets_directional_derivatives(order):
    """Orders 2..5, S in {1, 2, 3, 5}, every pattern of test_gpu_knots whose constraint count reaches the order, w in
    {0, 0.3}; the 40-digit adjoint against differences of the 50-digit solve, relative per output, gate 1e-12.
    Measured worst: order 2: 6.5e-16, 3: 3.7e-16, 4: 4.9e-16, 5: 2.6e-16 -- the rounding of both results to doubles."""
    worst = 0.0
    for S in SEGMENTS:
        for pattern in PATTERNS:
            path, time, mask, values, w, pbar, jbar = _case(order, S, pattern)
            if knots_ref.constraint_count(order, mask) < order:
                continue
            ref = knots_vjp_ref.adjoint(order, path, time, mask, values, pbar, jbar, w)
            fd = _directional(order, path, time, mask, values, w, pbar, jbar)
            for name, a, b in zip(("waypoints", "times", "values"), ref, fd):
                e = rel_err_rows(a.reshape(1, -1), b.reshape(1, -1))
                worst = max(worst, e)
                assert e <= FD_GATE, (order, S, pattern, name, e)
    print("order %d: reference adjoint against directional derivatives, worst %.2e" % (order, worst))


@pytest.mark.parametrize("order", ORDERS)
def test_free_slots_have_gradient_exactly_zero(order):
    n = order - 1
    for S in SEGMENTS:
        for pattern in PATTERNS:
            path, time, mask, values, w, pbar, jbar = _case(order, S, pattern)
            if knots_ref.constraint_count(order, mask) < order:
                continue
            values = values.copy()
            free = ((mask[:, None] >> np.arange(n)[None, :]) & 1) == 0
            for dps in (40, None):
                g = knots_vjp_ref.adjoint(order, path, time, mask, values, pbar, jbar, w, dps=dps)
                assert not g.values[free].any() and not np.signbit(g.values[free]).any(), (order, S, pattern, dps)


@pytest.mark.parametrize("order", ORDERS)
def test_standard_mask_is_the_open_chain_adjoint(order):
    """With knots_ref.standard_problem's mask the float run is tests/vjp_ref.adjoint plus cost_vjp_ref on waypoints and
    times, and the end knots' value rows 0 and 1 are its bc gradient."""
    rng = np.random.default_rng(300 + order)
    for S in (1, 2, 3, 5, 16):
        path, time = np.cumsum(rng.normal(size=(S + 1, 3)) * 5, 0), rng.uniform(0.5, 2.0, S)
        bc = rng.normal(size=(4, 3))
        if order == 2:
            bc[2:] = 0.0
        w = 0.3 if S % 2 else 0.0
        pbar, jbar = rng.normal(size=(S, 3, 2 * order)), float(rng.normal())
        mask, values = knots_ref.standard_problem(order, S, bc)
        for pb, jb in ((pbar, 0.0), (pbar, jbar), (None, jbar)):
            got = knots_vjp_ref.adjoint(order, path, time, mask, values, pb, jb, w, dps=None)
            ref = cost_vjp(order, path, time, bc, pb, jb, w)
            gbc = np.zeros((4, 3))
            gbc[0], gbc[1] = got.values[0, 0], got.values[S, 0]
            if order > 2:
                gbc[2], gbc[3] = got.values[0, 1], got.values[S, 1]
            for name, a, b in (("waypoints", got.waypoints, ref["waypoints"]), ("times", got.times, ref["times"]),
                               ("bc", gbc, ref["bc"])):
                e = rel_err_rows(a.reshape(1, -1), np.asarray(b).reshape(1, -1))
                assert e <= GATE_NUMPY[order], (order, S, name, pb is None, jb, e)


# --------------------------------------------------------------------------------------------------------------- the C-ABI

def test_symbols_exported(csp):
    for name in ("csp_minsnap_solve_knots_batch_vjp", "csp_minsnap_knots_vjp_workspace_bytes"):
        assert name in csp.EXPORTED_SYMBOLS
        assert getattr(ctypes.CDLL(csp.LIB_PATH), name)
    assert callable(csp.solve_knots_batch_vjp) and callable(csp.knots_vjp_workspace_bytes)
    assert callable(csp.solve_knots_batch_autograd) and csp.KnotsVjpResult(1, 2, 3, 4).knot_values == 3


def test_workspace_bytes_formula(csp):
    up = lambda v: (v + 255) // 256 * 256
    for order in ORDERS:
        n = order - 1
        for B, S in ((1, 1), (65, 17), (7, 300)):
            for pbar, c in ((True, 6), (False, 3)):
                want = up((S + 1) * (n * n + c * n) * B * 8)
                off = np.zeros(B + 1, dtype=np.int64)
                assert csp.knots_vjp_workspace_bytes(csp.make_desc(order, B, S), pbar) == want
                assert csp.knots_vjp_workspace_bytes(csp.make_desc(order, B, 0, seg_offsets_ptr=off.ctypes.data, max_segments=S),
                                                     pbar) == want
                assert csp.knots_vjp_workspace_bytes(csp.make_desc(order, B, S, dtype=csp.DTYPE_F32), pbar) == want
    for bad in (csp.make_desc(1, 4, 3), csp.make_desc(6, 4, 3), csp.make_desc(4, 4, 3, path_weight=0.5),
                csp.make_desc(4, 4, 3, flags=csp.FLAG_SEGMENT_MAJOR),
                csp.make_desc(4, 4, 3, dtype=csp.DTYPE_F32, flags=csp.FLAG_F32_ARITH)):
        assert csp.knots_vjp_workspace_bytes(bad, True) == 0 and csp.knots_vjp_workspace_bytes(bad, False) == 0


def _p(a):
    return None if a is None else (a if isinstance(a, int) else a.ctypes.data)


def _call(csp, desc, wp, tm, mk, kv, gco, gj, gwp, gtm, gkv, status=None, ws=None, ws_bytes=0):
    return csp.raw_lib().csp_minsnap_solve_knots_batch_vjp(ctypes.byref(desc), _p(wp), _p(tm), _p(mk), _p(kv), _p(gco), _p(gj),
                                                           _p(gwp), _p(gtm), _p(gkv), _p(status), _p(ws), ws_bytes, None)


def test_every_return_code_comes_back_without_a_device(csp):
    B, S, order = 4, 3, 4
    n = order - 1
    wp, tm = np.zeros((B, S + 1, 3)), np.ones((B, S))
    mk, kv = np.zeros((B, S + 1), np.uint8), np.zeros((B, S + 1, n, 3))
    gco, gj = np.zeros((B, S, 3, 2 * order)), np.zeros(B)
    gwp, gtm, gkv = np.zeros_like(wp), np.zeros_like(tm), np.zeros_like(kv)
    call = lambda d: _call(csp, d, wp, tm, mk, kv, gco, gj, gwp, gtm, gkv)
    unsupported = {"order 1": csp.make_desc(1, B, S),
                   "order 6": csp.make_desc(6, B, S),
                   "path penalty": csp.make_desc(order, B, S, path_weight=0.5),
                   "segment major": csp.make_desc(order, B, S, flags=csp.FLAG_SEGMENT_MAJOR),
                   "f32 arithmetic": csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, flags=csp.FLAG_F32_ARITH)}
    for name, d in unsupported.items():
        assert call(d) == UNSUPPORTED, name
    host = csp.make_desc(order, B, S)
    bad = csp.make_desc(order, B, S)
    bad.abi_version = 99
    assert call(bad) == INVALID_ARG
    assert call(csp.make_desc(order, B, S, vel_zero_weight=-1.0)) == INVALID_ARG
    # null required pointers, both cotangents null, all outputs null
    assert _call(csp, host, None, tm, mk, kv, gco, gj, gwp, gtm, gkv) == INVALID_ARG
    assert _call(csp, host, wp, None, mk, kv, gco, gj, gwp, gtm, gkv) == INVALID_ARG
    assert _call(csp, host, wp, tm, None, kv, gco, gj, gwp, gtm, gkv) == INVALID_ARG
    assert _call(csp, host, wp, tm, mk, None, gco, gj, gwp, gtm, gkv) == INVALID_ARG
    assert _call(csp, host, wp, tm, mk, kv, None, None, gwp, gtm, gkv) == INVALID_ARG
    assert _call(csp, host, wp, tm, mk, kv, gco, gj, None, None, None) == INVALID_ARG
    # ragged host call: offsets outside 0..max_segments
    off = np.array([0, 3, 2, 8, 12], dtype=np.int64)
    rag = csp.make_desc(order, B, 0, seg_offsets_ptr=off.ctypes.data, max_segments=6)
    assert _call(csp, rag, np.zeros((16, 3)), np.ones(12), np.zeros(16, np.uint8), np.zeros((16, n, 3)),
                 np.zeros((12, 3, 2 * order)), gj, np.zeros((16, 3)), np.zeros(12), np.zeros((16, n, 3))) == INVALID_ARG
    # device-memory form: workspace size and alignment and the cotangent's alignment, from the pointers' values alone
    dev = csp.make_desc(order, B, S, mem_space=csp.MEM_DEVICE)
    dev32 = csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, mem_space=csp.MEM_DEVICE)
    need, need3 = csp.knots_vjp_workspace_bytes(dev, True), csp.knots_vjp_workspace_bytes(dev, False)
    assert need3 < need
    a = (4096,) * 4
    o = (4096,) * 3
    assert _call(csp, dev, *a, 4096, 4096, *o, ws=None, ws_bytes=0) == WORKSPACE
    assert _call(csp, dev, *a, 4096, 4096, *o, ws=8192, ws_bytes=need - 1) == WORKSPACE
    assert _call(csp, dev, *a, 4096, 4096, *o, ws=8192, ws_bytes=need3) == WORKSPACE          # six columns need the larger one
    assert _call(csp, dev, *a, None, 4096, *o, ws=8192, ws_bytes=need3 - 1) == WORKSPACE
    assert _call(csp, dev, *a, 4096, 4096, *o, ws=8196, ws_bytes=need) == WORKSPACE           # not 8-byte aligned
    assert _call(csp, dev, *a, 4104, 4096, *o, ws=8192, ws_bytes=need) == INVALID_ARG         # grad_coeffs: 16 bytes
    assert _call(csp, dev32, *a, 4100, 4096, *o, ws=8192, ws_bytes=need) == INVALID_ARG       # fp32: 8 bytes
    # nothing to do: CSP_OK, with or without a device
    assert _call(csp, csp.make_desc(order, 0, S), None, None, None, None, None, None, None, None, None) == OK
    if csp.device_count() == 0:   # everything in order: only now is a device looked for
        assert call(host) == NO_DEVICE
        assert _call(csp, host, wp, tm, mk, kv, None, gj, None, gtm, None) == NO_DEVICE
        assert _call(csp, dev, *a, 4096, 4096, *o, ws=8192, ws_bytes=need) == NO_DEVICE
        assert _call(csp, dev, *a, None, 4096, *o, ws=8192, ws_bytes=need3) == NO_DEVICE
        assert _call(csp, dev32, *a, 4104, None, *o, ws=8192, ws_bytes=need) == NO_DEVICE
        with pytest.raises(csp.CspError) as e:
            csp.solve_knots_batch_vjp(wp, tm, mk, kv, grad_coeffs=gco, order=order)
        assert e.value.code == NO_DEVICE
    with pytest.raises(ValueError):
        csp.solve_knots_batch_vjp(wp, tm, mk, kv, order=order)
    with pytest.raises(ValueError):
        csp.solve_knots_batch_vjp(wp, tm, mk, kv, grad_coeffs=gco, order=order, want=("bc",))
