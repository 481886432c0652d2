"""CPU checks of the open-chain solve's reverse mode with a cost cotangent: the dense numpy restatement
(tests/cost_vjp_ref.py) against directional derivatives of the 80-bit oracle's cost and coefficients, the identities the
gradient of J obeys, and the C-ABI surface of csp_minsnap_solve_batch_cost_vjp without a device.

Gates are those of tests/test_vjp_math.py for the same order: waypoints / bc 2e-10 (1e-8 at order 5), times 1e-9 (1e-7)."""
import ctypes

import numpy as np
import pytest

from tests import synth
from tests.cost_vjp_ref import cost_adjoint, cost_coeff_cotangent, cost_vjp, oracle_cost_directional
from tests.timeopt_ref import cost_from_coeffs
from tests.vjp_ref import adjoint, oracle_directional

OK, INVALID_ARG, UNSUPPORTED, WORKSPACE, NO_DEVICE = 0, -1, -2, -3, -5


def _gates(order):
    return (1e-8, 1e-7) if order == 5 else (2e-10, 1e-9)


def _case(order, S):
    wp, tm = synth.make_batch(1, S, config_id=3)
    bc = np.random.default_rng(100 * order + S).normal(size=(4, 3))
    return wp[0], tm[0], bc


def _rel(got, ref):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(ref))) / np.max(np.abs(ref)))


@pytest.mark.parametrize("order", [2, 3, 4, 5])
@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("w", [0.0, 0.3])
@pytest.mark.parametrize("jbar", [0.0, 0.7])
def test_restatement_matches_oracle_directional_derivatives(oracle_mod, order, S, w, jbar):
    """L = <pbar, coeffs> + jbar J along every coordinate of waypoints, bc and times."""
    path, time, bc = _case(order, S)
    pbar = np.random.default_rng(order * 7 + S).normal(size=(S, 3, 2 * order))
    r = cost_vjp(order, path, time, bc, pbar, jbar, w)
    fwp, fbc, ft = oracle_directional(oracle_mod, order, path, time, bc, pbar, w)
    if jbar:
        jwp, jbc, jt = oracle_cost_directional(oracle_mod, order, path, time, bc, w)
        fwp, fbc, ft = fwp + jbar * jwp, fbc + jbar * jbc, ft + jbar * jt
    e_lin = _rel(np.concatenate([r["waypoints"].ravel(), r["bc"].ravel()]), np.concatenate([fwp.ravel(), fbc.ravel()]))
    e_t = _rel(r["times"], ft)
    print("order %d S %d w %g jbar %g: waypoints/bc %.2e times %.2e" % (order, S, w, jbar, e_lin, e_t))
    g_lin, g_t = _gates(order)
    assert e_lin < g_lin and e_t < g_t, (e_lin, e_t)


@pytest.mark.parametrize("order", [2, 3, 4, 5])
@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("w", [0.0, 0.3])
def test_cost_gradient_alone_matches_oracle(oracle_mod, order, S, w):
    """The J part on its own (what the cost-only kernel computes), and its J against the oracle's."""
    path, time, bc = _case(order, S)
    r = cost_adjoint(order, path, time, bc, w)
    c, _ = oracle_mod.solve_batch(order, path[None], time[None], bc[None], vel_zero_weight=w, long_double=True)
    Jo = cost_from_coeffs(order, c[0], time, w)
    assert abs(r["cost"] - Jo) <= 1e-9 * abs(Jo)
    jwp, jbc, jt = oracle_cost_directional(oracle_mod, order, path, time, bc, w)
    e_lin = _rel(np.concatenate([r["waypoints"].ravel(), r["bc"].ravel()]), np.concatenate([jwp.ravel(), jbc.ravel()]))
    e_t = _rel(r["times"], jt)
    print("order %d S %d w %g: waypoints/bc %.2e times %.2e" % (order, S, w, e_lin, e_t))
    g_lin, g_t = _gates(order)
    assert e_lin < g_lin and e_t < g_t, (e_lin, e_t)
    if order == 2:
        assert not r["bc"][2:].any()    # no acceleration slot at order 2


@pytest.mark.parametrize("order", [2, 3, 4, 5])
@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("w", [0.0, 0.3])
def test_translation_and_homogeneity(order, S, w):
    """J does not depend on a translation: sum_k dJ/dP_k = 0.  J is homogeneous of degree 2 in (waypoints, bc) jointly,
    at any w: sum P.dJ/dP + sum bc.dJ/dbc = 2 J."""
    path, time, bc = _case(order, S)
    r = cost_adjoint(order, path, time, bc, w)
    g_lin, _ = _gates(order)
    scale = np.max(np.abs(r["waypoints"]))
    assert np.max(np.abs(r["waypoints"].sum(axis=0))) < g_lin * scale * (S + 1)
    euler = np.sum(path * r["waypoints"]) + np.sum(bc * r["bc"])
    # the products P.dJ/dP cancel down from |P| |dJ/dP| to 2J: the gate is on the terms that are summed
    terms = np.sum(np.abs(path * r["waypoints"])) + np.sum(np.abs(bc * r["bc"]))
    assert abs(euler - 2.0 * r["cost"]) < g_lin * max(terms, abs(r["cost"])), (euler, r["cost"])


@pytest.mark.parametrize("order", [2, 3, 4, 5])
@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("w", [0.0, 0.3])
def test_cost_gradient_is_the_adjoint_of_its_coefficient_gradient(order, S, w):
    """J = sum c^T (Q + w V) c over segments and axes, so dJ/d(waypoints, bc) = adjoint(p_bar = 2 (Q + w V) p); for the
    times the same plus the explicit terms p^(o)(T)^2 + 2 w v(T) a(T)."""
    path, time, bc = _case(order, S)
    o, m = order, 2 * order
    coeffs = adjoint(o, path, time, bc, np.zeros((S, 3, m)), w)["coeffs"]
    pbar, explicit = cost_coeff_cotangent(o, coeffs, time, w)
    via = adjoint(o, path, time, bc, pbar, w)
    r = cost_adjoint(o, path, time, bc, w)
    g_lin, g_t = _gates(order)
    e_lin = _rel(np.concatenate([r["waypoints"].ravel(), r["bc"].ravel()]),
                 np.concatenate([via["waypoints"].ravel(), via["bc"].ravel()]))
    # the two parts of the time gradient cancel (the envelope term is what is left): measured against the larger part
    tt = via["times"] + explicit
    e_t = float(np.max(np.abs(r["times"] - tt)) / max(np.max(np.abs(via["times"])), np.max(np.abs(explicit)), np.max(np.abs(tt))))
    print("order %d S %d w %g: waypoints/bc %.2e times %.2e" % (order, S, w, e_lin, e_t))
    assert e_lin < g_lin and e_t < g_t, (e_lin, e_t)


# ---- the C-ABI surface, no device ----

def test_symbols_exported(csp):
    for name in ("csp_minsnap_solve_batch_cost_vjp", "csp_minsnap_cost_vjp_workspace_bytes"):
        assert name in csp.EXPORTED_SYMBOLS
        assert getattr(ctypes.CDLL(csp.LIB_PATH), name)
    assert callable(csp.cost_vjp_workspace_bytes)


def _formula(order, smax, B, shared_bc, pbar):
    n = order - 1
    factors = (max(smax - 1, 0) * (n * n + (6 if pbar else 3) * n) * B * 8 + 255) // 256 * 256
    return factors + (12 * ((B + 63) // 64) * 8 if shared_bc else 0)


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_workspace_formulas(csp, order):
    for S, B, per in [(16, 65536, False), (1, 100, False), (7, 3, True), (40, 129, False), (2, 1, True), (17, 65, False)]:
        for dtype in (csp.DTYPE_F64, csp.DTYPE_F32):
            d = csp.make_desc(order, B, S, dtype=dtype, bc_per_trajectory=per)
            assert csp.cost_vjp_workspace_bytes(d, True) == _formula(order, S, B, not per, True) == csp.vjp_workspace_bytes(d)
            assert csp.cost_vjp_workspace_bytes(d, False) == _formula(order, S, B, not per, False)
            if per:
                assert csp.cost_vjp_workspace_bytes(d, False) == csp.cost_workspace_bytes(d)
    off = np.array([0, 3, 3, 10], dtype=np.int64)
    d = csp.make_desc(order, 3, 0, seg_offsets_ptr=off.ctypes.data, max_segments=9)   # sized by max_segments, not the data
    assert csp.cost_vjp_workspace_bytes(d, True) == _formula(order, 9, 3, True, True)
    assert csp.cost_vjp_workspace_bytes(d, False) == _formula(order, 9, 3, True, False)
    for pb in (True, False):
        assert csp.cost_vjp_workspace_bytes(csp.make_desc(order, 0, 5), pb) == 0


def _unsupported(csp):
    return {"path_weight": csp.make_desc(4, 4, 3, path_weight=0.1),
            "order 1": csp.make_desc(1, 4, 3),
            "order 6": csp.make_desc(6, 4, 3),
            "segment major": csp.make_desc(4, 4, 3, flags=csp.FLAG_SEGMENT_MAJOR),
            "f32 arithmetic": csp.make_desc(4, 4, 3, dtype=csp.DTYPE_F32, flags=csp.FLAG_F32_ARITH)}


def test_workspace_of_unsupported_descriptors_is_zero(csp):
    for name, d in _unsupported(csp).items():
        assert csp.cost_vjp_workspace_bytes(d, True) == 0 and csp.cost_vjp_workspace_bytes(d, False) == 0, name
    bad = csp.make_desc(4, 4, 3)
    bad.abi_version = 99
    assert csp.cost_vjp_workspace_bytes(bad, False) == 0
    assert csp.cost_vjp_workspace_bytes(csp.make_desc(4, 4, 0), False) == 0   # ragged without offsets


def _call(csp, desc, wp, tm, bc, gco, gj, gwp, gtm, gbc, ws=None, ws_bytes=0):
    p = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)
    return csp.raw_lib().csp_minsnap_solve_batch_cost_vjp(ctypes.byref(desc), p(wp), p(tm), p(bc), p(gco), p(gj), p(gwp), p(gtm),
                                                          p(gbc), None, p(ws), ws_bytes, None)


def test_argument_errors_come_back_without_a_device(csp):
    B, S, order = 4, 3, 4
    wp, tm, bc, gco = np.zeros((B, S + 1, 3)), np.ones((B, S)), np.zeros((1, 4, 3)), np.zeros((B, S, 3, 2 * order))
    gwp, gtm, gbc, gj = np.zeros((B, S + 1, 3)), np.zeros((B, S)), np.zeros((1, 4, 3)), np.zeros(B)
    for name, d in _unsupported(csp).items():
        assert _call(csp, d, wp, tm, bc, gco, gj, gwp, gtm, gbc) == UNSUPPORTED, name
        assert _call(csp, d, wp, tm, bc, None, gj, gwp, gtm, gbc) == UNSUPPORTED, name
    host = csp.make_desc(order, B, S)
    assert _call(csp, host, wp, tm, bc, None, None, gwp, gtm, gbc) == INVALID_ARG     # both cotangents null
    assert _call(csp, host, wp, tm, bc, gco, gj, None, None, None) == INVALID_ARG     # all three outputs null
    assert _call(csp, host, wp, tm, bc, None, gj, None, None, None) == INVALID_ARG
    assert _call(csp, host, None, tm, bc, gco, gj, gwp, gtm, gbc) == INVALID_ARG
    assert _call(csp, host, wp, None, bc, gco, gj, gwp, gtm, gbc) == INVALID_ARG
    assert _call(csp, host, wp, tm, None, gco, gj, gwp, gtm, gbc) == INVALID_ARG
    bad = csp.make_desc(order, B, S)
    bad.abi_version = 99
    assert _call(csp, bad, wp, tm, bc, gco, gj, gwp, gtm, gbc) == INVALID_ARG
    assert _call(csp, csp.make_desc(order, 0, S), None, None, None, None, None, None, None, None) == OK   # empty batch: a no-op
    # ragged host call: offsets outside 0..max_segments
    off = np.array([0, 3, 2, 8, 12], dtype=np.int64)
    rag = csp.make_desc(order, B, 0, seg_offsets_ptr=off.ctypes.data, max_segments=6)
    assert _call(csp, rag, np.zeros((16, 3)), np.ones(12), bc, None, gj, np.zeros((16, 3)), None, None) == INVALID_ARG
    # device-memory form: workspace and alignment are checked from the pointers' values alone
    dev = csp.make_desc(order, B, S, mem_space=csp.MEM_DEVICE)
    for gcp, pb in ((4096, True), (None, False)):
        need = csp.cost_vjp_workspace_bytes(dev, pb)
        assert need == _formula(order, S, B, True, pb) > 0
        assert _call(csp, dev, 4096, 4096, 4096, gcp, 4096, 4096, None, None, None, 0) == WORKSPACE
        assert _call(csp, dev, 4096, 4096, 4096, gcp, 4096, 4096, None, None, 8192, need - 1) == WORKSPACE
        assert _call(csp, dev, 4096, 4096, 4096, gcp, 4096, 4096, None, None, 8196, need) == WORKSPACE   # not 8-byte aligned
    need = csp.cost_vjp_workspace_bytes(dev, True)
    assert csp.cost_vjp_workspace_bytes(dev, False) < need
    assert _call(csp, dev, 4096, 4096, 4096, 4104, 4096, 4096, None, None, 8192, need) == INVALID_ARG    # grad_coeffs: 16 bytes
    dev32 = csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, mem_space=csp.MEM_DEVICE)
    assert _call(csp, dev32, 4096, 4096, 4096, 4100, 4096, 4096, None, None, 8192, need) == INVALID_ARG  # fp32: 8 bytes
    if csp.device_count() == 0:   # everything in order: only now is a device looked for
        assert _call(csp, host, wp, tm, bc, gco, gj, gwp, gtm, gbc) == NO_DEVICE
        assert _call(csp, host, wp, tm, bc, None, gj, None, gtm, None) == NO_DEVICE
        assert _call(csp, host, wp, tm, bc, gco, None, gwp, None, None) == NO_DEVICE
        assert _call(csp, dev32, 4096, 4096, 4096, 4104, 4096, 4096, None, None, 8192, need) == NO_DEVICE
        with pytest.raises(csp.CspError) as e:
            csp.solve_batch_vjp(wp, tm, None, grad_cost=gj, order=order)
        assert e.value.code == NO_DEVICE
    with pytest.raises(ValueError):
        csp.solve_batch_vjp(wp, tm, None, order=order)
    with pytest.raises(ValueError):
        csp.solve_batch_vjp(wp, tm, None, grad_cost=np.zeros(B + 1), order=order)
