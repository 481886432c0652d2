"""CPU checks of the solve's reverse mode: the dense numpy adjoint (tests/vjp_ref.py) against directional derivatives of
the long-double oracle, and the C-ABI surface of csp_minsnap_solve_batch_vjp without a device."""
import ctypes
import os

import numpy as np
import pytest

from tests import synth
from tests.conftest import load_cases
from tests.vjp_ref import adjoint, oracle_directional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_case(oracle_mod, order, path, time, bc, w, seed):
    S = len(time)
    pbar = np.random.default_rng(seed).normal(size=(S, 3, 2 * order))
    r = adjoint(order, path, time, bc, pbar, w)
    # the forward of the restatement is the oracle's solve
    c_ld, _ = oracle_mod.solve_batch(order, path[None], time[None], bc[None], vel_zero_weight=w, long_double=True)
    assert synth.rel_err_per_power(r["coeffs"], c_ld[0]) < 1e-8
    fd_wp, fd_bc, fd_t = oracle_directional(oracle_mod, order, path, time, bc, pbar, w)
    fd = np.concatenate([fd_wp.ravel(), fd_bc.ravel()])
    got = np.concatenate([r["waypoints"].ravel(), r["bc"].ravel()])
    err_lin = np.max(np.abs(got - fd)) / np.max(np.abs(fd))
    err_t = np.max(np.abs(r["times"] - fd_t)) / np.max(np.abs(fd_t))
    return err_lin, err_t


@pytest.mark.parametrize("order", [2, 3, 4, 5])
@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("w", [0.0, 0.3])
def test_adjoint_matches_oracle_directional_derivatives(oracle_mod, order, S, w):
    wp, tm = synth.make_batch(1, S, config_id=3)
    rng = np.random.default_rng(100 * order + S)
    bc = rng.normal(size=(4, 3))
    err_lin, err_t = _check_case(oracle_mod, order, wp[0], tm[0], bc, w, seed=order * 7 + S)
    # measured (worst over S, w): waypoints / bc 9e-16 / 9e-14 / 2e-11 / 8e-10 at orders 2 / 3 / 4 / 5,
    # times 6e-11 / 4e-11 / 8e-11 / 1.4e-8 -- the restatement's dense fp64 inverses of M, not the difference quotients
    assert err_lin < (1e-8 if order == 5 else 2e-10), err_lin
    assert err_t < (1e-7 if order == 5 else 1e-9), err_t


def test_adjoint_golden_f3(oracle_mod):
    cases = load_cases("F3_wellscaled.json")
    assert cases
    for i, c in enumerate(cases):
        err_lin, err_t = _check_case(oracle_mod, c["order"], c["path"], c["time"], c["bc"], 0.0, seed=i)
        # measured: waypoints / bc <= 5.5e-11, times <= 1.6e-10 (order 4, S = 8 and 16)
        assert err_lin < 5e-10, (i, err_lin)
        assert err_t < 1.5e-9, (i, err_t)


def test_vjp_symbols_exported(csp):
    assert "csp_minsnap_solve_batch_vjp" in csp.EXPORTED_SYMBOLS
    assert "csp_minsnap_vjp_workspace_bytes" in csp.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(csp.LIB_PATH)
    assert lib.csp_minsnap_solve_batch_vjp and lib.csp_minsnap_vjp_workspace_bytes
    assert callable(csp.solve_batch_vjp) and callable(csp.solve_batch_autograd)


def _formula(order, smax, B, shared_bc):
    n = order - 1
    factors = (max(smax - 1, 0) * (n * n + 6 * n) * B * 8 + 255) // 256 * 256
    return factors + (12 * ((B + 63) // 64) * 8 if shared_bc else 0)


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_vjp_workspace_formula(csp, order):
    for S, B, per in [(16, 65536, False), (1, 100, False), (7, 3, True), (40, 129, False), (2, 1, True)]:
        d = csp.make_desc(order, B, S, bc_per_trajectory=per)
        assert csp.vjp_workspace_bytes(d) == _formula(order, S, B, not per), (S, B, per)
    off = np.array([0, 3, 3, 10], dtype=np.int64)
    d = csp.make_desc(order, 3, 0, seg_offsets_ptr=off.ctypes.data, max_segments=7)
    assert csp.vjp_workspace_bytes(d) == _formula(order, 7, 3, True)
    assert csp.vjp_workspace_bytes(csp.make_desc(order, 0, 5)) == 0


def test_vjp_workspace_unsupported_is_zero(csp):
    assert csp.vjp_workspace_bytes(csp.make_desc(1, 10, 4)) == 0
    assert csp.vjp_workspace_bytes(csp.make_desc(4, 10, 4, path_weight=0.1)) == 0
    assert csp.vjp_workspace_bytes(csp.make_desc(6, 10, 4)) == 0


def test_vjp_codes_without_device(csp):
    """path_weight and a NULL grad_coeffs are refused before the device check; a valid call without a gfx950 device
    returns CSP_ERR_NO_DEVICE (on a machine with one, the last part does not apply)."""
    f = csp.raw_lib().csp_minsnap_solve_batch_vjp
    wp, tm, bc = np.zeros((2, 4, 3)), np.ones((2, 3)), np.zeros((1, 4, 3))
    g = np.zeros((2, 3, 3, 8))
    args = lambda gco: (wp.ctypes.data, tm.ctypes.data, bc.ctypes.data, gco, None, None, None, None, None, 0, None)
    assert f(csp.make_desc(4, 2, 3, path_weight=0.5), *args(g.ctypes.data)) == -2
    assert f(csp.make_desc(4, 2, 3), *args(None)) == -1
    if csp.device_count() > 0:
        return
    assert f(csp.make_desc(4, 2, 3), *args(g.ctypes.data)) == -5
    with pytest.raises(csp.CspError) as e:
        csp.solve_batch_vjp(wp, tm, g)
    assert e.value.code == -5


def test_vjp_validation_codes(csp):
    """Argument checks come before the device check, so these hold on any machine."""
    f = csp.raw_lib().csp_minsnap_solve_batch_vjp
    wp, tm, bc = np.zeros((2, 4, 3)), np.ones((2, 3)), np.zeros((1, 4, 3))
    g = np.zeros((2, 3, 3, 8))
    args = (wp.ctypes.data, tm.ctypes.data, bc.ctypes.data, g.ctypes.data, None, None, None, None, None, 0, None)
    assert f(csp.make_desc(1, 2, 3), *args) == -2
    assert f(csp.make_desc(6, 2, 3), *args) == -2
    assert f(csp.make_desc(4, 2, 3, flags=csp.FLAG_SEGMENT_MAJOR), *args) == -2
    assert f(csp.make_desc(4, 2, 3, dtype=csp.DTYPE_F32, flags=csp.FLAG_F32_ARITH), *args) == -2
    assert f(csp.make_desc(4, 2, 3, path_weight=-1.0), *args) == -1
    assert f(csp.make_desc(0, 2, 3), *args) == -1
    assert f(None, *args) == -1
    assert f(csp.make_desc(4, 0, 3), None, None, None, None, None, None, None, None, None, 0, None) == 0
