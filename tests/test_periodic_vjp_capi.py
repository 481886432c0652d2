"""The C-ABI surface of csp_minsnap_solve_periodic_batch_vjp without a device: the two symbols, the workspace formula
and every argument check, all of which come back before a device is looked for."""
import ctypes

import numpy as np
import pytest

OK, INVALID_ARG, UNSUPPORTED, WORKSPACE, NO_DEVICE = 0, -1, -2, -3, -5


def test_symbols_exported(csp):
    for name in ("csp_minsnap_solve_periodic_batch_vjp", "csp_minsnap_periodic_vjp_workspace_bytes"):
        assert name in csp.EXPORTED_SYMBOLS
        assert getattr(ctypes.CDLL(csp.LIB_PATH), name)
    assert callable(csp.solve_periodic_batch_vjp) and callable(csp.solve_periodic_batch_autograd)
    assert callable(csp.periodic_vjp_workspace_bytes)


def _formula(order, smax, B):
    n = order - 1
    return (max(smax - 1, 0) * (2 * n * n + 6 * n) * B * 8 + 255) // 256 * 256


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_workspace_formula(csp, order):
    for S, B in [(16, 65536), (1, 100), (7, 3), (40, 129), (2, 1), (17, 65)]:
        assert csp.periodic_vjp_workspace_bytes(csp.make_desc(order, B, S)) == _formula(order, S, B), (S, B)
        assert csp.periodic_vjp_workspace_bytes(csp.make_desc(order, B, S, dtype=csp.DTYPE_F32)) == _formula(order, S, B)
    off = np.array([0, 3, 3, 10], dtype=np.int64)
    d = csp.make_desc(order, 3, 0, seg_offsets_ptr=off.ctypes.data, max_segments=9)   # sized by max_segments, not the data
    assert csp.periodic_vjp_workspace_bytes(d) == _formula(order, 9, 3)
    assert csp.periodic_vjp_workspace_bytes(csp.make_desc(order, 0, 5)) == 0
    assert csp.periodic_vjp_workspace_bytes(csp.make_desc(order, 7, 1)) == 0


def _unsupported(csp):
    return {"path_weight": csp.make_desc(4, 4, 3, path_weight=0.1),
            "order 1": csp.make_desc(1, 4, 3),
            "order 6": csp.make_desc(6, 4, 3),
            "segment major": csp.make_desc(4, 4, 3, flags=csp.FLAG_SEGMENT_MAJOR),
            "f32 arithmetic": csp.make_desc(4, 4, 3, dtype=csp.DTYPE_F32, flags=csp.FLAG_F32_ARITH)}


def test_workspace_of_unsupported_descriptors_is_zero(csp):
    for name, d in _unsupported(csp).items():
        assert csp.periodic_vjp_workspace_bytes(d) == 0, name
    bad = csp.make_desc(4, 4, 3)
    bad.abi_version = 99
    assert csp.periodic_vjp_workspace_bytes(bad) == 0
    assert csp.periodic_vjp_workspace_bytes(csp.make_desc(4, 4, 0)) == 0   # ragged without offsets


def _call(csp, desc, wp, tm, gco, gcost, gwp, gtm, ws=None, ws_bytes=0):
    p = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)
    return csp.raw_lib().csp_minsnap_solve_periodic_batch_vjp(ctypes.byref(desc), p(wp), p(tm), p(gco), p(gcost), p(gwp), p(gtm),
                                                              None, p(ws), ws_bytes, None)


def test_argument_errors_come_back_without_a_device(csp):
    B, S, order = 4, 3, 4
    wp, tm, gco = np.zeros((B, S, 3)), np.ones((B, S)), np.zeros((B, S, 3, 2 * order))
    gwp, gtm, gj = np.zeros((B, S, 3)), np.zeros((B, S)), np.zeros(B)
    for name, d in _unsupported(csp).items():
        assert _call(csp, d, wp, tm, gco, gj, gwp, gtm) == UNSUPPORTED, name
    host = csp.make_desc(order, B, S)
    assert _call(csp, host, wp, tm, gco, gj, None, None) == INVALID_ARG          # both outputs null
    assert _call(csp, host, None, tm, gco, gj, gwp, gtm) == INVALID_ARG
    assert _call(csp, host, wp, None, gco, gj, gwp, gtm) == INVALID_ARG
    assert _call(csp, host, wp, tm, None, gj, gwp, gtm) == INVALID_ARG
    bad = csp.make_desc(order, B, S)
    bad.abi_version = 99
    assert _call(csp, bad, wp, tm, gco, gj, gwp, gtm) == INVALID_ARG
    assert _call(csp, csp.make_desc(order, 0, S), None, None, None, None, None, None) == OK   # an empty batch is a no-op
    # ragged host call: offsets outside 0..max_segments
    off = np.array([0, 3, 2, 8, 12], dtype=np.int64)
    rag = csp.make_desc(order, B, 0, seg_offsets_ptr=off.ctypes.data, max_segments=6)
    w12, t12, g12 = np.zeros((12, 3)), np.ones(12), np.zeros((12, 3, 2 * order))
    assert _call(csp, rag, w12, t12, g12, None, np.zeros((12, 3)), None) == INVALID_ARG
    # device-memory form: workspace and alignment are checked from the pointers' values alone
    dev = csp.make_desc(order, B, S, mem_space=csp.MEM_DEVICE)
    need = csp.periodic_vjp_workspace_bytes(dev)
    assert need == _formula(order, S, B) > 0
    assert _call(csp, dev, 4096, 4096, 4096, None, 4096, None, None, 0) == WORKSPACE
    assert _call(csp, dev, 4096, 4096, 4096, None, 4096, None, 8192, need - 1) == WORKSPACE
    assert _call(csp, dev, 4096, 4096, 4096, None, 4096, None, 8196, need) == WORKSPACE       # not 8-byte aligned
    assert _call(csp, dev, 4096, 4096, 4104, None, 4096, None, 8192, need) == INVALID_ARG     # grad_coeffs not 16-byte aligned
    dev32 = csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, mem_space=csp.MEM_DEVICE)
    assert _call(csp, dev32, 4096, 4096, 4100, None, 4096, None, 8192, need) == INVALID_ARG   # fp32: 8-byte aligned
    if csp.device_count() == 0:   # everything in order: only now is a device looked for
        assert _call(csp, host, wp, tm, gco, gj, gwp, gtm) == NO_DEVICE
        assert _call(csp, host, wp, tm, gco, None, None, gtm) == NO_DEVICE
        assert _call(csp, dev32, 4096, 4096, 4104, None, 4096, None, 8192, need) == NO_DEVICE
        with pytest.raises(csp.CspError) as e:
            csp.solve_periodic_batch_vjp(wp, tm, gco, order=order)
        assert e.value.code == NO_DEVICE
