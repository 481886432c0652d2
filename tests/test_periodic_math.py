"""CPU checks of the periodic (closed-loop) solve: the dense KKT of tests/periodic_ref.py against itself in mpmath, against
closed-form invariants and against the reference's open chain unrolled over many laps; and the C-ABI entry's argument
checks through the built library (no device needed)."""
import ctypes

import numpy as np
import pytest

from tests import periodic_ref as pr
from tests import synth


def _loop(S, seed, tlo=1.0, thi=3.0):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 3.0, size=(S, 3)), rng.uniform(tlo, thi, size=S)


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_numpy_kkt_matches_mpmath(order):
    # fp64 dense KKT against the same system at 40 digits.  Measured worst (coefficients per power, J, gradient):
    # 4.2e-13 / 1.2e-15 / 3.5e-15, 2.1e-13 / 5.2e-14 / 5.5e-14, 2.0e-11 / 2.4e-13 / 3.1e-13, 1.3e-10 / 6.2e-12 / 2.0e-11
    # at orders 2 / 3 / 4 / 5: the monomial KKT loses digits with the order, which is why the order-5 GPU gates are loose
    gate = {2: 5e-12, 3: 2e-12, 4: 2e-10, 5: 1.5e-9}[order]
    for S, (tlo, thi) in ((1, (1.0, 3.0)), (2, (1.0, 3.0)), (5, (1.0, 3.0)), (4, (4.0, 8.0))):
        P, T = _loop(S, 10 * order + S, tlo, thi)
        for w in (0.0, 0.07):
            c, J, g = pr.solve(order, P, T, w)
            cm, Jm, gm = pr.solve(order, P, T, w, dps=40)
            assert synth.rel_err_per_power(c, cm) < gate
            assert abs(J - Jm) <= gate * max(abs(Jm), 1e-300)
            assert np.max(np.abs(g - gm)) <= gate * max(np.max(np.abs(gm)), 1e-300)


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_continuity_at_every_knot(order):
    # derivatives 0..o-1 by the constraints, o..2o-2 by optimality (w = 0), the wrap included; 2o-1 jumps
    P, T = _loop(6, order)
    c, _, _ = pr.solve(order, P, T, dps=30)
    S = len(T)
    for k in range(2 * order - 1):
        for j in range(S):
            end = np.array([pr.eval_deriv(c[j, ax], k, T[j]) for ax in range(3)])
            start = np.array([pr.eval_deriv(c[(j + 1) % S, ax], k, 0.0) for ax in range(3)])
            scale = max(np.max(np.abs(start)), 1.0)
            assert np.max(np.abs(end - start)) < 1e-10 * scale, (k, j)
    k = 2 * order - 1
    jumps = [abs(pr.eval_deriv(c[j, 0], k, T[j]) - pr.eval_deriv(c[(j + 1) % S, 0], k, 0.0)) for j in range(S)]
    assert max(jumps) > 1e-6


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_symmetries(order):
    P, T = _loop(5, 50 + order)
    c, J, g = pr.solve(order, P, T, 0.03)
    gs = np.max(np.abs(g))
    tol = {2: 1e-11, 3: 1e-11, 4: 1e-9, 5: 1e-8}[order]   # fp64 dense KKT noise (test_numpy_kkt_matches_mpmath)
    # cyclic shift: the same loop started at another point
    c1, J1, g1 = pr.solve(order, np.roll(P, -2, axis=0), np.roll(T, -2), 0.03)
    assert synth.rel_err_per_power(c1, np.roll(c, -2, axis=0)) < tol
    assert abs(J1 - J) < tol * J and np.max(np.abs(g1 - np.roll(g, -2))) < tol * gs
    # reversal: the loop P_0, P_{S-1}, ..., P_1; its segment j is segment S-1-j run backwards
    S = len(T)
    Pr = np.roll(P[::-1], 1, axis=0)
    Tr = T[::-1].copy()
    cr, Jr, gr = pr.solve(order, Pr, Tr, 0.03)
    assert abs(Jr - J) < tol * J and np.max(np.abs(gr - g[::-1])) < tol * gs
    for j in range(S):
        jj = S - 1 - j
        for ax in range(3):
            for k in range(order):
                a = pr.eval_deriv(cr[j, ax], k, 0.0)
                b = (-1) ** k * pr.eval_deriv(c[jj, ax], k, T[jj])
                assert abs(a - b) < tol * max(1.0, abs(b)), (j, ax, k)
    # translation moves only the constant coefficients
    m = 2 * order
    shift = np.array([100.0, -30.0, 7.0])
    ct, Jt, _ = pr.solve(order, P + shift, T, 0.03)
    assert np.max(np.abs(ct[..., :m - 1] - c[..., :m - 1])) < tol * np.max(np.abs(c[..., :m - 1]))
    assert np.array_equal(ct[..., m - 1], P + shift)
    assert abs(Jt - J) < tol * J


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_time_scaling_and_euler(order):
    P, T = _loop(5, 70 + order)
    _, J, g = pr.solve(order, P, T, dps=30)
    _, J2, _ = pr.solve(order, P, 1.7 * T, dps=30)
    assert abs(J2 - 1.7 ** (1 - 2 * order) * J) < 1e-14 * J
    assert abs(np.dot(T, g) - (1 - 2 * order) * J) < 1e-14 * J


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_gradient_against_richardson(order):
    P, T = _loop(4, 90 + order)
    w = 0.05
    _, _, g = pr.solve(order, P, T, w, dps=30)
    h = 1e-3
    for j in range(len(T)):
        def f(d):
            Td = T.copy()
            Td[j] += d
            return pr.solve(order, P, Td, w, dps=30)[1]
        d1 = (f(h) - f(-h)) / (2 * h)
        d2 = (f(h / 2) - f(-h / 2)) / h
        rich = (4 * d2 - d1) / 3
        assert abs(rich - g[j]) < 1e-8 * max(1.0, np.max(np.abs(g))), (j, rich, g[j])


# The middle lap of the reference's open chain over K laps from rest (oracle/numpy_ref.py) against the periodic
# solution: the truncation decays by ~0.73 per segment at order 4 (0.88 at order 5).  K per order puts it below the
# gate; order 5 converges more slowly, would need far more laps and is left out.  The smaller K is checked to be farther away.
@pytest.mark.parametrize("order,laps,gate", [(2, 9, 1e-10), (3, 13, 1e-8), (4, 17, 1e-6)])
def test_unrolled_chain_converges(order, laps, gate):
    P, T = _loop(5, 123)
    c, _, _ = pr.solve(order, P, T, dps=30)
    e_short = synth.rel_err_per_power(pr.unrolled_middle_lap(order, P, T, laps - 4), c)
    e = synth.rel_err_per_power(pr.unrolled_middle_lap(order, P, T, laps), c)
    assert e < e_short
    assert e < gate, e


# ---- C-ABI argument checks (no device needed: each is decided before a device is looked for)

def _call(csp, desc, wp=64, tm=64, co=64, ws=None, wsb=0):
    p = lambda v: ctypes.c_void_p(v) if v else None
    return csp.raw_lib().csp_minsnap_solve_periodic_batch(ctypes.byref(desc) if desc is not None else None, p(wp), p(tm),
                                                          p(co), None, None, None, p(ws), wsb, None)


def test_capi_argument_checks(csp):
    ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
    d = csp.make_desc(4, 8, 5, mem_space=csp.MEM_DEVICE)
    assert _call(csp, None) == ERR_INVALID
    for kw in (dict(wp=0), dict(tm=0), dict(co=0)):
        assert _call(csp, d, **kw) == ERR_INVALID, kw
    for o in (1, 6, 9):
        assert _call(csp, csp.make_desc(o, 8, 5, mem_space=csp.MEM_DEVICE)) == ERR_UNSUPPORTED, o
    assert _call(csp, csp.make_desc(0, 8, 5, mem_space=csp.MEM_DEVICE)) == ERR_INVALID
    assert _call(csp, csp.make_desc(4, 8, 5, path_weight=0.2, mem_space=csp.MEM_DEVICE)) == ERR_UNSUPPORTED
    assert _call(csp, csp.make_desc(4, 8, 5, mem_space=csp.MEM_DEVICE, flags=csp.FLAG_SEGMENT_MAJOR)) == ERR_UNSUPPORTED
    assert _call(csp, csp.make_desc(4, 8, 5, mem_space=csp.MEM_DEVICE, flags=csp.FLAG_F32_ARITH)) == ERR_UNSUPPORTED
    need = csp.periodic_workspace_bytes(d)
    assert need > 0
    assert _call(csp, d, ws=256, wsb=need - 1) == ERR_WORKSPACE
    assert _call(csp, d, ws=None, wsb=need) == ERR_WORKSPACE
    assert _call(csp, d, ws=260, wsb=need) == ERR_WORKSPACE             # 8-byte alignment
    assert _call(csp, d, ws=256, wsb=need, co=72) == ERR_INVALID       # fp64 records need 16-byte alignment
    # B = 0 is a no-op, no device needed
    assert _call(csp, csp.make_desc(4, 0, 5, mem_space=csp.MEM_DEVICE), wp=0, tm=0, co=0) == 0
    # host memory, ragged: a segment count outside 0..max_segments
    off = np.array([0, 3, 2], dtype=np.int64)
    dr = csp.make_desc(4, 2, 0, mem_space=csp.MEM_HOST, seg_offsets_ptr=off.ctypes.data, max_segments=3)
    assert _call(csp, dr) == ERR_INVALID


def test_capi_workspace_bytes(csp):
    for o in (2, 3, 4, 5):
        n = o - 1
        for S, B in ((1, 7), (2, 64), (16, 65536), (5, 3)):
            d = csp.make_desc(o, B, S, mem_space=csp.MEM_DEVICE)
            want = ((S - 1) * (2 * n * n + 3 * n) * B * 8 + 255) // 256 * 256
            assert csp.periodic_workspace_bytes(d) == want, (o, S, B)
        off = np.array([0, 4, 4, 9], dtype=np.int64)
        d = csp.make_desc(o, 3, 0, dtype=csp.DTYPE_F32, seg_offsets_ptr=off.ctypes.data, max_segments=5)
        assert csp.periodic_workspace_bytes(d) == (4 * (2 * n * n + 3 * n) * 3 * 8 + 255) // 256 * 256
    for bad in (dict(order=1), dict(order=6), dict(path_weight=0.5), dict(flags=csp.FLAG_F32_ARITH),
                dict(flags=csp.FLAG_SEGMENT_MAJOR)):
        kw = dict(order=4, batch=8, num_segments=5)
        kw.update(bad)
        assert csp.periodic_workspace_bytes(csp.make_desc(**kw)) == 0, bad
    assert csp.periodic_workspace_bytes(csp.make_desc(4, 8, 0)) == 0   # ragged without offsets
