"""The periodic (closed-loop) solve (csp_minsnap_solve_periodic_batch) on the MI355X, against the dense KKT of
tests/periodic_ref.py, the shipped open-chain solve_batch (unrolled laps), closed-form invariants and itself."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import periodic_ref as pr
from tests import synth

pytestmark = pytest.mark.gpu

# Gates, per order, against the fp64 dense KKT, placed from a survey run on the MI355X (worst over test_vs_reference,
# test_ragged_every_length and the C3 subset, fp64 storage): per-power coefficients 2.2e-14 / 2.3e-11 / 4.0e-11 /
# 1.2e-9, J 3.2e-15 / 4.8e-13 / 3.3e-11 / 1.6e-9, gradient 5.5e-15 / 4.0e-13 / 6.1e-11 / 1.4e-9 at orders 2 / 3 / 4 / 5
# (DESIGN.md §13).  At order 5 the dense fp64 KKT is the less accurate side: it differs from itself at 40 digits by up
# to 1.3e-10 (test_periodic_math.py::test_numpy_kkt_matches_mpmath), and test_continuity_long_ragged holds the kernel to
# 3.5e-10 on its own.
GATE_C = {2: 2e-13, 3: 2e-10, 4: 4e-10, 5: 1e-8}
GATE_J = {2: 3e-14, 3: 5e-12, 4: 3e-10, 5: 1e-8}
GATE_G = {2: 5e-14, 3: 4e-12, 4: 6e-10, 5: 1e-8}
SURVEY = os.environ.get("CSP_PERIODIC_SURVEY")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _loops(B, S, seed, tlo=0.5, thi=2.0):
    rng = np.random.default_rng(seed)
    wp = rng.uniform(-10, 10, size=(B, 1, 3)) + np.cumsum(rng.normal(0, 1, size=(B, S, 3)), axis=1)
    return wp, rng.uniform(tlo, thi, size=(B, S))


def _ragged(lengths, seed):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    wp = rng.uniform(-10, 10, size=(int(off[-1]), 3)) + rng.normal(0, 2, size=(int(off[-1]), 3))
    return wp, rng.uniform(0.5, 2.0, size=int(off[-1])), off


def _gate(tag, order, got_c, ref_c, got_j=None, ref_j=None, got_g=None, ref_g=None, widen=1.0):
    e_c = synth.rel_err_per_power(got_c, ref_c) if got_c.size else 0.0
    e_j = float(np.max(np.abs(got_j - ref_j) / np.maximum(np.abs(ref_j), 1e-300))) if got_j is not None and got_j.size else 0.0
    e_g = 0.0
    if got_g is not None and got_g.size:
        e_g = float(np.max(np.abs(got_g - ref_g)) / max(np.max(np.abs(ref_g)), 1e-300))
    if SURVEY:
        print("SURVEY %s order %d: coeffs %.2e  J %.2e  grad %.2e" % (tag, order, e_c, e_j, e_g))
    assert e_c < widen * GATE_C[order], (tag, e_c)
    assert e_j < widen * GATE_J[order], (tag, e_j)
    assert e_g < widen * GATE_G[order], (tag, e_g)


@pytest.mark.parametrize("order", [2, 3, 4, 5])
@pytest.mark.parametrize("S", [1, 2, 3, 5, 16, 64])
def test_vs_reference(csp, order, S):
    B = 4
    wp, tm = _loops(B, S, 100 * order + S)
    wper = np.array([0.0, 0.01, 0.1, 0.5])
    for w in (0.0, 0.05, wper):
        kw = dict(vel_zero_weight_per_traj=_dev(wper)) if np.ndim(w) else dict(vel_zero_weight=w)
        r = csp.solve_periodic_batch(_dev(wp), _dev(tm), order=order, want_cost=True, want_grad=True, **kw)
        torch.cuda.synchronize()
        assert not _host(r.status).any()
        rc, rj, rg = pr.solve_batch(order, wp, tm, w)
        _gate("S=%d w=%s" % (S, "per" if np.ndim(w) else w), order, _host(r.coeffs), rc, _host(r.cost), rj,
              _host(r.grad_times), rg)


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_ragged_every_length(csp, order):
    lengths = np.random.default_rng(order).permutation(np.arange(0, 65))
    wp, tm, off = _ragged(lengths, 7 + order)
    w = np.linspace(0.0, 0.2, len(lengths))
    for host in (True, False):
        args = (wp, tm) if host else (_dev(wp), _dev(tm))
        r = csp.solve_periodic_batch(*args, order=order, seg_offsets=off if host else _dev(off),
                                     vel_zero_weight_per_traj=w if host else _dev(w), want_cost=True, want_grad=True)
        torch.cuda.synchronize()
        st, cost = _host(r.status), _host(r.cost)
        assert not st.any()
        assert cost[lengths == 0].tolist() == [0.0] * int(np.sum(lengths == 0))
        rc, rj, rg = pr.solve_batch(order, wp, tm, w, seg_offsets=off)
        co, g = _host(r.coeffs), _host(r.grad_times)
        for b in range(len(lengths)):
            s0, s1 = off[b], off[b + 1]
            _gate("ragged S=%d" % lengths[b], order, co[s0:s1], rc[s0:s1], cost[b:b + 1], rj[b:b + 1], g[s0:s1], rg[s0:s1])


def _knot_jumps(co, tm, upto):
    """max over knots (the wrap included) and derivative k = 0..upto of |p_j^(k)(T_j) - p_{j+1}^(k)(0)|, relative to the
    largest |p^(k)(0)| of the loop."""
    S = len(tm)
    worst = 0.0
    for k in range(upto + 1):
        end = np.array([[pr.eval_deriv(co[j, ax], k, tm[j]) for ax in range(3)] for j in range(S)])
        start = np.array([[pr.eval_deriv(co[(j + 1) % S, ax], k, 0.0) for ax in range(3)] for j in range(S)])
        worst = max(worst, float(np.max(np.abs(end - start)) / max(np.max(np.abs(start)), 1e-300)))
    return worst


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_continuity_long_ragged(csp, order):
    # At w = 0 the minimiser is the unique periodic spline of continuity C^(2o-2) through the points: derivatives up to
    # o-1 by the constraints, o..2o-2 by optimality.  One batch reaches S = 1024.
    # Measured worst relative jump (derivatives 0..2o-2) over the loops of S <= 300: 4.3e-15 / 2.6e-14 / 1.2e-12 / 3.5e-10
    # at orders 2 / 3 / 4 / 5; the S = 1024 loop passes the same gates.
    lengths = np.array([1024, 3, 300, 1, 2, 77])
    wp, tm, off = _ragged(lengths, 31 + order)
    r = csp.solve_periodic_batch(_dev(wp), _dev(tm), order=order, seg_offsets=_dev(off))
    torch.cuda.synchronize()
    assert not _host(r.status).any()
    co = _host(r.coeffs)
    gate = {2: 1e-13, 3: 1e-12, 4: 3e-11, 5: 1e-8}[order]
    for b in range(len(lengths)):
        s0, s1 = off[b], off[b + 1]
        jump = _knot_jumps(co[s0:s1], tm[s0:s1], 2 * order - 2)
        if SURVEY:
            print("SURVEY continuity S=%d order %d: %.2e" % (lengths[b], order, jump))
        assert jump < gate, (lengths[b], jump)


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_single_segment_is_the_constant(csp, order):
    wp, tm = _loops(8, 1, 5)
    for w in (0.0, 0.3):
        r = csp.solve_periodic_batch(wp, tm, order=order, vel_zero_weight=w, want_cost=True, want_grad=True)
        co = r.coeffs
        assert np.all(co[..., :-1] == 0.0)
        assert np.array_equal(co[:, 0, :, -1], wp[:, 0, :])
        assert np.all(r.cost == 0.0) and np.all(r.grad_times == 0.0) and not r.status.any()


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_two_segments_sum_couplings(csp, order):
    # S = 2: both segments couple the same two knots; their blocks add (C_0^T + C_1).  Unequal times (up to 6 s, where
    # the fp64 dense KKT loses digits): against the KKT at 40 digits.  The spread of T^(2o-1) costs the kernel digits at
    # order 5: measured 2.2e-8 per power there, hence the widened gate at that order
    wp, tm = _loops(6, 2, 77)
    tm[:, 1] *= 3.0
    r = csp.solve_periodic_batch(wp, tm, order=order, vel_zero_weight=0.02, want_cost=True, want_grad=True)
    rc, rj, rg = pr.solve_batch(order, wp, tm, 0.02, dps=40)
    _gate("S=2 asym", order, r.coeffs, rc, r.cost, rj, r.grad_times, rg, widen=10.0 if order == 5 else 1.0)


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_fp32_storage(csp, order):
    # fp32 storage, fp64 arithmetic: against the fp64 reference on the fp32-rounded inputs; the gate is the fp32
    # rounding of the stored coefficients
    wp, tm = _loops(8, 12, 900 + order)
    wp32, tm32 = wp.astype(np.float32), tm.astype(np.float32)
    r = csp.solve_periodic_batch(_dev(wp32), _dev(tm32), order=order, want_cost=True, want_grad=True)
    torch.cuda.synchronize()
    rc, rj, rg = pr.solve_batch(order, wp32.astype(np.float64), tm32.astype(np.float64))
    co = _host(r.coeffs)
    assert co.dtype == np.float32 and _host(r.grad_times).dtype == np.float32
    e = synth.rel_err_per_power(co, rc)
    assert e < 5e-7, e
    assert np.max(np.abs(_host(r.cost) - rj) / rj) < 1e-9
    assert np.max(np.abs(_host(r.grad_times) - rg)) / np.max(np.abs(rg)) < 5e-7


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_cyclic_shift_and_regular_polygon(csp, order):
    wp, tm = _loops(4, 7, 41)
    r0 = csp.solve_periodic_batch(wp, tm, order=order, want_cost=True)
    for sh in (1, 3):
        r1 = csp.solve_periodic_batch(np.roll(wp, -sh, axis=1), np.roll(tm, -sh, axis=1), order=order, want_cost=True)
        e = synth.rel_err_per_power(r1.coeffs, np.roll(r0.coeffs, -sh, axis=1))
        assert e < GATE_C[order], e
        assert np.max(np.abs(r1.cost - r0.cost) / r0.cost) < GATE_J[order]
    # a regular polygon with equal times: segment j+1 is segment j rotated by 2 pi / S about the centre
    S = 8
    ang = 2 * np.pi * np.arange(S) / S
    poly = np.stack([5 * np.cos(ang), 5 * np.sin(ang), np.full(S, 2.0)], axis=1)[None]
    r = csp.solve_periodic_batch(poly, np.full((1, S), 1.5), order=order)
    co = r.coeffs[0]
    c, s = np.cos(2 * np.pi / S), np.sin(2 * np.pi / S)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    for j in range(S):
        want = rot @ co[j, :, :-1]   # every non-constant coefficient rotates with the polygon
        e = np.max(np.abs(co[(j + 1) % S, :, :-1] - want)) / np.max(np.abs(co[:, :, :-1]))
        assert e < 100 * GATE_C[order], (j, e)


@pytest.mark.parametrize("order", [2, 3, 4])
def test_unrolled_open_chain_converges(csp, order):
    # the shipped open-chain solve over K laps from rest: its middle lap converges geometrically to the periodic answer
    # (per lap of 5 segments ~0.2 at order 4); K = 15 puts the truncation below the gates.
    S, K = 5, 15
    wp, tm = _loops(3, S, 5150)
    per = csp.solve_periodic_batch(wp, tm, order=order).coeffs
    chain = np.concatenate([np.tile(wp, (1, K, 1)), wp[:, :1]], axis=1)
    r = csp.solve_batch(chain, np.tile(tm, (1, K)), order=order, force_generic=True)
    mid = r.coeffs.reshape(3, K * S, 3, 2 * order)[:, (K // 2) * S:(K // 2 + 1) * S]
    e = synth.rel_err_per_power(mid, per)
    assert e < {2: 1e-12, 3: 1e-9, 4: 1e-6}[order], e


def test_sampled_lap_closes(csp):
    wp, tm = _loops(4, 9, 8)
    r = csp.solve_periodic_batch(_dev(wp), _dev(tm), order=4)
    samples, counts, _ = csp.sample_batch(_dev(tm), r.coeffs, 0.25, 4096)
    torch.cuda.synchronize()
    samples, counts = _host(samples), _host(counts)
    for b in range(4):
        n = int(counts[b])
        assert n > 10
        assert np.max(np.abs(samples[b, n - 1] - samples[b, 0])) < 1e-9 * np.max(np.abs(wp[b]))
        assert np.max(np.abs(samples[b, 0] - wp[b, 0])) < 1e-12 * np.max(np.abs(wp[b]))


def test_bit_equality(csp):
    wp, tm = _loops(300, 16, 3)
    h = csp.solve_periodic_batch(wp, tm, order=4, vel_zero_weight=0.01)
    d1 = csp.solve_periodic_batch(_dev(wp), _dev(tm), order=4, vel_zero_weight=0.01)
    d2 = csp.solve_periodic_batch(_dev(wp), _dev(tm), order=4, vel_zero_weight=0.01, want_cost=True, want_grad=True)
    d3 = csp.solve_periodic_batch(_dev(wp), _dev(tm), order=4, vel_zero_weight=0.01, want_cost=True, want_grad=True)
    d4 = csp.solve_periodic_batch(_dev(wp), _dev(tm), order=4, vel_zero_weight=0.01, want_grad=True)
    torch.cuda.synchronize()
    for d in (d1, d2, d3, d4):
        assert np.array_equal(_host(d.coeffs).view(np.uint64), h.coeffs.view(np.uint64))
    assert np.array_equal(_host(d2.cost).view(np.uint64), _host(d3.cost).view(np.uint64))
    assert np.array_equal(_host(d2.grad_times).view(np.uint64), _host(d3.grad_times).view(np.uint64))
    assert np.array_equal(_host(d2.grad_times).view(np.uint64), _host(d4.grad_times).view(np.uint64))


def test_empty_and_large_batch(csp):
    r = csp.solve_periodic_batch(np.zeros((0, 16, 3)), np.zeros((0, 16)), order=4, want_cost=True)
    assert r.coeffs.shape == (0, 16, 3, 8) and r.cost.shape == (0,)
    B, S = 65536, 16
    wp, tm = synth.make_batch(B, S, config_id=3)
    wp = np.ascontiguousarray(wp[:, :S])
    r = csp.solve_periodic_batch(_dev(wp), _dev(tm), order=4, want_cost=True, want_grad=True)
    torch.cuda.synchronize()
    assert not _host(r.status).any()
    idx = np.random.default_rng(0).choice(B, 24, replace=False)
    rc, rj, rg = pr.solve_batch(4, wp[idx], tm[idx])
    _gate("C3 subset", 4, _host(r.coeffs)[idx], rc, _host(r.cost)[idx], rj, _host(r.grad_times)[idx], rg)


def test_status_bits(csp):
    wp, tm = _loops(6, 5, 12)
    tm[1, 2] = 0.0
    wp[3, 4, 1] = np.inf
    r = csp.solve_periodic_batch(_dev(wp), _dev(tm), order=4, want_cost=True, want_grad=True)
    torch.cuda.synchronize()
    st = _host(r.status)
    assert st[1] & csp.TRAJ_NOT_SPD
    assert st[3] & csp.TRAJ_NONFINITE
    ok = [0, 2, 4, 5]
    assert not st[ok].any()
    rc, rj, rg = pr.solve_batch(4, wp[ok], tm[ok])
    _gate("status neighbours", 4, _host(r.coeffs)[ok], rc, _host(r.cost)[ok], rj, _host(r.grad_times)[ok], rg)


def test_device_error_codes(csp):
    lib = csp.raw_lib()
    wp, tm = _dev(np.zeros((4, 5, 3))), _dev(np.ones((4, 5)))
    co = torch.empty((4, 5, 3, 8), dtype=torch.float64, device="cuda:0")
    d = csp.make_desc(4, 4, 5, mem_space=csp.MEM_DEVICE)
    need = csp.periodic_workspace_bytes(d)
    assert need == (4 * (2 * 9 + 9) * 4 * 8 + 255) // 256 * 256
    ws = torch.empty(need, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream

    def call(desc, wsb=need, coeffs=co.data_ptr(), w=wp.data_ptr()):
        return lib.csp_minsnap_solve_periodic_batch(ctypes.byref(desc), w, tm.data_ptr(), coeffs, None, None, None,
                                                    ws.data_ptr(), wsb, ctypes.c_void_p(st))
    assert call(d) == 0
    assert call(d, wsb=need - 1) == -3
    assert call(d, coeffs=co.data_ptr() + 8) == -1
    assert call(d, w=None) == -1
    for bad, code in ((dict(order=1), -2), (dict(order=6), -2), (dict(path_weight=0.1), -2),
                      (dict(flags=csp.FLAG_F32_ARITH), -2), (dict(flags=csp.FLAG_SEGMENT_MAJOR), -2)):
        kw = dict(order=4, batch=4, num_segments=5, mem_space=csp.MEM_DEVICE)
        kw.update(bad)
        assert call(csp.make_desc(**kw)) == code, bad
    torch.cuda.synchronize()


def test_periodic_time_alloc(csp):
    wp, _ = _loops(5, 6, 2)
    t = csp.periodic_time_alloc_batch(wp, 2.0, 0.3)
    closed = np.concatenate([wp, wp[:, :1]], axis=1)
    want = np.maximum(np.linalg.norm(np.diff(closed, axis=1), axis=2) / 2.0, 0.3)
    assert np.allclose(t, want, rtol=1e-15, atol=0)
    lengths = np.array([3, 0, 1, 6])
    rw, _, off = _ragged(lengths, 4)
    for host in (True, False):
        tr = csp.periodic_time_alloc_batch(rw if host else _dev(rw), 2.0, 0.3, seg_offsets=off if host else _dev(off))
        tr = _host(tr)
        for b in range(len(lengths)):
            p = rw[off[b]:off[b + 1]]
            if len(p) == 0:
                continue
            want = np.maximum(np.linalg.norm(np.roll(p, -1, axis=0) - p, axis=1) / 2.0, 0.3)
            assert np.allclose(tr[off[b]:off[b + 1]], want, rtol=1e-15, atol=0)
