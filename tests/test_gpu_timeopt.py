"""The snap cost, its time gradient and the segment-time optimiser (csp_minsnap_cost_batch,
csp_minsnap_optimize_times_batch) on the MI355X, against the numpy restatement (tests/timeopt_ref.py)."""
import numpy as np
import pytest
import torch

from oracle.numpy_ref import build_Q
from tests import synth
from tests.conftest import load_cases
from tests.timeopt_ref import NOT_CONVERGED, cost_from_coeffs, cost_grad, optimize, pg_measure

pytestmark = pytest.mark.gpu

# kernel vs numpy, per order: relative error of J, and per trajectory max-abs gradient error over max-abs gradient.
# Measured on the MI355X (worst over every case of test_cost_vs_numpy, fp64 storage): J 1.2e-15 / 8.9e-15 / 8.1e-13 /
# 4.2e-11, gradient 1.6e-15 / 1.0e-13 / 4.0e-12 / 2.4e-10 at orders 2 / 3 / 4 / 5
GATE_J = {2: 1e-13, 3: 1e-13, 4: 1e-11, 5: 1e-9}
GATE_G = {2: 1e-13, 3: 1e-12, 4: 1e-10, 5: 1e-8}
# the check through the VJP carries the VJP's own rounding (tests/test_gpu_vjp.py)
GATE_VJP = {2: 1e-10, 3: 1e-9, 4: 1e-7, 5: 1e-5}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _ragged(B, seed, smax=9):
    rng = np.random.default_rng(seed)
    S = rng.integers(1, smax + 1, size=B)
    off = np.concatenate([[0], np.cumsum(S)]).astype(np.int64)
    wps, tms = [], []
    for b in range(B):
        wp, tm = synth.make_batch(1, int(S[b]), config_id=3, offset=seed * 31 + b)
        wps.append(wp[0])
        tms.append(tm[0])
    return np.concatenate(wps), np.concatenate(tms), off


def _split(off, wp, tm):
    return [(wp[off[b] + b:off[b + 1] + b + 1], tm[off[b]:off[b + 1]]) for b in range(len(off) - 1)]


def _cost(csp, order, wp, tm, bc, w, host, off=None, f32=False):
    kw = dict(order=order)
    if np.ndim(w):
        kw["vel_zero_weight_per_traj"] = w if host else _dev(w)
    else:
        kw["vel_zero_weight"] = w
    dt = np.float32 if f32 else np.float64
    wp, tm, bc = wp.astype(dt), tm.astype(dt), bc.astype(dt)
    if host:
        r = csp.snap_cost_batch(wp, tm, bc, seg_offsets=off, **kw)
    else:
        r = csp.snap_cost_batch(_dev(wp), _dev(tm), _dev(bc), seg_offsets=None if off is None else _dev(off), **kw)
        torch.cuda.synchronize()
    return _host(r.cost), _host(r.grad_times).astype(np.float64), _host(r.status)


def _check_cost(order, pieces, bc, w, J, g, st, tag, f32=False):
    assert not st.any(), (tag, st)
    B = len(pieces)
    bc = bc.reshape(-1, 4, 3)
    wv = np.broadcast_to(np.asarray(w, dtype=np.float64), (B,))
    ej = eg = 0.0
    pos = 0
    for b, (p, t) in enumerate(pieces):
        if f32:
            p, t = p.astype(np.float32).astype(np.float64), t.astype(np.float32).astype(np.float64)
        Jr, gr = cost_grad(order, p, t, (bc[b] if bc.shape[0] > 1 else bc[0]).astype(np.float32 if f32 else np.float64),
                           wv[b])
        ej = max(ej, abs(J[b] - Jr) / abs(Jr))
        gk = g[pos:pos + len(t)]
        pos += len(t)
        eg = max(eg, np.max(np.abs(gk - gr)) / np.max(np.abs(gr)))
    # fp32 storage: the gradient is rounded to fp32 on the way out
    gate_g = max(GATE_G[order], 2e-7) if f32 else GATE_G[order]
    assert ej < GATE_J[order] and eg < gate_g, (tag, ej, eg)
    print("%s: J %.2e  grad %.2e" % (tag, ej, eg))


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_cost_vs_numpy(csp, order):
    i = 0
    for S in (1, 2, 5, 16):
        for per_bc, per_w, host, f32 in [(False, False, True, False), (True, True, False, False), (True, False, False, True),
                                         (False, True, True, True)]:
            i += 1
            B = 5
            wp, tm = synth.make_batch(B, S, config_id=3, offset=17 * order + i)
            rng = np.random.default_rng(i)
            bc = rng.normal(size=(B if per_bc else 1, 4, 3))
            w = rng.uniform(0, 0.5, size=B) if per_w else 0.3
            J, g, st = _cost(csp, order, wp, tm, bc, w, host, f32=f32)
            _check_cost(order, [(wp[b], tm[b]) for b in range(B)], bc, w, J, g.reshape(-1), st,
                        "o%d S%d per_bc=%d per_w=%d host=%d f32=%d" % (order, S, per_bc, per_w, host, f32), f32)
    for host in (True, False):
        wp, tm, off = _ragged(7, seed=order + 10 * host)
        bc = np.random.default_rng(order).normal(size=(7, 4, 3))
        J, g, st = _cost(csp, order, wp, tm, bc, 0.1, host, off=off)
        _check_cost(order, _split(off, wp, tm), bc, 0.1, J, g, st, "o%d ragged host=%d" % (order, host))


def test_cost_goldens(csp):
    for fname in ("F2_readme_uav31.json", "F3_wellscaled.json"):
        for c in load_cases(fname):
            o = c["order"]
            r = csp.snap_cost_batch(c["path"][None], c["time"][None], c["bc"][None], order=o)
            assert not r.status.any()
            Jr, gr = cost_grad(o, c["path"], c["time"], c["bc"])
            ej, eg = abs(r.cost[0] - Jr) / Jr, np.max(np.abs(r.grad_times[0] - gr)) / np.max(np.abs(gr))
            print("%s: J %.2e  grad %.2e" % (fname, ej, eg))
            assert ej <= 1e-8 and eg <= 1e-6, (fname, ej, eg)
            # the golden coefficients are the dense fp64 reference's: not the optimum to all digits, so their cost is
            # an upper bound (F2, the README flight at kilometre scale: 0.5 % above; F3 agrees to 1e-9)
            Jg = cost_from_coeffs(o, c["coeff"], c["time"])
            assert r.cost[0] <= Jg * (1 + 1e-9), (fname, r.cost[0], Jg)
            if fname.startswith("F3"):
                assert abs(r.cost[0] - Jg) <= 1e-9 * Jg


def _explicit_T_terms(order, c, T, w):
    """At fixed coefficients, d/dT_j of sum_ax [int_0^T (p^(o))^2 + w (v(0)^2 + v(T)^2)] = p^(o)(T)^2 + 2 w v(T) a(T)."""
    out = 0.0
    for ax in range(3):
        po = np.polyval(np.polyder(c[ax], order), T)
        v, a = np.polyval(np.polyder(c[ax], 1), T), np.polyval(np.polyder(c[ax], 2), T)
        out += po * po + 2 * w * v * a
    return out


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_gradient_through_vjp(csp, order):
    """dJ/dT_j = VJP(p_bar = dJ/dcoeffs at fixed T).times_j + the explicit T terms, summed over the axes."""
    B, S, w = 4, 5, 0.2
    wp, tm = synth.make_batch(B, S, config_id=3, offset=5 * order)
    bc = np.random.default_rng(order).normal(size=(1, 4, 3))
    co = csp.solve_batch(wp, tm, bc, order=order, vel_zero_weight=w).coeffs
    m = 2 * order
    pbar = np.zeros_like(co)
    expl = np.zeros((B, S))
    for b in range(B):
        for j in range(S):
            Q = build_Q(order, np.array([tm[b, j]]))
            vrow = lambda t: np.array([(m - 1 - i) * t ** (m - 2 - i) if i < m - 1 else 0.0 for i in range(m)])
            V = np.outer(vrow(0.0), vrow(0.0)) + np.outer(vrow(tm[b, j]), vrow(tm[b, j]))
            for ax in range(3):
                pbar[b, j, ax] = 2 * (Q + w * V) @ co[b, j, ax]
            expl[b, j] = _explicit_T_terms(order, co[b, j], tm[b, j], w)
    gv = csp.solve_batch_vjp(wp, tm, pbar, bc=bc, order=order, vel_zero_weight=w, want=("times",)).times
    r = csp.snap_cost_batch(wp, tm, bc, order=order, vel_zero_weight=w)
    ref = gv + expl
    err = np.max(np.abs(r.grad_times - ref)) / np.max(np.abs(ref))
    print("o%d through the VJP: %.2e" % (order, err))
    assert err < GATE_VJP[order], err


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_time_penalty_closed_form(csp, order):
    """S = 1, zero bc: J(T) = J(1) T^(1-2o), so J + rho T is minimal at T* = ((2o-1) J(1) / rho)^(1/(2o))."""
    wp, _ = synth.make_batch(3, 1, config_id=3, offset=order)
    one = np.ones((3, 1))
    J1 = csp.snap_cost_batch(wp, one, order=order).cost
    rho = 0.5 * float(J1.min())
    r = csp.optimize_times_batch(wp, one, order=order, mode="time_penalty", time_weight=rho, min_time=1e-3, tol=1e-9,
                                 max_iters=200)
    assert not r.status.any(), r.status
    Ts = ((2 * order - 1) * J1 / rho) ** (1.0 / (2 * order))
    assert np.max(np.abs(r.times[:, 0] - Ts) / Ts) < 1e-7, (r.times[:, 0], Ts)


@pytest.mark.parametrize("order", [3, 4])
def test_mirror_symmetric_equal_times(csp, order):
    wp = np.array([[[-1.0, 0.0, 0.0], [0.0, 0.7, 0.2], [1.0, 0.0, 0.0]]])
    r = csp.optimize_times_batch(wp, np.array([[0.6, 1.4]]), order=order, tol=1e-8, max_iters=200)
    assert not r.status.any()
    assert abs(r.times[0, 0] - r.times[0, 1]) < 1e-6 * r.times[0].sum(), r.times
    assert abs(r.times[0].sum() - 2.0) <= 1e-12 * 2.0


def _batch_problem(order, B, S, seed):
    wp, tm = synth.make_batch(B, S, config_id=3, offset=seed)
    bc = np.random.default_rng(seed).normal(size=(B, 4, 3)) * 0.5
    return wp, tm, bc


def _invariants(order, wp, tm, bc, w, r, mode, rho, tmin, tol, pieces=None, check_ref=4):
    T, obj, it, st = (_host(x) for x in (r.times, r.objective, r.iterations, r.status))
    pieces = pieces or [(wp[b], tm[b]) for b in range(len(tm))]
    T = T.reshape(-1) if T.ndim > 1 else T
    pos = 0
    nconv = 0
    for b, (p, t) in enumerate(pieces):
        tb = T[pos:pos + len(t)]
        pos += len(t)
        assert st[b] & ~NOT_CONVERGED == 0, (b, st[b])
        assert obj[b, 1] <= obj[b, 0], (b, obj[b])
        assert tb.min() >= tmin
        if mode == "fixed_total":
            assert abs(tb.sum() - t.sum()) <= 1e-12 * t.sum(), (b, tb.sum(), t.sum())
        bcb = bc[b] if bc.shape[0] > 1 else bc[0]
        J, g = cost_grad(order, p, tb, bcb, w)
        f = J + (rho * tb.sum() if mode == "time_penalty" else 0.0)
        assert abs(f - obj[b, 1]) <= (1e-6 if order == 5 else 1e-8) * abs(f), (b, f, obj[b, 1])
        if st[b] == 0:
            nconv += 1
            # the reference's gradient has its own rounding: a 2x margin on the measure
            pg = pg_measure(tb, g + (rho if mode == "time_penalty" else 0.0), t.mean(), obj[b, 0], tmin,
                            t.sum() if mode == "fixed_total" else None)
            assert pg <= 2 * tol, (b, pg)
        if b < check_ref:
            ref = optimize(order, p, t, bcb, w, mode, rho, tmin, tol, 500)
            assert abs(ref["f"] - obj[b, 1]) <= (1e-6 if order == 5 else 2e-7) * ref["f"], (b, ref["f"], obj[b, 1])
    return nconv


@pytest.mark.parametrize("order", [2, 3, 4, 5])
@pytest.mark.parametrize("mode", ["fixed_total", "time_penalty"])
def test_optimiser_invariants(csp, order, mode):
    B, S, tmin, tol = 32, 6, 0.1, 1e-6
    wp, tm, bc = _batch_problem(order, B, S, seed=order * 3 + (mode == "fixed_total"))
    rho = 0.0
    if mode == "time_penalty":
        J = csp.snap_cost_batch(wp, tm, bc, order=order).cost
        rho = float(np.median(J / tm.sum(axis=1)))
    r = csp.optimize_times_batch(wp, tm, bc, order=order, mode=mode, time_weight=rho, min_time=tmin, tol=tol,
                                 max_iters=300)
    nconv = _invariants(order, wp, tm, bc, 0.0, r, mode, rho, tmin, tol)
    print("o%d %s: converged %d / %d, iterations %s" % (order, mode, nconv, B, np.percentile(r.iterations, [0, 50, 100])))
    # measured: 23 / 32 at order 5 with the time penalty (the rest stop at max_iters or at the rounding floor of J,
    # NOT_CONVERGED), 26..32 / 32 elsewhere
    assert nconv >= (B * 5 // 8 if order == 5 else B * 3 // 4)


@pytest.mark.parametrize("order", [3, 4, 5])
def test_optimiser_ragged_device_f32(csp, order):
    wp, tm, off = _ragged(24, seed=40 + order)
    bc = np.random.default_rng(order).normal(size=(1, 4, 3)) * 0.5
    w = np.random.default_rng(order).uniform(0, 0.3, size=24)
    r = csp.optimize_times_batch(_dev(wp), _dev(tm), _dev(bc), order=order, seg_offsets=_dev(off), min_time=0.1,
                                 vel_zero_weight_per_traj=_dev(w), max_iters=300)
    torch.cuda.synchronize()
    pieces = _split(off, wp, tm)
    T, obj, st = _host(r.times), _host(r.objective), _host(r.status)
    for b, (p, t) in enumerate(pieces):
        tb = T[off[b]:off[b + 1]]
        assert st[b] & ~NOT_CONVERGED == 0 and obj[b, 1] <= obj[b, 0] and tb.min() >= 0.1
        assert abs(tb.sum() - t.sum()) <= 1e-12 * t.sum()
        J, _ = cost_grad(order, p, tb, bc[0], w[b])
        assert abs(J - obj[b, 1]) <= (1e-6 if order == 5 else 1e-8) * J
    assert (st == 0).sum() >= 18
    # fp32 storage, host memory: fp64 arithmetic, the returned times rounded to fp32
    r32 = csp.optimize_times_batch(wp.astype(np.float32), tm.astype(np.float32), bc.astype(np.float32), order=order,
                                   seg_offsets=off, min_time=0.1, vel_zero_weight_per_traj=w, max_iters=300)
    assert r32.times.dtype == np.float32 and r32.coeffs.dtype == np.float32
    for b, (p, t) in enumerate(pieces):
        tb = r32.times[off[b]:off[b + 1]].astype(np.float64)
        assert r32.objective[b, 1] <= r32.objective[b, 0] and tb.min() >= 0.1 * (1 - 1e-7)
        t32 = t.astype(np.float32).astype(np.float64)
        assert abs(tb.sum() - t32.sum()) <= 1e-6 * t32.sum()


def test_coeffs_bit_equal_and_deterministic(csp):
    for order, S in [(4, 16), (3, 7), (5, 40)]:
        wp, tm, bc = _batch_problem(order, 300, S, seed=S)
        d_wp, d_tm, d_bc = _dev(wp), _dev(tm), _dev(bc)
        r1 = csp.optimize_times_batch(d_wp, d_tm, d_bc, order=order, max_iters=50)
        r2 = csp.optimize_times_batch(d_wp, d_tm, d_bc, order=order, max_iters=50)
        torch.cuda.synchronize()
        ref = csp.solve_batch(d_wp, r1.times, d_bc, order=order)
        torch.cuda.synchronize()
        assert torch.equal(r1.coeffs, ref.coeffs), (order, S)
        for a, b in zip((r1.times, r1.coeffs, r1.objective, r1.iterations, r1.status),
                        (r2.times, r2.coeffs, r2.objective, r2.iterations, r2.status)):
            assert torch.equal(a, b)
        # host memory gives the same
        rh = csp.optimize_times_batch(wp, tm, bc, order=order, max_iters=50)
        assert np.array_equal(rh.times, _host(r1.times)) and np.array_equal(rh.coeffs, _host(r1.coeffs))


def test_max_iters_zero_and_one(csp):
    wp, tm, bc = _batch_problem(4, 64, 8, seed=99)
    r0 = csp.optimize_times_batch(wp, tm, bc, order=4, max_iters=0)
    assert np.array_equal(r0.times, tm)
    assert np.all(r0.status == NOT_CONVERGED) and not r0.iterations.any()
    assert np.array_equal(r0.objective[:, 0], r0.objective[:, 1])
    r1 = csp.optimize_times_batch(wp, tm, bc, order=4, max_iters=1)
    assert np.all(r1.status == NOT_CONVERGED) and np.all(r1.iterations == 1)
    assert np.all(r1.objective[:, 1] < r1.objective[:, 0])


def test_empty_batch(csp):
    wp, tm = np.zeros((0, 5, 3)), np.zeros((0, 4))
    assert csp.snap_cost_batch(wp, tm).cost.shape == (0,)
    assert csp.optimize_times_batch(wp, tm).times.shape == (0, 4)
    r = csp.optimize_times_batch(_dev(wp), _dev(tm))
    torch.cuda.synchronize()
    assert r.times.shape == (0, 4)


def test_c3_size(csp):
    """B = 65536, S = 16, order 4 (C3) in both modes; 256 trajectories spread across the batch checked."""
    B, S = 65536, 16
    wp, tm = synth.make_batch(B, S, config_id=3)
    bc = np.zeros((1, 4, 3))
    d_wp, d_tm = _dev(wp), _dev(tm)
    idx = np.linspace(0, B - 1, 256).astype(int)
    for mode, rho in (("fixed_total", 0.0), ("time_penalty", 50.0)):
        r = csp.optimize_times_batch(d_wp, d_tm, order=4, mode=mode, time_weight=rho, min_time=0.1, max_iters=200,
                                     want_coeffs=False)
        c = csp.snap_cost_batch(d_wp, d_tm, order=4)
        torch.cuda.synchronize()
        st = _host(r.status)
        assert not (st & ~NOT_CONVERGED).any()
        assert (st == 0).mean() > 0.9, (st == 0).mean()
        obj = _host(r.objective)
        assert np.all(obj[:, 1] <= obj[:, 0])
        assert np.allclose(obj[:, 0], _host(c.cost) + rho * tm.sum(axis=1), rtol=1e-14, atol=0)
        sub = type("R", (), dict(times=_host(r.times)[idx], objective=obj[idx], iterations=_host(r.iterations)[idx],
                                 status=st[idx]))
        _invariants(4, wp[idx], tm[idx], bc, 0.0, sub, mode, rho, 0.1, 1e-6, check_ref=2)
