"""The reverse-mode kernel (csp_minsnap_solve_batch_vjp) and the torch autograd op on the MI355X.

Gates are per trajectory: max-abs error over max-abs reference, for every gradient separately.  The numpy adjoint
(tests/vjp_ref.py) is itself a dense fp64 restatement with its own rounding (tests/test_vjp_math.py measures it
against the 80-bit oracle), so the kernel-vs-numpy gates carry both."""
import numpy as np
import pytest
import torch

from tests import synth
from tests.conftest import load_cases
from tests.vjp_ref import adjoint_batch, oracle_directional, rel_err_rows

pytestmark = pytest.mark.gpu

# kernel vs numpy adjoint, per order.  Measured on the MI355X (worst over uniform, ragged and the C3 sample):
# 2.2e-14 / 6.8e-13 / 4.1e-10 / 2.3e-7 at orders 2 / 3 / 4 / 5
GATE_NUMPY = {2: 1e-12, 3: 1e-11, 4: 4e-9, 5: 1e-6}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _inputs(order, B, S, seed, per_bc, per_w):
    wp, tm = synth.make_batch(B, S, config_id=3, offset=seed * 97)
    rng = np.random.default_rng(seed)
    bc = rng.normal(size=(B if per_bc else 1, 4, 3))
    w = rng.uniform(0.0, 0.5, size=B) if per_w else 0.2
    pbar = rng.normal(size=(B, S, 3, 2 * order))
    return wp, tm, bc, w, pbar


def _run(csp, order, wp, tm, bc, w, pbar, host, seg_offsets=None, want_status=True):
    kw = dict(bc=bc, order=order, want_status=want_status)
    if np.ndim(w):
        kw["vel_zero_weight_per_traj"] = w
    else:
        kw["vel_zero_weight"] = w
    if host:
        r = csp.solve_batch_vjp(wp, tm, pbar, seg_offsets=seg_offsets, **kw)
    else:
        if np.ndim(w):
            kw["vel_zero_weight_per_traj"] = _dev(w)
        kw["bc"] = _dev(bc)
        r = csp.solve_batch_vjp(_dev(wp), _dev(tm), _dev(pbar), seg_offsets=None if seg_offsets is None else _dev(seg_offsets), **kw)
        torch.cuda.synchronize()
    return _host(r.waypoints), _host(r.times), _host(r.bc), _host(r.status)


def _gate_all(order, got, ref, per_bc, tag):
    gwp, gt, gbc = got
    rwp, rt, rbc = ref
    B = rbc.shape[0]
    errs = [rel_err_rows(gwp.reshape(B, -1) if gwp.ndim == 3 else gwp, rwp.reshape(B, -1) if rwp.ndim == 3 else rwp)]
    errs.append(rel_err_rows(gt, rt))
    if per_bc:
        errs.append(rel_err_rows(gbc, rbc))
    else:
        errs.append(rel_err_rows(gbc.reshape(1, -1), rbc.sum(axis=0).reshape(1, -1)))
    assert max(errs) < GATE_NUMPY[order], (tag, errs)
    return errs


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_kernel_vs_numpy_uniform(csp, order):
    i, worst = 0, 0.0
    for S in (1, 2, 3, 7, 16, 17, 40):
        for per_bc in (False, True):
            i += 1
            per_w, host = i % 2 == 0, i % 3 == 0
            B = 6
            wp, tm, bc, w, pbar = _inputs(order, B, S, seed=100 * order + i, per_bc=per_bc, per_w=per_w)
            gwp, gt, gbc, st = _run(csp, order, wp, tm, bc, w, pbar, host)
            assert not st.any(), st
            ref = adjoint_batch(order, wp, tm, bc, pbar, w)
            worst = max(worst, max(_gate_all(order, (gwp, gt, gbc), ref, per_bc, (S, per_bc, per_w, host))))
    print("order %d: kernel vs numpy %.2e" % (order, worst))


@pytest.mark.parametrize("order", [2, 3, 4, 5])
@pytest.mark.parametrize("host", [False, True])
def test_kernel_vs_numpy_ragged(csp, order, host):
    rng = np.random.default_rng(order + 10 * host)
    lens = rng.integers(1, 65, size=20)
    lens[:3] = (1, 64, 2)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    wps, tms = [], []
    for b, S in enumerate(lens):
        w_, t_ = synth.make_batch(1, int(S), config_id=3, offset=b)
        wps.append(w_[0])
        tms.append(t_[0])
    wp, tm = np.concatenate(wps), np.concatenate(tms)
    pbar = rng.normal(size=(int(off[-1]), 3, 2 * order))
    for per_bc in (False, True):
        bc = rng.normal(size=(len(lens) if per_bc else 1, 4, 3))
        w = rng.uniform(0.0, 0.5, size=len(lens)) if per_bc else 0.1
        gwp, gt, gbc, st = _run(csp, order, wp, tm, bc, w, pbar, host, seg_offsets=off)
        assert not st.any()
        rwp, rt, rbc = adjoint_batch(order, wp, tm, bc, pbar, w, seg_offsets=off)
        # per trajectory
        errs = []
        for b in range(len(lens)):
            s0, s1 = off[b], off[b + 1]
            errs.append(rel_err_rows(gwp[s0 + b:s1 + b + 1].reshape(1, -1), rwp[s0 + b:s1 + b + 1].reshape(1, -1)))
            errs.append(rel_err_rows(gt[s0:s1].reshape(1, -1), rt[s0:s1].reshape(1, -1)))
        errs.append(rel_err_rows(gbc.reshape(-1 if per_bc else 1, 12), rbc.reshape(-1, 12) if per_bc else rbc.sum(0).reshape(1, 12)))
        assert max(errs) < GATE_NUMPY[order], (per_bc, max(errs))
        print("order %d ragged per_bc=%d: kernel vs numpy %.2e" % (order, per_bc, max(errs)))


def _oracle_case(csp, oracle_mod, order, path, time, bc, w, seed):
    S = len(time)
    pbar = np.random.default_rng(seed).normal(size=(S, 3, 2 * order))
    fwp, fbc, ft = oracle_directional(oracle_mod, order, path, time, bc, pbar, w)
    r = csp.solve_batch_vjp(_dev(path[None]), _dev(time[None]), _dev(pbar[None]), bc=_dev(bc.reshape(1, 4, 3)), order=order,
                            vel_zero_weight=w)
    torch.cuda.synchronize()
    lin = np.concatenate([_host(r.waypoints).ravel(), _host(r.bc).ravel()])
    fd = np.concatenate([fwp.ravel(), fbc.ravel()])
    e_lin = float(np.max(np.abs(lin - fd)) / np.max(np.abs(fd)))
    e_t = float(np.max(np.abs(_host(r.times)[0] - ft)) / np.max(np.abs(ft)))
    return e_lin, e_t


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_kernel_vs_oracle_directional(csp, oracle_mod, order):
    errs = []
    for S in (1, 2, 5, 9):
        for w in (0.0, 0.3):
            wp, tm = synth.make_batch(1, S, config_id=3, offset=S)
            bc = np.random.default_rng(S).normal(size=(4, 3))
            errs.append(_oracle_case(csp, oracle_mod, order, wp[0], tm[0], bc, w, seed=S))
    e_lin, e_t = np.max(errs, axis=0)
    # measured (waypoints / bc, times): order 2 3e-15, 6e-12; 3 7e-15, 4e-12; 4 2.4e-13, 5.8e-10; 5 1.0e-10, 1.4e-7
    gate = 1e-5 if order == 5 else 1e-7
    assert e_lin < gate and e_t < gate, (e_lin, e_t)
    print("order %d: kernel vs oracle waypoints/bc %.2e times %.2e" % (order, e_lin, e_t))


def test_kernel_vs_oracle_golden(csp, oracle_mod):
    """F3 (well scaled) and F2 (the README flight: T up to 734 s, cond(M) up to 1e20) against the oracle's directional
    derivatives.  Measured: F3 1.5e-10, F2 1.2e-8 (order 4, the longer time scale; times dominate)."""
    out = []
    for fname, gate in (("F3_wellscaled.json", 1e-8), ("F2_readme_uav31.json", 1e-7)):
        for i, c in enumerate(load_cases(fname)):
            if c.get("path_weight", 0.0) > 0.0:
                continue
            e = _oracle_case(csp, oracle_mod, c["order"], c["path"], c["time"], c["bc"], c.get("vel_zero_weight", 0.0), seed=i)
            out.append((fname, i, e))
            assert max(e) < gate, (fname, i, e)
    print(out)


def test_autograd_forward_bit_equal_and_backward(csp):
    order, B, S = 4, 64, 7
    wp, tm, bc, _, pbar = _inputs(order, B, S, seed=5, per_bc=False, per_w=False)
    d_wp = _dev(wp).requires_grad_(True)
    d_tm = _dev(tm).requires_grad_(True)
    d_bc = _dev(bc).requires_grad_(True)
    c = csp.solve_batch_autograd(d_wp, d_tm, d_bc, order=order, vel_zero_weight=0.1)
    ref = csp.solve_batch(_dev(wp), _dev(tm), _dev(bc), order=order, vel_zero_weight=0.1).coeffs
    assert c.grad_fn is not None
    assert torch.equal(c.detach(), ref)
    g = _dev(pbar)
    (c * g).sum().backward()
    v = csp.solve_batch_vjp(_dev(wp), _dev(tm), g, bc=_dev(bc), order=order, vel_zero_weight=0.1)
    assert torch.equal(d_wp.grad, v.waypoints)
    assert torch.equal(d_tm.grad, v.times)
    assert torch.equal(d_bc.grad, v.bc.reshape(d_bc.shape))


def test_autograd_only_requested(csp, monkeypatch):
    order, B, S = 3, 8, 5
    wp, tm, bc, _, pbar = _inputs(order, B, S, seed=6, per_bc=True, per_w=False)
    seen = []
    orig = csp.solve_batch_vjp

    def spy(*a, **k):
        seen.append(tuple(k.get("want")))
        return orig(*a, **k)
    monkeypatch.setattr(csp, "solve_batch_vjp", spy)
    d_tm = _dev(tm).requires_grad_(True)
    d_wp, d_bc = _dev(wp), _dev(bc)
    c = csp.solve_batch_autograd(d_wp, d_tm, d_bc, order=order)
    (c * _dev(pbar)).sum().backward()
    assert seen == [("times",)]
    assert d_wp.grad is None and d_bc.grad is None and d_tm.grad is not None
    ref = orig(d_wp, _dev(tm), _dev(pbar), bc=d_bc, order=order, want=("times",))
    assert ref.waypoints is None and ref.bc is None
    assert torch.equal(d_tm.grad, ref.times)


def test_autograd_gradcheck(csp):
    order, B, S = 3, 2, 4
    wp, tm = synth.make_batch(B, S, config_id=3)
    bc = np.random.default_rng(0).normal(size=(B, 4, 3))
    args = (_dev(wp).requires_grad_(True), _dev(tm).requires_grad_(True), _dev(bc).requires_grad_(True))
    f = lambda a, b, c: csp.solve_batch_autograd(a, b, c, order=order, vel_zero_weight=0.05)
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_autograd_ragged(csp):
    order = 4
    lens = np.array([3, 1, 6])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    wp = np.concatenate([synth.make_batch(1, int(S), 3, offset=b)[0][0] for b, S in enumerate(lens)])
    tm = np.concatenate([synth.make_batch(1, int(S), 3, offset=b)[1][0] for b, S in enumerate(lens)])
    d_wp, d_tm = _dev(wp).requires_grad_(True), _dev(tm).requires_grad_(True)
    c = csp.solve_batch_autograd(d_wp, d_tm, order=order, seg_offsets=_dev(off))
    pbar = np.random.default_rng(1).normal(size=c.shape)
    (c * _dev(pbar)).sum().backward()
    rwp, rt, _ = adjoint_batch(order, wp, tm, np.zeros((1, 4, 3)), pbar, 0.0, seg_offsets=off)
    assert rel_err_rows(_host(d_wp.grad).reshape(1, -1), rwp.reshape(1, -1)) < GATE_NUMPY[order]
    assert rel_err_rows(_host(d_tm.grad).reshape(1, -1), rt.reshape(1, -1)) < GATE_NUMPY[order]


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_f32_storage(csp, order):
    B, S = 32, 9
    wp, tm, bc, w, pbar = _inputs(order, B, S, seed=order, per_bc=True, per_w=True)
    wp, tm, bc, pbar = (a.astype(np.float32) for a in (wp, tm, bc, pbar))
    r32 = csp.solve_batch_vjp(_dev(wp), _dev(tm), _dev(pbar), bc=_dev(bc), order=order, vel_zero_weight_per_traj=_dev(w))
    r64 = csp.solve_batch_vjp(*(_dev(a.astype(np.float64)) for a in (wp, tm, pbar)), bc=_dev(bc.astype(np.float64)), order=order,
                              vel_zero_weight_per_traj=_dev(w))
    assert r32.waypoints.dtype == torch.float32
    # fp32 storage, fp64 arithmetic: the gradients differ by their final rounding to fp32 only (measured 5.8e-8)
    errs = [rel_err_rows(_host(a).reshape(B, -1), _host(b).reshape(B, -1))
            for a, b in ((r32.waypoints, r64.waypoints), (r32.times, r64.times), (r32.bc, r64.bc))]
    assert max(errs) < 1e-6, errs
    print("order %d: fp32 storage vs fp64 %.2e" % (order, max(errs)))


def test_determinism_and_shared_bc_sum(csp):
    order, B, S = 4, 1000, 12
    wp, tm, bc, w, pbar = _inputs(order, B, S, seed=11, per_bc=False, per_w=False)
    args = (_dev(wp), _dev(tm), _dev(pbar))
    r1 = csp.solve_batch_vjp(*args, bc=_dev(bc), order=order, vel_zero_weight=w)
    r2 = csp.solve_batch_vjp(*args, bc=_dev(bc), order=order, vel_zero_weight=w)
    for a, b in ((r1.waypoints, r2.waypoints), (r1.times, r2.times), (r1.bc, r2.bc)):
        assert torch.equal(a, b)
    rp = csp.solve_batch_vjp(*args, bc=_dev(np.repeat(bc, B, axis=0)), order=order, vel_zero_weight=w)
    assert torch.equal(rp.waypoints, r1.waypoints) and torch.equal(rp.times, r1.times)
    s = _host(rp.bc).sum(axis=0)
    assert np.max(np.abs(_host(r1.bc)[0] - s)) <= 1e-12 * np.max(np.abs(_host(rp.bc))) * B


def test_large_batch_c3_sample(csp):
    order, B, S = 4, 65536, 16
    wp, tm = synth.make_batch(B, S, config_id=3)
    rng = np.random.default_rng(3)
    bc = rng.normal(size=(1, 4, 3))
    d_pbar = torch.randn((B, S, 3, 2 * order), dtype=torch.float64, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(7))
    r = csp.solve_batch_vjp(_dev(wp), _dev(tm), d_pbar, bc=_dev(bc), order=order, want_status=True)
    torch.cuda.synchronize()
    assert not _host(r.status).any()
    idx = np.linspace(0, B - 1, 256).astype(np.int64)
    pbar = _host(d_pbar)[idx]
    rwp, rt, rbc = adjoint_batch(order, wp[idx], tm[idx], bc, pbar)
    e = (rel_err_rows(_host(r.waypoints)[idx].reshape(256, -1), rwp.reshape(256, -1)), rel_err_rows(_host(r.times)[idx], rt))
    assert max(e) < GATE_NUMPY[order], e
    print("C3 sample: kernel vs numpy %.2e" % max(e))
    assert np.all(np.isfinite(_host(r.bc)))


def test_empty_batch_is_noop(csp):
    wp = torch.zeros((0, 5, 3), dtype=torch.float64, device="cuda:0")
    tm = torch.zeros((0, 4), dtype=torch.float64, device="cuda:0")
    g = torch.zeros((0, 4, 3, 8), dtype=torch.float64, device="cuda:0")
    r = csp.solve_batch_vjp(wp, tm, g, order=4)
    assert r.waypoints.shape == (0, 5, 3) and r.times.shape == (0, 4)
    wpn, tmn, gn = np.zeros((0, 5, 3)), np.zeros((0, 4)), np.zeros((0, 4, 3, 8))
    r = csp.solve_batch_vjp(wpn, tmn, gn, order=4)
    assert r.waypoints.shape == (0, 5, 3)


def test_unsupported_codes(csp):
    import ctypes
    f = csp.raw_lib().csp_minsnap_solve_batch_vjp
    B, S, order = 4, 3, 4
    wp = torch.zeros((B, S + 1, 3), dtype=torch.float64, device="cuda:0")
    tm = torch.ones((B, S), dtype=torch.float64, device="cuda:0")
    bc = torch.zeros((1, 4, 3), dtype=torch.float64, device="cuda:0")
    g = torch.zeros((B, S, 3, 2 * order), dtype=torch.float64, device="cuda:0")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
    for desc in (csp.make_desc(order, B, S, path_weight=0.3, mem_space=csp.MEM_DEVICE),
                 csp.make_desc(order, B, S, mem_space=csp.MEM_DEVICE, flags=csp.FLAG_SEGMENT_MAJOR),
                 csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, mem_space=csp.MEM_DEVICE, flags=csp.FLAG_F32_ARITH)):
        rc = f(ctypes.byref(desc), wp.data_ptr(), tm.data_ptr(), bc.data_ptr(), g.data_ptr(), None, None, None, None,
               ws.data_ptr(), ws.numel(), None)
        with pytest.raises(csp.CspError) as e:
            csp._check(rc)
        assert e.value.code == -2
