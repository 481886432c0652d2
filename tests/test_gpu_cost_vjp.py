"""The reverse mode with a cost cotangent (csp_minsnap_solve_batch_cost_vjp) and solve_batch_autograd's
with_cost on the MI355X: accuracy against the numpy restatement (tests/cost_vjp_ref.py), agreement with the entries
that exist (VJP, cost pass), the torch op, and the memory / isolation contracts with guard-banded buffers.

Gates are per trajectory (tests/vjp_ref.rel_err_rows), per gradient.  GATE_NUMPY of tests/test_gpu_vjp.py is the ceiling:
the same arithmetic with three more products per segment and slot."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import guarded, synth
from tests.cost_vjp_ref import cost_coeff_cotangent, cost_vjp_batch
from tests.test_gpu_timeopt import GATE_G, GATE_VJP
from tests.test_gpu_vjp import GATE_NUMPY
from tests.vjp_ref import adjoint_batch, rel_err_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NONFINITE, NOT_SPD = 1, 2
ORDERS = [2, 3, 4, 5]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return None if t is None else (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t))


def _inputs(order, B, S, seed, per_bc, per_w):
    wp, tm = synth.make_batch(B, S, config_id=3, offset=seed * 97)
    rng = np.random.default_rng(seed)
    bc = rng.normal(size=(B if per_bc else 1, 4, 3))
    w = rng.uniform(0.0, 0.5, size=B) if per_w else 0.2
    pbar = rng.normal(size=(B, S, 3, 2 * order))
    jbar = rng.normal(size=B)
    return wp, tm, bc, w, pbar, jbar


def _run(csp, order, wp, tm, bc, w, pbar, jbar, host=False, seg_offsets=None, want=("waypoints", "times", "bc"), max_segments=None):
    """solve_batch_vjp with numpy inputs, in host or device memory; returns numpy (waypoints, times, bc, status)."""
    cv = (lambda a: a) if host else _dev
    kw = dict(bc=cv(bc), order=order, want_status=True, want=want, grad_cost=cv(jbar), seg_offsets=cv(seg_offsets),
              max_segments=max_segments)
    if np.ndim(w):
        kw["vel_zero_weight_per_traj"] = cv(w)
    else:
        kw["vel_zero_weight"] = w
    r = csp.solve_batch_vjp(cv(wp), cv(tm), cv(pbar), **kw)
    if not host:
        torch.cuda.synchronize()
    return _host(r.waypoints), _host(r.times), _host(r.bc), _host(r.status)


@functools.lru_cache(maxsize=None)
def _uniform_case(order, S):
    """Inputs and both references of one uniform shape, computed once: (inputs, ref cost-only, ref both)."""
    B = 65
    i = ORDERS.index(order) + (1, 2, 3, 5, 16, 17).index(S)
    per_bc, per_w = i % 2 == 1, (i // 2) % 2 == 1
    inp = _inputs(order, B, S, seed=100 * order + S, per_bc=per_bc, per_w=per_w)
    wp, tm, bc, w, pbar, jbar = inp
    rc = cost_vjp_batch(order, wp, tm, bc, None, jbar, w)
    ra = adjoint_batch(order, wp, tm, bc, pbar, w)
    return inp, per_bc, rc, tuple(a + b for a, b in zip(rc, ra))


def _errs(got, ref, per_bc):
    """rel_err_rows of (waypoints, times, bc); a part that was not asked for (None) is skipped."""
    gwp, gt, gbc = got
    rwp, rt, rbc = ref
    B = rbc.shape[0]
    out = {}
    if gwp is not None:
        out["waypoints"] = rel_err_rows(gwp.reshape(B, -1), rwp.reshape(B, -1))
    if gt is not None:
        out["times"] = rel_err_rows(gt, rt)
    if gbc is not None:
        out["bc"] = rel_err_rows(gbc, rbc) if per_bc else rel_err_rows(gbc.reshape(1, -1), rbc.sum(axis=0).reshape(1, -1))
    return out


@pytest.mark.parametrize("S", [1, 2, 3, 5, 16, 17])
@pytest.mark.parametrize("order", ORDERS)
def test_kernel_vs_numpy_uniform(csp, order, S):
    """B = 65 (one full wave and a tail of one lane): the cost-only call and the combined call, in device and in host
    memory, and a subset of the outputs, which is bit-equal to the full call's."""
    (wp, tm, bc, w, pbar, jbar), per_bc, ref_cost, ref_both = _uniform_case(order, S)
    worst = {}
    for name, pb, ref in (("cost-only", None, ref_cost), ("both", pbar, ref_both)):
        full = None
        for host in (False, True):
            gwp, gt, gbc, st = _run(csp, order, wp, tm, bc, w, pb, jbar, host=host)
            assert not st.any(), st
            e = _errs((gwp, gt, gbc), ref, per_bc)
            assert max(e.values()) < GATE_NUMPY[order], (name, host, e)
            worst[name] = max(worst.get(name, 0.0), max(e.values()))
            if full is None:
                full = (gwp, gt, gbc)
            else:   # host staging changes no bit
                assert all(a.tobytes() == b.tobytes() for a, b in zip(full, (gwp, gt, gbc))), (name, "host != device")
        for want in (("times",), ("waypoints", "bc")):
            sub = _run(csp, order, wp, tm, bc, w, pb, jbar, want=want)
            for k, a, b in zip(("waypoints", "times", "bc"), sub[:3], full):
                assert (a is None) == (k not in want)
                assert a is None or a.tobytes() == b.tobytes(), (name, want, k)
    if order == 2:
        assert not full[2][:, 2:].any()   # acceleration rows of grad_bc
    print("order %d S %d: kernel vs numpy, cost-only %.2e, both %.2e" % (order, S, worst["cost-only"], worst["both"]))


@functools.lru_cache(maxsize=None)
def _ragged_case(order):
    rng = np.random.default_rng(order)
    lens = rng.integers(0, 65, size=70)
    lens[:5] = (0, 64, 1, 2, 0)
    lens[-1] = 0                      # an empty trajectory in the tail wave too
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    wps, tms = [], []
    for b, S in enumerate(lens):
        w_, t_ = synth.make_batch(1, max(int(S), 1), config_id=3, offset=b)
        wps.append(w_[0][:int(S) + 1])
        tms.append(t_[0][:int(S)])
    wp, tm = np.concatenate(wps), np.concatenate(tms)
    pbar = rng.normal(size=(int(off[-1]), 3, 2 * order))
    jbar = rng.normal(size=len(lens))
    out = {}
    for per_bc in (False, True):
        bc = rng.normal(size=(len(lens) if per_bc else 1, 4, 3))
        w = rng.uniform(0.0, 0.5, size=len(lens)) if per_bc else 0.1
        rc = cost_vjp_batch(order, wp, tm, bc, None, jbar, w, seg_offsets=off)
        ra = adjoint_batch(order, wp, tm, bc, pbar, w, seg_offsets=off)
        out[per_bc] = (bc, w, rc, tuple(a + b for a, b in zip(rc, ra)))
    return lens, off, wp, tm, pbar, jbar, out


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("order", ORDERS)
def test_kernel_vs_numpy_ragged(csp, order, host):
    """B = 70, S_b from 0 to 64 with empty trajectories (zero gradients, status 0), max_segments above the longest."""
    lens, off, wp, tm, pbar, jbar, cases = _ragged_case(order)
    for per_bc, (bc, w, ref_cost, ref_both) in cases.items():
        for name, pb, ref in (("cost-only", None, ref_cost), ("both", pbar, ref_both)):
            gwp, gt, gbc, st = _run(csp, order, wp, tm, bc, w, pb, jbar, host=host, seg_offsets=off, max_segments=66)
            assert not st.any()
            rwp, rt, rbc = ref
            errs = []
            for b in range(len(lens)):
                s0, s1 = off[b], off[b + 1]
                errs.append(rel_err_rows(gwp[s0 + b:s1 + b + 1].reshape(1, -1), rwp[s0 + b:s1 + b + 1].reshape(1, -1)))
                if s1 > s0:
                    errs.append(rel_err_rows(gt[s0:s1].reshape(1, -1), rt[s0:s1].reshape(1, -1)))
                else:
                    assert not gwp[s0 + b].any() and (not per_bc or not gbc[b].any())
            errs.append(rel_err_rows(gbc.reshape(-1 if per_bc else 1, 12), rbc.reshape(-1, 12) if per_bc else rbc.sum(0).reshape(1, 12)))
            assert max(errs) < GATE_NUMPY[order], (per_bc, name, max(errs))
            print("order %d ragged per_bc=%d %s: kernel vs numpy %.2e" % (order, per_bc, name, max(errs)))


@pytest.mark.parametrize("order", ORDERS)
def test_f32_storage(csp, order):
    B, S = 32, 9
    wp, tm, bc, w, pbar, jbar = _inputs(order, B, S, seed=order, per_bc=True, per_w=True)
    wp, tm, bc, pbar = (a.astype(np.float32) for a in (wp, tm, bc, pbar))
    for pb in (None, pbar):
        r32 = _run(csp, order, wp, tm, bc, w, pb, jbar)
        r64 = _run(csp, order, *(None if a is None else a.astype(np.float64) for a in (wp, tm, bc)), w,
                   None if pb is None else pb.astype(np.float64), jbar)
        assert r32[0].dtype == np.float32 and r32[1].dtype == np.float32 and r32[2].dtype == np.float32
        # fp32 storage, fp64 arithmetic: the gradients differ by their final rounding to fp32 only
        errs = [rel_err_rows(a.reshape(B, -1), b.reshape(B, -1)) for a, b in zip(r32[:3], r64[:3])]
        assert max(errs) < 1e-6, errs
        print("order %d %s: fp32 storage vs fp64 %.2e" % (order, "cost-only" if pb is None else "both", max(errs)))


# ------------------------------------------------------------------------------------------- against the code that exists


def _raw_call(csp, order, B, S, d_wp, d_tm, d_bc, d_pbar, d_jbar, w, per_bc):
    """The new entry through the raw C-ABI (device memory, fp64, uniform), all three outputs."""
    desc = csp.make_desc(order, B, S, csp.DTYPE_F64, 0.0, w, csp.MEM_DEVICE, per_bc)
    need = csp.cost_vjp_workspace_bytes(desc, d_pbar is not None)
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=DEV)
    gwp, gtm, gbc = torch.empty_like(d_wp), torch.empty_like(d_tm), torch.empty_like(d_bc)
    p = lambda t: None if t is None else t.data_ptr()
    rc = csp.raw_lib().csp_minsnap_solve_batch_cost_vjp(
        ctypes.byref(desc), p(d_wp), p(d_tm), p(d_bc), p(d_pbar), p(d_jbar), p(gwp), p(gtm), p(gbc), None, ws.data_ptr(), need,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, csp.strerror(rc))
    torch.cuda.synchronize()
    return gwp, gtm, gbc


@pytest.mark.parametrize("order", ORDERS)
def test_null_grad_cost_is_the_existing_vjp(csp, order):
    B, S = 65, 5
    for per_bc in (False, True):
        wp, tm, bc, _, pbar, _ = _inputs(order, B, S, seed=31 + order, per_bc=per_bc, per_w=False)
        d = [_dev(a) for a in (wp, tm, bc, pbar)]
        got = _raw_call(csp, order, B, S, *d, None, 0.2, per_bc)
        ref = csp.solve_batch_vjp(d[0], d[1], d[3], bc=d[2], order=order, vel_zero_weight=0.2)
        assert torch.equal(got[0], ref.waypoints) and torch.equal(got[1], ref.times) and torch.equal(got[2], ref.bc)
        # and through the binding: without grad_cost nothing changes
        again = csp.solve_batch_vjp(d[0], d[1], d[3], bc=d[2], order=order, vel_zero_weight=0.2, grad_cost=None)
        assert torch.equal(again.waypoints, ref.waypoints) and torch.equal(again.times, ref.times)


@pytest.mark.parametrize("order", ORDERS)
def test_cost_only_times_are_the_cost_pass_gradient(csp, order):
    B, S = 65, 7
    wp, tm, bc, w, _, jbar = _inputs(order, B, S, seed=41 + order, per_bc=True, per_w=True)
    _, gt, _, st = _run(csp, order, wp, tm, bc, w, None, jbar)
    r = csp.snap_cost_batch(_dev(wp), _dev(tm), _dev(bc), order=order, vel_zero_weight_per_traj=_dev(w))
    ref = jbar[:, None] * _host(r.grad_times)
    err = rel_err_rows(gt, ref)
    print("order %d: cost-only grad_times vs J_bar * cost pass %.2e" % (order, err))
    assert not st.any() and err < GATE_G[order], err


@pytest.mark.parametrize("order", ORDERS)
def test_combined_is_vjp_plus_cost_only(csp, order):
    B, S = 65, 6
    for per_bc in (False, True):
        wp, tm, bc, w, pbar, jbar = _inputs(order, B, S, seed=51 + order, per_bc=per_bc, per_w=per_bc)
        both = _run(csp, order, wp, tm, bc, w, pbar, jbar)
        cost = _run(csp, order, wp, tm, bc, w, None, jbar)
        kw = {"vel_zero_weight_per_traj": _dev(w)} if np.ndim(w) else {"vel_zero_weight": w}
        v = csp.solve_batch_vjp(_dev(wp), _dev(tm), _dev(pbar), bc=_dev(bc), order=order, **kw)
        ref = [_host(a) + b for a, b in zip((v.waypoints, v.times, v.bc), cost[:3])]
        errs = [rel_err_rows(a.reshape(B, -1), b.reshape(B, -1)) for a, b in zip(both[:2], ref[:2])]
        errs.append(rel_err_rows(both[2].reshape(-1 if per_bc else 1, 12), ref[2].reshape(-1 if per_bc else 1, 12)))
        print("order %d per_bc=%d: combined vs VJP + cost-only %.2e" % (order, per_bc, max(errs)))
        assert max(errs) < GATE_NUMPY[order], errs
        # grad_cost = 0: the J_bar instantiation of the kernel against the one compiled without the J_bar terms
        zero = _run(csp, order, wp, tm, bc, w, pbar, np.zeros_like(jbar))
        plain = [_host(a) for a in (v.waypoints, v.times, v.bc)]
        errs0 = [rel_err_rows(a.reshape(B, -1), b.reshape(B, -1)) for a, b in zip(zero[:2], plain[:2])]
        errs0.append(rel_err_rows(zero[2].reshape(-1 if per_bc else 1, 12), plain[2].reshape(-1 if per_bc else 1, 12)))
        print("order %d per_bc=%d: combined with grad_cost = 0 vs VJP %.2e" % (order, per_bc, max(errs0)))
        assert max(errs0) < GATE_NUMPY[order], errs0


@pytest.mark.parametrize("order", ORDERS)
def test_cost_only_equals_the_detour_through_the_vjp(csp, order):
    """Today's detour: the existing VJP fed p_bar = 2 J_bar (Q + w V) p, plus J_bar times the explicit T terms."""
    B, S, w = 4, 5, 0.2
    wp, tm, bc, _, _, jbar = _inputs(order, B, S, seed=61 + order, per_bc=True, per_w=False)
    co = csp.solve_batch(wp, tm, bc, order=order, vel_zero_weight=w).coeffs
    pbar, expl = np.zeros_like(co), np.zeros((B, S))
    for b in range(B):
        pb, ex = cost_coeff_cotangent(order, co[b], tm[b], w)
        pbar[b], expl[b] = jbar[b] * pb, jbar[b] * ex
    v = csp.solve_batch_vjp(wp, tm, pbar, bc=bc, order=order, vel_zero_weight=w)
    gwp, gt, gbc, st = _run(csp, order, wp, tm, bc, w, None, jbar)
    errs = [rel_err_rows(gwp.reshape(B, -1), v.waypoints.reshape(B, -1)), rel_err_rows(gbc, v.bc)]
    # the VJP's time gradient and the explicit terms cancel down to the envelope term: the scale is the larger part
    tt = v.times + expl
    den = np.maximum(np.max(np.abs(v.times), axis=1), np.max(np.abs(tt), axis=1))
    errs.append(float(np.max(np.max(np.abs(gt - tt), axis=1) / den)))
    print("order %d: cost-only vs the detour through the VJP %s" % (order, ["%.2e" % e for e in errs]))
    assert not st.any() and max(errs) < GATE_VJP[order], errs


def test_determinism_and_shared_bc_sum(csp):
    order, B, S = 4, 130, 12
    wp, tm, bc, w, pbar, jbar = _inputs(order, B, S, seed=11, per_bc=False, per_w=False)
    for pb in (None, pbar):
        r1, r2 = _run(csp, order, wp, tm, bc, w, pb, jbar), _run(csp, order, wp, tm, bc, w, pb, jbar)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r1, r2))
        rp = _run(csp, order, wp, tm, np.repeat(bc, B, axis=0), w, pb, jbar)
        assert rp[0].tobytes() == r1[0].tobytes() and rp[1].tobytes() == r1[1].tobytes()
        assert np.max(np.abs(r1[2][0] - rp[2].sum(axis=0))) <= 1e-12 * np.max(np.abs(rp[2])) * B


# ------------------------------------------------------------------------------------------------------------- autograd


def test_autograd_forward_and_backward_bit_equal(csp):
    order, B, S = 4, 64, 7
    wp, tm, bc, _, pbar, jbar = _inputs(order, B, S, seed=5, per_bc=False, per_w=False)
    leaves = [_dev(a).requires_grad_(True) for a in (wp, tm, bc)]
    co, cost = csp.solve_batch_autograd(*leaves, order=order, vel_zero_weight=0.1, with_cost=True)
    assert co.grad_fn is not None and cost.grad_fn is not None and cost.shape == (B,) and cost.dtype == torch.float64
    assert torch.equal(co.detach(), csp.solve_batch(_dev(wp), _dev(tm), _dev(bc), order=order, vel_zero_weight=0.1).coeffs)
    assert torch.equal(cost.detach(), csp.snap_cost_batch(_dev(wp), _dev(tm), _dev(bc), order=order, vel_zero_weight=0.1).cost)
    g, gj = _dev(pbar), _dev(jbar)
    ((co * g).sum() + (cost * gj).sum()).backward()
    v = csp.solve_batch_vjp(_dev(wp), _dev(tm), g, bc=_dev(bc), order=order, vel_zero_weight=0.1, grad_cost=gj)
    assert torch.equal(leaves[0].grad, v.waypoints) and torch.equal(leaves[1].grad, v.times)
    assert torch.equal(leaves[2].grad, v.bc.reshape(leaves[2].shape))
    # without with_cost: one output, as before
    out = csp.solve_batch_autograd(_dev(wp), _dev(tm).requires_grad_(True), _dev(bc), order=order, vel_zero_weight=0.1)
    assert torch.is_tensor(out) and torch.equal(out.detach(), co.detach())


def test_autograd_cost_alone_makes_one_cost_only_call(csp, monkeypatch):
    order, B, S = 3, 8, 5
    wp, tm, bc, _, pbar, _ = _inputs(order, B, S, seed=6, per_bc=True, per_w=False)
    seen = []
    orig = csp.solve_batch_vjp

    def spy(*a, **k):
        seen.append((a[2] is None, tuple(k.get("want")), k.get("grad_cost") is not None))
        return orig(*a, **k)
    monkeypatch.setattr(csp, "solve_batch_vjp", spy)
    d_wp, d_tm, d_bc = _dev(wp).requires_grad_(True), _dev(tm).requires_grad_(True), _dev(bc)
    co, cost = csp.solve_batch_autograd(d_wp, d_tm, d_bc, order=order, with_cost=True)
    cost.sum().backward()
    assert seen == [(True, ("waypoints", "times"), True)]
    ref = orig(_dev(wp), _dev(tm), None, bc=d_bc, order=order, grad_cost=torch.ones(B, dtype=torch.float64, device=DEV),
               want=("waypoints", "times"))
    assert ref.bc is None and d_bc.grad is None
    assert torch.equal(d_wp.grad, ref.waypoints) and torch.equal(d_tm.grad, ref.times)
    # the coefficients alone: grad_cost is not passed at all
    del seen[:]
    d_tm2 = _dev(tm).requires_grad_(True)
    co, cost = csp.solve_batch_autograd(_dev(wp), d_tm2, d_bc, order=order, with_cost=True)
    (co * _dev(pbar)).sum().backward()
    assert seen == [(False, ("times",), False)]
    assert torch.equal(d_tm2.grad, orig(_dev(wp), _dev(tm), _dev(pbar), bc=d_bc, order=order, want=("times",)).times)


def test_autograd_gradcheck(csp):
    order, B, S = 3, 2, 4
    wp, tm = synth.make_batch(B, S, config_id=3)
    bc = np.random.default_rng(0).normal(size=(B, 4, 3))
    args = (_dev(wp).requires_grad_(True), _dev(tm).requires_grad_(True), _dev(bc).requires_grad_(True))
    f = lambda a, b, c: csp.solve_batch_autograd(a, b, c, order=order, vel_zero_weight=0.05, with_cost=True)
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_autograd_descent_on_cost(csp):
    """Five plain gradient steps on the interior waypoints and the times lower J for every trajectory.  The step moves no
    time by more than 2 % of the trajectory's shortest time and no waypoint by more than 2 % of its shortest chord."""
    order, B, S = 4, 8, 6
    wp, tm = synth.make_batch(B, S, config_id=3, offset=7)
    p, t = _dev(wp), _dev(tm)
    chord = (p[:, 1:] - p[:, :-1]).norm(dim=2).min(dim=1).values.reshape(B, 1, 1)
    costs = []
    for _ in range(6):
        p, t = p.detach().requires_grad_(True), t.detach().requires_grad_(True)
        _, cost = csp.solve_batch_autograd(p, t, order=order, with_cost=True)
        costs.append(cost.detach().clone())
        cost.sum().backward()
        gp = p.grad.clone()
        gp[:, 0], gp[:, -1] = 0.0, 0.0
        step_t = 0.02 * t.detach().min(dim=1, keepdim=True).values / t.grad.abs().max(dim=1, keepdim=True).values
        step_p = 0.02 * chord / gp.norm(dim=2).max(dim=1).values.reshape(B, 1, 1)
        p, t = p.detach() - step_p * gp, t.detach() - step_t * t.grad
    print("cost, first and after five steps:", costs[0].cpu().numpy(), costs[-1].cpu().numpy())
    assert torch.all(costs[-1] < costs[0])


# ------------------------------------------------------------------------------------------------------ memory and isolation


def _guard_cases():
    """B in {1, 63, 65, 130} x S in {1, 2, 3, 17} with the order rotating over the grid, both variants at every shape
    (fp32 storage and a shared bc alternate), and ragged batches with empty trajectories and max_segments above the
    longest trajectory."""
    out = []
    for bi, B in enumerate((1, 63, 65, 130)):
        for si, S in enumerate((1, 2, 3, 17)):
            order = 2 + (bi + si) % 4
            for pb in (False, True):
                out.append(((S,) * B, True, order, (bi + si + pb) % 3 == 0, 0, pb, (bi + pb) % 2 == 0))
    rag1, rag2 = (1, 2, 0, 17, 1, 5), (17,) * 64 + (0, 1)
    for pb in (False, True):
        out += [(rag1, False, 3, True, 32, pb, True), (rag1, False, 4, False, 17, pb, False), (rag2, False, 5, pb, 32, pb, not pb),
                (rag2, False, 2, False, 20, pb, True)]
    return out


def _gid(c):
    lens, uniform, order, f32, ms, pb, per_bc = c
    shape = "B%dxS%d" % (len(lens), lens[0]) if uniform else "ragged%d_max%d" % (len(lens), ms)
    return "%s-o%d-%s-%s-%s" % (shape, order, "f32" if f32 else "f64", "both" if pb else "costonly", "perbc" if per_bc else "sharedbc")


GUARD_CASES = [pytest.param(c, id=_gid(c)) for c in _guard_cases()]


def _guard_inputs(case, seed):
    lens, uniform, order, f32, ms, pb, per_bc = case
    B = len(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    wps, tms = [], []
    for b, S in enumerate(lens):
        w_, t_ = synth.make_batch(1, max(int(S), 1), config_id=3, offset=seed + b)
        wps.append(w_[0][:int(S) + 1])
        tms.append(t_[0][:int(S)])
    rng = np.random.default_rng(seed)
    fl = np.float32 if f32 else np.float64
    d = dict(waypoints=np.concatenate(wps).astype(fl), times=np.concatenate(tms).astype(fl),
             bc=rng.normal(size=(B if per_bc else 1, 4, 3)).astype(fl), grad_cost=rng.normal(size=B),
             vw=rng.uniform(0.0, 0.3, size=B))
    if pb:
        d["grad_coeffs"] = rng.normal(size=(int(off[-1]), 3, 2 * order)).astype(fl)
    if not uniform:
        d["seg_offsets"] = off
    return d


def _guarded_call(csp, case, host, fill):
    """One device-memory call through the raw C-ABI: the workspace at exactly csp_minsnap_cost_vjp_workspace_bytes, the three
    gradient arrays and the status at exactly their sizes, the inputs in carves too; workspace and outputs start as `fill`
    bytes.  Checks the return code, every guard band and that no input byte changed."""
    lens, uniform, order, f32, ms, pb, per_bc = case
    B = len(lens)
    ins = {k: guarded.carve_from(v, DEV, name=k) for k, v in host.items()}
    elt = 4 if f32 else 8
    total = int(sum(lens))
    outs = {"grad_waypoints": guarded.Guarded((total + B) * 3 * elt, DEV, name="grad_waypoints").fill(fill),
            "grad_times": guarded.Guarded(total * elt, DEV, name="grad_times").fill(fill),
            "grad_bc": guarded.Guarded((B if per_bc else 1) * 12 * elt, DEV, name="grad_bc").fill(fill),
            "status": guarded.Guarded(B * 4, DEV, name="status").fill(fill)}
    desc = csp.make_desc(order, B, lens[0] if uniform else 0, csp.DTYPE_F32 if f32 else csp.DTYPE_F64, 0.0, 0.02, csp.MEM_DEVICE,
                         per_bc, None if uniform else ins["seg_offsets"].data_ptr(), 0 if uniform else ms, ins["vw"].data_ptr())
    need = csp.cost_vjp_workspace_bytes(desc, pb)
    n = order - 1
    assert need == ((max((lens[0] if uniform else ms) - 1, 0) * (n * n + (6 if pb else 3) * n) * B * 8 + 255) // 256 * 256
                    + (0 if per_bc else 12 * ((B + 63) // 64) * 8))
    ws = guarded.Guarded(need, DEV, name="workspace").fill(fill)
    rc = csp.raw_lib().csp_minsnap_solve_batch_cost_vjp(
        ctypes.byref(desc), ins["waypoints"].data_ptr(), ins["times"].data_ptr(), ins["bc"].data_ptr(),
        ins["grad_coeffs"].data_ptr() if pb else None, ins["grad_cost"].data_ptr(), outs["grad_waypoints"].data_ptr(),
        outs["grad_times"].data_ptr(), outs["grad_bc"].data_ptr(), outs["status"].data_ptr(), ws.data_ptr(), need,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (_gid(case), rc, csp.strerror(rc))
    torch.cuda.synchronize()
    for g in [ws] + list(ins.values()) + list(outs.values()):
        g.check()
    for k, g in ins.items():
        assert g.bytes().tobytes() == np.ascontiguousarray(host[k]).tobytes(), (_gid(case), k, "an input changed")
    fl = np.float32 if f32 else np.float64
    return dict(grad_waypoints=outs["grad_waypoints"].numpy(fl), grad_times=outs["grad_times"].numpy(fl),
                grad_bc=outs["grad_bc"].numpy(fl), status=outs["status"].numpy(np.int32))


@pytest.mark.parametrize("case", GUARD_CASES)
def test_guard_bands_and_stale_memory(csp, case):
    """The same call over a 0x00-filled and a 0xFF-filled (NaN / -1) workspace and outputs: every band intact, no input
    byte changed, the outputs bit-equal between the two calls (a shared bc's sum included) with no all-ones element left,
    status 0 everywhere (an empty trajectory included), and the gradients bit-equal with the Python binding's call, so the
    guarded call ran the kernel."""
    lens, uniform, order, f32, ms, pb, per_bc = case
    host = _guard_inputs(case, seed=700 + 13 * len(lens) + sum(lens) + order)
    a, b = _guarded_call(csp, case, host, 0x00), _guarded_call(csp, case, host, 0xFF)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (k, "differs between a 0x00 and a 0xFF start")
        assert not (b[k].reshape(-1, 1).view(np.uint8).reshape(b[k].size, -1).min(axis=1) == 0xFF).any(), (k, "stale 0xFF elements")
    assert not a["status"].any(), a["status"]
    B = len(lens)
    wp = host["waypoints"].reshape((B, lens[0] + 1, 3) if uniform else (-1, 3))
    tm = host["times"].reshape((B, lens[0]) if uniform else (-1,))
    r = csp.solve_batch_vjp(_dev(wp), _dev(tm), _dev(host.get("grad_coeffs")), bc=_dev(host["bc"]), grad_cost=_dev(host["grad_cost"]),
                            order=order, vel_zero_weight=0.02, vel_zero_weight_per_traj=_dev(host["vw"]),
                            seg_offsets=None if uniform else _dev(host["seg_offsets"]), max_segments=None if uniform else ms)
    torch.cuda.synchronize()
    assert _host(r.waypoints).tobytes() == a["grad_waypoints"].tobytes() and _host(r.times).tobytes() == a["grad_times"].tobytes()
    assert _host(r.bc).tobytes() == a["grad_bc"].tobytes()


@pytest.mark.parametrize("pb", [False, True], ids=["costonly", "both"])
@pytest.mark.parametrize("order", ORDERS)
def test_bad_lanes(csp, order, pb):
    """B = 65, S = 5, per-trajectory bc.  Lane 0 has a time of 0.0, lane 31 a negative time, lane 63 an infinite waypoint,
    lane 64 (alone in the tail wave) a NaN time, lane 7 an infinite grad_cost entry; every buffer guarded, workspace and
    outputs 0xFF-filled.  CSP_TRAJ_NOT_SPD for the non-positive times, CSP_TRAJ_NONFINITE for the non-finite inputs, and
    every other lane has status 0 and outputs bit-equal to a run in which the bad lanes hold benign data.  The kernel's
    loops run over k < S and k >= 0 from S - 1 only, with fully unrolled fixed-size inner loops, whatever the data."""
    B, S = 65, 5
    case = ((S,) * B, True, order, order == 3, 0, pb, True)
    good = _guard_inputs(case, seed=4200 + order)
    bad = {k: v.copy() for k, v in good.items()}
    tm, wp = bad["times"].reshape(B, S), bad["waypoints"].reshape(B, S + 1, 3)
    tm[0, 2], tm[31, 2], wp[63, 3, 1], tm[64, 1] = 0.0, -0.3, np.inf, np.nan
    bad["grad_cost"][7] = np.inf
    lanes = [0, 7, 31, 63, 64]
    out_bad, out_good = _guarded_call(csp, case, bad, 0xFF), _guarded_call(csp, case, good, 0xFF)
    st = out_bad["status"]
    print("order %d: status of the bad lanes" % order, {k: int(st[k]) for k in lanes})
    others = np.setdiff1d(np.arange(B), lanes)
    assert not st[others].any() and not out_good["status"].any(), st
    for k in ("grad_waypoints", "grad_times", "grad_bc"):
        rb, rg = out_bad[k].reshape(B, -1), out_good[k].reshape(B, -1)
        assert rb[others].tobytes() == rg[others].tobytes(), (k, "a bad lane disturbed another lane")
    assert st[0] & NOT_SPD and st[31] & NOT_SPD, (st[0], st[31])
    assert st[63] & NONFINITE and st[64] & NONFINITE and st[7] & NONFINITE, (st[63], st[64], st[7])
    assert st[63] == NONFINITE and st[7] == NONFINITE   # the matrix depends on the times alone: its pivots stay positive


def test_error_codes(csp):
    f = csp.raw_lib().csp_minsnap_solve_batch_cost_vjp
    B, S, order = 4, 3, 4
    wp = torch.zeros((B, S + 1, 3), dtype=torch.float64, device=DEV)
    tm = torch.ones((B, S), dtype=torch.float64, device=DEV)
    bc = torch.zeros((1, 4, 3), dtype=torch.float64, device=DEV)
    g = torch.zeros((B, S, 3, 2 * order), dtype=torch.float64, device=DEV)
    gj = torch.ones(B, dtype=torch.float64, device=DEV)
    gw, gt, gb = torch.zeros_like(wp), torch.zeros_like(tm), torch.zeros_like(bc)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()

    def call(d, gco, gcost, a, b_, c, nws=ws.numel()):
        return f(ctypes.byref(d), p(wp), p(tm), p(bc), p(gco), p(gcost), p(a), p(b_), p(c), None, ws.data_ptr(), nws, None)
    for d in (csp.make_desc(order, B, S, path_weight=0.3, mem_space=csp.MEM_DEVICE),
              csp.make_desc(1, B, S, mem_space=csp.MEM_DEVICE), csp.make_desc(6, B, S, mem_space=csp.MEM_DEVICE),
              csp.make_desc(order, B, S, mem_space=csp.MEM_DEVICE, flags=csp.FLAG_SEGMENT_MAJOR),
              csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, mem_space=csp.MEM_DEVICE, flags=csp.FLAG_F32_ARITH)):
        assert call(d, g, gj, gw, gt, gb) == -2 and call(d, None, gj, gw, gt, gb) == -2
    ok = csp.make_desc(order, B, S, mem_space=csp.MEM_DEVICE)
    assert call(ok, None, None, gw, gt, gb) == -1
    assert call(ok, g, gj, None, None, None) == -1
    assert call(ok, None, gj, gw, gt, gb, nws=8) == -3 and call(ok, g, gj, gw, gt, gb, nws=8) == -3
    for gco in (None, g):
        assert call(ok, gco, gj, gw, None, None) == 0 and call(ok, gco, gj, None, gt, None) == 0 and call(ok, gco, gj, None, None, gb) == 0
    torch.cuda.synchronize()


def test_empty_batch_is_noop(csp):
    wp, tm, g, gj = np.zeros((0, 5, 3)), np.zeros((0, 4)), np.zeros((0, 4, 3, 8)), np.zeros(0)
    for pb in (None, g):
        r = csp.solve_batch_vjp(wp, tm, pb, grad_cost=gj, order=4)
        assert r.waypoints.shape == (0, 5, 3) and r.times.shape == (0, 4)
        r = csp.solve_batch_vjp(_dev(wp), _dev(tm), _dev(pb), grad_cost=_dev(gj), order=4)
        assert r.waypoints.shape == (0, 5, 3) and r.times.shape == (0, 4)
