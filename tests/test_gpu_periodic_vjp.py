"""The periodic solve's reverse mode (csp_minsnap_solve_periodic_batch_vjp) and its torch autograd op on the MI355X.

Gates are per trajectory: max-abs error over max-abs reference (tests/vjp_ref.rel_err_rows), for each gradient
separately.  The numpy adjoint (tests/periodic_vjp_ref.py) is a dense fp64 restatement with its own rounding
(tests/test_periodic_vjp_math.py measures it against 30-digit derivatives), so the kernel-vs-numpy gates carry both.
Memory and isolation checks drive the C-ABI through raw pointers with every buffer inside a guarded allocation
(tests/guarded.py); no test here aims at a fault: every loop of the kernel runs over the segments only, whatever the
data, and the guard band (64 KiB) is larger than a whole workspace step of these shapes ((2(o-1)^2 + 6(o-1)) * B * 8 =
56 * 130 * 8 bytes at order 5)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import guarded, synth
from tests import periodic_vjp_ref as R
from tests.vjp_ref import rel_err_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NONFINITE, NOT_SPD = 1, 2
# kernel vs numpy adjoint, per order: the open-chain VJP's gates (tests/test_gpu_vjp.py) as a ceiling.  Measured on the
# MI355X (worst over the uniform grid and the ragged batch; the times dominate): 8.7e-14 / 4.9e-12 / 6.4e-10 / 3.4e-7 at
# orders 2 / 3 / 4 / 5
GATE_NUMPY = {2: 1e-12, 3: 1e-11, 4: 4e-9, 5: 1e-6}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _loops(B, S, seed):
    """B closed loops of S points: (waypoints [B,S,3], times [B,S])."""
    wp, tm = synth.make_batch(B, S, config_id=3, offset=seed * 97)
    return np.ascontiguousarray(wp[:, :S]), tm


def _ragged(lens, seed):
    wps, tms = [], []
    for b, S in enumerate(lens):
        if S:
            w_, t_ = _loops(1, int(S), seed + b)
            wps.append(w_[0])
            tms.append(t_[0])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.concatenate(wps), np.concatenate(tms), off


def _run(csp, order, wp, tm, pbar, jbar, w, host, seg_offsets=None, max_segments=None, want=("waypoints", "times")):
    kw = dict(order=order, want_status=True, want=want, max_segments=max_segments)
    conv = (lambda a: a) if host else _dev
    kw["vel_zero_weight_per_traj" if np.ndim(w) else "vel_zero_weight"] = conv(w) if np.ndim(w) else w
    r = csp.solve_periodic_batch_vjp(conv(wp), conv(tm), conv(pbar), grad_cost=None if jbar is None else conv(jbar),
                                     seg_offsets=None if seg_offsets is None else conv(seg_offsets), **kw)
    if not host:
        torch.cuda.synchronize()
    return (None if r.waypoints is None else _host(r.waypoints), None if r.times is None else _host(r.times), _host(r.status))


def _per_loop_errs(gwp, gt, rwp, rt, off):
    e = np.zeros(2)
    for b in range(len(off) - 1):
        s0, s1 = off[b], off[b + 1]
        if s1 > s0:
            e = np.maximum(e, [rel_err_rows(gwp[s0:s1].reshape(1, -1), rwp[s0:s1].reshape(1, -1)),
                               rel_err_rows(gt[s0:s1].reshape(1, -1), rt[s0:s1].reshape(1, -1))])
    return e


# ------------------------------------------------------------------------------------------- against the numpy adjoint


@pytest.mark.parametrize("S", [1, 2, 3, 5, 16, 17])
@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_kernel_vs_numpy_uniform(csp, order, S):
    """B = 65 (one full wave plus one lane); w in {0, 0.3} and per trajectory, with and without grad_cost, host and
    device memory: twelve calls against six reference batches."""
    B = 65
    wp, tm = _loops(B, S, seed=10 * order + S)
    rng = np.random.default_rng(1000 * order + S)
    pbar, jbar, wper = rng.normal(size=(B, S, 3, 2 * order)), rng.normal(size=B), rng.uniform(0.0, 0.5, size=B)
    worst = np.zeros(2)
    for w in (0.0, 0.3, wper):
        for jb in (None, jbar):
            rwp, rt = R.adjoint_batch(order, wp, tm, pbar, jb, w)
            for host in (False, True):
                gwp, gt, st = _run(csp, order, wp, tm, pbar, jb, w, host)
                assert not st.any(), st
                e = [rel_err_rows(gwp, rwp), rel_err_rows(gt, rt) if S > 1 else float(np.max(np.abs(gt)))]
                worst = np.maximum(worst, e)
                assert max(e) < GATE_NUMPY[order], (np.ndim(w) or w, jb is not None, host, e)
    print("order %d S %d: kernel vs numpy waypoints %.2e times %.2e" % (order, S, worst[0], worst[1]))


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_kernel_vs_numpy_ragged(csp, order, host):
    """B = 70: every length 0..64 once (an empty loop, S = 1 and S = 2 included) and five more, in a shuffled order;
    max_segments larger than the longest loop; per-trajectory w and grad_cost."""
    rng = np.random.default_rng(order)
    lens = rng.permutation(np.concatenate([np.arange(65), [0, 1, 2, 17, 64]]))
    assert len(lens) == 70 and set(range(65)) <= set(lens.tolist())
    wp, tm, off = _ragged(lens, seed=order)
    pbar = rng.normal(size=(int(off[-1]), 3, 2 * order))
    jbar, w = rng.normal(size=70), rng.uniform(0.0, 0.5, size=70)
    gwp, gt, st = _run(csp, order, wp, tm, pbar, jbar, w, host, seg_offsets=off, max_segments=80)
    assert not st.any(), st
    rwp, rt = R.adjoint_batch(order, wp, tm, pbar, jbar, w, seg_offsets=off)
    e = _per_loop_errs(gwp, gt, rwp, rt, off)
    print("order %d ragged host=%d: kernel vs numpy waypoints %.2e times %.2e" % (order, host, e[0], e[1]))
    assert max(e) < GATE_NUMPY[order], e


# ------------------------------------------------------------------- against the recorded 30-digit directional derivatives

# kernel vs 30-digit derivatives of tests/periodic_ref.solve (S in {2, 3}; waypoints / times), 10 x the sum of
#   the two references' measured agreement on these loops (tests/test_periodic_vjp_math.py): waypoints 9.6e-16 / 2.5e-14 /
#   2.5e-12 / 1.4e-8, times 2.3e-12 / 9.3e-13 / 2.7e-11 / 3.0e-8 at orders 2 / 3 / 4 / 5, and
#   the kernel's measured error against the numpy adjoint at S in {2, 3} (test_kernel_vs_numpy_uniform): waypoints
#   7.1e-15 / 6.3e-13 / 3.5e-11 / 3.0e-8, times 8.7e-14 / 4.9e-12 / 2.3e-10 / 1.5e-7.
# Measured kernel vs 30 digits: waypoints 5.3e-16 / 4.2e-15 / 1.2e-12 / 5.1e-10, times 2.3e-12 / 9.3e-13 / 1.5e-12 / 6.0e-10
# (the kernel is closer to the 30-digit derivatives than the numpy adjoint is: the latter's dense inverses of M dominate)
GATE_DIR_WP = {2: 8e-14, 3: 6.6e-12, 4: 3.8e-10, 5: 4.4e-7}
GATE_DIR_T = {2: 2.4e-11, 3: 5.8e-11, 4: 2.6e-9, 5: 1.8e-6}


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_kernel_vs_recorded_directional_derivatives(csp, order):
    cases = [c for c in R.golden_cases() if c["order"] == order and c["S"] in (2, 3)]
    assert len(cases) == 4
    worst = np.zeros(2)
    for c in cases:
        for jb in (0.0, 0.7):
            gwp, gt, st = _run(csp, order, c["path"][None], c["time"][None], c["pbar"][None], None if jb == 0.0 else np.array([jb]),
                               c["w"], host=False)
            assert not st.any()
            fw, ft = c["wp_p"] + jb * c["wp_J"], c["t_p"] + jb * c["t_J"]
            worst = np.maximum(worst, [np.max(np.abs(gwp[0] - fw)) / np.max(np.abs(fw)), np.max(np.abs(gt[0] - ft)) / np.max(np.abs(ft))])
    print("order %d: kernel vs 30-digit derivatives waypoints %.2e times %.2e" % (order, worst[0], worst[1]))
    assert worst[0] < GATE_DIR_WP[order] and worst[1] < GATE_DIR_T[order], worst


# ------------------------------------------------------------------------------------- identities that need no reference


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_translation_and_time_scaling_identities(csp, order):
    """B = 130, S = 5.  sum_k dL/dP_k = sum_j p_bar_j[power 0] per axis; at w = 0,
    sum_j T_j T_bar_j = -sum pow_i p_i p_bar_i + (1-2o) J J_bar with p and J from the unchanged forward.
    Every gradient is within GATE_NUMPY of the exact one relative to its trajectory's largest entry, and the exact ones
    obey the identities, so a sum of S of them misses by at most S x GATE_NUMPY x the largest term (the forward's own
    error, ~1e-13 x its largest term, is below that)."""
    B, S, m = 130, 5, 2 * order
    wp, tm = _loops(B, S, seed=order)
    rng = np.random.default_rng(order)
    pbar, jbar = rng.normal(size=(B, S, 3, m)), rng.normal(size=B)
    gate = S * GATE_NUMPY[order]
    for w in (0.0, 0.3):
        gwp, gt, st = _run(csp, order, wp, tm, pbar, jbar, w, host=False)
        assert not st.any()
        res = np.abs(gwp.sum(axis=1) - pbar[..., m - 1].sum(axis=1)).max(axis=1)
        e_tr = float(np.max(res / np.abs(gwp).reshape(B, -1).max(axis=1)))
        assert e_tr < gate, e_tr
        if w == 0.0:
            f = csp.solve_periodic_batch(_dev(wp), _dev(tm), order=order, want_cost=True)
            co, J = _host(f.coeffs), _host(f.cost)
            t1 = -np.sum(np.arange(m - 1, -1, -1.0) * co * pbar, axis=(1, 2, 3))
            t2 = (1 - m) * J * jbar
            lhs = np.sum(tm * gt, axis=1)
            scale = np.maximum(np.abs(tm * gt).max(axis=1), np.maximum(np.abs(t1), np.abs(t2)))
            e_sc = float(np.max(np.abs(lhs - t1 - t2) / scale))
            assert e_sc < gate, e_sc
            print("order %d: translation %.2e time scaling %.2e" % (order, e_tr, e_sc))


# -------------------------------------------------------------------------------------------- subsets, determinism, fp32


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_want_subsets_and_determinism(csp, order):
    B, S = 130, 7
    wp, tm = _loops(B, S, seed=order + 5)
    rng = np.random.default_rng(order)
    pbar, jbar = rng.normal(size=(B, S, 3, 2 * order)), rng.normal(size=B)
    for jb in (None, jbar):
        full = _run(csp, order, wp, tm, pbar, jb, 0.1, host=False)
        again = _run(csp, order, wp, tm, pbar, jb, 0.1, host=False)
        assert full[0].tobytes() == again[0].tobytes() and full[1].tobytes() == again[1].tobytes()
        only_wp = _run(csp, order, wp, tm, pbar, jb, 0.1, host=False, want=("waypoints",))
        only_t = _run(csp, order, wp, tm, pbar, jb, 0.1, host=False, want=("times",))
        assert only_wp[1] is None and only_t[0] is None
        assert only_wp[0].tobytes() == full[0].tobytes() and only_t[1].tobytes() == full[1].tobytes()
        assert not (full[2].any() or only_wp[2].any() or only_t[2].any())
    with pytest.raises(csp.CspError) as e:
        _run(csp, order, wp, tm, pbar, None, 0.1, host=False, want=())
    assert e.value.code == -1


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_f32_storage(csp, order):
    """fp32 storage, fp64 arithmetic: against fp64 storage of the same (fp32-representable) inputs the gradients differ by
    their final rounding to fp32 only (2^-24 = 6e-8 of an entry; gate 1e-6 as DESIGN.md §11.3)."""
    B, S = 65, 9
    wp, tm = _loops(B, S, seed=order)
    rng = np.random.default_rng(order)
    pbar, jbar, w = rng.normal(size=(B, S, 3, 2 * order)), rng.normal(size=B), rng.uniform(0.0, 0.5, size=B)
    wp, tm, pbar = (a.astype(np.float32) for a in (wp, tm, pbar))
    r32 = csp.solve_periodic_batch_vjp(_dev(wp), _dev(tm), _dev(pbar), grad_cost=_dev(jbar), order=order,
                                       vel_zero_weight_per_traj=_dev(w), want_status=True)
    r64 = csp.solve_periodic_batch_vjp(*(_dev(a.astype(np.float64)) for a in (wp, tm, pbar)), grad_cost=_dev(jbar), order=order,
                                       vel_zero_weight_per_traj=_dev(w))
    assert r32.waypoints.dtype == torch.float32 and r32.times.dtype == torch.float32 and not _host(r32.status).any()
    errs = [rel_err_rows(_host(a).reshape(B, -1), _host(b).reshape(B, -1)) for a, b in ((r32.waypoints, r64.waypoints), (r32.times, r64.times))]
    print("order %d: fp32 storage vs fp64 %.2e" % (order, max(errs)))
    assert max(errs) < 1e-6, errs


# ---------------------------------------------------------------------------------------------------------------- autograd


def test_autograd_forward_bit_equal_and_backward(csp):
    order, B, S = 4, 65, 6
    wp, tm = _loops(B, S, seed=3)
    rng = np.random.default_rng(3)
    pbar, jbar = rng.normal(size=(B, S, 3, 2 * order)), rng.normal(size=B)
    ref = csp.solve_periodic_batch(_dev(wp), _dev(tm), order=order, vel_zero_weight=0.1, want_cost=True)
    d_wp, d_tm = _dev(wp).requires_grad_(True), _dev(tm).requires_grad_(True)
    only = csp.solve_periodic_batch_autograd(d_wp, d_tm, order=order, vel_zero_weight=0.1)
    assert torch.is_tensor(only) and only.grad_fn is not None and torch.equal(only.detach(), ref.coeffs)
    co, cost = csp.solve_periodic_batch_autograd(d_wp, d_tm, order=order, vel_zero_weight=0.1, with_cost=True)
    assert torch.equal(co.detach(), ref.coeffs) and torch.equal(cost.detach(), ref.cost)
    ((co * _dev(pbar)).sum() + (cost * _dev(jbar)).sum()).backward()
    v = csp.solve_periodic_batch_vjp(_dev(wp), _dev(tm), _dev(pbar), grad_cost=_dev(jbar), order=order, vel_zero_weight=0.1)
    assert torch.equal(d_wp.grad, v.waypoints) and torch.equal(d_tm.grad, v.times)


def test_autograd_only_what_is_needed(csp, monkeypatch):
    """One VJP call per backward, for the inputs that require a gradient only, and grad_cost only when the cost received
    a cotangent."""
    order, B, S = 3, 8, 5
    wp, tm = _loops(B, S, seed=4)
    pbar = _dev(np.random.default_rng(4).normal(size=(B, S, 3, 2 * order)))
    seen = []
    orig = csp.solve_periodic_batch_vjp

    def spy(*a, **k):
        seen.append((tuple(k.get("want")), k.get("grad_cost") is not None))
        return orig(*a, **k)
    monkeypatch.setattr(csp, "solve_periodic_batch_vjp", spy)
    d_wp, d_tm = _dev(wp), _dev(tm).requires_grad_(True)
    co, cost = csp.solve_periodic_batch_autograd(d_wp, d_tm, order=order, with_cost=True)
    (co * pbar).sum().backward()
    assert seen == [(("times",), False)]
    assert d_wp.grad is None and torch.equal(d_tm.grad, orig(d_wp, _dev(tm), pbar, order=order, want=("times",)).times)
    d_wp2, d_tm2 = _dev(wp).requires_grad_(True), _dev(tm)
    co, cost = csp.solve_periodic_batch_autograd(d_wp2, d_tm2, order=order, with_cost=True)
    cost.sum().backward()
    assert seen[1:] == [(("waypoints",), True)]
    ref = orig(_dev(wp), d_tm2, torch.zeros_like(pbar), grad_cost=torch.ones(B, dtype=torch.float64, device=DEV), order=order,
               want=("waypoints",))
    assert d_tm2.grad is None and torch.equal(d_wp2.grad, ref.waypoints)
    out = csp.solve_periodic_batch_autograd(_dev(wp), _dev(tm), order=order)
    assert out.grad_fn is None


def test_autograd_gradcheck(csp):
    order, B, S = 3, 2, 4
    wp, tm = _loops(B, S, seed=0)
    args = (_dev(wp).requires_grad_(True), _dev(tm).requires_grad_(True))
    f = lambda a, b: csp.solve_periodic_batch_autograd(a, b, order=order, vel_zero_weight=0.05, with_cost=True)
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_autograd_descent_on_lap_cost(csp):
    """The lap-time use case with torch alone: five steps of plain gradient descent on the snap cost with respect to the
    times, the lap time sum T restored after each step, lower every loop's cost."""
    order, B, S = 4, 8, 6
    wp, tm = _loops(B, S, seed=7)
    d_wp, t = _dev(wp), _dev(tm)
    total = t.sum(dim=1, keepdim=True)
    costs = []
    for _ in range(6):
        t = t.detach().requires_grad_(True)
        _, cost = csp.solve_periodic_batch_autograd(d_wp, t, order=order, with_cost=True)
        costs.append(cost.detach().clone())
        cost.sum().backward()
        g = t.grad
        step = 0.05 * t.detach().min(dim=1, keepdim=True).values / g.abs().max(dim=1, keepdim=True).values   # moves no time by more than 5 % of the shortest
        t = t.detach() - step * g
        t = t * (total / t.sum(dim=1, keepdim=True))
    print("lap cost, first and after five steps:", costs[0].cpu().numpy(), costs[-1].cpu().numpy())
    assert torch.all(costs[-1] < costs[0])
    assert torch.allclose(t.sum(dim=1, keepdim=True), total, rtol=1e-12)


# ------------------------------------------------------------------------------------------------------ memory and isolation


def _guard_cases():
    """B in {1, 63, 65, 130} x S in {1, 2, 3, 17} with the order rotating over the grid (fp32 storage at the odd orders
    in every other row), and ragged batches with an empty loop and max_segments above the longest loop."""
    out = []
    for bi, B in enumerate((1, 63, 65, 130)):
        for si, S in enumerate((1, 2, 3, 17)):
            order = 2 + (bi + si) % 4
            out.append(((S,) * B, True, order, order in (3, 5) and bi % 2 == 0, 0, (bi + si) % 2 == 0))
    rag1, rag2 = (1, 2, 0, 17, 1, 5), (17,) * 64 + (0, 1)
    out += [(rag1, False, 3, True, 32, True), (rag1, False, 4, False, 17, False), (rag2, False, 5, True, 32, False),
            (rag2, False, 2, False, 20, True), (rag2, False, 5, False, 32, True)]
    return out


def _gid(c):
    lens, uniform, order, f32, ms, jb = c
    shape = "B%dxS%d" % (len(lens), lens[0]) if uniform else "ragged%d_max%d" % (len(lens), ms)
    return "%s-o%d-%s-%s" % (shape, order, "f32" if f32 else "f64", "jbar" if jb else "nojbar")


GUARD_CASES = [pytest.param(c, id=_gid(c)) for c in _guard_cases()]


def _guard_inputs(case, seed):
    lens, uniform, order, f32, ms, jb = case
    wp, tm, off = _ragged(lens, seed)
    rng = np.random.default_rng(seed)
    fl = np.float32 if f32 else np.float64
    d = dict(waypoints=wp.astype(fl), times=tm.astype(fl), grad_coeffs=rng.normal(size=(int(off[-1]), 3, 2 * order)).astype(fl),
             vw=rng.uniform(0.0, 0.3, size=len(lens)))
    if jb:
        d["grad_cost"] = rng.normal(size=len(lens))
    if not uniform:
        d["seg_offsets"] = off
    return d


def _guarded_call(csp, case, host, fill):
    """One device-memory call through the raw C-ABI: the workspace at exactly csp_minsnap_periodic_vjp_workspace_bytes,
    both gradient arrays and the status at exactly their sizes, the inputs in carves too; workspace and outputs start as
    `fill` bytes.  Checks the return code, every guard band and that no input byte changed."""
    lens, uniform, order, f32, ms, jb = case
    B = len(lens)
    ins = {k: guarded.carve_from(v, DEV, name=k) for k, v in host.items()}
    elt = 4 if f32 else 8
    total = int(sum(lens))
    outs = {"grad_waypoints": guarded.Guarded(total * 3 * elt, DEV, name="grad_waypoints").fill(fill),
            "grad_times": guarded.Guarded(total * elt, DEV, name="grad_times").fill(fill),
            "status": guarded.Guarded(B * 4, DEV, name="status").fill(fill)}
    desc = csp.make_desc(order, B, lens[0] if uniform else 0, csp.DTYPE_F32 if f32 else csp.DTYPE_F64, 0.0, 0.02, csp.MEM_DEVICE, False,
                         None if uniform else ins["seg_offsets"].data_ptr(), 0 if uniform else ms, ins["vw"].data_ptr())
    need = csp.periodic_vjp_workspace_bytes(desc)
    n = order - 1
    assert need == (max((lens[0] if uniform else ms) - 1, 0) * (2 * n * n + 6 * n) * B * 8 + 255) // 256 * 256
    ws = guarded.Guarded(need, DEV, name="workspace").fill(fill)
    rc = csp.raw_lib().csp_minsnap_solve_periodic_batch_vjp(
        ctypes.byref(desc), ins["waypoints"].data_ptr(), ins["times"].data_ptr(), ins["grad_coeffs"].data_ptr(),
        ins["grad_cost"].data_ptr() if jb else None, outs["grad_waypoints"].data_ptr(), outs["grad_times"].data_ptr(),
        outs["status"].data_ptr(), ws.data_ptr(), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (_gid(case), rc, csp.strerror(rc))
    torch.cuda.synchronize()
    for g in [ws] + list(ins.values()) + list(outs.values()):
        g.check()
    for k, g in ins.items():
        assert g.bytes().tobytes() == np.ascontiguousarray(host[k]).tobytes(), (_gid(case), k, "an input changed")
    fl = np.float32 if f32 else np.float64
    return dict(grad_waypoints=outs["grad_waypoints"].numpy(fl), grad_times=outs["grad_times"].numpy(fl),
                status=outs["status"].numpy(np.int32))


@pytest.mark.parametrize("case", GUARD_CASES)
def test_guard_bands_and_stale_memory(csp, case):
    """The same call over a 0x00-filled and a 0xFF-filled (NaN / -1) workspace and outputs: every band intact, no input
    byte changed, the outputs bit-equal between the two with no all-ones element left, status 0 everywhere (an empty
    loop included), and the gradients bit-equal with the Python binding's call, so the guarded call ran the kernel."""
    lens, uniform, order, f32, ms, jb = case
    host = _guard_inputs(case, seed=700 + 13 * len(lens) + sum(lens) + order)
    a, b = _guarded_call(csp, case, host, 0x00), _guarded_call(csp, case, host, 0xFF)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (k, "differs between a 0x00 and a 0xFF start")
        assert not (b[k].reshape(-1, 1).view(np.uint8).reshape(b[k].size, -1).min(axis=1) == 0xFF).any(), (k, "stale 0xFF elements")
    assert not a["status"].any(), a["status"]
    shape = (len(lens), lens[0]) if uniform else (-1,)
    r = csp.solve_periodic_batch_vjp(_dev(host["waypoints"].reshape(shape + (3,))), _dev(host["times"].reshape(shape)),
                                     _dev(host["grad_coeffs"]), grad_cost=_dev(host["grad_cost"]) if jb else None, order=order,
                                     vel_zero_weight=0.02, vel_zero_weight_per_traj=_dev(host["vw"]),
                                     seg_offsets=None if uniform else _dev(host["seg_offsets"]), max_segments=None if uniform else ms)
    torch.cuda.synchronize()
    assert _host(r.waypoints).tobytes() == a["grad_waypoints"].tobytes() and _host(r.times).tobytes() == a["grad_times"].tobytes()


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_bad_lanes(csp, order):
    """B = 65, S = 5.  Lane 0 has a time of 0.0, lane 31 a negative time, lane 63 an infinite waypoint, lane 64 (alone in
    the tail wave) a NaN time, lane 7 an infinite grad_coeffs entry; every buffer guarded, workspace and outputs 0xFF-
    filled.  CSP_TRAJ_NOT_SPD for the non-positive times, CSP_TRAJ_NONFINITE for the non-finite inputs, and every other
    lane has status 0 and outputs bit-equal to a run in which the bad lanes hold benign data.  The kernel's loops run
    over k < S and k >= 0 from S - 1 only, with fully unrolled fixed-size inner loops, whatever the data."""
    B, S, m = 65, 5, 2 * order
    case = ((S,) * B, True, order, order == 3, 0, True)
    good = _guard_inputs(case, seed=4200 + order)
    bad = {k: v.copy() for k, v in good.items()}
    tm, wp = bad["times"].reshape(B, S), bad["waypoints"].reshape(B, S, 3)
    tm[0, 2], tm[31, 2], wp[63, 3, 1], tm[64, 1] = 0.0, -0.3, np.inf, np.nan
    bad["grad_coeffs"].reshape(B, S, 3, m)[7, 2, 1, 3] = np.inf
    lanes = [0, 7, 31, 63, 64]
    out_bad, out_good = _guarded_call(csp, case, bad, 0xFF), _guarded_call(csp, case, good, 0xFF)
    st = out_bad["status"]
    print("order %d: status of the bad lanes" % order, {k: int(st[k]) for k in lanes})
    others = np.setdiff1d(np.arange(B), lanes)
    assert not st[others].any() and not out_good["status"].any(), st
    for k in ("grad_waypoints", "grad_times"):
        rb, rg = out_bad[k].reshape(B, -1), out_good[k].reshape(B, -1)
        assert rb[others].tobytes() == rg[others].tobytes(), (k, "a bad lane disturbed another lane")
    assert st[0] & NOT_SPD and st[31] & NOT_SPD, (st[0], st[31])
    assert st[63] & NONFINITE and st[64] & NONFINITE and st[7] & NONFINITE, (st[63], st[64], st[7])
    assert st[63] == NONFINITE and st[7] == NONFINITE   # the matrix depends on the times alone: its pivots stay positive


def test_error_codes(csp):
    f = csp.raw_lib().csp_minsnap_solve_periodic_batch_vjp
    B, S, order = 4, 3, 4
    wp = torch.zeros((B, S, 3), dtype=torch.float64, device=DEV)
    tm = torch.ones((B, S), dtype=torch.float64, device=DEV)
    g = torch.zeros((B, S, 3, 2 * order), dtype=torch.float64, device=DEV)
    gw, gt = torch.zeros_like(wp), torch.zeros_like(tm)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    call = lambda d, a, b_: f(ctypes.byref(d), wp.data_ptr(), tm.data_ptr(), g.data_ptr(), None, a, b_, None, ws.data_ptr(), ws.numel(), None)
    for d in (csp.make_desc(order, B, S, path_weight=0.3, mem_space=csp.MEM_DEVICE),
              csp.make_desc(1, B, S, mem_space=csp.MEM_DEVICE), csp.make_desc(6, B, S, mem_space=csp.MEM_DEVICE),
              csp.make_desc(order, B, S, mem_space=csp.MEM_DEVICE, flags=csp.FLAG_SEGMENT_MAJOR),
              csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, mem_space=csp.MEM_DEVICE, flags=csp.FLAG_F32_ARITH)):
        assert call(d, gw.data_ptr(), gt.data_ptr()) == -2
    ok = csp.make_desc(order, B, S, mem_space=csp.MEM_DEVICE)
    assert call(ok, None, None) == -1
    assert f(ctypes.byref(ok), wp.data_ptr(), tm.data_ptr(), g.data_ptr(), None, gw.data_ptr(), None, None, ws.data_ptr(), 8, None) == -3
    assert call(ok, gw.data_ptr(), None) == 0 and call(ok, None, gt.data_ptr()) == 0
    torch.cuda.synchronize()


def test_empty_batch_is_noop(csp):
    wp, tm, g = np.zeros((0, 5, 3)), np.zeros((0, 5)), np.zeros((0, 5, 3, 8))
    r = csp.solve_periodic_batch_vjp(wp, tm, g, order=4)
    assert r.waypoints.shape == (0, 5, 3) and r.times.shape == (0, 5)
    r = csp.solve_periodic_batch_vjp(_dev(wp), _dev(tm), _dev(g), order=4)
    assert r.waypoints.shape == (0, 5, 3) and r.times.shape == (0, 5)
