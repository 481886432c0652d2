"""Memory and robustness contracts of the entries that keep their factors in a caller-supplied workspace
(csp_minsnap_solve_batch on its generic and span paths, _solve_batch_vjp, _cost_batch, _optimize_times_batch,
_solve_periodic_batch, _solve_mixed), driven through raw pointers with every buffer inside a guarded allocation
(tests/guarded.py):

A. guard bands      -- workspace carved at exactly *_workspace_bytes(desc), every output at exactly its documented size,
                       inputs in carves too: no byte outside is written, no input byte changes;
B. stale memory     -- the same call over a 0x00-filled and over a 0xFF-filled (NaN / -1) workspace and outputs gives the
                       same bits, no 0xFF pattern survives where the header says "written", and it survives where the
                       header says "left untouched";
C. bad lanes        -- non-positive times, inf / NaN inputs in single lanes of the VJP, cost and optimiser kernels: the
                       documented status bits, and the other lanes of the wave bit-equal to a run with benign data;
D. optimiser edges  -- infeasible fixed total, start below the bound, bound active at the solution, S = 1.

Almost every assertion is exact (bit equality, byte patterns); the value checks of part D use the gates of
tests/test_gpu_timeopt.py.  No test here aims at a fault: the guard band (64 KiB) is larger than the largest whole
workspace step of these shapes ((o-1)^2 + 6(o-1)) * B * 8 = 40 * 130 * 8 bytes at order 5), and every loop of the
kernels that get non-finite data is bounded by S, max_iters or kMaxBacktrack whatever the data (see test_bad_lanes).
"""
import collections
import ctypes

import numpy as np
import pytest
import torch

from tests import guarded
from tests.staged import (WORKSPACE_ENTRIES, Carved, arg_pointers, carve_args, check_carves, mixed_block_elements, mixed_buffers,
                          staged_buffers)
from tests.timeopt_ref import NOT_CONVERGED, cost_grad, optimize

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VW = 0.02                       # the descriptor's vel_zero_weight of every call here
NONFINITE, NOT_SPD, SKIPPED = 1, 2, 4
GATE_J = {2: 1e-13, 3: 1e-13, 4: 1e-11, 5: 1e-9}     # tests/test_gpu_timeopt.py: kernel J against tests/timeopt_ref.py

# lens: segments per trajectory; uniform: num_segments = lens[0] (else ragged with max_segments); opt: the optional
# outputs are passed; orders: per trajectory (the mixed entry only)
Case = collections.namedtuple("Case", "lens uniform order f32 bc_per opt max_segments orders")
R1, R2 = (1, 2, 17, 1, 5), (17,) * 64 + (1,)


def _case_id(c):
    shape = "B%dxS%d" % (len(c.lens), c.lens[0]) if c.uniform else "ragged%d_max%d" % (len(c.lens), c.max_segments)
    return "%s-o%s-%s-%s-%s" % (shape, "mix" if c.orders is not None else c.order, "f32" if c.f32 else "f64",
                                "bcper" if c.bc_per else "bcshared", "opt" if c.opt else "noopt")


def _uniform_cases():
    """B in {1, 63, 65, 130} x S in {1, 2, 3, 17}; order, storage type, bc form and optional outputs rotate over the
    grid so that every value of every axis occurs (fp32 storage at orders 3 and 5, among them odd order x odd S)."""
    out = []
    for bi, B in enumerate((1, 63, 65, 130)):
        for si, S in enumerate((1, 2, 3, 17)):
            order = 2 + (bi + si) % 4
            out.append(Case((S,) * B, True, order, order in (3, 5) and bi % 2 == 0, si % 2 == 0, (bi + si // 2) % 2 == 0, 0, None))
    return out


def _ragged_cases():
    """Lengths (1, 2, 17, 1, 5) and 64 x 17 + one of 1 (a tail wave of one short lane), max_segments the true maximum
    and 32: the workspace is sized by max_segments, not by the data."""
    return [Case(R1, False, 3, True, True, True, 17, None), Case(R1, False, 4, False, False, False, 32, None),
            Case(R2, False, 5, False, True, False, 17, None), Case(R2, False, 2, False, False, True, 32, None),
            Case(R2, False, 5, True, False, True, 32, None)]


def _mixed_cases():
    """Orders 2..5 in rotation over the ragged lengths plus one 65-segment trajectory (the chunked family; skipped
    when max_segments = 32)."""
    out = []
    for lens, ms, f32, bc_per, opt in ((R1 + (65,), 65, False, True, True), (R1 + (65,), 32, True, False, True),
                                       (R2 + (65,), 65, True, True, False), (R2 + (65,), 32, False, False, False)):
        out.append(Case(lens, False, 0, f32, bc_per, opt, ms, tuple(2 + i % 4 for i in range(len(lens)))))
    return out


def _cases(entry):
    if entry == "solve_mixed":
        return _mixed_cases()
    extra = []
    if entry == "solve_batch_span":       # the span kernel's own range: more than 256 segments
        extra = [Case((257,) * 65, True, 4, False, True, True, 0, None)]
    if entry == "solve_periodic_batch":   # an empty loop between others: cost 0, status 0, nothing else written
        extra = [Case((1, 2, 0, 17, 1, 5), False, 3, True, False, True, 17, None)]
    return _uniform_cases() + _ragged_cases() + extra


ALL = [pytest.param(e, c, id="%s-%s" % (e, _case_id(c))) for e in sorted(WORKSPACE_ENTRIES) for c in _cases(e)]


def _host_buffers(entry, case, seed):
    if entry == "solve_mixed":
        return mixed_buffers(case.lens, case.orders, case.f32, case.bc_per, seed)
    return staged_buffers(entry, case.lens, case.order, case.f32, case.bc_per, seed)


def _weights(entry, case, seed):
    """Per-trajectory velocity-zero weights go with per-trajectory bc (the mixed binding takes none)."""
    if entry == "solve_mixed" or not case.bc_per:
        return None
    return np.random.default_rng(seed + 1).uniform(0.0, 0.3, size=len(case.lens))


def _offsets(case):
    return np.concatenate([[0], np.cumsum(case.lens)]).astype(np.int64)


def _timeopt_params(csp, **kw):
    d = dict(mode=csp.TIMEOPT_FIXED_TOTAL, min_time=0.01, tol=1e-6, max_iters=5)
    d.update(kw)
    return csp.make_timeopt_params(**d)


def _call(csp, entry, case, host, fill, vw=None, prm=None):
    """One device-memory call of `entry` with the workspace at exactly its documented size and every pointer argument
    in a carve of exactly its size; workspace and outputs start as `fill` bytes.  Checks the return code, every guard
    band and that no input byte changed; returns ({output name: numpy array}, workspace bytes)."""
    sym, ws_fn, args, flag = WORKSPACE_ENTRIES[entry]
    lib = csp.raw_lib()
    B, ragged = len(case.lens), not case.uniform
    tag = (entry, _case_id(case), hex(fill))
    ins, outs = carve_args(args, host, case.opt, fill, DEV)
    extra = {}
    if ragged:
        extra["seg_offsets"] = Carved(_offsets(case), DEV, "seg_offsets")
    if vw is not None:
        extra["vel_zero_weight_per_traj"] = Carved(vw, DEV, "vel_zero_weight_per_traj")
    desc = csp.make_desc(case.order, B, 0 if ragged else case.lens[0], csp.DTYPE_F32 if case.f32 else csp.DTYPE_F64, 0.0, VW,
                         csp.MEM_DEVICE, case.bc_per, extra["seg_offsets"].data_ptr() if ragged else None,
                         case.max_segments if ragged else 0,
                         extra["vel_zero_weight_per_traj"].data_ptr() if vw is not None else None,
                         flags=getattr(csp, flag) if flag else 0)
    need = int(getattr(lib, ws_fn)(ctypes.byref(desc)))
    ws = guarded.Guarded(need, DEV, name="workspace").fill(fill)
    call = [ctypes.byref(desc)] + ([ctypes.byref(prm if prm is not None else _timeopt_params(csp))]
                                   if entry == "optimize_times_batch" else [])
    call += arg_pointers(args, ins, outs)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = getattr(lib, sym)(*call, ws.data_ptr(), need, stream)
    assert rc == 0, (tag, rc, csp.strerror(rc))
    torch.cuda.synchronize()
    # every band intact; no byte of the inputs, the offsets or the weights changed
    check_carves((tag, "workspace %d bytes" % need), [ws] + list(ins.values()) + list(outs.values()) + list(extra.values()),
                 list(ins.values()) + list(extra.values()))
    return {n: g.numpy() for n, g in outs.items()}, need


def _expected_status(entry, case):
    st = np.zeros(len(case.lens), np.int32)
    if entry == "solve_mixed":
        st[np.asarray(case.lens) > case.max_segments] = SKIPPED
    return st


def _check_status(csp, entry, case, out, tag):
    if "status" not in out:
        return
    st = out["status"] & ~NOT_CONVERGED if entry == "optimize_times_batch" else out["status"]
    assert np.array_equal(st, _expected_status(entry, case)), (tag, out["status"])


def _binding_output(csp, entry, case, host, vw, fill):
    """(name, bytes) of one output of the Python binding's call for the same inputs."""
    B, ragged = len(case.lens), not case.uniform
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    S = case.lens[0]
    n_wp = S if entry == "solve_periodic_batch" else S + 1
    wp = dev(host["waypoints"] if ragged else host["waypoints"].reshape(B, n_wp, 3))
    tm = dev(host["times"] if ragged else host["times"].reshape(B, S))
    kw = dict(vel_zero_weight=VW)
    if ragged:
        kw.update(seg_offsets=dev(_offsets(case)), max_segments=case.max_segments)
    if entry == "solve_mixed":
        p = csp.PreparedMixed(dev(host["orders"]), wp, tm, kw["seg_offsets"], dev(host["bc"]), VW, case.max_segments)
        p.out.view(torch.uint8).fill_(fill)
        p.run()
        torch.cuda.synchronize()
        return "coeffs", p.out[:host["coeffs"].size].cpu().numpy().tobytes()
    if vw is not None:
        kw["vel_zero_weight_per_traj"] = dev(vw)
    if entry != "solve_periodic_batch":
        kw["bc"] = dev(host["bc"])
    if entry in ("solve_batch_generic", "solve_batch_span"):
        bc = kw.pop("bc")
        r = csp.solve_batch(wp, tm, bc, order=case.order, force_generic=entry.endswith("generic"), span=entry.endswith("span"), **kw)
        if entry.endswith("generic"):
            assert r.kernel.startswith("generic_o%d" % case.order), r.kernel
        elif max(case.max_segments, max(case.lens)) > 16:
            assert r.kernel.startswith("span_o%d" % case.order), r.kernel
        name, t = "coeffs", r.coeffs
    elif entry == "solve_batch_vjp":
        name, t = "grad_times", csp.solve_batch_vjp(wp, tm, dev(host["grad_coeffs"]), order=case.order, want=("times",), **kw).times
    elif entry == "cost_batch":
        name, t = "cost", csp.snap_cost_batch(wp, tm, order=case.order, want_grad=False, **kw).cost
    elif entry == "optimize_times_batch":
        name, t = "times_out", csp.optimize_times_batch(wp, tm, order=case.order, min_time=0.01, tol=1e-6, max_iters=5,
                                                        want_coeffs=False, **kw).times
    else:
        name, t = "coeffs", csp.solve_periodic_batch(wp, tm, order=case.order, **kw).coeffs
    torch.cuda.synchronize()
    return name, t.cpu().numpy().tobytes()


def _seed(entry, case):
    return 9000 + 31 * sorted(WORKSPACE_ENTRIES).index(entry) + 7 * len(case.lens) + sum(case.lens) + case.order


# ------------------------------------------------------------------------------------------------------ A. guard bands


@pytest.mark.parametrize("entry,case", ALL)
def test_guard_bands(csp, entry, case):
    """One call with the workspace carved at exactly *_workspace_bytes(desc) and every output at exactly its documented
    size (0xA5 bands around each, the inputs included): no band byte changes, no input byte changes, the status is 0
    (NOT_CONVERGED allowed for the optimiser, SKIPPED expected for the mixed entry's over-long trajectory), and one
    output is bit-equal with the Python binding's call for the same inputs, so the guarded call ran the kernel."""
    seed = _seed(entry, case)
    host, vw = _host_buffers(entry, case, seed), _weights(entry, case, seed)
    out, need = _call(csp, entry, case, host, 0x5A, vw)
    tag = (entry, _case_id(case), need)
    _check_status(csp, entry, case, out, tag)
    if entry == "solve_mixed" and "coeff_offsets" in out:
        want = np.concatenate([[0], np.cumsum(mixed_block_elements(case.orders, case.lens, case.f32))])
        assert np.array_equal(out["coeff_offsets"], want), tag
    name, ref = _binding_output(csp, entry, case, host, vw, 0x5A)
    if name in out:     # the VJP without its optional outputs writes nothing that could be compared
        assert out[name].tobytes() == ref, (tag, name)
    else:
        assert entry == "solve_batch_vjp" and not case.opt, tag


# ----------------------------------------------------------------------------------------------------- B. stale memory


def _untouched(entry, case, name, arr):
    """Byte mask of `arr` (output `name`) the header says the call leaves untouched."""
    mask = np.zeros(arr.nbytes, bool)
    if entry == "solve_mixed" and name == "coeffs":
        elt = arr.itemsize
        blocks = mixed_block_elements(case.orders, case.lens, case.f32)
        off = np.concatenate([[0], np.cumsum(blocks)])
        for b, (n, o) in enumerate(zip(case.lens, case.orders)):
            used = 0 if n > case.max_segments else 6 * o * n     # CSP_TRAJ_SKIPPED: the whole block; else the padding
            mask[(off[b] + used) * elt:off[b + 1] * elt] = True
    return mask


@pytest.mark.parametrize("entry,case", ALL)
def test_independent_of_stale_memory(csp, entry, case):
    """The same call twice, workspace and outputs first 0x00-filled, then 0xFF-filled (NaN for fp32 / fp64, -1 for
    int32): every output the header says is written is bit-equal between the two and holds no all-ones element (every
    trajectory here has status 0 or is skipped); what the header says is left untouched -- the mixed entry's
    CSP_TRAJ_SKIPPED block and the two fp32 elements of padding after a block of odd order and odd segment count -- still
    holds the fill.  A periodic trajectory of no segments gets cost 0 and status 0."""
    seed = _seed(entry, case)
    host, vw = _host_buffers(entry, case, seed), _weights(entry, case, seed)
    runs = [_call(csp, entry, case, host, fill, vw)[0] for fill in (0x00, 0xFF)]
    tag = (entry, _case_id(case))
    saw_untouched = False
    for name in runs[0]:
        a, b = runs[0][name], runs[1][name]
        mask = _untouched(entry, case, name, a)
        saw_untouched |= bool(mask.any())
        ab, bb = a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)
        assert np.array_equal(ab[~mask], bb[~mask]), (tag, name, "differs between a 0x00 and a 0xFF start")
        assert (ab[mask] == 0x00).all() and (bb[mask] == 0xFF).all(), (tag, name, "untouched bytes were written")
        elem_mask = mask.reshape(-1, a.itemsize).all(axis=1)
        ones = bb.reshape(-1, a.itemsize).min(axis=1) == 0xFF
        assert not (ones & ~elem_mask).any(), (tag, name, "stale 0xFF elements", np.flatnonzero(ones & ~elem_mask)[:8])
    _check_status(csp, entry, case, runs[1], tag)
    if entry == "solve_mixed" and (case.f32 or min(case.lens) <= case.max_segments < max(case.lens)):
        assert saw_untouched, tag
    if entry == "solve_periodic_batch" and 0 in case.lens and case.opt:
        k = case.lens.index(0)
        assert runs[1]["cost"][k] == 0.0 and runs[1]["status"][k] == 0, tag


# --------------------------------------------------------------------------------------------------------- C. bad lanes


def _rows(out, B):
    return {n: a.reshape(B, -1).view(np.uint8).reshape(B, -1) for n, a in out.items()}


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("entry", ["solve_batch_vjp", "cost_batch", "optimize_times_batch"])
def test_bad_lanes(csp, entry, order):
    """B = 65, S = 5, per-trajectory bc (grad_bc has no cross-lane sum).  Lane 0 has a time of 0.0, lane 31 a negative
    time, lane 63 an infinite waypoint, lane 64 (alone in the tail wave) a NaN time, and for the VJP lane 7 an infinite
    grad_coeffs entry.  Every buffer is guarded, workspace and outputs start 0xFF-filled.

    Loop bounds (read in the kernels): minsnap_vjp_kernel and cost_pass loop over k < S and k >= 0 from S - 1 only, with
    fully unrolled fixed-size inner loops; proj_theta makes at most S + 1 passes of S; the optimiser's while loop ends a
    pass by breaking, by ++backtracks (break above kMaxBacktrack = 30; a comparison with NaN counts as a failed Armijo
    test) or by ++iters (break at max_iters), so it makes at most (max_iters + 1) * (kMaxBacktrack + 1) passes whatever
    the data.

    VJP and cost kernel: CSP_TRAJ_NOT_SPD for the non-positive times, CSP_TRAJ_NONFINITE for the non-finite inputs.
    Optimiser (include/csp_minsnap.h): a time below min_time -- zero and negative ones included -- is not an error, the
    start is projected onto the feasible set, so lanes 0 and 31 are ordinary trajectories whose results keep the sum
    and the bound; lanes 63 and 64 get CSP_TRAJ_NONFINITE, 0 iterations and their input times back, bit for bit.
    Every other lane has status 0 (the optimiser: at most NOT_CONVERGED) and every output bit-equal to a second run in
    which the bad lanes hold benign data."""
    B, S, m = 65, 5, 2 * order
    case = Case((S,) * B, True, order, False, True, True, 0, None)
    good = staged_buffers(entry, case.lens, order, False, True, 4200 + order)
    vw = np.random.default_rng(order).uniform(0.0, 0.3, size=B)
    bad = {k: v.copy() for k, v in good.items()}
    tm, wp = bad["times"].reshape(B, S), bad["waypoints"].reshape(B, S + 1, 3)
    tm[0, 2], tm[31, 2], wp[63, 3, 1], tm[64, 1] = 0.0, -0.3, np.inf, np.nan
    lanes = [0, 31, 63, 64]
    if entry == "solve_batch_vjp":
        bad["grad_coeffs"].reshape(B, S, 3, m)[7, 2, 1, 3] = np.inf
        lanes.append(7)
    prm = _timeopt_params(csp, max_iters=20)
    out_bad, _ = _call(csp, entry, case, bad, 0xFF, vw, prm)
    out_good, _ = _call(csp, entry, case, good, 0xFF, vw, prm)
    st, tag = out_bad["status"], (entry, order)
    print(tag, "status of the bad lanes", {k: int(st[k]) for k in lanes})
    others = np.setdiff1d(np.arange(B), lanes)
    allowed = NOT_CONVERGED if entry == "optimize_times_batch" else 0
    assert not (st[others] & ~allowed).any() and not (out_good["status"] & ~allowed).any(), (tag, st)
    rb, rg = _rows(out_bad, B), _rows(out_good, B)
    for n in rb:
        assert np.array_equal(rb[n][others], rg[n][others]), (tag, n, "a bad lane disturbed another lane")
    if entry != "optimize_times_batch":
        assert st[0] & NOT_SPD and st[31] & NOT_SPD, (tag, st[0], st[31])
        assert st[63] & NONFINITE and st[64] & NONFINITE, (tag, st[63], st[64])
        if entry == "solve_batch_vjp":
            assert st[7] & NONFINITE, (tag, st[7])
        return
    tin, tout, obj, its = bad["times"].reshape(B, S), out_bad["times_out"].reshape(B, S), out_bad["objective"], out_bad["iterations"]
    for k in (0, 31):   # projected start, then an ordinary optimisation
        assert not st[k] & (NOT_SPD | NONFINITE), (tag, k, st[k])
        assert tout[k].min() >= prm.min_time and abs(tout[k].sum() - tin[k].sum()) <= 1e-12 * tin[k].sum(), (tag, k, tout[k])
        assert obj[k, 1] <= obj[k, 0], (tag, k, obj[k])
    for k in (63, 64):  # nothing can be evaluated: the trajectory stops at its start
        assert st[k] & NONFINITE and its[k] == 0, (tag, k, st[k], its[k])
        assert tout[k].tobytes() == tin[k].tobytes(), (tag, k, tout[k])
    assert np.isnan(obj[64]).all(), (tag, obj[64])   # a non-finite total: nothing was evaluated


# --------------------------------------------------------------------------------------- D. the optimiser's edge contract


def _timeopt_case(order, S=6, B=65):
    return Case((S,) * B, True, order, False, True, True, 0, None)


def _project_by_sorting(v, lo, total):
    """Euclidean projection onto {sum y = total, y >= lo}: with u = v - lo on the simplex of size total - S lo, the
    threshold from the sorted u (the classical sort-based rule), independent of the kernel's iteration over theta."""
    u = np.asarray(v, dtype=np.float64) - lo
    z = total - len(u) * lo
    s = np.sort(u)[::-1]
    cs = np.cumsum(s) - z
    j = np.arange(1, len(u) + 1)
    rho = np.flatnonzero(s - cs / j > 0)[-1]
    return np.maximum(u - cs[rho] / (rho + 1), 0.0) + lo


@pytest.mark.parametrize("order", [3, 4])
def test_optimiser_infeasible_fixed_total(csp, order):
    """Lanes 3 and 64 (the tail wave's only lane) have sum T < S min_time.  Device memory: their times come back bit for
    bit, status exactly NOT_CONVERGED, 0 iterations, both objectives NaN, and every other lane is bit-equal to a run
    without the infeasible lanes.  Host memory: CSP_ERR_INVALID_ARG, nothing written."""
    case = _timeopt_case(order)
    B, S = len(case.lens), case.lens[0]
    good = staged_buffers("optimize_times_batch", case.lens, order, False, True, 5100 + order)   # times in [0.5, 2]
    vw = np.random.default_rng(order).uniform(0.0, 0.3, size=B)
    bad = {k: v.copy() for k, v in good.items()}
    bad["times"].reshape(B, S)[[3, 64]] = 0.3
    prm = _timeopt_params(csp, min_time=0.5, max_iters=20)
    out_bad, _ = _call(csp, "optimize_times_batch", case, bad, 0xFF, vw, prm)
    out_good, _ = _call(csp, "optimize_times_batch", case, good, 0xFF, vw, prm)
    tin, tout = bad["times"].reshape(B, S), out_bad["times_out"].reshape(B, S)
    for k in (3, 64):
        assert tout[k].tobytes() == tin[k].tobytes(), (k, tout[k])
        assert out_bad["status"][k] == NOT_CONVERGED and out_bad["iterations"][k] == 0, (k, out_bad["status"][k])
        assert np.isnan(out_bad["objective"][k]).all(), (k, out_bad["objective"][k])
    others = np.setdiff1d(np.arange(B), [3, 64])
    assert not (out_bad["status"][others] & ~NOT_CONVERGED).any(), out_bad["status"]
    rb, rg = _rows(out_bad, B), _rows(out_good, B)
    for n in rb:
        assert np.array_equal(rb[n][others], rg[n][others]), (order, n)
    # the host-memory form checks the totals before it touches anything
    names = [n for n, _, _ in WORKSPACE_ENTRIES["optimize_times_batch"][2]]
    host = {n: bad[n].copy() for n in names}
    for n, kind, _ in WORKSPACE_ENTRIES["optimize_times_batch"][2]:
        if kind == "out":
            host[n].reshape(-1).view(np.uint8)[:] = 0x5A
    before = {n: host[n].tobytes() for n in names}
    desc = csp.make_desc(order, B, S, csp.DTYPE_F64, 0.0, VW, csp.MEM_HOST, True, None, 0, vw.ctypes.data)
    rc = csp.raw_lib().csp_minsnap_optimize_times_batch(ctypes.byref(desc), ctypes.byref(prm), *[host[n].ctypes.data for n in names],
                                                        None, 0, None)
    assert rc == -1, (rc, csp.strerror(rc))   # CSP_ERR_INVALID_ARG
    for n in names:
        assert host[n].tobytes() == before[n], n


@pytest.mark.parametrize("order", [3, 4])
def test_optimiser_projects_a_start_below_the_bound(csp, order):
    """max_iters = 0 returns the start: for the lanes with one (b % 4 == 1) or two (b % 4 == 2) entries below min_time
    and a feasible total that is the Euclidean projection onto {sum T = C, T >= min_time}, computed here by sorting;
    the other lanes come back bit for bit.  Compared at 1e-12 relative to the total C (both sides are a handful of fp64
    additions of numbers below C: ~S eps C); the sum holds to 1e-12 relative and no entry is below min_time.
    objective[:, 0] is the cost at the projected times (tests/timeopt_ref.cost_grad, GATE_J)."""
    case = _timeopt_case(order)
    B, S, lo = len(case.lens), case.lens[0], 0.5
    host = staged_buffers("optimize_times_batch", case.lens, order, False, True, 5200 + order)
    rng = np.random.default_rng(5200 + order)
    tin = rng.uniform(0.8, 2.0, size=(B, S))      # four entries of 0.8 and two of 0.2: still above S min_time
    tin[1::4, 2] = 0.2
    tin[2::4, 0], tin[2::4, 4] = 0.1, 0.3
    host["times"] = tin.reshape(-1).copy()
    vw = rng.uniform(0.0, 0.3, size=B)
    assert (tin.sum(axis=1) >= S * lo).all()
    prm = _timeopt_params(csp, min_time=lo, max_iters=0)
    out, _ = _call(csp, "optimize_times_batch", case, host, 0xFF, vw, prm)
    tout, obj = out["times_out"].reshape(B, S), out["objective"]
    assert not (out["status"] & ~NOT_CONVERGED).any() and not out["iterations"].any(), out["status"]
    assert obj[:, 0].tobytes() == obj[:, 1].tobytes()
    wp, bc = host["waypoints"].reshape(B, S + 1, 3), host["bc"]
    worst = 0.0
    for b in range(B):
        C = tin[b].sum()
        if b % 4 in (1, 2):
            want = _project_by_sorting(tin[b], lo, C)
            assert np.max(np.abs(tout[b] - want)) <= 1e-12 * C, (b, tout[b], want)
            assert (tout[b] == lo).sum() == (1 if b % 4 == 1 else 2), (b, tout[b])
        else:
            assert tout[b].tobytes() == tin[b].tobytes(), b
        assert abs(tout[b].sum() - C) <= 1e-12 * C and tout[b].min() >= lo, (b, tout[b])
        J, _ = cost_grad(order, wp[b], tout[b], bc[b], vw[b])
        worst = max(worst, abs(obj[b, 0] - J) / J)
    print("order %d: objective at the projected start against numpy, worst relative error %.2e" % (order, worst))
    assert worst < GATE_J[order], worst


def _active_bound_problem(order):
    case = _timeopt_case(order)
    B, S = len(case.lens), case.lens[0]
    host = staged_buffers("optimize_times_batch", case.lens, order, False, True, 5300 + order)
    t = host["times"].reshape(B, S)
    t *= S / t.sum(axis=1, keepdims=True)        # every trajectory has mean time 1, so min_time = 0.9 mean(T_in)
    return case, host, np.zeros(B)


@pytest.mark.parametrize("order", [3, 4])
def test_optimiser_with_the_bound_active_at_the_solution(csp, order):
    """min_time = 0.9 mean(T_in), fixed total, 300 iterations at most: the total leaves 0.6 of slack over six segments,
    and a random-walk path wants some segment shorter than that.  tests/timeopt_ref.optimize alone ends with the bound
    active on every one of the 65 trajectories of both orders (checked on the CPU when this test was written, and
    asserted here for the trajectories whose reference is computed).  "Active" per trajectory means: the smallest time
    is min_time up to the rounding of the last projection.  A trial point T + lam d is projected once more to remove
    the drift of its sum, and when the sum drifted down that theta is a negative multiple of an ulp, which lifts the
    clipped entries from min_time to min_time + 1 ulp (the reference does the same on 22 / 16 of the 65 trajectories at
    orders 3 / 4); the drift is bounded by the documented 1e-12 relative of the total.  So every trajectory must have
    an entry within 1e-12 C of min_time, and the result as a whole entries exactly at min_time.  The final objective
    must be within the margin of test_gpu_timeopt._invariants (2e-7 relative) of the reference optimiser's, the sum
    hold to 1e-12 relative and no entry be below the bound."""
    case, host, vw = _active_bound_problem(order)
    B, S, lo = len(case.lens), case.lens[0], 0.9
    prm = _timeopt_params(csp, min_time=lo, max_iters=300)
    out, _ = _call(csp, "optimize_times_batch", case, host, 0xFF, vw, prm)
    tin, tout, obj = host["times"].reshape(B, S), out["times_out"].reshape(B, S), out["objective"]
    assert not (out["status"] & ~NOT_CONVERGED).any(), out["status"]
    assert (obj[:, 1] <= obj[:, 0]).all()
    assert (tout.min(axis=1) >= lo).all()
    assert (np.abs(tout.sum(axis=1) - tin.sum(axis=1)) <= 1e-12 * tin.sum(axis=1)).all()
    C = tin.sum(axis=1)
    assert (tout.min(axis=1) - lo <= 1e-12 * C).all(), np.flatnonzero(tout.min(axis=1) - lo > 1e-12 * C)
    exact = (tout == lo).any(axis=1)
    print("order %d: %d of %d trajectories with an entry exactly at min_time, largest gap %.2e" % (order, exact.sum(), B, (tout.min(axis=1) - lo).max()))
    assert exact.any()
    wp, bc = host["waypoints"].reshape(B, S + 1, 3), host["bc"]
    for b in (0, 21, 42, 64):
        ref = optimize(order, wp[b], tin[b], bc[b], vw[b], "fixed_total", 0.0, lo, 1e-6, 500)
        assert ref["times"].min() - lo <= 1e-12 * C[b], (b, ref["times"])
        assert abs(ref["f"] - obj[b, 1]) <= 2e-7 * ref["f"], (b, ref["f"], obj[b, 1])


@pytest.mark.parametrize("order", [3, 4])
def test_optimiser_single_segment_fixed_total(csp, order):
    """S = 1 with a fixed total: the feasible set is the one point T = T_in, so the times come back bit for bit, the
    final objective is the initial one bit for bit, there are no iterations and no status bit other than possibly
    NOT_CONVERGED."""
    case = _timeopt_case(order, S=1)
    B = len(case.lens)
    host = staged_buffers("optimize_times_batch", case.lens, order, False, True, 5400 + order)
    vw = np.random.default_rng(order).uniform(0.0, 0.3, size=B)
    out, _ = _call(csp, "optimize_times_batch", case, host, 0xFF, vw, _timeopt_params(csp, min_time=0.1, max_iters=50))
    assert out["times_out"].tobytes() == host["times"].tobytes()
    assert out["objective"][:, 0].tobytes() == out["objective"][:, 1].tobytes() and np.isfinite(out["objective"]).all()
    assert not (out["status"] & ~NOT_CONVERGED).any() and not out["iterations"].any(), (out["status"], out["iterations"])
    # the coefficients are the solve's at those times
    ref = csp.solve_batch(host["waypoints"].reshape(B, 2, 3), host["times"].reshape(B, 1), host["bc"], order=order,
                          vel_zero_weight=VW, vel_zero_weight_per_traj=vw)
    assert out["coeffs"].tobytes() == ref.coeffs.tobytes()
