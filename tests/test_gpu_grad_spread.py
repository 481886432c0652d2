"""The reverse-mode, cost, knot-constraint and optimiser entries under unequal segment times (R = max T / min T = 16 inside
one trajectory; 256 on constant-speed legs), against 40-digit references.

tests/test_gpu_time_spread.py put every forward solve family under time spread; the entries below kept accuracy tests with
times U(0.5, 2) (R <= 4) and fixed gates that also carry the rounding of a dense numpy restatement.  Their kernels share
no elimination code with the forward kernels (six columns, bordered, identity rows for pinned unknowns), and the time
gradient is a difference of sums whose terms scale with powers of T up to 2 order - 1.

  entry                                         kernel                                   reference
  csp_minsnap_solve_batch_vjp / _cost_vjp       minsnap_vjp_kernel<O, IO, PBAR, JBAR>    spread_vjp_ref.open_chain (40 digits)
  csp_minsnap_cost_batch                        minsnap_timeopt.hip                      the same (J, dJ/dT)
  csp_minsnap_solve_periodic_batch_vjp          minsnap_periodic_vjp_kernel              spread_vjp_ref.loop (40 digits)
  csp_minsnap_solve_knots_batch                 minsnap_knots_kernel                     knots_ref.solve (40 digits)
  csp_minsnap_optimize_times_batch              minsnap_timeopt.hip                      test_gpu_timeopt._invariants, unchanged

The table, inputs, references and metrics are tests/grad_spread_cases.py's; tests/test_spread_vjp_ref.py ties the
references down and evaluates the table on the CPU.  Each parametrised id is one (family, order, pattern) group.  Per case:
status 0 on every trajectory; every copy of a trajectory bit-equal with its first copy (two calls bit-equal for a shared
bc, whose gradient is a sum over the batch); and per output

  relative   e_k <= max(10 e_cpu64, floor).  e_cpu64: the reference's own code in Python floats against 40 digits; floor:
             the gate the entry already carries at R <= 4 (GATE_NUMPY; GATE_J / GATE_G for the cost entry; TOL_LD for
             the knots; TOL_F32 where the output is stored in fp32).
  absolute   the 1e-6 north star on every case whose e_cpu64 is at most 1e-7 (every R = 16 case at orders <= 4:
             asserted on the CPU by tests/test_spread_vjp_ref.py); on a loop e_same must be within 1e-7 as well.

Outputs: grad_waypoints, grad_times, grad_bc of the three instantiations (grad_coeffs alone, grad_cost alone, both) under
two kinds of grad_coeffs (standard normal; standard normal times T_j^pow_i), J and dJ/dT of the cost entry, the knot
coefficients per power and their J.  Every time gradient is judged twice: max-abs over max-abs, and the same of g_j T_j
(the gradient with respect to log T) -- tests/test_spread_vjp_ref.py shows an error the first form cannot see.

With CSP_PARITY_SURVEY=<file> every gate appends its figures to the file and does not assert.

Measured on an MI355X (surveys of 2026-10-21), worst e_k at orders 2 / 3 / 4 / 5:
  open chain, R = 16     gradients 2.3e-14 / 1.5e-13 / 1.4e-10 / 9.8e-9, J 5.8e-16 / 3.6e-14 / 1.1e-12 / 4.5e-10, dJ/dT 3.3e-15 /
                         8.9e-14 / 8.5e-12 / 1.0e-9: nothing above its floor; fp32 storage 5.9e-8
  open chain, dist256    gradients 5.2e-14 / 1.6e-9 / 2.8e-7 at orders 2 / 3 / 4, at most 6.8 x e_cpu64; the cost entry's dJ/dT
                         3.1e-14 / 1.0e-10 / 6.7e-8, at most 0.64 x.  Before the reverse-mode and the cost kernel formed their
                         right-hand sides from the legs: gradients 3.7e-12 / 2.2e-8 / 2.6e-5 (up to 1774 x), the cost-only
                         grad_bc at order 4 9.1e-9 (270 x), dJ/dT 1.9e-13 / 9.7e-11 / 1.7e-6 (83 x / 45 x / 2.7 x)
  periodic, R = 16       2.2e-14 / 1.3e-11 / 2.6e-9 / 3.4e-5 (62 x at order 3, 9.4e6 x at order 5): RATIO_GATE, within 2.1 x e_same
  knots, R = 16          coefficients 4.4e-15 / 1.7e-12 / 2.2e-9 / 4.1e-6, J 1.2e-15 / 3.5e-14 / 3.9e-10 / 4.1e-7, at most 1.25 x e_cpu64
  optimiser              64 - 65 of 65 lanes converged at orders 2 - 4 and 56 - 60 at order 5 in the first surveys (required 48 / 40)
"""
import functools
import json
import os

import numpy as np
import pytest

from tests import grad_spread_cases as gc
from tests import knots_ref
from tests import spread_cases as sc
from tests import test_gpu_knots as tk
from tests.test_gpu_edges import TOL_F32, TOL_LD
from tests.test_gpu_timeopt import GATE_G, GATE_J, _invariants
from tests.test_gpu_vjp import GATE_NUMPY

pytestmark = pytest.mark.gpu

SURVEY = os.environ.get("CSP_PARITY_SURVEY")


# Where a (quantity, order) exceeds the factor 10 for a cause that is understood and belongs to the formulation, it is gated
# at twice the worst ratio e_k / e_cpu64 of the survey run (the margin of 2: run-to-run and case-to-case variation of a
# worst-case figure, as tests/test_gpu_time_spread.py's RATIO_GATE), and a second relative gate with the ordinary factor
# 10 holds it to e_same: plain fp64 on the CPU doing the kernel's own math.
#   periodic: the free-derivative loop system, formed in fp64, has lost the digits (section 17.3).  e_same =
#     tests/periodic_vjp_ref.py, that system in numpy fp64; the kernel is within 2.1 x of it.  At order 5 the reverse mode,
#     like the forward, does not reach the 1e-6 north star under R = 16 (3.4e-5 at worst).  The north star is asserted on a
#     loop only where e_same is within 1e-7 too (tests/test_spread_vjp_ref.py: every case up to order 4, not order 5).
#     At order 5 the ratio gates (1e6 and more times an e_cpu64 of up to 8e-8) bound nothing by themselves: the effective
#     gate there is the second one, 10 x e_same (numpy, up to 3.2e-4), a hundred times the kernel's measured 3.4e-5.
# The open-chain kernels need no entry: the reverse-mode and the cost kernel lost up to 1774 x and 83 x e_cpu64 on dist256
# while they summed four nearly opposite products of the waypoints per knot; both now form their right-hand sides from
# the legs.
RATIO_GATE = {("periodic", 3, "times"): 2 * 62.2, ("periodic", 5, "times"): 2 * 9.45e6, ("periodic", 5, "times_T"): 2 * 1.823e6,
              ("periodic", 5, "waypoints"): 2 * 2.373e6}


def _judge(tag, e_k, e_cpu, floor, absolute, factor=gc.FACTOR):
    if SURVEY:
        with open(SURVEY, "a") as f:
            f.write(json.dumps({"tag": [str(t) for t in tag], "e_k": e_k, "e_cpu64": e_cpu, "ratio": e_k / max(e_cpu, 1e-300),
                                "floor": floor, "absolute": bool(absolute)}) + "\n")
        return
    assert gc.within(e_k, e_cpu, floor, factor), ("relative gate", tag, "factor %.4g" % factor, "e_k %.3e" % e_k, "e_cpu64 %.3e" % e_cpu,
                                                  "floor %.1e" % floor)
    if absolute:
        assert e_k <= gc.NORTH_STAR_TOL, ("north star", tag, e_k)


def _judge_all(c, e_k, e_cpu, floor_of, same_math=None):
    """same_math(c) -> {key: e_same} where the family has a formulation of its own (the loops)."""
    group = "periodic" if c.family == "periodic" else "open256" if c.pattern == "dist256" else "open"
    e_same = same_math(c) if same_math else None
    absolute = max(e_cpu.values()) <= gc.ABSOLUTE_AT and (e_same is None or max(e_same.values()) <= gc.ABSOLUTE_AT)
    for key in sorted(e_cpu):
        print("%s %s: e_k %.3e  e_cpu64 %.3e" % (c.id, key, e_k[key], e_cpu[key]))
        rg = RATIO_GATE.get((group, c.order, key[1]))
        _judge((c.family, c.order, c.id) + key, e_k[key], e_cpu[key], floor_of(key[1]), absolute, rg or gc.FACTOR)
        if rg and e_k[key] > floor_of(key[1]):
            _judge((c.family + " same-math", c.order, c.id) + key, e_k[key], e_same[key], floor_of(key[1]), False)


def _same_bytes(a, b, tag):
    for x, y in zip(a, b):
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), tag


def _copies_are_bit_equal(a, rows, tag):
    a = np.ascontiguousarray(a)
    for b in range(rows, a.shape[0]):
        assert a[b].tobytes() == a[b % rows].tobytes(), ("copy differs from the first copy of its trajectory", tag, b)


# ------------------------------------------------------------------------------------------------------------- open chain


def _open_batch(c):
    """The batch of a case in the call's layouts: (wp, tm, bc, w, pbar [2, ...], jbar, seg_offsets or None, slices)."""
    ms = gc.members(c)
    ins = [gc.open_inputs(c, m) for m in ms]
    cot = [gc.cotangents("open", c.pattern, c.order, m[0], c.f32, m[1]) for m in ms]
    if c.lens:
        off = np.concatenate([[0], np.cumsum(c.lens)]).astype(np.int64)
        wp, tm = np.concatenate([i[0] for i in ins]), np.concatenate([i[1] for i in ins])
        bc, w = np.stack([i[2] for i in ins]), np.array([i[3] for i in ins])
        pb = np.concatenate([q[0] for q in cot], axis=1)
        jb = np.array([q[1] for q in cot])
        sl = [(slice(off[b] + b, off[b + 1] + b + 1), slice(off[b], off[b + 1]), b) for b in range(len(ms))]
    else:
        off = None
        idx = np.arange(gc.B) % c.rows
        wp, tm = np.stack([i[0] for i in ins])[idx], np.stack([i[1] for i in ins])[idx]
        bc = np.stack([i[2] for i in ins])[idx] if c.bc_per else ins[0][2][None]
        w = np.array([i[3] for i in ins])[idx] if c.bc_per else sc.VW
        pb = np.stack([q[0] for q in cot], axis=1)[:, idx]
        jb = np.array([q[1] for q in cot])[idx]
        sl = [(r, r, r) for r in range(c.rows)]
    if c.f32:
        wp, tm, bc, pb = (x.astype(np.float32) for x in (wp, tm, bc, pb))
    return tuple(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x for x in (wp, tm, bc, w, pb, jb)) + (off, sl)


def _open_kernel_source(csp, c):
    wp, tm, bc, w, pb, jb, off, sl = _open_batch(c)
    kw = dict(order=c.order, seg_offsets=off, max_segments=max(c.lens) if c.lens else None)
    kw["vel_zero_weight_per_traj" if np.ndim(w) else "vel_zero_weight"] = w
    fl = np.float32 if c.f32 else np.float64
    src = {}
    for call in gc.CALLS:
        gco = pb[int(call[-1])] if call[:4] in ("coef", "both") else None
        gj = jb if call[:4] in ("cost", "both") else None
        r = csp.solve_batch_vjp(wp, tm, gco, bc=bc, grad_cost=gj, want_status=True, **kw)
        assert not r.status.any(), (c.id, call, "status raised on valid inputs", r.status)
        assert r.waypoints.dtype == fl and r.times.dtype == fl and r.bc.dtype == fl
        if not c.lens:
            _copies_are_bit_equal(r.waypoints, c.rows, (c.id, call, "waypoints"))
            _copies_are_bit_equal(r.times, c.rows, (c.id, call, "times"))
            if c.bc_per:
                _copies_are_bit_equal(r.bc, c.rows, (c.id, call, "bc"))
        if not c.bc_per:
            again = csp.solve_batch_vjp(wp, tm, gco, bc=bc, grad_cost=gj, **kw)
            _same_bytes((r.waypoints, r.times, r.bc), (again.waypoints, again.times, again.bc), (c.id, call, "two calls differ"))
        gbc = r.bc.reshape(-1, 4, 3)
        per = [dict(waypoints=r.waypoints[a].astype(np.float64), times=r.times[b].astype(np.float64),
                    bc=gbc[i].astype(np.float64) if c.bc_per else None) for a, b, i in sl]
        src[call] = (per, None if c.bc_per else gbc[0].astype(np.float64))
    r = csp.snap_cost_batch(wp, tm, bc, **kw)
    assert not r.status.any(), (c.id, "cost entry", r.status)
    if not c.lens:
        _copies_are_bit_equal(r.cost, c.rows, (c.id, "J"))
        _copies_are_bit_equal(r.grad_times, c.rows, (c.id, "dJ/dT"))
    src["costentry"] = [(float(r.cost[i]), r.grad_times[b].astype(np.float64)) for _, b, i in sl]
    return src


def _open_floor(c, out):
    if out == "J":
        return GATE_J[c.order]               # J is stored in fp64 whatever the storage type
    base = GATE_G[c.order] if out.startswith("dJdT") else GATE_NUMPY[c.order]
    return max(base, TOL_F32) if c.f32 else base


@pytest.mark.parametrize("order,pattern", gc.OPEN_GROUPS, ids=["o%d-%s" % g for g in gc.OPEN_GROUPS])
def test_open_chain_vjp_cost_vjp_and_cost(csp, order, pattern):
    """B = 65 (one full wave and one lane of the next), uniform S in {1, 2, 3, 16, 40} with a shared and with per-trajectory
    bc, fp32 storage at S = 3 and 16, one ragged batch (1, 2, 17, 1, 5, 64); dist256 at order 4 is one case."""
    for c in gc.open_cases(order, pattern):
        _judge_all(c, gc.open_errors(c, _open_kernel_source(csp, c)), gc.open_cpu64(c), functools.partial(_open_floor, c))


# -------------------------------------------------------------------------------------------------------------- periodic


def _loop_kernel_source(csp, c):
    ms = gc.members(c)
    ins = [gc.loop_inputs(c, m) for m in ms]
    cot = [gc.cotangents("periodic", c.pattern, c.order, m[0], False, m[1]) for m in ms]
    if c.lens:
        off = np.concatenate([[0], np.cumsum(c.lens)]).astype(np.int64)
        wp, tm, w = np.concatenate([i[0] for i in ins]), np.concatenate([i[1] for i in ins]), np.array([i[2] for i in ins])
        pb, jb = np.concatenate([q[0] for q in cot], axis=1), np.array([q[1] for q in cot])
        sl = [slice(off[b], off[b + 1]) for b in range(len(ms))]
    else:
        off = None
        idx = np.arange(gc.B) % c.rows
        wp, tm, w = (np.ascontiguousarray(np.stack([i[k] for i in ins])[idx]) for k in range(3))
        pb, jb = np.ascontiguousarray(np.stack([q[0] for q in cot], axis=1)[:, idx]), np.array([q[1] for q in cot])[idx]
        sl = list(range(c.rows))
    src = {}
    for call in gc.PERIODIC_CALLS:
        r = csp.solve_periodic_batch_vjp(wp, tm, np.ascontiguousarray(pb[int(call[-1])]), grad_cost=jb if call.startswith("both") else None,
                                         order=c.order, vel_zero_weight_per_traj=w, seg_offsets=off,
                                         max_segments=max(c.lens) if c.lens else None, want_status=True)
        assert not r.status.any(), (c.id, call, r.status)
        if not c.lens:
            _copies_are_bit_equal(r.waypoints, c.rows, (c.id, call, "waypoints"))
            _copies_are_bit_equal(r.times, c.rows, (c.id, call, "times"))
        src[call] = [dict(waypoints=r.waypoints[s], times=r.times[s]) for s in sl]
    return src


@pytest.mark.parametrize("order,pattern", gc.PERIODIC_GROUPS, ids=["o%d-%s" % g for g in gc.PERIODIC_GROUPS])
def test_periodic_vjp(csp, order, pattern):
    """The loops of spread_cases.loops (shared with the forward test), S in {1, 2, 3, 5, 12}, B = 65, with and without
    grad_cost, and the ragged batch (12, 3, 1, 2, 5)."""
    from tests.test_gpu_periodic_vjp import GATE_NUMPY as GATE_PERIODIC
    for c in gc.periodic_cases(order, pattern):
        _judge_all(c, gc.loop_errors(c, _loop_kernel_source(csp, c)), gc.loop_cpu64(c), lambda out: GATE_PERIODIC[order], gc.loop_same_math)


# ----------------------------------------------------------------------------------------------------------------- knots


@functools.lru_cache(maxsize=None)
def _knot_case(order, S, mask, pattern, row):
    """tests/test_gpu_knots.py::make_case's mask, values and weight on the pattern's waypoints and times, with its
    references: (path, time, mask, values, w, 40-digit Solution or None when the mask is unsolvable, the same in floats)."""
    _, _, mk, kv, w = tk.make_case(order, S, mask, row)
    wp, tm = gc.knot_times(pattern, S)
    if knots_ref.constraint_count(order, mk) < order:
        return wp[row], tm[row], mk, kv, w, None, None
    hi = knots_ref.solve(order, wp[row], tm[row], mk, kv, vel_zero_weight=w)
    lo = knots_ref.solve(order, wp[row], tm[row], mk, kv, vel_zero_weight=w, dps=None)
    return wp[row], tm[row], mk, kv, w, hi, lo


KNOT_GROUPS = [(o, p) for o in gc.ORDERS for p in gc.R16]


@pytest.mark.parametrize("order,pattern", KNOT_GROUPS, ids=["o%d-%s" % g for g in KNOT_GROUPS])
def test_knots(csp, order, pattern):
    """make_case's masks (standard, free_end, vel_mid, hermite, random) at S in {3, 16, 17}, B = 65, want_cost; unsolvable
    mask / shape combinations are skipped by knots_ref.constraint_count as tests/test_gpu_knots.py does."""
    for mask in gc.KNOT_MASKS:
        for S in gc.KNOT_S:
            cs = [_knot_case(order, S, mask, pattern, r) for r in range(gc.KNOT_K)]
            if any(x[5] is None for x in cs):
                assert mask == "random" and S + 1 < order, (order, S, mask)
                continue
            idx = np.arange(gc.B) % gc.KNOT_K
            wp, tm, mk, kv, w = (np.ascontiguousarray(np.stack([x[i] for x in cs])[idx]) for i in range(5))
            r = csp.solve_knots_batch(wp, tm, mk, kv, order=order, vel_zero_weight_per_traj=w, want_cost=True)
            tag = ("knots", order, pattern, mask, S)
            assert not r.status.any(), (tag, r.status)
            _copies_are_bit_equal(r.coeffs, gc.KNOT_K, tag)
            _copies_are_bit_equal(r.cost, gc.KNOT_K, tag)
            ek = ej = ck = cj = 0.0
            for row, (p, t, m_, _, _, hi, lo) in enumerate(cs):
                a, b = tk.errors(order, r.coeffs[row], r.cost[row], hi, p, t, m_)
                c_, d = tk.errors(order, lo.coeffs, lo.cost, hi, p, t, m_)
                ek, ej, ck, cj = max(ek, a), max(ej, b), max(ck, c_), max(cj, d)
            print("%s: coeffs e_k %.3e e_cpu64 %.3e, J e_k %.3e e_cpu64 %.3e" % (tag, ek, ck, ej, cj))
            absolute = max(ck, cj) <= gc.ABSOLUTE_AT
            _judge(tag + ("coeffs",), ek, ck, TOL_LD[order], absolute)
            _judge(tag + ("cost",), ej, cj, TOL_LD[order], absolute)


# ------------------------------------------------------------------------------------------------------------- optimiser


@pytest.mark.parametrize("mode", gc.OPT_MODES)
@pytest.mark.parametrize("pattern", gc.OPT_PATTERNS)
@pytest.mark.parametrize("order", gc.ORDERS)
def test_optimiser_from_spread_starts(csp, order, pattern, mode):
    """optimize_times_batch from starts of ratio 16, B = 65, S = 6: tests/test_gpu_timeopt.py::_invariants unchanged (bounds,
    exact total, objective against timeopt_ref, the projected-gradient measure on converged lanes, the reference
    optimiser's objective on the first four), and the converged share of test_optimiser_invariants: 5/8 at order 5, 3/4
    otherwise -- which the reference optimiser alone reaches from these starts (tests/test_spread_vjp_ref.py)."""
    wp, tm, bc, rho = gc.opt_problem(order, pattern, mode)
    # the trajectories the reference optimiser can judge lead the batch: 0 - 3, but none at order 5 under alt16 with a fixed
    # total (grad_spread_cases.opt_ref_lanes, tests/test_spread_vjp_ref.py)
    perm = gc.opt_batch_order(order, pattern, mode)
    wp, tm, bc = wp[perm], tm[perm], bc[perm]
    r = csp.optimize_times_batch(np.array(wp), np.array(tm), np.array(bc), order=order, mode=mode, time_weight=rho, min_time=gc.OPT_TMIN,
                                 tol=gc.OPT_TOL, max_iters=gc.OPT_ITERS)
    nconv = _invariants(order, wp, tm, bc, 0.0, r, mode, rho, gc.OPT_TMIN, gc.OPT_TOL, check_ref=len(gc.opt_ref_lanes(order, pattern, mode)))
    print("o%d %s %s: converged %d / %d, iterations %s" % (order, pattern, mode, nconv, gc.B, np.percentile(r.iterations, [0, 50, 100])))
    if SURVEY:
        with open(SURVEY, "a") as f:
            f.write(json.dumps({"tag": ["opt", str(order), pattern, mode], "converged": int(nconv), "need": gc.opt_share(order)}) + "\n")
        return
    assert nconv >= gc.opt_share(order), (nconv, gc.opt_share(order))
