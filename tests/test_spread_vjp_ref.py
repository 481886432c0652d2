"""tests/spread_vjp_ref.py (the 40-digit adjoint of the open-chain and the periodic solve) tied down without a GPU, and
the case table of tests/grad_spread_cases.py evaluated on the CPU.

  central differences   the adjoint's gradients against 40-digit central differences of the FORWARD references
                        (knots_ref.solve(raw=True) with the standard mask; periodic_ref.solve(raw=True)).  Waypoints and
                        bc move by 1 (L is linear in them and J quadratic, so the difference is exact; the inputs are
                        rounded to multiples of 2^-20 so that x +- 1 is an exact double); times are multiples of 2^-20 and
                        move by 2^-30 and 2^-31 (every T +- h an exact double), the two differences Richardson-
                        extrapolated.  Truncation O(h^4) ~ 1e-36, rounding ~ 1e-40 / h ~ 1e-31: 1e-20 relative per
                        gradient leaves ten digits for the growth of the higher derivatives and is four digits below a
                        double's rounding.
  40 against 60 digits  rounded to double they agree within 4 ulp of the largest entry of each gradient, on every distinct
                        trajectory of the table (the rule of tests/test_spread_ref.py).
  the table             per (family, order, pattern): e_cpu64 (the adjoint in Python floats against 40 digits) and the
                        errors of the dense numpy restatements (vjp_ref, cost_vjp_ref, timeopt_ref, periodic_vjp_ref) in the
                        GPU test's metrics, printed; asserted: e_cpu64 <= 1e-7 on every R = 16 case at orders <= 4 -- the
                        condition under which the GPU test asserts the 1e-6 north star on the kernel.  Where it does not
                        hold (order 5, dist256) the case is printed and keeps the relative gate only.
  sensitivity           why the time gradient is gated in two metrics (see the test).
  the optimiser         the reference optimiser alone reaches the converged shares the GPU test requires.

Measured (this file's table test, worst over the table, orders 2 / 3 / 4 / 5): see DESIGN.md section 21.
"""
import numpy as np
import pytest

from tests import grad_spread_cases as gc
from tests import knots_ref, periodic_ref
from tests import spread_ref as sr
from tests import spread_vjp_ref as sv

FD_TOL = 1e-20
Q20 = 2.0 ** 20
H1, H2 = 2.0 ** -30, 2.0 ** -31


def _q(a):
    return np.round(np.asarray(a, dtype=np.float64) * Q20) / Q20


def _rel(got, ref):
    import mpmath
    got, ref = np.asarray(got, dtype=object).reshape(-1), np.asarray(ref, dtype=object).reshape(-1)
    den = max([abs(v) for v in ref] + [mpmath.mpf(0)])
    num = max(abs(a - b) for a, b in zip(got, ref))
    return num / den if den != 0 else num


def _fd_inputs(order, S, pattern, loop):
    wp, tm = (sr.spread_loops if loop else sr.spread_batch)(pattern, 2, S, 7)
    rng = np.random.default_rng([order, S, int(loop), "la".index(pattern[0])])
    return _q(wp[1]), _q(tm[1]), _q(rng.normal(size=(4, 3))), rng.normal(size=(S, 3, 2 * order)), float(rng.normal())


def _central(f, x, idx, h):
    a, b = x.copy(), x.copy()
    a[idx] += h
    b[idx] -= h
    return (f(a) - f(b)) / (2 * h)


def _check_fd(f_L, f_J, adj, wp, tm, bc, tag):
    """f_L / f_J (wp, tm, bc) -> mpmath scalars <pbar, coeffs> and J; adj the Adjoint (raw, jbar = 1)."""
    import mpmath
    for name, f, gw, gt, gb in (("L", f_L, adj.waypoints, adj.times, adj.bc), ("J", f_J, adj.cost_waypoints, adj.cost_times, adj.cost_bc)):
        fw = np.array([[_central(lambda x: f(x, tm, bc), wp, (k, ax), 1.0) for ax in range(3)] for k in range(wp.shape[0])], dtype=object)
        assert _rel(gw, fw) <= FD_TOL, (tag, name, "waypoints", mpmath.nstr(_rel(gw, fw), 3))
        if bc is not None:
            fb = np.array([[_central(lambda x: f(wp, tm, x), bc, (r, ax), 1.0) for ax in range(3)] for r in range(4)], dtype=object)
            assert _rel(gb, fb) <= FD_TOL, (tag, name, "bc", mpmath.nstr(_rel(gb, fb), 3))
        d1 = [_central(lambda x: f(wp, x, bc), tm, j, H1) for j in range(len(tm))]
        d2 = [_central(lambda x: f(wp, x, bc), tm, j, H2) for j in range(len(tm))]
        ft = np.array([(4 * b - a) / 3 for a, b in zip(d1, d2)], dtype=object)
        assert _rel(gt, ft) <= FD_TOL, (tag, name, "times", mpmath.nstr(_rel(gt, ft), 3))


@pytest.mark.parametrize("pattern", ["log16", "alt16"])
@pytest.mark.parametrize("order", gc.ORDERS)
def test_open_chain_against_central_differences(order, pattern):
    import mpmath
    for S in (1, 2, 3, 5):
        for w in (0.0, 0.3):
            wp, tm, bc, pbar, _ = _fd_inputs(order, S, pattern, False)

            def forward(p, t, b):
                mask, values = knots_ref.standard_problem(order, S, b)
                return knots_ref.solve(order, p, t, mask, values, vel_zero_weight=w, dps=40, raw=True)

            def f_L(p, t, b):
                co = forward(p, t, b).coeffs
                with mpmath.workdps(40):
                    return sum(mpmath.mpf(float(pbar[j, ax, i])) * co[j][ax][i] for j in range(S) for ax in range(3) for i in range(2 * order))

            with mpmath.workdps(40):
                adj = sv.open_chain(order, wp, tm, bc, w, pbar, 1.0, dps=40, raw=True)
                _check_fd(f_L, lambda p, t, b: forward(p, t, b).cost, adj, wp, tm, bc, (order, pattern, S, w))


@pytest.mark.parametrize("pattern", ["log16", "alt16"])
@pytest.mark.parametrize("order", gc.ORDERS)
def test_loop_against_central_differences(order, pattern):
    import mpmath
    for S in (1, 2, 3, 5):
        for w in (0.0, 0.3):
            wp, tm, _, pbar, _ = _fd_inputs(order, S, pattern, True)

            def f_L(p, t, b):
                co = periodic_ref.solve(order, p, t, w, dps=40, raw=True)[0]
                with mpmath.workdps(40):
                    return sum(mpmath.mpf(float(pbar[j, ax, i])) * co[j, ax, i] for j in range(S) for ax in range(3) for i in range(2 * order))

            with mpmath.workdps(40):
                adj = sv.loop(order, wp, tm, w, pbar, 1.0, dps=40, raw=True)
                _check_fd(f_L, lambda p, t, b: periodic_ref.solve(order, p, t, w, dps=40, raw=True)[1], adj, wp, tm, None,
                          (order, pattern, S, w))


def test_float_mode_and_forward_agree_with_the_forward_references():
    """dps=None runs in Python floats (no mpmath number leaks out), and the adjoint's own forward solve returns the
    coefficients of spread_ref.solve / periodic_ref.solve to the last bits of a double."""
    for order in gc.ORDERS:
        wp, tm, bc, pbar, jbar = _fd_inputs(order, 5, "log16", False)
        lo = sv.open_chain(order, wp, tm, bc, 0.3, pbar, jbar, dps=None, raw=True)
        assert all(type(v) is float for v in lo.times.reshape(-1)) and type(lo.cost) is float
        hi = sv.open_chain(order, wp, tm, bc, 0.3, pbar, jbar)
        ref = sr.solve(order, wp, tm, bc, 0.3)
        assert np.max(np.abs(hi.coeffs - ref)) <= 4 * np.finfo(np.float64).eps * np.max(np.abs(ref))
        lw, lt, _, lp, _ = _fd_inputs(order, 5, "log16", True)
        hl = sv.loop(order, lw, lt, 0.3, lp, jbar)
        rc, rj, rg = periodic_ref.solve(order, lw, lt, 0.3, dps=40)
        assert np.max(np.abs(hl.coeffs - rc)) <= 4 * np.finfo(np.float64).eps * np.max(np.abs(rc))
        assert abs(hl.cost - rj) <= 4 * np.finfo(np.float64).eps * abs(rj)
        assert np.max(np.abs(hl.cost_grad_times - rg)) <= 4 * np.finfo(np.float64).eps * np.max(np.abs(rg))
        assert type(sv.loop(order, lw, lt, 0.3, lp, jbar, dps=None, raw=True).cost) is float


# ---------------------------------------------------------------------------------------------------------------- the table


def _ulp4(a, b, tag):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    big = max(float(np.max(np.abs(a))), 1e-300)
    assert np.max(np.abs(a - b)) <= 4 * np.spacing(big), (tag, float(np.max(np.abs(a - b))), big)


def _agree(x, y, tag):
    for k in ("coeffs", "cost_grad_times", "waypoints", "times", "bc", "cost_waypoints", "cost_times", "cost_bc"):
        if getattr(x, k) is None:
            continue
        a, b = np.asarray(getattr(x, k)), np.asarray(getattr(y, k))
        if k in ("waypoints", "times", "bc"):          # one gradient per cotangent
            for i in range(a.shape[0]):
                _ulp4(a[i], b[i], tag + (k, i))
        elif k == "coeffs":                            # per power, as the forward table does
            for i in range(a.shape[-1]):
                _ulp4(a[..., i], b[..., i], tag + (k, i))
        else:
            _ulp4(a, b, tag + (k,))
    _ulp4(x.cost, y.cost, tag + ("cost",))


@pytest.mark.parametrize("order,pattern", gc.OPEN_GROUPS, ids=["o%d-%s" % g for g in gc.OPEN_GROUPS])
def test_open_table_cpu(order, pattern, capsys):
    """40 against 60 digits on every distinct trajectory; e_cpu64 and the numpy restatements' errors per case."""
    worst_cpu, worst_np = {}, {}
    for c in gc.open_cases(order, pattern):
        for mem in gc.members(c):
            _agree(gc.open_adjoint(c, mem, 40), gc.open_adjoint(c, mem, 60), (c.id, mem))
        cpu, npy = gc.open_cpu64(c), gc.open_errors(c, gc.numpy_source(c))
        for k in cpu:
            gc._worst(worst_cpu, k[1], cpu[k])
            gc._worst(worst_np, k[1], npy[k])
        e = max(cpu.values())
        if pattern != "dist256" and order <= 4:
            assert e <= gc.ABSOLUTE_AT, (c.id, max(cpu, key=cpu.get), e)
        elif e > gc.ABSOLUTE_AT:
            with capsys.disabled():
                print("\n%s: e_cpu64 %.2e at %s -- relative gate only on the outputs above %.0e" % (c.id, e, max(cpu, key=cpu.get), gc.ABSOLUTE_AT))
    with capsys.disabled():
        print("\nopen o%d %s  e_cpu64 | numpy restatement: " % (order, pattern)
              + "  ".join("%s %.1e | %.1e" % (k, worst_cpu[k], worst_np[k]) for k in sorted(worst_cpu)))


@pytest.mark.parametrize("order,pattern", gc.PERIODIC_GROUPS, ids=["o%d-%s" % g for g in gc.PERIODIC_GROUPS])
def test_periodic_table_cpu(order, pattern, capsys):
    worst_cpu, worst_np = {}, {}
    for c in gc.periodic_cases(order, pattern):
        for mem in gc.members(c):
            _agree(gc.loop_adjoint(c, mem, 40), gc.loop_adjoint(c, mem, 60), (c.id, mem))
        cpu, npy = gc.loop_cpu64(c), gc.loop_errors(c, gc.loop_numpy_source(c))
        for k in cpu:
            gc._worst(worst_cpu, k[1], cpu[k])
            gc._worst(worst_np, k[1], npy[k])
        e = max(cpu.values())
        if order <= 4:
            assert e <= gc.ABSOLUTE_AT, (c.id, max(cpu, key=cpu.get), e)
        elif e > gc.ABSOLUTE_AT:
            with capsys.disabled():
                print("\n%s: e_cpu64 %.2e at %s -- relative gate only on the outputs above %.0e" % (c.id, e, max(cpu, key=cpu.get), gc.ABSOLUTE_AT))
    with capsys.disabled():
        print("\nperiodic o%d %s  e_cpu64 | numpy restatement: " % (order, pattern)
              + "  ".join("%s %.1e | %.1e" % (k, worst_cpu[k], worst_np[k]) for k in sorted(worst_cpu)))


@pytest.mark.parametrize("order", gc.ORDERS)
def test_numpy_restatements_at_small_spread(order, capsys):
    """The errors GATE_NUMPY carries, separated, where the existing tests live (times U(0.5, 2), R <= 4): the dense numpy
    restatements and the adjoint in Python floats, both against 40 digits, same metrics.  Printed;
    asserted: each alone stays inside GATE_NUMPY, the fixed gate that carries the restatement's error and the kernel's."""
    from tests import cost_vjp_ref, synth, vjp_ref
    from tests.test_gpu_vjp import GATE_NUMPY
    worst = {"cpu64": 0.0, "numpy": 0.0}
    for S in (3, 16, 40):
        wp, tm = synth.make_batch(2, S, config_id=3, offset=order)
        rng = np.random.default_rng([order, S])
        bc, pbar, jbar, w = rng.normal(size=(4, 3)), rng.normal(size=(S, 3, 2 * order)), float(rng.normal()), 0.2
        hi = sv.open_chain(order, wp[0], tm[0], bc, w, pbar, jbar)
        lo = sv.open_chain(order, wp[0], tm[0], bc, w, pbar, jbar, dps=None)
        r, cj = vjp_ref.adjoint(order, wp[0], tm[0], bc, pbar, w), cost_vjp_ref.cost_adjoint(order, wp[0], tm[0], bc, w)
        ref = {k: getattr(hi, k) + getattr(hi, "cost_" + k) for k in ("waypoints", "times", "bc")}
        worst["cpu64"] = max([worst["cpu64"]] + list(gc.grad_errors({k: getattr(lo, k) + getattr(lo, "cost_" + k) for k in ref}, ref, tm[0]).values()))
        worst["numpy"] = max([worst["numpy"]] + list(gc.grad_errors({k: r[k] + jbar * cj[k] for k in ref}, ref, tm[0]).values()))
    with capsys.disabled():
        print("\nR <= 4, order %d: float adjoint %.1e, numpy restatements %.1e" % (order, worst["cpu64"], worst["numpy"]))
    assert max(worst.values()) <= GATE_NUMPY[order], worst


# -------------------------------------------------------------------------------------------------------------- sensitivity


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("order", [4, 5])
def test_both_time_gradient_metrics_are_needed(order, S):
    """The two smallest alt16 cases with a short and a long segment.  The 40-digit time gradient, wrong in the entry of a
    LONG segment by 100 x the figure the T-weighted gate allows ten of (max(e_cpu64, floor / 10) of the T-weighted metric,
    times the largest |g_j T_j|), is fed in as the kernel's answer: the T-weighted gate fails, and the plain max-abs
    metric, whose denominator is the short segment's entry (about 16^(2o) / 16 times larger), would have passed."""
    from tests.test_gpu_vjp import GATE_NUMPY
    c = gc.Case("open", "alt16", order, S)
    mem = gc.members(c)[1]
    tm = gc.open_inputs(c, mem)[1]
    ref = gc.combine(gc.open_adjoint(c, mem, 40), "both0")
    cpu = gc.grad_errors(gc.combine(gc.open_adjoint(c, mem, None), "both0"), ref, tm)
    floor = GATE_NUMPY[order]
    j = int(np.argmax(tm))
    assert tm[j] >= 8 * tm.min()
    bad = {k: np.array(v, dtype=np.float64) for k, v in ref.items()}
    bad["times"][j] += 100.0 * max(cpu["times_T"], floor / 10.0) * np.max(np.abs(ref["times"] * tm)) / tm[j]
    e = gc.grad_errors(bad, ref, tm)
    assert not gc.within(e["times_T"], cpu["times_T"], floor), (e, cpu)
    assert gc.within(e["times"], cpu["times"], floor), (e, cpu)


# ---------------------------------------------------------------------------------------------------------------- optimiser


@pytest.mark.parametrize("mode", gc.OPT_MODES)
@pytest.mark.parametrize("pattern", gc.OPT_PATTERNS)
@pytest.mark.parametrize("order", gc.ORDERS)
def test_reference_optimiser_reaches_the_share(order, pattern, mode):
    """The converged share the GPU test requires of the kernel (5/8 at order 5, 3/4 otherwise: test_optimiser_invariants')
    is reached by tests/timeopt_ref.optimize alone from these starts; otherwise the seed would have to change, not the
    share."""
    from tests.timeopt_ref import optimize
    wp, tm, bc, rho = gc.opt_problem(order, pattern, mode)
    st = [optimize(order, wp[b], tm[b], bc[b], 0.0, mode, rho, gc.OPT_TMIN, gc.OPT_TOL, gc.OPT_ITERS)["status"] for b in range(gc.B)]
    assert sum(s == 0 for s in st) >= gc.opt_share(order), (sum(s == 0 for s in st), gc.opt_share(order))


@pytest.mark.parametrize("mode", gc.OPT_MODES)
@pytest.mark.parametrize("pattern", gc.OPT_PATTERNS)
@pytest.mark.parametrize("order", gc.ORDERS)
def test_reference_optimiser_reproduces_itself_where_it_judges(order, pattern, mode, capsys):
    """The GPU test compares the kernel's final objective with the reference optimiser's on the first four trajectories
    on which the reference's own result moves by at most a tenth of that comparison's bound under last-bit changes of
    the start.  Those are trajectories 0 - 3 in every group (at order 4 under alt16 with a fixed total after the seed
    moved) but one.  At order 5 under alt16 with a fixed total the reference reproduces itself on NO trajectory of the
    batch (median spread 3e-5, smallest 1.5e-7, bound 1e-6; over six seeds tried, 1 trajectory of 390 did), so no seed
    can help and that comparison is not made in that group; its other invariants are."""
    lanes = gc.opt_ref_lanes(order, pattern, mode)
    if (order, pattern, mode) == (5, "alt16", "fixed_total"):
        sp = sorted(gc.opt_ref_spread(order, pattern, mode, b) for b in range(gc.B))
        with capsys.disabled():
            print("\no5 alt16 fixed_total: the reference's own objective moves by %.1e (smallest) .. %.1e (median) .. %.1e" % (sp[0], sp[gc.B // 2], sp[-1]))
        assert lanes == () and sp[0] > 0.1 * gc.OPT_REF_TOL[order], (lanes, sp[0])
    else:
        assert lanes == (0, 1, 2, 3), lanes


@pytest.mark.parametrize("mode", gc.OPT_MODES)
@pytest.mark.parametrize("pattern", gc.OPT_PATTERNS)
@pytest.mark.parametrize("order", gc.ORDERS)
def test_numpy_cost_can_judge_the_optimisers_objective(order, pattern, mode):
    """_invariants holds the kernel's final objective to timeopt_ref.cost_grad's J at the returned times (1e-8; 1e-6 at order
    5).  At the times the reference optimiser ends on, that numpy J is within a tenth of the bound of the 40-digit J on
    every trajectory -- otherwise the seed moves (grad_spread_cases.OPT_RESEED)."""
    assert gc.opt_yardstick_error(order, pattern, mode) <= 0.1 * gc.OPT_J_TOL[order]


# ------------------------------------------------------------------------------------------------ the kernels' own math


@pytest.mark.parametrize("order", [2, 3, 4])
def test_positions_as_the_kernels_take_them_cost_the_digits_on_dist256(order, capsys):
    """The reference in Python floats with the waypoints entering the products Qt d as they are ("none": the four-product
    form ep0 P_k + ep1 P_k+1 + sp0 P_k+1 + sp1 P_k+2) or from the first waypoint ("first") instead of from each
    segment's start.  On dist256 (legs of 0.3 to 80 m on a path hundreds of metres from its start) that alone costs the
    digits: at S = 16 the time gradients lose at least 10 x against the careful form.  It is why the reverse-mode and
    the cost kernel form their right-hand sides from the legs."""
    c = gc.Case("open", "dist256", order, 16)
    cpu = gc.open_cpu64(c)
    first, asis = (gc.open_errors(c, gc.adjoint_source(c, None, origin)) for origin in ("first", "none"))
    worst, worst_asis = {}, {}
    for k in cpu:
        gc._worst(worst, k[1], first[k] / max(cpu[k], 1e-300))
        gc._worst(worst_asis, k[1], asis[k] / max(cpu[k], 1e-300))
    with capsys.disabled():
        print("\ndist256 o%d S 16, from the first waypoint / e_cpu64: dJdT %.0f dJdT_T %.0f J %.0f;  with the waypoints as they "
              "are / e_cpu64: times %.0f times_T %.0f waypoints %.0f"
              % (order, worst["dJdT"], worst["dJdT_T"], worst["J"], worst_asis["times"], worst_asis["times_T"], worst_asis["waypoints"]))
    assert worst["dJdT"] >= 10.0 and worst_asis["times"] >= 10.0, (worst, worst_asis)


@pytest.mark.parametrize("order", gc.ORDERS)
def test_the_free_derivative_loop_system_costs_the_digits(order, capsys):
    """e_same of the loops -- the free-derivative system the periodic kernels solve, in numpy fp64
    (tests/periodic_vjp_ref.py) -- against e_cpu64, the KKT system in the coefficients.  At orders 3 and 5, where the
    GPU test gates the kernel by a measured ratio, e_same is at least 10 x e_cpu64 on the worst case, so the loss is the
    formulation's.  Up to order 4 e_same stays within 1e-7 on every case (the GPU test then asserts the 1e-6 north
    star); at order 5 it does not (every pattern has a case above), and the north star is not asserted there."""
    worst_ratio, above = 0.0, {}
    for pattern in gc.R16:
        for c in gc.periodic_cases(order, pattern):
            cpu, same = gc.loop_cpu64(c), gc.loop_same_math(c)
            worst_ratio = max([worst_ratio] + [same[k] / max(cpu[k], 1e-300) for k in cpu if same[k] > 1e-13])
            above[pattern] = max(above.get(pattern, 0.0), max(same.values()))
            if order <= 4:
                assert max(same.values()) <= gc.ABSOLUTE_AT, (c.id, max(same.values()))
    with capsys.disabled():
        print("\nperiodic o%d: worst e_same / e_cpu64 %.0f; worst e_same per pattern %s" % (order, worst_ratio, {k: "%.1e" % v for k, v in above.items()}))
    if order in (3, 5):
        assert worst_ratio >= 10.0, worst_ratio
    if order == 5:
        assert all(v > gc.ABSOLUTE_AT for v in above.values()), above
