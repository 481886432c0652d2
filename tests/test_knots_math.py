"""CPU tests of the per-knot constraint solve (csp_minsnap_solve_knots_batch): the reference
tests/knots_ref.py against tests/spread_ref.py and against the natural boundary conditions of the QP, the count rule,
the C-ABI's argument checks (every one of them comes back with no device present) and the binding."""
import ctypes

import numpy as np
import pytest

from tests import knots_ref, spread_ref, synth

OK, INVALID_ARG, UNSUPPORTED, WORKSPACE, NO_DEVICE = 0, -1, -2, -3, -5
ORDERS = (2, 3, 4, 5)
SEGMENTS = (1, 2, 3, 5, 16)
# 40-digit arithmetic on systems of condition <= 1e12 (order 5, T in [0.5, 2]): identities hold to 1e-28 of their terms
MP_GATE = 1e-25


def _traj(rng, S):
    return np.cumsum(rng.normal(size=(S + 1, 3)) * 5, 0), rng.uniform(0.5, 2.0, S)


@pytest.mark.parametrize("order", ORDERS)
def test_standard_mask_is_the_open_chain_solve(order):
    """With the ends fully pinned from bc and the interior free the problem is spread_ref.solve's: at 40 digits the two
    references (assembled band system here, block recursion there) round to the same doubles.  Measured: 0.0."""
    rng = np.random.default_rng(100 + order)
    for S in SEGMENTS:
        path, time = _traj(rng, S)
        bc = rng.normal(size=(4, 3))
        w = 0.3 if S % 2 else 0.0
        mask, values = knots_ref.standard_problem(order, S, bc)
        got = knots_ref.solve(order, path, time, mask, values, vel_zero_weight=w)
        ref = spread_ref.solve(order, path, time, bc, vel_zero_weight=w)
        assert synth.rel_err_per_power(got.coeffs, ref) <= 1e-15, (order, S)


def _deriv_at(c, d, t, mp, span):
    """d-th derivative at t of the polynomial with coefficients c (highest power first, mpmath numbers): (value, the sum
    of its terms' magnitudes at t = span -- the size the derivative has over the segment, also where t = 0 leaves one
    term)."""
    m = len(c)
    v, scale = mp.mpf(0), mp.mpf(0)
    for i, ci in enumerate(c):
        pw = m - 1 - i
        if pw < d:
            continue
        f = 1
        for q in range(d):
            f *= pw - q
        v += ci * f * (t ** (pw - d) if pw > d else 1)
        scale += abs(ci * f * span ** (pw - d))
    return v, scale


@pytest.mark.parametrize("order", ORDERS)
def test_natural_boundary_conditions(order):
    """What the minimiser must satisfy where nothing is pinned (vel_zero_weight = 0), checked on the 40-digit
    coefficients: a free derivative r at an end knot makes p^(2o-1-r) vanish there; at an interior knot derivative
    2o-1-r is continuous when r is free (so a fully free knot is C^(2o-2)) and only a pinned r lets it jump; a pinned
    derivative takes its value on both sides."""
    import mpmath as mp
    o, n = order, order - 1
    rng = np.random.default_rng(200 + order)
    S = 5
    path, time = _traj(rng, S)
    values = rng.normal(size=(S + 1, n, 3))
    full = (1 << n) - 1
    mask = np.zeros(S + 1, dtype=np.uint8)
    mask[0] = 1                     # start: velocity pinned, the rest free
    mask[S] = 0                     # free end
    mask[2] = full & 0b10 or 1      # acceleration alone where there is one, else velocity
    mask[3] = full                  # everything pinned
    sol = knots_ref.solve(o, path, time, mask, values, raw=True)
    with mp.workdps(40):
        T = [mp.mpf(float(t)) for t in time]
        for ax in range(3):
            seg = lambda j: sol.coeffs[j][ax]
            for r in range(1, o):
                d = 2 * o - 1 - r
                for k, (j, t) in ((0, (0, mp.mpf(0))), (S, (S - 1, T[S - 1]))):
                    v, scale = _deriv_at(seg(j), d, t, mp, T[j])
                    if not (mask[k] >> (r - 1)) & 1:
                        assert abs(v) <= MP_GATE * scale, ("end", o, k, r, ax)
                for k in range(1, S):
                    pinned = (mask[k] >> (r - 1)) & 1
                    left, sl = _deriv_at(seg(k - 1), d, T[k - 1], mp, T[k - 1])
                    right, sr = _deriv_at(seg(k), d, mp.mpf(0), mp, T[k])
                    if not pinned:
                        assert abs(left - right) <= MP_GATE * (sl + sr), ("interior", o, k, r, ax)
                    else:
                        want = mp.mpf(float(values[k, r - 1, ax]))
                        for got, sc in (_deriv_at(seg(k - 1), r, T[k - 1], mp, T[k - 1]), _deriv_at(seg(k), r, mp.mpf(0), mp, T[k])):
                            assert abs(got - want) <= MP_GATE * (sc + abs(want)), ("pinned", o, k, r, ax)
    # the pinned knot 3 really separates: derivative 2o-2 (r = 1) jumps there for a generic input
    with mp.workdps(40):
        left, _ = _deriv_at(sol.coeffs[2][0], 2 * o - 2, mp.mpf(float(time[2])), mp, mp.mpf(1))
        right, sc = _deriv_at(sol.coeffs[3][0], 2 * o - 2, mp.mpf(0), mp, mp.mpf(float(time[3])))
        assert abs(left - right) > 1e-6 * sc


def test_count_rule():
    """Order 4, both ends free: S = 1 and 2 have 2 and 3 constraints and no unique minimiser; S = 3 has 4, the cubic
    through the four points costs nothing and is the minimiser: its coefficients of t^7 .. t^4 vanish."""
    rng = np.random.default_rng(7)
    for S in (1, 2):
        path, time = _traj(rng, S)
        assert knots_ref.constraint_count(4, np.zeros(S + 1, np.uint8)) == S + 1
        with pytest.raises(knots_ref.Underdetermined):
            knots_ref.solve(4, path, time, np.zeros(S + 1, np.uint8), np.zeros((S + 1, 3, 3)))
    # bits from order-1 upward do not count
    assert knots_ref.constraint_count(4, np.full(3, 0xF8, np.uint8)) == 3
    path, time = _traj(rng, 3)
    sol = knots_ref.solve(4, path, time, np.zeros(4, np.uint8), np.full((4, 3, 3), np.nan))
    scale = np.abs(path).max()
    assert np.abs(sol.coeffs[:, :, :4]).max() <= 1e-30 * scale
    assert abs(sol.cost) <= 1e-30 * scale ** 2
    # and it is the interpolating cubic: one polynomial, re-expanded per segment
    t_knots = np.concatenate([[0.0], np.cumsum(time)])
    for ax in range(3):
        cubic = np.polyfit(t_knots, path[:, ax], 3)
        for j in range(3):
            shifted = np.poly1d(cubic)(np.poly1d([1.0, t_knots[j]])).coeffs
            assert np.allclose(sol.coeffs[j, ax, 4:], shifted, rtol=1e-9, atol=1e-9 * scale)


def test_unit_table_times_factorial_is_integral():
    """M(1)^-1 (o-1)! is a table of integers: what lets the kernel's coefficient recovery sum exact products."""
    import math
    import mpmath as mp
    for order in ORDERS:
        G, _ = spread_ref.unit_tables(order)
        with mp.workdps(50):
            assert all(v * math.factorial(order - 1) == mp.nint(v * math.factorial(order - 1)) for row in G for v in row), order
            assert max(abs(v) for row in G for v in row) * math.factorial(order - 1) < 2 ** 20


@pytest.mark.parametrize("order", (4, 5))
def test_plain_fp64_recovery_misses_its_own_end_derivatives(order):
    """Why the kernel recovers its coefficients in double-double arithmetic.  From the 40-digit knot derivatives of a
    trajectory whose end velocity and acceleration are pinned, the last segment's coefficients are recovered the
    plain way, c = diag(T^-p) G diag(T^a) d in fp64, and the pinned derivatives are evaluated at t = T in exact rational
    arithmetic: they miss the pinned values by several times gamma(2M + 2) A, the whole rounding budget eval_batch has
    for given coefficients, because the sums G d cancel.  The correctly rounded coefficients
    of the same interpolant stay inside that budget.  Measured here: 3.7 (order 4) and 18.8 (order 5) times the gate
    for the plain recovery, 0.02 for the correctly rounded coefficients; 17 and 22 on the GPU tests' inputs."""
    from fractions import Fraction as F
    from tests import eval_ref
    o, M, S = order, 2 * order, 16
    G = [[float(v) for v in row] for row in spread_ref.unit_tables(o)[0]]
    rng = np.random.default_rng(300 + order)
    plain = exact = 0.0
    for _ in range(3):
        path, time = _traj(rng, S)
        mask, values = knots_ref.standard_problem(o, S, rng.normal(size=(4, 3)))
        mask[S // 2] |= 1
        values[S // 2] = rng.normal(size=(o - 1, 3))
        sol = knots_ref.solve(o, path, time, mask, values)
        T = float(time[S - 1])
        for ax in range(3):
            d = [0.0] * M
            d[o] = path[S, ax] - path[S - 1, ax]
            for r in range(1, o):
                d[r], d[o + r] = sol.x[S - 1, r - 1, ax], sol.x[S, r - 1, ax]
            dh = [d[a] * T ** (a % o) for a in range(M)]
            c = [sum(G[i][a] * dh[a] for a in range(1, M)) * (1.0 / T) ** (M - 1 - i) for i in range(M - 1)] + [0.0]
            good = list(sol.coeffs[S - 1, ax, :M - 1]) + [0.0]         # the segment's start as origin, as above
            for coeffs, which in ((c, "plain"), (good, "exact")):
                for dd in range(1, o):
                    if not (mask[S] >> (dd - 1)) & 1:
                        continue
                    val, A = F(0), 0.0
                    for i, ci in enumerate(coeffs):
                        p = M - 1 - i
                        if p >= dd:
                            term = F(float(ci)) * int(np.prod(np.arange(p, p - dd, -1))) * F(T) ** (p - dd)
                            val, A = val + term, A + abs(float(term))
                    ratio = abs(float(val - F(float(values[S, dd - 1, ax])))) / (eval_ref.gamma(2 * M + 2) * A)
                    if which == "plain":
                        plain = max(plain, ratio)
                    else:
                        exact = max(exact, ratio)
    print("order %d: error / gate at t = T, plain fp64 recovery %.1f, correctly rounded coefficients %.2f" % (order, plain, exact))
    assert plain > 1.0 and exact <= 1.0


def test_fp64_run_of_the_reference_is_close():
    """dps=None is the same code in Python floats (e_cpu64): it must be a sane fp64 solve, not a second algorithm."""
    rng = np.random.default_rng(11)
    for order, gate in ((2, 1e-13), (3, 1e-11), (4, 1e-9), (5, 1e-6)):
        path, time = _traj(rng, 6)
        n = order - 1
        mask = rng.integers(0, 1 << n, size=7).astype(np.uint8)
        values = rng.normal(size=(7, n, 3))
        hi = knots_ref.solve(order, path, time, mask, values)
        lo = knots_ref.solve(order, path, time, mask, values, dps=None)
        assert synth.rel_err_per_power(lo.coeffs, hi.coeffs) <= gate, order
        assert abs(lo.cost - hi.cost) <= gate * abs(hi.cost)


# ---------------------------------------------------------------------------------------------------- the C-ABI surface

def test_symbols_exported(csp):
    for name in ("csp_minsnap_solve_knots_batch", "csp_minsnap_knots_workspace_bytes"):
        assert name in csp.EXPORTED_SYMBOLS
        assert getattr(ctypes.CDLL(csp.LIB_PATH), name)
    assert callable(csp.solve_knots_batch) and callable(csp.knots_workspace_bytes) and callable(csp.knots_from_bc)


def _p(a):
    return None if a is None else (a if isinstance(a, int) else a.ctypes.data)


def _call(csp, desc, wp, tm, mk, kv, co, cost=None, status=None, ws=None, ws_bytes=0):
    return csp.raw_lib().csp_minsnap_solve_knots_batch(ctypes.byref(desc), _p(wp), _p(tm), _p(mk), _p(kv), _p(co), _p(cost),
                                                       _p(status), _p(ws), ws_bytes, None)


def test_workspace_bytes_formula(csp):
    up = lambda v: (v + 255) // 256 * 256
    for order in ORDERS:
        n = order - 1
        for B, S in ((1, 1), (65, 17), (7, 300)):
            want = up((S + 1) * (n * n + 3 * n) * B * 8)
            assert csp.knots_workspace_bytes(csp.make_desc(order, B, S)) == want
            off = np.zeros(B + 1, dtype=np.int64)
            assert csp.knots_workspace_bytes(csp.make_desc(order, B, 0, seg_offsets_ptr=off.ctypes.data, max_segments=S)) == want
            assert csp.knots_workspace_bytes(csp.make_desc(order, B, S, dtype=csp.DTYPE_F32)) == want
    for bad in (csp.make_desc(1, 4, 3), csp.make_desc(6, 4, 3), csp.make_desc(4, 4, 3, path_weight=0.5),
                csp.make_desc(4, 4, 3, flags=csp.FLAG_SEGMENT_MAJOR),
                csp.make_desc(4, 4, 3, dtype=csp.DTYPE_F32, flags=csp.FLAG_F32_ARITH)):
        assert csp.knots_workspace_bytes(bad) == 0


def test_every_return_code_comes_back_without_a_device(csp):
    B, S, order = 4, 3, 4
    n = order - 1
    wp, tm = np.zeros((B, S + 1, 3)), np.ones((B, S))
    mk, kv = np.zeros((B, S + 1), np.uint8), np.zeros((B, S + 1, n, 3))
    co = np.zeros((B, S, 3, 2 * order))
    call = lambda d: _call(csp, d, wp, tm, mk, kv, co)
    unsupported = {"order 1": csp.make_desc(1, B, S),
                   "order 6": csp.make_desc(6, B, S),
                   "path penalty": csp.make_desc(order, B, S, path_weight=0.5),
                   "segment major": csp.make_desc(order, B, S, flags=csp.FLAG_SEGMENT_MAJOR),
                   "f32 arithmetic": csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, flags=csp.FLAG_F32_ARITH)}
    for name, d in unsupported.items():
        assert call(d) == UNSUPPORTED, name
    host = csp.make_desc(order, B, S)
    bad = csp.make_desc(order, B, S)
    bad.abi_version = 99
    assert call(bad) == INVALID_ARG
    assert call(csp.make_desc(order, B, S, vel_zero_weight=-1.0)) == INVALID_ARG
    # null required pointers
    assert _call(csp, host, None, tm, mk, kv, co) == INVALID_ARG
    assert _call(csp, host, wp, None, mk, kv, co) == INVALID_ARG
    assert _call(csp, host, wp, tm, None, kv, co) == INVALID_ARG
    assert _call(csp, host, wp, tm, mk, None, co) == INVALID_ARG
    assert _call(csp, host, wp, tm, mk, kv, None) == INVALID_ARG
    # ragged host call: offsets outside 0..max_segments
    off = np.array([0, 3, 2, 8, 12], dtype=np.int64)
    rag = csp.make_desc(order, B, 0, seg_offsets_ptr=off.ctypes.data, max_segments=6)
    assert _call(csp, rag, np.zeros((16, 3)), np.ones(12), np.zeros(16, np.uint8), np.zeros((16, n, 3)),
                 np.zeros((12, 3, 2 * order))) == INVALID_ARG
    # device-memory form: workspace size and alignment and the coefficients' alignment, from the pointers' values alone
    dev = csp.make_desc(order, B, S, mem_space=csp.MEM_DEVICE)
    dev32 = csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, mem_space=csp.MEM_DEVICE)
    need = csp.knots_workspace_bytes(dev)
    assert _call(csp, dev, 4096, 4096, 4096, 4096, 4096, ws=None, ws_bytes=0) == WORKSPACE
    assert _call(csp, dev, 4096, 4096, 4096, 4096, 4096, ws=8192, ws_bytes=need - 1) == WORKSPACE
    assert _call(csp, dev, 4096, 4096, 4096, 4096, 4096, ws=8196, ws_bytes=need) == WORKSPACE       # not 8-byte aligned
    assert _call(csp, dev, 4096, 4096, 4096, 4096, 4104, ws=8192, ws_bytes=need) == INVALID_ARG     # coeffs: 16 bytes
    assert _call(csp, dev32, 4096, 4096, 4096, 4096, 4100, ws=8192, ws_bytes=need) == INVALID_ARG   # fp32: 8 bytes
    # nothing to do: CSP_OK, with or without a device
    assert _call(csp, csp.make_desc(order, 0, S), None, None, None, None, None) == OK
    if csp.device_count() == 0:   # everything in order: only now is a device looked for
        assert call(host) == NO_DEVICE
        assert _call(csp, dev, 4096, 4096, 4096, 4096, 4096, ws=8192, ws_bytes=need) == NO_DEVICE
        assert _call(csp, dev32, 4096, 4096, 4096, 4096, 4104, ws=8192, ws_bytes=need) == NO_DEVICE
        with pytest.raises(csp.CspError) as e:
            csp.solve_knots_batch(wp, tm, mk, kv, order=order)
        assert e.value.code == NO_DEVICE


# ------------------------------------------------------------------------------------------------------------ the binding

def test_knots_from_bc(csp):
    rng = np.random.default_rng(5)
    for order in ORDERS:
        n = order - 1
        for S in (1, 4):
            bc = rng.normal(size=(3, 4, 3))
            mask, values = csp.knots_from_bc(bc, S, order)
            assert mask.shape == (3, S + 1) and mask.dtype == np.uint8
            assert values.shape == (3, S + 1, n, 3) and values.dtype == np.float64
            for b in range(3):
                rm, rv = knots_ref.standard_problem(order, S, bc[b])
                assert np.array_equal(mask[b], rm) and np.array_equal(values[b], rv)
            # a shared bc repeated over a batch; None is the zero bc; fp32 stays fp32
            m1, v1 = csp.knots_from_bc(bc[0], S, order, batch=5)
            assert m1.shape == (5, S + 1) and all(np.array_equal(v1[b], values[0]) for b in range(5))
            m0, v0 = csp.knots_from_bc(None, S, order, batch=2)
            assert np.array_equal(m0, mask[:2]) and not v0.any()
            assert csp.knots_from_bc(bc.astype(np.float32), S, order)[1].dtype == np.float32
    with pytest.raises(ValueError):
        csp.knots_from_bc(np.zeros((3, 4, 3)), 4, 4, batch=2)
    with pytest.raises(ValueError):
        csp.knots_from_bc(None, 4, 1)


def test_numpy_and_torch_inputs_take_one_path(csp):
    """Both kinds of input go through _mem / _CallInputs: what is wrong with the arrays is found there, before the
    library is called, with the same message; a torch CPU tensor is refused by the device backend as everywhere."""
    import torch
    B, S, order = 3, 4, 3
    wp, tm = np.zeros((B, S + 1, 3)), np.ones((B, S))
    mask, values = csp.knots_from_bc(None, S, order, batch=B)
    with pytest.raises(ValueError, match="knot_mask must hold 15 elements"):
        csp.solve_knots_batch(wp, tm, mask[:, :-1], values, order=order)
    with pytest.raises(ValueError, match="knot_values must hold 90 elements"):
        csp.solve_knots_batch(wp, tm, mask, values[:, :, :1], order=order)
    with pytest.raises(ValueError, match="CUDA tensors"):
        csp.solve_knots_batch(torch.from_numpy(wp), torch.from_numpy(tm), torch.from_numpy(mask), torch.from_numpy(values),
                              order=order)
    # a mask given as a list or as another integer type is converted by the same contig() as every other input
    if csp.device_count() == 0:
        with pytest.raises(csp.CspError) as e:
            csp.solve_knots_batch(wp, tm, mask.astype(np.int64).tolist(), values.astype(np.float32), order=order)
        assert e.value.code == NO_DEVICE
