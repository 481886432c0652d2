"""The evaluation entries without a device: the exact reference of tests/eval_ref.py against numpy and against an
independent fractions.Fraction evaluation, the adjoint identity of the reference's reverse mode in exact rationals, and
the C-ABI surface of csp_minsnap_eval_batch / csp_minsnap_eval_batch_vjp (symbols and every return code of the scope
list, all of which come back before a device is looked for)."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from tests import eval_ref

OK, INVALID_ARG, UNSUPPORTED, NO_DEVICE = 0, -1, -2, -5


def _dyadic(rng, shape, lo, hi, bits=6):
    """Multiples of 2**-bits in [lo, hi]: few enough bits that fp64 polynomial evaluation is exact."""
    return rng.integers(int(lo * 2 ** bits), int(hi * 2 ** bits) + 1, size=shape) / 2.0 ** bits


def _case(rng, order, B=3, S=4, Q=9):
    M = 2 * order
    times = _dyadic(rng, (B, S), 0.25, 2.0, bits=2)
    times[0, 1] = 0.0                                     # a zero-length segment
    coeffs = _dyadic(rng, (B, S, 3, M), -2.0, 2.0, bits=3)
    cum = np.concatenate([np.zeros((B, 1)), np.cumsum(times, axis=1)], axis=1)
    query = _dyadic(rng, (B, Q), 0.0, 1.0, bits=3) * cum[:, -1:]
    query = np.round(query * 8) / 8
    query[:, 0] = -0.5                                    # clamped low
    query[:, 1] = cum[:, -1] + 0.25                       # clamped high
    query[:, 2] = cum[:, 2]                               # on a knot
    query[:, 3] = cum[:, -1]                              # the end: in range
    query[:, 4] = 0.0
    return times, coeffs, query


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_reference_agrees_with_numpy_on_dyadic_inputs(order):
    """Small dyadic inputs: numpy.polyval of numpy.polyder is exact in fp64, and so must equal the reference."""
    rng = np.random.default_rng(order)
    times, coeffs, query = _case(rng, order)
    ref = eval_ref.Ref(times, coeffs, query, 5)
    exact, A = ref.values(5)
    got = exact.floats()
    for b in range(times.shape[0]):
        for q in range(query.shape[1]):
            j, tau = ref.seg[b, q], ref.tau[b, q]
            for d in range(5):
                for a in range(3):
                    p = np.polyder(coeffs[b, j, a], d) if d else coeffs[b, j, a]
                    want = np.polyval(p, tau) if np.size(p) else 0.0
                    assert got[b, q, d, a] == want, (b, q, d, a)
    assert np.all(exact.abs_err(got) == 0.0)
    assert np.all(A >= np.abs(got))
    # rule 3: a knot belongs to the later segment, zero-length segments are skipped, the end belongs to the last one
    assert np.all(ref.seg[:, 0] == 0) and np.all(ref.seg[:, 1] == times.shape[1] - 1)
    assert ref.seg[0, 2] == 2 and np.all(ref.tau[:, 2] == 0.0)
    assert np.all(ref.seg[:, 3] == times.shape[1] - 1) and np.all(ref.seg[:, 4] == 0)
    assert not ref.high[:, 3].any() and ref.high[:, 1].all() and ref.low[:, 0].all()


def test_dyadic_arithmetic_is_fraction_arithmetic():
    rng = np.random.default_rng(7)
    x, y, z = rng.standard_normal((3, 5, 4)) * np.array([1e-9, 1.0, 1e7])[:, None, None]
    got = ((eval_ref.Dy.of(x) * eval_ref.Dy.of(y) + eval_ref.Dy.of(z)) * 6 - eval_ref.Dy.of(x)).fractions()
    for i in np.ndindex(x.shape):
        assert got[i] == (Fraction(x[i]) * Fraction(y[i]) + Fraction(z[i])) * 6 - Fraction(x[i])
    d = eval_ref.Dy.of(x) * eval_ref.Dy.of(y)
    assert np.all(d.abs_err(d.floats()) <= np.abs(x * y) * 2.0 ** -52)


def _poly_deriv(c, d):
    """Coefficients (Fractions, highest power first) of the d-th derivative."""
    c = list(c)
    for _ in range(d):
        n = len(c) - 1
        c = [ck * (n - k) for k, ck in enumerate(c[:-1])]
    return c


def _poly_at(c, x):
    r = Fraction(0)
    for ck in c:
        r = r * x + ck
    return r


@pytest.mark.parametrize("order,D", [(2, 5), (3, 3), (4, 4), (5, 1), (5, 5)])
def test_reference_vjp_is_the_adjoint_of_the_exact_jvp(order, D):
    """<g, J v> = <J^T g, v> in exact rationals, with J v from polynomial differentiation in c, T and t: clamped,
    on-knot and end-of-trajectory queries included."""
    rng = np.random.default_rng(100 * order + D)
    times, coeffs, query = _case(rng, order)
    B, S = times.shape
    Q = query.shape[1]
    g = rng.standard_normal((B, Q, D, 3))
    vc, vT, vt = rng.standard_normal(coeffs.shape), rng.standard_normal(times.shape), rng.standard_normal(query.shape)
    ref = eval_ref.Ref(times, coeffs, query, D)
    r = ref.vjp(g)
    rhs = sum((r[k][0].fractions() * np.vectorize(Fraction, otypes=[object])(v)).sum()
              for k, v in (("coeffs", vc), ("times", vT), ("query", vt)))
    lhs = Fraction(0)
    F = lambda a: [Fraction(float(v)) for v in a]
    for b in range(B):
        for q in range(Q):
            j, tau = int(ref.seg[b, q]), Fraction(float(ref.tau[b, q]))
            if ref.low[b, q]:
                dtau = Fraction(0)
            elif ref.high[b, q]:
                dtau = Fraction(float(vT[b, S - 1]))
            else:
                dtau = Fraction(float(vt[b, q])) - sum(F(vT[b, :j]), Fraction(0))
            for a in range(3):
                c, dc = F(coeffs[b, j, a]), F(vc[b, j, a])
                for d in range(D):
                    jv = _poly_at(_poly_deriv(dc, d), tau) + _poly_at(_poly_deriv(c, d + 1), tau) * dtau
                    lhs += Fraction(float(g[b, q, d, a])) * jv
    assert lhs == rhs
    # the count of queries per segment is what the grad_coeffs gate is built from
    assert r["count"].sum() == B * Q


def test_reference_ignores_nonfinite_queries():
    rng = np.random.default_rng(3)
    times, coeffs, query = _case(rng, 3)
    g = rng.standard_normal(query.shape + (2, 3))
    base = eval_ref.Ref(times, coeffs, query, 2).vjp(g)
    q2, g2 = np.concatenate([query, np.full((3, 1), np.nan)], axis=1), np.concatenate([g, g[:, :1]], axis=1)
    ref = eval_ref.Ref(times, coeffs, q2, 2)
    more = ref.vjp(g2)
    assert np.all(ref.seg[:, -1] == -1)
    for k in ("coeffs", "times"):
        assert np.all((more[k][0] - base[k][0]).n == 0)
    assert np.all(more["count"] == base["count"])


# ---------------------------------------------------------------------------------------------------- the C-ABI surface

def test_symbols_exported(csp):
    for name in ("csp_minsnap_eval_batch", "csp_minsnap_eval_batch_vjp"):
        assert name in csp.EXPORTED_SYMBOLS
        assert getattr(ctypes.CDLL(csp.LIB_PATH), name)
    assert callable(csp.eval_batch) and callable(csp.eval_batch_vjp) and callable(csp.eval_batch_autograd)


def _p(a):
    return None if a is None else (a if isinstance(a, int) else a.ctypes.data)


def _fwd(csp, desc, tm, co, qr, Q, D, out):
    return csp.raw_lib().csp_minsnap_eval_batch(ctypes.byref(desc), _p(tm), _p(co), _p(qr), Q, D, _p(out), None, None, None)


def _vjp(csp, desc, tm, co, qr, Q, D, go, gc, gt, gq):
    return csp.raw_lib().csp_minsnap_eval_batch_vjp(ctypes.byref(desc), _p(tm), _p(co), _p(qr), Q, D, _p(go), _p(gc), _p(gt),
                                                    _p(gq), None, None)


def test_every_return_code_comes_back_without_a_device(csp):
    B, S, order, Q, D = 4, 3, 4, 5, 3
    tm, co, qr = np.ones((B, S)), np.zeros((B, S, 3, 2 * order)), np.zeros((B, Q))
    out, go = np.zeros((B, Q, D, 3)), np.zeros((B, Q, D, 3))
    gc, gt, gq = np.zeros_like(co), np.zeros_like(tm), np.zeros_like(qr)
    both = lambda d, Q=Q, D=D: (_fwd(csp, d, tm, co, qr, Q, D, out), _vjp(csp, d, tm, co, qr, Q, D, go, gc, gt, gq))
    unsupported = {"order 1": csp.make_desc(1, B, S),
                   "order 6": csp.make_desc(6, B, S),
                   "S > 1024": csp.make_desc(order, B, 1025),
                   "ragged max_segments > 1024": csp.make_desc(order, B, 0, seg_offsets_ptr=qr.ctypes.data, max_segments=1025),
                   "segment major": csp.make_desc(order, B, S, flags=csp.FLAG_SEGMENT_MAJOR),
                   "f32 arithmetic": csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, flags=csp.FLAG_F32_ARITH)}
    for name, d in unsupported.items():
        assert both(d) == (UNSUPPORTED, UNSUPPORTED), name
    host = csp.make_desc(order, B, S)
    for D_bad in (0, 6, -1):
        assert both(host, D=D_bad) == (INVALID_ARG, INVALID_ARG), D_bad
    assert both(host, Q=-1) == (INVALID_ARG, INVALID_ARG)
    bad = csp.make_desc(order, B, S)
    bad.abi_version = 99
    assert both(bad) == (INVALID_ARG, INVALID_ARG)
    # null required pointers
    assert _fwd(csp, host, None, co, qr, Q, D, out) == INVALID_ARG
    assert _fwd(csp, host, tm, None, qr, Q, D, out) == INVALID_ARG
    assert _fwd(csp, host, tm, co, None, Q, D, out) == INVALID_ARG
    assert _fwd(csp, host, tm, co, qr, Q, D, None) == INVALID_ARG
    assert _vjp(csp, host, None, co, qr, Q, D, go, gc, gt, gq) == INVALID_ARG
    assert _vjp(csp, host, tm, None, qr, Q, D, go, gc, gt, gq) == INVALID_ARG
    assert _vjp(csp, host, tm, co, None, Q, D, go, gc, gt, gq) == INVALID_ARG
    assert _vjp(csp, host, tm, co, qr, Q, D, None, gc, gt, gq) == INVALID_ARG
    assert _vjp(csp, host, tm, co, qr, Q, D, go, None, None, None) == INVALID_ARG      # all three outputs null
    # ragged host call: offsets outside 0..max_segments
    off = np.array([0, 3, 2, 8, 12], dtype=np.int64)
    rag = csp.make_desc(order, B, 0, seg_offsets_ptr=off.ctypes.data, max_segments=6)
    t12, c12 = np.ones(12), np.zeros((12, 3, 2 * order))
    assert _fwd(csp, rag, t12, c12, qr, Q, D, out) == INVALID_ARG
    assert _vjp(csp, rag, t12, c12, qr, Q, D, go, np.zeros_like(c12), None, None) == INVALID_ARG
    # device-memory form: alignment is checked from the pointers' values alone
    dev = csp.make_desc(order, B, S, mem_space=csp.MEM_DEVICE)
    dev32 = csp.make_desc(order, B, S, dtype=csp.DTYPE_F32, mem_space=csp.MEM_DEVICE)
    assert _fwd(csp, dev, 4096, 4104, 4096, Q, D, 4096) == INVALID_ARG                  # coeffs not 16-byte aligned
    assert _fwd(csp, dev32, 4096, 4100, 4096, Q, D, 4096) == INVALID_ARG                # fp32: 8-byte aligned
    assert _vjp(csp, dev, 4096, 4104, 4096, Q, D, 4096, 4096, None, None) == INVALID_ARG
    assert _vjp(csp, dev, 4096, 4096, 4096, Q, D, 4096, 4104, None, None) == INVALID_ARG  # the cotangent's alignment
    assert _vjp(csp, dev32, 4096, 4096, 4096, Q, D, 4096, 4100, None, None) == INVALID_ARG
    # nothing to do: CSP_OK, with or without a device
    assert _fwd(csp, csp.make_desc(order, 0, S), None, None, None, Q, D, None) == OK
    assert _vjp(csp, csp.make_desc(order, 0, S), None, None, None, Q, D, None, None, None, 4096) == OK
    assert _fwd(csp, host, tm, co, None, 0, D, None) == OK
    if csp.device_count() == 0:   # everything in order: only now is a device looked for
        assert both(host) == (NO_DEVICE, NO_DEVICE)
        assert _fwd(csp, dev32, 4096, 4104, 4096, Q, D, 4096) == NO_DEVICE
        assert _vjp(csp, host, tm, co, None, 0, D, None, gc, gt, None) == NO_DEVICE      # Q = 0 still writes zeros
        with pytest.raises(csp.CspError) as e:
            csp.eval_batch(tm, co, qr)
        assert e.value.code == NO_DEVICE
        with pytest.raises(csp.CspError) as e:
            csp.eval_batch_vjp(tm, co, qr, go)
        assert e.value.code == NO_DEVICE
