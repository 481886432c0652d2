"""csp_minsnap_eval_batch / csp_minsnap_eval_batch_vjp on the GPU against the exact reference of tests/eval_ref.py.

Gates are the running-error bound gamma(n) * A of the contract (A: the sum of the absolute values of all products that
enter the output, from the reference; n: the roundings on the longest path to it), plus 2**-24 |exact| for the output
rounding of fp32 storage:

    values       n = 2M + 2
    grad_coeffs  n = M + 2 + D * Q_j   (Q_j queries in segment j)
    grad_query   n = 2M + 3 + 3D
    grad_times   n = 2M + 3 + 3D + Q + S

The kernel's scheme (minsnap_eval.hip) stays inside these counts: a power costs at most M - 2 roundings, a term two more,
a sum of M terms M - 1; g_tau adds one product and 3D - 1 additions; a record accumulates D Q_j terms of M roundings each;
grad_times adds at most Q additions per segment sum and S in the suffix sum.  Every test prints its worst ratio to the
gate before it asserts.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import eval_ref, guarded, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NP = {"f64": np.float64, "f32": np.float32}
NONFINITE = 1


def _inputs(seed, B, S, Q, order, dtype, D=5):
    """Random normal coefficients and cotangents, times in [0.05, 3], queries uniform in [-0.2, sum T + 0.2], in the
    storage type."""
    rng = np.random.default_rng(seed)
    times = rng.uniform(0.05, 3.0, (B, S)).astype(NP[dtype])
    coeffs = rng.standard_normal((B, S, 3, 2 * order)).astype(NP[dtype])
    total = times.astype(np.float64).sum(axis=1, keepdims=True)
    query = rng.uniform(-0.2, total + 0.2, (B, Q)).astype(NP[dtype])
    g = rng.standard_normal((B, Q, D, 3)).astype(NP[dtype])
    return times, coeffs, query, g


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _np(t):
    return None if t is None else (t.cpu().numpy() if hasattr(t, "cpu") else t)


def _bits(a):
    a = np.ascontiguousarray(_np(a))
    return a.view(np.uint8).reshape(-1)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _gate(name, got, exact, A, n, dtype):
    """|got - exact| <= gamma(n) A (+ 2**-24 |exact| for fp32 storage); prints the worst ratio."""
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), name
    err = exact.abs_err(got)
    bound = eval_ref.gamma(n) * A
    if dtype == "f32":
        bound = bound + 2.0 ** -24 * np.abs(exact.floats())
    ratio = np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0)
    print("%s: worst error / gate = %.3f" % (name, ratio))
    assert np.all(err <= bound), (name, ratio)


def _check_all(tag, ref, g, dtype, values, seg, grads):
    """values [B,Q,D,3], seg [B,Q], grads = (coeffs, times, query) of one call against the reference."""
    D, M, S, Q = g.shape[2], ref.M, ref.S, ref.Q
    exact, A = ref.values(D)
    _gate(tag + " values", values, exact, A, 2 * M + 2, dtype)
    assert np.array_equal(seg, ref.seg), tag
    r = ref.vjp(g.astype(np.float64))
    gc, gt, gq = (np.asarray(x, np.float64) for x in grads)
    _gate(tag + " grad_coeffs", gc.reshape(r["coeffs"][1].shape), *r["coeffs"], (M + 2 + D * r["count"])[:, :, None, None], dtype)
    _gate(tag + " grad_query", gq, *r["query"], 2 * M + 3 + 3 * D, dtype)
    _gate(tag + " grad_times", gt, *r["times"], 2 * M + 3 + 3 * D + Q + S, dtype)
    clamped = ref.low | ref.high
    assert np.all(gq[clamped] == 0.0), tag
    assert np.all(gc.reshape(ref.B, S, -1)[r["count"] == 0] == 0.0), tag


def _uniform_ref(S, Q, order, dtype):
    times, coeffs, query, g = _inputs(1000 * S + 10 * Q + order, 65, S, Q, order, dtype)
    return times, coeffs, query, g, eval_ref.Ref(times, coeffs, query, 5)


# ------------------------------------------------------------------------------------------------------ accuracy, uniform

@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("order", [2, 3, 4, 5])
@pytest.mark.parametrize("Q", [1, 7, 64, 65])
@pytest.mark.parametrize("S", [1, 2, 16, 17])
def test_accuracy_uniform(csp, S, Q, order, dtype):
    """B = 65 (one full wave and a one-lane tail) for D in 1, 3, 5: forward and the three gradients against the gates,
    seg_index exact, host memory bit-equal to device memory, a `want` subset bit-equal to the full call."""
    times, coeffs, query, g5, ref = _uniform_ref(S, Q, order, dtype)
    d_t, d_c, d_q = _dev(times, coeffs, query)
    for D in (1, 3, 5):
        g = np.ascontiguousarray(g5[:, :, :D])
        d_g, = _dev(g)
        f = csp.eval_batch(d_t, d_c, d_q, num_derivs=D, want_seg_index=True, want_status=True)
        v = csp.eval_batch_vjp(d_t, d_c, d_q, d_g, want_status=True)
        assert not _np(f.status).any() and not _np(v.status).any()
        _check_all("S=%d Q=%d o=%d %s D=%d" % (S, Q, order, dtype, D), ref, g, dtype, _np(f.values), _np(f.seg_index),
                   (_np(v.coeffs), _np(v.times), _np(v.query)))
        hf = csp.eval_batch(times, coeffs, query, num_derivs=D, want_seg_index=True, want_status=True)
        hv = csp.eval_batch_vjp(times, coeffs, query, g, want_status=True)
        assert hf.values.dtype == NP[dtype] and hv.coeffs.dtype == NP[dtype]
        for a, b in ((hf.values, f.values), (hf.seg_index, f.seg_index), (hf.status, f.status), (hv.coeffs, v.coeffs),
                     (hv.times, v.times), (hv.query, v.query), (hv.status, v.status)):
            assert _same_bits(a, b), (S, Q, order, dtype, D)
        for name in ("coeffs", "times", "query"):
            one = csp.eval_batch_vjp(d_t, d_c, d_q, d_g, want=(name,))
            assert _same_bits(getattr(one, name), getattr(v, name)), (name, D)
            assert all(getattr(one, o) is None for o in ("coeffs", "times", "query") if o != name)


# ------------------------------------------------------------------------------------------------------- accuracy, ragged

def _ragged_inputs(seed, B, max_len, Q, order, dtype, D):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, B)
    lens[[0, B // 2, B - 1]] = 0
    lens[1], lens[2] = max_len, 1
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    times = rng.uniform(0.05, 3.0, off[-1]).astype(NP[dtype])
    coeffs = rng.standard_normal((off[-1], 3, 2 * order)).astype(NP[dtype])
    total = np.array([times[off[b]:off[b + 1]].astype(np.float64).sum() for b in range(B)])[:, None]
    query = rng.uniform(-0.2, total + 0.2, (B, Q)).astype(NP[dtype])
    g = rng.standard_normal((B, Q, D, 3)).astype(NP[dtype])
    return lens, off, times, coeffs, query, g


def _check_ragged(tag, dtype, lens, off, times, coeffs, query, g, values, seg, grads):
    gc, gt, gq = grads
    for b in range(len(lens)):
        lo, hi = off[b], off[b + 1]
        if lens[b] == 0:
            assert np.all(np.isnan(values[b])) and np.all(seg[b] == -1) and np.all(gq[b] == 0.0), (tag, b)
            continue
        ref = eval_ref.Ref(times[None, lo:hi], coeffs[None, lo:hi], query[None, b], g.shape[2])
        _check_all("%s b=%d" % (tag, b), ref, g[None, b], dtype, values[None, b], seg[None, b],
                   (gc[None, lo:hi], gt[None, lo:hi], gq[None, b]))


@pytest.mark.parametrize("order,dtype,D", [(2, "f64", 5), (3, "f32", 3), (4, "f64", 3), (4, "f32", 1), (5, "f64", 5)])
def test_accuracy_ragged(csp, order, dtype, D):
    """B = 70, lengths drawn from 0..64 with 0, 1 and 64 present, Q = 9; device and host memory."""
    B, Q = 70, 9
    lens, off, times, coeffs, query, g = _ragged_inputs(order * 7 + D, B, 64, Q, order, dtype, D)
    d_t, d_c, d_q, d_g, d_off = _dev(times, coeffs, query, g, off)
    f = csp.eval_batch(d_t, d_c, d_q, num_derivs=D, seg_offsets=d_off, max_segments=64, want_seg_index=True, want_status=True)
    v = csp.eval_batch_vjp(d_t, d_c, d_q, d_g, seg_offsets=d_off, max_segments=64, want_status=True)
    assert not _np(f.status).any() and not _np(v.status).any()
    _check_ragged("ragged o=%d %s" % (order, dtype), dtype, lens, off, times, coeffs, query, g, _np(f.values), _np(f.seg_index),
                  (_np(v.coeffs), _np(v.times), _np(v.query)))
    hf = csp.eval_batch(times, coeffs, query, num_derivs=D, seg_offsets=off, want_seg_index=True, want_status=True)
    hv = csp.eval_batch_vjp(times, coeffs, query, g, seg_offsets=off, want_status=True)
    for a, b in ((hf.values, f.values), (hf.seg_index, f.seg_index), (hf.status, f.status), (hv.coeffs, v.coeffs),
                 (hv.times, v.times), (hv.query, v.query), (hv.status, v.status)):
        assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------------------ long trajectories

@pytest.mark.parametrize("order,dtype", [(2, "f32"), (4, "f64"), (5, "f64")])
def test_long_trajectories(csp, order, dtype):
    """B = 3, S = 1024, Q = 130: thirteen segment blocks in the reverse kernel, one trajectory per workgroup."""
    times, coeffs, query, g = _inputs(50 + order, 3, 1024, 130, order, dtype, D=3)
    ref = eval_ref.Ref(times, coeffs, query, 3)
    d_t, d_c, d_q, d_g = _dev(times, coeffs, query, g)
    f = csp.eval_batch(d_t, d_c, d_q, num_derivs=3, want_seg_index=True, want_status=True)
    v = csp.eval_batch_vjp(d_t, d_c, d_q, d_g, want_status=True)
    assert not _np(f.status).any() and not _np(v.status).any()
    _check_all("long o=%d %s" % (order, dtype), ref, g, dtype, _np(f.values), _np(f.seg_index),
               (_np(v.coeffs), _np(v.times), _np(v.query)))


def test_query_tiles_and_segment_blocks(csp):
    """S = 100 is two segment blocks of the reverse kernel and Q = 2100 two LDS tiles of queries (2048 slots): a record's
    accumulators and a segment's sum carry over from one tile to the next."""
    times, coeffs, query, g = _inputs(91, 2, 100, 2100, 2, "f64", D=2)
    ref = eval_ref.Ref(times, coeffs, query, 2)
    d_t, d_c, d_q, d_g = _dev(times, coeffs, query, g)
    f = csp.eval_batch(d_t, d_c, d_q, num_derivs=2, want_seg_index=True, want_status=True)
    v = csp.eval_batch_vjp(d_t, d_c, d_q, d_g, want_status=True)
    assert not _np(f.status).any() and not _np(v.status).any()
    _check_all("two tiles, two blocks", ref, g, "f64", _np(f.values), _np(f.seg_index), (_np(v.coeffs), _np(v.times), _np(v.query)))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_misaligned_device_coefficients_are_cloned(csp, dtype):
    """The kernels read records in 16-byte (fp32: 8-byte) pieces; the binding clones a coefficient tensor that does not
    start on such a boundary, and the results are the aligned call's bits."""
    times, coeffs, query, g = _inputs(92, 65, 3, 5, 3, dtype, D=2)
    d_t, d_c, d_q, d_g = _dev(times, coeffs, query, g)
    buf = torch.empty(d_c.numel() + 1, dtype=d_c.dtype, device=DEV)
    view = buf[1:].view(d_c.shape)
    view.copy_(d_c)
    assert view.data_ptr() % 16 != 0
    assert _same_bits(csp.eval_batch(d_t, view, d_q, num_derivs=2).values, csp.eval_batch(d_t, d_c, d_q, num_derivs=2).values)
    a, b = csp.eval_batch_vjp(d_t, view, d_q, d_g), csp.eval_batch_vjp(d_t, d_c, d_q, d_g)
    assert _same_bits(a.coeffs, b.coeffs) and _same_bits(a.times, b.times) and _same_bits(a.query, b.query)


# ---------------------------------------------------------------------------------------------------- knots and clamps

KNOT_TIMES = [0.5, 1.0, 2.0, 0.25, 0.0, 1.0]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_knots_and_clamps_exact(csp, order, dtype):
    """Dyadic times with a zero-length segment inside: queries at every knot, at 0, at sum T, below 0, above sum T and
    one NaN."""
    S, D = len(KNOT_TIMES), 3
    rng = np.random.default_rng(order)
    times = np.tile(np.array(KNOT_TIMES, NP[dtype]), (2, 1))
    coeffs = rng.standard_normal((2, S, 3, 2 * order)).astype(NP[dtype])
    cum = np.concatenate([[0.0], np.cumsum(KNOT_TIMES)])
    #        knots 0..6 (cum[4] == cum[5]: the zero-length segment)      below  above  NaN
    q_list = list(cum) + [-1.0, 5.5, np.nan]
    want_seg = [0, 1, 2, 3, 5, 5, 5, 0, 5, -1]
    nan_at, low_at, high_at = 9, 7, 8
    order_q = [0, 1, 9, 2, 3, 7, 4, 5, 8, 6]                 # the NaN query in the middle
    query = np.tile(np.array(q_list, NP[dtype])[order_q], (2, 1))
    want_seg = np.array(want_seg)[order_q]
    Q = query.shape[1]
    g = rng.standard_normal((2, Q, D, 3)).astype(NP[dtype])
    d_t, d_c, d_q, d_g = _dev(times, coeffs, query, g)
    f = csp.eval_batch(d_t, d_c, d_q, num_derivs=D, want_seg_index=True, want_status=True)
    v = csp.eval_batch_vjp(d_t, d_c, d_q, d_g, want_status=True)
    vals, seg, gq = _np(f.values), _np(f.seg_index), _np(v.query)
    assert not _np(f.status).any() and not _np(v.status).any()          # a NaN query alone does not flag the trajectory
    assert np.array_equal(seg, np.tile(want_seg, (2, 1)))
    pos = {orig: i for i, orig in enumerate(order_q)}
    for k in range(6):                                                   # knots 0..5 start a segment: tau = 0
        j = want_seg[pos[k]]
        assert _same_bits(vals[:, pos[k], 0, :], coeffs[:, j, :, -1]), k
    assert np.all(np.isnan(vals[:, pos[nan_at]])) and np.all(np.isnan(gq[:, pos[nan_at]]))
    assert np.all(gq[:, pos[low_at]] == 0.0) and np.all(gq[:, pos[high_at]] == 0.0)
    keep = [i for i in range(Q) if i != pos[nan_at]]
    ref = eval_ref.Ref(times, coeffs, query[:, keep], D)
    _check_all("knots o=%d %s" % (order, dtype), ref, g[:, keep], dtype, vals[:, keep], seg[:, keep],
               (_np(v.coeffs), _np(v.times), gq[:, keep]))
    # the NaN query has no effect on grad_coeffs and grad_times: the same bits as the call without it
    d_qk, d_gk = _dev(query[:, keep], g[:, keep])
    w = csp.eval_batch_vjp(d_t, d_c, d_qk, d_gk)
    assert _same_bits(w.coeffs, v.coeffs) and _same_bits(w.times, v.times)
    assert _same_bits(_np(w.query), gq[:, keep])
    # a clamped-high query moves grad_times[S-1] only
    d_qh, d_gh = _dev(query[:, [pos[high_at]]], g[:, [pos[high_at]]])
    h = csp.eval_batch_vjp(d_t, d_c, d_qh, d_gh)
    ht = _np(h.times)
    assert np.all(ht[:, :S - 1] == 0.0) and np.all(ht[:, S - 1] != 0.0) and np.all(_np(h.query) == 0.0)
    # and a clamped-low one moves no time at all
    d_ql, d_gl = _dev(query[:, [pos[low_at]]], g[:, [pos[low_at]]])
    assert np.all(_np(csp.eval_batch_vjp(d_t, d_c, d_ql, d_gl).times) == 0.0)


# ------------------------------------------------------------------------------------------- raw calls on guarded buffers

class _Raw:
    """One forward and one reverse call through raw pointers, every array in a guard-banded buffer of its exact size.
    Outputs are filled with 0xFF first."""

    def __init__(self, csp, dtype, order, times, coeffs, query, g, off=None, max_segments=0):
        self.csp, self.dtype = csp, dtype
        self.B, self.Q = query.shape
        self.D = g.shape[2]
        self.inputs = {"times": times, "coeffs": coeffs, "query": query, "g": g}
        if off is not None:
            self.inputs["off"] = off
        self.ins = {k: guarded.carve_from(a, DEV, name=k) for k, a in self.inputs.items()}
        nq = self.B * self.Q
        item = 4 if dtype == "f32" else 8
        sizes = {"out": nq * self.D * 3 * item, "seg": nq * 4, "fstatus": self.B * 4, "gc": coeffs.size * item,
                 "gt": times.size * item, "gq": nq * item, "vstatus": self.B * 4}
        self.outs = {k: guarded.Guarded(n, DEV, name=k).fill(0xFF) for k, n in sizes.items()}
        S = 0 if off is not None else times.shape[1]
        self.desc = csp.make_desc(order, self.B, S, csp.DTYPE_F32 if dtype == "f32" else csp.DTYPE_F64, mem_space=csp.MEM_DEVICE,
                                  seg_offsets_ptr=self.ins["off"].data_ptr() if off is not None else None,
                                  max_segments=max_segments)

    def run(self):
        i, o, lib = self.ins, self.outs, self.csp.raw_lib()
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.csp_minsnap_eval_batch(ctypes.byref(self.desc), i["times"].data_ptr(), i["coeffs"].data_ptr(), i["query"].data_ptr(),
                                        self.Q, self.D, o["out"].data_ptr(), o["seg"].data_ptr(), o["fstatus"].data_ptr(), st)
        assert rc == 0, rc
        rc = lib.csp_minsnap_eval_batch_vjp(ctypes.byref(self.desc), i["times"].data_ptr(), i["coeffs"].data_ptr(),
                                            i["query"].data_ptr(), self.Q, self.D, i["g"].data_ptr(), o["gc"].data_ptr(),
                                            o["gt"].data_ptr(), o["gq"].data_ptr(), o["vstatus"].data_ptr(), st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        for b in list(i.values()) + list(o.values()):
            b.check()
        for k, a in self.inputs.items():
            assert np.array_equal(i[k].bytes(), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), k
        f = NP[self.dtype]
        return {"out": o["out"].numpy(f), "seg": o["seg"].numpy(np.int32), "fstatus": o["fstatus"].numpy(np.int32),
                "gc": o["gc"].numpy(f), "gt": o["gt"].numpy(f), "gq": o["gq"].numpy(f), "vstatus": o["vstatus"].numpy(np.int32)}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("spread", [False, True])
def test_accumulation_order_zeros_and_determinism(csp, spread, dtype):
    """Q = 65 queries of every trajectory in ONE segment, or spread over all sixteen: grad_coeffs within the gate,
    records without a query exactly zero in a buffer that held 0xFF, two runs bit-identical."""
    B, S, Q, order, D = 65, 16, 65, 4, 5
    times, coeffs, query, g = _inputs(77, B, S, Q, order, dtype, D)
    cum = np.concatenate([np.zeros((B, 1)), np.cumsum(times.astype(np.float64), axis=1)], axis=1)
    rng = np.random.default_rng(78)
    if spread:
        j = np.arange(Q) % S
        u = rng.uniform(0.05, 0.95, (B, Q))
        query = (cum[:, j] + u * times.astype(np.float64)[:, j]).astype(NP[dtype])
    else:
        u = rng.uniform(0.05, 0.95, (B, Q))
        query = (cum[:, 7:8] + u * times.astype(np.float64)[:, 7:8]).astype(NP[dtype])
    ref = eval_ref.Ref(times, coeffs, query, D)
    if not spread:
        assert np.all(ref.seg == 7)
    else:
        assert np.all(ref.vjp(g)["count"] >= 4)
    raw = _Raw(csp, dtype, order, times, coeffs, query, g)
    a = raw.run()
    _check_all("accumulation spread=%s %s" % (spread, dtype), ref, g, dtype, a["out"].reshape(B, Q, D, 3), a["seg"].reshape(B, Q),
               (a["gc"], a["gt"].reshape(B, S), a["gq"].reshape(B, Q)))
    if not spread:
        gc = a["gc"].reshape(B, S, -1)
        assert np.all(gc[:, np.arange(S) != 7] == 0.0) and not np.any(np.signbit(gc[:, np.arange(S) != 7]))
    for o in raw.outs.values():
        o.fill(0xFF)
    b = raw.run()
    for k in a:
        assert _same_bits(a[k], b[k]), k


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("B,Q", [(1, 1), (1, 65), (65, 1), (65, 65)])
def test_isolation_and_memory_uniform(csp, B, Q, dtype):
    """Guard bands intact, inputs unchanged; with one trajectory's time NaN and another's -1 those two are flagged and
    NaN and every other trajectory keeps the clean run's bits."""
    S, order, D = 5, 3, 4
    times, coeffs, query, g = _inputs(5 * B + Q, B, S, Q, order, dtype, D)
    clean = _Raw(csp, dtype, order, times, coeffs, query, g).run()
    assert not clean["fstatus"].any() and not clean["vstatus"].any()
    ref = eval_ref.Ref(times, coeffs, query, D)
    _check_all("guarded B=%d Q=%d %s" % (B, Q, dtype), ref, g, dtype, clean["out"].reshape(B, Q, D, 3), clean["seg"].reshape(B, Q),
               (clean["gc"], clean["gt"].reshape(B, S), clean["gq"].reshape(B, Q)))
    if B == 1:
        return
    bad = [3, 64]
    t2 = times.copy()
    t2[3, 2], t2[64, 0] = np.nan, -1.0
    dirty = _Raw(csp, dtype, order, t2, coeffs, query, g).run()
    _check_bad(clean, dirty, bad, B, rows={"out": Q * D * 3, "seg": Q, "gc": S * 6 * order, "gt": S, "gq": Q})


def _check_bad(clean, dirty, bad, B, rows=None, spans=None):
    """rows: elements per trajectory of every per-trajectory array; spans: name -> [B+1] element offsets (ragged)."""
    good = np.setdiff1d(np.arange(B), bad)
    for st in ("fstatus", "vstatus"):
        assert np.all(dirty[st][bad] == NONFINITE) and not dirty[st][good].any(), st
    for k in ("out", "seg", "gc", "gt", "gq"):
        for b in range(B):
            lo, hi = (b * rows[k], (b + 1) * rows[k]) if spans is None or k not in spans else (spans[k][b], spans[k][b + 1])
            if b in bad:
                assert np.all(dirty[k][lo:hi] == -1) if k == "seg" else np.all(np.isnan(dirty[k][lo:hi])), (k, b)
            else:
                assert _same_bits(dirty[k][lo:hi], clean[k][lo:hi]), (k, b)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_isolation_and_memory_ragged(csp, dtype):
    B, Q, order, D = 70, 9, 4, 3
    lens, off, times, coeffs, query, g = _ragged_inputs(11, B, 64, Q, order, dtype, D)
    clean = _Raw(csp, dtype, order, times, coeffs, query, g, off, 64).run()
    assert not clean["fstatus"].any() and not clean["vstatus"].any()
    _check_ragged("guarded ragged " + dtype, dtype, lens, off, times, coeffs, query, g, clean["out"].reshape(B, Q, D, 3),
                  clean["seg"].reshape(B, Q), (clean["gc"].reshape(-1, 3, 2 * order), clean["gt"], clean["gq"].reshape(B, Q)))
    bad = [1, 40] if lens[40] > 0 else [1, 41]
    assert all(lens[b] > 0 for b in bad)
    t2 = times.copy()
    t2[off[bad[0]] + 5], t2[off[bad[1]]] = np.nan, -1.0
    dirty = _Raw(csp, dtype, order, t2, coeffs, query, g, off, 64).run()
    _check_bad(clean, dirty, bad, B, rows={"out": Q * D * 3, "seg": Q, "gq": Q}, spans={"gc": off * 6 * order, "gt": off})


def test_nan_coefficients_flag_their_trajectory_only(csp):
    times, coeffs, query, g = _inputs(9, 65, 4, 7, 4, "f64", 3)
    coeffs[10] = np.nan
    d_t, d_c, d_q, d_g = _dev(times, coeffs, query, g)
    f = csp.eval_batch(d_t, d_c, d_q, num_derivs=3, want_status=True)
    v = csp.eval_batch_vjp(d_t, d_c, d_q, d_g, want=("query",), want_status=True)
    want = np.zeros(65, np.int32)
    want[10] = NONFINITE
    assert np.array_equal(_np(f.status), want) and np.array_equal(_np(v.status), want)


def test_no_queries(csp):
    times, coeffs, query, g = _inputs(9, 65, 4, 0, 4, "f64", 3)
    d_t, d_c, d_q, d_g = _dev(times, coeffs, query, g)
    f = csp.eval_batch(d_t, d_c, d_q, num_derivs=3, want_status=True)
    assert tuple(f.values.shape) == (65, 0, 3, 3) and not _np(f.status).any()
    v = csp.eval_batch_vjp(d_t, d_c, d_q, d_g, num_derivs=3)
    for x in (v.coeffs, v.times):
        assert np.all(_np(x) == 0.0) and not np.any(np.signbit(_np(x)))
    hv = csp.eval_batch_vjp(times, coeffs, query, g, num_derivs=3)
    assert _same_bits(hv.coeffs, v.coeffs) and _same_bits(hv.times, v.times)


# -------------------------------------------------------------------------------------------------- composition, autograd

def test_composition_with_the_solve(csp):
    """solve_batch, then eval_batch at the knots: the later segment's start is the stored coefficient bit for bit, the
    earlier segment's end meets the waypoint within the order-4 parity gate."""
    from tests.test_gpu_parity import TOL_WELL
    B, S, order = 65, 5, 4
    wp, tm = synth.make_batch(B, S, config_id=3)
    d_wp, d_tm = _dev(wp, tm)
    co = csp.solve_batch(d_wp, d_tm, order=order).coeffs
    cum = np.concatenate([np.zeros((B, 1)), np.cumsum(tm, axis=1)], axis=1)
    for k in range(1, S):
        assert np.all(cum[:, k] < cum[:, k + 1])
    d_q, = _dev(cum[:, :S])
    f = csp.eval_batch(d_tm, co, d_q, num_derivs=1, want_seg_index=True)
    assert np.array_equal(_np(f.seg_index), np.tile(np.arange(S), (B, 1)))
    assert _same_bits(_np(f.values)[:, :, 0, :], _np(co)[:, :, :, -1])
    scale = np.max(np.abs(wp))
    worst = 0.0
    for j in range(S):      # segment j at tau = T_j through a one-segment view of its record
        e = csp.eval_batch(d_tm[:, j:j + 1].contiguous(), co[:, j:j + 1].contiguous(), d_tm[:, j:j + 1].contiguous(), num_derivs=1,
                           want_seg_index=True)
        assert not _np(e.seg_index).any()
        worst = max(worst, np.max(np.abs(_np(e.values)[:, 0, 0, :] - wp[:, j + 1])) / scale)
    print("segment ends vs waypoints: %.3e of the waypoints' scale (gate %.1e)" % (worst, TOL_WELL))
    assert worst <= TOL_WELL


def _leaf(a, grad=True):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def test_autograd_matches_the_entries(csp):
    times, coeffs, query, _ = _inputs(21, 65, 6, 11, 4, "f64")
    w = torch.from_numpy(np.random.default_rng(22).standard_normal((65, 11, 3, 3))).to(DEV)
    c, t, q = _leaf(coeffs), _leaf(times), _leaf(query)
    vals = csp.eval_batch_autograd(c, t, q, num_derivs=3)
    assert _same_bits(vals.detach(), csp.eval_batch(t.detach(), c.detach(), q.detach(), num_derivs=3).values)
    loss = (vals * w).sum()
    loss.backward()
    v = csp.eval_batch_vjp(t.detach(), c.detach(), q.detach(), w)
    assert _same_bits(c.grad, v.coeffs) and _same_bits(t.grad, v.times) and _same_bits(q.grad, v.query)
    with pytest.raises(RuntimeError):
        loss.backward()                                   # the graph is gone: a second backward raises
    # inputs that do not require grad get None
    c2, t2, q2 = _leaf(coeffs, False), _leaf(times), _leaf(query, False)
    (csp.eval_batch_autograd(c2, t2, q2, num_derivs=3) * w).sum().backward()
    assert c2.grad is None and q2.grad is None and _same_bits(t2.grad, v.times)
    # first-order only
    c3 = _leaf(coeffs)
    g3, = torch.autograd.grad((csp.eval_batch_autograd(c3, t.detach(), q.detach()) * w).sum(), c3, create_graph=True)
    with pytest.raises(RuntimeError):
        g3.sum().backward()


@pytest.mark.parametrize("periodic", [False, True])
def test_autograd_chain_with_the_solves(csp, periodic):
    """solve -> eval -> sum w * values: waypoints.grad is the solve's VJP of eval's grad_coeffs, times.grad is eval's
    explicit grad_times plus the solve's, bit for bit."""
    B, S, order, Q, D = 65, 5, 4, 7, 3
    wp, tm = synth.make_batch(B, S, config_id=3)
    if periodic:
        wp = wp[:, :S]
    rng = np.random.default_rng(31)
    query = rng.uniform(-0.2, tm.sum(axis=1, keepdims=True) + 0.2, (B, Q))
    w, d_q = _dev(rng.standard_normal((B, Q, D, 3)), query)
    d_wp, d_tm = _leaf(wp), _leaf(tm)
    solve, solve_vjp = ((csp.solve_periodic_batch_autograd, csp.solve_periodic_batch_vjp) if periodic
                        else (csp.solve_batch_autograd, csp.solve_batch_vjp))
    co = solve(d_wp, d_tm, order=order)
    vals = csp.eval_batch_autograd(co, d_tm, d_q, num_derivs=D)
    (vals * w).sum().backward()
    ev = csp.eval_batch_vjp(d_tm.detach(), co.detach(), d_q, w, want=("coeffs", "times"))
    sv = solve_vjp(d_wp.detach(), d_tm.detach(), ev.coeffs, order=order, want=("waypoints", "times"))
    assert _same_bits(d_wp.grad, sv.waypoints)
    assert _same_bits(d_tm.grad, ev.times + sv.times)
