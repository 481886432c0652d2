"""csp_minsnap_solve_knots_batch_vjp on the GPU: accuracy against the 40-digit reference adjoint of
tests/knots_vjp_ref.py under the seven mask patterns of tests/test_gpu_knots.py, the ties to the entries that exist
(the open chain's reverse mode, the snap cost's time gradient), exact zeros and ignored entries, memory and isolation
with guard-banded buffers (tests/guarded.py), and the torch op with its chain into eval_batch_autograd.

Inputs are tests/test_gpu_knots.py's: B = 65, orders 2..5, uniform S in {1, 2, 3, 16, 17} and the ragged batch, K = 3
distinct trajectories tiled over each batch, per-trajectory w.  Cotangents: grad_coeffs of two kinds (N(0,1) per entry;
(T_j / 2)^pow_i, the cotangent of the sum of the midpoint positions), grad_cost ~ N(0,1) per trajectory; calls with
grad_coeffs alone, grad_cost alone and both.  The adjoint is linear in the cotangents, so the reference of the call
with both is the sum of the two references.

Gate, per output and call: e_k <= max(10 e_cpu64, floor) with tests/vjp_ref.rel_err_rows' metric (per trajectory max-abs
error over max-abs reference), the time gradient also in its T-weighted form (g_j T_j); e_cpu64 is the reference's own
code in Python floats, floor GATE_NUMPY[order] of tests/test_gpu_vjp.py (max with TOL_F32 under fp32 storage).  With
CSP_PARITY_SURVEY=<file> every gate appends its figures to the file and does not assert.

Where the constraint count is <= order the minimiser is a polynomial of degree < order and J is exactly zero
(tests/test_gpu_knots.py): every gradient of the grad_cost-alone call is then exactly zero and the metric divides by
nothing.  An output whose 40-digit reference is below 1e-25 of its scale in every entry is measured against that scale
instead: |grad_cost| L / T_min^(2o-1) for the waypoints, |grad_cost| L^2 / T_min^(2o) for the times (T_min^(2o-1) in the
T-weighted form) and |grad_cost| L / T_min^(2o-2) for the values, L the longest leg.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import eval_ref, guarded, knots_ref, knots_vjp_ref
from tests import test_gpu_knots as tk
from tests.test_gpu_edges import TOL_F32
from tests.test_gpu_timeopt import GATE_G
from tests.test_gpu_vjp import GATE_NUMPY
from tests.vjp_ref import rel_err_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NONFINITE, NOT_SPD, SKIPPED = 1, 2, 4
ORDERS, SEGMENTS, PATTERNS, K, B = tk.ORDERS, tk.SEGMENTS, tk.PATTERNS, tk.K, tk.B
FACTOR = 10.0
SURVEY = os.environ.get("CSP_PARITY_SURVEY")
OUTPUTS = ("waypoints", "times", "knot_values")
CALLS = ("pbar", "jbar", "both", "pbar_mid")


# ----------------------------------------------------------------------------------------------------------------- inputs

def cotangents(order, S, pattern, row, time, f32=False):
    """(grad_coeffs N(0,1) [S,3,2o], grad_coeffs (T_j/2)^pow_i [S,3,2o], grad_cost) of one trajectory."""
    m = 2 * order
    rng = np.random.default_rng([order, S, PATTERNS.index(pattern), row, 20261021])
    pn = rng.normal(size=(S, 3, m))
    pm = np.broadcast_to((np.asarray(time, np.float64)[:, None, None] / 2.0) ** np.arange(m - 1, -1, -1.0)[None, None, :], (S, 3, m)).copy()
    if f32:
        pn, pm = pn.astype(np.float32).astype(np.float64), pm.astype(np.float32).astype(np.float64)
    return pn, pm, float(rng.normal())


def _sum(a, b):
    return knots_vjp_ref.Adjoint(*(x + y for x, y in zip(a, b)))


@functools.lru_cache(maxsize=None)
def reference(order, S, pattern, row, f32=False):
    """{call: (40-digit Adjoint, the same code in Python floats)} of one distinct trajectory; computed once, never
    changed.  f32: the inputs and grad_coeffs as rounded to fp32."""
    path, time, mask, values, w = tk.make_case(order, S, pattern, row)
    if f32:
        path, time, values = (a.astype(np.float32).astype(np.float64) for a in (path, time, values))
    pn, pm, jb = cotangents(order, S, pattern, row, time, f32)
    out = {}
    runs = [knots_vjp_ref.adjoints(order, path, time, mask, values, [(pn, 0.0), (None, jb), (pm, 0.0)], w, dps=d) for d in (40, None)]
    for i, call in enumerate(("pbar", "jbar", "pbar_mid")):
        out[call] = (runs[0][i], runs[1][i])
    out["both"] = (_sum(runs[0][0], runs[0][1]), _sum(runs[1][0], runs[1][1]))
    for pair in out.values():
        for adj in pair:
            for a in adj:
                a.setflags(write=False)
    return out


def batch(order, S, pattern, rows=B, f32=False):
    """test_gpu_knots.batch plus the tiled cotangents: dict of host arrays."""
    wp, tm, mk, kv, w = tk.batch(order, S, pattern, rows=rows)
    fl = np.float32 if f32 else np.float64
    wp, tm, kv = wp.astype(fl), tm.astype(fl), kv.astype(fl)
    cs = [cotangents(order, S, pattern, r, tm[r].astype(np.float64), f32) for r in range(min(K, rows))]
    idx = np.arange(rows) % K
    pn, pm, jb = (np.ascontiguousarray(np.stack([np.asarray(c[i]) for c in cs])[idx]) for i in range(3))
    return dict(wp=wp, tm=tm, mk=mk, kv=kv, w=w, pn=pn.astype(fl), pm=pm.astype(fl), jb=jb)


def cot_of(h, call):
    return {"pbar": (h["pn"], None), "jbar": (None, h["jb"]), "both": (h["pn"], h["jb"]), "pbar_mid": (h["pm"], None)}[call]


def run(csp, order, h, call, **kw):
    gco, gj = cot_of(h, call)
    return csp.solve_knots_batch_vjp(h["wp"], h["tm"], h["mk"], h["kv"], grad_coeffs=gco, grad_cost=gj, order=order,
                                     vel_zero_weight_per_traj=h["w"], want_status=True, **kw)


def zero_scales(order, path, time, jb):
    """The module docstring's scales of one trajectory's outputs under a grad_cost jb."""
    L = float(np.max(np.linalg.norm(np.diff(np.asarray(path, np.float64), axis=0), axis=1)))
    tmin, m, jb = float(np.min(time)), 2 * order, abs(float(jb))
    return {"waypoints": jb * L / tmin ** (m - 1), "times": jb * L * L / tmin ** m, "times_T": jb * L * L / tmin ** (m - 1),
            "knot_values": jb * L / tmin ** (m - 2)}


def errors(got, ref, tm, scales=None):
    """got / ref: lists (one per trajectory) of (waypoints, times, values); the metric per output.  scales: per
    trajectory zero_scales() or None."""
    tm = [np.asarray(t, np.float64) for t in tm]
    scales = scales or [None] * len(tm)

    def worst(key, gs, rs):
        e = 0.0
        for g, r, sc in zip(gs, rs, scales):
            g, r = np.asarray(g, np.float64).reshape(1, -1), np.asarray(r, np.float64).reshape(1, -1)
            if sc is not None and sc[key] > 0 and np.max(np.abs(r)) < tk.EXACT_ZERO * sc[key]:
                e = max(e, float(np.max(np.abs(g - r))) / sc[key])
            else:
                e = max(e, rel_err_rows(g, r))
        return e
    return {"waypoints": worst("waypoints", [g[0] for g in got], [r[0] for r in ref]),
            "times": worst("times", [g[1] for g in got], [r[1] for r in ref]),
            "times_T": worst("times_T", [np.asarray(g[1], np.float64) * t for g, t in zip(got, tm)], [r[1] * t for r, t in zip(ref, tm)]),
            "knot_values": worst("knot_values", [g[2] for g in got], [r[2] for r in ref])}


def judge(tag, e_k, e_cpu, floor):
    print("%s: e_k %.3e  e_cpu64 %.3e  ratio %.2f  floor %.1e" % (tag, e_k, e_cpu, e_k / max(e_cpu, 1e-300), floor))
    if SURVEY:
        with open(SURVEY, "a") as f:
            f.write(json.dumps({"tag": [str(t) for t in tag], "e_k": e_k, "e_cpu64": e_cpu, "ratio": e_k / max(e_cpu, 1e-300),
                                "floor": floor}) + "\n")
        return
    assert e_k <= max(FACTOR * e_cpu, floor), ("relative gate", tag, "e_k %.3e" % e_k, "e_cpu64 %.3e" % e_cpu, "floor %.1e" % floor)


def gate(tag, got, hi, lo, tm, floor, scales=None):
    ek, ec = errors(got, hi, tm, scales), errors(lo, hi, tm, scales)
    for key in ek:
        judge(tag + (key,), ek[key], ec[key], floor)


def triple(g, row=None):
    pick = (lambda a: a) if row is None else (lambda a: a[row])
    return pick(g.waypoints), pick(g.times), pick(g.knot_values)


# --------------------------------------------------------------------------------------------------------------- accuracy

@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("order", ORDERS)
def test_accuracy_uniform(csp, order, pattern):
    for S in SEGMENTS:
        if not tk.solvable(order, S, pattern):
            assert pattern in ("both_free", "random") and S + 1 < order, (order, S, pattern)
            continue
        h = batch(order, S, pattern)
        refs = [reference(order, S, pattern, r) for r in range(K)]
        for call in CALLS:
            g = run(csp, order, h, call)
            assert not g.status.any(), (order, S, pattern, call, g.status)
            for a in triple(g):
                tk.copies_bit_equal(a, (order, S, pattern, call))
            gate(("knots vjp", order, pattern, S, call), [triple(g, r) for r in range(K)], [refs[r][call][0] for r in range(K)],
                 [refs[r][call][1] for r in range(K)], h["tm"][:K], GATE_NUMPY[order],
                 [zero_scales(order, h["wp"][r], h["tm"][r], h["jb"][r]) for r in range(K)] if call == "jbar" else None)


@pytest.mark.parametrize("S", (3, 16))
@pytest.mark.parametrize("order", ORDERS)
def test_accuracy_f32_storage(csp, order, S):
    """fp32 storage, fp64 arithmetic: the reference is solved on the inputs and cotangents as rounded to fp32."""
    pattern = "random" if tk.solvable(order, S, "random") else "free_end"
    h = batch(order, S, pattern, f32=True)
    refs = [reference(order, S, pattern, r, True) for r in range(K)]
    for call in CALLS:
        g = run(csp, order, h, call)
        assert g.waypoints.dtype == np.float32 and g.times.dtype == np.float32 and g.knot_values.dtype == np.float32
        assert not g.status.any()
        for a in triple(g):
            tk.copies_bit_equal(a, (order, S, "f32", call))
        gate(("knots vjp f32", order, pattern, S, call), [triple(g, r) for r in range(K)], [refs[r][call][0] for r in range(K)],
             [refs[r][call][1] for r in range(K)], h["tm"][:K], max(GATE_NUMPY[order], TOL_F32),
             [zero_scales(order, h["wp"][r], h["tm"][r], h["jb"][r]) for r in range(K)] if call == "jbar" else None)


def ragged(order):
    """test_gpu_knots.ragged_batch plus cotangents; members: (length, pattern, row) per trajectory."""
    wp, tm, mk, kv, w, off = tk.ragged_batch(order)
    members, pn, pm, jb = [], [], [], []
    for i, n in enumerate(tk.RAGGED_LENS):
        if n == 0:
            members.append((0, None, None))
            jb.append(0.5)
            continue
        pat = "random" if tk.solvable(order, n, "random") else "standard"
        members.append((n, pat, i % K))
        a, b, c = cotangents(order, n, pat, i % K, tm[off[i]:off[i + 1]])
        pn.append(a), pm.append(b), jb.append(c)
    return dict(wp=wp, tm=tm, mk=mk, kv=kv, w=w, off=off, pn=np.concatenate(pn), pm=np.concatenate(pm), jb=np.array(jb)), members


@pytest.mark.parametrize("order", ORDERS)
def test_accuracy_ragged(csp, order):
    h, members = ragged(order)
    off = h["off"]
    for call in CALLS:
        g = run(csp, order, h, call, seg_offsets=off)
        assert not g.status.any(), g.status
        got, hi, lo, tms, scales = [], [], [], [], []
        for i, (n, pat, row) in enumerate(members):
            k0, k1 = off[i] + i, off[i + 1] + i + 1
            if n == 0:   # its one knot row: zeros
                assert not g.waypoints[k0:k1].any() and not g.knot_values[k0:k1].any()
                continue
            got.append((g.waypoints[k0:k1], g.times[off[i]:off[i + 1]], g.knot_values[k0:k1]))
            r = reference(order, n, pat, row)[call]
            hi.append(r[0]), lo.append(r[1]), tms.append(h["tm"][off[i]:off[i + 1]])
            scales.append(zero_scales(order, h["wp"][k0:k1], tms[-1], h["jb"][i]))
        gate(("knots vjp ragged", order, call), got, hi, lo, tms, GATE_NUMPY[order], scales if call == "jbar" else None)


# ------------------------------------------------------------------------------------------------ ties to what exists

@pytest.mark.parametrize("order", ORDERS)
def test_standard_mask_meets_the_open_chain_vjp_and_the_snap_cost(csp, order):
    """knots_from_bc's problem is solve_batch's: grad_waypoints and grad_times sit within the gate of this file of
    solve_batch_vjp(..., grad_cost=...) with a per-trajectory bc, the end knots' value rows 0 and 1 are its grad_bc, and
    the grad_cost-alone grad_times divided by grad_cost is within GATE_G of snap_cost_batch's grad_times."""
    for S in SEGMENTS:
        h = batch(order, S, "standard")
        kv = h["kv"]
        bc = np.zeros((B, 4, 3))
        bc[:, 0], bc[:, 1] = kv[:, 0, 0], kv[:, S, 0]
        if order > 2:
            bc[:, 2], bc[:, 3] = kv[:, 0, 1], kv[:, S, 1]
        mk, kv2 = csp.knots_from_bc(bc, S, order)
        assert np.array_equal(mk, h["mk"])
        h = dict(h, kv=kv2)
        refs = [reference(order, S, "standard", r) for r in range(K)]
        for call in ("pbar", "jbar", "both"):
            gco, gj = cot_of(h, call)
            g = run(csp, order, h, call)
            v = csp.solve_batch_vjp(h["wp"], h["tm"], gco, bc, order=order, vel_zero_weight_per_traj=h["w"], grad_cost=gj,
                                    want_status=True)
            assert not g.status.any() and not v.status.any()
            gbc = np.zeros((B, 4, 3))
            gbc[:, 0], gbc[:, 1] = g.knot_values[:, 0, 0], g.knot_values[:, S, 0]
            if order > 2:
                gbc[:, 2], gbc[:, 3] = g.knot_values[:, 0, 1], g.knot_values[:, S, 1]
            vbc = v.bc.copy()
            if order == 2:
                vbc[:, 2:] = 0.0
            ec = errors([refs[r][call][1] for r in range(K)], [refs[r][call][0] for r in range(K)], h["tm"][:K])
            for key, a, b in (("waypoints", g.waypoints, v.waypoints), ("times", g.times, v.times), ("knot_values", gbc, vbc)):
                judge(("knots vjp vs open chain", order, S, call, key), rel_err_rows(a, b), ec[key], GATE_NUMPY[order])
        g = run(csp, order, h, "jbar", want=("times",))
        c = csp.snap_cost_batch(h["wp"], h["tm"], bc, order=order, vel_zero_weight_per_traj=h["w"])
        e = rel_err_rows(g.times / h["jb"][:, None], c.grad_times)
        print("order %d S %d: grad_times / grad_cost against snap_cost_batch %.3e" % (order, S, e))
        assert e <= GATE_G[order], (order, S, e)


# --------------------------------------------------------------------------------------- exact zeros and ignored entries

@pytest.mark.parametrize("order", ORDERS)
def test_free_slots_are_zero_and_unmasked_values_and_high_mask_bits_change_nothing(csp, order):
    n = order - 1
    for S in (1, 3, 17):
        pattern = "random" if tk.solvable(order, S, "random") else "free_end"
        h = batch(order, S, pattern)
        free = ((h["mk"][:, :, None] >> np.arange(n)[None, None, :]) & 1) == 0
        kv2 = h["kv"].copy()
        kv2[free] = np.nan
        kv2[0][free[0]] = np.inf
        h2 = dict(h, kv=kv2, mk=(h["mk"] | (0xFF & ~((1 << n) - 1))).astype(np.uint8))
        for call in ("pbar", "jbar", "both"):
            a, b = run(csp, order, h, call), run(csp, order, h2, call)
            assert not a.status.any() and not b.status.any()
            for x, y in zip(triple(a), triple(b)):
                assert x.tobytes() == y.tobytes(), (order, S, call)
            z = a.knot_values[free]
            assert z.size and not z.view(np.uint64).any(), (order, S, call, "a free slot's gradient is not +0.0")


# ----------------------------------------------------------------------------------------------------- memory and isolation

def _guarded_call(csp, order, host, cots, uniform_S, max_segments, fill, f32, want=OUTPUTS):
    """One device-memory call through the raw C-ABI with every array in a guard-banded buffer of exactly its documented
    size; workspace and outputs start as `fill` bytes.  Checks the return code, every band, and that no input or
    cotangent changed.  host: waypoints, times, knot_mask, knot_values, vw (, seg_offsets); cots: grad_coeffs and / or
    grad_cost."""
    Bn = host["vw"].shape[0]
    total, knots = host["times"].size, host["knot_mask"].size
    elt = 4 if f32 else 8
    n = order - 1
    ins = {k: guarded.carve_from(v, DEV, name=k) for k, v in dict(host, **cots).items()}
    sizes = {"waypoints": knots * 3 * elt, "times": total * elt, "knot_values": knots * n * 3 * elt}
    outs = {k: guarded.Guarded(sizes[k], DEV, name="grad_" + k).fill(fill) for k in OUTPUTS}
    outs["status"] = guarded.Guarded(Bn * 4, DEV, name="status").fill(fill)
    is_ragged = uniform_S is None
    desc = csp.make_desc(order, Bn, 0 if is_ragged else uniform_S, csp.DTYPE_F32 if f32 else csp.DTYPE_F64, 0.0, 0.0, csp.MEM_DEVICE,
                         False, ins["seg_offsets"].data_ptr() if is_ragged else None, max_segments if is_ragged else 0,
                         ins["vw"].data_ptr())
    c = 6 if "grad_coeffs" in cots else 3
    need = csp.knots_vjp_workspace_bytes(desc, c == 6)
    smax = max_segments if is_ragged else uniform_S
    assert need == ((smax + 1) * (n * n + c * n) * Bn * 8 + 255) // 256 * 256
    ws = guarded.Guarded(need, DEV, name="workspace").fill(fill)
    ptr = lambda d, k: d[k].data_ptr() if k in d else None
    rc = csp.raw_lib().csp_minsnap_solve_knots_batch_vjp(
        ctypes.byref(desc), ins["waypoints"].data_ptr(), ins["times"].data_ptr(), ins["knot_mask"].data_ptr(),
        ins["knot_values"].data_ptr(), ptr(ins, "grad_coeffs"), ptr(ins, "grad_cost"),
        *(outs[k].data_ptr() if k in want else None for k in OUTPUTS),
        outs["status"].data_ptr(), ws.data_ptr(), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, csp.strerror(rc))
    torch.cuda.synchronize()
    for g in [ws] + list(ins.values()) + list(outs.values()):
        g.check()
    for k, g in ins.items():
        src = host[k] if k in host else cots[k]
        assert g.bytes().tobytes() == np.ascontiguousarray(src).tobytes(), (k, "an input changed")
    fl = np.float32 if f32 else np.float64
    res = {k: outs[k].numpy(fl) for k in OUTPUTS}
    for k in OUTPUTS:
        if k not in want:
            assert (outs[k].bytes() == fill).all(), (k, "an output that was not asked for was written")
    res["status"] = outs["status"].numpy(np.int32)
    return res


def _host(h, f32, off=None):
    fl = np.float32 if f32 else np.float64
    d = dict(waypoints=h["wp"].astype(fl), times=h["tm"].astype(fl), knot_mask=h["mk"], knot_values=h["kv"].astype(fl), vw=h["w"])
    if off is not None:
        d["seg_offsets"] = off
    return d


def _cots(h, c, f32):
    fl = np.float32 if f32 else np.float64
    return dict(grad_coeffs=h["pn"].astype(fl), grad_cost=h["jb"]) if c == 6 else dict(grad_cost=h["jb"])


@pytest.mark.parametrize("c", (6, 3))
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("Bn", [1, 65])
@pytest.mark.parametrize("order", ORDERS)
def test_guard_bands_stale_workspace_and_host_call(csp, order, Bn, f32, c):
    """Nothing is written outside the requested outputs and status, inputs and cotangents are untouched, a 0x00-filled
    and a 0xFF-filled start give identical bits (so do two runs), each output's bits do not depend on which other
    outputs are asked for, and the host-memory call returns the device call's bits."""
    for S in (1, 2, 17):
        pattern = "random" if tk.solvable(order, S, "random") else "free_end"
        h = batch(order, S, pattern, rows=Bn, f32=f32)
        host, cots = _host(h, f32), _cots(h, c, f32)
        a = _guarded_call(csp, order, host, cots, S, None, 0x00, f32)
        b = _guarded_call(csp, order, host, cots, S, None, 0xFF, f32)
        d = _guarded_call(csp, order, host, cots, S, None, 0xFF, f32)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes() == d[k].tobytes(), (k, "differs between a 0x00 and a 0xFF start, or run to run")
        assert not a["status"].any()
        for k in OUTPUTS:
            one = _guarded_call(csp, order, host, cots, S, None, 0xFF, f32, want=(k,))
            assert one[k].tobytes() == a[k].tobytes(), (k, "depends on which other outputs are asked for")
            assert not one["status"].any()
        g = csp.solve_knots_batch_vjp(host["waypoints"], host["times"], host["knot_mask"], host["knot_values"],
                                      grad_coeffs=cots.get("grad_coeffs"), grad_cost=cots["grad_cost"], order=order,
                                      vel_zero_weight_per_traj=host["vw"], want_status=True)
        for k, x in zip(OUTPUTS, triple(g)):
            assert x.tobytes() == a[k].tobytes(), (k, "the host call differs from the device call")
        assert not g.status.any()


@pytest.mark.parametrize("c", (6, 3))
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("order", ORDERS)
def test_guard_bands_ragged(csp, order, f32, c):
    """The ragged batch (empty trajectories included, max_segments above the longest): as the uniform guard test; an
    empty trajectory gets status 0 and zeros in its one knot row."""
    h, members = ragged(order)
    off = h["off"]
    host, cots = _host(h, f32, off), _cots(h, c, f32)
    a = _guarded_call(csp, order, host, cots, None, 40, 0x00, f32)
    b = _guarded_call(csp, order, host, cots, None, 40, 0xFF, f32)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert not a["status"].any()
    n = order - 1
    for i, (length, _, _) in enumerate(members):
        if length == 0:
            k0 = off[i] + i
            assert not a["waypoints"].reshape(-1, 3)[k0].view(np.uint8).any()
            assert not a["knot_values"].reshape(-1, 3 * n)[k0].view(np.uint8).any()
    g = csp.solve_knots_batch_vjp(host["waypoints"], host["times"], host["knot_mask"], host["knot_values"],
                                  grad_coeffs=cots.get("grad_coeffs"), grad_cost=cots["grad_cost"], order=order,
                                  vel_zero_weight_per_traj=host["vw"], seg_offsets=off, max_segments=40)
    for k, x in zip(OUTPUTS, triple(g)):
        assert x.reshape(-1).tobytes() == a[k].tobytes(), k


@pytest.mark.parametrize("order", ORDERS)
def test_ragged_trajectory_longer_than_max_segments_is_skipped(csp, order):
    """Device memory, max_segments = 5 with the 33-segment member in the batch and the workspace (guard-banded) sized
    for 5: that trajectory gets CSP_TRAJ_SKIPPED and NaN in every gradient row it owns, nothing is written outside the
    buffers, and every other trajectory has the bits of the call with max_segments = 40."""
    h, members = ragged(order)
    off = h["off"]
    host, cots = _host(h, False, off), _cots(h, 6, False)
    full = _guarded_call(csp, order, host, cots, None, 40, 0xFF, False)
    short = _guarded_call(csp, order, host, cots, None, 5, 0xFF, False)
    n = order - 1
    for i, (length, _, _) in enumerate(members):
        k0, k1 = off[i] + i, off[i + 1] + i + 1
        rows = lambda x: (x["waypoints"].reshape(-1, 3)[k0:k1], x["times"][off[i]:off[i + 1]], x["knot_values"].reshape(-1, 3 * n)[k0:k1])
        if length > 5:
            assert short["status"][i] == SKIPPED and all(np.isnan(x).all() for x in rows(short))
        else:
            assert short["status"][i] == 0
            for x, y in zip(rows(short), rows(full)):
                assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("order", ORDERS)
def test_bad_lanes(csp, order):
    """B = 65, S = 2: a NaN time on lane 5, T = -1 on lane 64 (alone in the tail wave), an infinite grad_coeffs entry on
    lane 21, both ends free on lane 40 (count 3: rejected by the count rule at orders 4 and 5, a valid problem at orders 2
    and 3): flagged as specified, and every other lane keeps the clean run's bits."""
    S = 2
    h = batch(order, S, "standard")
    good, cots = _host(h, False), _cots(h, 6, False)
    bad, bcots = {k: v.copy() for k, v in good.items()}, {k: v.copy() for k, v in cots.items()}
    bad["times"][5, 1] = np.nan
    bad["times"][64, 0] = -1.0
    bcots["grad_coeffs"][21, 1, 2, 0] = np.inf
    bad["knot_mask"][40, 0] = bad["knot_mask"][40, S] = 0
    lanes = [5, 21, 40, 64]
    ob, og = _guarded_call(csp, order, bad, bcots, S, None, 0xFF, False), _guarded_call(csp, order, good, cots, S, None, 0xFF, False)
    st = ob["status"]
    print("order %d: status of the bad lanes" % order, {k: int(st[k]) for k in lanes})
    others = np.setdiff1d(np.arange(B), lanes)
    assert not st[others].any() and not og["status"].any()
    for k in OUTPUTS:
        assert ob[k].reshape(B, -1)[others].tobytes() == og[k].reshape(B, -1)[others].tobytes(), (k, "a bad lane disturbed another lane")
    assert st[5] & NONFINITE and st[64] & NOT_SPD and st[21] == NONFINITE, (st[5], st[64], st[21])
    g40 = np.concatenate([ob[k].reshape(B, -1)[40] for k in OUTPUTS])
    if S + 1 < order:
        assert st[40] == NOT_SPD and np.isnan(g40).all()
    else:
        assert st[40] == 0 and np.isfinite(g40).all()


@pytest.mark.parametrize("order", (3, 4, 5))
def test_count_rule_lanes_at_one_segment(csp, order):
    """B = 65, S = 1: lane 7 has no mask bit below order-1 (count 2: rejected), lane 33 has order-2 low bits at the start
    (count = order: accepted); both carry every bit from order-1 upward.  A rejected lane has CSP_TRAJ_NOT_SPD alone and
    NaN in every gradient row it owns; every other lane keeps the clean run's bits."""
    S, n = 1, order - 1
    hi_bits = 0xFF & ~((1 << n) - 1)
    h = batch(order, S, "standard")
    good, cots = _host(h, False), _cots(h, 6, False)
    bad = {k: v.copy() for k, v in good.items()}
    bad["knot_mask"][7] = (hi_bits, hi_bits)
    bad["knot_mask"][33] = (((1 << (order - 2)) - 1) | hi_bits, hi_bits)
    ob, og = _guarded_call(csp, order, bad, cots, S, None, 0xFF, False), _guarded_call(csp, order, good, cots, S, None, 0xFF, False)
    others = np.setdiff1d(np.arange(B), [7, 33])
    assert not ob["status"][others].any() and not og["status"].any()
    for k in OUTPUTS:
        assert ob[k].reshape(B, -1)[others].tobytes() == og[k].reshape(B, -1)[others].tobytes(), (k, "a lane disturbed another lane")
    g7, g33 = (np.concatenate([ob[k].reshape(B, -1)[lane] for k in OUTPUTS]) for lane in (7, 33))
    assert ob["status"][7] == NOT_SPD and np.isnan(g7).all()
    assert ob["status"][33] == 0 and np.isfinite(g33).all()


# ---------------------------------------------------------------------------------------------------------------------- torch

def _dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_(True) if grad else t


def test_autograd_forward_is_bit_equal_and_subsets_return_none(csp):
    order, S = 4, 5
    h = batch(order, S, "vel_mid", rows=7)
    r = csp.solve_knots_batch(h["wp"], h["tm"], h["mk"], h["kv"], order=order, vel_zero_weight_per_traj=h["w"], want_cost=True)
    for needs in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
        wp, tm, kv = (_dev(h[k], f) for k, f in zip(("wp", "tm", "kv"), needs))
        co, cost = csp.solve_knots_batch_autograd(wp, tm, h["mk"], kv, order=order, vel_zero_weight_per_traj=_dev(h["w"]), with_cost=True)
        assert co.detach().cpu().numpy().tobytes() == r.coeffs.tobytes() and cost.detach().cpu().numpy().tobytes() == r.cost.tobytes()
        ((co * _dev(h["pn"])).sum() + (cost * _dev(h["jb"])).sum()).backward()
        g = run(csp, order, h, "both")
        for t, f, ref in zip((wp, tm, kv), needs, triple(g)):
            assert (t.grad is not None) == f
            if f:
                assert t.grad.cpu().numpy().tobytes() == ref.tobytes()
    co = csp.solve_knots_batch_autograd(_dev(h["wp"]), _dev(h["tm"]), _dev(h["mk"]), _dev(h["kv"]), order=order,
                                        vel_zero_weight_per_traj=_dev(h["w"]))
    assert co.grad_fn is None and co.cpu().numpy().tobytes() == r.coeffs.tobytes()


def test_autograd_gradcheck(csp):
    """torch.autograd.gradcheck at order 3, S = 4, B = 2 with a mid-knot velocity pin, over waypoints, times and values
    (the free slots' analytic gradient is 0, and so is the numerical one: the entries are never read)."""
    order, S = 3, 4
    h = batch(order, S, "vel_mid", rows=2)
    wp, tm, kv = _dev(h["wp"], True), _dev(h["tm"], True), _dev(h["kv"], True)
    fn = lambda a, b, c: csp.solve_knots_batch_autograd(a, b, h["mk"], c, order=order, vel_zero_weight=0.2, with_cost=True)
    assert torch.autograd.gradcheck(fn, (wp, tm, kv), eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=0.0)


def test_cost_only_loss_runs_the_three_column_kernel(csp, monkeypatch):
    """A loss on the cost alone reaches solve_knots_batch_vjp with grad_coeffs None (no allocation, the smaller
    workspace) and matches the grad_cost-alone call bit for bit."""
    order, S = 4, 5
    h = batch(order, S, "free_end", rows=7)
    seen = []
    real = csp.solve_knots_batch_vjp
    monkeypatch.setattr(csp, "solve_knots_batch_vjp", lambda *a, **k: seen.append((k["grad_coeffs"], k["grad_cost"])) or real(*a, **k))
    wp, tm, kv = _dev(h["wp"], True), _dev(h["tm"], True), _dev(h["kv"], True)
    _, cost = csp.solve_knots_batch_autograd(wp, tm, h["mk"], kv, order=order, vel_zero_weight_per_traj=_dev(h["w"]), with_cost=True)
    (cost * _dev(h["jb"])).sum().backward()
    assert len(seen) == 1 and seen[0][0] is None and seen[0][1] is not None
    g = run(csp, order, h, "jbar")
    for t, ref in zip((wp, tm, kv), triple(g)):
        assert t.grad.cpu().numpy().tobytes() == ref.tobytes()
    seen.clear()
    co, _ = csp.solve_knots_batch_autograd(wp, tm, h["mk"], kv, order=order, vel_zero_weight_per_traj=_dev(h["w"]), with_cost=True)
    (co * _dev(h["pn"])).sum().backward()
    assert len(seen) == 1 and seen[0][0] is not None and seen[0][1] is None


@pytest.mark.parametrize("order", ORDERS)
def test_chain_into_eval_batch(csp, order):
    """L = sum eval_batch_autograd(coeffs, times, query) with a velocity pinned at S/2: dL/d(that velocity),
    dL/dwaypoints and dL/dtimes against the 40-digit reference adjoint composed with tests/eval_ref.py's exact cotangent
    (grad_coeffs of the evaluation, plus its explicit time gradient), under the accuracy gate of this file."""
    S, D, Q = 6, 3, 9
    D = min(D, order)
    h = batch(order, S, "vel_mid", rows=K)
    rng = np.random.default_rng(order)
    query = np.sort(rng.uniform(0.05, 0.95, size=(K, Q)) * h["tm"].sum(axis=1, keepdims=True), axis=1)
    wp, tm, kv = _dev(h["wp"], True), _dev(h["tm"], True), _dev(h["kv"], True)
    co = csp.solve_knots_batch_autograd(wp, tm, h["mk"], kv, order=order, vel_zero_weight_per_traj=_dev(h["w"]))
    csp.eval_batch_autograd(co, tm, _dev(query), num_derivs=D).sum().backward()
    got, hi, lo = [], [], []
    for b in range(K):
        path, time, mask, values, w = tk.make_case(order, S, "vel_mid", b)
        sol = knots_ref.solve(order, path, time, mask, values, vel_zero_weight=w)
        ev = eval_ref.Ref(time[None], sol.coeffs[None], query[b][None], D).vjp(np.ones((1, Q, D, 3)))
        pbar, direct = ev["coeffs"][0].floats()[0], ev["times"][0].floats()[0]
        for dps, into in ((40, hi), (None, lo)):
            a = knots_vjp_ref.adjoint(order, path, time, mask, values, pbar, 0.0, w, dps=dps)
            into.append((a.waypoints, a.times + direct, a.values))
        got.append((wp.grad[b].cpu().numpy(), tm.grad[b].cpu().numpy(), kv.grad[b].cpu().numpy()))
        mid = S // 2
        assert mask[mid] & 1 and np.abs(hi[-1][2][mid, 0]).max() > 0
    gate(("knots vjp chain", order), got, hi, lo, h["tm"], GATE_NUMPY[order])
