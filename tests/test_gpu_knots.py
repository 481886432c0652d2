"""csp_minsnap_solve_knots_batch on the GPU: accuracy against the 40-digit reference of
tests/knots_ref.py under seven mask patterns, the ties to the entries that exist (the generic solve, the snap cost),
ignored entries, memory and isolation with guard-banded buffers (tests/guarded.py), and chaining into eval_batch.

Shapes: B = 65 (one full wave and one lane of the next), orders 2..5, uniform S in {1, 2, 3, 16, 17} and one ragged batch
with lengths from {0, 1, 2, 5, 33}.  Times U(0.5, 2), waypoints random walks of step ~5, K = 3 distinct trajectories
tiled over each batch (the reference is solved once per distinct trajectory and shared; every copy must be bit-equal
with its first copy).  vel_zero_weight is per trajectory: 0, 0.3, 0 for the three rows.

Gate (tests/test_gpu_time_spread.py's rule): e_k <= max(10 e_cpu64, floor) per coefficient power
(synth.rel_err_per_power's metric) and for J; e_cpu64 is the reference's own code in Python floats, floor the generic
family's gate for the order (TOL_LD; TOL_F32 for fp32 storage).  Where the constraint count is <= order the minimiser is
a polynomial of degree < order: the exact coefficients of the powers p >= order are zero, that metric divides by nothing,
and those powers are scaled by L / T_min^p (L the longest leg) instead; J is exactly zero there and is scaled by
L^2 / T_min^(2o-1).  The same happens to single powers at S = 1: a free derivative r at an end makes the coefficient of
t^(2o-1-r) of the only segment exactly zero (the natural boundary condition).  So the rule is applied to every power
whose 40-digit coefficient is below 1e-25 of L / T_min^p in every segment, which contains the count rule's case.
Combinations whose
count is below the order have no unique minimiser and are dropped from the accuracy cases (the count rule has its own
test).  With CSP_PARITY_SURVEY=<file> every gate appends its figures to the file and does not assert.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import guarded, knots_ref
from tests.test_gpu_edges import TOL_F32, TOL_LD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NONFINITE, NOT_SPD = 1, 2
ORDERS = (2, 3, 4, 5)
SEGMENTS = (1, 2, 3, 16, 17)
RAGGED_LENS = (5, 0, 1, 33, 2, 2, 0, 5, 1)
PATTERNS = ("standard", "free_end", "both_free", "vel_mid", "acc_mid", "hermite", "random")
K = 3
B = 65
VW = (0.0, 0.3, 0.0)
FACTOR = 10.0
SURVEY = os.environ.get("CSP_PARITY_SURVEY")
EXACT_ZERO = 1e-25


# ----------------------------------------------------------------------------------------------------------------- inputs

def make_case(order, S, pattern, row, dyadic=False):
    """(path [S+1,3], time [S], mask [S+1], values [S+1,o-1,3], w) of one trajectory, a function of its arguments alone.
    dyadic: the times are rounded to multiples of 2^-20, so that every sum of them -- every knot's time -- is an exact
    double (the chaining tests, which ask eval_batch for the state AT a knot)."""
    n = order - 1
    full = (1 << n) - 1
    rng = np.random.default_rng([order, S, PATTERNS.index(pattern), row, 20261020])
    path = np.cumsum(rng.normal(size=(S + 1, 3)) * 5, axis=0)
    time = rng.uniform(0.5, 2.0, S)
    if dyadic:
        time = np.round(time * 2.0 ** 20) / 2.0 ** 20
    values = rng.normal(size=(S + 1, n, 3))
    values[0, 2:] = values[S, 2:] = 0.0          # the standard problem: jerk and snap at the ends are zero
    mask = np.zeros(S + 1, dtype=np.uint8)
    mask[0] = mask[S] = full
    mid = S // 2
    if pattern == "free_end":
        mask[S] = 0
    elif pattern == "both_free":
        mask[0] = mask[S] = 0
    elif pattern == "vel_mid":
        mask[mid] |= 1
    elif pattern == "acc_mid":
        mask[mid] = 2 if n > 1 else 1
    elif pattern == "hermite":
        mask[:] = full
    elif pattern == "random":
        mask[:] = rng.integers(0, full + 1, size=S + 1)
    return path, time, mask, values, VW[row % K]


def solvable(order, S, pattern):
    return all(knots_ref.constraint_count(order, make_case(order, S, pattern, r)[2]) >= order for r in range(K))


@functools.lru_cache(maxsize=None)
def reference(order, S, pattern, row, dyadic=False):
    """(40-digit Solution, the same code in Python floats) of one distinct trajectory; computed once, never changed."""
    path, time, mask, values, w = make_case(order, S, pattern, row, dyadic)
    hi = knots_ref.solve(order, path, time, mask, values, vel_zero_weight=w)
    lo = knots_ref.solve(order, path, time, mask, values, vel_zero_weight=w, dps=None)
    for s in (hi, lo):
        s.coeffs.setflags(write=False)
        s.x.setflags(write=False)
    return hi, lo


def batch(order, S, pattern, rows=B, dyadic=False):
    cs = [make_case(order, S, pattern, r, dyadic) for r in range(K)]
    idx = np.arange(rows) % K
    return tuple(np.ascontiguousarray(np.stack([c[i] for c in cs])[idx]) for i in range(5))


def errors(order, got, got_j, ref, path, time, mask):
    """(per-power coefficient error, J error) of one trajectory against a Solution, with the module docstring's scaling."""
    m = 2 * order
    den = np.max(np.abs(ref.coeffs), axis=(0, 1))
    L = np.max(np.linalg.norm(np.diff(path, axis=0), axis=1))
    tmin = float(np.min(time))
    for i in range(m):
        alt = L / tmin ** (m - 1 - i)
        if den[i] < EXACT_ZERO * alt:     # exactly zero in every segment (1e-40 of the scale in the 40-digit solve)
            den[i] = alt
    jalt = L * L / tmin ** (2 * order - 1)
    jden = abs(ref.cost) if abs(ref.cost) >= EXACT_ZERO * jalt else jalt
    e = float(np.max(np.abs(np.asarray(got, np.float64) - ref.coeffs) / den))
    return e, abs(float(got_j) - ref.cost) / jden


def judge(tag, e_k, e_cpu, floor):
    print("%s: e_k %.3e  e_cpu64 %.3e  ratio %.2f  floor %.1e" % (tag, e_k, e_cpu, e_k / max(e_cpu, 1e-300), floor))
    if SURVEY:
        with open(SURVEY, "a") as f:
            f.write(json.dumps({"tag": [str(t) for t in tag], "e_k": e_k, "e_cpu64": e_cpu, "ratio": e_k / max(e_cpu, 1e-300),
                                "floor": floor}) + "\n")
        return
    assert e_k <= max(FACTOR * e_cpu, floor), ("relative gate", tag, "e_k %.3e" % e_k, "e_cpu64 %.3e" % e_cpu, "floor %.1e" % floor)


def copies_bit_equal(a, tag):
    a = np.ascontiguousarray(a)
    for b in range(K, a.shape[0]):
        assert a[b].tobytes() == a[b % K].tobytes(), ("copy differs from the first copy of its trajectory", tag, b)


def gate_against_reference(order, S, pattern, coeffs, cost, floor, tag):
    ek = ej = ck = cj = 0.0
    for row in range(K):
        path, time, mask, values, w = make_case(order, S, pattern, row)
        hi, lo = reference(order, S, pattern, row)
        a, b = errors(order, coeffs[row], cost[row], hi, path, time, mask)
        c, d = errors(order, lo.coeffs, lo.cost, hi, path, time, mask)
        ek, ej, ck, cj = max(ek, a), max(ej, b), max(ck, c), max(cj, d)
    judge(tag + ("coeffs",), ek, ck, floor)
    judge(tag + ("cost",), ej, cj, floor)


# --------------------------------------------------------------------------------------------------------------- accuracy

@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("order", ORDERS)
def test_accuracy_uniform(csp, order, pattern):
    for S in SEGMENTS:
        if not solvable(order, S, pattern):
            assert pattern in ("both_free", "random") and S + 1 < order, (order, S, pattern)
            continue
        wp, tm, mk, kv, w = batch(order, S, pattern)
        r = csp.solve_knots_batch(wp, tm, mk, kv, order=order, vel_zero_weight_per_traj=w, want_cost=True)
        assert not r.status.any(), (order, S, pattern, r.status)
        copies_bit_equal(r.coeffs, (order, S, pattern))
        copies_bit_equal(r.cost, (order, S, pattern))
        gate_against_reference(order, S, pattern, r.coeffs, r.cost, TOL_LD[order], ("knots", order, pattern, S))


@pytest.mark.parametrize("order", ORDERS)
def test_accuracy_f32_storage(csp, order):
    """fp32 storage, fp64 arithmetic: the reference is solved on the inputs as rounded to fp32."""
    S, pattern = 5, "random"
    ek = ej = 0.0
    cs = [make_case(order, S, pattern, r) for r in range(K)]
    idx = np.arange(B) % K
    wp, tm, mk, kv, w = (np.ascontiguousarray(np.stack([c[i] for c in cs])[idx]) for i in range(5))
    wp, tm, kv = wp.astype(np.float32), tm.astype(np.float32), kv.astype(np.float32)
    r = csp.solve_knots_batch(wp, tm, mk, kv, order=order, vel_zero_weight_per_traj=w, want_cost=True)
    assert r.coeffs.dtype == np.float32 and not r.status.any()
    copies_bit_equal(r.coeffs, (order, "f32"))
    for row in range(K):
        hi = knots_ref.solve(order, wp[row], tm[row], mk[row], kv[row], vel_zero_weight=w[row])
        a, b = errors(order, r.coeffs[row], r.cost[row], hi, wp[row].astype(np.float64), tm[row].astype(np.float64), mk[row])
        ek, ej = max(ek, a), max(ej, b)
    judge(("knots f32", order, "coeffs"), ek, 0.0, TOL_F32)
    judge(("knots f32", order, "cost"), ej, 0.0, TOL_LD[order])     # J is stored in fp64


def ragged_batch(order, pattern="random"):
    """The ragged batch: lengths RAGGED_LENS, trajectory i is make_case(order, len, pattern, i % K)."""
    wps, tms, mks, kvs, ws = [], [], [], [], []
    for i, n in enumerate(RAGGED_LENS):
        if n == 0:
            rng = np.random.default_rng(i)
            wps.append(rng.normal(size=(1, 3)))
            tms.append(np.zeros(0))
            mks.append(np.array([0xFF], np.uint8))
            kvs.append(rng.normal(size=(1, order - 1, 3)))
            ws.append(0.0)
            continue
        pat = pattern if solvable(order, n, pattern) else "standard"
        p, t, m, v, w = make_case(order, n, pat, i % K)
        wps.append(p), tms.append(t), mks.append(m), kvs.append(v), ws.append(w)
    off = np.concatenate([[0], np.cumsum(RAGGED_LENS)]).astype(np.int64)
    return np.concatenate(wps), np.concatenate(tms), np.concatenate(mks), np.concatenate(kvs), np.array(ws), off


@pytest.mark.parametrize("order", ORDERS)
def test_accuracy_ragged(csp, order):
    wp, tm, mk, kv, w, off = ragged_batch(order)
    r = csp.solve_knots_batch(wp, tm, mk, kv, order=order, vel_zero_weight_per_traj=w, seg_offsets=off, want_cost=True)
    assert not r.status.any(), r.status
    ek = ej = ck = cj = 0.0
    for i, n in enumerate(RAGGED_LENS):
        if n == 0:
            assert r.cost[i] == 0.0
            continue
        pat = "random" if solvable(order, n, "random") else "standard"
        path, time, mask, values, _ = make_case(order, n, pat, i % K)
        hi, lo = reference(order, n, pat, i % K)
        a, b = errors(order, r.coeffs[off[i]:off[i + 1]], r.cost[i], hi, path, time, mask)
        c, d = errors(order, lo.coeffs, lo.cost, hi, path, time, mask)
        ek, ej, ck, cj = max(ek, a), max(ej, b), max(ck, c), max(cj, d)
    judge(("knots ragged", order, "coeffs"), ek, ck, TOL_LD[order])
    judge(("knots ragged", order, "cost"), ej, cj, TOL_LD[order])


# ------------------------------------------------------------------------------------------------ ties to what exists

@pytest.mark.parametrize("order", ORDERS)
def test_standard_mask_meets_the_generic_solve_and_the_snap_cost(csp, order):
    """knots_from_bc's problem is solve_batch's: the coefficients sit within the gate of this file,
    max(10 e_cpu64, floor), of solve_batch(force_generic=True) per coefficient power (on the generic solve's scale), and
    the cost within it of snap_cost_batch; e_cpu64 is the standard case's, from the shared reference."""
    for S in SEGMENTS:
        wp, tm, _, kv, w = batch(order, S, "standard")
        bc = np.zeros((B, 4, 3))
        bc[:, 0], bc[:, 1] = kv[:, 0, 0], kv[:, S, 0]
        if order > 2:
            bc[:, 2], bc[:, 3] = kv[:, 0, 1], kv[:, S, 1]
        mk, kv2 = csp.knots_from_bc(bc, S, order)
        r = csp.solve_knots_batch(wp, tm, mk, kv2, order=order, vel_zero_weight_per_traj=w, want_cost=True)
        g = csp.solve_batch(wp, tm, bc, order=order, vel_zero_weight_per_traj=w, force_generic=True, want_status=True)
        j = csp.snap_cost_batch(wp, tm, bc, order=order, vel_zero_weight_per_traj=w, want_grad=False)
        assert not r.status.any() and not g.status.any() and not j.status.any()
        den = np.max(np.abs(g.coeffs), axis=(1, 2), keepdims=True)
        e = float(np.max(np.abs(r.coeffs - g.coeffs) / np.where(den == 0, 1.0, den)))
        ej = float(np.max(np.abs(r.cost - j.cost) / np.abs(j.cost)))
        ck = cj = 0.0
        for row in range(K):
            path, time, mask, _, _ = make_case(order, S, "standard", row)
            hi, lo = reference(order, S, "standard", row)
            c, d = errors(order, lo.coeffs, lo.cost, hi, path, time, mask)
            ck, cj = max(ck, c), max(cj, d)
        judge(("knots vs generic", order, S, "coeffs"), e, ck, TOL_LD[order])
        judge(("knots vs snap_cost_batch", order, S, "cost"), ej, cj, TOL_LD[order])


@pytest.mark.parametrize("order", ORDERS)
def test_free_end_never_costs_more(csp, order):
    """Freeing the end state enlarges the feasible set: on every trajectory J(free end) <= J(standard) for the same
    waypoints and times, up to the rounding of the two sums (the accuracy floor of the order, relative)."""
    for S in SEGMENTS:
        wp, tm, mk, kv, w = batch(order, S, "standard")
        std = csp.solve_knots_batch(wp, tm, mk, kv, order=order, vel_zero_weight_per_traj=w, want_cost=True)
        mk2 = mk.copy()
        mk2[:, S] = 0
        free = csp.solve_knots_batch(wp, tm, mk2, kv, order=order, vel_zero_weight_per_traj=w, want_cost=True)
        assert not std.status.any() and not free.status.any()
        assert np.all(free.cost <= std.cost * (1 + TOL_LD[order])), (order, S, np.max(free.cost - std.cost))


# --------------------------------------------------------------------------------------------------------- ignored entries

@pytest.mark.parametrize("order", ORDERS)
def test_unmasked_values_and_high_mask_bits_change_nothing(csp, order):
    n = order - 1
    for S in (1, 3, 17):
        pattern = "random" if solvable(order, S, "random") else "free_end"
        wp, tm, mk, kv, w = batch(order, S, pattern)
        a = csp.solve_knots_batch(wp, tm, mk, kv, order=order, vel_zero_weight_per_traj=w, want_cost=True)
        free = ((mk[:, :, None] >> np.arange(n)[None, None, :]) & 1) == 0
        kv2 = kv.copy()
        kv2[free] = np.nan
        kv2[0][free[0]] = np.inf
        mk2 = (mk | (0xFF & ~((1 << n) - 1))).astype(np.uint8)
        b = csp.solve_knots_batch(wp, tm, mk2, kv2, order=order, vel_zero_weight_per_traj=w, want_cost=True)
        assert not a.status.any() and not b.status.any()
        assert a.coeffs.tobytes() == b.coeffs.tobytes() and a.cost.tobytes() == b.cost.tobytes(), (order, S)


# ----------------------------------------------------------------------------------------------------- memory and isolation

def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("order", ORDERS)
def test_device_tensors_give_the_host_call_bits(csp, order):
    """The binding with torch CUDA tensors (device memory, the caller's workspace and stream), the mask and the values
    once as device tensors and once as knots_from_bc's numpy arrays beside device waypoints: the host call's bits."""
    S = 5
    wp, tm, _, _, w = batch(order, S, "standard")
    mk, kv = csp.knots_from_bc(np.random.default_rng(order).normal(size=(B, 4, 3)), S, order)
    h = csp.solve_knots_batch(wp, tm, mk, kv, order=order, vel_zero_weight_per_traj=w, want_cost=True)
    ws = torch.empty(csp.knots_workspace_bytes(csp.make_desc(order, B, S)), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    d1 = csp.solve_knots_batch(_dev(wp), _dev(tm), _dev(mk), _dev(kv), order=order, vel_zero_weight_per_traj=_dev(w), want_cost=True,
                               workspace=ws, stream=stream.cuda_stream)
    stream.synchronize()
    d2 = csp.solve_knots_batch(_dev(wp), _dev(tm), mk, kv, order=order, vel_zero_weight_per_traj=_dev(w), want_cost=True)
    torch.cuda.synchronize()
    for d in (d1, d2):
        assert d.coeffs.is_cuda and d.coeffs.shape == (B, S, 3, 2 * order)
        assert d.coeffs.cpu().numpy().tobytes() == h.coeffs.tobytes() and d.cost.cpu().numpy().tobytes() == h.cost.tobytes()
        assert not d.status.cpu().numpy().any()


def _guarded_call(csp, order, host, uniform_S, max_segments, fill, f32, want_cost=True):
    """One device-memory call through the raw C-ABI with every array in a guard-banded buffer of exactly its documented
    size; workspace and outputs start as `fill` bytes.  Checks the return code, every band, and that no input changed."""
    Bn = host["vw"].shape[0]
    total = host["times"].size
    elt = 4 if f32 else 8
    n = order - 1
    ins = {k: guarded.carve_from(v, DEV, name=k) for k, v in host.items()}
    outs = {"coeffs": guarded.Guarded(total * 3 * 2 * order * elt, DEV, name="coeffs").fill(fill),
            "cost": guarded.Guarded(Bn * 8, DEV, name="cost").fill(fill),
            "status": guarded.Guarded(Bn * 4, DEV, name="status").fill(fill)}
    ragged = uniform_S is None
    desc = csp.make_desc(order, Bn, 0 if ragged else uniform_S, csp.DTYPE_F32 if f32 else csp.DTYPE_F64, 0.0, 0.0, csp.MEM_DEVICE,
                         False, ins["seg_offsets"].data_ptr() if ragged else None, max_segments if ragged else 0, ins["vw"].data_ptr())
    need = csp.knots_workspace_bytes(desc)
    smax = max_segments if ragged else uniform_S
    assert need == ((smax + 1) * (n * n + 3 * n) * Bn * 8 + 255) // 256 * 256
    ws = guarded.Guarded(need, DEV, name="workspace").fill(fill)
    rc = csp.raw_lib().csp_minsnap_solve_knots_batch(
        ctypes.byref(desc), ins["waypoints"].data_ptr(), ins["times"].data_ptr(), ins["knot_mask"].data_ptr(),
        ins["knot_values"].data_ptr(), outs["coeffs"].data_ptr(), outs["cost"].data_ptr() if want_cost else None,
        outs["status"].data_ptr(), ws.data_ptr(), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, csp.strerror(rc))
    torch.cuda.synchronize()
    for g in [ws] + list(ins.values()) + list(outs.values()):
        g.check()
    for k, g in ins.items():
        assert g.bytes().tobytes() == np.ascontiguousarray(host[k]).tobytes(), (k, "an input changed")
    fl = np.float32 if f32 else np.float64
    return dict(coeffs=outs["coeffs"].numpy(fl), cost=outs["cost"].numpy(np.float64), status=outs["status"].numpy(np.int32))


def _host_inputs(order, Bn, S, f32, pattern="random"):
    fl = np.float32 if f32 else np.float64
    pat = pattern if solvable(order, S, pattern) else "free_end"
    wp, tm, mk, kv, w = batch(order, S, pat, rows=Bn)
    return dict(waypoints=wp.astype(fl), times=tm.astype(fl), knot_mask=mk, knot_values=kv.astype(fl), vw=w)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("Bn", [1, 65])
@pytest.mark.parametrize("order", ORDERS)
def test_guard_bands_stale_workspace_and_host_call(csp, order, Bn, f32):
    """Nothing is written outside coeffs / cost / status, inputs are untouched, a 0x00-filled and a 0xFF-filled start
    give identical bits (so do two runs), the coefficients do not depend on the cost being asked for, and the
    host-memory call returns the device call's bits."""
    for S in (1, 2, 17):
        host = _host_inputs(order, Bn, S, f32)
        a = _guarded_call(csp, order, host, S, None, 0x00, f32)
        b = _guarded_call(csp, order, host, S, None, 0xFF, f32)
        c = _guarded_call(csp, order, host, S, None, 0xFF, f32)
        d = _guarded_call(csp, order, host, S, None, 0x00, f32, want_cost=False)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), (k, "differs between a 0x00 and a 0xFF start, or run to run")
        assert a["coeffs"].tobytes() == d["coeffs"].tobytes() and not d["cost"].any()
        assert not a["status"].any()
        h = csp.solve_knots_batch(host["waypoints"], host["times"], host["knot_mask"], host["knot_values"], order=order,
                                  vel_zero_weight_per_traj=host["vw"], want_cost=True)
        assert h.coeffs.tobytes() == a["coeffs"].tobytes() and h.cost.tobytes() == a["cost"].tobytes()
        assert not h.status.any()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("order", ORDERS)
def test_guard_bands_ragged(csp, order, f32):
    """The ragged batch (empty trajectories included, max_segments above the longest): as the uniform guard test; an
    empty trajectory gets cost 0 and status 0 and nothing else."""
    fl = np.float32 if f32 else np.float64
    wp, tm, mk, kv, w, off = ragged_batch(order)
    host = dict(waypoints=wp.astype(fl), times=tm.astype(fl), knot_mask=mk, knot_values=kv.astype(fl), vw=w, seg_offsets=off)
    a = _guarded_call(csp, order, host, None, 40, 0x00, f32)
    b = _guarded_call(csp, order, host, None, 40, 0xFF, f32)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert not a["status"].any()
    assert all(a["cost"][i] == 0.0 for i, n in enumerate(RAGGED_LENS) if n == 0)
    h = csp.solve_knots_batch(host["waypoints"], host["times"], mk, host["knot_values"], order=order, vel_zero_weight_per_traj=w,
                              seg_offsets=off, max_segments=40, want_cost=True)
    assert h.coeffs.reshape(-1).tobytes() == a["coeffs"].tobytes() and h.cost.tobytes() == a["cost"].tobytes()


@pytest.mark.parametrize("order", ORDERS)
def test_ragged_trajectory_longer_than_max_segments_is_skipped(csp, order):
    """Device memory, max_segments = 5 with the 33-segment member in the batch and the workspace (guard-banded) sized
    for 5: that trajectory gets CSP_TRAJ_SKIPPED and a NaN cost, its coefficients are not written, nothing is written
    outside the buffers, and every other trajectory has the bits of the call with max_segments = 40."""
    wp, tm, mk, kv, w, off = ragged_batch(order)
    host = dict(waypoints=wp, times=tm, knot_mask=mk, knot_values=kv, vw=w, seg_offsets=off)
    full = _guarded_call(csp, order, host, None, 40, 0xFF, False)
    short = _guarded_call(csp, order, host, None, 5, 0xFF, False)
    M = 2 * order
    for i, n in enumerate(RAGGED_LENS):
        a, b = (x["coeffs"].reshape(-1, 3 * M)[off[i]:off[i + 1]] for x in (short, full))
        if n > 5:
            assert short["status"][i] == 4 and np.isnan(short["cost"][i])
            assert (a.view(np.uint8) == 0xFF).all(), "coefficients of the skipped trajectory were written"
        else:
            assert short["status"][i] == 0 and a.tobytes() == b.tobytes()
            assert short["cost"][i].tobytes() == full["cost"][i].tobytes()


@pytest.mark.parametrize("order", (3, 4, 5))
def test_count_rule_lanes(csp, order):
    """B = 65, S = 1 (two positions), where the count rule reads the masks at every order >= 3.  Three lanes carry every
    mask bit from order-1 upward at both knots, over different low bits.  Lane 7: no low bit (count 2: rejected); lane
    20: bit 0 at the start alone (count 3: rejected at orders 4 and 5, accepted at order 3); lane 33: order-2 low bits
    at the start, which bring the count to exactly the order (accepted).  A rejected lane has status CSP_TRAJ_NOT_SPD
    alone and NaN coefficients and cost; the high bits change no output bit; every other lane keeps the clean run's
    bits."""
    S, n = 1, order - 1
    hi_bits = 0xFF & ~((1 << n) - 1)
    good = _host_inputs(order, B, S, False, pattern="standard")
    bad = {k: v.copy() for k, v in good.items()}
    low = {7: (0, 0), 20: (1, 0), 33: ((1 << (order - 2)) - 1, 0)}          # popcounts 0, 1, order - 2
    for lane, (m0, m1) in low.items():
        bad["knot_mask"][lane] = (m0 | hi_bits, m1 | hi_bits)
    plain = {k: v.copy() for k, v in bad.items()}
    plain["knot_mask"] = (bad["knot_mask"] & ~np.uint8(hi_bits)).astype(np.uint8)
    ob, op, og = (_guarded_call(csp, order, h, S, None, 0xFF, False) for h in (bad, plain, good))
    st = ob["status"]
    print("order %d: status of lanes 7, 20, 33:" % order, [int(st[k]) for k in low])
    others = np.setdiff1d(np.arange(B), list(low))
    assert not st[others].any() and not og["status"].any()
    for k in ("coeffs", "cost"):
        assert ob[k].reshape(B, -1)[others].tobytes() == og[k].reshape(B, -1)[others].tobytes(), (k, "a lane disturbed another lane")
        assert ob[k].tobytes() == op[k].tobytes(), (k, "mask bits from order-1 upward changed an output")
    assert np.array_equal(st, op["status"])
    for lane in low:
        count = knots_ref.constraint_count(order, bad["knot_mask"][lane])
        assert count == 2 + bin(low[lane][0]).count("1")
        co, jv = ob["coeffs"].reshape(B, -1)[lane], ob["cost"][lane]
        if count < order:
            assert st[lane] == NOT_SPD and np.isnan(co).all() and np.isnan(jv), (lane, st[lane])
        else:
            assert st[lane] == 0 and np.isfinite(co).all() and np.isfinite(jv), (lane, st[lane])
            assert co.tobytes() == op["coeffs"].reshape(B, -1)[lane].tobytes()


@pytest.mark.parametrize("order", ORDERS)
def test_bad_lanes(csp, order):
    """B = 65, S = 2, both ends free on lane 40 alone (count 3: rejected by the count rule at orders 4 and 5, a valid
    problem at orders 2 and 3), a NaN time on lane 5, T = -1 on lane 64 (alone in the tail wave): flagged as specified,
    and every other lane keeps the clean run's bits."""
    S = 2
    good = _host_inputs(order, B, S, False, pattern="standard")
    bad = {k: v.copy() for k, v in good.items()}
    bad["times"][5, 1] = np.nan
    bad["times"][64, 0] = -1.0
    bad["knot_mask"][40, 0] = bad["knot_mask"][40, S] = 0
    lanes = [5, 40, 64]
    ob, og = (_guarded_call(csp, order, h, S, None, 0xFF, False) for h in (bad, good))
    st = ob["status"]
    print("order %d: status of the bad lanes" % order, {k: int(st[k]) for k in lanes})
    others = np.setdiff1d(np.arange(B), lanes)
    assert not st[others].any() and not og["status"].any()
    for k in ("coeffs", "cost"):
        assert ob[k].reshape(B, -1)[others].tobytes() == og[k].reshape(B, -1)[others].tobytes(), (k, "a bad lane disturbed another lane")
    assert st[5] & NONFINITE and st[64] & NOT_SPD, (st[5], st[64])
    co40, j40 = ob["coeffs"].reshape(B, -1)[40], ob["cost"][40]
    if S + 1 < order:
        assert st[40] == NOT_SPD and np.isnan(co40).all() and np.isnan(j40)
    else:
        assert st[40] == 0 and np.isfinite(co40).all() and np.isfinite(j40)


# ------------------------------------------------------------------------------------------------------------------ chaining

CHAIN_CASES = ((3, "free_end"), (16, "vel_mid"), (17, "random"))


def _chain(csp, order, S, pattern):
    """The solve of one chaining case and eval_batch at every knot's time: (mask, values, eval result, per-knot worst
    error / gate of the pinned derivatives [K, S+1], NaN where a knot pins nothing)."""
    from tests import eval_ref
    M = 2 * order
    if not solvable(order, S, pattern):
        pattern = "free_end"
    wp, tm, mk, kv, w = batch(order, S, pattern, dyadic=True)
    r = csp.solve_knots_batch(wp, tm, mk, kv, order=order, vel_zero_weight_per_traj=w)
    assert not r.status.any()
    cum = np.concatenate([np.zeros((B, 1)), np.cumsum(tm, axis=1)], axis=1)     # eval_batch's own left-to-right sums
    ev = csp.eval_batch(tm, r.coeffs, cum, num_derivs=order, want_seg_index=True, want_status=True)
    assert not ev.status.any()
    ratio = np.full((K, S + 1), np.nan)
    for b in range(K):
        for k in range(S + 1):
            j = int(ev.seg_index[b, k])
            assert j == min(k, S - 1)
            tau = cum[b, k] - cum[b, j]
            assert tau == (tm[b, S - 1] if k == S else 0.0)      # the query is the knot, not a rounded neighbour of it
            for d in range(1, order):
                if not (mk[b, k] >> (d - 1)) & 1:
                    continue
                ff = np.array([np.prod(np.arange(p, p - d, -1.0)) if p >= d else 0.0 for p in range(M - 1, -1, -1)])
                pw = np.array([tau ** max(p - d, 0) for p in range(M - 1, -1, -1)])
                A = np.sum(np.abs(r.coeffs[b, j] * ff * pw), axis=1)
                err = np.abs(ev.values[b, k, d] - kv[b, k, d - 1])
                bound = eval_ref.gamma(2 * M + 2) * A      # A = 0: a zero pinned at tau = 0 is a zero coefficient, exactly
                rel = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
                ratio[b, k] = np.nanmax([ratio[b, k], float(np.max(rel))])
    return pattern, ev, ratio


@pytest.mark.parametrize("order", ORDERS)
def test_eval_batch_returns_the_pinned_values_and_the_free_end_state(csp, order):
    """eval_batch reads the coefficients unchanged.  At the time of every knot 0..S-1 with a pinned derivative (the
    query falls on the later segment's start) it returns the pinned value within DESIGN.md §19.3's gate
    gamma(2M + 2) A (A: the sum of the magnitudes of the terms of that derivative of the segment's polynomial at the
    query); at a free end it returns the reference's end state within the accuracy gate of this file, on the scale of
    that derivative over the trajectory's knots.  The last knot has its own test below."""
    for S, pattern in CHAIN_CASES:
        pattern, ev, ratio = _chain(csp, order, S, pattern)
        worst = float(np.nanmax(ratio[:, :S]))
        print("order %d S %d %s: pinned values at knots 0..S-1 through eval_batch, worst error / gate = %.3f" % (order, S, pattern, worst))
        assert worst <= 1.0, (order, S, pattern, worst)
        if pattern == "free_end":
            e = ec = 0.0
            for b in range(K):
                hi, lo = reference(order, S, pattern, b, True)
                den = np.max(np.abs(hi.x), axis=(0, 2))
                e = max(e, float(np.max(np.abs(ev.values[b, S, 1:] - hi.x[S]) / den[:, None])))
                ec = max(ec, float(np.max(np.abs(lo.x[S] - hi.x[S]) / den[:, None])))
            judge(("knots free end state", order, S), e, ec, TOL_LD[order])


@pytest.mark.parametrize("order", ORDERS)
def test_eval_batch_returns_the_pinned_values_at_the_last_knot(csp, order):
    """The same gate at knot S, whose query is the last segment's END (tau = T): the whole polynomial is evaluated, and
    it meets the pinned value only as far as the recovered coefficients are those of the Hermite interpolant of the
    knot derivatives.  A recovery in plain fp64 misses this gate 17 (order 4) to 29 (order 5) times over, because the
    sums G d cancel; the kernel recovers in double-double arithmetic for that reason.  With
    times that are not dyadic the query itself is off the knot by the rounding of the running sum (tau != T), which
    costs up to the whole gate whatever the coefficients are: hence make_case's dyadic times."""
    worst = 0.0
    for S, pattern in CHAIN_CASES:
        pattern, ev, ratio = _chain(csp, order, S, pattern)
        if np.isfinite(ratio[:, S]).any():
            w = float(np.nanmax(ratio[:, S]))
            print("order %d S %d %s: pinned values at knot S through eval_batch, worst error / gate = %.3f" % (order, S, pattern, w))
            worst = max(worst, w)
    assert worst <= 1.0, (order, worst)
