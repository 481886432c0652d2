"""The solver entries at their edge shapes.

* Long trajectories (the span kernel, 257..1024 segments; order 5 on both sides of its switch from the chunked kernel; the
  generic kernel at 1024 segments; fp32 storage; the mixed entry's chunked family) against an independent reference: the
  long-double structured solver of oracle/structured_oracle.cpp (block-tridiagonal formulation in 80-bit arithmetic with
  tables of its own; tests/test_oracle.py ties it to the 80-bit dense oracle and the 60-digit KKT fixture).  The dense
  oracle is O(S^3) and loses digits there, so before this file these families were only compared with each other.
* Order 1 through csp_minsnap_solve_batch (the generic kernel) and plan / sample.
* Entry contracts: the device-resident sharded call when a chunk boundary falls on an odd trajectory, the mixed entry's
  over-long trajectories in its host and device forms, the altitude cyclic-reduction kernels on problems of 1..5 samples.

Every case asserts the kernel it reaches.  Two gates per trajectory: the per-power gate (synth.parity_gate) at a tolerance
placed from a CSP_PARITY_SURVEY run on the MI355X (measured maximum quoted beside it), and the norm-wise north-star figure.
"""
import os

import numpy as np
import pytest

import oracle
from tests import synth
from tests.staged import STAGED as _STAGED, staged_buffers as _staged_buffers

pytestmark = pytest.mark.gpu

NORTH_STAR_TOL = 1e-6
# Per-power tolerances against the long-double structured reference, by order: about 10x the worst figure of a
# CSP_PARITY_SURVEY run on the MI355X over every case of this file at that order (540 gate evaluations).  Measured maxima:
#   order 1: 2.6e-16 (generic, uniform and ragged, S <= 1024)
#   order 2: 1.0e-15 (span, S = 300)                      order 3: 3.6e-13 (generic, S = 1024; span <= 3.8e-14)
#   order 4: 1.9e-11 (span, S = 1000)                     order 5: 7.1e-9 (chunked, S = 17; span <= 4.7e-9 at S = 17,
#                                                                 2.3e-10 from S = 257; generic 1.1e-9 at S = 1024)
# Norm-wise, the worst is 1.1e-11 (order 5): the north-star 1e-6 holds with five orders of magnitude to spare.
TOL_LD = {1: 5e-15, 2: 1e-14, 3: 5e-12, 4: 2e-10, 5: 7e-8}
TOL_DENSE_O1 = 2e-14     # order 1 against the fp64 dense oracle (uniform, and with the path penalty): 2.1e-15
TOL_F32 = 3e-7           # fp32 storage (inputs and coefficients rounded to fp32, 2^-24 = 6e-8 per element): 5.9e-8
NTHREADS = min(16, oracle.max_threads())
SURVEY = bool(os.environ.get("CSP_PARITY_SURVEY"))


def _ld(order, wp, tm, bc=None, vw=0.0, vw_per=None):
    return oracle.struct_solve_batch(order, wp, tm, bc, vel_zero_weight=vw, long_double=True, vel_zero_weight_per_traj=vw_per,
                                     nthreads=NTHREADS)


def _gates(got, ref, tol, tag):
    """The per-power gate and the norm-wise north star, for every trajectory of got / ref ([B,S,3,m] or [S,3,m])."""
    pp, nw = synth.parity_gate(got, ref, tol, tag)
    if not SURVEY:
        assert nw <= NORTH_STAR_TOL, ("north star (norm-wise)", tag, nw)
    return pp, nw


def _inputs(B, S, order, seed):
    rng = np.random.default_rng(seed)
    wp, tm = synth.make_batch(B, S, config_id=seed % 997)
    bc = rng.normal(size=(B, 4, 3))
    vw = rng.uniform(0.0, 0.3, size=B)
    vw[0] = 0.0
    return wp, tm, bc, vw


def _ragged(lens, seed):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    wps, tms = [], []
    for n in lens:
        p0 = rng.uniform(-10, 10, size=(1, 3))
        wps.append(np.concatenate([p0, p0 + np.cumsum(rng.normal(size=(int(n), 3)), axis=0)]))
        tms.append(rng.uniform(0.5, 2.0, size=int(n)))
    return off, wps, tms


# ---------------------------------------------------------------------------------------------------- long trajectories


@pytest.mark.parametrize("S", [257, 300, 512, 1000, 1024])
@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_span_kernel_uniform_against_the_long_double_reference(csp, order, S):
    """Span kernel, uniform batch of an odd size (the last workgroup partial), per-trajectory boundary conditions and
    velocity-zero weights."""
    B = 33
    wp, tm, bc, vw = _inputs(B, S, order, 1000 + 10 * S + order)
    r = csp.solve_batch(wp, tm, bc, order=order, vel_zero_weight_per_traj=vw, want_status=True)
    assert r.kernel.startswith("span_o%d_f64_l" % order), r.kernel
    assert not r.status.any()
    _gates(r.coeffs, _ld(order, wp, tm, bc, vw_per=vw), TOL_LD[order], ("span uniform", order, S))


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_span_kernel_ragged_against_the_long_double_reference(csp, order):
    """One ragged batch with max_segments = 1024 and lengths from 1 to 1024 (both sides of 16, 256 and 1024)."""
    lens = np.array([1, 16, 17, 256, 257, 1023, 1024, 2, 600, 31, 129])
    off, wps, tms = _ragged(lens, 77 + order)
    B = len(lens)
    rng = np.random.default_rng(order)
    bc, vw = rng.normal(size=(B, 4, 3)), rng.uniform(0.0, 0.3, size=B)
    r = csp.solve_batch(np.concatenate(wps), np.concatenate(tms), bc, order=order, seg_offsets=off, max_segments=1024,
                        vel_zero_weight_per_traj=vw, want_status=True)
    assert r.kernel == "span_o%d_f64_l64_ragged" % order, r.kernel
    assert not r.status.any()
    for i, n in enumerate(lens):
        ref = _ld(order, wps[i][None], tms[i][None], bc[i][None], vw_per=vw[i:i + 1])
        _gates(r.coeffs[off[i]:off[i + 1]], ref[0], TOL_LD[order], ("span ragged", order, int(n)))


@pytest.mark.parametrize("S", [17, 24, 32, 33, 48, 64])
def test_order_5_on_both_sides_of_the_span_switch(csp, S):
    """Order 5 from 17 segments goes to the span kernel once the batch fills a wave per SIMD with span lanes
    (B << span_lanes_log2(S) >= 65536, minsnap_capi.hip: pick_kernel); one trajectory fewer stays on the chunked kernel."""
    lanes_log2 = (S - 1).bit_length() - 4          # span_lanes_log2: 16 segments per lane, rounded up to a power of two
    B_span = 65536 >> lanes_log2
    wp, tm, bc, vw = _inputs(B_span, S, 5, 3000 + S)
    ref = _ld(5, wp, tm, bc, vw_per=vw)
    for B, fam in ((B_span - 1, "chunked"), (B_span, "span")):
        r = csp.solve_batch(wp[:B], tm[:B], bc[:B], order=5, vel_zero_weight_per_traj=vw[:B], want_status=True)
        assert r.kernel.startswith("%s_o5_f64_l" % fam), (B, r.kernel)
        assert not r.status.any()
        _gates(r.coeffs, ref[:B], TOL_LD[5], ("order-5 switch", fam, S))


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_generic_kernel_at_1024_segments(csp, order):
    B, S = 5, 1024
    wp, tm, bc, vw = _inputs(B, S, order, 4000 + order)
    r = csp.solve_batch(wp, tm, bc, order=order, vel_zero_weight_per_traj=vw, force_generic=True, want_status=True)
    assert r.kernel == "generic_o%d_f64" % order, r.kernel
    assert not r.status.any()
    _gates(r.coeffs, _ld(order, wp, tm, bc, vw_per=vw), TOL_LD[order], ("generic S=1024", order))


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_fp32_storage_at_300_segments(csp, order):
    """fp32 inputs and coefficients, fp64 arithmetic (span kernel).  The reference solves the fp32-rounded inputs."""
    B, S = 17, 300
    wp, tm, bc, vw = _inputs(B, S, order, 5000 + order)
    wp32, tm32, bc32 = wp.astype(np.float32), tm.astype(np.float32), bc.astype(np.float32)
    r = csp.solve_batch(wp32, tm32, bc32, order=order, vel_zero_weight_per_traj=vw, want_status=True)
    assert r.kernel.startswith("span_o%d_f32io_f64_l" % order), r.kernel
    assert r.coeffs.dtype == np.float32 and not r.status.any()
    ref = _ld(order, wp32.astype(np.float64), tm32.astype(np.float64), bc32.astype(np.float64), vw_per=vw)
    _gates(r.coeffs.astype(np.float64), ref, TOL_F32, ("fp32 storage S=300", order))


def test_mixed_entry_long_trajectories_against_the_long_double_reference(csp):
    """csp_minsnap_solve_mixed's chunked family (65..256 segments) at every order and its order 5 from 33 segments, host
    form with per-trajectory boundary conditions and weights: what tests/test_gpu_round3.py only compares with the same
    chunked kernel behind csp_minsnap_solve_batch."""
    lens, orders = [], []
    for o in (2, 3, 4, 5):
        for n in (65, 66, 100, 127, 128, 129, 200, 255, 256):
            lens.append(n), orders.append(o)
    for n in (33, 34, 40, 47, 63, 64):
        lens.append(n), orders.append(5)
    lens, orders = np.array(lens), np.array(orders, dtype=np.int32)
    perm = np.random.default_rng(3).permutation(len(lens))
    lens, orders = lens[perm], orders[perm]
    off, wps, tms = _ragged(lens, 91)
    B = len(lens)
    rng = np.random.default_rng(92)
    bc, vw = rng.normal(size=(B, 4, 3)), rng.uniform(0.0, 0.3, size=B)
    r = csp.solve_mixed(orders, np.concatenate(wps), np.concatenate(tms), off, bc=bc, vel_zero_weight_per_traj=vw, want_status=True)
    assert not r.status.any()
    for i in range(B):
        o, n = int(orders[i]), int(lens[i])
        got = r.coeffs[r.coeff_offsets[i]:r.coeff_offsets[i] + 6 * o * n].reshape(n, 3, 2 * o)
        ref = _ld(o, wps[i][None], tms[i][None], bc[i][None], vw_per=vw[i:i + 1])
        _gates(got, ref[0], TOL_LD[o], ("mixed long", o, n))


# ---------------------------------------------------------------------------------------------------------------- order 1


@pytest.mark.parametrize("S", [1, 2, 16, 17, 100, 300])
def test_order_1_uniform_batches(csp, oracle_mod, S):
    """Order 1 (the generic kernel): B = 1, 63, 64, 65, 1000 against the long-double reference, per-trajectory boundary
    conditions (order 1 has no free derivative: the kernel must ignore them as the oracle does) and velocity-zero weights;
    up to S = 100 also the first 65 trajectories against the dense oracle."""
    wp, tm, bc, vw = _inputs(1000, S, 1, 6000 + S)
    for B in (1, 63, 64, 65, 1000):
        r = csp.solve_batch(wp[:B], tm[:B], bc[:B], order=1, vel_zero_weight_per_traj=vw[:B], want_status=True)
        assert r.kernel == "generic_o1_f64", r.kernel
        assert not r.status.any()
        ref = _ld(1, wp[:B], tm[:B], bc[:B], vw_per=vw[:B])
        _gates(r.coeffs, ref, TOL_LD[1], ("order 1 uniform", B, S))
        # batch-wide boundary conditions and weight, device memory
        import torch
        d = csp.solve_batch(torch.from_numpy(wp[:B]).cuda(), torch.from_numpy(tm[:B]).cuda(), torch.from_numpy(bc[:1]).cuda(), order=1,
                            vel_zero_weight=0.07)
        torch.cuda.synchronize()
        _gates(d.coeffs.cpu().numpy(), _ld(1, wp[:B], tm[:B], bc[:1], vw=0.07), TOL_LD[1], ("order 1 uniform, device", B, S))
    if S <= 100:
        for b in range(65):
            dense, _ = oracle_mod.solve(1, wp[b], bc[b, [0, 1]], bc[b, [2, 3]], tm[b], 0.0, float(vw[b]))
            got = csp.solve_batch(wp[b:b + 1], tm[b:b + 1], bc[b:b + 1], order=1, vel_zero_weight=float(vw[b])).coeffs[0]
            _gates(got, dense, TOL_DENSE_O1, ("order 1 vs dense", b, S))


def test_order_1_ragged_fp32_segment_major_and_path_penalty(csp, oracle_mod):
    import torch
    lens = np.array([1, 2, 3, 16, 17, 64, 65, 100, 300, 5])
    off, wps, tms = _ragged(lens, 61)
    B = len(lens)
    rng = np.random.default_rng(62)
    bc, vw = rng.normal(size=(B, 4, 3)), rng.uniform(0.0, 0.3, size=B)
    r = csp.solve_batch(np.concatenate(wps), np.concatenate(tms), bc, order=1, seg_offsets=off, vel_zero_weight_per_traj=vw, want_status=True)
    assert r.kernel == "generic_o1_f64_ragged", r.kernel
    assert not r.status.any()
    for i, n in enumerate(lens):
        _gates(r.coeffs[off[i]:off[i + 1]], _ld(1, wps[i][None], tms[i][None], bc[i][None], vw_per=vw[i:i + 1])[0], TOL_LD[1],
               ("order 1 ragged", int(n)))
    # fp32 storage
    wp, tm, bc, vw = _inputs(65, 40, 1, 63)
    r = csp.solve_batch(wp.astype(np.float32), tm.astype(np.float32), bc.astype(np.float32), order=1, vel_zero_weight_per_traj=vw)
    assert r.kernel == "generic_o1_f32io_f64", r.kernel
    ref = _ld(1, wp.astype(np.float32).astype(np.float64), tm.astype(np.float32).astype(np.float64), bc.astype(np.float32).astype(np.float64),
              vw_per=vw)
    _gates(r.coeffs.astype(np.float64), ref, TOL_F32, ("order 1 fp32", 40))
    # segment-major layout [S,B,3,m] (device memory)
    d = csp.solve_batch(torch.from_numpy(wp).cuda(), torch.from_numpy(tm).cuda(), torch.from_numpy(bc).cuda(), order=1,
                        vel_zero_weight_per_traj=torch.from_numpy(vw).cuda(), segment_major=True)
    torch.cuda.synchronize()
    assert d.kernel == "generic_o1_f64", d.kernel
    _gates(np.ascontiguousarray(d.coeffs.cpu().numpy().transpose(1, 0, 2, 3)), _ld(1, wp, tm, bc, vw_per=vw), TOL_LD[1],
           ("order 1 segment-major", 40))
    # the path penalty: coefficients and max_dev against the dense oracle
    wp, tm, bc, _ = _inputs(65, 12, 1, 64)
    for pw, vwt in ((0.3, 0.0), (1e-2, 0.05)):
        r = csp.solve_batch(wp, tm, bc, order=1, path_weight=pw, vel_zero_weight=vwt, want_max_dev=True, want_status=True)
        assert r.kernel == "generic_o1_f64", r.kernel
        assert not r.status.any()
        ref, md = oracle_mod.solve_batch(1, wp, tm, bc, path_weight=pw, vel_zero_weight=vwt, nthreads=NTHREADS)
        _gates(r.coeffs, ref, TOL_DENSE_O1, ("order 1 path penalty", pw))
        assert np.max(np.abs(r.max_dev - md)) <= 1e-9 * max(1.0, float(np.max(md))), (pw, np.max(np.abs(r.max_dev - md)))


def test_order_1_plan_and_sample(csp, oracle_mod):
    B, S = 12, 6
    wp, _ = synth.make_batch(B, S, config_id=21)
    wp = wp * 4.0
    v_avg, min_t, sd = 5.0, 0.1, 0.7
    plan = csp.plan_batch(wp, v_avg, min_t, order=1)
    assert not plan.status.any()
    samples, counts, stats = csp.sample_batch(plan.times, plan.coeffs, sd, 4096)
    for b in range(B):
        ref, info = oracle_mod.generate_trajectory(wp[b], order=1, v_avg=v_avg, min_time_s=min_t, sample_distance=sd)
        assert np.allclose(plan.times[b], info["time"], rtol=0, atol=1e-15 * np.max(info["time"]))
        scale = np.max(np.abs(info["coeff"]))
        assert np.max(np.abs(plan.coeffs[b] - info["coeff"])) < 1e-12 * scale, b
        assert counts[b] == len(ref), (b, counts[b], len(ref))
        assert np.max(np.abs(samples[b, :counts[b]] - ref)) < 1e-9 * np.max(np.abs(ref)), b
        assert abs(stats[b, 0] - info["max_climb_rate"]) < 1e-6 * max(1.0, info["max_climb_rate"])


# ---------------------------------------------------------------------------------------------------------- entry contracts


@pytest.mark.parametrize("B", [8194, 10002, 20002])
def test_sharded_entry_when_a_cut_falls_on_an_odd_trajectory(csp, B):
    """csp_minsnap_solve_batch_sharded with ngpu = 1: the device-resident form cuts its shard into chunks (two at B = 8194,
    four at 20002: cuts at 4097 / 5000.5 / 10001 before they were rounded to 64-trajectory slices) and must be bit-equal with
    the plain call on the fixed kernel (S = 16 and 15), the path kernel (status, max_dev), the generic and the chunked
    kernel.  The host-memory form at the same sizes."""
    import torch
    rng = np.random.default_rng(B)
    bc = torch.from_numpy(rng.normal(size=(B, 4, 3))).cuda()
    cases = ((16, dict(order=4), "fixed_"), (15, dict(order=4), "fixed_"),
             (16, dict(order=2, path_weight=1e-3, vel_zero_weight=0.01, bc=bc, want_status=True, want_max_dev=True), "fixedpath_"),
             (16, dict(order=4, force_generic=True, want_status=True), "generic_"), (40, dict(order=4), "chunked_"))
    for S, kw, fam in cases:
        wp, tm = synth.make_batch(B, S, config_id=97)
        d_wp, d_tm = torch.from_numpy(wp).cuda(), torch.from_numpy(tm).cuda()
        kw = dict(kw)
        b = kw.pop("bc", None)
        one = csp.solve_batch(d_wp, d_tm, b, **kw)
        sh = csp.solve_batch(d_wp, d_tm, b, ngpu=1, **kw)
        torch.cuda.synchronize()
        assert one.kernel.startswith(fam), (fam, one.kernel)
        assert torch.equal(one.coeffs, sh.coeffs), (B, S, kw)
        if kw.get("want_status"):
            assert torch.equal(one.status, sh.status)
        if kw.get("want_max_dev"):
            assert torch.equal(one.max_dev, sh.max_dev)
        if fam in ("fixed_", "generic_"):   # host-memory sharded form
            hb = b.cpu().numpy() if b is not None else None
            h1 = csp.solve_batch(wp, tm, hb, **kw)
            hs = csp.solve_batch(wp, tm, hb, ngpu=1, **kw)
            assert np.array_equal(h1.coeffs, hs.coeffs) and np.array_equal(h1.coeffs, one.coeffs.cpu().numpy()), (B, S, kw)


def test_mixed_entry_over_long_trajectories_in_both_forms(csp, oracle_mod):
    """Two trajectories longer than an explicit max_segments: the host and the device form both mark those two (only)
    CSP_TRAJ_SKIPPED, give the same coefficient offsets, leave the two blocks as they were and solve the others."""
    import torch
    lens = np.array([5, 12, 30, 7, 20, 1, 24, 40, 3])
    orders = np.array([2, 3, 4, 5, 2, 3, 4, 5, 3], dtype=np.int32)
    smax = 24
    long_ones = lens > smax
    assert np.flatnonzero(long_ones).tolist() == [2, 7]
    off, wps, tms = _ragged(lens, 55)
    wp, tm = np.concatenate(wps), np.concatenate(tms)
    total = csp.mixed_coeff_total(orders, off)
    host_out = np.full(total, -7.0)
    h = csp.solve_mixed(orders, wp, tm, off, max_segments=smax, want_status=True, out=host_out)
    d = [torch.from_numpy(x).cuda() for x in (orders, wp, tm, off)]
    p = csp.PreparedMixed(d[0], d[1], d[2], d[3], want_status=True, max_segments=smax)
    p.out.fill_(-7.0)
    p.run()
    torch.cuda.synchronize()
    cof_d, st_d, out_d = p.coeff_offsets.cpu().numpy(), p.status.cpu().numpy(), p.out.cpu().numpy()
    assert np.array_equal(h.coeff_offsets, cof_d)
    assert np.array_equal(h.status, st_d)
    assert (st_d[long_ones] == csp.TRAJ_SKIPPED).all() and not st_d[~long_ones].any(), st_d
    for out in (h.coeffs, out_d):
        for i in range(len(lens)):
            blk = out[cof_d[i]:cof_d[i + 1]]
            if long_ones[i]:
                assert (blk == -7.0).all(), i
                continue
            o, n = int(orders[i]), int(lens[i])
            ref, _ = oracle_mod.solve(o, wps[i], np.zeros((2, 3)), np.zeros((2, 3)), tms[i], long_double=o == 5)
            # the dense oracle's gates of tests/test_gpu_round3.py (measured here: 2.4e-10 per power)
            _gates(blk[:6 * o * n].reshape(n, 3, 2 * o), ref, 1e-6 if o == 5 else 5e-8, ("mixed skip", i, o, n))
    assert np.array_equal(h.coeffs, out_d)


@pytest.mark.parametrize("entry", sorted(_STAGED))
def test_host_and_device_memory_calls_are_bit_equal(csp, entry):
    """The host-memory form of an entry is its device-memory form behind a staging copy: the same inputs give the same
    bits in every output.  Smallest shapes at which the staging can go wrong: a uniform batch of one full 64-trajectory
    slice plus one (B = 65, S = 3) and a ragged one of lengths (1, 2, 5); every optional output absent and present;
    shared and per-trajectory bc; with and without per-trajectory weights; orders 2 and 4; fp64 and one fp32-storage
    case."""
    import ctypes
    import torch
    sym, ws_fn, args = _STAGED[entry]
    lib = csp.raw_lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    combos = [(order, False, lens, opt, bc_per, vw_per) for order in (2, 4) for lens in ((3,) * 65, (1, 2, 5))
              for opt in (False, True) for bc_per in (False, True) for vw_per in (False, True)]
    combos += [(4, True, (3,) * 65, True, True, True), (2, True, (1, 2, 5), True, False, True)]
    for k, (order, f32, lens, opt, bc_per, vw_per) in enumerate(combos):
        tag = (entry, order, "f32" if f32 else "f64", len(lens), opt, bc_per, vw_per)
        ragged = len(lens) == 3
        B = len(lens)
        host = _staged_buffers(entry, lens, order, f32, bc_per, 7000 + k)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        vw = np.random.default_rng(k).uniform(0.0, 0.3, size=B)
        dev = {n: torch.from_numpy(host[n]).cuda() for n, _, _ in args}
        d_off, d_vw = torch.from_numpy(off).cuda(), torch.from_numpy(vw).cuda()
        prm = csp.make_timeopt_params(csp.TIMEOPT_FIXED_TOTAL, min_time=0.01, tol=1e-6, max_iters=20)
        got = {}
        for form in ("host", "device"):
            ptr = (lambda n: host[n].ctypes.data) if form == "host" else (lambda n: dev[n].data_ptr())
            desc = csp.make_desc(order, B, 0 if ragged else lens[0], csp.DTYPE_F32 if f32 else csp.DTYPE_F64, 0.0, 0.02,
                                 csp.MEM_HOST if form == "host" else csp.MEM_DEVICE, bc_per,
                                 (off.ctypes.data if form == "host" else d_off.data_ptr()) if ragged else None,
                                 max(lens) if ragged else 0,
                                 (vw.ctypes.data if form == "host" else d_vw.data_ptr()) if vw_per else None)
            call = [ctypes.byref(desc)] + ([ctypes.byref(prm)] if entry == "optimize_times_batch" else [])
            call += [ptr(n) if (req or opt) else None for n, _, req in args]
            need = int(getattr(lib, ws_fn)(ctypes.byref(desc)))
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda") if form == "device" else None
            rc = getattr(lib, sym)(*call, ws.data_ptr() if ws is not None else None, need if ws is not None else 0, stream)
            assert rc == 0, (tag, form, rc, csp.strerror(rc))
            torch.cuda.synchronize()
            got[form] = {n: (host[n] if form == "host" else dev[n].cpu().numpy()) for n, kind, req in args
                         if kind == "out" and (req or opt)}
        # nothing failed (the optimiser may stop at max_iters: CSP_TRAJ_NOT_CONVERGED), so every output element was written;
        # the VJP without its optional outputs has none to compare: both forms returned CSP_OK
        assert not (got["host"].get("status", np.zeros(1, np.int32)) & ~csp.TRAJ_NOT_CONVERGED).any(), tag
        for n in got["host"]:
            assert got["host"][n].tobytes() == got["device"][n].tobytes(), (tag, n)


def _alt_problems(lens, seed):
    rng = np.random.default_rng(seed)
    xyz, elev = [], []
    for n in lens:
        xy = np.cumsum(rng.uniform(20, 60, size=(n, 2)), axis=0)
        z = 100 + np.cumsum(rng.normal(0, 8, n))
        e = 80 + 10 * np.sin(np.arange(n) / 5.0) + rng.normal(0, 2, n)
        if n > 7:
            e[rng.integers(0, n, max(1, n // 7))] = np.nan
        xyz.append(np.column_stack([xy, z])), elev.append(e)
    return xyz, elev


@pytest.mark.parametrize("lens", [[1, 2000], [1, 1, 1, 3000], [2000, 1, 3, 2, 1500], [5, 4097], [4, 2, 2900, 1]])
def test_altitude_cyclic_reduction_with_short_problems(csp, lens):
    """Short problems ahead of, between and after long ones take the cyclic-reduction path (at most 64 problems averaging
    at least 512 samples, alt.hip: use_cr); each against the CPU oracle at 1e-8 relative, with the same number of
    active-set solves, in host and device memory."""
    import torch
    assert len(lens) <= 64 and sum(lens) >= 512 * len(lens), "not the cyclic-reduction path"
    xyz, elev = _alt_problems(lens, sum(lens))
    X, E = np.concatenate(xyz), np.concatenate(elev)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    zin = X[:, 2].copy()
    refs_o, refs_g = [], []
    for k, n in enumerate(lens):
        banded = n > 777
        refs_o.append(oracle.alt_optimize(xyz[k], elev[k], 1.0, 0.5, 50.0, 2.0, banded=banded))
        refs_g.append(oracle.alt_global_smooth(xyz[k][:, 2], xyz[k], 1.0, 2.0, banded=banded))
    d = [torch.from_numpy(x).cuda() for x in (X, E, off, zin)]
    for form in ("host", "device"):
        if form == "host":
            zo = csp.alt_optimize_heights_batch(X, E, off, 1.0, 0.5, 50.0, 2.0)
            zg, sv = csp.alt_global_smooth_batch(zin, X, off, 1.0, 2.0)
        else:
            zo = csp.alt_optimize_heights_batch(d[0], d[1], d[2], 1.0, 0.5, 50.0, 2.0).cpu().numpy()
            zg, sv = csp.alt_global_smooth_batch(d[3], d[0], d[2], 1.0, 2.0)
            zg, sv = zg.cpu().numpy(), sv.cpu().numpy()
        for k, n in enumerate(lens):
            ro, (rg, nref) = refs_o[k], refs_g[k]
            assert np.max(np.abs(zo[off[k]:off[k + 1]] - ro)) <= 1e-8 * np.max(np.abs(ro)), (form, "optimize", k, n)
            assert np.max(np.abs(zg[off[k]:off[k + 1]] - rg)) <= 1e-8 * np.max(np.abs(rg)), (form, "global smooth", k, n)
            assert int(sv[k]) == nref, (form, k, n, int(sv[k]), nref)
