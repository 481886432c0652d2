"""Memory, edge and bad-input contracts of csp_bezier_generate_batch (include/csp_bezier.h), driven through raw pointers
with waypoints, offsets, samples and counts each inside a guarded carve (tests/guarded.py) of exactly its size.

Loop bounds of bezier_kernel (read in cs-pathplan_amd/csrc/bezier.hip), whatever the waypoints hold:
  - the round loop `s0 < n - 1; s0 += 64` and the heading / point loads depend on the path's point count n, which comes
    from `offsets` (a launch argument of the caller), not from the coordinates;
  - the curvature loop makes at most 10 attempts, the prefix sum 6 shuffles;
  - the two parameter loops `for (t = 0; t <= 1; t += step)` run only when step >= 2^-24.  Then t + step > t for every
    t <= 1 (an ulp of t is at most 2^-52), so t grows by at least 2^-24 (1 - 2^-28) per trip and the loop ends after at
    most 2^24 + 1 trips.  A NaN, zero or negative step (NaN or infinite length) fails `step >= 2^-24` and gives no
    samples; a positive step below 2^-24 -- a coordinate like 1e15 -- is not walked either and the path's count becomes
    CSP_BEZIER_UNSAMPLEABLE.  Before that change such a step below an ulp of t (t + step == t) never left the loop.
No test here aims at a fault or a hang: the oversize inputs are only ever given to the bounded kernel, and the 64 KiB
band is larger than a whole path's rows (capacity * 24 bytes <= ~35 KB here), so a misplaced path stays inside the
test's own allocation.

Counts are compared EXACTLY with tests/test_dropin_callsites.py::bezier_reference_py.  A count is the number of trips of
the accumulated parameter loop, so a last-ulp difference between the device's and the host's sin / cos / hypot could
change it when the final t lands within rounding of 1.  _assert_counts_are_stable proves on the CPU, inside each test,
that every segment's count is the same with `step` moved by -4 .. +4 ulps: such a difference cannot decide a count here.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.staged import Carved, check_carves
from tests.test_dropin_callsites import bezier_reference_py

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 2 ** 31 - 1      # CSP_BEZIER_UNSAMPLEABLE
SEGMENTS = (1, 63, 64, 65, 128, 129)    # both sides of the 64-segments-per-round boundary, one and two full rounds


def _path(rng, npts, scale):
    p = np.cumsum(rng.normal(size=(npts, 3)) * scale, axis=0) + rng.uniform(-100, 100, size=3)
    p[:, 2] = 100.0 + np.abs(p[:, 2]) * 0.05
    return p


def _paths(seed):
    """One path per entry of SEGMENTS, a path of one point (no samples), and a path whose FIRST leg is shorter than 0.1
    in the plane (it contributes its end point and the next segment still drops its first sample)."""
    rng = np.random.default_rng(seed)
    paths = [_path(rng, s + 1, 120.0) for s in SEGMENTS]
    paths.append(_path(rng, 1, 1.0))
    paths.append(np.array([[10.0, 20.0, 100.0], [10.05, 20.03, 101.0], [80.0, 30.0, 104.0], [150.0, -20.0, 110.0]]))
    return paths


def _segment_counts(P, resolution, ks, ulps=0):
    """Samples each segment contributes in the restatement (its own parameter loop; `ks` are the arm factors that
    bezier_reference_py chose), with `step` moved by `ulps` units in the last place."""
    n = len(P)
    hd = []
    for i in range(n):
        lo, hi = max(i - 1, 0), min(i + 1, n - 1)
        hd.append(math.atan2(P[hi][1] - P[lo][1], P[hi][0] - P[lo][0]))
    out = []
    for i in range(n - 1):
        p0, p3, k = P[i], P[i + 1], ks[i]
        dis = math.hypot(p0[0] - p3[0], p0[1] - p3[1])
        if k is None:
            out.append(1)
            continue
        p1 = (p0[0] + math.cos(hd[i]) * dis * k, p0[1] + math.sin(hd[i]) * dis * k)
        p2 = (p3[0] - math.cos(hd[i + 1]) * dis * k, p3[1] - math.sin(hd[i + 1]) * dis * k)
        step = resolution / (math.hypot(p2[0] - p1[0], p2[1] - p1[1]) + dis * 2.0 / 3.0)
        for _ in range(abs(ulps)):
            step = np.nextafter(step, np.inf if ulps > 0 else 0.0)
        step, t, c = float(step), 0.0, 0
        while t <= 1.0:
            c += 1
            t += step
        out.append(c - (1 if i > 0 else 0))
    return out


def _reference(paths, resolution, min_radius):
    """[(samples, per-segment counts)] of the restatement; asserts that no count depends on the last ulps of step."""
    refs = []
    for p in paths:
        if len(p) < 2:
            refs.append((np.zeros((0, 3)), []))
            continue
        s, ks = bezier_reference_py(p.tolist(), resolution, min_radius)
        per = _segment_counts(p.tolist(), resolution, ks)
        assert sum(per) == len(s)
        for u in (-4, -1, 1, 4):
            assert _segment_counts(p.tolist(), resolution, ks, u) == per, ("a count depends on the last ulps of step", len(p), u)
        refs.append((s, per))
    return refs


def _flatten(paths):
    return np.concatenate(paths), np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)


def _call(csp, wp, off, resolution, min_radius, capacity, fill):
    """One device-memory call with every buffer in a carve of exactly its size, samples and counts starting as `fill`
    bytes: return code 0, no guard byte and no input byte changed.  Returns (samples [B, capacity, 3], counts [B])."""
    B = len(off) - 1
    g_wp, g_off = Carved(wp, DEV, "waypoints"), Carved(off, DEV, "offsets")
    g_s = Carved(np.zeros((B, capacity, 3)), DEV, "samples", fill)
    g_c = Carved(np.zeros(B, np.int32), DEV, "counts", fill)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = csp.raw_lib().csp_bezier_generate_batch(g_wp.data_ptr(), g_off.data_ptr(), B, float(resolution), float(min_radius), int(capacity),
                                                 g_s.data_ptr(), g_c.data_ptr(), csp.MEM_DEVICE, -1, stream)
    assert rc == 0, (rc, csp.strerror(rc))
    torch.cuda.synchronize()
    check_carves(("bezier", B, capacity, hex(fill)), [g_wp, g_off, g_s, g_c], [g_wp, g_off])
    return g_s.numpy(), g_c.numpy()


def _untouched(rows, fill):
    return bool((rows.reshape(-1).view(np.uint8) == fill).all())


@pytest.mark.parametrize("min_radius", [1.0, 300.0])
def test_round_boundaries_capacities_and_stale_rows(csp, min_radius):
    """Paths of 1, 63, 64, 65, 128 and 129 segments (plus an empty one and one with a short first leg) at every capacity
    that is some path's count or one less, at 1 and at the largest count + 3, samples and counts starting 0x00- and
    0xFF-filled: counts are the restatement's whatever the capacity; rows below min(count, capacity) match the
    restatement to 1e-9 relative, are the same bits at every capacity and for both fills, and are bit-equal with the
    Python binding's device call; rows at and past min(count, capacity) still hold the fill, byte for byte."""
    resolution = 25.0
    paths = _paths(31)
    refs = _reference(paths, resolution, min_radius)
    want = np.array([len(s) for s, _ in refs], np.int32)
    assert want[len(SEGMENTS)] == 0 and refs[-1][1][0] == 1          # the empty path; the short first leg's end point
    wp, off = _flatten(paths)
    big = int(want.max()) + 3
    caps = sorted({1, big} | {int(c) for c in want if c > 0} | {int(c) - 1 for c in want if c > 1})
    full, _ = _call(csp, wp, off, resolution, min_radius, big, 0x00)
    s_b, n_b = csp.bezier_generate_batch(torch.from_numpy(wp).to(DEV), torch.from_numpy(off).to(DEV), resolution, min_radius, big)
    torch.cuda.synchronize()
    assert np.array_equal(n_b.cpu().numpy(), want)
    assert np.array_equal(s_b.cpu().numpy(), full)                   # the binding zero-fills, like the 0x00 start
    for b, (s, _) in enumerate(refs):
        if len(s):
            assert np.max(np.abs(full[b, :len(s)] - s)) <= 1e-9 * np.max(np.abs(s)), b
    for cap in caps:
        for fill in (0x00, 0xFF):
            got, n = _call(csp, wp, off, resolution, min_radius, cap, fill)
            assert np.array_equal(n, want), (cap, fill, n, want)
            for b in range(len(paths)):
                k = min(int(want[b]), cap)
                assert np.array_equal(got[b, :k], full[b, :k]), (cap, fill, b)
                assert _untouched(got[b, k:], fill), (cap, fill, b, "rows past min(count, capacity) were written")


def _benign_batch(seed):
    rng = np.random.default_rng(seed)
    return [_path(rng, n, 120.0) for n in (9, 66, 2, 70, 5)]


@pytest.mark.parametrize("bad,where", [(1e15, 33), (float("nan"), 33), (float("inf"), 33), (-1e15, 65), (1e15, 0)])
def test_one_bad_path_leaves_the_others_alone(csp, bad, where):
    """Path 1 (65 segments, two rounds) gets one x coordinate of 1e15, NaN or inf -- in the first round, in the second
    round's only segment or at the first point.  Every other path's rows, untouched rows and counts are bit-equal to the
    benign run; nothing outside path 1's own `capacity` rows is written (guard bands, fill pattern).

    1e15: the two legs at that waypoint have a step of ~2.5e-14 < 2^-24, so counts[1] is CSP_BEZIER_UNSAMPLEABLE.
    NaN at waypoint j: legs j-1 and j have a NaN chord, which fails `chord >= 0.1`: one (end point) row each, as for a
    short leg; legs j-2 and j+1 get a NaN heading, a NaN length and no samples; the other legs keep their counts, so
    counts[1] is their sum + 2.  inf: legs j-1 and j have an infinite or NaN length (step 0 or NaN) and no samples; legs
    j-2 and j+1 are walked with a heading of 0, pi or +-pi/2, so counts[1] is at least the sum over the untouched legs
    and not the sentinel."""
    resolution, min_radius, fill = 25.0, 300.0, 0xFF
    good = _benign_batch(77)
    refs = _reference(good, resolution, min_radius)
    want = np.array([len(s) for s, _ in refs], np.int32)
    cap = int(want.max()) + 3
    paths = [p.copy() for p in good]
    paths[1][where, 0] = bad
    wp_g, off = _flatten(good)
    wp_b, _ = _flatten(paths)
    s_g, n_g = _call(csp, wp_g, off, resolution, min_radius, cap, fill)
    s_b, n_b = _call(csp, wp_b, off, resolution, min_radius, cap, fill)
    assert np.array_equal(n_g, want)
    others = [0, 2, 3, 4]
    assert np.array_equal(n_b[others], n_g[others]), (n_b, n_g)
    assert s_b[others].tobytes() == s_g[others].tobytes(), "the bad path disturbed another path"
    per = refs[1][1]
    untouched = sum(c for i, c in enumerate(per) if not (where - 2 <= i <= where + 1))
    print("bad =", bad, "at waypoint", where, "-> counts[1] =", int(n_b[1]), "(benign %d)" % want[1])
    if np.isnan(bad):
        assert n_b[1] == untouched + 2, (n_b[1], untouched)
    elif np.isinf(bad):
        assert untouched <= n_b[1] < SENTINEL, (n_b[1], untouched)
    else:
        assert n_b[1] == SENTINEL, n_b[1]


def test_a_long_legitimate_segment_returns_its_true_count(csp):
    """One leg of 3e5 m at resolution 1 (a step of ~3.3e-6, far above 2^-24) between two ordinary legs, capacity 16: the
    true count (~3e5) comes back, exactly the restatement's, and the 16 rows are the restatement's first 16."""
    P = np.array([[0.0, 0.0, 100.0], [40.0, 5.0, 101.0], [300040.0, 1234.5, 150.0], [300090.0, 1200.0, 151.0]])
    (s, per), = _reference([P], 1.0, 1.0)
    assert 2.9e5 < per[1] < 3.5e5, per
    wp, off = _flatten([P])
    got, n = _call(csp, wp, off, 1.0, 1.0, 16, 0xFF)
    assert n[0] == len(s), (n[0], len(s))
    assert np.max(np.abs(got[0] - s[:16])) <= 1e-9 * np.max(np.abs(s[:16]))
