"""Memory, isolation, edge and precision contracts of csp_alt_optimize_heights_batch and csp_alt_global_smooth_batch
(include/csp_alt.h; cs-pathplan_amd/csrc/alt.hip: three device mappings -- one lane, one wave or one 1024-thread
workgroup (block cyclic reduction) per problem), driven through raw pointers with every buffer inside a guarded carve
(tests/guarded.py) and the workspace at exactly csp_alt_workspace_bytes(total).

The band is 256 KiB: the largest problem here, n = 2915, owns (15 * 1458 + 2 + 2915) * 8 = 198 296 bytes of workspace
(alt_cr_layout.h), so one whole misplaced region -- and any row of the 32-byte-per-sample recurrence layout shifted by a
whole problem -- still lands inside the test's own allocation.  No test aims at a fault.

Arms (the smallest shapes that reach each path; dispatch rules of alt.hip: cyclic reduction when batch <= 64 and total >=
512 * batch, else one wave per problem when batch < 2048, else one lane per problem):
    lane        batch 2048 + 5, lengths cycling through (1, 2, 3, 7, 8, 9, 16, 17, 65): both sides of the 8-row blocks
    wave        batch 9, lengths (1, 2, 3, 63, 64, 65, 128, 129, 200): both sides of the 64-row rounds
    cr, LDS     [2914] (the last length whose 13 * 8 * ceil(n / 2) bytes fit in 148 KiB), [1023], [1024], [1025] (block rows
                around the 512 = 1024 / 2 pairs that one pass of the 1024 threads covers)
    cr, global  [2915] (the first length in the workspace), [1, 2915, 2, 1024, 1025] (both stores in one call)

Contracts: A guard bands, B stale memory, C isolation of one non-finite problem, D empty problems, E parameter edges
against tests/alt_ref.py, F precision against tests/alt_ref.py, G the stiff case, and the dispatch edges.

Precision gate (F, G, E): with e(x) = max|x - ref| / max|ref| against the mpmath reference, e_kernel <= K * e_oracle +
FLOOR, where e_oracle is the error of the fp64 C oracle (dense Cholesky up to 777 samples, banded beyond) on the same
problem and FLOOR = 8 * 2^-52 (a few ulps of the largest value: the final rounding of any fp64 code).  K = 10 for every
case but one: twice the worst ratio measured elsewhere on an MI355X (4.86).  The exception has its own named constant,
K_STIFF_RECURRENCE_GLOBAL = 50, for the global smooth of the 80-sample stiff problem on the lane / wave kernels (measured
21.75).  Measured e_kernel / max(e_oracle, FLOOR), worst over an arm's problems, optimize / global smooth (DESIGN.md
section 16 has the full table):
    lane 1.05 / 1.41      wave 1.98 / 1.95      cr [1023] 0.81 / 0.91   cr [1024] 1.23 / 0.64   cr [1025] 0.96 / 0.17
    cr [2914] 1.00 / 0.42                       cr [2915] 1.31 / 1.55   cr [1, 2915, 2, 1024, 1025] 1.95 / 4.86
    dispatch edge 64 | 65: cr <= 1.38, wave <= 1.89         active-set growth: lane 0.20 (5 solves), cr 4.75 (4 solves)
    stiff g = 1e-3: wave = lane 0.90 / 21.75, cr 0.22 / 0.95        stiff g = 1e-5: wave = lane 0.38 / 13.05, cr 0.24 / 0.98
    parameter edges, worst over both entries: wave = lane 4.61 (max_climb_rate = 0), 1.19 (repeated xy), 1.09 (lambda_smooth
    = 0), 0.07 (both zero), 0 (lambda_follow = 0, all-NaN elev: exact zeros); cr (n = 600) 0.92 at most
The one ratio above 10: e_kernel 2.6e-14 against e_oracle 1.2e-15, the same 2.6e-14 at g = 1e-3 and 1e-5, so it does
not scale with the stiff pair, and the cyclic reduction (with its determinant pivot) is at 0.95 on its own stiff
problem.  What is known beyond that: a line-by-line fp64 restatement of banded_solve, run once on the CPU with IEEE
division (not committed), was 1.3e-14 from mpmath on the same problem -- about half of the kernel's figure, so the
recurrence's form accounts for a ratio of ~11 and the fused multiply-adds and the Newton reciprocal rcp64 for a further
factor of ~2 that was not separated.  Over 40 problems of that kind the restatement's ratio to the oracle reached 5.5
(median 1.4).  The likely cause is the mild ill-conditioning of runs of free samples between samples pinned at 1e8;
that is a reading of these figures, not a proof.
Solve counts of the global smooth are compared exactly, and only for cases whose tie margin from alt_ref (the smallest
distance of a not-yet-active z_i from the threshold zin_i - 1e-3) exceeds 100 * e_oracle * max|z|: asserted per case.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
from tests import alt_ref, guarded
from tests.staged import Carved, check_carves
from tests.test_alt import _problem

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAND = 256 * 1024
K_GATE = 10.0                     # every case but one: twice the worst ratio measured elsewhere (4.86)
K_STIFF_RECURRENCE_GLOBAL = 50.0  # the global smooth of the 80-sample stiff problem on the lane / wave kernels: measured 21.75
FLOOR = 8 * 2.0 ** -52
OPT = (1.0, 0.5, 50.0, 2.0)        # lambda_smooth, lambda_follow, safe_distance, max_climb_rate
GLB = (1.0, 2.0)                   # lambda_smooth, max_climb_rate
LANE_CYCLE = (1, 2, 3, 7, 8, 9, 16, 17, 65)
WAVE_LENS = (1, 2, 3, 63, 64, 65, 128, 129, 200)
ARMS = {
    "lane": tuple(LANE_CYCLE[i % 9] for i in range(2048 + 5)),
    "wave": WAVE_LENS,
    "cr_lds_2914": (2914,), "cr_lds_1023": (1023,), "cr_lds_1024": (1024,), "cr_lds_1025": (1025,),
    "cr_ws_2915": (2915,), "cr_ws_mixed": (1, 2915, 2, 1024, 1025),
}
ENTRIES = ("optimize", "global")


def mapping(lens):
    """The device mapping alt.hip picks for a batch (use_cr, kWaveBatch)."""
    B, total = len(lens), int(np.sum(lens))
    if B <= 64 and total >= 512 * B:
        return "cr"
    return "wave" if B < 2048 else "lane"


for _arm, _lens in ARMS.items():
    assert mapping(_lens) == _arm.split("_")[0], _arm


class Batch:
    """Problems of `lens` samples from tests/test_alt.py::_problem (advancing xy, random-walk z, terrain with gaps)."""

    def __init__(self, lens, seed):
        rng = np.random.default_rng(seed)
        self.lens = tuple(int(n) for n in lens)
        probs = [_problem(rng, n, with_gaps=n > 3) if n else (np.zeros((0, 3)), np.zeros(0)) for n in self.lens]
        self.xyz = np.concatenate([p[0] for p in probs]).reshape(-1, 3)
        self.elev = np.concatenate([p[1] for p in probs])
        self.zin = self.xyz[:, 2] + rng.uniform(0.0, 10.0, len(self.xyz))
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)

    @classmethod
    def of(cls, lens, xyz, elev, zin):
        """A batch of given data (contiguous fp64 copies)."""
        c = cls.__new__(cls)
        c.lens = tuple(int(n) for n in lens)
        c.xyz = np.array(xyz, dtype=np.float64).reshape(-1, 3)
        c.elev, c.zin = np.array(elev, dtype=np.float64), np.array(zin, dtype=np.float64)
        c.off = np.concatenate([[0], np.cumsum(c.lens)]).astype(np.int64)
        assert len(c.xyz) == len(c.elev) == len(c.zin) == c.off[-1]
        return c

    def copy(self):
        return Batch.of(self.lens, self.xyz, self.elev, self.zin)

    def sub(self, picks):
        """The batch of the problems `picks`, in that order."""
        sel = np.concatenate([np.arange(self.off[k], self.off[k + 1]) for k in picks] + [np.zeros(0, np.int64)]).astype(np.int64)
        return Batch.of([self.lens[k] for k in picks], self.xyz[sel], self.elev[sel], self.zin[sel])

    def problem(self, k):
        s = slice(self.off[k], self.off[k + 1])
        return self.xyz[s], self.elev[s], self.zin[s]


@functools.lru_cache(maxsize=None)
def arm_batch(arm):
    return Batch(ARMS[arm], 700 + sorted(ARMS).index(arm))


def run(csp, entry, batch, params=None, fill=0xFF):
    """One device-memory call of `entry` with the workspace carved at exactly csp_alt_workspace_bytes(total), out_z and
    solves at their exact sizes and the inputs in carves too; workspace and outputs start as `fill` bytes.  Asserts the
    return code, every guard band and that no input byte changed.  Returns (out_z, solves or None)."""
    lib = csp.raw_lib()
    params = params if params is not None else (OPT if entry == "optimize" else GLB)
    total, B = len(batch.xyz), len(batch.lens)
    need = int(lib.csp_alt_workspace_bytes(total))
    ws = guarded.Guarded(need, DEV, BAND, name="workspace").fill(fill)
    g_xyz, g_off = Carved(batch.xyz, DEV, "xyz", None, BAND), Carved(batch.off, DEV, "offsets", None, BAND)
    g_a = Carved(batch.elev if entry == "optimize" else batch.zin, DEV, "elev" if entry == "optimize" else "input_z", None, BAND)
    g_out = Carved(np.zeros(total), DEV, "out_z", fill, BAND)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    carves, g_sv = [ws, g_xyz, g_off, g_a, g_out], None
    if entry == "optimize":
        p = csp.AltParams(*[float(v) for v in params])
        rc = lib.csp_alt_optimize_heights_batch(g_xyz.data_ptr(), g_a.data_ptr(), g_off.data_ptr(), B, ctypes.byref(p), g_out.data_ptr(),
                                                ws.data_ptr(), need, csp.MEM_DEVICE, -1, stream)
    else:
        p = csp.AltParams(float(params[0]), 0.0, 0.0, float(params[1]))
        g_sv = Carved(np.zeros(B, np.int32), DEV, "solves", fill, BAND)
        carves.append(g_sv)
        rc = lib.csp_alt_global_smooth_batch(g_a.data_ptr(), g_xyz.data_ptr(), g_off.data_ptr(), B, ctypes.byref(p), g_out.data_ptr(),
                                             g_sv.data_ptr(), ws.data_ptr(), need, csp.MEM_DEVICE, -1, stream)
    assert rc == 0, (entry, rc, csp.strerror(rc))
    torch.cuda.synchronize()
    check_carves((entry, B, total, "workspace %d bytes" % need, hex(fill)), carves, [g_xyz, g_off, g_a])
    return g_out.numpy(), (g_sv.numpy() if g_sv is not None else None)


def binding(csp, entry, batch, params=None):
    """The Python binding's device-memory call for the same inputs."""
    params = params if params is not None else (OPT if entry == "optimize" else GLB)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    if entry == "optimize":
        z, sv = csp.alt_optimize_heights_batch(d(batch.xyz), d(batch.elev), d(batch.off), *params), None
    else:
        z, sv = csp.alt_global_smooth_batch(d(batch.zin), d(batch.xyz), d(batch.off), *params)
    torch.cuda.synchronize()
    return z.cpu().numpy(), (sv.cpu().numpy() if sv is not None else None)


def reference(entry, xyz, a, params):
    """(alt_ref result, oracle result, alt_ref solves, oracle solves, tie margin) of one problem; solves None for optimize."""
    banded = len(a) > 777
    if entry == "optimize":
        return alt_ref.optimize(xyz, a, *params), oracle.alt_optimize(xyz, a, *params, banded=banded), None, None, None
    zr, kr, margin = alt_ref.global_smooth(a, xyz, *params)
    try:
        zo, ko = oracle.alt_global_smooth(a, xyz, *params, banded=banded)
    except ValueError:      # the oracle's Cholesky met a non-positive pivot (the stiffest recorded-only cases)
        zo, ko = np.full(len(a), np.nan), -1
    return zr, zo, kr, ko, margin


def gate(tag, got, solves, ref, want_count=True, k=K_GATE):
    """Prints the figures, then asserts e_kernel <= k e_oracle + FLOOR and, for the global smooth, the margin rule and
    equal solve counts (want_count=False: the values only, for a case the margin rule excludes from the count
    comparison -- the caller proves that it does).  Returns (e_kernel, e_oracle)."""
    zr, zo, kr, ko, margin = ref
    e_o, e_k = alt_ref.rel_err(zo, zr), alt_ref.rel_err(got, zr)
    ratio = e_k / e_o if e_o > 0 else (0.0 if e_k == 0 else float("inf"))
    print("%-44s e_oracle %.3e  e_kernel %.3e  ratio %8.2f%s" % (tag, e_o, e_k, ratio,
          "" if kr is None else "  solves %d/%d/%s margin %.2e" % (kr, ko, solves, margin)))
    assert np.isfinite(got).all(), tag
    if kr is not None and want_count:
        assert margin > 100 * e_o * np.max(np.abs(zr)), (tag, "too close to a tie for an exact solve count", margin, e_o)
        assert kr == ko == solves, (tag, kr, ko, solves)
    assert e_k <= k * e_o + FLOOR, (tag, k, e_k, e_o)
    return e_k, e_o


# --------------------------------------------------------------------------------------------------- A. guard bands


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("arm", sorted(ARMS))
def test_guard_bands(csp, arm, entry):
    """Workspace at exactly csp_alt_workspace_bytes(total), out_z and solves at their exact sizes, the inputs carved too,
    256 KiB of 0xA5 around each: no band byte and no input byte changes, and the results are bit-equal with the Python
    binding's device-memory call, so the guarded call ran the same kernel."""
    b = arm_batch(arm)
    z, sv = run(csp, entry, b, fill=0x5A)
    zb, svb = binding(csp, entry, b)
    assert z.tobytes() == zb.tobytes(), (arm, entry)
    if sv is not None:
        assert np.array_equal(sv, svb) and sv.min() >= 1 and sv.max() <= 10, (arm, sv)


# -------------------------------------------------------------------------------------------------- B. stale memory


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("arm", sorted(ARMS))
def test_independent_of_stale_memory(csp, arm, entry):
    """The same call over a 0x00-filled and over a 0xFF-filled (NaN / -1) workspace, out_z and solves gives the same bits,
    and no all-ones element survives: the active flags, the cyclic reduction's block rows and solution, and every
    element of the outputs are written before they are read."""
    b = arm_batch(arm)
    (z0, s0), (z1, s1) = run(csp, entry, b, fill=0x00), run(csp, entry, b, fill=0xFF)
    assert z0.tobytes() == z1.tobytes(), (arm, entry, "differs between a 0x00 and a 0xFF start")
    assert not (z1.view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)).any(), (arm, entry, "stale out_z")
    assert np.isfinite(z1).all(), (arm, entry)
    if s0 is not None:
        assert np.array_equal(s0, s1) and (s1 >= 1).all(), (arm, s0, s1)


# ------------------------------------------------------------------------------------------------------ C. isolation


BAD = {"lane": 70, "wave": 4, "cr_ws_mixed": 1}


# an inf in z only for optimize: the global-smooth kernels never read xyz's third column
BAD_KINDS = [(e, k) for e in ENTRIES for k in ("xy_nan", "xy_inf", "z_inf", "a_nan", "a_inf") if not (e == "global" and k == "z_inf")]


@pytest.mark.parametrize("entry,kind", BAD_KINDS)
@pytest.mark.parametrize("arm", sorted(BAD))
def test_one_bad_problem_leaves_the_others_alone(csp, arm, entry, kind):
    """One problem of the batch (mid-wave in the lane arm, the 64-sample one in the wave arm, the 2915-sample one whose
    block rows live in the workspace in the cyclic-reduction arm) carries a NaN or an inf in one x coordinate, an inf in
    one z (optimize only: the global smooth does not read z), or a NaN / inf in elev or input_z.  Offsets stay benign.  Every other problem is bit-equal to the benign run,
    solve counts included; the bad problem's own solve count stays within 1..10.

    Loop bounds (read in alt.hip): banded_solve and banded_solve_wave sweep i0 < n forwards and i0 >= 0 backwards in
    steps of 8 / 64 with inner loops of 8 / at most 64 rows; the post-check and active-set scans run over i < n; the
    active-set loop makes at most 10 passes (a comparison with NaN is false: no new violation, the loop ends early);
    cr_solve's level loops double / halve st below N2 = ceil(n / 2) and its row loops stride up to N2.  Nothing is bounded
    by a value computed from the data, so non-finite data cannot extend any loop."""
    good = arm_batch(arm)
    bad = good.copy()
    k = BAD[arm]
    i = int(good.off[k]) + good.lens[k] // 2
    if kind.startswith("a_"):
        arr = bad.elev if entry == "optimize" else bad.zin
        arr[i] = np.nan if kind == "a_nan" else np.inf
    else:
        bad.xyz[i, 2 if kind == "z_inf" else 0] = np.nan if kind == "xy_nan" else np.inf
    zg, sg = run(csp, entry, good)
    zb, sb = run(csp, entry, bad)
    keep = np.ones(len(zg), bool)
    keep[good.off[k]:good.off[k + 1]] = False
    assert zb[keep].tobytes() == zg[keep].tobytes(), (arm, entry, kind, "the bad problem disturbed another problem")
    if sg is not None:
        others = np.arange(len(sg)) != k
        assert np.array_equal(sb[others], sg[others]) and 1 <= sb[k] <= 10, (arm, kind, sb[k])


# ------------------------------------------------------------------------------------------- D. empty and tiny problems


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", ["wave_3050", "lane_3050", "cr_0_2915"])
def test_empty_problems(csp, shape, entry):
    """Lengths (3, 0, 5, 0) in the wave arm, the same four tiled 513 times (2052 problems) in the lane arm, and (0, 2915) in
    the cyclic-reduction arm: solves is 0 for the empty problems (0xFF-filled before the call, so it was written), the
    others are bit-equal to the call without the empty ones, and no guard byte changes.

    Why this cannot fault (read in alt.hip): every kernel reads offsets[b] and offsets[b + 1] -- B + 1 carved entries --
    and returns on n <= 0 before it forms any other address (the global-smooth kernels first store solves[b] = 0, inside
    its B entries); cr_region is not evaluated for an empty problem, and an empty problem's region would be empty anyway.
    The device-memory form builds no HostCall; the host form registers its buffers by byte counts taken from
    offsets[batch], so empty problems add nothing there either.  total > 0 in all three shapes, so the workspace is never
    the zero-byte one."""
    if shape == "cr_0_2915":
        full = Batch((0, 2915), 811)
    else:
        full = Batch((3, 0, 5, 0) * (1 if shape.startswith("wave") else 513), 812)
    assert mapping(full.lens) == shape.split("_")[0]
    nonempty = [k for k, n in enumerate(full.lens) if n]
    dense = full.sub(nonempty)
    zf, sf = run(csp, entry, full)
    zd, sd = run(csp, entry, dense)
    assert zf.tobytes() == zd.tobytes() and np.isfinite(zf).all(), (shape, entry)
    if sf is not None:
        empty = np.array([n == 0 for n in full.lens])
        assert (sf[empty] == 0).all() and np.array_equal(sf[~empty], sd) and (sd >= 1).all(), (shape, sf[:8])


# ----------------------------------------------------------------------------------------------------- dispatch edges


def test_dispatch_edges(csp):
    """The same problems on both sides of every switch of the host's kernel choice.
    batch 64 | 65 and total = 512 batch | one less: 65 problems of 512 samples.  The first 64 run cyclic reduction; the
    first 63 plus the 64th cut to 511 samples (total 64 * 512 - 1), and all 65, run one wave per problem.  The two wave
    runs agree bit for bit on the 63 problems they share, solve counts included; problems 0, 62 and 63 of the cyclic
    reduction and of the wave run are each held against tests/alt_ref.py at the module's precision gate, and the solve
    counts of the two mappings are equal on all 64.
    batch 2047 | 2048: the lane arm's first 2047 problems (wave) and first 2048 (lane) agree bit for bit on the 2047."""
    b65 = Batch((512,) * 65, 900)
    assert mapping(b65.lens[:64]) == "cr" and mapping(b65.lens) == "wave"
    b64 = b65.sub(range(64))
    cut = Batch.of(b64.lens[:63] + (511,), b64.xyz[:-1], b64.elev[:-1], b64.zin[:-1])
    assert mapping(cut.lens) == "wave"
    n63 = 63 * 512
    for entry in ENTRIES:
        z_cr, s_cr = run(csp, entry, b64)
        z_cut, s_cut = run(csp, entry, cut)
        z_65, s_65 = run(csp, entry, b65)
        assert z_cut[:n63].tobytes() == z_65[:n63].tobytes(), entry
        for k in (0, 62, 63):
            xyz, elev, zin = b65.problem(k)
            ref = reference(entry, xyz, elev if entry == "optimize" else zin, OPT if entry == "optimize" else GLB)
            sl = slice(b65.off[k], b65.off[k + 1])
            gate("edge 64|65 cr   %s problem %d" % (entry, k), z_cr[sl], None if s_cr is None else int(s_cr[k]), ref)
            gate("edge 64|65 wave %s problem %d" % (entry, k), z_65[sl], None if s_65 is None else int(s_65[k]), ref)
        if s_cr is not None:
            assert np.array_equal(s_cut[:63], s_65[:63]) and np.array_equal(s_cr, s_65[:64]), entry
    lane = arm_batch("lane")
    b2047, b2048 = lane.sub(range(2047)), lane.sub(range(2048))
    assert mapping(b2047.lens) == "wave" and mapping(b2048.lens) == "lane"
    m = len(b2047.xyz)
    for entry in ENTRIES:
        (zw, sw), (zl, sl) = run(csp, entry, b2047), run(csp, entry, b2048)
        assert zw.tobytes() == zl[:m].tobytes(), entry
        if sw is not None:
            assert np.array_equal(sw, sl[:2047]), entry


# ------------------------------------------------------------------------------------------ F. precision against mpmath


def _picks(arm):
    """The problems of an arm that get an mpmath reference: all, except in the lane arm (three of each length and the
    last problem; the others are the same code on the same lengths)."""
    return list(range(27)) + [len(ARMS[arm]) - 1] if arm == "lane" else list(range(len(ARMS[arm])))


@functools.lru_cache(maxsize=None)
def _arm_reference(arm, entry):
    b = arm_batch(arm)
    out = {}
    for k in _picks(arm):
        xyz, elev, zin = b.problem(k)
        out[k] = reference(entry, xyz, elev if entry == "optimize" else zin, OPT if entry == "optimize" else GLB)
    return out


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("arm", sorted(ARMS))
def test_precision_against_mpmath(csp, arm, entry):
    """Every arm's problems against tests/alt_ref.py at the gate of the module docstring, problem by problem; solve counts
    equal to alt_ref's and the oracle's wherever the tie margin allows the comparison (asserted)."""
    b = arm_batch(arm)
    z, sv = run(csp, entry, b)
    worst = 0.0
    for k, ref in _arm_reference(arm, entry).items():
        s = slice(b.off[k], b.off[k + 1])
        e_k, e_o = gate("%s %s problem %d n=%d" % (arm, entry, k, b.lens[k]), z[s], None if sv is None else int(sv[k]), ref)
        worst = max(worst, e_k / max(e_o, FLOOR))
    print("%s %s: worst e_kernel / max(e_oracle, floor) = %.2f" % (arm, entry, worst))


# -------------------------------------------------------------------------------------------------- E. parameter edges


def _tile(batch, times):
    return batch.sub(list(range(len(batch.lens))) * times)


def _grow_case():
    """A global-smooth problem whose active set grows over 5 solves (found by a CPU search over random-walk inputs)."""
    r = np.random.default_rng(1348)
    n = int(r.integers(5, 120))
    xy = np.cumsum(r.uniform(20, 60, size=(n, 2)), axis=0)
    zin = 100 + np.cumsum(r.normal(0, 8, n))
    return np.column_stack([xy, zin]), zin, (100.0, 0.5)


def _edge_batches():
    """{name: (Batch, optimize params or None, global params or None)}: lengths 1, 2, 3, 40 (and 600 alone, for the
    cyclic reduction)."""
    base = Batch((1, 2, 3, 40), 1000)
    long = Batch((600,), 1001)
    out = {}
    for tag, b in (("small", base), ("long", long)):
        out["ls0_" + tag] = (b, (0.0, 0.5, 50.0, 2.0), (0.0, 2.0))
        out["rate0_" + tag] = (b, (1.0, 0.5, 50.0, 0.0), (1.0, 0.0))
        out["ls0_rate0_" + tag] = (b, (0.0, 0.5, 50.0, 0.0), (0.0, 0.0))
        out["follow0_" + tag] = (b, (1.0, 0.0, 50.0, 2.0), None)
        nan = b.copy()
        nan.elev[:] = np.nan
        out["all_nan_elev_" + tag] = (nan, OPT, None)
        rep = b.copy()
        for k, n in enumerate(rep.lens):     # exactly repeated xy: every third sample sits on its predecessor (d = 0)
            o = int(rep.off[k])
            for i in range(1, n, 3):
                rep.xyz[o + i, :2] = rep.xyz[o + i - 1, :2]
        out["repeated_xy_" + tag] = (rep, OPT, GLB)
    return out


EDGES = _edge_batches()


@functools.lru_cache(maxsize=None)
def _edge_reference(name, entry):
    b, po, pg = EDGES[name]
    params = po if entry == "optimize" else pg
    out = []
    for k in range(len(b.lens)):
        xyz, elev, zin = b.problem(k)
        out.append(reference(entry, xyz, elev if entry == "optimize" else zin, params))
    return out


@pytest.mark.parametrize("name", sorted(EDGES))
def test_parameter_edges(csp, name):
    """lambda_smooth = 0, max_climb_rate = 0 (the first early-out of edge_w), both together with lambda_follow > 0,
    lambda_follow = 0, an all-NaN elev and exactly repeated xy (dist <= 1e-9: the edge is skipped), each at n = 1, 2, 3
    and 40 on the wave kernels, the same batch tiled 512 times (2048 problems) on the lane kernels, and at n = 600 on the
    cyclic reduction: against tests/alt_ref.py at the module's gate, solve counts equal.  With every weight zero the
    global smooth's interior rows are 1e-8 z = 0: z = 0 violates, everything turns active, two solves."""
    b, po, pg = EDGES[name]
    for entry, params in (("optimize", po), ("global", pg)):
        if params is None:
            continue
        refs = _edge_reference(name, entry)
        runs = [("", b)] if name.endswith("long") else [("wave ", b), ("lane ", _tile(b, 512))]
        for label, bb in runs:
            assert mapping(bb.lens) == (label.strip() or "cr")
            z, sv = run(csp, entry, bb, params)
            for k in range(len(b.lens)):     # the first copy of each problem; the tiles repeat it
                s = slice(bb.off[k], bb.off[k + 1])
                gate("%s%s %s n=%d" % (label, name, entry, b.lens[k]), z[s], None if sv is None else int(sv[k]), refs[k])
            if label == "lane ":             # and every tile is the first one again
                m = len(b.xyz)
                assert all(z[t * m:(t + 1) * m].tobytes() == z[:m].tobytes() for t in (1, 255, 511)), name


def test_active_set_growth(csp):
    """A global-smooth problem whose active set grows over 5 solves, on all three mappings
    (alone: wave; tiled 2048 times: lane; and a 600-sample one for the cyclic reduction that takes as many solves as the
    references say): counts equal to alt_ref's and the oracle's, values at the gate.
    A case that stops at the cap of 10 was looked for on the CPU and not found: 7000 random problems (random walks,
    sinusoids, ramps, sparse spikes of 1e-2 .. 1e6 on a flat profile, lambda_smooth 1e-2 .. 1e4, climb rates 0 .. 10) with
    the C oracle never took more than 5 solves -- each solve activates every violated sample at once, so the set
    settles in a few rounds."""
    xyz, zin, params = _grow_case()
    one = Batch.of((len(zin),), xyz, np.zeros(len(zin)), zin)
    ref = reference("global", xyz, zin, params)
    assert ref[2] >= 3, ref[2]
    for label, bb in (("wave", one), ("lane", _tile(one, 2048))):
        assert mapping(bb.lens) == label
        z, sv = run(csp, "global", bb, params)
        gate("growth %s n=%d" % (label, len(zin)), z[:len(zin)], int(sv[0]), ref)
        assert (sv == sv[0]).all()
    r = np.random.default_rng(5)
    n = 600
    xy = np.cumsum(r.uniform(20, 60, size=(n, 2)), axis=0)
    z600 = 100 + np.cumsum(r.normal(0, 8, n))
    long = Batch.of((n,), np.column_stack([xy, z600]), np.zeros(n), z600)
    assert mapping(long.lens) == "cr"
    ref = reference("global", long.xyz, z600, params)
    z, sv = run(csp, "global", long, params)
    gate("growth cr n=600", z, int(sv[0]), ref)
    assert ref[2] >= 3, ref[2]


# ------------------------------------------------------------------------------------------------------- G. stiff case


def _stiff(n, g, seed=77):
    """A benign problem in which samples (2, 3) -- inside one 8-row block, one 64-row round and one 2-row block of the
    cyclic reduction -- and samples (63, 64) -- across all three boundaries -- are a planar distance g apart."""
    xyz, elev = _problem(np.random.default_rng(seed), n, with_gaps=False)
    for i in (3, 64):
        shift = xyz[i, :2] - (xyz[i - 1, :2] + np.array([g, 0.0]))
        xyz[i:, :2] -= shift
    return Batch.of((n,), xyz, elev, xyz[:, 2] + 5.0)


@functools.lru_cache(maxsize=None)
def _stiff_reference(n, g, entry):
    b = _stiff(n, g)
    return reference(entry, b.xyz, b.elev if entry == "optimize" else b.zin, OPT if entry == "optimize" else GLB)


@pytest.mark.parametrize("g", [1e-3, 1e-5, 1e-6, 1e-7])
@pytest.mark.parametrize("label", ["wave", "lane", "cr"])
def test_stiff_pairs(csp, label, g):
    """Two pairs of samples a planar distance g apart: the climb-rate weight 1 / (2 g)^2 is 2.5e5, 2.5e9, 2.5e11 and 2.5e13
    against entries of order 1 elsewhere.  n = 80 alone (wave), tiled 2048 times (lane), n = 600 (cyclic reduction, whose
    2x2 pivots are determinants b00 b11 - b01^2 of such entries).
    g = 1e-3 and 1e-5 are gated like F on all three mappings and both entries.  Two named exceptions, both for the global
    smooth: on the lane / wave kernels the gate uses K_STIFF_RECURRENCE_GLOBAL = 50 (measured 21.75 at g = 1e-3 and 13.05
    at 1e-5: e_kernel 2.6e-14 against an e_oracle of 1.2e-15 / 2.0e-15; solve counts compared, the margin of 1e-3 is far
    above the 3e-11 needed); on the cyclic reduction's n = 600 problem at g = 1e-5 the values are gated (K = 10, measured
    0.98) but not the solve count: the oracle itself is 5.4e-2 off there, 100 * e_oracle * max|z| is ~1e3 against a margin
    of 1e-3, and the test asserts that the margin rule excludes the case.
    At g = 1e-6 and 1e-7 the figures are RECORDED ONLY: the fp64 reference itself is off by 1e-5 to 1 there (its Cholesky
    breaks down in the global smooth at 1e-7), so K * e_oracle would accept almost anything; nothing is asserted on
    them beyond the memory contract of run()."""
    n = 600 if label == "cr" else 80
    one = _stiff(n, g)
    bb = _tile(one, 2048) if label == "lane" else one
    assert mapping(bb.lens) == label
    for entry in ENTRIES:
        ref = _stiff_reference(n, g, entry)
        z, sv = run(csp, entry, bb)
        z1, k1 = z[:n], None if sv is None else int(sv[0])
        tag = "stiff g=%g %s %s n=%d" % (g, label, entry, n)
        if g >= 1e-5:
            k = K_STIFF_RECURRENCE_GLOBAL if entry == "global" and label != "cr" else K_GATE
            count = not (entry == "global" and label == "cr" and g < 1e-3)
            if not count:    # the margin rule itself excludes this case from the count comparison
                assert ref[4] <= 100 * alt_ref.rel_err(ref[1], ref[0]) * np.max(np.abs(ref[0])), (tag, ref[4])
            gate(tag, z1, k1, ref, want_count=count, k=k)
        else:
            e_o, e_k = alt_ref.rel_err(ref[1], ref[0]), alt_ref.rel_err(z1, ref[0])
            print("%-44s e_oracle %.3e  e_kernel %.3e  ratio %8.2f  (recorded only)%s" % (
                tag, e_o, e_k, e_k / e_o if e_o else float("nan"), "" if k1 is None else "  solves %d/%d/%d" % (ref[2], ref[3], k1)))
