"""The case table of tests/test_gpu_grad_spread.py: the reverse-mode, cost, knot-constraint and optimiser entries under
unequal segment times, with their inputs, references, metrics and the CPU figures the gates rest on.

TEST INFRASTRUCTURE ONLY.  Shared by the GPU test and by tests/test_spread_vjp_ref.py (which evaluates the table without a
GPU), so that both draw identical inputs.  The machinery is tests/spread_cases.py's: every uniform batch is K = 4 distinct
trajectories (spread_cases.problem: spread_ref.spread_batch, per-row bc and velocity-zero weights with row 0 at w = 0)
tiled over B = 65 rows; references (tests/spread_vjp_ref.py at 40 digits) and the fp64 figures are computed once per
distinct trajectory and cached for the process.

A *source* is what one open-chain case is judged on, whoever computed it (the kernel, the reference in Python floats, the
numpy restatements): {call: ([per member dict(waypoints, times, bc)], shared bc sum or None)} for the calls of CALLS, and
"costentry": [per member (J, dJ/dT)].  `open_errors` turns a source into {(call, output): error} in the metrics below.

Metrics.  Gradients: per trajectory max-abs error over max-abs reference (vjp_ref.rel_err_rows), worst trajectory.  Every
time gradient also in its T-weighted form max |dg_j T_j| / max |g_j T_j| -- the gradient with respect to log T: with
R = 16 the plain form is blind to the long segments, whose entries are small.  J: relative.
"""
import functools
from dataclasses import dataclass

import numpy as np

from tests import spread_cases as sc
from tests import spread_ref as sr
from tests import spread_vjp_ref as sv
from tests.vjp_ref import rel_err_rows

K = sc.K
B = 65
ORDERS = (2, 3, 4, 5)
R16 = sc.R16
SEED = {"open": 31, "periodic": sc._FAMILY_SEED["periodic"], "knots": 33, "opt": 34}
OPEN_S = (1, 2, 3, 16, 40)
OPEN_F32_S = (3, 16)
OPEN_RAGGED = (1, 2, 17, 1, 5, 64)
PERIODIC_S = (1, 2, 3, 5, 12)
PERIODIC_RAGGED = (12, 3, 1, 2, 5)
CALLS = ("coeffs0", "coeffs1", "cost", "both0", "both1")       # grad_coeffs kind 0 / 1 alone, grad_cost alone, both
PERIODIC_CALLS = ("coeffs0", "coeffs1", "both0", "both1")      # the periodic entry always takes grad_coeffs
ABSOLUTE_AT = 1e-7       # the 1e-6 north star is asserted on the kernel wherever e_cpu64 is at most this
NORTH_STAR_TOL = 1e-6


@dataclass(frozen=True)
class Case:
    family: str              # "open" or "periodic"
    pattern: str
    order: int
    S: int = 0
    f32: bool = False
    bc_per: bool = True      # per-trajectory bc and velocity-zero weights; False: one shared bc, the weight sc.VW
    lens: tuple = ()         # ragged: the segment counts
    rows: int = K

    @property
    def id(self):
        shape = "ragged" if self.lens else "s%d" % self.S
        return "%s-%s-o%d-%s%s%s" % (self.family, self.pattern, self.order, shape, "-f32" if self.f32 else "",
                                     "" if self.bc_per or self.family == "periodic" else "-sharedbc")


def open_patterns(order):
    """R = 16 everywhere, dist256 at orders 2 and 3, and at order 4 on one case (relative gate only, as in §17)."""
    return R16 + (("dist256",) if order in (2, 3, 4) else ())


def open_cases(order, pattern):
    if pattern == "dist256" and order == 4:
        return [Case("open", pattern, order, 16)]
    out = [Case("open", pattern, order, S, bc_per=per) for S in OPEN_S for per in (False, True)]
    out += [Case("open", pattern, order, S, f32=True) for S in OPEN_F32_S]
    out.append(Case("open", pattern, order, lens=OPEN_RAGGED))
    return out


def periodic_cases(order, pattern):
    out = [Case("periodic", pattern, order, S, rows=2 if S == 12 else K) for S in PERIODIC_S]
    out.append(Case("periodic", pattern, order, lens=PERIODIC_RAGGED))
    return out


OPEN_GROUPS = [(o, p) for o in ORDERS for p in open_patterns(o)]
PERIODIC_GROUPS = [(o, p) for o in ORDERS for p in R16]


def members(c):
    """The distinct trajectories of a case as (S, row) in batch order."""
    if c.lens:
        return [(int(n), i % K) for i, n in enumerate(c.lens)]
    return [(c.S, r) for r in range(c.rows)]


def counts(c):
    """How many rows of the B-row batch carry each distinct trajectory."""
    return np.bincount(np.arange(B) % c.rows, minlength=c.rows)


# ------------------------------------------------------------------------------------------------------------- open chain


def open_inputs(c, mem):
    """(path [S+1,3], time [S], bc [4,3], w) of one distinct trajectory."""
    S, row = mem
    return sc.row_inputs(c.pattern, c.order, S, SEED["open"], c.f32, row, c.bc_per, c.bc_per)


@functools.lru_cache(maxsize=None)
def cotangents(family, pattern, order, S, f32, row):
    """(pbar [2,S,3,2o], jbar): pbar[0] standard normal; pbar[1] standard normal times T_j^pow_i, which gives every power
    equal weight in the polynomial's value over its segment (with R = 16 the plain kind is dominated by the constant
    term on short segments and by the top power on long ones); jbar standard normal.  f32: pbar as rounded to fp32."""
    m = 2 * order
    if family == "open":
        tm = sc.problem(pattern, order, S, SEED["open"], f32)[1][row]
    else:
        tm = sc.loops(pattern, S, SEED["periodic"])[1][row]
    rng = np.random.default_rng([SEED[family], order, S, row, int(sr.PATTERNS[pattern][0] == "dist"), int(sr.PATTERNS[pattern][1]),
                                 "lard".index(pattern[0])])
    pb = rng.normal(size=(2, S, 3, m))
    pb[1] *= tm[:, None, None] ** (m - 1 - np.arange(m))[None, None, :]
    jbar = float(rng.normal())
    if f32:
        pb = pb.astype(np.float32).astype(np.float64)
    pb.setflags(write=False)
    return pb, jbar


@functools.lru_cache(maxsize=None)
def _open_adjoint(pattern, order, S, f32, row, bc_per, dps, origin):
    c = Case("open", pattern, order, S, f32=f32, bc_per=bc_per)
    p, t, bc, w = open_inputs(c, (S, row))
    pb, jbar = cotangents("open", pattern, order, S, f32, row)
    return sv.open_chain(order, p, t, bc, w, pb, jbar, dps=dps, origin=origin)


def open_adjoint(c, mem, dps=40, origin="segment"):
    return _open_adjoint(c.pattern, c.order, mem[0], c.f32, mem[1], c.bc_per, dps, origin)


def combine(adj, call):
    """dict(waypoints, times, bc) of one call out of an Adjoint: the <pbar, coeffs> part of kind 0 / 1, jbar times the
    J part, or their sum."""
    out = {}
    for k in ("waypoints", "times", "bc"):
        L, Jp = getattr(adj, k), getattr(adj, "cost_" + k)
        if L is None:                        # a loop has no bc
            continue
        v = 0.0
        if call[:4] in ("coef", "both"):
            v = v + L[int(call[-1])]
        if call[:4] in ("cost", "both"):
            v = v + Jp
        out[k] = v
    return out


def _one(a):
    return np.asarray(a, dtype=np.float64).reshape(1, -1)


def grad_errors(got, ref, tm):
    """{output: error} of one trajectory; got / ref dict(waypoints, times[, bc])."""
    e = {"waypoints": rel_err_rows(_one(got["waypoints"]), _one(ref["waypoints"])),
         "times": rel_err_rows(_one(got["times"]), _one(ref["times"])),
         "times_T": rel_err_rows(_one(np.asarray(got["times"], dtype=np.float64) * tm), _one(np.asarray(ref["times"]) * tm))}
    if got.get("bc") is not None and ref.get("bc") is not None:
        e["bc"] = rel_err_rows(_one(got["bc"]), _one(ref["bc"]))
    return e


def cost_errors(J, g, rJ, rg, tm):
    return {"J": abs(float(J) - rJ) / max(abs(rJ), 1e-300), "dJdT": rel_err_rows(_one(g), _one(rg)),
            "dJdT_T": rel_err_rows(_one(np.asarray(g, dtype=np.float64) * tm), _one(rg * tm))}


FACTOR = 10.0           # the project's: test_large_time_and_length_scales, DESIGN.md section 17


def within(e_k, e_cpu, floor, factor=FACTOR):
    """The relative gate: e_k <= max(factor e_cpu64, floor)."""
    return e_k <= max(factor * e_cpu, floor)


def _worst(into, key, e):
    into[key] = max(into.get(key, 0.0), float(e))


def shared_bc_sum(c, per_member_bc):
    """The count-weighted sum over the K distinct rows: what a shared bc's gradient is over the tiled batch."""
    return sum(float(n) * np.asarray(b, dtype=np.float64) for n, b in zip(counts(c), per_member_bc))


def adjoint_source(c, dps, origin="segment"):
    """The source of a case from spread_vjp_ref.open_chain at `dps` digits (None: Python floats); origin as there."""
    ms = members(c)
    adj = [open_adjoint(c, m, dps, origin) for m in ms]
    src = {"costentry": [(a.cost, a.cost_grad_times) for a in adj]}
    for call in CALLS:
        per = [combine(a, call) for a in adj]
        src[call] = (per, None if c.bc_per else shared_bc_sum(c, [p["bc"] for p in per]))
    return src


def numpy_source(c):
    """The same from the dense fp64 numpy restatements (vjp_ref.adjoint, cost_vjp_ref.cost_adjoint, timeopt_ref.cost_grad)."""
    from tests import cost_vjp_ref, timeopt_ref, vjp_ref
    ms = members(c)
    src = {"costentry": []}
    parts = []
    for mem in ms:
        p, t, bc, w = open_inputs(c, mem)
        pb, jbar = cotangents("open", c.pattern, c.order, mem[0], c.f32, mem[1])
        src["costentry"].append(timeopt_ref.cost_grad(c.order, p, t, bc, w))
        cj = cost_vjp_ref.cost_adjoint(c.order, p, t, bc, w)
        parts.append(([vjp_ref.adjoint(c.order, p, t, bc, pb[k], w) for k in (0, 1)], {k: jbar * cj[k] for k in ("waypoints", "times", "bc")}))
    for call in CALLS:
        per = []
        for L, Jp in parts:
            if call.startswith("cost"):
                per.append(dict(Jp))
            else:
                k = int(call[-1])
                per.append({n: L[k][n] + (Jp[n] if call.startswith("both") else 0.0) for n in ("waypoints", "times", "bc")})
        src[call] = (per, None if c.bc_per else shared_bc_sum(c, [p["bc"] for p in per]))
    return src


def open_errors(c, src):
    """{(call, output): worst error over the case's distinct trajectories} of a source against the 40-digit adjoint."""
    ref = adjoint_source(c, 40)
    out = {}
    for i, mem in enumerate(members(c)):
        tm = open_inputs(c, mem)[1]
        for call in CALLS:
            got, want = dict(src[call][0][i]), dict(ref[call][0][i])
            if not c.bc_per:
                got.pop("bc", None)
            for k, e in grad_errors(got, want, tm).items():
                _worst(out, (call, k), e)
        for k, e in cost_errors(*src["costentry"][i], float(ref["costentry"][i][0]), ref["costentry"][i][1], tm).items():
            _worst(out, ("costentry", k), e)
    if not c.bc_per:
        for call in CALLS:
            _worst(out, (call, "bc"), rel_err_rows(_one(src[call][1]), _one(ref[call][1])))
    return out


@functools.lru_cache(maxsize=None)
def open_cpu64(c):
    """{(call, output): e_cpu64}: spread_vjp_ref.open_chain in Python floats against itself at 40 digits."""
    return open_errors(c, adjoint_source(c, None))


# -------------------------------------------------------------------------------------------------------------- periodic


def loop_inputs(c, mem):
    """(path [S,3], time [S], w) of one distinct loop: spread_cases.loops, shared with tests/test_gpu_time_spread.py."""
    S, row = mem
    wp, tm, w = sc.loops(c.pattern, S, SEED["periodic"])
    return wp[row], tm[row], float(w[row])


@functools.lru_cache(maxsize=None)
def _loop_adjoint(pattern, order, S, row, dps):
    wp, tm, w = sc.loops(pattern, S, SEED["periodic"])
    pb, jbar = cotangents("periodic", pattern, order, S, False, row)
    return sv.loop(order, wp[row], tm[row], float(w[row]), pb, jbar, dps=dps)


def loop_adjoint(c, mem, dps=40):
    return _loop_adjoint(c.pattern, c.order, mem[0], mem[1], dps)


def loop_source(c, dps):
    adj = [loop_adjoint(c, m, dps) for m in members(c)]
    return {call: [combine(a, call) for a in adj] for call in PERIODIC_CALLS}


def loop_numpy_source(c):
    from tests import periodic_vjp_ref
    src = {call: [] for call in PERIODIC_CALLS}
    for mem in members(c):
        p, t, w = loop_inputs(c, mem)
        pb, jbar = cotangents("periodic", c.pattern, c.order, mem[0], False, mem[1])
        for call in PERIODIC_CALLS:
            r = periodic_vjp_ref.adjoint(c.order, p, t, pb[int(call[-1])], jbar if call.startswith("both") else 0.0, w)
            src[call].append({"waypoints": r["waypoints"], "times": r["times"]})
    return src


def loop_errors(c, src):
    ref = loop_source(c, 40)
    out = {}
    for i, mem in enumerate(members(c)):
        tm = loop_inputs(c, mem)[1]
        for call in PERIODIC_CALLS:
            for k, e in grad_errors(src[call][i], ref[call][i], tm).items():
                _worst(out, (call, k), e)
    return out


@functools.lru_cache(maxsize=None)
def loop_cpu64(c):
    return loop_errors(c, loop_source(c, None))


@functools.lru_cache(maxsize=None)
def loop_same_math(c):
    """e_same of a loop: the free-derivative system the periodic kernels solve (every knot's o-1 derivatives, the block-
    cyclic matrix summed in fp64), which tests/periodic_vjp_ref.py states in numpy fp64; e_cpu64 is the KKT system in the
    monomial coefficients, which never forms that matrix (DESIGN.md sections 17.3, 21.3)."""
    return loop_errors(c, loop_numpy_source(c))


# ----------------------------------------------------------------------------------------------------------------- knots

KNOT_MASKS = ("standard", "free_end", "vel_mid", "hermite", "random")
KNOT_S = (3, 16, 17)
KNOT_K = 3               # tests/test_gpu_knots.py's K: its velocity-zero weights come in threes


def knot_times(pattern, S):
    """(waypoints [KNOT_K,S+1,3], times [KNOT_K,S]) of the named R = 16 pattern (constant-speed legs under dist16)."""
    wp, tm = sr.spread_batch(pattern, KNOT_K, S, SEED["knots"])
    return wp, tm


# ------------------------------------------------------------------------------------------------------------- optimiser

OPT_PATTERNS = ("log16", "alt16")
OPT_S, OPT_TMIN, OPT_TOL, OPT_ITERS = 6, 0.1, 1e-6, 300
OPT_MODES = ("fixed_total", "time_penalty")


# Seeds moved (where a yardstick cannot judge from a draw, the seed changes, never the condition) until the conditions tests/test_spread_vjp_ref.py
# puts on the test's own yardsticks hold: the converged share reached by the reference optimiser alone, and
# timeopt_ref.cost_grad's J within a tenth of _invariants' bound of the 40-digit J at the reference optimiser's final times
# (at order 5 under alt16 with a fixed total the first draw ended one trajectory with a segment on min_time, times of
# ratio 57, where the numpy J is 8e-6 off).  Both are judged without a kernel.
OPT_RESEED = {(4, "alt16", "fixed_total"): 100, (5, "alt16", "fixed_total"): 100, (5, "log16", "time_penalty"): 100}
OPT_J_TOL = {2: 1e-8, 3: 1e-8, 4: 1e-8, 5: 1e-6}        # _invariants' bound on |J_numpy - objective| / J_numpy


def opt_share(order):
    """The converged share tests/test_gpu_timeopt.py::test_optimiser_invariants requires: 5/8 at order 5, 3/4 otherwise."""
    return B * 5 // 8 if order == 5 else B * 3 // 4


@functools.lru_cache(maxsize=None)
def opt_problem(order, pattern, mode):
    """B = 65 distinct trajectories of 6 segments whose start times are drawn by the pattern: (waypoints [B,7,3], times
    [B,6], bc [B,4,3], rho).  rho, the time weight of the time_penalty mode, is the median of J / sum T at the start (as in
    test_optimiser_invariants), from tests/timeopt_ref.py so that the CPU and the GPU test use the same number."""
    from tests.timeopt_ref import cost_grad
    kind, R = sr.PATTERNS[pattern]
    sd = SEED["opt"] + 10 * order + (mode == "fixed_total") + OPT_RESEED.get((order, pattern, mode), 0)
    tm = sr.spread_times(kind, R, B, OPT_S, sd)
    rng = np.random.default_rng([sd, order, "lard".index(kind[0])])
    p0 = rng.uniform(-10.0, 10.0, size=(B, 1, 3))
    wp = np.concatenate([p0, p0 + np.cumsum(rng.normal(size=(B, OPT_S, 3)), axis=1)], axis=1)
    bc = rng.normal(size=(B, 4, 3)) * 0.5
    rho = 0.0
    if mode == "time_penalty":
        rho = float(np.median([cost_grad(order, wp[b], tm[b], bc[b])[0] / tm[b].sum() for b in range(B)]))
    for x in (wp, tm, bc):
        x.setflags(write=False)
    return wp, tm, bc, rho


OPT_REF_TOL = {2: 2e-7, 3: 2e-7, 4: 2e-7, 5: 1e-6}     # _invariants' bound on |f_kernel - f_reference| / f_reference


@functools.lru_cache(maxsize=None)
def opt_ref_spread(order, pattern, mode, b):
    """How far the reference optimiser reproduces ITSELF on trajectory b: the relative spread of its final objective over
    three starts that differ in the last bits of the times (fixed_total: +-2^-50 in alternation, so the total is kept;
    time_penalty: one ulp).  From a start of ratio 16 the stopping rule (projected gradient scaled by the START's
    objective <= tol) is met well above the optimum, on a flat valley, and under alt16 with a fixed total at order 5 the
    point where the iteration stops there depends on the last bits of the start on most trajectories (1e-7 .. 7e-4)."""
    from tests.timeopt_ref import optimize
    wp, tm, bc, rho = opt_problem(order, pattern, mode)
    alt = np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0])
    f = []
    for k in range(3):
        t = tm[b] + k * 2.0 ** -50 * alt if mode == "fixed_total" else tm[b] * (1.0 + k * 2.0 ** -52 * alt)
        f.append(optimize(order, wp[b], t, bc[b], 0.0, mode, rho, OPT_TMIN, OPT_TOL, 500)["f"])
    return max(abs(x - f[0]) for x in f) / f[0]


@functools.lru_cache(maxsize=None)
def opt_ref_lanes(order, pattern, mode):
    """The trajectories on which _invariants compares the kernel's objective with the reference optimiser's: the first
    four of the batch on which the reference reproduces itself to a tenth of that comparison's bound (fewer if the batch
    has fewer).  A reference
    that moves by more than the bound under a last-bit change of its own start cannot judge a kernel to that bound."""
    lanes = []
    for b in range(B):
        if opt_ref_spread(order, pattern, mode, b) <= 0.1 * OPT_REF_TOL[order]:
            lanes.append(b)
            if len(lanes) == 4:
                break
    return tuple(lanes)


def opt_batch_order(order, pattern, mode):
    """The order in which the GPU test lays the 65 trajectories out: opt_ref_lanes first (_invariants compares the first
    four with the reference optimiser), the others behind them in their own order."""
    lead = list(opt_ref_lanes(order, pattern, mode))
    return np.array(lead + [b for b in range(B) if b not in lead])


@functools.lru_cache(maxsize=None)
def opt_yardstick_error(order, pattern, mode):
    """max over the 65 trajectories of |J_numpy - J_40| / J_40 at the times the reference optimiser ends on: the error of
    the yardstick _invariants holds the kernel's objective to."""
    from tests.timeopt_ref import cost_grad, optimize
    wp, tm, bc, rho = opt_problem(order, pattern, mode)
    worst = 0.0
    for b in range(B):
        T = optimize(order, wp[b], tm[b], bc[b], 0.0, mode, rho, OPT_TMIN, OPT_TOL, OPT_ITERS)["times"]
        hi = sv.open_chain(order, wp[b], T, bc[b], 0.0).cost
        worst = max(worst, abs(cost_grad(order, wp[b], T, bc[b], 0.0)[0] - hi) / hi)
    return worst
