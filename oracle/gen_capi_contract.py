"""Generates tests/golden/capi_contract.json -- TEST INFRASTRUCTURE.   Run on a machine WITHOUT a device:
    python oracle/gen_capi_contract.py

The host-side contract of the minimum-snap C-ABI (cs-pathplan_amd/csrc/minsnap_capi.hip), recorded from the built library
and nothing else, so that a change to that file's host code shows on the CPU:

  table A ("dispatch"): for a grid of descriptors, csp_minsnap_kernel_name and every *_workspace_bytes function.  These
      decide nothing but from the descriptor; tests/test_capi.py replays the table everywhere.
  table B ("return_codes"): for csp_minsnap_solve_batch, _solve_batch_vjp, _cost_batch, _optimize_times_batch and
      _solve_periodic_batch, the return code of calls that end before any device work.  Without a device a call that
      passes every check of its entry returns CSP_ERR_NO_DEVICE, which pins the ORDER of the checks relative to the
      device selection too (the periodic entry and the time optimiser look at ragged offsets before it, the other three
      after it).  Every non-null pointer is a real buffer large enough for the call.  Replayed only without a device.

The rows hold the whole descriptor, so the replay (replay_dispatch_row / run_return_code_case below, which the test
imports) builds its calls from the file alone.
"""
import ctypes
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "capi_contract.json")

WS_FUNCS = ("csp_minsnap_workspace_bytes", "csp_minsnap_vjp_workspace_bytes", "csp_minsnap_cost_workspace_bytes",
            "csp_minsnap_timeopt_workspace_bytes", "csp_minsnap_periodic_workspace_bytes",
            "csp_minsnap_plan_workspace_bytes", "csp_minsnap_mixed_workspace_bytes")
DISPATCH_COLUMNS = ("order", "num_segments", "max_segments", "batch", "dtype", "path_weight", "bc_per_trajectory", "flags")
SEGMENTS = (1, 2, 7, 8, 9, 16, 17, 40, 64, 256, 257, 1024, 1025)
BATCHES = (1, 100, 40000)
FG, SM, F32A, SPAN = 0x1, 0x2, 0x8, 0x20

_offsets_any = np.zeros(40001, dtype=np.int64)   # table A never reads the offsets: ragged descriptors only need a pointer


# ------------------------------------------------------------------------------------------------------------- table A


def dispatch_descriptors():
    """Orders 1..5 x the segment counts, uniform and ragged, plain (B = 100, fp64, no penalty, shared bc, no flag); the
    order-5 rule's big batch; every descriptor of test_validation_and_dispatch_names; and a seeded draw over the whole
    grid (batch, dtype, path_weight, bc_per_trajectory, one flag or none)."""
    rows = []
    for order in range(1, 6):
        for S in SEGMENTS:
            rows.append((order, S, 0, 100, 0, 0.0, 0, 0))
            rows.append((order, 0, S, 100, 0, 0.0, 0, 0))
    for S in SEGMENTS:
        rows.append((5, S, 0, 40000, 0, 0.0, 0, 0))
        rows.append((5, 0, S, 40000, 0, 0.0, 0, 0))
    for order, batch, S, kw in (
            (4, 65536, 16, {}), (4, 4096, 8, {}), (4, 65536, 16, dict(flags=FG)), (2, 100, 6, {}), (5, 100, 10, {}),
            (5, 100, 10, dict(flags=FG)), (4, 100, 64, dict(flags=SPAN)), (4, 100, 16, dict(flags=SPAN)),
            (3, 100, 16, dict(flags=SM)), (4, 10, 16, dict(pw=1e-3)), (4, 10, 16, dict(pw=1e-3, flags=FG)),
            (5, 10, 8, dict(pw=1e-3)), (4, 10, 17, dict(pw=1e-3)), (3, 10, 7, dict(dtype=1)),
            (3, 10, 7, dict(dtype=1, flags=FG)), (3, 10, 7, dict(dtype=1, flags=F32A)), (6, 1, 4, {}), (0, 1, 4, {})):
        rows.append((order, S, 0, batch, kw.get("dtype", 0), kw.get("pw", 0.0), 0, kw.get("flags", 0)))
    rng = np.random.default_rng(20261018)
    for _ in range(100):
        S = int(rng.choice(SEGMENTS))
        ragged = bool(rng.integers(2))
        rows.append((int(rng.integers(1, 6)), 0 if ragged else S, S if ragged else 0, int(rng.choice(BATCHES)),
                     int(rng.integers(2)), float(rng.choice((0.0, 1e-3))), int(rng.integers(2)),
                     int(rng.choice((0, 0, FG, SM, F32A, SPAN)))))
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def replay_dispatch_row(csp, row):
    """[kernel name or None, the seven workspace sizes] of one table-A descriptor."""
    order, S, smax, batch, dtype, pw, bc_per, flags = row
    d = csp.make_desc(order, batch, S, dtype=dtype, path_weight=pw, bc_per_trajectory=bool(bc_per), max_segments=smax,
                      seg_offsets_ptr=_offsets_any.ctypes.data if S == 0 else None, flags=flags)
    lib = csp.raw_lib()
    return [csp.kernel_name(d)] + [int(getattr(lib, f)(ctypes.byref(d))) for f in WS_FUNCS]


# ------------------------------------------------------------------------------------------------------------- table B

# per entry: the C symbol, its pointer arguments between the descriptor (and parameter block) and the workspace, the
# required ones, whether validate_vjp's limits apply
ENTRIES = {
    "solve_batch": ("csp_minsnap_solve_batch", ("waypoints", "times", "bc", "coeffs", "max_dev", "status"),
                    ("waypoints", "times", "bc", "coeffs"), False),
    "solve_batch_vjp": ("csp_minsnap_solve_batch_vjp", ("waypoints", "times", "bc", "grad_coeffs", "grad_waypoints",
                                                        "grad_times", "grad_bc", "status"),
                        ("waypoints", "times", "bc", "grad_coeffs"), True),
    "cost_batch": ("csp_minsnap_cost_batch", ("waypoints", "times", "bc", "cost", "grad_times", "status"),
                   ("waypoints", "times", "bc", "cost"), True),
    "optimize_times_batch": ("csp_minsnap_optimize_times_batch", ("waypoints", "times", "bc", "times_out", "coeffs",
                                                                  "objective", "iterations", "status"),
                             ("waypoints", "times", "bc", "times_out"), True),
    "solve_periodic_batch": ("csp_minsnap_solve_periodic_batch", ("waypoints", "times", "coeffs", "cost", "grad_times", "status"),
                             ("waypoints", "times", "coeffs"), True),
}
BASE_DESC = dict(abi_version=1, dtype=0, order=2, num_segments=2, batch=3, max_segments=0, bc_per_trajectory=0,
                 path_weight=0.0, vel_zero_weight=0.0, mem_space=0, device_id=-1, flags=0)
BASE_PRM = dict(abi_version=1, mode=0, time_weight=0.0, min_time=0.01, tol=1e-6, max_iters=100)


def return_code_cases():
    """Case dictionaries without their "rc".  Keys: entry, case, desc (every scalar field), offsets (list or None),
    vw_per (bool), null_desc, null_args, prm (dict, None = null pointer, absent for the other entries), times (fill)."""
    cases = []
    for entry, (_, args, required, vjp_scope) in ENTRIES.items():
        timeopt = entry == "optimize_times_batch"

        def add(case, desc=None, offsets=None, null_args=(), null_desc=False, prm=BASE_PRM, times=1.0, vw_per=False):
            c = dict(entry=entry, case=case, desc=dict(BASE_DESC, **(desc or {})), offsets=offsets, vw_per=vw_per,
                     null_desc=null_desc, null_args=list(null_args), times=times)
            if timeopt:
                c["prm"] = None if prm is None else dict(prm)
            cases.append(c)

        ragged = dict(num_segments=0, max_segments=2)
        add("valid host call")
        add("valid device-space call", dict(mem_space=1))
        add("valid device-space call, one segment", dict(mem_space=1, num_segments=1))
        add("valid host call, every optional output null", null_args=[a for a in args if a not in required])
        add("valid ragged host call", ragged, offsets=[0, 1, 3, 5], vw_per=True)
        add("null descriptor", null_desc=True)
        add("wrong abi_version", dict(abi_version=99))
        add("bad dtype", dict(dtype=7))
        add("bad mem_space", dict(mem_space=9))
        add("order 0", dict(order=0))
        add("order 6", dict(order=6))
        add("negative batch", dict(batch=-1))
        add("negative num_segments", dict(num_segments=-1))
        add("negative path_weight", dict(path_weight=-1.0))
        add("negative vel_zero_weight", dict(vel_zero_weight=-0.5))
        add("segment-major with a ragged batch", dict(ragged, flags=SM), offsets=[0, 1, 3, 5])
        add("ragged without offsets", ragged)
        add("ragged with max_segments 0", dict(ragged, max_segments=0), offsets=[0, 1, 3, 5])
        add("batch 0", dict(batch=0))
        add("batch 0, every pointer null", dict(batch=0), null_args=args)
        for a in required:
            add("null " + a, null_args=[a])
        add("order 1", dict(order=1))
        add("path_weight > 0", dict(path_weight=1e-3))
        add("segment-major", dict(flags=SM))
        add("f32 arithmetic", dict(dtype=1, flags=F32A))
        add("f32 storage", dict(dtype=1))
        add("ragged host call, a negative trajectory", ragged, offsets=[0, 2, 1, 3])
        add("ragged host call, an over-long trajectory", ragged, offsets=[0, 1, 4, 5])
        add("ragged device-space call, an over-long trajectory", dict(ragged, mem_space=1), offsets=[0, 1, 4, 5])
        if timeopt:
            add("null parameter block", prm=None)
            add("parameter block: wrong abi_version", prm=dict(BASE_PRM, abi_version=2))
            add("parameter block: bad mode", prm=dict(BASE_PRM, mode=2))
            add("parameter block: time penalty, weight 0", prm=dict(BASE_PRM, mode=1))
            add("parameter block: time penalty, weight inf", prm=dict(BASE_PRM, mode=1, time_weight="inf"))
            add("parameter block: time penalty, weight 2", prm=dict(BASE_PRM, mode=1, time_weight=2.0))
            add("parameter block: min_time 0", prm=dict(BASE_PRM, min_time=0.0))
            add("parameter block: min_time nan", prm=dict(BASE_PRM, min_time="nan"))
            add("parameter block: tol negative", prm=dict(BASE_PRM, tol=-1.0))
            add("parameter block: tol nan", prm=dict(BASE_PRM, tol="nan"))
            add("parameter block: max_iters negative", prm=dict(BASE_PRM, max_iters=-1))
            add("fixed total infeasible, host memory", times=0.001)
            add("fixed total infeasible, ragged host memory", ragged, offsets=[0, 1, 3, 5], times=0.001)
            add("fixed total infeasible, device space (not checked on the host)", dict(mem_space=1), times=0.001)
            add("time penalty with times below min_time", prm=dict(BASE_PRM, mode=1, time_weight=2.0), times=0.001)
            add("bad parameter block before a null pointer", prm=dict(BASE_PRM, mode=2), null_args=["waypoints"])
            add("infeasible total before the ragged check's negative trajectory", ragged, offsets=[0, 2, 1, 3], times=0.001)
    return cases


def run_return_code_case(csp, c):
    """Makes the call one table-B case describes and returns its code.  Buffers hold 8 trajectories x 16 segments of
    order 6 in fp64: larger than anything a case of the table describes."""
    sym, args, _, _ = ENTRIES[c["entry"]]
    NT, NS, M = 8, 16, 12
    f8, sizes = np.float64, dict(
        waypoints=(NS + NT) * 3, times=NS, bc=NT * 12, coeffs=NS * 3 * M, grad_coeffs=NS * 3 * M, grad_waypoints=(NS + NT) * 3,
        grad_times=NS, grad_bc=NT * 12, times_out=NS, max_dev=NT, cost=NT, objective=2 * NT)
    bufs = {k: np.zeros(n, dtype=f8) for k, n in sizes.items()}
    bufs["times"][:] = c["times"]
    if c["desc"]["dtype"] == 1:   # fp32 storage: the same fill value in the first (and every) element
        bufs["times"] = np.full(2 * NS, c["times"], dtype=np.float32)
    bufs["status"], bufs["iterations"] = np.zeros(NT, dtype=np.int32), np.zeros(NT, dtype=np.int32)
    off = np.asarray(c["offsets"], dtype=np.int64) if c["offsets"] is not None else None
    vw = np.full(NT, 0.1) if c["vw_per"] else None
    d = csp.Desc()
    for k, v in c["desc"].items():
        setattr(d, k, v)
    d.seg_offsets = off.ctypes.data if off is not None else None
    d.vel_zero_weight_per_traj = vw.ctypes.data if vw is not None else None
    d.reserved = 0
    call = [None if c["null_desc"] else ctypes.byref(d)]
    if "prm" in c:
        prm = None
        if c["prm"] is not None:
            prm = csp.TimeOptParams()
            for k, v in c["prm"].items():
                setattr(prm, k, float(v) if isinstance(v, str) else v)
            prm.reserved = 0
        call.append(None if prm is None else ctypes.byref(prm))
    call += [None if a in c["null_args"] else bufs[a].ctypes.data for a in args]
    return int(getattr(csp.raw_lib(), sym)(*call, None, 0, None))


def record(csp):
    cases = return_code_cases()
    for c in cases:
        c["rc"] = run_return_code_case(csp, c)
    return {"dispatch": {"columns": list(DISPATCH_COLUMNS) + ["kernel_name"] + [f[len("csp_minsnap_"):] for f in WS_FUNCS],
                         "rows": [list(r) + replay_dispatch_row(csp, r) for r in dispatch_descriptors()]},
            "return_codes": cases}


def main():
    sys.path.insert(0, ROOT)
    csp = importlib.import_module("cs-pathplan_amd")
    if csp.device_count() > 0:
        raise SystemExit("table B is the contract WITHOUT a device: record it on a CPU-only machine")
    doc = record(csp)
    with open(OUT, "w") as f:
        f.write('{"dispatch": {"columns": %s, "rows": [\n' % json.dumps(doc["dispatch"]["columns"]))
        f.write(",\n".join(json.dumps(r) for r in doc["dispatch"]["rows"]))
        f.write('\n]}, "return_codes": [\n')
        f.write(",\n".join(json.dumps(c) for c in doc["return_codes"]))
        f.write("\n]}\n")
    print("%s: %d dispatch rows, %d return-code cases" % (OUT, len(doc["dispatch"]["rows"]), len(doc["return_codes"])))


if __name__ == "__main__":
    main()
