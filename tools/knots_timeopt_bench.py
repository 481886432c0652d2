"""Segment-time optimiser under per-knot constraints (csp_minsnap_optimize_times_knots_batch) against the existing optimiser
(csp_minsnap_optimize_times_batch) in the same run.

    python tools/knots_timeopt_bench.py [--steps K] [--warmup W]          (on the GPU box; prints one JSON line)

Shape: C3 (B = 65536, S = 16, order 4, fp64, zero bc), fixed total, 100 iterations at most, tol 1e-6.  Four calls on the same
waypoints and times: the existing optimiser; the new one with knots_from_bc's mask (the same problem); with a free end
(the last knot's mask 0); with a rest stop (every bit set, zero values, at knot S/2).  Per call: microseconds, the
distribution of accepted iterations (min / median / max), per wave of 64 lanes the passes the slowest lane needs (lower
bound: 1 + its iterations; backtracking passes are not reported by the entries) and the time per such wave-pass."""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import timed  # noqa: E402
from tests import synth  # noqa: E402

csp = importlib.import_module("cs-pathplan_amd")
ORDER, MIN_TIME, TOL, MAX_ITERS = 4, 0.1, 1e-6, 100


def measure(dev, wp, tm, steps, warmup, label, mask=None, values=None):
    """mask None: the existing optimiser with a zero bc."""
    B, S = tm.shape
    desc = csp.make_desc(ORDER, B, S, csp.DTYPE_F64, 0.0, 0.0, csp.MEM_DEVICE, False, None, 0, None, dev.index or 0, 0)
    prm = csp.make_timeopt_params(csp.TIMEOPT_FIXED_TOTAL, 0.0, MIN_TIME, TOL, MAX_ITERS)
    need = csp.timeopt_workspace_bytes(desc) if mask is None else csp.knots_timeopt_workspace_bytes(desc)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    tout = torch.empty_like(tm)
    obj = torch.empty((B, 2), dtype=torch.float64, device=dev)
    its = torch.empty(B, dtype=torch.int32, device=dev)
    stt = torch.empty(B, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    tail = (tout.data_ptr(), None, obj.data_ptr(), its.data_ptr(), stt.data_ptr(), ws.data_ptr(), need, st)
    if mask is None:
        bc = torch.zeros((1, 4, 3), dtype=torch.float64, device=dev)
        f = csp.raw_lib().csp_minsnap_optimize_times_batch
        args = (ctypes.byref(desc), ctypes.byref(prm), wp.data_ptr(), tm.data_ptr(), bc.data_ptr()) + tail
    else:
        mk, kv = torch.from_numpy(mask).to(dev), torch.from_numpy(values).to(dev)
        f = csp.raw_lib().csp_minsnap_optimize_times_knots_batch
        args = (ctypes.byref(desc), ctypes.byref(prm), wp.data_ptr(), tm.data_ptr(), mk.data_ptr(), kv.data_ptr()) + tail

    def opt():
        rc = f(*args)
        if rc:
            csp._check(rc)
    ms = timed(opt, steps, warmup, dev)
    it, s, o_np = its.cpu().numpy(), stt.cpu().numpy(), obj.cpu().numpy()
    pad = (-B) % 64
    wave_passes = 1 + np.concatenate([it, np.zeros(pad, dtype=it.dtype)]).reshape(-1, 64).max(axis=1)
    return {"workload": label, "batch": B, "segments": S, "order": ORDER, "workspace_bytes": need,
            "optimize_us": round(ms * 1e3, 1),
            "iterations_min_median_max": [int(it.min()), float(np.median(it)), int(it.max())],
            "wave_passes_mean_lower_bound": round(float(wave_passes.mean()), 2),
            "optimize_us_per_wave_pass_upper_bound": round(ms * 1e3 / float(wave_passes.mean()), 1),
            "converged_frac": round(float((s == 0).mean()), 4), "not_converged": int(((s & 8) != 0).sum()),
            "other_status": int(((s & ~8) != 0).sum()),
            "objective_ratio_median": round(float(np.median(o_np[:, 1] / o_np[:, 0])), 4), "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, S = 65536, 16
    wp, tm = synth.make_batch(B, S, config_id=3)
    wp, tm = torch.from_numpy(wp).to(dev), torch.from_numpy(tm).to(dev)
    mk, kv = csp.knots_from_bc(None, S, ORDER, batch=B)
    free_end = mk.copy()
    free_end[:, S] = 0
    rest_stop = mk.copy()
    rest_stop[:, S // 2] = (1 << (ORDER - 1)) - 1
    out = [measure(dev, wp, tm, a.steps, a.warmup, "C3, existing optimiser (zero bc)"),
           measure(dev, wp, tm, a.steps, a.warmup, "C3, knots optimiser, standard mask", mk, kv),
           measure(dev, wp, tm, a.steps, a.warmup, "C3, knots optimiser, free end", free_end, kv),
           measure(dev, wp, tm, a.steps, a.warmup, "C3, knots optimiser, rest stop at knot S/2", rest_stop, kv)]
    out[1]["over_existing"] = round(out[1]["optimize_us"] / out[0]["optimize_us"], 3)
    print(json.dumps({"tool": "knots_timeopt_bench", "results": out}))


if __name__ == "__main__":
    main()
