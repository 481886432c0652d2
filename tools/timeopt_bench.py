"""Segment-time optimiser (csp_minsnap_optimize_times_batch) and the cost pass (csp_minsnap_cost_batch) against the
generic forward kernel in the same run.

    python tools/timeopt_bench.py [--steps K] [--warmup W]          (on the GPU box; prints one JSON line)

Shapes: C3 (B = 65536, S = 16, order 4, fp64, zero bc) in both modes, and a ragged batch with S ~ U{4..64} at order 4
(fixed total).  Per call: microseconds, the distribution of accepted iterations over the trajectories (min / median /
max) and, per wave of 64 lanes, the passes the slowest lane needs (lower bound: 1 + its iterations; backtracking passes
are not reported by the entry).  One pass is the cost kernel's work at the current times; its time is measured too, and
the optimiser's time per wave-pass is set against the generic forward (solve_batch with force_generic) on the same
inputs."""
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


def measure(dev, wp, tm, o, steps, warmup, mode, rho, seg_offsets=None, label=""):
    ragged = seg_offsets is not None
    B = (seg_offsets.numel() - 1) if ragged else tm.shape[0]
    smax = int((seg_offsets[1:] - seg_offsets[:-1]).max().item()) if ragged else tm.shape[1]
    bc = torch.zeros((1, 4, 3), dtype=torch.float64, device=dev)
    desc = csp.make_desc(o, B, 0 if ragged else tm.shape[1], csp.DTYPE_F64, 0.0, 0.0, csp.MEM_DEVICE, False,
                         seg_offsets.data_ptr() if ragged else None, smax if ragged else 0, None, dev.index or 0, 0)
    prm = csp.make_timeopt_params(csp.TIMEOPT_TIME_PENALTY if mode == "time_penalty" else csp.TIMEOPT_FIXED_TOTAL, rho,
                                  0.1, 1e-6, 100)
    need = csp.timeopt_workspace_bytes(desc)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    tout = torch.empty_like(tm)
    obj = torch.empty((B, 2), dtype=torch.float64, device=dev)
    its = torch.empty(B, dtype=torch.int32, device=dev)
    stt = torch.empty(B, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    f = csp.raw_lib().csp_minsnap_optimize_times_batch
    args = (ctypes.byref(desc), ctypes.byref(prm), wp.data_ptr(), tm.data_ptr(), bc.data_ptr(), tout.data_ptr(), None,
            obj.data_ptr(), its.data_ptr(), stt.data_ptr(), ws.data_ptr(), need, st)

    def opt():
        rc = f(*args)
        if rc:
            csp._check(rc)
    ms_opt = timed(opt, steps, warmup, dev)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    grad = torch.empty_like(tm)
    fc = csp.raw_lib().csp_minsnap_cost_batch
    cneed = csp.cost_workspace_bytes(desc)
    cargs = (ctypes.byref(desc), wp.data_ptr(), tm.data_ptr(), bc.data_ptr(), cost.data_ptr(), grad.data_ptr(), None,
             ws.data_ptr(), cneed, st)

    def cst():
        rc = fc(*cargs)
        if rc:
            csp._check(rc)
    ms_cost = timed(cst, steps, warmup, dev)
    prep = csp.PreparedSolve(wp, tm, bc=bc, order=o, force_generic=True, seg_offsets=seg_offsets,
                             max_segments=smax if ragged else None, stream=torch.cuda.current_stream(dev).cuda_stream)
    ms_fwd = timed(prep.run, steps, warmup, dev)
    it = its.cpu().numpy()
    s = stt.cpu().numpy()
    pad = (-B) % 64
    wave_passes = 1 + np.concatenate([it, np.zeros(pad, dtype=it.dtype)]).reshape(-1, 64).max(axis=1)
    o_np = obj.cpu().numpy()
    return {"workload": label, "batch": B, "order": o, "mode": mode, "time_weight": rho,
            "optimize_us": round(ms_opt * 1e3, 1), "cost_pass_us": round(ms_cost * 1e3, 1),
            "forward_generic_us": round(ms_fwd * 1e3, 1), "cost_pass_over_forward": round(ms_cost / ms_fwd, 3),
            "iterations_min_median_max": [int(it.min()), float(np.median(it)), int(it.max())],
            "wave_passes_mean_lower_bound": round(float(wave_passes.mean()), 2),
            "optimize_us_per_wave_pass_upper_bound": round(ms_opt * 1e3 / float(wave_passes.mean()), 1),
            "per_wave_pass_over_forward_upper_bound": round(ms_opt / float(wave_passes.mean()) / ms_fwd, 3),
            "converged_frac": round(float((s == 0).mean()), 4), "not_converged": int(((s & 8) != 0).sum()),
            "other_status": int(((s & ~8) != 0).sum()),
            "objective_ratio_median": round(float(np.median(o_np[:, 1] / o_np[:, 0])), 4),
            "forward_kernel": prep.kernel, "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    o = 4
    B, S = 65536, 16
    wp, tm = synth.make_batch(B, S, config_id=3)
    wp, tm = torch.from_numpy(wp).to(dev), torch.from_numpy(tm).to(dev)
    out = [measure(dev, wp, tm, o, a.steps, a.warmup, "fixed_total", 0.0,
                   label="C3: B=65536 x 16 segments, order 4, fp64, fixed total"),
           measure(dev, wp, tm, o, a.steps, a.warmup, "time_penalty", 50.0,
                   label="C3: B=65536 x 16 segments, order 4, fp64, time penalty rho=50")]
    Br = 16384
    rng = np.random.default_rng(5)
    lens = rng.integers(4, 65, size=Br)
    wp_r = np.empty((int(lens.sum()) + Br, 3))
    tm_r = np.empty(int(lens.sum()))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    for b in range(Br):
        p0 = rng.uniform(-10, 10, size=(1, 3))
        wp_r[off[b] + b:off[b + 1] + b + 1] = np.concatenate([p0, p0 + np.cumsum(rng.normal(size=(lens[b], 3)), axis=0)])
        tm_r[off[b]:off[b + 1]] = rng.uniform(0.5, 2.0, size=lens[b])
    out.append(measure(dev, torch.from_numpy(wp_r).to(dev), torch.from_numpy(tm_r).to(dev), o, a.steps, a.warmup,
                       "fixed_total", 0.0, seg_offsets=torch.from_numpy(off).to(dev),
                       label="ragged: B=16384, S ~ U{4..64}, order 4, fp64, fixed total"))
    print(json.dumps({"tool": "timeopt_bench", "results": out}))


if __name__ == "__main__":
    main()
