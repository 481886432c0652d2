"""Lap-time optimiser of the periodic solve (csp_minsnap_optimize_times_periodic_batch) against the periodic forward with
cost and gradient and against the same number of iterations driven from torch, in the same run.

    python tools/periodic_timeopt_bench.py [--steps K] [--warmup W]          (on the GPU box; prints one JSON line)

Shape: C3 as a loop (B = 65536, S = 16, order 4, fp64; the first S waypoints of each C3 trajectory), fixed total,
min_time 0.1.  Three things on the same waypoints and times:
  * csp_minsnap_solve_periodic_batch with cost and gradient (one evaluation of the objective, coefficients included);
  * the optimiser at tol = 0 with max_iters 10 and 100, so that every lane that can move takes all its iterations: per
    call microseconds, accepted iterations, and the time per evaluation when every iteration cost one (an upper bound:
    backtracking passes are not reported by the entry, and at tol = 0 a lane that has reached the rounding floor of J
    spends up to 30 of them per iteration), and once more at tol = 1e-6, the default, with 100 iterations at most;
  * a projected-gradient loop on the host side through solve_periodic_batch_autograd: per iteration one forward with
    cost, one backward (csp_minsnap_solve_periodic_batch_vjp), a step and the exact projection onto the fixed total in
    torch -- what a caller had before this entry.  It takes fixed steps (no line search), so its launches per iteration
    are a lower bound for a torch optimiser that evaluates the objective more than once."""
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
ORDER, MIN_TIME = 4, 0.1


def forward_with_cost(dev, wp, tm, steps, warmup):
    B, S = tm.shape
    desc = csp.make_desc(ORDER, B, S, csp.DTYPE_F64, 0.0, 0.0, csp.MEM_DEVICE, False, None, 0, None, dev.index or 0, 0)
    need = csp.periodic_workspace_bytes(desc)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    co = torch.empty((B, S, 3, 2 * ORDER), dtype=torch.float64, device=dev)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    grad = torch.empty_like(tm)
    stt = torch.empty(B, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    f = csp.raw_lib().csp_minsnap_solve_periodic_batch
    args = (ctypes.byref(desc), wp.data_ptr(), tm.data_ptr(), co.data_ptr(), cost.data_ptr(), grad.data_ptr(), stt.data_ptr(),
            ws.data_ptr(), need, st)

    def go():
        rc = f(*args)
        if rc:
            csp._check(rc)
    return timed(go, steps, warmup, dev) * 1e3, cost


def optimiser(dev, wp, tm, steps, warmup, max_iters, tol=0.0):
    B, S = tm.shape
    desc = csp.make_desc(ORDER, B, S, csp.DTYPE_F64, 0.0, 0.0, csp.MEM_DEVICE, False, None, 0, None, dev.index or 0, 0)
    prm = csp.make_timeopt_params(csp.TIMEOPT_FIXED_TOTAL, 0.0, MIN_TIME, tol, max_iters)
    need = csp.periodic_timeopt_workspace_bytes(desc)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    tout = torch.empty_like(tm)
    obj = torch.empty((B, 2), dtype=torch.float64, device=dev)
    its = torch.empty(B, dtype=torch.int32, device=dev)
    stt = torch.empty(B, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    f = csp.raw_lib().csp_minsnap_optimize_times_periodic_batch
    args = (ctypes.byref(desc), ctypes.byref(prm), wp.data_ptr(), tm.data_ptr(), tout.data_ptr(), None, obj.data_ptr(),
            its.data_ptr(), stt.data_ptr(), ws.data_ptr(), need, st)

    def go():
        rc = f(*args)
        if rc:
            csp._check(rc)
    us = timed(go, steps, warmup, dev) * 1e3
    it, s, o_np = its.cpu().numpy(), stt.cpu().numpy(), obj.cpu().numpy()
    return {"tol": tol, "max_iters": max_iters, "workspace_bytes": need, "optimize_us": round(us, 1),
            "iterations_min_median_max": [int(it.min()), float(np.median(it)), int(it.max())],
            "us_per_evaluation_upper_bound": round(us / (1 + max_iters), 1),
            "not_converged": int(((s & 8) != 0).sum()), "other_status": int(((s & ~8) != 0).sum()),
            "objective_ratio_median": round(float(np.median(o_np[:, 1] / o_np[:, 0])), 4)}


def project_fixed_total(v, total, lo):
    """Rows of v onto {sum = total, entries >= lo}: the sort-based simplex projection of v - lo."""
    S = v.shape[1]
    y = v - lo
    z = (total - S * lo).unsqueeze(1)
    u, _ = torch.sort(y, dim=1, descending=True)
    css = torch.cumsum(u, dim=1) - z
    k = torch.arange(1, S + 1, device=v.device, dtype=v.dtype)
    cond = u - css / k > 0
    rho = cond.to(torch.int64).cumsum(dim=1).argmax(dim=1, keepdim=True)
    theta = css.gather(1, rho) / (rho + 1).to(v.dtype)
    return torch.clamp(y - theta, min=0.0) + lo


def torch_loop(dev, wp, tm, iters, steps, warmup, cost0):
    total = tm.sum(dim=1)
    # the optimiser's own scaling of the first step: tau^2 / f0 per loop, a tenth of it as the fixed step
    step = (0.1 * tm.mean(dim=1) ** 2 / cost0).unsqueeze(1)
    last = {}

    def go():
        T = tm.clone()
        for _ in range(iters):
            T.requires_grad_(True)
            _, cost = csp.solve_periodic_batch_autograd(wp, T, order=ORDER, with_cost=True)
            g, = torch.autograd.grad(cost.sum(), T)
            T = project_fixed_total(T.detach() - step * g, total, MIN_TIME)
        last["T"] = T
    us = timed(go, steps, warmup, dev) * 1e3
    cost = csp.solve_periodic_batch(wp, last["T"], order=ORDER, want_cost=True).cost
    return us, float(torch.median(cost / cost0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, S = 65536, 16
    wp, tm = synth.make_batch(B, S, config_id=3)
    wp = torch.from_numpy(np.ascontiguousarray(wp[:, :S])).to(dev)
    tm = torch.from_numpy(tm).to(dev)
    fwd_us, cost0 = forward_with_cost(dev, wp, tm, a.steps, a.warmup)
    cost0 = cost0.clone()
    out = {"tool": "periodic_timeopt_bench", "workload": "C3 as a loop: B=65536 x 16 segments, order 4, fp64, fixed total",
           "periodic_with_cost_grad_us": round(fwd_us, 1), "optimiser": [], "torch_loop": []}
    for k in (10, 100):
        o = optimiser(dev, wp, tm, a.steps, a.warmup, k)
        o["us_per_evaluation_over_forward"] = round(o["us_per_evaluation_upper_bound"] / fwd_us, 3)
        out["optimiser"].append(o)
    for k, o in zip((10, 100), out["optimiser"]):
        us, ratio = torch_loop(dev, wp, tm, k, max(1, a.steps * 5 // k), 1, cost0)
        out["torch_loop"].append({"iterations": k, "loop_us": round(us, 1), "us_per_iteration": round(us / k, 1),
                                  "objective_ratio_median": round(ratio, 4),
                                  "over_optimiser": round(us / o["optimize_us"], 2)})
    # what a caller runs: the default stopping rule, where a lane leaves the loop once it has converged
    out["optimiser_tol_1e-6"] = optimiser(dev, wp, tm, a.steps, a.warmup, 100, 1e-6)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
