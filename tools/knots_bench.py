"""The solve with per-knot derivative constraints (csp_minsnap_solve_knots_batch) against the generic forward kernel in
the same run.

    python tools/knots_bench.py [--steps K] [--warmup W]          (on the GPU box; prints one JSON line)

Shape: C3's (B = 65536, S = 16, order 4, fp64).  Three masks over the same waypoints and times: the standard problem
(knots_from_bc), a free end, and a velocity pinned at every fourth waypoint; each with and without the cost.  The
yardstick is solve_batch(force_generic=True) on the standard problem: the same one-lane-per-trajectory sweep over
S - 1 knots instead of S + 1."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    o, B, S = 4, 65536, 16
    n = o - 1
    wp, tm = synth.make_batch(B, S, config_id=3)
    rng = np.random.default_rng(20)
    bc = rng.normal(size=(1, 4, 3))
    mask, values = csp.knots_from_bc(bc, S, o, batch=B)
    values[:, 1:S] = rng.normal(size=(B, S - 1, n, 3))      # read only where a mask pins them
    masks = {"standard": mask, "free_end": mask.copy(), "pinned_every_4th": mask.copy()}
    masks["free_end"][:, S] = 0
    masks["pinned_every_4th"][:, 4:S:4] |= 1
    d_wp, d_tm, d_bc, d_kv = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (wp, tm, bc, values))
    desc = csp.make_desc(o, B, S, csp.DTYPE_F64, 0.0, 0.0, csp.MEM_DEVICE, False, None, 0, None, dev.index or 0, 0)
    need = csp.knots_workspace_bytes(desc)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    co = torch.empty((B, S, 3, 2 * o), dtype=torch.float64, device=dev)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    stt = torch.empty(B, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    f = csp.raw_lib().csp_minsnap_solve_knots_batch

    def run(d_mk, c):
        def go():
            rc = f(ctypes.byref(desc), d_wp.data_ptr(), d_tm.data_ptr(), d_mk.data_ptr(), d_kv.data_ptr(), co.data_ptr(), c,
                   stt.data_ptr(), ws.data_ptr(), need, st)
            if rc:
                csp._check(rc)
        return go
    prep = csp.PreparedSolve(d_wp, d_tm, bc=d_bc, order=o, force_generic=True, stream=torch.cuda.current_stream(dev).cuda_stream)
    ms_f = timed(prep.run, a.steps, a.warmup, dev)
    out = {"tool": "knots_bench", "workload": "C3: B=65536 x 16 segments, order 4, fp64", "forward_generic_us": round(ms_f * 1e3, 1),
           "forward_kernel": prep.kernel, "workspace_bytes_per_solve": round(need / B, 1), "steps": a.steps, "masks": {}}
    for name, mk in masks.items():
        d_mk = torch.from_numpy(mk).to(dev)
        ms = timed(run(d_mk, None), a.steps, a.warmup, dev)
        ms_c = timed(run(d_mk, cost.data_ptr()), a.steps, a.warmup, dev)
        bad = int((stt.cpu().numpy() != 0).sum())
        out["masks"][name] = {"knots_us": round(ms * 1e3, 1), "knots_with_cost_us": round(ms_c * 1e3, 1),
                              "knots_over_forward": round(ms / ms_f, 3), "knots_with_cost_over_forward": round(ms_c / ms_f, 3),
                              "status_nonzero": bad}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
