"""The periodic (closed-loop) solve (csp_minsnap_solve_periodic_batch) against the generic forward kernel in the same run.

    python tools/periodic_bench.py [--steps K] [--warmup W]          (on the GPU box; prints one JSON line)

Shapes: C3's as a loop (B = 65536, S = 16, order 4, fp64: the first 16 points of each C3 trajectory) and a ragged loop
batch (B = 16384, S ~ U{4..64}, order 4).  Per shape: microseconds of the periodic solve with and without cost and time
gradient, and of the generic forward (solve_batch with force_generic) over the same points plus the closing point."""
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


def measure(dev, wp, tm, o, steps, warmup, seg_offsets=None, label=""):
    """wp: the loop points ([B,S,3], or [sum S_b,3] ragged), tm: [B,S] (or [sum S_b])."""
    ragged = seg_offsets is not None
    B = (seg_offsets.numel() - 1) if ragged else tm.shape[0]
    smax = int((seg_offsets[1:] - seg_offsets[:-1]).max().item()) if ragged else tm.shape[1]
    desc = csp.make_desc(o, B, 0 if ragged else tm.shape[1], csp.DTYPE_F64, 0.0, 0.0, csp.MEM_DEVICE, False,
                         seg_offsets.data_ptr() if ragged else None, smax if ragged else 0, None, dev.index or 0, 0)
    need = csp.periodic_workspace_bytes(desc)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    total = int(tm.numel())
    co = torch.empty((total, 3, 2 * o), dtype=torch.float64, device=dev)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    grad = torch.empty_like(tm)
    stt = torch.empty(B, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    f = csp.raw_lib().csp_minsnap_solve_periodic_batch

    def run(c, g):
        def go():
            rc = f(ctypes.byref(desc), wp.data_ptr(), tm.data_ptr(), co.data_ptr(), c, g, stt.data_ptr(), ws.data_ptr(),
                   need, st)
            if rc:
                csp._check(rc)
        return go
    ms_p = timed(run(None, None), steps, warmup, dev)
    ms_pc = timed(run(cost.data_ptr(), grad.data_ptr()), steps, warmup, dev)
    s = stt.cpu().numpy()
    # the open chain over the same points and the closing point
    if ragged:
        off = seg_offsets.cpu().numpy()
        lens = np.diff(off)
        idx = np.empty(total + B, dtype=np.int64)
        idx[np.arange(total) + np.repeat(np.arange(B), lens)] = np.arange(total)
        idx[off[:-1] + np.arange(B) + lens] = off[:-1]
        chain = wp[torch.from_numpy(idx).to(dev)]
    else:
        chain = torch.cat([wp, wp[:, :1]], dim=1)
    bc = torch.zeros((1, 4, 3), dtype=torch.float64, device=dev)
    prep = csp.PreparedSolve(chain.contiguous(), tm, bc=bc, order=o, force_generic=True, seg_offsets=seg_offsets,
                             max_segments=smax if ragged else None, stream=torch.cuda.current_stream(dev).cuda_stream)
    ms_f = timed(prep.run, steps, warmup, dev)
    return {"workload": label, "batch": B, "order": o, "periodic_us": round(ms_p * 1e3, 1),
            "periodic_with_cost_grad_us": round(ms_pc * 1e3, 1), "forward_generic_us": round(ms_f * 1e3, 1),
            "periodic_over_forward": round(ms_p / ms_f, 3), "periodic_with_cost_grad_over_forward": round(ms_pc / ms_f, 3),
            "workspace_bytes_per_solve": round(need / B, 1), "status_nonzero": int((s != 0).sum()),
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
    wp = torch.from_numpy(np.ascontiguousarray(wp[:, :S])).to(dev)
    out = [measure(dev, wp, torch.from_numpy(tm).to(dev), o, a.steps, a.warmup,
                   label="C3 as a loop: B=65536 x 16 segments, order 4, fp64")]
    Br = 16384
    rng = np.random.default_rng(5)
    lens = rng.integers(4, 65, size=Br)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    wp_r = np.empty((int(off[-1]), 3))
    for b in range(Br):
        p0 = rng.uniform(-10, 10, size=(1, 3))
        wp_r[off[b]:off[b + 1]] = p0 + np.cumsum(rng.normal(size=(lens[b], 3)), axis=0)
    tm_r = rng.uniform(0.5, 2.0, size=int(off[-1]))
    out.append(measure(dev, torch.from_numpy(wp_r).to(dev), torch.from_numpy(tm_r).to(dev), o, a.steps, a.warmup,
                       seg_offsets=torch.from_numpy(off).to(dev), label="ragged loops: B=16384, S ~ U{4..64}, order 4, fp64"))
    print(json.dumps({"tool": "periodic_bench", "results": out}))


if __name__ == "__main__":
    main()
