"""The periodic solve's reverse mode (csp_minsnap_solve_periodic_batch_vjp) against its forward in the same run.

    python tools/periodic_vjp_bench.py [--steps K] [--warmup W] [--repeats R]     (on the GPU box; prints one JSON line)

Shapes: C3's as a loop (B = 65536, S = 16, order 4, fp64: the first 16 points of each C3 trajectory) and a ragged loop
batch (B = 16384, S ~ U{4..64}, order 4), as tools/periodic_bench.py.  Per shape: microseconds of the VJP (both
gradients) without and with grad_cost, and of csp_minsnap_solve_periodic_batch with cost and time gradient, each the
median of R alternating rounds of K launches (HIP events), with the spread (min .. max) of the rounds; the ratios are
of the medians."""
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


def measure(dev, wp, tm, o, steps, warmup, repeats, seg_offsets=None, label=""):
    """wp: the loop points ([B,S,3], or [sum S_b,3] ragged), tm: [B,S] (or [sum S_b])."""
    ragged = seg_offsets is not None
    B = (seg_offsets.numel() - 1) if ragged else tm.shape[0]
    smax = int((seg_offsets[1:] - seg_offsets[:-1]).max().item()) if ragged else tm.shape[1]
    desc = csp.make_desc(o, B, 0 if ragged else tm.shape[1], csp.DTYPE_F64, 0.0, 0.0, csp.MEM_DEVICE, False,
                         seg_offsets.data_ptr() if ragged else None, smax if ragged else 0, None, dev.index or 0, 0)
    need_f, need_v = csp.periodic_workspace_bytes(desc), csp.periodic_vjp_workspace_bytes(desc)
    ws = torch.empty(max(need_f, need_v), dtype=torch.uint8, device=dev)
    total = int(tm.numel())
    gen = torch.Generator(dev).manual_seed(7)
    co = torch.empty((total, 3, 2 * o), dtype=torch.float64, device=dev)
    pbar = torch.randn((total, 3, 2 * o), dtype=torch.float64, device=dev, generator=gen)
    jbar = torch.randn(B, dtype=torch.float64, device=dev, generator=gen)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    grad, gtm, gwp = torch.empty_like(tm), torch.empty_like(tm), torch.empty_like(wp)
    stt = torch.empty(B, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lib = csp.raw_lib()

    def forward():
        rc = lib.csp_minsnap_solve_periodic_batch(ctypes.byref(desc), wp.data_ptr(), tm.data_ptr(), co.data_ptr(), cost.data_ptr(),
                                                  grad.data_ptr(), stt.data_ptr(), ws.data_ptr(), need_f, st)
        if rc:
            csp._check(rc)

    def vjp(jb):
        def go():
            rc = lib.csp_minsnap_solve_periodic_batch_vjp(ctypes.byref(desc), wp.data_ptr(), tm.data_ptr(), pbar.data_ptr(), jb,
                                                          gwp.data_ptr(), gtm.data_ptr(), stt.data_ptr(), ws.data_ptr(), need_v, st)
            if rc:
                csp._check(rc)
        return go
    runs = {"forward_with_cost_grad": forward, "vjp": vjp(None), "vjp_with_grad_cost": vjp(jbar.data_ptr())}
    ms = {k: [] for k in runs}
    for r in range(repeats):   # the three alternate, so that a drift of the machine hits them alike
        for k, f in runs.items():
            ms[k].append(timed(f, steps, warmup if r == 0 else 1, dev))
    bad = int((stt.cpu().numpy() != 0).sum())
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"workload": label, "batch": B, "order": o, "steps": steps, "repeats": repeats, "status_nonzero": bad,
           "vjp_workspace_bytes_per_solve": round(need_v / B, 1)}
    for k, v in ms.items():
        out[k + "_us"] = round(med[k] * 1e3, 1)
        out[k + "_us_min_max"] = [round(min(v) * 1e3, 1), round(max(v) * 1e3, 1)]
    out["vjp_over_forward"] = round(med["vjp"] / med["forward_with_cost_grad"], 3)
    out["vjp_with_grad_cost_over_forward"] = round(med["vjp_with_grad_cost"] / med["forward_with_cost_grad"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    o = 4
    B, S = 65536, 16
    wp, tm = synth.make_batch(B, S, config_id=3)
    wp = torch.from_numpy(np.ascontiguousarray(wp[:, :S])).to(dev)
    out = [measure(dev, wp, torch.from_numpy(tm).to(dev), o, a.steps, a.warmup, a.repeats,
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
    out.append(measure(dev, torch.from_numpy(wp_r).to(dev), torch.from_numpy(tm_r).to(dev), o, a.steps, a.warmup, a.repeats,
                       seg_offsets=torch.from_numpy(off).to(dev), label="ragged loops: B=16384, S ~ U{4..64}, order 4, fp64"))
    print(json.dumps({"tool": "periodic_vjp_bench", "results": out}))


if __name__ == "__main__":
    main()
