"""Reverse-mode kernel (csp_minsnap_solve_batch_vjp) against the generic forward kernel in the same run.

    python tools/vjp_bench.py [--steps K] [--warmup W] [--order O]     (on the GPU box; prints one JSON line)

Shapes: C3 (B = 65536, S = 16, fp64, shared bc, all three gradients) and a ragged batch with S ~ U{4..64}, both at order O
(default 4).  Algorithmic bytes per trajectory: p_bar read (3 S 2o words) + waypoints and times read + their gradients
written, 8 bytes a word -- 4144 B at C3, order 4.  The forward is solve_batch(force_generic=True) on the same inputs."""
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
from bench import HBM_PEAK_GBPS, timed  # noqa: E402
from tests import synth  # noqa: E402

csp = importlib.import_module("cs-pathplan_amd")


def vjp_bytes(S_list, o):
    S = np.asarray(S_list, dtype=np.int64)
    return int(np.sum(8 * (3 * S * 2 * o + 2 * (3 * (S + 1) + S))))


def measure(dev, wp, tm, bc, o, steps, warmup, seg_offsets=None, label=""):
    ragged = seg_offsets is not None
    B = (seg_offsets.numel() - 1) if ragged else tm.shape[0]
    S_list = (seg_offsets[1:] - seg_offsets[:-1]).cpu().numpy() if ragged else np.full(B, tm.shape[1])
    smax = int(S_list.max())
    total = int(S_list.sum())
    gco = torch.randn((total, 3, 2 * o), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    gwp, gtm, gbc = torch.empty_like(wp), torch.empty_like(tm), torch.empty_like(bc)
    desc = csp.make_desc(o, B, 0 if ragged else tm.shape[1], csp.DTYPE_F64, 0.0, 0.0, csp.MEM_DEVICE, bc.shape[0] == B and B != 1,
                         seg_offsets.data_ptr() if ragged else None, smax if ragged else 0, None, dev.index or 0, 0)
    need = csp.vjp_workspace_bytes(desc)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    args = (ctypes.byref(desc), wp.data_ptr(), tm.data_ptr(), bc.data_ptr(), gco.data_ptr(), gwp.data_ptr(), gtm.data_ptr(),
            gbc.data_ptr(), None, ws.data_ptr(), need, st)
    f = csp.raw_lib().csp_minsnap_solve_batch_vjp

    def vjp():
        rc = f(*args)
        if rc:
            csp._check(rc)
    ms_vjp = timed(vjp, steps, warmup, dev)
    prep = csp.PreparedSolve(wp, tm, bc=bc, order=o, force_generic=True, seg_offsets=seg_offsets, max_segments=smax if ragged else None,
                             stream=torch.cuda.current_stream(dev).cuda_stream)
    ms_fwd = timed(prep.run, steps, warmup, dev)
    nbytes = vjp_bytes(S_list, o)
    gbps = nbytes / (ms_vjp * 1e-3) / 1e9
    return {"workload": label, "batch": B, "order": o, "vjp_us": round(ms_vjp * 1e3, 1), "forward_generic_us": round(ms_fwd * 1e3, 1),
            "vjp_over_forward": round(ms_vjp / ms_fwd, 3), "algorithmic_bytes": nbytes,
            "algorithmic_bytes_per_traj": round(nbytes / B, 1), "achieved_GBps": round(gbps, 1),
            "frac_of_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4), "forward_kernel": prep.kernel, "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--order", type=int, default=4, choices=(2, 3, 4, 5))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    o = a.order
    B, S = 65536, 16
    wp, tm = synth.make_batch(B, S, config_id=3)
    bc = torch.from_numpy(np.random.default_rng(0).normal(size=(1, 4, 3))).to(dev)
    out = [measure(dev, torch.from_numpy(wp).to(dev), torch.from_numpy(tm).to(dev), bc, o, a.steps, a.warmup,
                   label="C3: B=65536 x 16 segments, order %d, fp64, shared bc, all gradients" % o)]
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
    out.append(measure(dev, torch.from_numpy(wp_r).to(dev), torch.from_numpy(tm_r).to(dev), bc, o, a.steps, a.warmup,
                       seg_offsets=torch.from_numpy(off).to(dev), label="ragged: B=16384, S ~ U{4..64}, order %d, fp64, shared bc" % o))
    print(json.dumps({"tool": "vjp_bench", "results": out}))


if __name__ == "__main__":
    main()
