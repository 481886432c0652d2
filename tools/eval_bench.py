"""Trajectory evaluation at query times (csp_minsnap_eval_batch) and its reverse mode (csp_minsnap_eval_batch_vjp)
against a restatement in torch ops, in the same process.

    python tools/eval_bench.py [--steps K] [--warmup W] [--repeats R]     (on the GPU box; prints one JSON line)

Shape: C3's (B = 65536, S = 16, order 4, fp64; the coefficients are csp_minsnap_solve_batch's), Q = 32 queries per
trajectory uniform in [-0.05, 1.05] of the trajectory's duration, D = 3 (position, velocity, acceleration).
Per entry: microseconds, the median of R alternating rounds of K launches (HIP events), with the spread (min .. max) of
the rounds; algorithmic bytes per second (forward: times + coefficients + queries in, values out; reverse: times +
coefficients + queries + grad_out in, the three gradients out) and that rate's fraction of the 8 TB/s HBM peak.  The
torch restatement is searchsorted + gather + powers for the forward and its autograd backward (on a retained graph, so
that the backward alone is timed); its outputs are compared with the kernels' before anything is timed."""
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
HBM_PEAK = 8.0e12


def torch_eval(times, coeffs, query, D):
    """The contract of csp_minsnap_eval_batch in torch ops: [B,Q,D,3]."""
    B, S = times.shape
    M = coeffs.shape[-1]
    cum = torch.cat([times.new_zeros((B, 1)), torch.cumsum(times, dim=1)], dim=1)
    tc = torch.minimum(torch.clamp(query, min=0.0), cum[:, -1:])
    j = torch.clamp(torch.searchsorted(cum.detach(), tc.detach(), right=True) - 1, max=S - 1)
    tau = tc - torch.gather(cum, 1, j)
    rec = torch.gather(coeffs, 1, j[:, :, None, None].expand(B, query.shape[1], 3, M))      # [B,Q,3,M]
    p = torch.arange(M - 1, -1, -1, device=times.device)
    rows = []
    for d in range(D):
        ff = torch.ones(M, dtype=times.dtype, device=times.device)
        for i in range(d):
            ff = ff * torch.clamp(p - i, min=0)
        pw = tau[:, :, None] ** torch.clamp(p - d, min=0)                                    # [B,Q,M]
        rows.append((rec * (ff * pw)[:, :, None, :]).sum(dim=-1))
    return torch.stack(rows, dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, S, o, Q, D = 65536, 16, 4, 32, 3
    M = 2 * o
    wp, tm = synth.make_batch(B, S, config_id=3)
    times = torch.from_numpy(tm).to(dev)
    coeffs = csp.solve_batch(torch.from_numpy(wp).to(dev), times, order=o).coeffs
    gen = torch.Generator(dev).manual_seed(11)
    u = torch.rand((B, Q), dtype=torch.float64, device=dev, generator=gen) * 1.1 - 0.05
    query = u * times.sum(dim=1, keepdim=True)
    gout = torch.randn((B, Q, D, 3), dtype=torch.float64, device=dev, generator=gen)
    out = torch.empty((B, Q, D, 3), dtype=torch.float64, device=dev)
    gco, gtm, gq = torch.empty_like(coeffs), torch.empty_like(times), torch.empty_like(query)
    desc = csp.make_desc(o, B, S, csp.DTYPE_F64, mem_space=csp.MEM_DEVICE, device_id=dev.index or 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lib = csp.raw_lib()

    def forward():
        rc = lib.csp_minsnap_eval_batch(ctypes.byref(desc), times.data_ptr(), coeffs.data_ptr(), query.data_ptr(), Q, D,
                                        out.data_ptr(), None, None, st)
        if rc:
            csp._check(rc)

    def vjp():
        rc = lib.csp_minsnap_eval_batch_vjp(ctypes.byref(desc), times.data_ptr(), coeffs.data_ptr(), query.data_ptr(), Q, D,
                                            gout.data_ptr(), gco.data_ptr(), gtm.data_ptr(), gq.data_ptr(), None, st)
        if rc:
            csp._check(rc)

    leaves = [x.detach().clone().requires_grad_(True) for x in (coeffs, times, query)]
    graph = torch_eval(leaves[1], leaves[0], leaves[2], D)

    def torch_forward():
        with torch.no_grad():
            torch_eval(times, coeffs, query, D)

    def torch_backward():
        torch.autograd.grad(graph, leaves, gout, retain_graph=True)

    # the restatement computes what the kernels compute
    forward()
    vjp()
    tg = torch.autograd.grad(graph, leaves, gout, retain_graph=True)
    scale = lambda x: float(x.abs().max())
    agree = {"values": float((graph.detach() - out).abs().max()) / scale(out),
             "grad_coeffs": float((tg[0] - gco).abs().max()) / scale(gco),
             "grad_times": float((tg[1] - gtm).abs().max()) / scale(gtm),
             "grad_query": float((tg[2] - gq).abs().max()) / scale(gq)}
    assert all(v < 1e-9 for v in agree.values()), agree

    runs = {"eval": forward, "eval_vjp": vjp, "torch_forward": torch_forward, "torch_backward": torch_backward}
    ms = {k: [] for k in runs}
    for r in range(a.repeats):   # the four alternate, so that a drift of the machine hits them alike
        for k, f in runs.items():
            ms[k].append(timed(f, a.steps, a.warmup if r == 0 else 1, dev))
    n_in = 8 * (B * S + B * S * 3 * M + B * Q)
    fwd_bytes = n_in + 8 * B * Q * D * 3
    vjp_bytes = n_in + 8 * B * Q * D * 3 + 8 * (B * S * 3 * M + B * S + B * Q)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = {"tool": "eval_bench", "workload": "C3: B=65536 x 16 segments, order 4, fp64; Q=32, D=3", "steps": a.steps,
           "repeats": a.repeats, "max_rel_difference_to_torch": {k: float("%.2e" % v) for k, v in agree.items()},
           "forward_bytes": fwd_bytes, "vjp_bytes": vjp_bytes}
    for k, v in ms.items():
        res[k + "_us"] = round(med[k] * 1e3, 1)
        res[k + "_us_min_max"] = [round(min(v) * 1e3, 1), round(max(v) * 1e3, 1)]
    for k, nbytes in (("eval", fwd_bytes), ("eval_vjp", vjp_bytes), ("torch_forward", fwd_bytes), ("torch_backward", vjp_bytes)):
        rate = nbytes / (med[k] * 1e-3)
        res[k + "_algorithmic_TBps"] = round(rate / 1e12, 3)
        res[k + "_fraction_of_hbm_peak"] = round(rate / HBM_PEAK, 3)
    res["torch_forward_over_eval"] = round(med["torch_forward"] / med["eval"], 2)
    res["torch_backward_over_eval_vjp"] = round(med["torch_backward"] / med["eval_vjp"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
