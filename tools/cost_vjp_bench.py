"""The open-chain solve's reverse mode with a cost cotangent (csp_minsnap_solve_batch_cost_vjp) against the entries that
existed before it, in the same run.

    python tools/cost_vjp_bench.py [--steps K] [--warmup W] [--repeats R]     (on the GPU box; prints one JSON line)

Shapes: C3 (B = 65536, S = 16, order 4, fp64) and a ragged batch (B = 16384, S ~ U{4..64}, order 4).  Per shape,
microseconds of
  cost_only  the new entry with grad_cost alone (three gradients; the bc is shared, so its gradient takes the second,
             one-wave reduce kernel -- cost_only_no_grad_bc is the same call without grad_bc),
  combined   the new entry with both cotangents,
  vjp        csp_minsnap_solve_batch_vjp,
  cost_pass  csp_minsnap_cost_batch with its time gradient,
  detour     what a caller had to do before: p_bar = 2 J_bar Q(T) p built with torch ops from the forward's coefficients
             (w = 0; the explicit T terms the times would need on top are left out), then csp_minsnap_solve_batch_vjp,
each the median of R alternating rounds of K launches (HIP events), with the spread (min .. max) of the rounds; the
ratios are of the medians."""
import argparse
import ctypes
import importlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import timed  # noqa: E402
from tests import synth  # noqa: E402

csp = importlib.import_module("cs-pathplan_amd")


def _q_tables(o, dev):
    """Q_ik(T) = s_i(T) H_ik s_k(T) T over monomial coefficients (highest power first): s_i = a_i T^(e_i - o) with
    e_i = 2o-1-i and a_i = e_i! / (e_i - o)! for e_i >= o (else 0), H_ik = 1 / (e_i + e_k - 2o + 1)."""
    m = 2 * o
    e = np.arange(m - 1, -1, -1)
    a = np.array([math.factorial(k) / math.factorial(k - o) if k >= o else 0.0 for k in e])
    H = np.array([[1.0 / (ei + ek - 2 * o + 1) if ei >= o and ek >= o else 0.0 for ek in e] for ei in e])
    expo = np.maximum(e - o, 0).astype(np.float64)
    return torch.from_numpy(a).to(dev), torch.from_numpy(H).to(dev), torch.from_numpy(expo).to(dev)


def measure(dev, wp, tm, o, steps, warmup, repeats, seg_offsets=None, label=""):
    """wp: [B,S+1,3] (or [sum (S_b+1),3] ragged), tm: [B,S] (or [sum S_b])."""
    ragged = seg_offsets is not None
    B = (seg_offsets.numel() - 1) if ragged else tm.shape[0]
    lens = (seg_offsets[1:] - seg_offsets[:-1]) if ragged else torch.full((B,), tm.shape[1], dtype=torch.int64, device=dev)
    smax = int(lens.max().item())
    desc = csp.make_desc(o, B, 0 if ragged else tm.shape[1], csp.DTYPE_F64, 0.0, 0.0, csp.MEM_DEVICE, False,
                         seg_offsets.data_ptr() if ragged else None, smax if ragged else 0, None, dev.index or 0, 0)
    need = {"cost_only": csp.cost_vjp_workspace_bytes(desc, False), "combined": csp.cost_vjp_workspace_bytes(desc, True),
            "vjp": csp.vjp_workspace_bytes(desc), "cost_pass": csp.cost_workspace_bytes(desc)}
    ws = torch.empty(max(need.values()), dtype=torch.uint8, device=dev)
    total = int(tm.numel())
    gen = torch.Generator(dev).manual_seed(7)
    bc = torch.zeros((1, 4, 3), dtype=torch.float64, device=dev)
    pbar = torch.randn((total, 3, 2 * o), dtype=torch.float64, device=dev, generator=gen)
    jbar = torch.randn(B, dtype=torch.float64, device=dev, generator=gen)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    gwp, gtm, gbc = torch.empty_like(wp), torch.empty_like(tm), torch.empty_like(bc)
    stt = torch.empty(B, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lib = csp.raw_lib()
    kw = dict(order=o, seg_offsets=seg_offsets) if ragged else dict(order=o)
    co = csp.solve_batch(wp, tm, bc, **kw).coeffs.reshape(total, 3, 2 * o)   # the forward's coefficients: the detour's input
    a_i, H, expo = _q_tables(o, dev)

    def check(rc):
        if rc:
            csp._check(rc)

    def cost_vjp(gco, key, want_bc=True):
        def go():
            check(lib.csp_minsnap_solve_batch_cost_vjp(ctypes.byref(desc), wp.data_ptr(), tm.data_ptr(), bc.data_ptr(), gco,
                                                       jbar.data_ptr(), gwp.data_ptr(), gtm.data_ptr(),
                                                       gbc.data_ptr() if want_bc else None, stt.data_ptr(), ws.data_ptr(),
                                                       need[key], st))
        return go

    def vjp(gco=None):
        check(lib.csp_minsnap_solve_batch_vjp(ctypes.byref(desc), wp.data_ptr(), tm.data_ptr(), bc.data_ptr(),
                                              (pbar if gco is None else gco).data_ptr(), gwp.data_ptr(), gtm.data_ptr(),
                                              gbc.data_ptr(), stt.data_ptr(), ws.data_ptr(), need["vjp"], st))

    def cost_pass():
        check(lib.csp_minsnap_cost_batch(ctypes.byref(desc), wp.data_ptr(), tm.data_ptr(), bc.data_ptr(), cost.data_ptr(),
                                         gtm.data_ptr(), stt.data_ptr(), ws.data_ptr(), need["cost_pass"], st))

    def detour():
        T = tm.reshape(total, 1)
        s = a_i * T ** expo                                        # [total, 2o]
        r = torch.matmul(co * s[:, None, :], H)                    # H is symmetric
        jseg = torch.repeat_interleave(jbar, lens, output_size=total)
        vjp((2.0 * jseg * T[:, 0])[:, None, None] * r * s[:, None, :])

    # the detour is the cost-only call's gradient by another road (waypoints): one look before timing
    cost_vjp(None, "cost_only")()
    ref = gwp.clone()
    detour()
    agree = float(((gwp - ref).abs().max() / ref.abs().max()).item())
    runs = {"cost_only": cost_vjp(None, "cost_only"), "cost_only_no_grad_bc": cost_vjp(None, "cost_only", False),
            "combined": cost_vjp(pbar.data_ptr(), "combined"), "vjp": vjp, "cost_pass": cost_pass, "detour": detour}
    ms = {k: [] for k in runs}
    for r in range(repeats):   # they alternate, so that a drift of the machine hits them alike
        for k, f in runs.items():
            ms[k].append(timed(f, steps, warmup if r == 0 else 1, dev))
    bad = int((stt.cpu().numpy() != 0).sum())
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"workload": label, "batch": B, "order": o, "steps": steps, "repeats": repeats, "status_nonzero": bad,
           "detour_vs_cost_only_rel_diff": agree,
           "workspace_bytes_per_solve": {k: round(v / B, 1) for k, v in need.items()}}
    for k, v in ms.items():
        out[k + "_us"] = round(med[k] * 1e3, 1)
        out[k + "_us_min_max"] = [round(min(v) * 1e3, 1), round(max(v) * 1e3, 1)]
    for k in ("vjp", "detour", "cost_pass"):
        out["cost_only_over_" + k] = round(med["cost_only"] / med[k], 3)
    out["combined_over_vjp"] = round(med["combined"] / med["vjp"], 3)
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
    out = [measure(dev, torch.from_numpy(wp).to(dev), torch.from_numpy(tm).to(dev), o, a.steps, a.warmup, a.repeats,
                   label="C3: B=65536 x 16 segments, order 4, fp64")]
    Br = 16384
    rng = np.random.default_rng(5)
    lens = rng.integers(4, 65, size=Br)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    wp_r = np.empty((int(off[-1]) + Br, 3))
    for b in range(Br):
        p0 = rng.uniform(-10, 10, size=(1, 3))
        wp_r[off[b] + b:off[b + 1] + b + 1] = p0 + np.cumsum(rng.normal(size=(lens[b] + 1, 3)), axis=0)
    tm_r = rng.uniform(0.5, 2.0, size=int(off[-1]))
    out.append(measure(dev, torch.from_numpy(wp_r).to(dev), torch.from_numpy(tm_r).to(dev), o, a.steps, a.warmup, a.repeats,
                       seg_offsets=torch.from_numpy(off).to(dev), label="ragged: B=16384, S ~ U{4..64}, order 4, fp64"))
    print(json.dumps({"tool": "cost_vjp_bench", "results": out}))


if __name__ == "__main__":
    main()
