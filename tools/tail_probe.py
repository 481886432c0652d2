#!/usr/bin/env python3
"""Diagnostic: how much of the headline launch lies after its last wave has ended?

    python tools/tail_probe.py [--batch B] [--json out.json]              # needs build.py --stamps; run it under
                                                                          # rocprofv3 --kernel-trace to get its trace
    python tools/tail_probe.py --summarise out.json --trace-dir DIR [--kernel-us X]

The stamps build records a real-time stamp (100 MHz) at each wave's start and after its last store is issued.  The first
form runs the launch and prints: first wave start -> last wave end, and the spread of the wave end times.  The second
form sets that span against the SAME launch's duration in the rocprofv3 kernel trace of that run: duration - span is the
part of the launch outside every wave (dispatch in front, cache write-back behind).  --kernel-us is the duration of the
normal build (its own rocprofv3 run), against which the shares are quoted.  Shares and differences only -- never quote
the stamps build's run time."""
import argparse
import csv
import ctypes
import glob
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNEL = "minsnap_fixed_persistent"


def run(args):
    import torch
    from tests import synth
    csp = importlib.import_module("cs-pathplan_amd")
    lib = ctypes.CDLL(os.path.join(ROOT, "cs-pathplan_amd", "libcsp_minsnap_stamps.so"))
    lib.csp_minsnap_solve_batch.restype = ctypes.c_int
    lib.csp_minsnap_solve_batch.argtypes = [ctypes.POINTER(csp.Desc)] + [ctypes.c_void_p] * 7 + [ctypes.c_size_t, ctypes.c_void_p]
    lib.csp_minsnap_workspace_bytes.restype = ctypes.c_size_t
    lib.csp_minsnap_workspace_bytes.argtypes = [ctypes.POINTER(csp.Desc)]
    lib.csp_minsnap_kernel_name.restype = ctypes.c_char_p
    lib.csp_minsnap_kernel_name.argtypes = [ctypes.POINTER(csp.Desc)]
    csp._lib = lib  # route the binding through the diagnostic library
    B, S = args.batch, 16
    wp, tm = synth.make_batch(B, S)
    d_wp, d_tm = torch.from_numpy(wp).cuda(), torch.from_numpy(tm).cuda()
    prep = csp.PreparedSolve(d_wp, d_tm, order=4)
    recs = []
    n = 4096 * 8
    buf = (ctypes.c_ulonglong * n)()
    for it in range(args.launches):
        prep.run()
        torch.cuda.synchronize()
        # every translation unit has its own stamp buffer: the launch went to whichever holds the newest stamp
        raws = []
        for reader in (lib.csp_debug_read_stamps, lib.csp_debug_read_stamps_wt):
            reader(buf, n)
            raws.append(np.frombuffer(buf, dtype=np.uint64).reshape(-1, 8)[:4096].astype(np.int64))
        raw = max(raws, key=lambda r: r[:, 6].max())
        raw = raw[(raw[:, 5] > 0) & (raw[:, 6] > 0)]        # rows a wave actually wrote
        rt0, rt1 = raw[:, 5], raw[:, 6]
        end = (rt1 - rt0.min()) / 100.0
        recs.append({"waves": int(len(raw)), "span_us": float(end.max()),
                     "start_spread_us": float((rt0.max() - rt0.min()) / 100.0),
                     "end_spread_us": float(end.max() - end.min()),
                     "end_p10_us": float(np.percentile(end, 10)), "end_p50_us": float(np.percentile(end, 50)),
                     "end_p90_us": float(np.percentile(end, 90))})
    keep = recs[args.launches // 2:]      # the first launches warm the clocks
    out = {"B": B, "S": S, "store_policy_env": os.environ.get("CSP_STORE_POLICY"), "launches": recs,
           "median": {k: float(np.median([r[k] for r in keep])) for k in keep[0]}}
    print(json.dumps(out["median"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


def summarise(args):
    with open(args.summarise) as f:
        doc = json.load(f)
    durs = []
    for path in glob.glob(os.path.join(args.trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows = [r for r in csv.DictReader(f) if KERNEL in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        durs += [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    assert len(durs) == len(doc["launches"]), (len(durs), len(doc["launches"]))
    half = len(durs) // 2
    outside = [d - r["span_us"] for d, r in zip(durs, doc["launches"])][half:]
    m = doc["median"]
    res = {"B": doc["B"], "store_policy_env": doc["store_policy_env"],
           "first_start_to_last_end_us": round(m["span_us"], 2), "wave_end_spread_us": round(m["end_spread_us"], 2),
           "wave_end_p10_p50_p90_us": [round(m[k], 2) for k in ("end_p10_us", "end_p50_us", "end_p90_us")],
           "wave_start_spread_us": round(m["start_spread_us"], 2),
           "outside_waves_us": {"median": round(float(np.median(outside)), 2), "min": round(min(outside), 2), "max": round(max(outside), 2)},
           "note": "outside_waves = traced duration of the stamped launch - (first wave start -> last wave end): dispatch in front plus write-back behind"}
    if args.kernel_us:
        res["normal_build_kernel_us"] = args.kernel_us
        res["outside_waves_share_of_normal_kernel"] = round(float(np.median(outside)) / args.kernel_us, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--json")
    ap.add_argument("--summarise")
    ap.add_argument("--trace-dir")
    ap.add_argument("--kernel-us", type=float)
    a = ap.parse_args()
    summarise(a) if a.summarise else run(a)
