"""CPU test of the launch plans of the evaluation kernels (cs-pathplan_amd/csrc/minsnap_eval_plan.h) through the
stand-alone program cs-pathplan_amd/host/eval_plan_check.cpp: tile sizes and LDS bytes over the whole supported range,
and the plans of the shapes the GPU tests and the benchmark use, worked out by hand."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXXFLAGS = ["-std=c++17", "-O1", "-Wall", "-Werror"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("eval_plan") / "eval_plan_check")
    subprocess.check_call(["g++"] + CXXFLAGS + [os.path.join(ROOT, "cs-pathplan_amd", "host", "eval_plan_check.cpp"), "-o", out])
    return out


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}


def test_lds_and_tiles_over_the_whole_supported_range(exe):
    s = _run(exe, "sweep")
    assert s["bad"] == 0
    assert s["max_lds"] <= 163840           # what a CU has
    assert s["max_lds"] <= 65536            # and no launch needs more than the default dynamic limit
    assert s["min_tb"] >= 1 and s["min_qt"] >= 1
    assert s["max_slots"] <= 2048
    assert s["max_record_lanes"] <= s["threads"] == 256


def _common(tb, smax):
    return tb * (smax + 1) * 8 + tb * 8 + (3 * tb + 1) // 2 * 2 * 4


def test_plan_of_the_benchmark_shape(exe):
    # S = 16, Q = 32, B = 65536: 64 trajectories per forward workgroup; 85 // 16 = 5 per reverse workgroup, one block
    p = _run(exe, "plan", 16, 32, 65536)
    assert (p["fwd_tb"], p["fwd_grid"], p["fwd_lds"]) == (64, 1024, _common(64, 16))
    assert (p["vjp_tb"], p["vjp_qt"], p["vjp_blocks"], p["vjp_grid"]) == (5, 32, 1, 13108)
    assert p["vjp_lds"] == _common(5, 16) + (5 * 16 + 5) * 8 + 160 * 20


@pytest.mark.parametrize("smax,Q,tb,qt,blocks", [(1, 65, 64, 32, 1), (2, 7, 42, 7, 1), (17, 64, 5, 64, 1), (17, 65, 5, 65, 1),
                                                  (64, 9, 1, 9, 1), (85, 1, 1, 1, 1), (86, 1, 1, 1, 2), (1024, 130, 1, 130, 13),
                                                  (1024, 5000, 1, 2048, 13), (16, 0, 5, 0, 1)])
def test_reverse_plans_at_the_thresholds(exe, smax, Q, tb, qt, blocks):
    p = _run(exe, "plan", smax, Q, 65)
    assert (p["vjp_tb"], p["vjp_qt"], p["vjp_blocks"]) == (tb, qt, blocks)
    assert p["vjp_grid"] == -(-65 // tb)
    slots = (tb * qt + 1) // 2 * 2
    assert p["vjp_lds"] == _common(tb, smax) + (tb * smax + tb) * 8 + slots * 20


@pytest.mark.parametrize("smax,tb", [(1, 64), (16, 64), (17, 60), (1024, 1), (1000, 1), (512, 2)])
def test_forward_plans(exe, smax, tb):
    p = _run(exe, "plan", smax, 9, 70)
    assert p["fwd_tb"] == tb and p["fwd_grid"] == -(-70 // tb) and p["fwd_lds"] == _common(tb, smax)
