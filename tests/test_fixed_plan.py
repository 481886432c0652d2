"""CPU test of the launch plan of the fixed-size solve kernels (cs-pathplan_amd/csrc/minsnap_fixed_plan.h): which path, slice
width, lane mapping, grid, kernel body and store flavour a launch takes, and both sides of every threshold, through the
stand-alone program cs-pathplan_amd/host/fixed_plan_check.cpp.  The GPU suites prove that every flavour writes the same
bits; this one sees which flavour runs.  Expected values are DESIGN.md 5.1 / 5.1.2 / 5.1b worked out by hand:
coefficient bytes of a launch = B * S * 48 * order, against 32 MiB (L2), 256 MiB (Infinity Cache) and 48 MiB (path kernels)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXXFLAGS = ["-std=c++17", "-O1", "-Wall", "-Werror"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fixed_plan") / "fixed_plan_check")
    subprocess.check_call(["g++"] + CXXFLAGS + [os.path.join(ROOT, "cs-pathplan_amd", "host", "fixed_plan_check.cpp"), "-o", out])
    return out


def _run(exe, args, w=None, axis=None, nt=None, policy=None, stagger=None):
    env = ["-" if v is None else v for v in (w, axis, nt, policy, stagger)]
    r = subprocess.run([exe] + [str(a) for a in args] + env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {}
    for kv in r.stdout.split():
        k, v = kv.split("=")
        out[k] = int(v) if v.lstrip("-").isdigit() else v
    return out


def solve(exe, order, S, B, cus=256, flags="p", **env):
    """flags: s segment-major, p persistent (the library's default), b / v per-trajectory boundary conditions / weight, m multi"""
    return _run(exe, ["solve", order, S, B, cus, flags], **env)


def path(exe, order, S, B, **env):
    return _run(exe, ["path", order, S, B], **env)


def whole(n_full, rem, grid, body, store):
    return dict(path="whole", n_full=n_full, rem=rem, grid=grid, body=body, store=store)


def narrow(slice_w, axis_lanes, grid):
    return dict(path="narrow", slice_w=slice_w, axis_lanes=axis_lanes, grid=grid, store="plain")


# ---- order 4, S = 16 (3072 bytes per trajectory): 32 MiB lies between B = 10922 and 10923, 256 MiB between 87381 and 87382 ----
@pytest.mark.parametrize("B,body,store", [(10922, "persistent", "plain"), (10923, "persistent_wt", "wt"),
                                          (87381, "persistent_wt", "wt"), (87382, "persistent", "nt")])
def test_order4_thresholds_of_the_persistent_kernel(exe, B, body, store):
    assert solve(exe, 4, 16, B) == whole(B // 64, B % 64, min(B // 64, 512), body, store)


def test_tail_only_where_the_batch_is_ragged(exe):
    assert solve(exe, 4, 16, 171 * 64) == whole(171, 0, 171, "persistent_wt", "wt")
    assert solve(exe, 4, 16, 171 * 64 + 1)["rem"] == 1
    assert solve(exe, 4, 16, 60000 * 64 + 63) == whole(60000, 63, 512, "persistent", "nt")


@pytest.mark.parametrize("flags", ["-", "pb", "pv", "pbv"])
@pytest.mark.parametrize("B,store", [(10922, "plain"), (10923, "plain"), (87381, "plain"), (87382, "nt")])
def test_one_workgroup_per_slice_never_writes_through(exe, flags, B, store):
    assert solve(exe, 4, 16, B, flags=flags) == whole(B // 64, B % 64, B // 64, "slice", store)


def test_order4_odd_s_is_no_write_through_shape(exe):
    # S = 15: 2880 bytes per trajectory; 32 MiB between 11650 and 11651, 256 MiB between 93206 and 93207
    assert solve(exe, 4, 15, 11651) == whole(182, 3, 182, "persistent", "plain")
    assert solve(exe, 4, 15, 93206) == whole(1456, 22, 512, "persistent", "plain")
    assert solve(exe, 4, 15, 93207) == whole(1456, 23, 512, "persistent", "nt")
    assert solve(exe, 4, 15, 50000, policy="wt")["store"] == "plain"
    # S = 2 is even but has no paired record
    assert solve(exe, 4, 2, 400000) == whole(6250, 0, 512, "persistent", "plain")   # 73 MiB
    assert solve(exe, 4, 2, 400000, policy="wt")["body"] == "persistent"


def test_order4_segment_major(exe):
    for B, store in ((10923, "plain"), (87381, "plain"), (87382, "nt")):
        assert solve(exe, 4, 16, B, flags="sp") == whole(B // 64, B % 64, min(B // 64, 512), "persistent", store)
    for pol in ("wt", "nt"):    # CSP_STORE_POLICY is ignored ...
        assert solve(exe, 4, 16, 10923, flags="sp", policy=pol) == whole(170, 43, 170, "persistent", "plain")
    assert solve(exe, 4, 16, 87382, flags="sp", policy="plain")["store"] == "nt"
    assert solve(exe, 4, 16, 10923, flags="sp", nt="1")["store"] == "nt"   # ... CSP_NT_STORES honoured
    assert solve(exe, 4, 16, 87382, flags="sp", nt="0")["store"] == "plain"
    assert solve(exe, 4, 16, 87382, flags="s") == whole(1365, 22, 1365, "slice", "nt")


def test_segment_major_is_refused_without_an_instantiation(exe):
    for order, S in ((2, 8), (3, 8), (5, 8)):
        assert solve(exe, order, S, 4096, flags="sp") == dict(path="refused")
        assert solve(exe, order, S, 4096, flags="sp", w="16") == dict(path="refused")


# ---- narrow slices ----
def test_narrow_slices_up_to_32_trajectories_per_cu(exe):
    assert solve(exe, 4, 8, 8192) == narrow(16, 1, 512)
    assert solve(exe, 4, 8, 8193) == whole(128, 1, 128, "persistent", "plain")
    assert solve(exe, 4, 8, 2048, cus=64) == narrow(16, 1, 128)
    assert solve(exe, 4, 8, 2049, cus=64) == whole(32, 1, 32, "persistent", "plain")
    assert solve(exe, 4, 8, 17) == narrow(16, 1, 2)
    # the flags that keep a launch off the persistent kernel do not keep it off the narrow path
    assert solve(exe, 4, 8, 4096, flags="bv") == narrow(16, 1, 256)
    # the other orders have no axis-per-lane kernel
    assert solve(exe, 3, 8, 4096) == whole(64, 0, 64, "persistent", "plain")
    assert solve(exe, 5, 8, 100)["path"] == "whole"


def test_narrow_slice_overrides(exe):
    assert solve(exe, 4, 8, 4096, axis="0") == whole(64, 0, 64, "persistent", "plain")
    assert solve(exe, 4, 8, 4096, w="32") == narrow(32, 0, 128)
    assert solve(exe, 4, 8, 100000, w="32") == narrow(32, 0, 3125)    # a forced width holds at every batch size
    assert solve(exe, 4, 8, 4096, w="8") == narrow(8, 1, 512)
    assert solve(exe, 4, 8, 4096, w="8", axis="0") == narrow(8, 0, 512)
    assert solve(exe, 4, 8, 4096, w="64") == whole(64, 0, 64, "persistent", "plain")
    assert solve(exe, 4, 8, 4096, w="7") == narrow(16, 1, 256)        # ignored
    assert solve(exe, 4, 8, 8193, w="7")["path"] == "whole"
    assert solve(exe, 3, 8, 4096, w="16") == narrow(16, 0, 256)
    assert solve(exe, 4, 8, 4096, flags="sp", w="16") == whole(64, 0, 64, "persistent", "plain")
    assert solve(exe, 4, 8, 4096, flags="sp") == whole(64, 0, 64, "persistent", "plain")


# ---- orders 2, 3, 5 ----
@pytest.mark.parametrize("order,S,B", [(2, 4, 699050), (3, 8, 233016), (5, 8, 139810)])   # B * S * 48 * order <= 256 MiB < (B + 1) * ...
def test_other_orders_on_lines_take_the_infinity_cache_rule(exe, order, S, B):
    assert solve(exe, order, S, B) == whole(B // 64, B % 64, 512, "persistent", "plain")
    assert solve(exe, order, S, B + 1) == whole((B + 1) // 64, (B + 1) % 64, 512, "persistent", "nt")
    assert solve(exe, order, S, B + 1, flags="-")["store"] == "nt"
    assert solve(exe, order, S, B + 1, nt="0")["store"] == "plain"
    assert solve(exe, order, S, B + 1, policy="plain")["store"] == "nt"   # CSP_STORE_POLICY is for the write-through shapes
    assert solve(exe, order, S, 70000, policy="wt") == whole(1093, 48, 512, "persistent", "plain")


@pytest.mark.parametrize("order,S", [(2, 3), (3, 5), (5, 3)])
def test_other_orders_off_lines_never_store_non_temporally(exe, order, S):
    B = 3000000   # 0.8 - 2 GiB
    assert solve(exe, order, S, B)["store"] == "plain"
    assert solve(exe, order, S, B, policy="nt")["store"] == "plain"
    assert solve(exe, order, S, B, nt="1")["store"] == "nt"
    assert solve(exe, order, S, 9000, nt="1") == whole(140, 40, 140, "persistent", "nt")
    assert solve(exe, order, S, B, nt="0")["store"] == "plain"


# ---- overrides at a write-through shape (order 4, S = 16) ----
def test_override_precedence_at_a_write_through_shape(exe):
    small, mid, big = 9000, 50000, 100000    # 26 MiB, 146 MiB, 293 MiB
    assert solve(exe, 4, 16, small, policy="wt") == whole(140, 40, 140, "persistent_wt", "wt")
    assert solve(exe, 4, 16, small, policy="wt", flags="-") == whole(140, 40, 140, "slice", "plain")
    assert solve(exe, 4, 16, mid, policy="wt", flags="pb")["store"] == "plain"
    assert solve(exe, 4, 16, big, policy="plain") == whole(1562, 32, 512, "persistent", "plain")
    assert solve(exe, 4, 16, small, policy="nt", nt="0") == whole(140, 40, 140, "persistent", "nt")
    assert solve(exe, 4, 16, big, policy="wt", nt="1")["body"] == "persistent_wt"
    assert solve(exe, 4, 16, mid, policy="plain", nt="1")["store"] == "plain"
    assert solve(exe, 4, 16, small, nt="1") == whole(140, 40, 140, "persistent", "nt")
    assert solve(exe, 4, 16, mid, nt="0") == whole(781, 16, 512, "persistent", "plain")
    assert solve(exe, 4, 16, mid, nt="1")["store"] == "nt"
    assert solve(exe, 4, 16, mid) == whole(781, 16, 512, "persistent_wt", "wt")
    # the smallest write-through shape: S = 4, 768 bytes per trajectory, 32 MiB between 43690 and 43691
    assert solve(exe, 4, 4, 43690)["store"] == "plain"
    assert solve(exe, 4, 4, 43691)["body"] == "persistent_wt"


def test_multi_batch_launch_ignores_everything(exe):
    want = dict(path="multi", slice_w=64, store="plain")
    assert solve(exe, 4, 8, 4096, flags="pm") == want
    assert solve(exe, 4, 16, 50000, flags="pm", w="16", axis="0", nt="1", policy="wt") == want
    assert solve(exe, 3, 8, 1, flags="spbvm", w="8") == want


# ---- path kernels ----
def test_path_kernel_store_rule(exe):
    # order 4, S = 16: B = 16384 writes 48 MiB exactly, and the rule is >=
    assert path(exe, 4, 16, 16383) == dict(grid=256, nt=0, stagger=3)
    assert path(exe, 4, 16, 16384) == dict(grid=256, nt=1, stagger=3)
    assert path(exe, 4, 16, 16385)["grid"] == 257
    # order 3, S = 8 (starts on lines; 1152 bytes per trajectory): 48 MiB between 43690 and 43691
    assert path(exe, 3, 8, 43690)["nt"] == 0 and path(exe, 3, 8, 43691)["nt"] == 1
    assert path(exe, 3, 5, 3000000)["nt"] == 0
    assert path(exe, 2, 3, 3000000)["nt"] == 0
    # order 2, S = 8 (dense, half-height ring; 768 bytes): 48 MiB at B = 65536 exactly
    assert path(exe, 2, 8, 65535)["nt"] == 0 and path(exe, 2, 8, 65536)["nt"] == 1
    # order 4 takes the rule at every S
    assert path(exe, 4, 15, 17476)["nt"] == 0 and path(exe, 4, 15, 17477)["nt"] == 1
    assert path(exe, 4, 16, 64, nt="1")["nt"] == 1 and path(exe, 3, 5, 64, nt="1")["nt"] == 1
    assert path(exe, 4, 16, 524288, nt="0")["nt"] == 0
    assert path(exe, 4, 16, 524288, policy="plain")["nt"] == 1     # CSP_STORE_POLICY is not for these kernels


def test_path_kernel_stagger(exe):
    assert path(exe, 2, 16, 65536)["stagger"] == 4
    assert path(exe, 2, 8, 65536)["stagger"] == 4
    assert path(exe, 2, 7, 65536)["stagger"] == 0
    assert path(exe, 2, 4, 65536)["stagger"] == 0
    assert path(exe, 3, 16, 65536)["stagger"] == 1
    assert path(exe, 3, 7, 65536)["stagger"] == 0
    assert path(exe, 4, 16, 65536)["stagger"] == 3
    assert path(exe, 4, 2, 65536)["stagger"] == 0
    for order, S in ((2, 16), (2, 4), (3, 16), (4, 16)):
        assert path(exe, order, S, 65536, stagger="0")["stagger"] == 0
        assert path(exe, order, S, 65536, stagger="6")["stagger"] == 6
    assert path(exe, 4, 16, 65536, stagger="-1")["stagger"] == 3


# ---- the parser ----
def test_override_parser(exe):
    def env(**kw):
        return _run(exe, ["env"], **kw)
    assert env() == dict(slice_w=0, axis_lanes=1, nt=-1, policy="unset", stagger=-1)
    for s in ("8", "16", "32", "64", "16x"):
        assert env(w=s)["slice_w"] == int(s[:2])
    for s in ("7", "0", "4", "128", "-16", "abc", ""):
        assert env(w=s)["slice_w"] == 0
    for s, on in (("0", 0), ("00", 0), ("0n", 0), ("1", 1), ("", 1), ("off", 1), ("no", 1)):
        assert env(axis=s)["axis_lanes"] == on
    for s, v in (("0", 0), ("0x", 0), ("1", 1), ("2", 1), ("yes", 1), ("", 1), ("no", 1)):
        assert env(nt=s)["nt"] == v
    for s, v in (("wt", "wt"), ("w", "wt"), ("write-through", "wt"), ("nt", "nt"), ("n", "nt"), ("plain", "plain"), ("p", "plain"),
                 ("", "plain"), ("WT", "plain"), ("0", "plain")):
        assert env(policy=s)["policy"] == v
    for s, v in (("0", 0), ("3", 3), ("6", 6), ("abc", 0), ("", 0), ("-2", -2)):
        assert env(stagger=s)["stagger"] == v
