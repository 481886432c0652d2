"""Memory and isolation contracts of the workspace-free kernels, driven through raw pointers with every buffer inside a
guarded allocation (tests/guarded.py), after the pattern of tests/test_gpu_bounds.py (which does the same for the entries
that take a caller's workspace).

Arms covered (FastCase.arm; read off launch_s / fixed_supported / pick_kernel, and checked against a restatement of
those rules on the CPU by test_case_table_names_its_kernels):

  persistent -- fixed_o{2..5}: persistent workgroups + a separate tail launch (shared bc, no per-trajectory weights), every
                store scheme (record at a time, whole-line ring with the line cut by / on the role boundary, order-4 single
                records, pairs, a middle pair stored singly, odd S), B = 64*3 + 5 (one slice per workgroup) and
                64*(2 CUs + 3) + 5 (workgroups walk several slices); order 4 from B = 32 CUs + 64*3 + 5 on
  slice      -- the same shapes with one workgroup per slice (per-trajectory bc, per-trajectory weights or
                CSP_FLAG_NO_PERSISTENT), B in {64, 65, 64*3 + 63}; order 4 at 32 CUs + 64 and 32 CUs + 64*3 + 5
  tail       -- the tail launch alone, B in {1, 63}, orders 2, 3, 5
  axis3      -- order 4 up to 32 CUs trajectories: three lanes per trajectory in slices of 16, B in {1, 15, 16, 17, 33, 130}
  segmajor   -- CSP_FLAG_SEGMENT_MAJOR (order 4): S in {2, 7, 16} x B in {1, 65, 32 CUs + 64*3 + 5}
  path       -- fixedpath_o{2,3,4} (path_weight = 0.7), both sides of order 2's dense-residency switch, with and without
                max_dev / status
  chunked    -- chunked_o{2..5}: fp32 storage at S <= 16 (odd order: 8-byte store pieces), fp64 at S = 1, both types at
                S in {17, 33, 64, 65, 256}, ragged batches with max_segments at the true maximum and at 32
  and csp_minsnap_solve_multi, csp_minsnap_time_alloc_batch, _plan_batch, _sample_batch, _generate_batch.

Contracts, per case:
  A. guard bands   -- outputs start as 0x5A bytes; no band byte of any buffer (inputs, seg_offsets, weights included) and no
                      input byte changes; status 0; coefficients bit-equal with the Python binding's call
  B. stale memory  -- the same call over 0x00- and 0xFF-filled outputs gives the same bits and leaves no all-ones element in
                      anything the header says is written (max_dev and status included, on every arm)
  C. alignment     -- waypoints, times, bc and coeffs each 16 bytes past a 256-byte boundary (coeffs 8 bytes past it for the
                      chunked kernel with fp32 storage of odd order): same bits; one step further (8 where 16 is required, 4
                      where 8 is) returns CSP_ERR_INVALID_ARG and writes nothing
  D. precision     -- against the long-double structured reference at TOL_LD / TOL_F32 of tests/test_gpu_edges.py; the path
                      kernels against the dense oracle at TOL_PEN and the max_dev gate of test_path_penalty_register_kernel
  E. store flavour -- CSP_STORE_POLICY=nt / wt and CSP_NT_STORES=1 in child processes: guard bands there, bits equal here
  F. bad lanes     -- zero / NaN / negative times, a NaN / inf waypoint on one axis, a NaN boundary condition in single
                      trajectories: status non-zero on exactly those, every other trajectory bit-equal to a benign run

Band size.  A fast kernel's plausible worst single mistake is a tail launch treated as a full slice: 64 x S x 48 x order
bytes, at most 64 * 16 * 192 = 245,760 (order 5 stops at S = 8: 122,880).  BAND = 256 KiB covers it, so whatever these
tests can detect stays inside the test's own allocation.  No test here aims at a fault.

Loop bounds for the bad-lane inputs (read in the kernels).  fixed_body / persistent_role_loop (minsnap_fixed_impl.h): the
segment loops are unrolled over the template parameter S, the slice loop runs to n_slices (a launch argument), the only
`while` walks the multi table to mt.n <= 32.  path_sweep (minsnap_fixed_path_impl.h): the same unrolled loops, the t* pick
is 17 fixed samples whose winner is an index 0..16 set by comparisons (a NaN loses every comparison and keeps the
initial index), the only other loops run to a.stagger, a launch argument.  chunked_body / iface_solve
(minsnap_chunked_impl.h, minsnap_iface.h): every loop is bounded by CMAX = 4, N = order - 1, M = 2 order or the lanes per
trajectory, which follow max_segments; the segment count of a ragged trajectory comes from seg_offsets, which stay
benign.  No loop anywhere is bounded by a value computed from waypoints, times or bc.

Measured per-power maxima against the long-double reference (MI355X, every unpenalised case of this file; the gates are
TOL_LD = 1e-14 / 5e-12 / 2e-10 / 7e-8 at orders 2 / 3 / 4 / 5 and TOL_F32 = 3e-7, unchanged):
                                  order 2    order 3    order 4    order 5
  fixed_o* (every launch form)    2.5e-15    1.7e-13    8.9e-11    2.9e-9
  chunked_o*, fp64 storage        1.4e-15    5.9e-14    1.6e-11    5.6e-10
  chunked_o*, fp32 storage        5.7e-8     5.9e-8     5.8e-8     5.8e-8
  fixedpath_o* against the dense fp64 oracle (TOL_PEN = 5e-8): 6.4e-14 / 3.3e-12 / 3.7e-9 at orders 2 / 3 / 4.
The short fixed kernels (fast_rcp) lose no digits against the long families: order 4 sits at 0.45 of its gate, order 5
at 0.04, fp32 storage at 0.2 of TOL_F32 (an earlier draw of the same cases gave 2.0e-7 at order 5: 0.65 of it).
"""
import collections
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import guarded, synth
from tests.staged import FAST_ENTRIES, Carved, arg_pointers, carve_args, check_carves, staged_buffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
VW = 0.02                       # the descriptor's vel_zero_weight of every call here
PW = 0.7                        # path_weight of the path-kernel cases
BAND = 256 * 1024
NONFINITE, NOT_SPD = 1, 2
INVALID_ARG = -1
R1, R2 = (1, 2, 17, 1, 5), (17,) * 64 + (1,)

# B = (k, c) stands for k * CUs + c trajectories; lens: the segment counts of a ragged batch (else None, uniform S);
# flags: names of descriptor flags; path: path_weight; opt: max_dev and status are passed
FastCase = collections.namedtuple("FastCase", "arm order S B bc_per vw_per opt flags f32 lens max_segments path")


def _mk(arm, order, S, B, bc_per=False, vw_per=False, opt=True, flags=(), f32=False, lens=None, max_segments=0, path=0.0):
    return FastCase(arm, order, S, B if isinstance(B, tuple) else (0, B), bool(bc_per), bool(vw_per), bool(opt), tuple(flags),
                    bool(f32), lens, max_segments, path)


def batch_of(c, cus):
    return len(c.lens) if c.lens is not None else c.B[0] * cus + c.B[1]


def case_id(c):
    shape = ("B%s%dxS%d" % ("%dcu+" % c.B[0] if c.B[0] else "", c.B[1], c.S) if c.lens is None
             else "ragged%d_max%d" % (len(c.lens), c.max_segments))
    return "-".join([c.arm, "o%d" % c.order, shape, "f32" if c.f32 else "f64", "bcper" if c.bc_per else "bcshared",
                     "vwper" if c.vw_per else "vwscalar", "opt" if c.opt else "noopt"]
                    + [f[5:].lower() for f in c.flags])


# (order, S) of every store scheme of fixed_o* (LineGeom<O, S>::OK <=> (S * 48 * O) % 128 == 0)
SCHEMES = [(2, 2), (2, 3), (2, 4), (2, 8), (2, 16), (3, 5), (3, 8), (3, 16), (5, 3), (5, 8),
           (4, 2), (4, 4), (4, 6), (4, 7), (4, 16)]
SINGLE = (0, 64 * 3 + 5)          # one slice per persistent workgroup, and a tail
SINGLE_O4 = (32, 64 * 3 + 5)      # order 4 leaves the three-lane mapping above 32 CUs
WALK = (128, 64 * 3 + 5)          # 64 * (2 CUs + 3) + 5: persistent workgroups walk several slices


def _persistent_cases():
    out = [_mk("persistent", o, S, SINGLE_O4 if o == 4 else SINGLE, opt=i % 2 == 0) for i, (o, S) in enumerate(SCHEMES)]
    out += [_mk("persistent", o, S, WALK, opt=i % 2 == 1) for i, (o, S) in enumerate(((2, 4), (3, 8), (4, 4), (5, 8)))]
    return out


_SLICE_FORMS = (dict(bc_per=True), dict(vw_per=True), dict(flags=("FLAG_NO_PERSISTENT",)), dict(bc_per=True, vw_per=True))


def _slice_cases():
    out = []
    others = [s for s in SCHEMES if s[0] != 4]
    for i, (o, S) in enumerate(others):        # i % 3 and i // 3 walk every (B, form) pair over the ten shapes
        out.append(_mk("slice", o, S, (64, 65, 64 * 3 + 63)[i % 3], opt=i % 2 == 0, **_SLICE_FORMS[(i // 3) % 4]))
    for i, (o, S) in enumerate([s for s in SCHEMES if s[0] == 4]):
        out.append(_mk("slice", o, S, (SINGLE_O4, (32, 64))[i % 2], opt=i % 2 == 1, **_SLICE_FORMS[i % 4]))
    out.append(_mk("slice", 4, 6, (32, 64), opt=True, flags=("FLAG_NO_PERSISTENT",)))
    out.append(_mk("slice", 2, 8, 64 * 3 + 63, opt=False, flags=("FLAG_NO_PERSISTENT",)))
    return out


def _tail_cases():
    out = []
    for i, (o, S) in enumerate([s for s in SCHEMES if s[0] != 4]):
        out.append(_mk("tail", o, S, (1, 63)[i % 2], bc_per=i % 4 >= 2, vw_per=i % 3 == 1, opt=i % 3 != 2,
                       flags=("FLAG_NO_PERSISTENT",) if i % 5 == 4 else ()))
    return out


def _axis3_cases():
    out = []
    Ss = (2, 4, 6, 7, 16)
    for i, B in enumerate((1, 15, 16, 17, 33, 130, 16, 17, 130, 1)):
        out.append(_mk("axis3", 4, Ss[(i + 2 * (i // 6)) % 5], B, bc_per=i % 2 == 1, vw_per=i % 3 == 2, opt=i % 4 < 2,
                       flags=("FLAG_NO_PERSISTENT",) if i == 5 else ()))
    return out


def _segmajor_cases():
    out = []
    for i, (S, B) in enumerate((S, B) for S in (2, 7, 16) for B in (1, 65, SINGLE_O4)):
        out.append(_mk("segmajor", 4, S, B, bc_per=i % 3 == 1, vw_per=i % 4 == 2, opt=i % 2 == 0,
                       flags=("FLAG_SEGMENT_MAJOR",) + (("FLAG_NO_PERSISTENT",) if i == 7 else ())))
    return out


def _path_cases():
    shapes = [(2, S) for S in (2, 4, 8, 13, 16)] + [(3, S) for S in (5, 8, 16)] + [(4, S) for S in (2, 7, 8, 16)]
    Bs = (1, 64, 64 * 3 + 29)
    out = []
    for i, (o, S) in enumerate(shapes):
        out.append(_mk("path", o, S, Bs[i % 3], bc_per=i % 2 == 0, vw_per=i % 4 >= 2, opt=(i // 3) % 2 == 0, path=PW))
    for i, (o, S) in enumerate(((2, 13), (2, 8), (3, 8), (3, 5), (4, 7), (4, 16))):   # the other batch sizes, opt the other way
        out.append(_mk("path", o, S, Bs[(i + 2) % 3] if i % 2 else 64 * 3 + 29, bc_per=i % 2 == 1, vw_per=i % 3 == 0,
                       opt=i % 2 == 1, path=PW))
    return out


def _chunked_cases():
    out, Bs, i = [], (1, 63, 65), 0
    for S in (1, 3, 4, 5, 16):                       # fp32 storage at the fixed kernels' sizes
        for o in (2, 3, 4, 5):
            out.append(_mk("chunked", o, S, Bs[i % 3], bc_per=i % 2 == 0, vw_per=i % 3 == 0, opt=(i // 2) % 2 == 0, f32=True))
            i += 1
    for o in (2, 3, 4, 5):                           # fp64: the fixed kernels need S >= 2
        out.append(_mk("chunked", o, 1, Bs[o % 3], bc_per=o % 2 == 1, vw_per=o == 4, opt=o < 4))
    for S in (17, 33, 64, 65, 256):                  # 8 .. 64 lanes per trajectory, both storage types
        for o in (2, 3, 4):
            for f32 in (False, True):
                out.append(_mk("chunked", o, S, Bs[i % 3], bc_per=(i // 2) % 2 == 0, vw_per=i % 5 == 0, opt=i % 3 != 0, f32=f32))
                i += 1
    for S, B, f32 in ((17, 63, False), (64, 1, True), (33, 65, False)):    # order 5: B << lanes stays below the span rule
        out.append(_mk("chunked", 5, S, B, bc_per=f32, opt=not f32, f32=f32))
    for k, (lens, ms) in enumerate(((R1, 17), (R1, 32), (R2, 17), (R2, 32))):
        for j, o in enumerate(((2, 5), (3, 4), (4, 3), (5, 2))[k]):
            out.append(_mk("chunked", o, 0, 0, bc_per=(k + j) % 2 == 0, vw_per=k == 1, opt=j == 0, f32=(k + j) % 2 == 1, lens=lens,
                           max_segments=ms))
    return out


CASES = (_persistent_cases() + _slice_cases() + _tail_cases() + _axis3_cases() + _segmajor_cases() + _path_cases()
         + _chunked_cases())
PARAMS = [pytest.param(c, id=case_id(c)) for c in CASES]


def arm_of(c, cus):
    """The arm `c` reaches, restated from pick_kernel / fixed_supported / launch_s."""
    B = batch_of(c, cus)
    segmaj, nopers = "FLAG_SEGMENT_MAJOR" in c.flags, "FLAG_NO_PERSISTENT" in c.flags
    fixed = not c.f32 and c.lens is None and 2 <= c.S <= (8 if c.order == 5 else 16) and 2 <= c.order <= 5
    if c.path > 0.0:
        return "path" if fixed and c.order <= 4 and not segmaj else "generic"
    if not fixed or (segmaj and c.order != 4):
        smax = c.max_segments if c.lens is not None else c.S
        span = smax > 256 or (c.order == 5 and smax > 16 and B * max(1, 2 ** int(np.ceil(np.log2(smax / 16.0)))) >= 65536)
        return "chunked" if not segmaj and not span and 1 <= smax <= 256 else "other"
    if segmaj:
        return "segmajor"
    if c.order == 4 and B <= 32 * cus:
        return "axis3"
    if B < 64:
        return "tail"
    return "slice" if (c.bc_per or c.vw_per or nopers) else "persistent"


def kernel_name_of(c):
    if c.arm == "chunked":
        smax, lanes = (c.max_segments if c.lens is not None else c.S), 1
        while 4 * lanes < smax:
            lanes *= 2
        return "chunked_o%d_%s_l%d%s" % (c.order, "f32io_f64" if c.f32 else "f64", lanes, "_ragged" if c.lens is not None else "")
    return "fixed%s_o%d_s%d_f64" % ("path" if c.arm == "path" else "", c.order, c.S)


def _lens(c, cus):
    return c.lens if c.lens is not None else (c.S,) * batch_of(c, cus)


def _flags(csp, c):
    f = 0
    for name in c.flags:
        f |= getattr(csp, name)
    return f


def _desc(csp, c, cus, seg_off_ptr=None, vw_ptr=None, mem=None):
    ragged = c.lens is not None
    return csp.make_desc(c.order, batch_of(c, cus), 0 if ragged else c.S, csp.DTYPE_F32 if c.f32 else csp.DTYPE_F64, c.path, VW,
                         csp.MEM_DEVICE if mem is None else mem, c.bc_per, seg_off_ptr, c.max_segments if ragged else 0, vw_ptr,
                         flags=_flags(csp, c))


# ------------------------------------------------------------------------------- 4. the case table, on the build machine


def test_case_table_names_its_kernels():
    """Not a GPU test: for every case above, at 256 CUs, csp_minsnap_kernel_name names the family the case claims and
    csp_minsnap_workspace_bytes is 0; the arm each case claims is the one launch_s's rules (restated in arm_of) give at
    that CU count; every value of every secondary axis occurs on every arm that admits it; ids are unique."""
    import importlib
    csp = importlib.import_module("cs-pathplan_amd")
    keep = np.zeros(70, np.int64)
    for c in CASES:
        d = _desc(csp, c, 256, keep.ctypes.data if c.lens is not None else None, keep.ctypes.data if c.vw_per else None)
        assert csp.kernel_name(d) == kernel_name_of(c), (case_id(c), csp.kernel_name(d))
        assert csp.workspace_bytes(d) == 0, case_id(c)
        for cus in (256, 304, 64):
            assert arm_of(c, cus) == c.arm, (case_id(c), cus, arm_of(c, cus))
    assert len({case_id(c) for c in CASES}) == len(CASES)
    for arm in ("persistent", "slice", "tail", "axis3", "segmajor", "path", "chunked"):
        mine = [c for c in CASES if c.arm == arm]
        assert {c.opt for c in mine} == {True, False}, arm
        if arm != "persistent":     # the persistent kernel is the shared-bc, scalar-weight form by definition
            assert {c.bc_per for c in mine} == {True, False} and {c.vw_per for c in mine} == {True, False}, arm
        if arm in ("slice", "tail", "axis3", "segmajor"):
            assert any("FLAG_NO_PERSISTENT" in c.flags for c in mine), arm
        if arm == "chunked":
            assert {c.f32 for c in mine} == {True, False} and {c.order for c in mine} == {2, 3, 4, 5}
    print("%d solve_batch cases" % len(CASES))
    for order, S, f32 in MULTI_CASES:
        d = csp.make_desc(order, 65, S, csp.DTYPE_F32 if f32 else csp.DTYPE_F64, 0.0, VW, csp.MEM_DEVICE)
        want = "chunked_o%d_f32io_f64_l2" % order if f32 else "fixed_o%d_s%d_f64" % (order, S)
        assert csp.kernel_name(d) == want and csp.workspace_bytes(d) == 0, ("multi", order, S)
    for pc in PLAN_CASES:
        d = csp.make_desc(pc.order, pc.B, pc.S, csp.DTYPE_F64, pc.path, VW, csp.MEM_DEVICE, pc.bc_per)
        assert csp.kernel_name(d).startswith(pc.kernel), (pc, csp.kernel_name(d))
        assert (csp.workspace_bytes(d) == 0) == (not pc.kernel.startswith("generic")), pc


# --------------------------------------------------------------------------------------- 1. csp_minsnap_solve_batch


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _seed(c):
    return 7000 + 13 * CASES.index(c) if c in CASES else 6000 + 17 * c.order + c.S


def _inputs(c, cus):
    lens = _lens(c, cus)
    host = staged_buffers("solve_batch", lens, c.order, c.f32, c.bc_per, _seed(c))
    vw = np.random.default_rng(_seed(c) + 1).uniform(0.0, 0.3, size=len(lens)) if c.vw_per else None
    return host, vw


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _solve_call(csp, c, cus, host, vw, fill, shift=None, expect_rc=0):
    """One device-memory csp_minsnap_solve_batch for case `c` with every pointer argument in a carve of exactly its size
    (BAND bytes of guard on either side) and the outputs starting as `fill` bytes.  Asserts the kernel name, that no
    workspace is needed, the return code, every guard band and that no input byte changed.  Returns {output: array}."""
    import torch
    sym, ws_fn, args = FAST_ENTRIES["solve_batch"]
    lib = csp.raw_lib()
    tag = (case_id(c), hex(fill), shift)
    ins, outs = carve_args(args, host, c.opt, fill, DEV, BAND, shift)
    extra = {}
    if c.lens is not None:
        extra["seg_offsets"] = Carved(_offsets(c.lens), DEV, "seg_offsets", band=BAND)
    if vw is not None:
        extra["vel_zero_weight_per_traj"] = Carved(vw, DEV, "vel_zero_weight_per_traj", band=BAND)
    desc = _desc(csp, c, cus, extra["seg_offsets"].data_ptr() if c.lens is not None else None,
                 extra["vel_zero_weight_per_traj"].data_ptr() if vw is not None else None)
    assert csp.kernel_name(desc) == kernel_name_of(c), (tag, csp.kernel_name(desc))
    assert arm_of(c, cus) == c.arm, (tag, arm_of(c, cus))
    assert int(getattr(lib, ws_fn)(ctypes.byref(desc))) == 0, tag
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = getattr(lib, sym)(ctypes.byref(desc), *arg_pointers(args, ins, outs), None, 0, stream)
    torch.cuda.synchronize()
    assert rc == expect_rc, (tag, rc, csp.strerror(rc))
    check_carves(tag, list(ins.values()) + list(outs.values()) + list(extra.values()), list(ins.values()) + list(extra.values()))
    return {n: g.numpy() for n, g in outs.items()}


def _binding(csp, c, cus, host, vw):
    """The Python binding's call for the same inputs (it allocates its own outputs)."""
    import torch
    B = batch_of(c, cus)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    kw = dict(order=c.order, path_weight=c.path, vel_zero_weight=VW, want_max_dev=True, want_status=True,
              segment_major="FLAG_SEGMENT_MAJOR" in c.flags, no_persistent="FLAG_NO_PERSISTENT" in c.flags)
    if c.lens is not None:
        wp, tm = dev(host["waypoints"]), dev(host["times"])
        kw.update(seg_offsets=dev(_offsets(c.lens)), max_segments=c.max_segments)
    else:
        wp, tm = dev(host["waypoints"].reshape(B, c.S + 1, 3)), dev(host["times"].reshape(B, c.S))
    if vw is not None:
        kw["vel_zero_weight_per_traj"] = dev(vw)
    r = csp.solve_batch(wp, tm, dev(host["bc"]), **kw)
    torch.cuda.synchronize()
    assert r.kernel == kernel_name_of(c), r.kernel
    return r


def _per_traj(c, cus, coeffs):
    """Coefficients as a list over trajectories of [S_b, 3, 2 order] arrays, whatever the layout."""
    lens, m = _lens(c, cus), 2 * c.order
    if "FLAG_SEGMENT_MAJOR" in c.flags:
        return list(coeffs.reshape(c.S, len(lens), 3, m).transpose(1, 0, 2, 3))
    off = _offsets(lens)
    flat = coeffs.reshape(-1, 3, m)
    return [flat[off[b]:off[b + 1]] for b in range(len(lens))]


@pytest.mark.gpu
@pytest.mark.parametrize("c", PARAMS)
def test_guard_bands(csp, c):
    """Contract A."""
    cus = _cus()
    host, vw = _inputs(c, cus)
    out = _solve_call(csp, c, cus, host, vw, 0x5A)
    if c.opt:
        assert not out["status"].any(), (case_id(c), np.flatnonzero(out["status"])[:8])
    r = _binding(csp, c, cus, host, vw)
    assert not r.status.cpu().numpy().any(), case_id(c)
    assert out["coeffs"].tobytes() == r.coeffs.cpu().numpy().tobytes(), (case_id(c), "differs from the binding's call")
    if c.opt:
        assert out["max_dev"].tobytes() == r.max_dev.cpu().numpy().tobytes(), (case_id(c), "max_dev differs from the binding's call")


def _assert_same_and_written(tag, a, b):
    """`a` started as 0x00 bytes, `b` as 0xFF bytes: identical bits, and no all-ones element in b."""
    for name in a:
        ab, bb = a[name].reshape(-1).view(np.uint8), b[name].reshape(-1).view(np.uint8)
        assert np.array_equal(ab, bb), (tag, name, "differs between a 0x00 and a 0xFF start",
                                        np.flatnonzero(ab != bb)[:8] // a[name].itemsize)
        ones = bb.reshape(-1, a[name].itemsize).min(axis=1) == 0xFF
        assert not ones.any(), (tag, name, "stale 0xFF elements", np.flatnonzero(ones)[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("c", PARAMS)
def test_independent_of_stale_memory(csp, c):
    """Contract B: coeffs, and max_dev / status when passed, are written everywhere on every arm."""
    cus = _cus()
    host, vw = _inputs(c, cus)
    runs = [_solve_call(csp, c, cus, host, vw, fill) for fill in (0x00, 0xFF)]
    _assert_same_and_written(case_id(c), runs[0], runs[1])
    if c.opt:
        assert not runs[1]["status"].any() and (runs[1]["max_dev"] >= 0.0).all(), case_id(c)
        if c.path == 0.0:   # the deviation metric is evaluated at t* = 0, where it vanishes
            assert not runs[1]["max_dev"].any(), case_id(c)


def _co_align(c):
    """Bytes the coefficient pointer must be a multiple of (dispatch in minsnap_capi.hip)."""
    return 8 if (c.arm == "chunked" and c.f32 and c.order % 2 == 1) else 16


@pytest.mark.gpu
@pytest.mark.parametrize("c", PARAMS)
def test_minimum_alignment(csp, c):
    """Contract C.  The fixed and path kernels require waypoints, times and coeffs on 16 bytes, the chunked kernel only
    coeffs (it reads its inputs as scalars)."""
    cus = _cus()
    host, vw = _inputs(c, cus)
    base = _solve_call(csp, c, cus, host, vw, 0xFF)
    shifted = _solve_call(csp, c, cus, host, vw, 0xFF, dict(waypoints=16, times=16, bc=16, coeffs=_co_align(c)))
    for name in base:
        assert base[name].tobytes() == shifted[name].tobytes(), (case_id(c), name, "differs at the minimum alignment")
    strict = ("coeffs",) if c.arm == "chunked" else ("waypoints", "times", "coeffs")
    for name in strict:
        step = _co_align(c) // 2 if name == "coeffs" else 8
        out = _solve_call(csp, c, cus, host, vw, 0x5A, {name: step}, expect_rc=INVALID_ARG)
        for n, a in out.items():
            assert (a.reshape(-1).view(np.uint8) == 0x5A).all(), (case_id(c), name, n, "written by a rejected call")


def _ld_reference(c, cus, host, vw):
    from tests.test_gpu_edges import _ld
    lens = _lens(c, cus)
    B, f8 = len(lens), lambda a: np.asarray(a, dtype=np.float64)
    if c.lens is None:
        return list(_ld(c.order, f8(host["waypoints"]).reshape(B, c.S + 1, 3), f8(host["times"]).reshape(B, c.S), f8(host["bc"]),
                        vw=VW, vw_per=vw).reshape(B, c.S, 3, 2 * c.order))
    off, ref = _offsets(lens), []
    for b, n in enumerate(lens):
        bc = f8(host["bc"])[b if c.bc_per else 0][None]
        ref.append(_ld(c.order, f8(host["waypoints"])[off[b] + b:off[b + 1] + b + 1][None], f8(host["times"])[off[b]:off[b + 1]][None],
                       bc, vw=VW, vw_per=None if vw is None else vw[b:b + 1]).reshape(n, 3, 2 * c.order))
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("c", PARAMS)
def test_precision(csp, oracle_mod, c):
    """Contract D.  Unpenalised: every trajectory against the long-double structured solver, per power, at TOL_LD[order]
    (fp64) / TOL_F32 (fp32 storage; the reference gets the fp32-rounded inputs).  Path penalty: the dense fp64 oracle at
    TOL_PEN, max_dev at 1e-7 relative to max(1, max_dev) (tests/test_gpu_parity.py::test_path_penalty_register_kernel);
    whole batches with the scalar weight, trajectories 0, 63, 64, B // 2 and B - 1 with per-trajectory weights."""
    from tests.test_gpu_edges import TOL_F32, TOL_LD, _gates
    from tests.test_gpu_parity import TOL_PEN
    cus = _cus()
    host, vw = _inputs(c, cus)
    out = _solve_call(csp, c, cus, host, vw, 0xFF)
    got = _per_traj(c, cus, out["coeffs"].astype(np.float64))
    B = batch_of(c, cus)
    if c.path == 0.0:
        ref = _ld_reference(c, cus, host, vw)
        tol = TOL_F32 if c.f32 else TOL_LD[c.order]
        if c.lens is None:
            pp, _ = _gates(np.stack(got), np.stack(ref), tol, ("fast vs long double", case_id(c)))
        else:
            pp = max(_gates(g, r, tol, ("fast vs long double", case_id(c), b))[0] for b, (g, r) in enumerate(zip(got, ref)))
        print("LDGATE %s o%d %s per-power %.3e tol %.1e" % (c.arm, c.order, "f32" if c.f32 else "f64", pp, tol))
        return
    wp, tm, bc = host["waypoints"].reshape(B, c.S + 1, 3), host["times"].reshape(B, c.S), host["bc"]
    if vw is None:
        ref, ref_md = oracle_mod.solve_batch(c.order, wp, tm, bc, path_weight=c.path, vel_zero_weight=VW, nthreads=min(16, oracle_mod.max_threads()))
        idx = list(range(B))
    else:
        idx = sorted({0, min(63, B - 1), min(64, B - 1), B // 2, B - 1})
        pairs = [oracle_mod.solve(c.order, wp[b], bc[b if c.bc_per else 0, [0, 1]], bc[b if c.bc_per else 0, [2, 3]], tm[b], c.path, float(vw[b]))
                 for b in idx]
        ref, ref_md = np.stack([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    pp, _ = synth.parity_gate(np.stack([got[b] for b in idx]), ref, TOL_PEN, ("path kernel vs oracle", case_id(c)))
    print("PENGATE o%d per-power %.3e" % (c.order, pp))
    if c.opt:
        md = out["max_dev"][idx]
        assert np.max(np.abs(md - ref_md)) < 1e-7 * max(1.0, float(np.max(ref_md))), (case_id(c), md[:4], ref_md[:4])


# ------------------------------------------------------------------------------------------- E. forced store flavours

# persistent-kernel cases of contract A by store policy: CSP_STORE_POLICY=nt -- every order, one ring (order 4: paired)
# shape and one record-at-a-time shape; =wt -- the write-through shapes; CSP_NT_STORES=1 alone -- orders 2, 3, 5
FLAVOURS = (("nt", dict(CSP_STORE_POLICY="nt"), ((2, 3), (2, 8), (3, 5), (3, 16), (5, 3), (5, 8), (4, 7), (4, 16))),
            ("wt", dict(CSP_STORE_POLICY="wt"), ((4, 4), (4, 6), (4, 16))),
            ("ntstores", dict(CSP_NT_STORES="1"), ((2, 3), (2, 8), (3, 5), (3, 16), (5, 3), (5, 8))))


def _flavour_case(order, S):
    return next(c for c in CASES if c.arm == "persistent" and (c.order, c.S) == (order, S) and c.B[0] in (0, 32))


def _flavour_run(csp, shapes):
    """Contract A's guarded call of the persistent cases of `shapes`, status included: {"o<order>s<S>": coefficients}."""
    cus, out = _cus(), {}
    for order, S in shapes:
        c = _flavour_case(order, S)._replace(opt=True)
        host, vw = _inputs(c, cus)
        r = _solve_call(csp, c, cus, host, vw, 0x5A)
        assert not r["status"].any(), case_id(c)
        out["o%ds%d" % (order, S)] = r["coeffs"]
    return out


@pytest.mark.gpu
def test_forced_store_flavours(csp, tmp_path):
    """Contract E.  The library reads CSP_STORE_POLICY and CSP_NT_STORES once per process, and the non-temporal and
    write-through instantiations otherwise run only above 256 MiB / 32 MiB of coefficients: each setting runs the guarded
    persistent-kernel calls in a child process of its own (one after another; the child checks its guard bands), and the
    coefficients it saves are bit-equal with this process's."""
    assert not os.environ.get("CSP_STORE_POLICY") and not os.environ.get("CSP_NT_STORES")
    here = _flavour_run(csp, sorted({s for _, _, shapes in FLAVOURS for s in shapes}))
    for name, env, shapes in FLAVOURS:
        path = str(tmp_path / (name + ".npz"))
        p = subprocess.run([sys.executable, "-m", "tests.test_gpu_bounds_fast", path] + ["%d,%d" % s for s in shapes],
                           env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (name, p.returncode, p.stdout[-2000:], p.stderr[-3000:])
        there = np.load(path)
        for order, S in shapes:
            key = "o%ds%d" % (order, S)
            assert there[key].tobytes() == here[key].tobytes(), (name, key, "differs from the default store flavour")


# ------------------------------------------------------------------------------------------------------- F. bad lanes

BAD_CASES = [
    _mk("persistent", 2, 8, SINGLE), _mk("persistent", 4, 6, SINGLE_O4), _mk("persistent", 3, 5, WALK),
    _mk("slice", 3, 8, 64 * 3 + 63, bc_per=True, vw_per=True), _mk("slice", 4, 7, SINGLE_O4, bc_per=True),
    _mk("slice", 5, 8, 65, flags=("FLAG_NO_PERSISTENT",)),
    _mk("tail", 5, 3, 63, bc_per=True), _mk("tail", 2, 4, 63),
    _mk("axis3", 4, 16, 130, bc_per=True), _mk("axis3", 4, 6, 33, bc_per=True, vw_per=True), _mk("axis3", 4, 7, 130),
    _mk("segmajor", 4, 7, SINGLE_O4, bc_per=True, flags=("FLAG_SEGMENT_MAJOR",)),
    _mk("path", 2, 13, 64 * 3 + 29, bc_per=True, path=PW), _mk("path", 3, 8, 64 * 3 + 29, bc_per=True, vw_per=True, path=PW),
    _mk("path", 4, 7, 64 * 3 + 29, path=PW),
    _mk("chunked", 4, 33, 65, bc_per=True), _mk("chunked", 3, 5, 65, bc_per=True, f32=True),
    _mk("chunked", 5, 17, 63, vw_per=True), _mk("chunked", 2, 0, 0, bc_per=True, lens=R2, max_segments=32),
]


def _poison(c, cus, host):
    """A copy of `host` with one bad value in each of a handful of trajectories; returns (bad host, {trajectory: kind}).
    Trajectories: the first and the last of the batch, the last of the first slice and the first of the second (slices of
    64; for the three-lane kernel also of 16), the first of the tail slice, one in the middle.  Segments: the first, a
    middle one and the last (for the chunked kernel: in a trajectory's first and last chunk)."""
    lens = _lens(c, cus)
    B, off = len(lens), _offsets(lens)
    bad = {k: v.copy() for k, v in host.items()}
    tm, wp, bc = bad["times"].reshape(-1), bad["waypoints"].reshape(-1, 3), bad["bc"]
    seg = lambda b, where: int(off[b]) + {"first": 0, "middle": lens[b] // 2, "last": lens[b] - 1}[where]
    plan = [(0, "zero_time", "first"), (63, "nan_time", "middle"), (64, "neg_time", "last"), (B - 1, "nan_wp", "middle"),
            (B // 64 * 64, "inf_wp", "last"), (B // 2 + 1, "nan_bc", None), (15, "inf_wp", "first"), (16, "zero_time", "last"),
            (B - 2, "nan_time", "first"), (17, "neg_time", "first"), (B // 2 + 2, "nan_wp", "last"), (62, "nan_bc", None)]
    kinds = {}
    for b, kind, where in plan:
        if not 0 <= b < B or b in kinds or (kind == "nan_bc" and not c.bc_per):
            continue
        if kind == "neg_time" and lens[b] == 1:
            kind = "nan_time"          # one segment: no free derivative, hence no pivot that a negative time could spoil
        kinds[b] = kind
        if kind == "nan_bc":
            bc[b, 1, 1] = np.nan      # end velocity, y: used at every order
        elif kind.endswith("time"):
            tm[seg(b, where)] = {"zero_time": 0.0, "nan_time": np.nan, "neg_time": -0.3}[kind]
        else:                          # one axis only: the three-lane mapping keeps two healthy sibling lanes
            wp[seg(b, where) + b + (1 if where == "last" else 0), 1 if kind == "nan_wp" else 2] = np.nan if kind == "nan_wp" else np.inf
    return bad, kinds


@pytest.mark.gpu
@pytest.mark.parametrize("c", [pytest.param(c, id=case_id(c)) for c in BAD_CASES])
def test_bad_lanes_bit_exact(csp, c):
    """Contract F (loop bounds: module docstring).  status is non-zero on exactly the poisoned trajectories, with
    CSP_TRAJ_NONFINITE for a zero time (1 / T = inf) and for every NaN / inf input, CSP_TRAJ_NOT_SPD for a negative time
    in a trajectory of two or more segments (a one-segment trajectory has no free derivative, so no pivot: the chunked
    kernel returns finite coefficients and status 0 there, and the ragged case puts a NaN time into it instead).  Every
    other trajectory's coefficients, status
    and max_dev are bit-equal with a run over benign data: the LDS carry exchange between the roles, the chunked kernel's
    lanes of one trajectory and the path kernel's t* pick leak nothing, finite or not."""
    cus = _cus()
    assert arm_of(c, cus) == c.arm
    host, vw = _inputs(c, cus)
    bad, kinds = _poison(c, cus, host)
    out_bad = _solve_call(csp, c, cus, bad, vw, 0xFF)
    out_good = _solve_call(csp, c, cus, host, vw, 0xFF)
    B, st = batch_of(c, cus), out_bad["status"]
    print(case_id(c), "status of the bad trajectories", {b: (k, int(st[b])) for b, k in sorted(kinds.items())})
    assert not out_good["status"].any(), case_id(c)
    others = np.setdiff1d(np.arange(B), list(kinds))
    assert not st[others].any(), (case_id(c), "a healthy trajectory was flagged", others[np.flatnonzero(st[others])][:8])
    for b, kind in kinds.items():
        assert st[b] != 0, (case_id(c), b, kind, "not flagged")
        assert st[b] & (NOT_SPD if kind == "neg_time" else NONFINITE), (case_id(c), b, kind, int(st[b]))
    cb, cg = _per_traj(c, cus, out_bad["coeffs"]), _per_traj(c, cus, out_good["coeffs"])
    leaked = [int(b) for b in others if cb[b].tobytes() != cg[b].tobytes()]
    assert not leaked, (case_id(c), "a bad trajectory disturbed the coefficients of", leaked[:8])
    assert out_bad["max_dev"][others].tobytes() == out_good["max_dev"][others].tobytes(), case_id(c)


# --------------------------------------------------------------------------------------- 2. csp_minsnap_solve_multi

MULTI_SIZES = [1, 63, 64, 65, 0, 130] + [1] * 29       # 34 non-empty batches: the 32-entry table twice
MULTI_CASES = [(4, 6, False), (2, 4, False), (3, 5, False), (3, 5, True)]   # (order, S, fp32): the last is not a table shape


def _multi_call(csp, order, S, f32, hosts, fill, shift=None, expect_rc=0, bc_per=False):
    """csp_minsnap_solve_multi with every batch's four buffers and its status array in carves of their own."""
    import torch
    args = tuple(a for a in FAST_ENTRIES["solve_batch"][2] if a[0] != "max_dev")
    n = len(hosts)
    carved = [carve_args(args, h, True, fill, DEV, BAND, shift) if h is not None else None for h in hosts]
    col = lambda name: (ctypes.c_void_p * n)(*[(dict(cv[0], **cv[1])[name].data_ptr() if cv else None) for cv in carved])
    sizes = (ctypes.c_int64 * n)(*[0 if h is None else len(h["status"]) for h in hosts])
    desc = csp.make_desc(order, 0, S, csp.DTYPE_F32 if f32 else csp.DTYPE_F64, 0.0, VW, csp.MEM_DEVICE, bc_per)
    cols = [col(k) for k in ("waypoints", "times", "bc", "coeffs", "status")]
    rc = csp.raw_lib().csp_minsnap_solve_multi(ctypes.byref(desc), n, ctypes.cast(sizes, ctypes.c_void_p),
                                               *[ctypes.cast(x, ctypes.c_void_p) for x in cols],
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == expect_rc, (order, S, f32, rc, csp.strerror(rc))
    res = []
    for k, cv in enumerate(carved):
        if cv is None:
            res.append(None)
            continue
        check_carves(("multi", order, S, f32, "batch", k), list(cv[0].values()) + list(cv[1].values()), list(cv[0].values()))
        res.append({name: g.numpy() for name, g in cv[1].items()})
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("order,S,f32", MULTI_CASES, ids=lambda v: str(v))
def test_multi_batches(csp, order, S, f32):
    """Batches of 1, 63, 64, 65, 0 and 130 trajectories plus 29 of one (34 non-empty: two tables), shared bc per batch.
    A: bands, inputs, status 0 and bit-equality with csp_minsnap_solve_batch per batch; B: 0x00 / 0xFF starts; C: every
    waypoints / times / bc / coeffs pointer 16 bytes past a 256-byte boundary, then 8 bytes (rejected, nothing written).
    fp32 S = 5 is no table shape: one chunked launch per batch, whose odd order takes coefficients on 8 bytes."""
    import torch
    hosts = [staged_buffers("solve_batch", (S,) * B, order, f32, False, 8000 + 41 * k + order) if B else None
             for k, B in enumerate(MULTI_SIZES)]
    a = _multi_call(csp, order, S, f32, hosts, 0x5A)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    for k, (h, r) in enumerate(zip(hosts, a)):
        if h is None:
            continue
        B = len(h["status"])
        assert not r["status"].any(), (k, r["status"])
        one = csp.solve_batch(dev(h["waypoints"].reshape(B, S + 1, 3)), dev(h["times"].reshape(B, S)), dev(h["bc"]), order=order,
                              vel_zero_weight=VW, want_status=True)
        assert one.kernel == ("chunked_o%d_f32io_f64_l2" % order if f32 else "fixed_o%d_s%d_f64" % (order, S)), one.kernel
        assert r["coeffs"].tobytes() == one.coeffs.cpu().numpy().tobytes(), ("multi differs from solve_batch", k, B)
    z, f = _multi_call(csp, order, S, f32, hosts, 0x00), _multi_call(csp, order, S, f32, hosts, 0xFF)
    co = 8 if f32 and order % 2 else 16
    s = _multi_call(csp, order, S, f32, hosts, 0xFF, dict(waypoints=16, times=16, bc=16, coeffs=co))
    for k, h in enumerate(hosts):
        if h is None:
            continue
        _assert_same_and_written(("multi", order, S, f32, k), z[k], f[k])
        for name in f[k]:
            assert f[k][name].tobytes() == a[k][name].tobytes() == s[k][name].tobytes(), (k, name)
    for name in ("coeffs",) if f32 else ("waypoints", "times", "coeffs"):
        rej = _multi_call(csp, order, S, f32, hosts, 0x5A, {name: co // 2 if name == "coeffs" else 8}, expect_rc=INVALID_ARG)
        for k, r in enumerate(rej):   # the first table (the first batch's launch, fp32) is rejected before anything is launched
            assert r is None or all((x.reshape(-1).view(np.uint8) == 0x5A).all() for x in r.values()), (name, k)


# ------------------------------------------------------------------- 3. time allocation, plan, sample, generate

V_AVG, MIN_TIME = 5.0, 0.1       # the plan / generate calls (tests/test_gpu_plan_sample.py)

# pointer and scalar arguments between the descriptor and the workspace / stream, in the C signature's order
_ARGLIST = {
    "time_alloc_batch": lambda p, s: [p["waypoints"], s["v_avg"], s["min_time_s"], p["times"]],
    "plan_batch": lambda p, s: [p["waypoints"], s["v_avg"], s["min_time_s"], p["bc"], p["times"], p["coeffs"], p["max_dev"],
                                p["vel_zero_weight_out"], p["iterations"], p["status"]],
    "sample_batch": lambda p, s: [p["times"], p["coeffs"], s["sample_distance"], s["capacity"], p["samples"], p["counts"], p["stats"]],
    "generate_batch": lambda p, s: [p["waypoints"], s["v_avg"], s["min_time_s"], p["bc"], s["sample_distance"], s["capacity"],
                                    p["samples"], p["counts"], p["stats"], p["times"], p["coeffs"], p["max_dev"],
                                    p["vel_zero_weight_out"], p["iterations"], p["status"]],
}


def _chain_call(csp, entry, make_desc, host, opt, fill, scalars, lens=None, vw=None, alias_vw=False):
    """One device-memory call of a FAST_ENTRIES entry other than the solve: every pointer argument in a carve of exactly
    its size, the workspace (where the entry has one) at exactly its *_workspace_bytes, outputs and workspace starting as
    `fill` bytes.  make_desc(seg_offsets pointer, weights pointer) builds the descriptor.  alias_vw: vel_zero_weight_out
    IS desc->vel_zero_weight_per_traj (it starts as `vw`).  Checks the return code, the bands and the inputs."""
    import torch
    sym, ws_fn, args = FAST_ENTRIES[entry]
    lib = csp.raw_lib()
    ins, outs = carve_args(args, host, opt, fill, DEV, BAND)
    extra = {}
    if lens is not None:
        extra["seg_offsets"] = Carved(_offsets(lens), DEV, "seg_offsets", band=BAND)
    vw_ptr = None
    if alias_vw:
        vw_ptr = outs["vel_zero_weight_out"].put(vw).data_ptr()
    elif vw is not None:
        extra["vel_zero_weight_per_traj"] = Carved(vw, DEV, "vel_zero_weight_per_traj", band=BAND)
        vw_ptr = extra["vel_zero_weight_per_traj"].data_ptr()
    desc = make_desc(extra["seg_offsets"].data_ptr() if lens is not None else None, vw_ptr)
    ptrs = {n: None for n, _, _ in args}
    ptrs.update({n: g.data_ptr() for n, g in list(ins.items()) + list(outs.items())})
    call = [ctypes.byref(desc)] + _ARGLIST[entry](ptrs, scalars)
    carves = list(ins.values()) + list(outs.values()) + list(extra.values())
    need = 0
    if ws_fn is not None:
        need = int(getattr(lib, ws_fn)(ctypes.byref(desc)))
        ws = guarded.Guarded(need, DEV, BAND, name="workspace").fill(fill)
        call += [ws.data_ptr(), need]
        carves.append(ws)
    rc = getattr(lib, sym)(*call, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    tag = (entry, hex(fill), "workspace %d bytes" % need)
    assert rc == 0, (tag, rc, csp.strerror(rc))
    check_carves(tag, carves, list(ins.values()) + list(extra.values()))
    return {n: g.numpy() for n, g in outs.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_time_alloc(csp, ragged, f32):
    """csp_minsnap_time_alloc_batch, uniform (B = 65, S = 7) and ragged (1, 2, 17, 1, 5): bands and inputs, 0x00 / 0xFF
    starts, and the values exactly those of the header's formula T_i = max(|p_{i+1} - p_i| / V_avg, min_time_s) evaluated in
    numpy at the storage type (min_time_s = 1.0 against steps of ~1.7 / 1.3: both branches of the max occur)."""
    lens = R1 if ragged else (7,) * 65
    io = np.float32 if f32 else np.float64
    host = staged_buffers("solve_batch", lens, 3, f32, False, 9100 + ragged)
    scal = dict(v_avg=1.3, min_time_s=1.0)
    mk = lambda so, vwp: csp.make_desc(1, len(lens), 0 if ragged else lens[0], csp.DTYPE_F32 if f32 else csp.DTYPE_F64, 0.0, 0.0,
                                       csp.MEM_DEVICE, False, so, 1 if ragged else 0)
    runs = [_chain_call(csp, "time_alloc_batch", mk, host, True, fill, scal, lens if ragged else None) for fill in (0x5A, 0x00, 0xFF)]
    _assert_same_and_written(("time_alloc", ragged, f32), runs[1], runs[2])
    assert runs[0]["times"].tobytes() == runs[2]["times"].tobytes()
    off, wp = _offsets(lens), host["waypoints"]
    want = np.empty(int(off[-1]), io)
    for b in range(len(lens)):
        p = wp[off[b] + b:off[b + 1] + b + 1]
        d = p[1:] - p[:-1]
        want[off[b]:off[b + 1]] = np.maximum(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) / io(1.3), io(1.0))
    got = runs[0]["times"]
    assert want.dtype == got.dtype and (want == io(1.0)).any() and (want > io(1.0)).any()
    diff = np.flatnonzero(got != want)
    print("time_alloc %s %s: %d of %d differ from numpy, largest %.3e relative" % (
        "ragged" if ragged else "uniform", io.__name__, diff.size, got.size,
        float(np.max(np.abs(got.astype(np.float64) - want) / want)) if diff.size else 0.0))
    assert diff.size == 0, (diff[:8], got[diff[:8]], want[diff[:8]])


PlanCase = collections.namedtuple("PlanCase", "order S B path bc_per kernel")
PLAN_CASES = [PlanCase(4, 8, 64 * 3 + 17, 0.0, False, "fixed_o4_s8"), PlanCase(3, 20, 65, 0.0, True, "chunked_o3_f64_l8"),
              PlanCase(3, 8, 64 * 3 + 17, 0.3, True, "fixedpath_o3_s8"), PlanCase(4, 20, 65, 0.3, True, "generic_o4_f64")]
_PLAN_OPT = ("max_dev", "vel_zero_weight_out", "iterations", "status")


def _plan_inputs(pc, io=np.float64):
    """Waypoints and bc after part (b) of test_path_kernel_whole_line_stores_and_the_skip_mask: slice 0 and every other
    trajectory of slice 1 fly nearly straight at V_avg (deviation below 0.2: no re-solve), the others wiggle."""
    rng = np.random.default_rng(9200 + pc.order * 17 + pc.S)
    B, S = pc.B, pc.S
    wig, _ = synth.make_batch(B, S, config_id=26)
    t = np.linspace(0.0, 1.0, S + 1)[None, :, None]
    span = rng.uniform(20, 60, size=(B, 1, 3))
    straight = rng.uniform(-50, 50, size=(B, 1, 3)) + t * span + rng.normal(scale=0.02, size=(B, S + 1, 3))
    vdir = V_AVG * span[:, 0, :] / np.linalg.norm(span[:, 0, :], axis=1, keepdims=True)
    wp, bc = wig * 4.0, np.zeros((B, 4, 3))
    sel = np.zeros(B, dtype=bool)
    sel[:64] = True
    sel[64:128:2] = True
    wp[sel] = straight[sel]
    bc[sel, 0] = vdir[sel]
    bc[sel, 1] = vdir[sel]
    if not pc.bc_per:
        bc = np.zeros((1, 4, 3))
    m = 2 * pc.order
    return dict(waypoints=wp.reshape(-1, 3).astype(io), bc=bc.astype(io), times=np.zeros(B * S, io), coeffs=np.zeros((B * S, 3, m), io),
                max_dev=np.zeros(B), vel_zero_weight_out=np.zeros(B), iterations=np.zeros(B, np.int32), status=np.zeros(B, np.int32))


def _plan_desc(csp, pc):
    return lambda so, vwp: csp.make_desc(pc.order, pc.B, pc.S, csp.DTYPE_F64, pc.path, VW, csp.MEM_DEVICE, pc.bc_per, None, 0, vwp)


_PLAN_SCAL = dict(v_avg=V_AVG, min_time_s=MIN_TIME)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [True, False], ids=["opt", "noopt"])
@pytest.mark.parametrize("pc", PLAN_CASES, ids=lambda pc: "%s-B%d" % (pc.kernel, pc.B))
def test_plan(csp, pc, opt):
    """csp_minsnap_plan_batch with the workspace carved at exactly csp_minsnap_plan_workspace_bytes, with max_dev,
    vel_zero_weight_out, iterations and status passed and left out (the loop state then lives in the workspace).
    A: bands, inputs, times and coefficients bit-equal with the binding's call; B: 0x00 / 0xFF starts of outputs and
    workspace.  The fixed-path shape has trajectories that loop and trajectories that do not."""
    import torch
    host = _plan_inputs(pc)
    d = _plan_desc(csp, pc)(None, None)
    assert csp.kernel_name(d).startswith(pc.kernel), csp.kernel_name(d)
    runs = [_chain_call(csp, "plan_batch", _plan_desc(csp, pc), host, opt, fill, _PLAN_SCAL) for fill in (0x5A, 0x00, 0xFF)]
    _assert_same_and_written(("plan", pc, opt), runs[1], runs[2])
    for name in runs[0]:
        assert runs[0][name].tobytes() == runs[2][name].tobytes(), (pc, name)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    r = csp.plan_batch(dev(host["waypoints"].reshape(pc.B, pc.S + 1, 3)), V_AVG, MIN_TIME, bc=dev(host["bc"]), order=pc.order,
                       path_weight=pc.path, vel_zero_weight=VW)
    torch.cuda.synchronize()
    assert runs[0]["times"].tobytes() == r.times.cpu().numpy().tobytes(), pc
    assert runs[0]["coeffs"].tobytes() == r.coeffs.cpu().numpy().tobytes(), (pc, "differs from the binding's call")
    if opt:
        for name, t in (("max_dev", r.max_dev), ("vel_zero_weight_out", r.vel_zero_weight), ("iterations", r.iterations), ("status", r.status)):
            assert runs[0][name].tobytes() == t.cpu().numpy().tobytes(), (pc, name)
        assert not runs[0]["status"].any(), pc
        it = runs[0]["iterations"]
        if pc.path > 0.0 and pc.kernel.startswith("fixedpath"):
            assert (it > 0).any() and (it[:64] == 0).all(), it
        if pc.path == 0.0:
            assert not it.any() and (runs[0]["vel_zero_weight_out"] == VW).all() and not runs[0]["max_dev"].any()


@pytest.mark.gpu
def test_plan_updates_the_weights_in_place(csp):
    """vel_zero_weight_out may alias desc->vel_zero_weight_per_traj (include/csp_minsnap.h): on the fixed-path shape, every
    output is bit-equal with the run whose weights are a separate input array."""
    pc = PLAN_CASES[2]
    host = _plan_inputs(pc)
    vw = np.random.default_rng(9300).uniform(0.0, 0.05, size=pc.B)
    apart = _chain_call(csp, "plan_batch", _plan_desc(csp, pc), host, True, 0xFF, _PLAN_SCAL, vw=vw)
    alias = _chain_call(csp, "plan_batch", _plan_desc(csp, pc), host, True, 0xFF, _PLAN_SCAL, vw=vw, alias_vw=True)
    assert (apart["iterations"] > 0).any() and (apart["vel_zero_weight_out"] >= vw).all()
    for name in apart:
        assert apart[name].tobytes() == alias[name].tobytes(), name


# (sampler, descriptor flag, S): the segment sampler at 1, 7 and 64 segments and, beyond 64, the sampler the entry picks
SAMPLE_CASES = [(smp, S) for smp in ("default", "one_lane", "wave") for S in (1, 7, 64)] + [("default", 65)]
_SAMPLER_FLAG = {"default": None, "one_lane": "FLAG_FORCE_GENERIC", "wave": "FLAG_LONG_SEGMENTS"}
_PLANNED = {}


def _planned(csp, order, S, B=65):
    """Times and coefficients of a plan of B trajectories, as host arrays (computed once per shape)."""
    import torch
    if (order, S) not in _PLANNED:
        wp, _ = synth.make_batch(B, S, config_id=24)
        wp = wp * 3.0
        plan = csp.plan_batch(torch.from_numpy(wp).to(DEV), V_AVG, MIN_TIME, order=order)
        torch.cuda.synchronize()
        _PLANNED[(order, S)] = (wp, plan.times.cpu().numpy().reshape(-1), plan.coeffs.cpu().numpy().reshape(B * S, 3, 2 * order))
    return _PLANNED[(order, S)]


def _check_samples(tag, runs, capacity):
    """runs: the outputs of the same sampling call over 0x5A, 0x00 and 0xFF starts.  counts, stats and every trajectory's
    first min(counts, capacity) rows are bit-equal and hold no all-ones element; the rows beyond keep their fill."""
    a, z, f = runs
    counts = f["counts"]
    assert (counts >= 2).all(), (tag, counts)
    for name in ("counts", "stats"):
        if name in f:
            _assert_same_and_written((tag, name), {name: z[name]}, {name: f[name]})
            assert a[name].tobytes() == f[name].tobytes(), (tag, name)
    item = f["samples"].itemsize
    for b, n in enumerate(np.minimum(counts, capacity)):
        rows = [r["samples"][b].reshape(capacity, 3) for r in (a, z, f)]
        assert rows[0][:n].tobytes() == rows[1][:n].tobytes() == rows[2][:n].tobytes(), (tag, b, "rows in use differ between fills")
        assert not (rows[2][:n].reshape(-1).view(np.uint8).reshape(-1, item).min(axis=1) == 0xFF).any(), (tag, b, "stale element")
        for r, fill in zip(rows, (0x5A, 0x00, 0xFF)):
            assert (r[n:].reshape(-1).view(np.uint8) == fill).all(), (tag, b, "a row beyond the count was written", hex(fill))


@pytest.mark.gpu
@pytest.mark.parametrize("overflow", [False, True], ids=["fits", "overflows"])
@pytest.mark.parametrize("sampler,S", SAMPLE_CASES)
def test_sample(csp, sampler, S, overflow):
    """csp_minsnap_sample_batch, B = 65, `samples` carved at exactly `capacity` rows: a capacity that fits
    (csp_minsnap_sample_capacity, sample_distance 1.0) and one that every trajectory overflows (sample_distance 1e-9,
    capacity 5); stats passed, and left out for S = 7 when it overflows and for S = 64 when it fits.  Contracts A and B; the rows in
    use equal the binding's; rows beyond min(counts, capacity) are left as they were (include/csp_minsnap.h)."""
    import torch
    order, B = {1: 3, 7: 4, 64: 3, 65: 4}[S], 65
    wp, tm, co = _planned(csp, order, S)
    capacity = 5 if overflow else csp.sample_capacity(wp, V_AVG, MIN_TIME, order=order)
    sd = 1e-9 if overflow else 1.0
    with_stats = not ((overflow and S == 7) or (not overflow and S == 64))
    host = dict(times=tm, coeffs=co, samples=np.zeros((B, capacity, 3)), counts=np.zeros(B, np.int32), stats=np.zeros((B, 2)))
    flag = getattr(csp, _SAMPLER_FLAG[sampler]) if _SAMPLER_FLAG[sampler] else 0
    mk = lambda so, vwp: csp.make_desc(order, B, S, csp.DTYPE_F64, 0.0, 0.0, csp.MEM_DEVICE, flags=flag)
    scal = dict(sample_distance=sd, capacity=capacity)
    runs = [_chain_call(csp, "sample_batch", mk, host, with_stats, fill, scal) for fill in (0x5A, 0x00, 0xFF)]
    tag = ("sample", sampler, S, capacity)
    _check_samples(tag, runs, capacity)
    counts = runs[0]["counts"]
    assert (counts > capacity).all() if overflow else (counts <= capacity).all(), (tag, counts)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    ref = csp.sample_batch(dev(tm.reshape(B, S)), dev(co.reshape(B, S, 3, 2 * order)), sd, capacity, one_lane=sampler == "one_lane",
                           long_segments=sampler == "wave")
    torch.cuda.synchronize()
    assert counts.tobytes() == ref[1].cpu().numpy().tobytes(), tag
    rs = ref[0].cpu().numpy()
    for b, n in enumerate(np.minimum(counts, capacity)):
        assert runs[0]["samples"][b, :n].tobytes() == rs[b, :n].tobytes(), (tag, b)
    if with_stats:
        assert runs[0]["stats"].tobytes() == ref[2].cpu().numpy().tobytes(), tag


@pytest.mark.gpu
@pytest.mark.parametrize("pc", [PLAN_CASES[0], PLAN_CASES[2]], ids=lambda pc: pc.kernel)
def test_generate(csp, pc):
    """csp_minsnap_generate_batch on one unpenalised and one penalised plan shape, workspace at its exact size, `samples`
    at exactly `capacity` rows: contracts A and B, and every output bit-equal with csp_minsnap_plan_batch followed by
    csp_minsnap_sample_batch, as the header promises."""
    host = _plan_inputs(pc)
    B, S = pc.B, pc.S
    capacity = csp.sample_capacity(host["waypoints"].reshape(B, S + 1, 3), V_AVG, MIN_TIME, order=pc.order)
    host.update(samples=np.zeros((B, capacity, 3)), counts=np.zeros(B, np.int32), stats=np.zeros((B, 2)))
    scal = dict(_PLAN_SCAL, sample_distance=1.0, capacity=capacity)
    runs = [_chain_call(csp, "generate_batch", _plan_desc(csp, pc), host, True, fill, scal) for fill in (0x5A, 0x00, 0xFF)]
    _check_samples(("generate", pc), runs, capacity)
    plan_names = ("times", "coeffs") + _PLAN_OPT
    _assert_same_and_written(("generate", pc), {n: runs[1][n] for n in plan_names}, {n: runs[2][n] for n in plan_names})
    assert (runs[0]["counts"] <= capacity).all()
    plan = _chain_call(csp, "plan_batch", _plan_desc(csp, pc), host, True, 0x5A, _PLAN_SCAL)
    smp_host = dict(host, times=plan["times"], coeffs=plan["coeffs"])
    mk = lambda so, vwp: csp.make_desc(pc.order, B, S, csp.DTYPE_F64, 0.0, 0.0, csp.MEM_DEVICE)
    smp = _chain_call(csp, "sample_batch", mk, smp_host, True, 0x5A, dict(sample_distance=1.0, capacity=capacity))
    for name in plan_names:
        assert runs[0][name].tobytes() == plan[name].tobytes(), (pc, name, "generate differs from plan")
    for name in ("samples", "counts", "stats"):
        assert runs[0][name].tobytes() == smp[name].tobytes(), (pc, name, "generate differs from plan + sample")


if __name__ == "__main__":
    # child process of test_forced_store_flavours: argv = [output .npz, "order,S", ...]
    import importlib
    sys.path.insert(0, ROOT)
    np.savez(sys.argv[1], **_flavour_run(importlib.import_module("cs-pathplan_amd"),
                                         [tuple(int(x) for x in a.split(",")) for a in sys.argv[2:]]))
