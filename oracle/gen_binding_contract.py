"""Generates tests/golden/binding_contract.json -- TEST INFRASTRUCTURE.
    python oracle/gen_binding_contract.py            (host table; no device needed)
    python oracle/gen_binding_contract.py --device   (device table; needs an MI355X)

What the Python binding (cs-pathplan_amd/__init__.py) hands to the C-ABI, recorded by a stand-in for the module's `_lib`
(the binding looks `_lib` up at call time, so the stand-in needs no hook in the product).  Per case -- one call of a public
function, or the construction and one run() of a Prepared* object -- a row holds

  calls   every call made through `_lib`: the symbol; the descriptor / parameter block as field values (pointer fields as
          null / non-null; descriptor fields at their default left out); every scalar argument by value; every pointer
          argument as null or the ROLE of the array it points at -- the name of the call's input or of the result's attribute with that data pointer, "temp" when it is neither
          (a copy the binding made, a workspace it allocated); the value the library returned
  result  the shape and dtype of every array attribute of what the call returned (None-ness included), plain values as is
  error   instead of the two: type and message of the exception the call raised

Entries that do no device work (*_workspace_bytes, kernel_name, sample_capacity, strerror, ...) are forwarded to the real
library in both tables.  The compute entries are NOT forwarded in the host table (numpy inputs; they return CSP_OK), so that
table replays on a machine without a device; in the device table (torch CUDA tensors) they run.  tests/test_binding.py
imports cases() / run_case() from here and compares row for row.
"""
import ctypes
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "binding_contract.json")

NO_DEVICE_WORK = ("kernel_name", "sample_capacity", "strerror", "version", "device_count", "last_hip_error",
                  "release_cached_memory")


def does_no_device_work(symbol):
    return symbol.endswith("workspace_bytes") or symbol.split("csp_minsnap_")[-1] in NO_DEVICE_WORK


# ------------------------------------------------------------------------------------------------------------ the stand-in


# descriptor fields are written only where they differ from these (mem_space / device_id: from the table's own)
DESC_DEFAULTS = dict(abi_version=1, dtype=0, num_segments=0, seg_offsets="null", max_segments=0, bc_per_trajectory=0,
                     path_weight=0.0, vel_zero_weight=0.0, vel_zero_weight_per_traj="null", flags=0, reserved=0)
SPACE_DEFAULTS = {"host": dict(mem_space=0, device_id=-1), "device": dict(mem_space=1, device_id=0)}


def _struct_fields(obj, space):
    out = {}
    for name, ftype in obj._fields_:
        v = getattr(obj, name)
        out[name] = ("non-null" if v else "null") if ftype is ctypes.c_void_p else v
    if "abi_version" in out and "batch" in out:
        defaults = dict(DESC_DEFAULTS, **SPACE_DEFAULTS[space])
        out = {k: v for k, v in out.items() if k not in defaults or defaults[k] != v}
    return out


class Recorder:
    """Stands in for the binding's `_lib`.  Pointer arguments are kept as addresses until resolve() names them."""

    def __init__(self, real, space):
        self.real, self.space, self.forward_compute, self.calls = real, space, space == "device", []

    def __getattr__(self, symbol):
        fn = getattr(self.real, symbol)

        def call(*args):
            argtypes = fn.argtypes or ()
            assert len(args) == len(argtypes), (symbol, len(args), len(argtypes))
            rec = []
            for i, (t, a) in enumerate(zip(argtypes, args)):
                if t is ctypes.c_void_p:
                    addr = (a.value if isinstance(a, ctypes.c_void_p) else a) or 0
                    if symbol == "csp_minsnap_solve_multi" and addr:   # tables of args[1] entries: batch sizes, then pointers
                        n = args[1]
                        if i == 2:
                            rec.append(("vals", list((ctypes.c_int64 * n).from_address(addr))))
                        else:
                            rec.append(("table", [p or 0 for p in (ctypes.c_void_p * n).from_address(addr)]))
                    else:
                        rec.append(("ptr", addr))
                elif isinstance(t, type) and issubclass(t, ctypes._Pointer):
                    rec.append(("vals", None if a is None else _struct_fields(a._obj, self.space)))
                else:
                    rec.append(("vals", float(a) if t is ctypes.c_double else int(a)))
            ret = 0
            if self.forward_compute or does_no_device_work(symbol):
                ret = fn(*args)
            self.calls.append((symbol, rec, ret.decode() if isinstance(ret, bytes) else ret))
            return ret
        return call

    def resolve(self, roles):
        """Per call [symbol without "csp_" / "csp_minsnap_", arguments..., "->", returned value]; a returned 0 is left out, and a structure
        equal to the one before it in the case is written "="."""
        name = lambda p: "null" if not p else roles.get(p, "temp")
        out, last = [], None
        for symbol, rec, ret in self.calls:
            args = [v if kind == "vals" else (name(v) if kind == "ptr" else [name(p) for p in v]) for kind, v in rec]
            for k, a in enumerate(args):
                if isinstance(a, dict):
                    args[k], last = ("=" if a == last else a), a
            out.append([symbol[len("csp_"):].replace("minsnap_", "")] + args + (["->", ret] if ret != 0 else []))
        return out


# ------------------------------------------------------------------------------------------------- arrays, roles and results


def _is_array(x):
    return isinstance(x, np.ndarray) or type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _data_ptr(x):
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def _add_roles(roles, name, v):
    if _is_array(v):
        roles.setdefault(_data_ptr(v), name)
    elif isinstance(v, (list, tuple)):
        for k, e in enumerate(v):
            _add_roles(roles, "%s[%d]" % (name, k), e)
    elif name == "stream" and isinstance(v, int):
        roles.setdefault(v, name)


def _describe(v):
    if _is_array(v):
        dtype = str(v.dtype).replace("torch.", "").replace("float", "f").replace("uint", "u").replace("int", "i")
        return "%s %s" % ("x".join(str(n) for n in v.shape), dtype)
    if isinstance(v, (list, tuple)):
        return [_describe(e) for e in v]
    return v if v is None or isinstance(v, (bool, int, float, str)) else "<%s>" % type(v).__name__


def _attributes(obj):
    """Public attributes of a result holder or prepared object, in declaration order."""
    names = []
    for klass in reversed(type(obj).__mro__):
        names += [n for n in getattr(klass, "__slots__", ())]
    names += list(getattr(obj, "__dict__", {}))
    return [(n, getattr(obj, n, None)) for n in names if not n.startswith("_")]


class NC:
    """An input to hand over as a non-contiguous view."""
    def __init__(self, a):
        self.a = a


class Off:
    """An input whose data pointer is 8 bytes past a 16-byte boundary (contiguous)."""
    def __init__(self, a):
        self.a = a


class WS:
    """A caller's workspace of n bytes."""
    def __init__(self, n):
        self.n = n


class CpuTorch:
    """A torch tensor in host memory (the binding refuses it); a machine without torch leaves the case out."""
    def __init__(self, shape):
        self.shape = shape


class NewStream:
    """stream=: a stream of the caller's (device table), any handle (host table, where it is ignored)."""


class Np:
    """An input that stays a numpy array in both tables (knots_from_bc's arrays beside device waypoints)."""
    def __init__(self, a):
        self.a = a


class Backward:
    """backward=: the case calls an *_autograd function, then backward() of the sum of the outputs in `loss` ("coeffs" or
    "values": the first output, "cost": the second); of `inputs`, the function's differentiable ones, those in `wrt` require grad.
    The row's result also holds the shape and dtype, or None, of every such input's .grad."""
    def __init__(self, loss, inputs, wrt):
        self.loss, self.inputs, self.wrt = loss, inputs, wrt


def _forward_backward(target, kw, bw):
    """What the function returned, and the (name, .grad) of every differentiable input after backward()."""
    for n in bw.wrt:
        kw[n].requires_grad_()
    res = target(**kw)
    outs = dict(zip(("coeffs", "cost"), res if isinstance(res, tuple) else (res,)))
    outs["values"] = outs["coeffs"]   # eval_batch_autograd's one output
    sum(outs[n].double().sum() for n in bw.loss).backward()
    return res, [("grad " + n, getattr(kw[n], "grad", None)) for n in bw.inputs]


def _materialise(v, space, keep):
    if isinstance(v, Np):
        return _materialise(v.a, "host", keep)
    if isinstance(v, (NC, Off)):
        a = _materialise(v.a, space, keep)
        if space == "host":
            if isinstance(v, NC):
                return np.repeat(a, 2, axis=-1)[..., ::2]
            buf = np.empty(a.size + 3, dtype=a.dtype)
            k = ((16 - buf.ctypes.data % 16) % 16) // a.itemsize + 8 // a.itemsize
            buf[k:k + a.size] = a.reshape(-1)
            return buf[k:k + a.size].reshape(a.shape)
        import torch
        if isinstance(v, NC):
            return torch.repeat_interleave(a, 2, dim=-1)[..., ::2]
        k = 8 // a.element_size()
        buf = torch.empty(a.numel() + k, dtype=a.dtype, device=a.device)
        buf[k:] = a.reshape(-1)
        return buf[k:].reshape(a.shape)
    if isinstance(v, WS):
        v = np.zeros(v.n, dtype=np.uint8)
    if isinstance(v, CpuTorch):
        import torch
        return torch.ones(v.shape)
    if isinstance(v, NewStream):
        if space == "host":
            return 0x1230
        import torch
        keep.append(torch.cuda.Stream())
        return keep[-1].cuda_stream
    if isinstance(v, np.ndarray) and space == "device":
        import torch
        return torch.from_numpy(v).cuda()
    if isinstance(v, (list, tuple)):
        return type(v)(_materialise(e, space, keep) for e in v)
    return v


def run_case(csp, rec, space, fn, kwargs):
    """One row (without its name); None when the case needs torch tensors in host memory and torch is not installed.
    `rec` is the Recorder the caller has installed as csp._lib."""
    rec.calls = []
    keep = []
    try:
        kw = {k: _materialise(v, space, keep) for k, v in kwargs.items()}
    except ImportError:
        if space == "host" and any(isinstance(v, CpuTorch) for v in kwargs.values()):
            return None
        raise
    roles, grads, bw = {}, [], kw.pop("backward", None)
    for k, v in kw.items():
        _add_roles(roles, k, v)
    try:
        target = getattr(csp, fn)
        if bw is not None:
            res, grads = _forward_backward(target, kw, bw)
        else:
            res = target(**kw)
        if isinstance(target, type):   # a Prepared* class: the construction, then one run()
            n_ctor = len(rec.calls)
            ret = res.run()
            assert ret is res.out
        if space == "device":
            import torch
            torch.cuda.synchronize()
    except Exception as e:   # noqa: BLE001 -- the row is the exception
        return {"error": [type(e).__name__, str(e)]}
    if _is_array(res):
        attrs = [("ret", res)]
    elif isinstance(res, tuple):
        attrs = [("ret[%d]" % k, e) for k, e in enumerate(res)]
    else:
        attrs = _attributes(res)
    for n, v in attrs:
        _add_roles(roles, n, v)
    row = {"calls": rec.resolve(roles), "result": {n: _describe(v) for n, v in attrs + grads}}   # a .grad names no pointer
    if isinstance(target, type):
        row["calls_in_constructor"] = n_ctor
    return row


# ----------------------------------------------------------------------------------------------------------------- the cases


def cases(space):
    """(name, public function or class, keyword arguments) of every case of a table; arrays as numpy (run_case moves them)."""
    rng = np.random.default_rng(20261018)
    f4 = lambda a: a.astype(np.float32)
    dev = space == "device"

    def chain(n, S):   # waypoints of n trajectories of S segments, positive times
        return np.cumsum(rng.normal(0, 2, size=(n, S + 1, 3)), axis=1), rng.uniform(0.5, 2.0, size=(n, S))

    wp, tm = chain(3, 4)
    wp1, tm1 = chain(1, 4)
    wp0, tm0 = np.zeros((0, 5, 3)), np.zeros((0, 4))
    off = np.array([0, 1, 4, 6], dtype=np.int64)              # ragged lengths 1, 3, 2
    rwp, rtm = np.cumsum(rng.normal(0, 2, size=(9, 3)), axis=0), rng.uniform(0.5, 2.0, size=6)
    bc1, bc3 = rng.normal(0, 0.3, size=(1, 4, 3)), rng.normal(0, 0.3, size=(3, 4, 3))
    vw = rng.uniform(0, 0.2, size=3)
    out = []

    def add(name, fn, **kw):
        out.append((name, fn, kw))

    def family(fn, U, R, ONE, Z, bc=True, extra=None, b0=True, vwp=True, full=True):
        """The waypoints / times / bc / seg_offsets / per-trajectory-weight inputs every solve entry shares.  full=False: the
        entries that were written on _CallInputs from the start get the cases that tell its arms apart, not every one."""
        extra = extra or (lambda w, t: {})
        x = lambda d: dict(d, **extra(d["waypoints"], d["times"]))
        U, R, ONE, Z = x(U), x(R), x(ONE), x(Z)
        w = dict(vel_zero_weight_per_traj=NC(vw)) if vwp else {}
        add("uniform", fn, **U)
        add("ragged", fn, **R)
        add("B = 1", fn, **ONE)
        if b0:
            add("B = 0", fn, **Z)
        if bc:
            add("bc [B,4,3]", fn, **U, bc=bc3)
            add("bc [2,4,3]: neither shared nor per trajectory", fn, **U, bc=bc3[:2])
            add("B = 1, bc [1,4,3]", fn, **ONE, bc=bc1)
        add("non-contiguous inputs", fn, **{k: NC(v) if isinstance(v, np.ndarray) else v for k, v in R.items()}, **w)
        if full:
            add("f32 waypoints, f64 times", fn, **x(dict(U, waypoints=f4(U["waypoints"]))))
            add("stream", fn, **U, stream=NewStream())
            add("ragged, max_segments given", fn, **R, max_segments=3)
            add("uniform, max_segments given", fn, **U, max_segments=9)
            add("f64 waypoints, f32 times", fn, **dict(U, times=f4(U["times"])))
            if bc:
                add("B = 1, bc [4,3]", fn, **ONE, bc=bc1[0])
                add("bc in the other dtype, non-contiguous", fn, **U, bc=NC(f4(bc1)))
            if vwp:
                add("vel_zero_weight_per_traj as f32", fn, **U, vel_zero_weight=0.05, vel_zero_weight_per_traj=f4(vw))
        return U, R, ONE

    base = (dict(waypoints=wp, times=tm), dict(waypoints=rwp, times=rtm, seg_offsets=off), dict(waypoints=wp1, times=tm1),
            dict(waypoints=wp0, times=tm0))

    # ---- solve_batch
    U, R, ONE = family("solve_batch", *base)
    for k in ("want_max_dev", "want_status", "force_generic", "segment_major", "no_persistent", "span"):
        add(k, "solve_batch", **U, **{k: True})
    add("f32_arith", "solve_batch", waypoints=f4(wp), times=f4(tm), f32_arith=True)
    add("every flag and both wants", "solve_batch", **U, want_max_dev=True, want_status=True, force_generic=True,
        segment_major=True, no_persistent=True, span=True, order=3, path_weight=1e-3, vel_zero_weight=0.02)
    add("segment_major with seg_offsets", "solve_batch", **R, segment_major=True)
    add("out=", "solve_batch", **U, out=np.zeros((3, 4, 3, 8)))
    add("workspace too small", "solve_batch", **U, force_generic=True, workspace=WS(16))
    add("workspace large enough", "solve_batch", **U, force_generic=True, workspace=WS(1 << 16))
    add("ngpu=1", "solve_batch", **U, ngpu=1, want_status=True, want_max_dev=True)
    if not dev:
        add("torch tensors that are not CUDA tensors", "solve_batch", waypoints=CpuTorch((3, 5, 3)), times=CpuTorch((3, 4)))

    # ---- solve_batch_vjp
    gco = lambda w, t: dict(grad_coeffs=rng.normal(size=(t.size, 3, 8)).reshape(t.shape + (3, 8)))
    U, R, ONE = family("solve_batch_vjp", *base, extra=gco)   # (the device table runs B = 0 where a GPU test already does)
    for want in ((), ("times",), ["bc", "waypoints"]):
        add("want=%r" % (want,), "solve_batch_vjp", **U, want=want)
    add("want= an unknown name", "solve_batch_vjp", **U, want=("coeffs",))
    add("want_status", "solve_batch_vjp", **U, want_status=True)
    add("grad_coeffs not 16-byte aligned", "solve_batch_vjp", **dict(U, grad_coeffs=Off(U["grad_coeffs"])))
    add("grad_coeffs in the other dtype, non-contiguous", "solve_batch_vjp", **dict(U, grad_coeffs=NC(f4(U["grad_coeffs"]))))
    add("grad_coeffs of the wrong size", "solve_batch_vjp", **dict(U, grad_coeffs=np.zeros((3, 3, 3, 8))))
    add("workspace too small", "solve_batch_vjp", **U, workspace=WS(16))
    add("workspace large enough", "solve_batch_vjp", **U, workspace=WS(1 << 20))
    add("B = 1, bc [1,4,3], workspace large enough", "solve_batch_vjp", **ONE, bc=bc1, workspace=WS(1 << 20))

    # ---- snap_cost_batch, optimize_times_batch
    U, R, ONE = family("snap_cost_batch", *base, b0=not dev, full=False)
    add("want_grad=False", "snap_cost_batch", **U, want_grad=False)
    add("workspace too small", "snap_cost_batch", **U, workspace=WS(16))
    add("workspace large enough", "snap_cost_batch", **U, workspace=WS(1 << 20))
    U, R, ONE = family("optimize_times_batch", *base, b0=not dev, full=False)
    add("time_penalty, every parameter", "optimize_times_batch", **U, mode="time_penalty", time_weight=2.0, min_time=0.05,
        tol=1e-4, max_iters=7, order=3)
    add("want_coeffs=False", "optimize_times_batch", **R, want_coeffs=False)
    add("an unknown mode", "optimize_times_batch", **U, mode="fastest")
    add("workspace too small", "optimize_times_batch", **U, workspace=WS(16))
    add("workspace large enough", "optimize_times_batch", **U, workspace=WS(1 << 20))

    # ---- solve_periodic_batch (closed loops: S waypoints per trajectory), periodic_time_alloc_batch
    loops = (dict(waypoints=wp[:, :4], times=tm), dict(waypoints=rwp[:6], times=rtm, seg_offsets=off),
             dict(waypoints=wp1[:, :4], times=tm1), dict(waypoints=wp0[:, :4], times=tm0))
    U, R, ONE = family("solve_periodic_batch", *loops, bc=False, b0=not dev, full=False)
    add("want_cost", "solve_periodic_batch", **U, want_cost=True)
    add("want_grad", "solve_periodic_batch", **R, want_grad=True)
    add("workspace too small", "solve_periodic_batch", **U, want_cost=True, want_grad=True, workspace=WS(16))
    add("workspace large enough", "solve_periodic_batch", **U, workspace=WS(1 << 20))
    add("uniform", "periodic_time_alloc_batch", waypoints=wp[:, :4], v_avg=5.0, min_time_s=0.1)
    add("ragged", "periodic_time_alloc_batch", waypoints=rwp[:6], v_avg=5.0, min_time_s=0.1, seg_offsets=off)

    # ---- PreparedSolve (device memory only)
    if dev:
        U, R, ONE = family("PreparedSolve", *base, b0=False, vwp=False)
        for k in ("force_generic", "segment_major", "no_persistent", "span"):
            add(k, "PreparedSolve", **U, **{k: True})
        add("segment_major with seg_offsets", "PreparedSolve", **R, segment_major=True)
        add("out=, weights, order 3", "PreparedSolve", **U, out=np.zeros((3, 4, 3, 6)), order=3, path_weight=1e-3, vel_zero_weight=0.02)
    else:
        add("host arrays", "PreparedSolve", waypoints=wp, times=tm)

    # ---- solve_mixed, PreparedMixed
    orders = np.array([3, 5, 4], dtype=np.int32)
    M = dict(orders=orders, waypoints=rwp, times=rtm, seg_offsets=off)
    if not dev:
        add("host arrays", "PreparedMixed", **M)
    for fn in ("solve_mixed", "PreparedMixed") if dev else ("solve_mixed",):
        add("base", fn, **M)
        add("f32 waypoints, orders as int64, max_segments", fn, **dict(M, waypoints=f4(rwp), orders=orders.astype(np.int64)),
            max_segments=3)
        add("non-contiguous inputs", fn, **{k: NC(v) for k, v in M.items()}, bc=NC(bc3))
        add("bc [4,3]", fn, **M, bc=bc1[0])
        add("bc [B,4,3], want_status", fn, **M, bc=bc3, vel_zero_weight=0.02, want_status=True)
        add("B = 1, bc [1,4,3]", fn, orders=orders[:1], waypoints=rwp[:4], times=rtm[:3], seg_offsets=off[[0, 2]] * 3 // 4, bc=bc1)
        add("stream", fn, **M, stream=NewStream())
        add("out= large enough", fn, **M, out=np.zeros(256))
    add("B = 0", "solve_mixed", orders=np.zeros(0, np.int32), waypoints=np.zeros((0, 3)), times=np.zeros(0),
        seg_offsets=np.zeros(1, np.int64))
    add("vel_zero_weight_per_traj", "solve_mixed", **M, vel_zero_weight_per_traj=f4(vw))
    add("out= too small", "solve_mixed", **M, out=np.zeros(8))
    add("out= in the wrong dtype", "solve_mixed", **M, out=np.zeros(256, dtype=np.float32))

    # ---- PreparedMulti (device memory only; host arrays end in an AttributeError, which is no contract)
    if dev:
        w2, t2 = chain(2, 4)
        add("two batches", "PreparedMulti", waypoints=[wp, w2], times=[tm, t2])
        add("bcs per trajectory, want_status, stream, order 3", "PreparedMulti", waypoints=[wp, NC(w2)], times=[f4(tm), t2],
            bcs=[bc3, f4(bc3[:2])], order=3, vel_zero_weight=0.02, want_status=True, stream=NewStream())
        add("bcs shared or None", "PreparedMulti", waypoints=[wp, w2], times=[tm, t2], bcs=[None, bc1])

    # ---- time_alloc_batch, plan_batch, generate_batch, sample_capacity, sample_batch
    big = wp * 4.0
    add("uniform", "time_alloc_batch", waypoints=wp, v_avg=5.0, min_time_s=0.1)
    add("ragged, stream", "time_alloc_batch", waypoints=rwp, v_avg=5.0, min_time_s=0.1, seg_offsets=off, stream=NewStream())
    add("f32, non-contiguous", "time_alloc_batch", waypoints=NC(f4(rwp)), v_avg=2, min_time_s=1, seg_offsets=NC(off.astype(np.int32)))
    if not dev:
        add("B = 0", "time_alloc_batch", waypoints=wp0, v_avg=5.0, min_time_s=0.1)
    for fn, kw in (("plan_batch", {}), ("generate_batch", dict(sample_distance=0.7, capacity=64))):
        P = dict(waypoints=big, v_avg=5.0, min_time_s=0.1, **kw)
        add("base", fn, **P)
        add("f32, non-contiguous, order 4, weights", fn, **dict(P, waypoints=NC(f4(big))), order=4, path_weight=1e-4, vel_zero_weight=0.02)
        add("bc [4,3]", fn, **P, bc=bc1[0])
        add("bc [B,4,3] in the other dtype", fn, **P, bc=f4(bc3))
        add("bc [2,4,3]: no check here", fn, **P, bc=NC(bc3[:2]))
        add("B = 1, bc [1,4,3]", fn, **dict(P, waypoints=wp1 * 4.0), bc=bc1)
    add("capacity omitted", "generate_batch", waypoints=big, v_avg=5.0, min_time_s=0.1, sample_distance=0.7)
    add("long_segments", "generate_batch", waypoints=big, v_avg=5.0, min_time_s=0.1, sample_distance=0.7, capacity=64, long_segments=True)
    if not dev:
        add("base", "sample_capacity", waypoints=big, v_avg=5.0, min_time_s=0.1)
        add("f32, non-contiguous, order 4", "sample_capacity", waypoints=NC(f4(big)), v_avg=5.0, min_time_s=0.1, order=4)
    stm = rng.uniform(0.5, 1.0, size=(3, 4))
    sco = rng.normal(0, 0.5, size=(3, 4, 3, 6))
    Sa = dict(times=stm, coeffs=sco, sample_distance=0.7, capacity=64)
    add("base", "sample_batch", **Sa)
    add("order given, one_lane, long_segments", "sample_batch", **Sa, order=3, one_lane=True, long_segments=True)
    add("f32 times, f64 coeffs, non-contiguous", "sample_batch", **dict(Sa, times=NC(f4(stm)), coeffs=NC(sco)))
    add("out=", "sample_batch", **Sa, out=(np.zeros((3, 64, 3)), np.zeros(3, np.int32), np.zeros((3, 2))))
    add("seg_offsets", "sample_batch", **dict(Sa, times=stm.reshape(-1)[:6], coeffs=sco.reshape(-1, 3, 6)[:6]), seg_offsets=off.astype(np.int32))
    if not dev:
        add("B = 0", "sample_batch", **dict(Sa, times=tm0, coeffs=np.zeros((0, 4, 3, 6))))

    # ---- the memory-space wrappers without a descriptor: geo, altitude, bezier
    lla = np.column_stack([rng.uniform(116.0, 116.1, 5), rng.uniform(39.9, 40.0, 5), rng.uniform(0, 500, 5)])
    ref = np.array([116.05, 39.95, 30.0])
    for fn, pts in (("wgs84_to_enu_batch", "lla"), ("enu_to_wgs84_batch", "enu")):
        add("base", fn, **{pts: lla, "ref": ref.tolist()})
        add("f32 points, non-contiguous, ref as a tuple", fn, **{pts: NC(f4(lla)), "ref": tuple(f4(ref))})
    n = 20
    xyz = np.column_stack([np.cumsum(rng.uniform(20, 60, size=(n, 2)), axis=0), 100 + np.cumsum(rng.normal(0, 8, n))])
    elev = 80 + 10 * np.sin(np.arange(n) / 5.0)
    aoff = np.array([0, 8, 20], dtype=np.int64)
    add("base", "alt_optimize_heights_batch", xyz=xyz, elev=elev, offsets=aoff)
    add("f32, non-contiguous, every parameter", "alt_optimize_heights_batch", xyz=NC(f4(xyz)), elev=NC(f4(elev)),
        offsets=NC(aoff.astype(np.int32)), lambda_smooth=2.0, lambda_follow=0.5, safe_distance=40.0, max_climb_rate=1.5)
    add("base", "alt_global_smooth_batch", input_z=xyz[:, 2] + 5.0, xyz=xyz, offsets=aoff)
    add("f32, non-contiguous, every parameter", "alt_global_smooth_batch", input_z=NC(f4(xyz[:, 2])), xyz=NC(f4(xyz)),
        offsets=NC(aoff.astype(np.int32)), lambda_smooth=2.0, max_climb_rate=1.5)
    bwp = np.cumsum(rng.uniform(5, 20, size=(7, 3)), axis=0)
    boff = np.array([0, 3, 7], dtype=np.int64)
    add("base", "bezier_generate_batch", waypoints=bwp, offsets=boff, capacity=64)
    add("f32, non-contiguous, every parameter", "bezier_generate_batch", waypoints=NC(f4(bwp)), offsets=NC(boff.astype(np.int32)),
        resolution=0.5, min_radius=2.0, capacity=128)

    # ---- reverse mode, knots and evaluation.  Appended here: every draw above keeps its place in the rng's sequence.
    subsets = lambda names: [tuple(n for k, n in enumerate(names) if m >> k & 1) for m in range(1 << len(names))]
    nB = lambda t: t.shape[0] if t.ndim == 2 else off.size - 1
    gj = lambda w, t: dict(grad_cost=rng.normal(size=nB(t)))
    wrong = np.zeros((3, 3, 3, 8))   # a grad_coeffs of the wrong size

    # ---- solve_periodic_batch_vjp
    fn = "solve_periodic_batch_vjp"
    U, R, ONE = family(fn, *loops, bc=False, extra=gco, b0=not dev, full=False)
    add("order 3", fn, **dict(U, grad_coeffs=U["grad_coeffs"][..., :6]), order=3)
    add("grad_cost", fn, **U, **gj(wp, tm))
    add("ragged, grad_cost as f32", fn, **R, grad_cost=f4(gj(rwp, rtm)["grad_cost"]))
    for want in ((), ("times",), ["times", "waypoints"]):
        add("want=%r" % (want,), fn, **U, want=want)
    add("want= an unknown name", fn, **U, want=("bc",))
    add("want_status", fn, **U, want_status=True)
    add("grad_coeffs not 16-byte aligned", fn, **dict(U, grad_coeffs=Off(U["grad_coeffs"])))
    add("grad_coeffs in the other dtype, non-contiguous", fn, **dict(U, grad_coeffs=NC(f4(U["grad_coeffs"]))))
    add("grad_coeffs of the wrong size", fn, **dict(U, grad_coeffs=wrong))
    add("grad_cost of the wrong size", fn, **U, grad_cost=np.zeros(2))
    add("workspace too small", fn, **U, workspace=WS(16))
    add("workspace large enough", fn, **U, workspace=WS(1 << 20))

    # ---- solve_knots_batch: the standard problem's knots (knots_from_bc), then a free start and a pinned interior knot
    knots_from_bc = importlib.import_module("cs-pathplan_amd").knots_from_bc

    def knots(w, t, order=4):
        if t.ndim == 2:
            mk, kv = knots_from_bc({3: bc3, 1: bc1}.get(t.shape[0]), t.shape[1], order, batch=t.shape[0])
        else:
            mk, kv = (np.concatenate([a[0] for a in part])
                      for part in zip(*(knots_from_bc(None, int(n), order) for n in np.diff(off))))
        return dict(knot_mask=mk, knot_values=kv)

    chains = tuple(dict(d, **knots(d["waypoints"], d["times"])) for d in base)
    fn = "solve_knots_batch"
    U, R, ONE = family(fn, *chains, bc=False, b0=not dev, full=False)
    pinned = dict(U, knot_mask=U["knot_mask"].copy(), knot_values=U["knot_values"] + rng.normal(0, 0.3, size=(3, 5, 3, 3)))
    pinned["knot_mask"][:, 0], pinned["knot_mask"][:, 2] = 0, 0b001
    add("a free start, velocity pinned at knot 2", fn, **pinned)
    add("order 3", fn, **dict(U, **knots(wp, tm, order=3)), order=3)
    add("want_cost", fn, **U, want_cost=True)
    add("knot_mask of the wrong size", fn, **dict(U, knot_mask=U["knot_mask"][:, :4]))
    add("knot_values of the wrong size", fn, **dict(U, knot_values=U["knot_values"][:, :, :2]))
    add("knot_mask and knot_values as numpy arrays", fn, **dict(U, knot_mask=Np(U["knot_mask"]), knot_values=Np(U["knot_values"])))
    add("workspace too small", fn, **U, want_cost=True, workspace=WS(16))
    add("workspace large enough", fn, **U, workspace=WS(1 << 20))

    # ---- solve_knots_batch_vjp
    fn = "solve_knots_batch_vjp"
    U, R, ONE = family(fn, *chains, bc=False, extra=lambda w, t: dict(gco(w, t), **gj(w, t)), b0=not dev, full=False)
    only = lambda d, drop: {k: v for k, v in d.items() if k != drop}
    add("a free start, velocity pinned at knot 2", fn, **dict(U, knot_mask=pinned["knot_mask"], knot_values=pinned["knot_values"]))
    add("order 3", fn, **dict(U, **knots(wp, tm, order=3), grad_coeffs=U["grad_coeffs"][..., :6]), order=3)
    add("grad_coeffs alone", fn, **only(U, "grad_cost"))
    add("grad_cost alone", fn, **only(U, "grad_coeffs"))
    add("neither cotangent", fn, **only(only(U, "grad_cost"), "grad_coeffs"))
    for want in subsets(("waypoints", "times", "knot_values")):
        add("want=%r" % (want,), fn, **U, want=want)
    add("want= a list", fn, **U, want=["knot_values", "waypoints"])
    add("want= an unknown name", fn, **U, want=("bc",))
    add("want_status", fn, **U, want_status=True)
    add("knot_mask and knot_values as numpy arrays", fn, **dict(U, knot_mask=Np(U["knot_mask"]), knot_values=Np(U["knot_values"])))
    add("grad_coeffs not 16-byte aligned", fn, **dict(U, grad_coeffs=Off(U["grad_coeffs"])))
    add("grad_coeffs in the other dtype, non-contiguous", fn, **dict(U, grad_coeffs=NC(f4(U["grad_coeffs"]))))
    add("grad_coeffs of the wrong size", fn, **dict(U, grad_coeffs=wrong))
    add("grad_cost of the wrong size", fn, **dict(U, grad_cost=np.zeros(2)))
    add("workspace too small", fn, **U, workspace=WS(16))
    add("workspace large enough", fn, **U, workspace=WS(1 << 20))
    add("grad_cost alone, workspace large enough", fn, **only(U, "grad_coeffs"), workspace=WS(1 << 20))

    # ---- eval_batch, eval_batch_vjp (no _CallInputs: times / coeffs / query)
    Q = 5
    eco, eco1 = rng.normal(0, 0.5, size=(3, 4, 3, 8)), rng.normal(0, 0.5, size=(1, 4, 3, 8))
    qry = lambda t: rng.uniform(0, 1, size=(t.shape[0], Q)) * t.sum(axis=1, keepdims=True)
    rq = rng.uniform(0, 1, size=(3, Q)) * np.add.reduceat(rtm, off[:-1])[:, None]
    EU, ER = dict(times=tm, coeffs=eco, query=qry(tm)), dict(times=rtm, coeffs=eco.reshape(-1, 3, 8)[:6], query=rq, seg_offsets=off)
    EONE = dict(times=tm1, coeffs=eco1, query=qry(tm1))
    gout = rng.normal(size=(3, Q, 3, 3))
    for fn, g in (("eval_batch", {}), ("eval_batch_vjp", dict(grad_out=gout))):
        add("uniform", fn, **EU, **g)
        add("ragged", fn, **ER, **g)
        add("ragged, max_segments given", fn, **ER, **g, max_segments=3)
        add("B = 1", fn, **EONE, **{k: v[:1] for k, v in g.items()})
        add("order given", fn, **EU, **g, order=4)
        add("order 3", fn, **dict(EU, coeffs=eco[..., :6]), **g)
        add("Q = 0", fn, **dict(EU, query=np.zeros((3, 0))), **{k: v[:, :0] for k, v in g.items()})
        add("want_status", fn, **EU, **g, want_status=True)
        add("non-contiguous inputs", fn, **{k: NC(v) for k, v in ER.items()}, **{k: NC(v) for k, v in g.items()})
        add("f32 times, f64 coeffs and query", fn, **dict(EU, times=f4(tm)), **g)
        add("stream", fn, **EU, **g, stream=NewStream())
        add("coeffs not 16-byte aligned", fn, **dict(EU, coeffs=Off(eco)), **g)
        add("coeffs of the wrong size", fn, **dict(EU, coeffs=eco[:, :3]), **g)
        add("query [2,Q]", fn, **dict(EU, query=EU["query"][:2]), **g)
        add("query [Q]", fn, **dict(EU, query=EU["query"][0]), **g)
    add("want_seg_index", "eval_batch", **EU, want_seg_index=True)
    add("num_derivs=1", "eval_batch", **EU, num_derivs=1)
    fn = "eval_batch_vjp"
    add("num_derivs given, grad_out [B,Q,9]", fn, **EU, grad_out=gout.reshape(3, Q, 9), num_derivs=3)
    add("num_derivs taken from grad_out [B,Q,2,3]", fn, **EU, grad_out=gout[:, :, :2])
    add("grad_out of the wrong size", fn, **EU, grad_out=gout[:, :, :2], num_derivs=3)
    add("grad_out in the other dtype", fn, **EU, grad_out=f4(gout))
    for want in subsets(("coeffs", "times", "query")):
        add("want=%r" % (want,), fn, **EU, grad_out=gout, want=want)
    add("want= a list", fn, **EU, grad_out=gout, want=["query", "coeffs"])
    add("want= an unknown name", fn, **EU, grad_out=gout, want=("waypoints",))

    # ---- the *_autograd functions: forward, then backward() (device memory only)
    if dev:
        def autograd(fn, inputs, losses, U, R, U3=None):
            for loss, kw in losses:
                for wrt in (inputs,) + tuple((n,) for n in inputs):
                    add("loss on %s%s, grad of %s" % (" + ".join(loss), ", with_cost" if kw.get("with_cost") else "", ", ".join(wrt)),
                        fn, **U, **kw, backward=Backward(loss, inputs, wrt))
            add("ragged, loss on %s" % " + ".join(loss), fn, **R, **kw, backward=Backward(loss, inputs, inputs))
            if U3 is not None:
                add("order 3, f32, loss on %s" % " + ".join(loss), fn, **{k: f4(v) if v.dtype == np.float64 else v for k, v in U3.items()},
                    order=3, **kw, backward=Backward(loss, inputs, inputs))

        C = dict(with_cost=True)
        losses = ((("coeffs",), {}), (("coeffs",), C), (("cost",), C), (("coeffs", "cost"), C))
        U, R = dict(base[0], bc=bc3), dict(base[1], bc=bc3)
        autograd("solve_batch_autograd", ("waypoints", "times", "bc"), losses, U, R, U)
        add("bc [4,3], loss on coeffs + cost, grad of bc", "solve_batch_autograd", **base[0], bc=bc1[0], with_cost=True,
            backward=Backward(("coeffs", "cost"), ("waypoints", "times", "bc"), ("bc",)))
        add("bc=None, loss on cost, grad of times", "solve_batch_autograd", **base[0], with_cost=True,
            backward=Backward(("cost",), ("waypoints", "times"), ("times",)))
        autograd("solve_periodic_batch_autograd", ("waypoints", "times"), losses, loops[0], loops[1], loops[0])
        U = chains[0]
        autograd("solve_knots_batch_autograd", ("waypoints", "times", "knot_values"), losses, U, chains[1],
                 dict(U, **knots(wp, tm, order=3)))
        add("knot_mask and knot_values as numpy arrays, loss on cost", "solve_knots_batch_autograd",
            **dict(U, knot_mask=Np(U["knot_mask"]), knot_values=Np(U["knot_values"])), with_cost=True,
            backward=Backward(("cost",), ("waypoints", "times"), ("waypoints", "times")))
        autograd("eval_batch_autograd", ("coeffs", "times", "query"), ((("values",), {}),), EU, ER)
    return [("%s: %s" % (fn, name), fn, kw) for name, fn, kw in out]


def record(csp, space):
    rec = Recorder(csp.raw_lib(), space)
    real, csp._lib = csp._lib, rec
    try:
        return [dict(case=name, **run_case(csp, rec, space, fn, kw)) for name, fn, kw in cases(space)]
    finally:
        csp._lib = real


def _dumps(row):
    return json.dumps(row, separators=(",", ":"))


def main():
    sys.path.insert(0, ROOT)
    csp = importlib.import_module("cs-pathplan_amd")
    space = "device" if "--device" in sys.argv[1:] else "host"
    doc = {"host": [], "device": []}
    if os.path.exists(OUT):
        with open(OUT) as f:
            doc = json.load(f)
    doc[space] = record(csp, space)
    with open(OUT, "w") as f:
        f.write('{"host": [\n' + ",\n".join(_dumps(r) for r in doc["host"]))
        f.write('\n], "device": [\n' + ",\n".join(_dumps(r) for r in doc["device"]) + "\n]}\n")
    print("%s: %d host rows, %d device rows" % (OUT, len(doc["host"]), len(doc["device"])))


if __name__ == "__main__":
    main()
