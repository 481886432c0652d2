"""cs-pathplan_amd -- MI355X-native batched minimum-snap solver (Python binding of the C-ABI).

The directory name carries a hyphen, so import it with

    import importlib; csp = importlib.import_module("cs-pathplan_amd")

This module is a thin ctypes layer over libcsp_minsnap.so (include/csp_minsnap.h).  It is used
by tests/, bench.py and the torch.distributed sharding helper; the drop-in for the reference's
C++ callers is the class shim in host/math_util/minimum_snap.hpp.

There is NO CPU fallback: importing fails loudly when the HIP extension has not been built,
and every solve call raises when no gfx950 device is visible.
"""
import ctypes
import math
import operator
import os

import numpy as np

try:
    # Must precede the CDLL below.  torch bundles its own libamdhip64.so.7; if ours (linked to
    # /opt/rocm) were loaded first the process would hold two HIP runtimes and torch would then
    # report "No HIP GPUs are available".  Loading torch first makes both share one runtime.
    import torch  # noqa: F401
except ImportError:  # the C-ABI itself does not need torch (host-memory calls, C++ callers)
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcsp_minsnap.so")

ABI_VERSION = 1
DTYPE_F64, DTYPE_F32 = 0, 1
MEM_HOST, MEM_DEVICE = 0, 1
FLAG_FORCE_GENERIC = 0x1
FLAG_SEGMENT_MAJOR = 0x2
FLAG_NO_PERSISTENT = 0x4
FLAG_F32_ARITH = 0x8
FLAG_LONG_SEGMENTS = 0x10
FLAG_SPAN = 0x20
TRAJ_OK, TRAJ_NONFINITE, TRAJ_NOT_SPD, TRAJ_SKIPPED = 0, 1, 2, 4
TRAJ_NOT_CONVERGED = 8
TIMEOPT_FIXED_TOTAL, TIMEOPT_TIME_PENALTY = 0, 1

EXPORTED_SYMBOLS = (
    "csp_minsnap_solve_batch", "csp_minsnap_solve_batch_sharded", "csp_minsnap_workspace_bytes", "csp_minsnap_time_alloc_batch",
    "csp_minsnap_solve_batch_vjp", "csp_minsnap_vjp_workspace_bytes",
    "csp_minsnap_solve_batch_cost_vjp", "csp_minsnap_cost_vjp_workspace_bytes",
    "csp_minsnap_cost_batch", "csp_minsnap_cost_workspace_bytes", "csp_minsnap_optimize_times_batch",
    "csp_minsnap_timeopt_workspace_bytes",
    "csp_minsnap_solve_periodic_batch", "csp_minsnap_periodic_workspace_bytes",
    "csp_minsnap_solve_periodic_batch_vjp", "csp_minsnap_periodic_vjp_workspace_bytes",
    "csp_minsnap_solve_knots_batch", "csp_minsnap_knots_workspace_bytes",
    "csp_minsnap_solve_knots_batch_vjp", "csp_minsnap_knots_vjp_workspace_bytes",
    "csp_minsnap_optimize_times_knots_batch", "csp_minsnap_knots_timeopt_workspace_bytes",
    "csp_minsnap_optimize_times_periodic_batch", "csp_minsnap_periodic_timeopt_workspace_bytes",
    "csp_minsnap_eval_batch", "csp_minsnap_eval_batch_vjp",
    "csp_minsnap_solve_mixed", "csp_minsnap_mixed_workspace_bytes", "csp_minsnap_solve_multi",
    "csp_minsnap_plan_batch", "csp_minsnap_plan_workspace_bytes", "csp_minsnap_sample_batch",
    "csp_minsnap_generate_batch", "csp_minsnap_sample_capacity",
    "csp_minsnap_kernel_name", "csp_minsnap_device_count", "csp_minsnap_version",
    "csp_minsnap_strerror", "csp_minsnap_last_hip_error", "csp_minsnap_release_cached_memory",
    "csp_geo_wgs84_to_enu_batch", "csp_geo_enu_to_wgs84_batch",
    "csp_alt_workspace_bytes", "csp_alt_optimize_heights_batch", "csp_alt_global_smooth_batch",
    "csp_bezier_generate_batch",
)


class CspError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        super().__init__("csp_minsnap error %d (%s)%s" % (code, strerror(code), (": " + detail) if detail else ""))


class Desc(ctypes.Structure):
    """Mirror of `csp_minsnap_desc` (include/csp_minsnap.h)."""
    _fields_ = [
        ("abi_version", ctypes.c_uint32), ("dtype", ctypes.c_uint32),
        ("order", ctypes.c_int32), ("num_segments", ctypes.c_int32),
        ("batch", ctypes.c_int64),
        ("seg_offsets", ctypes.c_void_p),
        ("max_segments", ctypes.c_int32), ("bc_per_trajectory", ctypes.c_uint32),
        ("path_weight", ctypes.c_double), ("vel_zero_weight", ctypes.c_double),
        ("vel_zero_weight_per_traj", ctypes.c_void_p),
        ("mem_space", ctypes.c_uint32), ("device_id", ctypes.c_int32),
        ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]


class TimeOptParams(ctypes.Structure):
    """Mirror of `csp_minsnap_timeopt_params` (include/csp_minsnap.h)."""
    _fields_ = [
        ("abi_version", ctypes.c_uint32), ("mode", ctypes.c_uint32),
        ("time_weight", ctypes.c_double), ("min_time", ctypes.c_double), ("tol", ctypes.c_double),
        ("max_iters", ctypes.c_int32), ("reserved", ctypes.c_uint32),
    ]


def make_timeopt_params(mode=TIMEOPT_FIXED_TOTAL, time_weight=0.0, min_time=0.01, tol=1e-6, max_iters=100):
    p = TimeOptParams()
    p.abi_version = ABI_VERSION
    p.mode = int(mode)
    p.time_weight = float(time_weight)
    p.min_time = float(min_time)
    p.tol = float(tol)
    p.max_iters = int(max_iters)
    p.reserved = 0
    return p


class AltParams(ctypes.Structure):
    """Mirror of `csp_alt_params` (include/csp_alt.h; reference AltitudeParams, uavPathPlanning.hpp:415-421)."""
    _fields_ = [("lambda_smooth", ctypes.c_double), ("lambda_follow", ctypes.c_double),
                ("safe_distance", ctypes.c_double), ("max_climb_rate", ctypes.c_double)]


if not os.path.exists(LIB_PATH):
    raise ImportError(
        "cs-pathplan_amd: %s is missing.  Build the HIP extension first "
        "(python cs-pathplan_amd/build.py, or __graft_entry__.build()); there is no CPU fallback." % LIB_PATH)

_lib = ctypes.CDLL(LIB_PATH)

# every prototype of the library: symbol -> (restype, argtypes)
_I, _I32, _I64, _U32, _SZ, _F, _P, _S = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_size_t,
                                         ctypes.c_double, ctypes.c_void_p, ctypes.c_char_p)
_D, _ALT = ctypes.POINTER(Desc), ctypes.POINTER(AltParams)
_PROTOTYPES = {
    "csp_minsnap_solve_batch": (_I, [_D] + [_P] * 7 + [_SZ, _P]),
    "csp_minsnap_solve_batch_sharded": (_I, [_D] + [_P] * 6 + [_I]),
    "csp_minsnap_workspace_bytes": (_SZ, [_D]),
    "csp_minsnap_solve_batch_vjp": (_I, [_D] + [_P] * 9 + [_SZ, _P]),
    "csp_minsnap_vjp_workspace_bytes": (_SZ, [_D]),
    "csp_minsnap_solve_batch_cost_vjp": (_I, [_D] + [_P] * 10 + [_SZ, _P]),
    "csp_minsnap_cost_vjp_workspace_bytes": (_SZ, [_D, _I]),
    "csp_minsnap_cost_batch": (_I, [_D] + [_P] * 7 + [_SZ, _P]),
    "csp_minsnap_cost_workspace_bytes": (_SZ, [_D]),
    "csp_minsnap_optimize_times_batch": (_I, [_D, ctypes.POINTER(TimeOptParams)] + [_P] * 9 + [_SZ, _P]),
    "csp_minsnap_timeopt_workspace_bytes": (_SZ, [_D]),
    "csp_minsnap_solve_periodic_batch": (_I, [_D] + [_P] * 7 + [_SZ, _P]),
    "csp_minsnap_periodic_workspace_bytes": (_SZ, [_D]),
    "csp_minsnap_solve_periodic_batch_vjp": (_I, [_D] + [_P] * 8 + [_SZ, _P]),
    "csp_minsnap_periodic_vjp_workspace_bytes": (_SZ, [_D]),
    "csp_minsnap_solve_knots_batch": (_I, [_D] + [_P] * 8 + [_SZ, _P]),
    "csp_minsnap_knots_workspace_bytes": (_SZ, [_D]),
    "csp_minsnap_solve_knots_batch_vjp": (_I, [_D] + [_P] * 11 + [_SZ, _P]),
    "csp_minsnap_knots_vjp_workspace_bytes": (_SZ, [_D, _I]),
    "csp_minsnap_optimize_times_knots_batch": (_I, [_D, ctypes.POINTER(TimeOptParams)] + [_P] * 10 + [_SZ, _P]),
    "csp_minsnap_knots_timeopt_workspace_bytes": (_SZ, [_D]),
    "csp_minsnap_optimize_times_periodic_batch": (_I, [_D, ctypes.POINTER(TimeOptParams)] + [_P] * 8 + [_SZ, _P]),
    "csp_minsnap_periodic_timeopt_workspace_bytes": (_SZ, [_D]),
    "csp_minsnap_eval_batch": (_I, [_D, _P, _P, _P, _I64, _I32, _P, _P, _P, _P]),
    "csp_minsnap_eval_batch_vjp": (_I, [_D, _P, _P, _P, _I64, _I32, _P, _P, _P, _P, _P, _P]),
    "csp_minsnap_solve_multi": (_I, [_D, _I] + [_P] * 7),
    "csp_minsnap_solve_mixed": (_I, [_D] + [_P] * 8 + [_SZ, _P]),
    "csp_minsnap_mixed_workspace_bytes": (_SZ, [_D]),
    "csp_minsnap_time_alloc_batch": (_I, [_D, _P, _F, _F, _P, _P]),
    "csp_minsnap_plan_batch": (_I, [_D, _P, _F, _F] + [_P] * 8 + [_SZ, _P]),
    "csp_minsnap_plan_workspace_bytes": (_SZ, [_D]),
    "csp_minsnap_sample_batch": (_I, [_D, _P, _P, _F, _I64, _P, _P, _P, _P]),
    "csp_minsnap_generate_batch": (_I, [_D, _P, _F, _F, _P, _F, _I64] + [_P] * 10 + [_SZ, _P]),
    "csp_minsnap_sample_capacity": (_I64, [_D, _P, _F, _F]),
    "csp_minsnap_kernel_name": (_S, [_D]),
    "csp_minsnap_device_count": (_I, None),
    "csp_minsnap_version": (_S, None),
    "csp_minsnap_strerror": (_S, [_I]),
    "csp_minsnap_last_hip_error": (_S, None),
    "csp_minsnap_release_cached_memory": (None, None),
    "csp_geo_wgs84_to_enu_batch": (_I, [_P, _P, _P, _I64, _U32, _I32, _P]),
    "csp_geo_enu_to_wgs84_batch": (_I, [_P, _P, _P, _I64, _U32, _I32, _P]),
    "csp_alt_workspace_bytes": (_SZ, [_I64]),
    "csp_alt_optimize_heights_batch": (_I, [_P, _P, _P, _I64, _ALT, _P, _P, _SZ, _U32, _I32, _P]),
    "csp_alt_global_smooth_batch": (_I, [_P, _P, _P, _I64, _ALT, _P, _P, _P, _SZ, _U32, _I32, _P]),
    "csp_bezier_generate_batch": (_I, [_P, _P, _I64, _F, _F, _I64, _P, _P, _U32, _I32, _P]),
}
for _n, (_r, _a) in _PROTOTYPES.items():
    getattr(_lib, _n).restype = _r
    if _a is not None:
        getattr(_lib, _n).argtypes = _a


def release_cached_memory():
    """Frees the idle staging arenas host-memory calls keep between calls (include/csp_minsnap.h)."""
    _lib.csp_minsnap_release_cached_memory()


def raw_lib():
    return _lib


def version():
    return _lib.csp_minsnap_version().decode()


def strerror(code):
    return _lib.csp_minsnap_strerror(int(code)).decode()


def device_count():
    return int(_lib.csp_minsnap_device_count())


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def make_desc(order, batch, num_segments=0, dtype=DTYPE_F64, path_weight=0.0, vel_zero_weight=0.0,
              mem_space=MEM_HOST, bc_per_trajectory=False, seg_offsets_ptr=None, max_segments=0,
              vw_per_ptr=None, device_id=-1, flags=0):
    d = Desc()
    d.abi_version = ABI_VERSION
    d.dtype = dtype
    d.order = int(order)
    d.num_segments = int(num_segments)
    d.batch = int(batch)
    d.seg_offsets = seg_offsets_ptr
    d.max_segments = int(max_segments)
    d.bc_per_trajectory = 1 if bc_per_trajectory else 0
    d.path_weight = float(path_weight)
    d.vel_zero_weight = float(vel_zero_weight)
    d.vel_zero_weight_per_traj = vw_per_ptr
    d.mem_space = mem_space
    d.device_id = int(device_id)
    d.flags = int(flags)
    d.reserved = 0
    return d


def _flags(force_generic=False, segment_major=False, no_persistent=False, f32_arith=False, long_segments=False, span=False):
    return ((FLAG_FORCE_GENERIC if force_generic else 0) | (FLAG_SEGMENT_MAJOR if segment_major else 0)
            | (FLAG_NO_PERSISTENT if no_persistent else 0) | (FLAG_F32_ARITH if f32_arith else 0)
            | (FLAG_LONG_SEGMENTS if long_segments else 0) | (FLAG_SPAN if span else 0))


def workspace_bytes(desc):
    return int(_lib.csp_minsnap_workspace_bytes(ctypes.byref(desc)))


def kernel_name(desc):
    r = _lib.csp_minsnap_kernel_name(ctypes.byref(desc))
    return r.decode() if r else None


def _check(rc):
    if rc != 0:
        raise CspError(rc, _lib.csp_minsnap_last_hip_error().decode() if rc == -4 or rc == -5 else "")


# ---- the inputs of a call, in the memory space they arrived in ----
# A backend is that memory space: numpy arrays -> CSP_MEM_HOST, torch CUDA tensors -> CSP_MEM_DEVICE.  Element kinds are named
# "f32" / "f64" (kind() of the array that sets the storage dtype), "i32", "i64", "u8"; every entry point below is written
# once against the backend's contig / ptr / empty / zeros / workspace / stream / sync, mem_space and device_id.

_DTYPE_NAME = {"f32": "float32", "f64": "float64", "i32": "int32", "i64": "int64", "u8": "uint8"}
_NP_DTYPE = {k: np.dtype(v) for k, v in _DTYPE_NAME.items()}
_TORCH_DTYPE = {} if torch is None else {k: getattr(torch, v) for k, v in _DTYPE_NAME.items()}


class _HostMem:
    """numpy arrays.  The library stages host-memory calls itself: they take no workspace and no stream."""
    mem_space, device_id = MEM_HOST, -1

    def kind(self, x):
        return "f32" if (x if isinstance(x, np.ndarray) else np.asarray(x)).dtype == np.float32 else "f64"

    def contig(self, x, kind):
        return np.ascontiguousarray(x, dtype=_NP_DTYPE[kind])

    addr = staticmethod(operator.attrgetter("ctypes.data"))   # of an array that is there; ptr() also takes None

    def ptr(self, a):
        return a.ctypes.data if a is not None else None

    def empty(self, shape, kind):
        return np.empty(shape, dtype=_NP_DTYPE[kind])

    def zeros(self, shape, kind):
        return np.zeros(shape, dtype=_NP_DTYPE[kind])

    def workspace(self, need, given=None):
        return None, 0

    def stream(self, given=None):
        return None

    def sync(self):
        pass


_HOST = _HostMem()


class _DeviceMem:
    """torch CUDA tensors on the device of `like`; calls are enqueued on the caller's stream or torch's current one."""
    mem_space = MEM_DEVICE

    def __init__(self, like):
        if not like.is_cuda:
            raise ValueError("torch inputs must be CUDA tensors (use numpy arrays for host memory)")
        self.dev = like.device
        self.device_id = self.dev.index if self.dev.index is not None else -1

    def kind(self, x):
        return "f32" if x.dtype == torch.float32 else "f64"

    def contig(self, x, kind):
        dt = _TORCH_DTYPE[kind]
        if x.dtype != dt or x.device != self.dev:
            x = x.to(device=self.dev, dtype=dt)
        return x.contiguous()

    addr = staticmethod(operator.methodcaller("data_ptr"))

    def ptr(self, t):
        return t.data_ptr() if t is not None else None

    def empty(self, shape, kind):
        return torch.empty(shape, dtype=_TORCH_DTYPE[kind], device=self.dev)

    def zeros(self, shape, kind):
        return torch.zeros(shape, dtype=_TORCH_DTYPE[kind], device=self.dev)

    def workspace(self, need, given=None):
        """(pointer, bytes) of `need` bytes: the caller's `given` when it is large enough, else a new allocation, which
        lives as long as this object."""
        if not need:
            return None, 0
        if given is None or given.numel() * given.element_size() < need:
            given = self._ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        return given.data_ptr(), need

    def stream(self, given=None):
        return ctypes.c_void_p(given if given is not None else torch.cuda.current_stream(self.dev).cuda_stream)

    def sync(self):
        torch.cuda.current_stream(self.dev).synchronize()


def _mem(x):
    return _DeviceMem(x) if type(x).__module__.startswith("torch") else _HOST


def _dtype_code(kind):
    return DTYPE_F32 if kind == "f32" else DTYPE_F64


def _ragged_dims(mem, seg_offsets, times, max_segments):
    """(seg_offsets as contiguous int64 or None, B, S, segments in total, max_segments) of uniform times [B,S], or of
    ragged times [sum S_b] with seg_offsets [B+1] (S = 0; max_segments taken from the offsets when not given)."""
    if seg_offsets is None:
        B, S = times.shape
        return None, B, S, B * S, max_segments
    off = mem.contig(seg_offsets, "i64")
    B = off.shape[0] - 1
    if max_segments is None:
        max_segments = int((off[1:] - off[:-1]).max()) if B else 1
    return off, B, 0, math.prod(times.shape), max_segments


def _bc_block(mem, bc, kind):
    """bc as [rows,4,3] in the storage dtype; None = one shared row block of zeros."""
    return mem.zeros((1, 4, 3), kind) if bc is None else mem.contig(bc, kind).reshape(-1, 4, 3)


def _workspace(mem, given, size_fn, *size_args):
    """(pointer, bytes) of a call's workspace, the caller's `given` where it is large enough.  Only device-memory calls
    take one, and only they ask for its size."""
    if mem.mem_space == MEM_HOST:
        return None, 0
    return mem.workspace(size_fn(*size_args), given)


def _scratch(mem, size_fn, *size_args):
    """(pointer, bytes) of the workspace of an entry that takes none from its caller (plan, generate, altitude): a device
    call gets a pointer that is never null, whatever size the library asks for."""
    if mem.mem_space == MEM_HOST:
        return None, 0
    need = size_fn(*size_args)
    return mem.workspace(max(need, 1))[0], need


class _CallInputs:
    """waypoints / times / bc / seg_offsets / per-trajectory weights of one call, made contiguous in the memory space
    they came in.  Whether bc rows are per trajectory, and whether their count is checked, is the entry's choice."""

    def __init__(self, waypoints, times, bc=None, seg_offsets=None, max_segments=None, vel_zero_weight_per_traj=None):
        self.mem = mem = _mem(waypoints)
        self.io = io = mem.kind(waypoints)
        self.waypoints, self.times = mem.contig(waypoints, io), mem.contig(times, io)
        self.seg_offsets, self.B, self.S, self.total, self.max_segments = _ragged_dims(mem, seg_offsets, self.times, max_segments)
        self.bc = _bc_block(mem, bc, io)
        self.vwp = None if vel_zero_weight_per_traj is None else mem.contig(vel_zero_weight_per_traj, "f64")

    def checked_bc_per_trajectory(self):
        if self.bc.shape[0] not in (1, self.B):
            raise ValueError("bc must be [4,3], [1,4,3] or [B,4,3]")
        return self.bc.shape[0] == self.B

    def desc(self, order, bc_per_trajectory, path_weight=0.0, vel_zero_weight=0.0, flags=0):
        mem = self.mem
        return make_desc(order, self.B, self.S, _dtype_code(self.io), path_weight, vel_zero_weight, mem.mem_space,
                         bc_per_trajectory, mem.ptr(self.seg_offsets), self.max_segments or 0, mem.ptr(self.vwp),
                         mem.device_id, flags)

    def coeffs_shape(self, order, segment_major=False):
        m = 2 * int(order)
        if self.seg_offsets is not None:
            return (self.total, 3, m)
        return (self.S, self.B, 3, m) if segment_major else (self.B, self.S, 3, m)


def _cotangents(ci, grad_coeffs, grad_cost, order):
    """(grad_coeffs in the storage dtype, grad_cost as f64) of a reverse-mode call on `ci`, contiguous and checked against
    its sizes.  One that is None stays None: which of the two may be is the entry's choice."""
    mem = ci.mem
    gco = gj = None
    if grad_coeffs is not None:
        gco = mem.contig(grad_coeffs, ci.io)
        if mem.mem_space == MEM_DEVICE and gco.data_ptr() % 16:   # the kernel reads it in 16-byte pieces (host memory is staged)
            gco = gco.clone()
        n = ci.total * 3 * 2 * int(order)
        if math.prod(gco.shape) != n:
            raise ValueError("grad_coeffs must hold %d elements (the coefficients' layout)" % n)
    if grad_cost is not None:
        gj = mem.contig(grad_cost, "f64")
        if math.prod(gj.shape) != ci.B:
            raise ValueError("grad_cost must hold %d elements (one per trajectory)" % ci.B)
    return gco, gj


def _wanted(mem, want, names, like, kind):
    """Checks `want` against the family's `names`; then one uninitialised gradient array per name, in the family's order
    and shaped as the input in `like`, None where the name is not wanted."""
    want = tuple(want)
    for w in want:
        if w not in names:
            raise ValueError("want: a subset of %r" % (names,))
    return [mem.empty(x.shape, kind) if name in want else None for name, x in zip(names, like)]


class Result:
    __slots__ = ("coeffs", "max_dev", "status", "kernel")

    def __init__(self, coeffs, max_dev, status, kernel):
        self.coeffs, self.max_dev, self.status, self.kernel = coeffs, max_dev, status, kernel


def solve_batch(waypoints, times, bc=None, order=4, path_weight=0.0, vel_zero_weight=0.0,
                seg_offsets=None, max_segments=None, vel_zero_weight_per_traj=None,
                want_max_dev=False, want_status=False, out=None, workspace=None, stream=None, ngpu=None,
                force_generic=False, segment_major=False, no_persistent=False, f32_arith=False, span=False):
    """Batched SolveQPClosedForm (math_util/minimum_snap.hpp:45-53).

    numpy inputs  -> CSP_MEM_HOST (staged through the device, synchronous);
    torch CUDA tensors -> CSP_MEM_DEVICE (enqueued on `stream` or torch's current stream).
    Uniform batches: waypoints [B,S+1,3], times [B,S]; ragged: pass seg_offsets [B+1] (int64)
    with concatenated waypoints [sum(S_b+1),3] and times [sum S_b].
    bc: [4,3] / [1,4,3] shared or [B,4,3] per trajectory; rows start vel, end vel, start acc,
    end acc (reference Vel/Acc); None = zeros (MinimumSnapConfig defaults, minimum_snap.hpp:29-32).
    ngpu: csp_minsnap_solve_batch_sharded, synchronous, from this one process -- a host batch cut into contiguous chunks
    over `ngpu` devices, a device batch scattered from / gathered to its (root) device over RCCL.
    Returns Result(coeffs [B,S,3,2o] (ragged: [sum S_b,3,2o]), max_dev, status, kernel name).
    """
    if segment_major and seg_offsets is not None:
        raise ValueError("segment_major needs a uniform batch")
    ci = _CallInputs(waypoints, times, bc, seg_offsets, max_segments, vel_zero_weight_per_traj)
    mem, p = ci.mem, ci.mem.ptr
    desc = ci.desc(order, ci.checked_bc_per_trajectory(), path_weight, vel_zero_weight,
                   _flags(force_generic, segment_major, no_persistent, f32_arith, span=span))
    if out is None:
        out = mem.empty(ci.coeffs_shape(order, segment_major), ci.io)
    md = mem.empty((ci.B,), "f64") if want_max_dev else None
    stt = mem.empty((ci.B,), "i32") if want_status else None
    wsp, need = _workspace(mem, workspace, workspace_bytes, desc)
    args = (ctypes.byref(desc), p(ci.waypoints), p(ci.times), p(ci.bc), p(out), p(md), p(stt))
    if ngpu is not None:
        _check(_lib.csp_minsnap_solve_batch_sharded(*args, int(ngpu)))
    else:
        _check(_lib.csp_minsnap_solve_batch(*args, wsp, need, mem.stream(stream)))
    return Result(out, md, stt, kernel_name(desc))


def vjp_workspace_bytes(desc):
    return int(_lib.csp_minsnap_vjp_workspace_bytes(ctypes.byref(desc)))


def cost_vjp_workspace_bytes(desc, with_grad_coeffs=True):
    return int(_lib.csp_minsnap_cost_vjp_workspace_bytes(ctypes.byref(desc), 1 if with_grad_coeffs else 0))


class VjpResult:
    """Gradients of solve_batch_vjp; a gradient that was not asked for is None."""
    __slots__ = ("waypoints", "times", "bc", "status")

    def __init__(self, waypoints, times, bc, status):
        self.waypoints, self.times, self.bc, self.status = waypoints, times, bc, status


_VJP_WANT = ("waypoints", "times", "bc")


def solve_batch_vjp(waypoints, times, grad_coeffs, bc=None, order=4, vel_zero_weight=0.0, seg_offsets=None,
                    max_segments=None, vel_zero_weight_per_traj=None, want=_VJP_WANT, want_status=False,
                    workspace=None, stream=None, grad_cost=None):
    """Vector-Jacobian product of solve_batch (csp_minsnap_solve_batch_vjp): given grad_coeffs = dL/dcoeffs in the layout
    of solve_batch's coefficients, returns VjpResult(dL/dwaypoints, dL/dtimes, dL/dbc, status) for the names in `want`.
    Inputs as in solve_batch (no path penalty): numpy arrays -> CSP_MEM_HOST, torch CUDA tensors -> CSP_MEM_DEVICE.
    dL/dbc has the shape of bc after reshaping to [-1,4,3]: [1,4,3] summed over the batch, or [B,4,3]; bc=None is
    treated as a shared zero bc.
    grad_cost = dL/dcost [B] (the cost of snap_cost_batch at the same inputs) adds the cost's cotangent
    (csp_minsnap_solve_batch_cost_vjp); grad_coeffs may then be None: the cost-only kernel, which needs
    no adjoint solve and reads no coefficient cotangent."""
    ci = _CallInputs(waypoints, times, bc, seg_offsets, max_segments, vel_zero_weight_per_traj)
    mem, p = ci.mem, ci.mem.ptr
    if grad_coeffs is None and grad_cost is None:
        raise ValueError("grad_coeffs may be None only with a grad_cost")
    gco, gj = _cotangents(ci, grad_coeffs, grad_cost, order)
    # B == 1 counts as per trajectory here: the library sizes the workspace and picks the bc reduction from this flag
    desc = ci.desc(order, ci.checked_bc_per_trajectory(), 0.0, vel_zero_weight)
    gwp, gtm, gbc = _wanted(mem, want, _VJP_WANT, (ci.waypoints, ci.times, ci.bc), ci.io)
    stt = mem.empty((ci.B,), "i32") if want_status else None
    if gj is None:
        wsp, need = _workspace(mem, workspace, vjp_workspace_bytes, desc)
        _check(_lib.csp_minsnap_solve_batch_vjp(ctypes.byref(desc), p(ci.waypoints), p(ci.times), p(ci.bc), p(gco), p(gwp),
                                                p(gtm), p(gbc), p(stt), wsp, need, mem.stream(stream)))
    else:
        wsp, need = _workspace(mem, workspace, cost_vjp_workspace_bytes, desc, gco is not None)
        _check(_lib.csp_minsnap_solve_batch_cost_vjp(ctypes.byref(desc), p(ci.waypoints), p(ci.times), p(ci.bc), p(gco), p(gj),
                                                     p(gwp), p(gtm), p(gbc), p(stt), wsp, need, mem.stream(stream)))
    return VjpResult(gwp, gtm, gbc, stt)


_autograd_fns = {}


def _autograd_fn(names, forward, vjp):
    """The torch.autograd.Function of one family, built at first use.  apply() takes the family's differentiable inputs
    (`names`, in the order of its VJP's `want`), then whatever else `forward` and `vjp` take.  forward(*args) returns
    the outputs; backward makes one call, vjp(want, grad_coeffs, grad_cost, *args), for the inputs that need a gradient,
    and hands each back in its input's shape and dtype."""
    if forward in _autograd_fns:
        return _autograd_fns[forward]
    from torch.autograd.function import once_differentiable
    n = len(names)

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, *args):
            ctx.save_for_backward(*args[:n])
            ctx.rest = args[n:]
            ctx.set_materialize_grads(False)   # an output the loss does not use arrives as None, not as zeros
            return forward(*(x if x is None else x.detach() for x in args[:n]), *args[n:])

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_coeffs, grad_cost=None):
            xs, needs = ctx.saved_tensors, ctx.needs_input_grad[:n]
            want = tuple(k for k, f in zip(names, needs) if f)
            if not want or (grad_coeffs is None and grad_cost is None):
                return (None,) * (n + len(ctx.rest))
            g = vjp(want, grad_coeffs, grad_cost, *xs, *ctx.rest)
            return tuple(getattr(g, k).reshape(x.shape).to(x.dtype) if f else None
                         for k, x, f in zip(names, xs, needs)) + (None,) * len(ctx.rest)

    _autograd_fns[forward] = Fn
    return Fn


def _solve_kw(order, vel_zero_weight, seg_offsets, max_segments, vel_zero_weight_per_traj):
    """The keywords every solve family's forward and VJP take alike."""
    return dict(order=order, vel_zero_weight=vel_zero_weight, seg_offsets=seg_offsets, max_segments=max_segments,
                vel_zero_weight_per_traj=vel_zero_weight_per_traj)


def _solve_forward(wp, tm, bc, with_cost, kw):
    r = solve_batch(wp, tm, bc, **kw)
    return (r.coeffs, snap_cost_batch(wp, tm, bc, want_grad=False, **kw).cost) if with_cost else r.coeffs


def _solve_vjp(want, grad_coeffs, grad_cost, wp, tm, bc, with_cost, kw):
    ckw = {} if grad_cost is None else {"grad_cost": grad_cost}   # the cost alone: grad_coeffs stays None
    return solve_batch_vjp(wp, tm, grad_coeffs, bc=bc, want=want, **kw, **ckw)


def solve_batch_autograd(waypoints, times, bc=None, order=4, vel_zero_weight=0.0, seg_offsets=None, max_segments=None,
                         vel_zero_weight_per_traj=None, with_cost=False):
    """solve_batch as a differentiable torch op (CUDA tensors): returns the coefficients -- bit-equal to
    solve_batch(...).coeffs -- with a grad_fn when waypoints, times or bc require grad.  The backward pass is
    csp_minsnap_solve_batch_vjp for the inputs that need a gradient; it is first-order only (once_differentiable).
    No path penalty; no gradient with respect to the weights.
    with_cost: returns (coeffs, cost), the cost bit-equal to snap_cost_batch(...).cost.  The backward pass is then one
    csp_minsnap_solve_batch_cost_vjp with the cotangents that arrived; a loss on the cost alone runs the cost-only
    kernel (no adjoint solve, no zero coefficient cotangent is allocated)."""
    kw = _solve_kw(order, vel_zero_weight, seg_offsets, max_segments, vel_zero_weight_per_traj)
    return _autograd_fn(_VJP_WANT, _solve_forward, _solve_vjp).apply(waypoints, times, bc, with_cost, kw)


def cost_workspace_bytes(desc):
    return int(_lib.csp_minsnap_cost_workspace_bytes(ctypes.byref(desc)))


def timeopt_workspace_bytes(desc):
    return int(_lib.csp_minsnap_timeopt_workspace_bytes(ctypes.byref(desc)))


class CostResult:
    """snap_cost_batch: cost [B] f64, grad_times (layout of times, or None), status [B] i32."""
    __slots__ = ("cost", "grad_times", "status")

    def __init__(self, cost, grad_times, status):
        self.cost, self.grad_times, self.status = cost, grad_times, status


def snap_cost_batch(waypoints, times, bc=None, order=4, vel_zero_weight=0.0, seg_offsets=None, max_segments=None,
                    vel_zero_weight_per_traj=None, want_grad=True, workspace=None, stream=None):
    """The cost J the solve minimises at `times` and its gradient dJ/dtimes (csp_minsnap_cost_batch).
    Inputs as in solve_batch without the path penalty: numpy arrays -> host memory, torch CUDA tensors -> device memory
    (asynchronous on the current stream)."""
    ci = _CallInputs(waypoints, times, bc, seg_offsets, max_segments, vel_zero_weight_per_traj)
    mem, p = ci.mem, ci.mem.ptr
    desc = ci.desc(order, ci.checked_bc_per_trajectory(), 0.0, vel_zero_weight)
    cost = mem.empty((ci.B,), "f64")
    grad = mem.empty(ci.times.shape, ci.io) if want_grad else None
    stt = mem.empty((ci.B,), "i32")
    wsp, need = mem.workspace(cost_workspace_bytes(desc), workspace)
    _check(_lib.csp_minsnap_cost_batch(ctypes.byref(desc), p(ci.waypoints), p(ci.times), p(ci.bc), p(cost), p(grad), p(stt),
                                       wsp, need, mem.stream(stream)))
    return CostResult(cost, grad, stt)


class TimeOptResult:
    """optimize_times_batch: times (layout of the input), coeffs (or None), objective [B,2] f64 (initial, final),
    iterations [B] i32, status [B] i32."""
    __slots__ = ("times", "coeffs", "objective", "iterations", "status")

    def __init__(self, times, coeffs, objective, iterations, status):
        self.times, self.coeffs, self.objective, self.iterations, self.status = times, coeffs, objective, iterations, status


_TIMEOPT_MODES = {"fixed_total": TIMEOPT_FIXED_TOTAL, "time_penalty": TIMEOPT_TIME_PENALTY}


def optimize_times_batch(waypoints, times, bc=None, order=4, mode="fixed_total", time_weight=0.0, min_time=0.01, tol=1e-6,
                         max_iters=100, want_coeffs=True, vel_zero_weight=0.0, seg_offsets=None, max_segments=None,
                         vel_zero_weight_per_traj=None, workspace=None, stream=None):
    """Segment times that minimise the snap cost (csp_minsnap_optimize_times_batch), per trajectory in one
    launch.  mode "fixed_total": minimise J with sum(T) kept; "time_penalty": minimise J + time_weight * sum(T).
    T >= min_time throughout.  Stops when the scaled projected-gradient measure is <= tol, or after max_iters accepted
    iterations (status TRAJ_NOT_CONVERGED).  coeffs, when wanted, are solve_batch's at the returned times (bit-equal).
    Inputs as in snap_cost_batch."""
    if mode not in _TIMEOPT_MODES:
        raise ValueError("mode: one of %r" % (tuple(_TIMEOPT_MODES),))
    ci = _CallInputs(waypoints, times, bc, seg_offsets, max_segments, vel_zero_weight_per_traj)
    mem, p = ci.mem, ci.mem.ptr
    desc = ci.desc(order, ci.checked_bc_per_trajectory(), 0.0, vel_zero_weight)
    prm = make_timeopt_params(_TIMEOPT_MODES[mode], time_weight, min_time, tol, max_iters)
    tout = mem.empty(ci.times.shape, ci.io)
    co = mem.empty(ci.coeffs_shape(order), ci.io) if want_coeffs else None
    obj = mem.empty((ci.B, 2), "f64")
    its = mem.empty((ci.B,), "i32")
    stt = mem.empty((ci.B,), "i32")
    wsp, need = mem.workspace(timeopt_workspace_bytes(desc), workspace)
    _check(_lib.csp_minsnap_optimize_times_batch(ctypes.byref(desc), ctypes.byref(prm), p(ci.waypoints), p(ci.times),
                                                 p(ci.bc), p(tout), p(co), p(obj), p(its), p(stt), wsp, need,
                                                 mem.stream(stream)))
    return TimeOptResult(tout, co, obj, its, stt)


def periodic_workspace_bytes(desc):
    return int(_lib.csp_minsnap_periodic_workspace_bytes(ctypes.byref(desc)))


class PeriodicResult:
    """solve_periodic_batch: coeffs ([B,S,3,2o], or [sum S_b,3,2o] ragged), cost [B] f64 (or None), grad_times (layout
    of times, or None), status [B] i32."""
    __slots__ = ("coeffs", "cost", "grad_times", "status")

    def __init__(self, coeffs, cost, grad_times, status):
        self.coeffs, self.cost, self.grad_times, self.status = coeffs, cost, grad_times, status


def solve_periodic_batch(waypoints, times, order=4, vel_zero_weight=0.0, seg_offsets=None, max_segments=None,
                         vel_zero_weight_per_traj=None, want_cost=False, want_grad=False, workspace=None, stream=None):
    """The periodic (closed-loop) minimum-snap solve (csp_minsnap_solve_periodic_batch): segment j runs
    from waypoint j to waypoint (j+1) mod S, every knot is interior and there is no bc.  waypoints [B,S,3] (no repeated
    closing point), times [B,S]; ragged: waypoints [sum S_b,3] and times [sum S_b], both split by seg_offsets [B+1].
    numpy arrays -> host memory, torch CUDA tensors -> device memory (asynchronous on the current stream).  want_cost /
    want_grad add the snap cost J and dJ/dtimes; the coefficients are the same bits either way."""
    ci = _CallInputs(waypoints, times, None, seg_offsets, max_segments, vel_zero_weight_per_traj)
    mem, p = ci.mem, ci.mem.ptr
    desc = ci.desc(order, ci.checked_bc_per_trajectory(), 0.0, vel_zero_weight)
    co = mem.empty(ci.coeffs_shape(order), ci.io)
    cost = mem.empty((ci.B,), "f64") if want_cost else None
    grad = mem.empty(ci.times.shape, ci.io) if want_grad else None
    stt = mem.empty((ci.B,), "i32")
    wsp, need = mem.workspace(periodic_workspace_bytes(desc), workspace)
    _check(_lib.csp_minsnap_solve_periodic_batch(ctypes.byref(desc), p(ci.waypoints), p(ci.times), p(co), p(cost),
                                                 p(grad), p(stt), wsp, need, mem.stream(stream)))
    return PeriodicResult(co, cost, grad, stt)


def periodic_vjp_workspace_bytes(desc):
    return int(_lib.csp_minsnap_periodic_vjp_workspace_bytes(ctypes.byref(desc)))


class PeriodicVjpResult:
    """Gradients of solve_periodic_batch_vjp; a gradient that was not asked for is None."""
    __slots__ = ("waypoints", "times", "status")

    def __init__(self, waypoints, times, status):
        self.waypoints, self.times, self.status = waypoints, times, status


_PERIODIC_VJP_WANT = ("waypoints", "times")


def solve_periodic_batch_vjp(waypoints, times, grad_coeffs, grad_cost=None, order=4, vel_zero_weight=0.0, seg_offsets=None,
                             max_segments=None, vel_zero_weight_per_traj=None, want=_PERIODIC_VJP_WANT, want_status=False,
                             workspace=None, stream=None):
    """Vector-Jacobian product of solve_periodic_batch (csp_minsnap_solve_periodic_batch_vjp): given
    grad_coeffs = dL/dcoeffs in the layout of that call's coefficients and, optionally, grad_cost = dL/dcost [B], returns
    PeriodicVjpResult(dL/dwaypoints, dL/dtimes, status) for the names in `want`.  Inputs as in solve_periodic_batch:
    numpy arrays -> CSP_MEM_HOST, torch CUDA tensors -> CSP_MEM_DEVICE."""
    ci = _CallInputs(waypoints, times, None, seg_offsets, max_segments, vel_zero_weight_per_traj)
    mem, p = ci.mem, ci.mem.ptr
    gco, gj = _cotangents(ci, grad_coeffs, grad_cost, order)   # (the library refuses a null grad_coeffs)
    desc = ci.desc(order, ci.checked_bc_per_trajectory(), 0.0, vel_zero_weight)
    gwp, gtm = _wanted(mem, want, _PERIODIC_VJP_WANT, (ci.waypoints, ci.times), ci.io)
    stt = mem.empty((ci.B,), "i32") if want_status else None
    wsp, need = _workspace(mem, workspace, periodic_vjp_workspace_bytes, desc)
    _check(_lib.csp_minsnap_solve_periodic_batch_vjp(ctypes.byref(desc), p(ci.waypoints), p(ci.times), p(gco), p(gj), p(gwp),
                                                     p(gtm), p(stt), wsp, need, mem.stream(stream)))
    return PeriodicVjpResult(gwp, gtm, stt)


def knots_workspace_bytes(desc):
    return int(_lib.csp_minsnap_knots_workspace_bytes(ctypes.byref(desc)))


class KnotsResult:
    """solve_knots_batch: coeffs ([B,S,3,2o], or [sum S_b,3,2o] ragged), status [B] i32, cost [B] f64 (or None)."""
    __slots__ = ("coeffs", "status", "cost")

    def __init__(self, coeffs, status, cost):
        self.coeffs, self.status, self.cost = coeffs, status, cost


def knots_from_bc(bc, num_segments, order, batch=None):
    """(knot_mask, knot_values) of the standard problem of solve_batch for solve_knots_batch: both end knots carry every
    bit below order-1 (velocity and acceleration from bc, higher derivatives 0), every interior knot is free.
    bc: [4,3] / [1,4,3] shared (then `batch` trajectories, default 1) or [B,4,3]; None = zeros.  Rows: start vel, end vel,
    start acc, end acc.  Returns numpy arrays: mask [B,S+1] uint8, values [B,S+1,order-1,3] in bc's dtype (float64 unless
    bc is float32).  A ragged batch is built per trajectory and concatenated along the knot axis."""
    order, S = int(order), int(num_segments)
    if order < 2 or S < 1:
        raise ValueError("knots_from_bc needs order >= 2 and num_segments >= 1")
    if bc is None:
        bc = np.zeros((1, 4, 3))
    if _is_torch(bc):
        bc = bc.detach().cpu().numpy()
    bc = np.asarray(bc)
    bc = bc.astype(np.float32 if bc.dtype == np.float32 else np.float64, copy=False).reshape(-1, 4, 3)
    B = int(batch) if batch is not None else bc.shape[0]
    if bc.shape[0] not in (1, B):
        raise ValueError("bc must be [4,3], [1,4,3] or [B,4,3]")
    n = order - 1
    mask = np.zeros((B, S + 1), np.uint8)
    mask[:, 0] = mask[:, S] = (1 << n) - 1
    values = np.zeros((B, S + 1, n, 3), bc.dtype)
    values[:, 0, 0], values[:, S, 0] = bc[:, 0], bc[:, 1]
    if n > 1:
        values[:, 0, 1], values[:, S, 1] = bc[:, 2], bc[:, 3]
    return mask, values


def _knot_arrays(ci, knot_mask, knot_values, order):
    """knot_mask / knot_values of a knots call, contiguous in the call's memory space and checked against its knots."""
    mem = ci.mem
    n = int(order) - 1
    knots = ci.total + ci.B
    if mem.mem_space == MEM_DEVICE:   # knots_from_bc returns numpy arrays: they may be passed beside device waypoints
        knot_mask, knot_values = (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
                                  for a in (knot_mask, knot_values))
    mk, kv = mem.contig(knot_mask, "u8"), mem.contig(knot_values, ci.io)
    if math.prod(mk.shape) != knots:
        raise ValueError("knot_mask must hold %d elements (one per waypoint)" % knots)
    if math.prod(kv.shape) != knots * n * 3:
        raise ValueError("knot_values must hold %d elements ([knots][order-1][3])" % (knots * n * 3))
    return mk, kv


def solve_knots_batch(waypoints, times, knot_mask, knot_values, order=4, vel_zero_weight=0.0, seg_offsets=None,
                      max_segments=None, want_cost=False, workspace=None, stream=None, vel_zero_weight_per_traj=None):
    """The open-chain minimum-snap solve with per-knot derivative constraints (csp_minsnap_solve_knots_batch, DESIGN.md
    §20).  Positions are fixed at every waypoint; knot_mask [B,S+1] uint8 says per knot (waypoint) which derivatives are
    fixed: bit r set = derivative r+1 equals knot_values[b,k,r,:] ([B,S+1,order-1,3], the storage dtype of waypoints), bit
    clear = free, chosen by the solve (the entry is then never read).  A free end is an end knot with mask 0; the
    standard problem's mask is knots_from_bc's.  Ragged: waypoints [sum(S_b+1),3], times [sum S_b], knot_mask
    [sum(S_b+1)] and knot_values [sum(S_b+1),order-1,3] with seg_offsets [B+1].
    numpy arrays -> host memory, torch CUDA tensors -> device memory (asynchronous on the current stream); beside device
    waypoints, knot_mask and knot_values may be numpy arrays (knots_from_bc's) and are copied to the device.
    Returns KnotsResult(coeffs, status, cost): the coefficients have solve_batch's trajectory-major layout, so
    eval_batch, sample_batch and every other consumer of solve_batch's coefficients read them unchanged.  A trajectory
    with fewer constraints (its S+1 positions plus its set mask bits) than `order` has no unique minimiser: status
    TRAJ_NOT_SPD, NaN coefficients and cost.  want_cost adds the snap cost J of snap_cost_batch at the optimum."""
    ci = _CallInputs(waypoints, times, None, seg_offsets, max_segments, vel_zero_weight_per_traj)
    mem, p = ci.mem, ci.mem.ptr
    mk, kv = _knot_arrays(ci, knot_mask, knot_values, order)
    desc = ci.desc(order, False, 0.0, vel_zero_weight)
    co = mem.empty(ci.coeffs_shape(order), ci.io)
    cost = mem.empty((ci.B,), "f64") if want_cost else None
    stt = mem.empty((ci.B,), "i32")
    wsp, need = mem.workspace(knots_workspace_bytes(desc), workspace)
    _check(_lib.csp_minsnap_solve_knots_batch(ctypes.byref(desc), p(ci.waypoints), p(ci.times), p(mk), p(kv), p(co), p(cost),
                                              p(stt), wsp, need, mem.stream(stream)))
    return KnotsResult(co, stt, cost)


def knots_vjp_workspace_bytes(desc, with_grad_coeffs=True):
    return int(_lib.csp_minsnap_knots_vjp_workspace_bytes(ctypes.byref(desc), 1 if with_grad_coeffs else 0))


class KnotsVjpResult:
    """Gradients of solve_knots_batch_vjp; a gradient that was not asked for is None."""
    __slots__ = ("waypoints", "times", "knot_values", "status")

    def __init__(self, waypoints, times, knot_values, status):
        self.waypoints, self.times, self.knot_values, self.status = waypoints, times, knot_values, status


_KNOTS_VJP_WANT = ("waypoints", "times", "knot_values")


def solve_knots_batch_vjp(waypoints, times, knot_mask, knot_values, grad_coeffs=None, grad_cost=None, order=4,
                          vel_zero_weight=0.0, seg_offsets=None, max_segments=None, vel_zero_weight_per_traj=None,
                          want=_KNOTS_VJP_WANT, want_status=False, workspace=None, stream=None):
    """Vector-Jacobian product of solve_knots_batch (csp_minsnap_solve_knots_batch_vjp): given grad_coeffs
    = dL/dcoeffs in the layout of that call's coefficients and / or grad_cost = dL/dcost [B] (at least one), returns
    KnotsVjpResult(dL/dwaypoints, dL/dtimes, dL/dknot_values, status) for the names in `want`.  dL/dknot_values is exactly
    0.0 at every slot whose mask bit is clear.  Without grad_coeffs the three-column kernel runs and grad_coeffs is never
    allocated or read.  Inputs as in solve_knots_batch: numpy arrays -> CSP_MEM_HOST, torch CUDA tensors ->
    CSP_MEM_DEVICE (knot_mask and knot_values may be numpy arrays beside device waypoints)."""
    if grad_coeffs is None and grad_cost is None:
        raise ValueError("solve_knots_batch_vjp needs grad_coeffs, grad_cost or both")
    ci = _CallInputs(waypoints, times, None, seg_offsets, max_segments, vel_zero_weight_per_traj)
    mem, p = ci.mem, ci.mem.ptr
    mk, kv = _knot_arrays(ci, knot_mask, knot_values, order)
    gco, gj = _cotangents(ci, grad_coeffs, grad_cost, order)
    desc = ci.desc(order, False, 0.0, vel_zero_weight)
    gwp, gtm, gkv = _wanted(mem, want, _KNOTS_VJP_WANT, (ci.waypoints, ci.times, kv), ci.io)
    stt = mem.empty((ci.B,), "i32") if want_status else None
    wsp, need = _workspace(mem, workspace, knots_vjp_workspace_bytes, desc, gco is not None)
    _check(_lib.csp_minsnap_solve_knots_batch_vjp(ctypes.byref(desc), p(ci.waypoints), p(ci.times), p(mk), p(kv), p(gco), p(gj),
                                                  p(gwp), p(gtm), p(gkv), p(stt), wsp, need, mem.stream(stream)))
    return KnotsVjpResult(gwp, gtm, gkv, stt)


def knots_timeopt_workspace_bytes(desc):
    return int(_lib.csp_minsnap_knots_timeopt_workspace_bytes(ctypes.byref(desc)))


def optimize_times_knots_batch(waypoints, times, knot_mask, knot_values, order=4, mode="fixed_total", time_weight=0.0,
                               min_time=0.01, tol=1e-6, max_iters=100, want_coeffs=True, vel_zero_weight=0.0,
                               seg_offsets=None, max_segments=None, vel_zero_weight_per_traj=None, workspace=None, stream=None):
    """Segment times that minimise the snap cost under per-knot derivative constraints
    (csp_minsnap_optimize_times_knots_batch): optimize_times_batch for the problem of solve_knots_batch, per
    trajectory in one launch.  knot_mask / knot_values as in solve_knots_batch (knots_from_bc's numpy arrays may be passed
    beside device waypoints); mode, time_weight, min_time, tol and max_iters as in optimize_times_batch.  Returns a
    TimeOptResult; coeffs, when wanted, are solve_knots_batch's at the returned times (bit-equal).  A trajectory with fewer
    constraints than `order` is returned unchanged with status TRAJ_NOT_SPD, iterations 0 and NaN objectives."""
    if mode not in _TIMEOPT_MODES:
        raise ValueError("mode: one of %r" % (tuple(_TIMEOPT_MODES),))
    ci = _CallInputs(waypoints, times, None, seg_offsets, max_segments, vel_zero_weight_per_traj)
    mem, p = ci.mem, ci.mem.ptr
    mk, kv = _knot_arrays(ci, knot_mask, knot_values, order)
    desc = ci.desc(order, False, 0.0, vel_zero_weight)
    prm = make_timeopt_params(_TIMEOPT_MODES[mode], time_weight, min_time, tol, max_iters)
    tout = mem.empty(ci.times.shape, ci.io)
    co = mem.empty(ci.coeffs_shape(order), ci.io) if want_coeffs else None
    obj = mem.empty((ci.B, 2), "f64")
    its = mem.empty((ci.B,), "i32")
    stt = mem.empty((ci.B,), "i32")
    wsp, need = mem.workspace(knots_timeopt_workspace_bytes(desc), workspace)
    _check(_lib.csp_minsnap_optimize_times_knots_batch(ctypes.byref(desc), ctypes.byref(prm), p(ci.waypoints), p(ci.times),
                                                       p(mk), p(kv), p(tout), p(co), p(obj), p(its), p(stt), wsp, need,
                                                       mem.stream(stream)))
    return TimeOptResult(tout, co, obj, its, stt)


def periodic_timeopt_workspace_bytes(desc):
    return int(_lib.csp_minsnap_periodic_timeopt_workspace_bytes(ctypes.byref(desc)))


def optimize_times_periodic_batch(waypoints, times, order=4, mode="fixed_total", time_weight=0.0, min_time=0.01, tol=1e-6,
                                  max_iters=100, want_coeffs=True, vel_zero_weight=0.0, seg_offsets=None, max_segments=None,
                                  vel_zero_weight_per_traj=None, workspace=None, stream=None):
    """Lap times that minimise the snap cost of a closed loop (csp_minsnap_optimize_times_periodic_batch):
    optimize_times_batch for the problem of solve_periodic_batch, per loop in one launch.  waypoints [B,S,3] (no repeated
    closing point), times [B,S]; ragged: waypoints [sum S_b,3] and times [sum S_b], both split by seg_offsets [B+1].
    mode, time_weight, min_time, tol and max_iters as in optimize_times_batch ("fixed_total" keeps the lap time).  Returns
    a TimeOptResult; coeffs, when wanted, are solve_periodic_batch's at the returned times (bit-equal).  To differentiate
    through the result, call solve_periodic_batch_autograd at the returned times."""
    if mode not in _TIMEOPT_MODES:
        raise ValueError("mode: one of %r" % (tuple(_TIMEOPT_MODES),))
    ci = _CallInputs(waypoints, times, None, seg_offsets, max_segments, vel_zero_weight_per_traj)
    mem, p = ci.mem, ci.mem.ptr
    desc = ci.desc(order, False, 0.0, vel_zero_weight)
    prm = make_timeopt_params(_TIMEOPT_MODES[mode], time_weight, min_time, tol, max_iters)
    tout = mem.empty(ci.times.shape, ci.io)
    co = mem.empty(ci.coeffs_shape(order), ci.io) if want_coeffs else None
    obj = mem.empty((ci.B, 2), "f64")
    its = mem.empty((ci.B,), "i32")
    stt = mem.empty((ci.B,), "i32")
    wsp, need = mem.workspace(periodic_timeopt_workspace_bytes(desc), workspace)
    _check(_lib.csp_minsnap_optimize_times_periodic_batch(ctypes.byref(desc), ctypes.byref(prm), p(ci.waypoints), p(ci.times),
                                                          p(tout), p(co), p(obj), p(its), p(stt), wsp, need,
                                                          mem.stream(stream)))
    return TimeOptResult(tout, co, obj, its, stt)


def _knots_forward(wp, tm, kv, knot_mask, with_cost, kw):
    r = solve_knots_batch(wp, tm, knot_mask, kv, want_cost=with_cost, **kw)
    return (r.coeffs, r.cost) if with_cost else r.coeffs


def _knots_vjp(want, grad_coeffs, grad_cost, wp, tm, kv, knot_mask, with_cost, kw):
    return solve_knots_batch_vjp(wp, tm, knot_mask, kv, grad_coeffs=grad_coeffs, grad_cost=grad_cost, want=want, **kw)


def solve_knots_batch_autograd(waypoints, times, knot_mask, knot_values, order=4, vel_zero_weight=0.0, seg_offsets=None,
                               max_segments=None, vel_zero_weight_per_traj=None, with_cost=False):
    """solve_knots_batch as a differentiable torch op (CUDA tensors; knot_mask may be a numpy array): returns the
    coefficients, or (coeffs, cost) with `with_cost` -- bit-equal to solve_knots_batch(...) -- with a grad_fn when
    waypoints, times or knot_values require grad.  The backward pass is one csp_minsnap_solve_knots_batch_vjp for the
    inputs that need a gradient; grad_coeffs or grad_cost is passed only when that output received a cotangent, so a loss
    on the cost alone runs the three-column kernel.  The gradient of a value whose mask bit is clear is 0.  First-order
    only (once_differentiable); no gradient with respect to the mask or the weights."""
    if isinstance(knot_values, np.ndarray):
        knot_values = torch.from_numpy(np.ascontiguousarray(knot_values)).to(device=waypoints.device, dtype=waypoints.dtype)
    kw = _solve_kw(order, vel_zero_weight, seg_offsets, max_segments, vel_zero_weight_per_traj)
    fn = _autograd_fn(_KNOTS_VJP_WANT, _knots_forward, _knots_vjp)
    return fn.apply(waypoints, times, knot_values, knot_mask, with_cost, kw)


def _periodic_forward(wp, tm, with_cost, kw):
    r = solve_periodic_batch(wp, tm, want_cost=with_cost, **kw)
    return (r.coeffs, r.cost) if with_cost else r.coeffs


def _periodic_vjp(want, grad_coeffs, grad_cost, wp, tm, with_cost, kw):
    if grad_coeffs is None:   # the loss uses the cost alone
        grad_coeffs = tm.new_zeros((math.prod(tm.shape), 3, 2 * kw["order"]))
    return solve_periodic_batch_vjp(wp, tm, grad_coeffs, grad_cost=grad_cost, want=want, **kw)


def solve_periodic_batch_autograd(waypoints, times, order=4, vel_zero_weight=0.0, seg_offsets=None, max_segments=None,
                                  vel_zero_weight_per_traj=None, with_cost=False):
    """solve_periodic_batch as a differentiable torch op (CUDA tensors): returns the coefficients, or (coeffs, cost) with
    `with_cost` -- bit-equal to solve_periodic_batch(...) -- with a grad_fn when waypoints or times require grad.  The
    backward pass is one csp_minsnap_solve_periodic_batch_vjp for the inputs that need a gradient; grad_cost is passed
    only when the cost received a cotangent.  First-order only (once_differentiable); no gradient with respect to the
    weights."""
    kw = _solve_kw(order, vel_zero_weight, seg_offsets, max_segments, vel_zero_weight_per_traj)
    return _autograd_fn(_PERIODIC_VJP_WANT, _periodic_forward, _periodic_vjp).apply(waypoints, times, with_cost, kw)


def periodic_time_alloc_batch(waypoints, v_avg, min_time_s, seg_offsets=None):
    """Segment times of closed loops by the reference's rule T = max(|dP|/v_avg, min_time_s) (time_alloc_batch), the
    closing segment P_{S-1} -> P_0 included.  waypoints [B,S,3] -> times [B,S]; ragged: waypoints [sum S_b,3] split by
    seg_offsets [B+1] -> times [sum S_b].  numpy arrays or torch CUDA tensors."""
    is_t = _is_torch(waypoints)
    if seg_offsets is None:
        if is_t:
            import torch
            closed = torch.cat([waypoints, waypoints[:, :1]], dim=1)
        else:
            waypoints = np.asarray(waypoints)
            closed = np.concatenate([waypoints, waypoints[:, :1]], axis=1)
        return time_alloc_batch(closed, v_avg, min_time_s)
    # ragged: the open-chain layout puts S_b + 1 points per trajectory; an empty loop gets one (unused) zero point
    off = np.asarray(seg_offsets.cpu() if _is_torch(seg_offsets) else seg_offsets, dtype=np.int64)
    B = off.shape[0] - 1
    total = int(off[-1]) if B >= 0 else 0
    lens = np.diff(off)
    idx = np.empty(total + B, dtype=np.int64)
    dst = off[:-1] + np.arange(B)
    pos = np.arange(total) + np.repeat(np.arange(B), lens)
    idx[pos] = np.arange(total)
    idx[dst + lens] = np.where(lens > 0, off[:-1], total)
    if is_t:
        import torch
        src = torch.cat([waypoints.reshape(-1, 3), waypoints.new_zeros((1, 3))])
        closed = src[torch.from_numpy(idx).to(waypoints.device)]
        so = torch.from_numpy(off).to(waypoints.device)
    else:
        waypoints = np.asarray(waypoints)
        src = np.concatenate([waypoints.reshape(-1, 3), np.zeros((1, 3), dtype=waypoints.dtype)])
        closed, so = src[idx], off
    return time_alloc_batch(closed, v_avg, min_time_s, seg_offsets=so)


class PreparedMulti:
    """csp_minsnap_solve_multi with everything fixed: `run()` is one C-ABI call -- and one kernel launch for the fixed-size
    buckets -- over n independent uniform batches of one shape (lists of CUDA tensors [B_k,S+1,3] / [B_k,S])."""

    def __init__(self, waypoints, times, bcs=None, order=4, vel_zero_weight=0.0, want_status=False, stream=None):
        n = len(waypoints)
        mem = _DeviceMem(waypoints[0])
        self.dev, io = mem.dev, mem.kind(waypoints[0])
        S = times[0].shape[1]
        self.wp = [mem.contig(w, io) for w in waypoints]
        self.tm = [mem.contig(t, io) for t in times]
        zero = _bc_block(mem, None, io)
        self.bc = [zero if (bcs is None or bcs[k] is None) else _bc_block(mem, bcs[k], io) for k in range(n)]
        self.out = [mem.empty((t.shape[0], S, 3, 2 * int(order)), io) for t in self.tm]
        self.status = [mem.empty((t.shape[0],), "i32") for t in self.tm] if want_status else None
        self.desc = make_desc(order, 0, S, _dtype_code(io), 0.0, vel_zero_weight, MEM_DEVICE, self.bc[0].shape[0] != 1,
                              device_id=mem.device_id)
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
        self._keep = (arr(self.wp), arr(self.tm), arr(self.bc), arr(self.out), arr(self.status) if want_status else None,
                      (ctypes.c_int64 * n)(*[t.shape[0] for t in self.tm]))
        self.n, self._stream = n, stream

    def run(self, stream=None):
        import torch
        st = stream if stream is not None else (self._stream if self._stream is not None
                                                else torch.cuda.current_stream(self.dev).cuda_stream)
        wp, tm, bc, out, stt, nb = self._keep
        rc = _lib.csp_minsnap_solve_multi(ctypes.byref(self.desc), self.n, ctypes.cast(nb, ctypes.c_void_p), ctypes.cast(wp, ctypes.c_void_p),
                                          ctypes.cast(tm, ctypes.c_void_p), ctypes.cast(bc, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p),
                                          ctypes.cast(stt, ctypes.c_void_p) if stt is not None else None, ctypes.c_void_p(st))
        if rc:
            _check(rc)
        return self.out


class MixedResult:
    """coeffs: flat storage-dtype array, trajectory b's [S_b,3,2*order_b] block at coeff_offsets[b] .. coeff_offsets[b+1]."""
    def __init__(self, coeffs, coeff_offsets, status):
        self.coeffs, self.coeff_offsets, self.status = coeffs, coeff_offsets, status


def mixed_block_elements(orders, seg_offsets, f32):
    """Elements of every trajectory's coefficient block in csp_minsnap_solve_mixed's layout: 6 * order * S rounded up to whole
    16-byte pieces (fp32: a multiple of 4; fp64: no padding).  Host arrays or device tensors; returns the same kind."""
    pad = 4 if f32 else 2
    if _is_torch(seg_offsets):
        e = (seg_offsets[1:] - seg_offsets[:-1]) * 6 * orders.to(seg_offsets.dtype)
        return (e + pad - 1) // pad * pad
    e = np.diff(np.asarray(seg_offsets, dtype=np.int64)) * 6 * np.asarray(orders, dtype=np.int64)
    return (e + pad - 1) // pad * pad


def mixed_coeff_total(orders, seg_offsets, f32=False):
    """Elements of the coefficient array of a mixed batch (host or device shapes)."""
    e = mixed_block_elements(orders, seg_offsets, f32)
    return int(e.sum().item()) if _is_torch(seg_offsets) else int(np.sum(e))


class PreparedMixed:
    """csp_minsnap_solve_mixed with descriptor, buffers and workspace fixed: `run()` is ONE C-ABI call that buckets the batch
    by (order, length class) on the device and solves it, coefficients in the caller's order (include/csp_minsnap.h)."""

    def __init__(self, orders, waypoints, times, seg_offsets, bc=None, vel_zero_weight=0.0, max_segments=None, out=None,
                 want_status=False, stream=None):
        if not (_is_torch(waypoints) and waypoints.is_cuda):
            raise ValueError("PreparedMixed takes CUDA tensors (device memory space)")
        ci = _CallInputs(waypoints, times, bc, seg_offsets, max_segments)
        mem, B = ci.mem, ci.B
        self.dev, self.wp, self.tm, self.off, self.bc = mem.dev, ci.waypoints, ci.times, ci.seg_offsets, ci.bc
        self.orders = mem.contig(orders, "i32")
        self.total = mixed_coeff_total(self.orders, self.off, ci.io == "f32")
        self.out = out if out is not None else mem.empty(max(self.total, 1), ci.io)
        self.coeff_offsets = mem.empty(B + 1, "i64")
        self.status = mem.empty(B, "i32") if want_status else None
        self.desc = ci.desc(0, ci.bc.shape[0] == B and B != 1, 0.0, vel_zero_weight)
        self.ws_bytes = _lib.csp_minsnap_mixed_workspace_bytes(ctypes.byref(self.desc))
        self.ws = mem.empty(max(self.ws_bytes, 1), "u8")
        self._stream = stream
        self._args = (ctypes.byref(self.desc), self.orders.data_ptr(), self.wp.data_ptr(), self.tm.data_ptr(), self.bc.data_ptr(),
                      self.out.data_ptr(), self.coeff_offsets.data_ptr(), self.status.data_ptr() if want_status else None,
                      self.ws.data_ptr(), self.ws_bytes)

    def run(self, stream=None):
        import torch
        st = stream if stream is not None else (self._stream if self._stream is not None
                                                else torch.cuda.current_stream(self.dev).cuda_stream)
        rc = _lib.csp_minsnap_solve_mixed(*self._args, ctypes.c_void_p(st))
        if rc:
            _check(rc)
        return self.out


def solve_mixed(orders, waypoints, times, seg_offsets, bc=None, vel_zero_weight=0.0, vel_zero_weight_per_traj=None,
                max_segments=None, want_status=False, stream=None, out=None):
    """csp_minsnap_solve_mixed: a ragged batch whose trajectories carry their own derivative order (2..5).
    numpy inputs -> CSP_MEM_HOST, torch CUDA tensors -> CSP_MEM_DEVICE.  Returns MixedResult.  `out` (host form only): the
    flat coefficient array to write, of at least mixed_coeff_total() elements; the blocks of skipped trajectories keep
    their contents."""
    if _is_torch(waypoints):   # the device form is one PreparedMixed, run once
        if vel_zero_weight_per_traj is not None or out is not None:
            raise ValueError("per-trajectory weights or a given output: use the host-memory form or PreparedMixed")
        p = PreparedMixed(orders, waypoints, times, seg_offsets, bc, vel_zero_weight, max_segments, want_status=want_status, stream=stream)
        p.run()
        return MixedResult(p.out, p.coeff_offsets, p.status)
    ci = _CallInputs(waypoints, times, bc, seg_offsets, max_segments, vel_zero_weight_per_traj)
    mem, p, B = ci.mem, ci.mem.ptr, ci.B
    orders = mem.contig(orders, "i32")
    need = max(mixed_coeff_total(orders, ci.seg_offsets, ci.io == "f32"), 1)
    if out is None:
        out = mem.empty(need, ci.io)
    elif not (isinstance(out, np.ndarray) and out.dtype == _DTYPE_NAME[ci.io] and out.flags.c_contiguous and out.size >= need):
        raise ValueError("out: a contiguous %s array of at least %d elements" % (_DTYPE_NAME[ci.io], need))
    cof = mem.empty(B + 1, "i64")
    stt = mem.empty(B, "i32") if want_status else None
    desc = ci.desc(0, ci.bc.shape[0] == B and B != 1, 0.0, vel_zero_weight)
    _check(_lib.csp_minsnap_solve_mixed(ctypes.byref(desc), p(orders), p(ci.waypoints), p(ci.times), p(ci.bc), p(out), p(cof),
                                        p(stt), None, 0, None))
    return MixedResult(out, cof, stt)


class PreparedSolve:
    """A solve whose descriptor, buffers and workspace are fixed: `run()` is one C-ABI call.
    For callers that launch the same shape many times (bench.py, a planner's inner loop) --
    building the descriptor and checking tensors costs more host time than a 40-us kernel."""

    def __init__(self, waypoints, times, bc=None, order=4, path_weight=0.0, vel_zero_weight=0.0, out=None,
                 force_generic=False, segment_major=False, no_persistent=False, stream=None,
                 seg_offsets=None, max_segments=None, span=False):
        if not (_is_torch(waypoints) and waypoints.is_cuda):
            raise ValueError("PreparedSolve takes CUDA tensors (device memory space)")
        ragged = seg_offsets is not None
        if ragged and segment_major:
            raise ValueError("segment_major needs a uniform batch")
        ci = _CallInputs(waypoints, times, bc, seg_offsets, max_segments if ragged else None)
        mem, B = ci.mem, ci.B
        self.dev, self.wp, self.tm, self.bc = mem.dev, ci.waypoints, ci.times, ci.bc
        if ragged:   # concatenated trajectories: waypoints [sum(S_b)+B,3], times [sum S_b], offsets [B+1] on the device
            self.off = ci.seg_offsets
        self.out = out if out is not None else mem.empty(ci.coeffs_shape(order, segment_major), ci.io)
        self.desc = ci.desc(order, ci.bc.shape[0] == B and B != 1, path_weight, vel_zero_weight,
                            _flags(force_generic, segment_major, no_persistent, span=span))
        self.ws_bytes = workspace_bytes(self.desc)
        self.ws = mem.empty(max(self.ws_bytes, 1), "u8")
        self.kernel = kernel_name(self.desc)
        self._stream = stream
        self._args = (ctypes.byref(self.desc), self.wp.data_ptr(), self.tm.data_ptr(), self.bc.data_ptr(),
                      self.out.data_ptr(), None, None, self.ws.data_ptr() if self.ws_bytes else None, self.ws_bytes)

    def run(self, stream=None):
        import torch
        st = stream if stream is not None else (self._stream if self._stream is not None
                                                else torch.cuda.current_stream(self.dev).cuda_stream)
        rc = _lib.csp_minsnap_solve_batch(*self._args, ctypes.c_void_p(st))
        if rc:
            _check(rc)
        return self.out


def time_alloc_batch(waypoints, v_avg, min_time_s, seg_offsets=None, stream=None):
    """Batched T_i = max(|dp_i|/V_avg, min_time_s) (math_util/minimum_snap.cpp:63-72)."""
    mem = _mem(waypoints)
    io = mem.kind(waypoints)
    waypoints = mem.contig(waypoints, io)
    off = None
    if seg_offsets is not None:
        off = mem.contig(seg_offsets, "i64")
        B, S = off.shape[0] - 1, 0
        times = mem.empty(waypoints.shape[0] - B, io)
    else:
        B, S = waypoints.shape[0], waypoints.shape[1] - 1
        times = mem.empty((B, S), io)
    desc = make_desc(1, B, S, _dtype_code(io), mem_space=mem.mem_space, seg_offsets_ptr=mem.ptr(off),
                     max_segments=1 if off is not None else 0, device_id=mem.device_id)
    _check(_lib.csp_minsnap_time_alloc_batch(ctypes.byref(desc), mem.ptr(waypoints), float(v_avg), float(min_time_s),
                                             mem.ptr(times), mem.stream(stream)))
    return times


class Plan:
    __slots__ = ("times", "coeffs", "max_dev", "vel_zero_weight", "iterations", "status")


def _plan_inputs(waypoints, bc, order, path_weight, vel_zero_weight, flags=0):
    """(backend, storage kind, waypoints, bc, descriptor) of plan_batch / generate_batch: uniform waypoints [B,S+1,3]."""
    mem = _mem(waypoints)
    io = mem.kind(waypoints)
    waypoints = mem.contig(waypoints, io)
    B = waypoints.shape[0]
    bc = _bc_block(mem, bc, io)
    desc = make_desc(order, B, waypoints.shape[1] - 1, _dtype_code(io), path_weight, vel_zero_weight, mem.mem_space,
                     bc.shape[0] == B and B != 1, device_id=mem.device_id, flags=flags)
    return mem, io, waypoints, bc, desc


def _plan_outputs(r, mem, io, desc):
    """Allocates the Plan fields of `r`; returns their pointers in the C-ABI's order."""
    B, S = desc.batch, desc.num_segments
    r.times = mem.empty((B, S), io)
    r.coeffs = mem.empty((B, S, 3, 2 * desc.order), io)
    r.max_dev, r.vel_zero_weight = mem.empty(B, "f64"), mem.empty(B, "f64")
    r.iterations, r.status = mem.empty(B, "i32"), mem.empty(B, "i32")
    return [mem.ptr(a) for a in (r.times, r.coeffs, r.max_dev, r.vel_zero_weight, r.iterations, r.status)]


def _plan_workspace_bytes(desc):
    return int(_lib.csp_minsnap_plan_workspace_bytes(ctypes.byref(desc)))


def plan_batch(waypoints, v_avg, min_time_s, bc=None, order=3, path_weight=0.0, vel_zero_weight=0.0):
    """Batched solver half of GenerateTrajectoryMatrix (math_util/minimum_snap.cpp:59-90): time
    allocation + the <=10x vel_zero_weight doubling loop.  Uniform batches, numpy (host) or torch
    CUDA tensors.  waypoints [B,S+1,3]."""
    mem, io, waypoints, bc, desc = _plan_inputs(waypoints, bc, order, path_weight, vel_zero_weight)
    r = Plan()
    outs = _plan_outputs(r, mem, io, desc)
    wsp, need = _scratch(mem, _plan_workspace_bytes, desc)
    _check(_lib.csp_minsnap_plan_batch(ctypes.byref(desc), mem.ptr(waypoints), float(v_avg), float(min_time_s), mem.ptr(bc),
                                       *outs, wsp, need, mem.stream()))
    return r


def sample_capacity(waypoints, v_avg, min_time_s, order=3):
    """Upper bound of the samples per trajectory (csp_minsnap_sample_capacity), from host waypoints [B,S+1,3]."""
    io = _HOST.kind(waypoints)
    waypoints = _HOST.contig(waypoints, io)
    desc = make_desc(order, waypoints.shape[0], waypoints.shape[1] - 1, _dtype_code(io), mem_space=MEM_HOST)
    cap = int(_lib.csp_minsnap_sample_capacity(ctypes.byref(desc), waypoints.ctypes.data, float(v_avg), float(min_time_s)))
    if cap < 0:
        raise CspError(-1, "csp_minsnap_sample_capacity")
    return cap


class Generated(Plan):
    """Plan + samples [B,capacity,3], counts [B], stats [B,2]."""
    __slots__ = ("samples", "counts", "stats")


def _sample_outputs(mem, io, B, capacity):
    return mem.zeros((B, capacity, 3), io), mem.empty(B, "i32"), mem.empty((B, 2), "f64")


def generate_batch(waypoints, v_avg, min_time_s, sample_distance, capacity=None, bc=None, order=3, path_weight=0.0,
                   vel_zero_weight=0.0, long_segments=False):
    """The whole of GenerateTrajectoryMatrix (math_util/minimum_snap.cpp:22-206) in one call
    (csp_minsnap_generate_batch = plan_batch + sample_batch, bit for bit).  Uniform batches, numpy (host: one upload,
    one download, one synchronisation) or torch CUDA tensors (asynchronous; `capacity` required)."""
    mem, io, waypoints, bc, desc = _plan_inputs(waypoints, bc, order, path_weight, vel_zero_weight, _flags(long_segments=long_segments))
    if capacity is None:
        if mem.mem_space == MEM_DEVICE:   # csp_minsnap_sample_capacity reads the waypoints on the host
            raise ValueError("device-memory generate_batch needs a capacity")
        capacity = int(_lib.csp_minsnap_sample_capacity(ctypes.byref(desc), mem.ptr(waypoints), float(v_avg), float(min_time_s)))
    r = Generated()
    outs = _plan_outputs(r, mem, io, desc)
    r.samples, r.counts, r.stats = _sample_outputs(mem, io, desc.batch, capacity)
    wsp, need = _scratch(mem, _plan_workspace_bytes, desc)
    _check(_lib.csp_minsnap_generate_batch(ctypes.byref(desc), mem.ptr(waypoints), float(v_avg), float(min_time_s), mem.ptr(bc),
                                           float(sample_distance), int(capacity), mem.ptr(r.samples), mem.ptr(r.counts),
                                           mem.ptr(r.stats), *outs, wsp, need, mem.stream()))
    return r


def sample_batch(times, coeffs, sample_distance, capacity, order=None, out=None, one_lane=False, long_segments=False,
                 seg_offsets=None):
    """Batched sampling half of GenerateTrajectoryMatrix (math_util/minimum_snap.cpp:97-205).
    times [B,S], coeffs [B,S,3,2o].  Returns (samples [B,capacity,3], counts [B], stats [B,2]).
    `out` (device path): a (samples, counts, stats) triple to reuse; rows beyond counts[b] are then
    left as they were instead of zero.  `one_lane` forces the one-lane-per-trajectory kernel (A/B tests);
    `long_segments` (device path) selects the wave-per-trajectory kernel for legs of hundreds of candidates
    (the host path decides from the times).  Ragged batches (host arrays): times [sum S_b], coeffs [sum S_b,3,2o],
    `seg_offsets` [B+1]."""
    mem = _mem(times)
    device = mem.mem_space == MEM_DEVICE
    if seg_offsets is not None and device:
        raise ValueError("ragged sampling takes host arrays here")
    io = mem.kind(times)
    times, coeffs = mem.contig(times, io), mem.contig(coeffs, io)
    off, B, S, _, smax = _ragged_dims(mem, seg_offsets, times, None)
    order = int(order) if order is not None else int(coeffs.shape[-1]) // 2
    # a host-memory call always returns fresh arrays: `out` is the device path's
    samples, counts, stats = out if out is not None and device else _sample_outputs(mem, io, B, capacity)
    desc = make_desc(order, B, S, _dtype_code(io), mem_space=mem.mem_space, seg_offsets_ptr=mem.ptr(off),
                     max_segments=smax if off is not None and B else 0, device_id=mem.device_id,
                     flags=_flags(force_generic=one_lane, long_segments=long_segments))
    _check(_lib.csp_minsnap_sample_batch(ctypes.byref(desc), mem.ptr(times), mem.ptr(coeffs), float(sample_distance),
                                         int(capacity), mem.ptr(samples), mem.ptr(counts), mem.ptr(stats), mem.stream()))
    return samples, counts, stats


class EvalResult:
    """eval_batch: values [B,Q,D,3], seg_index [B,Q] i32 (or None), status [B] i32 (or None)."""
    __slots__ = ("values", "seg_index", "status")

    def __init__(self, values, seg_index, status):
        self.values, self.seg_index, self.status = values, seg_index, status


class EvalVjpResult:
    """Gradients of eval_batch_vjp; a gradient that was not asked for is None."""
    __slots__ = ("coeffs", "times", "query", "status")

    def __init__(self, coeffs, times, query, status):
        self.coeffs, self.times, self.query, self.status = coeffs, times, query, status


_EVAL_VJP_WANT = ("coeffs", "times", "query")


class _EvalInputs:
    """times / coeffs / query of one evaluation call, contiguous in the memory space of `times`, and their descriptor."""

    def __init__(self, times, coeffs, query, order, seg_offsets, max_segments):
        self.mem = mem = _mem(times)
        self.io = io = mem.kind(times)
        self.times, self.coeffs, self.query = mem.contig(times, io), mem.contig(coeffs, io), mem.contig(query, io)
        self.seg_offsets, self.B, self.S, self.total, smax = _ragged_dims(mem, seg_offsets, self.times, max_segments)
        self.order = int(order) if order is not None else int(self.coeffs.shape[-1]) // 2
        if math.prod(self.coeffs.shape) != self.total * 6 * self.order:
            raise ValueError("coeffs must hold %d elements ([segments,3,2*order])" % (self.total * 6 * self.order))
        if self.query.ndim != 2 or self.query.shape[0] != self.B:
            raise ValueError("query must be [B,Q] with B = %d" % self.B)
        self.Q = int(self.query.shape[1])
        if mem.mem_space == MEM_DEVICE and self.coeffs.data_ptr() % 16:   # records are read in 16-byte pieces
            self.coeffs = self.coeffs.clone()
        self.desc = make_desc(self.order, self.B, self.S, _dtype_code(io), mem_space=mem.mem_space,
                              seg_offsets_ptr=mem.ptr(self.seg_offsets), max_segments=(smax or 0) if self.seg_offsets is not None else 0,
                              device_id=mem.device_id)


def eval_batch(times, coeffs, query, num_derivs=3, order=None, seg_offsets=None, max_segments=None, want_seg_index=False,
               want_status=False, stream=None):
    """Position and its first num_derivs - 1 derivatives of every trajectory at its query times
    (csp_minsnap_eval_batch).  times [B,S], coeffs [B,S,3,2o] as solve_batch or
    solve_periodic_batch return them, query [B,Q] global times from the trajectory's start (clamped to [0, sum T]; a
    query on a knot belongs to the later segment).  Ragged: times [sum S_b], coeffs [sum S_b,3,2o], seg_offsets [B+1].
    numpy arrays -> host memory (synchronous), torch CUDA tensors -> device memory (asynchronous on the current stream).
    Returns EvalResult(values [B,Q,D,3], seg_index, status)."""
    ei = _EvalInputs(times, coeffs, query, order, seg_offsets, max_segments)
    mem, p, D = ei.mem, ei.mem.ptr, int(num_derivs)
    out = mem.empty((ei.B, ei.Q, max(D, 0), 3), ei.io)
    sg = mem.empty((ei.B, ei.Q), "i32") if want_seg_index else None
    stt = mem.zeros((ei.B,), "i32") if want_status else None   # zeros: no query, no launch
    _check(_lib.csp_minsnap_eval_batch(ctypes.byref(ei.desc), p(ei.times), p(ei.coeffs), p(ei.query), ei.Q, D, p(out), p(sg),
                                       p(stt), mem.stream(stream)))
    return EvalResult(out, sg, stt)


def eval_batch_vjp(times, coeffs, query, grad_out, num_derivs=None, order=None, seg_offsets=None, max_segments=None,
                   want=_EVAL_VJP_WANT, want_status=False, stream=None):
    """Vector-Jacobian product of eval_batch (csp_minsnap_eval_batch_vjp): given grad_out = dL/dvalues [B,Q,D,3] (D is
    taken from it unless num_derivs is given), returns EvalVjpResult(dL/dcoeffs, dL/dtimes, dL/dquery, status) for the
    names in `want`.  dL/dtimes is the explicit dependence through the local time only; the dependence of the
    coefficients on the times is solve_batch_vjp's.  Every record of dL/dcoeffs is written.  Deterministic run to run."""
    ei = _EvalInputs(times, coeffs, query, order, seg_offsets, max_segments)
    mem, p = ei.mem, ei.mem.ptr
    go = mem.contig(grad_out, ei.io)
    D = int(num_derivs) if num_derivs is not None else int(go.shape[-2])
    if math.prod(go.shape) != ei.B * ei.Q * D * 3:
        raise ValueError("grad_out must hold %d elements ([B,Q,D,3])" % (ei.B * ei.Q * D * 3))
    gco, gtm, gq = _wanted(mem, want, _EVAL_VJP_WANT, (ei.coeffs, ei.times, ei.query), ei.io)
    stt = mem.zeros((ei.B,), "i32") if want_status else None
    _check(_lib.csp_minsnap_eval_batch_vjp(ctypes.byref(ei.desc), p(ei.times), p(ei.coeffs), p(ei.query), ei.Q, D, p(go), p(gco),
                                           p(gtm), p(gq), p(stt), mem.stream(stream)))
    return EvalVjpResult(gco, gtm, gq, stt)


def _eval_forward(co, tm, query, kw):
    return eval_batch(tm, co, query, **kw).values


def _eval_vjp(want, grad_values, _, co, tm, query, kw):
    return eval_batch_vjp(tm, co, query, grad_values, want=want, **kw)


def eval_batch_autograd(coeffs, times, query, num_derivs=3, seg_offsets=None, max_segments=None):
    """eval_batch as a differentiable torch op (CUDA tensors): returns the values [B,Q,D,3] -- bit-equal to
    eval_batch(...).values -- with a grad_fn when coeffs, times or query require grad.  The backward pass is one
    csp_minsnap_eval_batch_vjp for the inputs that need a gradient; first-order only (once_differentiable).  Chains with
    solve_batch_autograd and solve_periodic_batch_autograd: pass their coefficients and the same times tensor, and
    autograd adds this op's explicit time gradient to the solve's."""
    kw = dict(num_derivs=num_derivs, seg_offsets=seg_offsets, max_segments=max_segments)
    return _autograd_fn(_EVAL_VJP_WANT, _eval_forward, _eval_vjp).apply(coeffs, times, query, kw)


def _geo(fn, pts, ref):
    ref = np.ascontiguousarray(ref, dtype=np.float64).reshape(3)
    mem = _mem(pts)
    pts = mem.contig(pts, "f64").reshape(-1, 3)
    out = mem.empty(pts.shape, "f64")
    _check(fn(mem.ptr(pts), ref.ctypes.data, mem.ptr(out), pts.shape[0], mem.mem_space, mem.device_id, mem.stream()))
    return out


def wgs84_to_enu_batch(lla, ref):
    """Batched UavPathPlanner::wgs84ToENU (uavPathPlanning.cpp:1046-1063, :1085-1095).
    lla [N,3] = (lon_deg, lat_deg, alt_m); ref [3] same convention."""
    return _geo(_lib.csp_geo_wgs84_to_enu_batch, lla, ref)


def enu_to_wgs84_batch(enu, ref):
    """Batched UavPathPlanner::enuToWGS84 (uavPathPlanning.cpp:1066-1083, :1098-1108)."""
    return _geo(_lib.csp_geo_enu_to_wgs84_batch, enu, ref)


def _alt_params(lambda_smooth, lambda_follow, safe_distance, max_climb_rate):
    return AltParams(float(lambda_smooth), float(lambda_follow), float(safe_distance), float(max_climb_rate))


def _alt_ws_bytes(total):
    return int(_lib.csp_alt_workspace_bytes(int(total)))


def _alt_inputs(xyz, z, offsets):
    """(backend, xyz [total,3], elev or input_z [total], offsets [B+1]) of the altitude entries, all fp64."""
    mem = _mem(xyz)
    return mem, mem.contig(xyz, "f64").reshape(-1, 3), mem.contig(z, "f64"), mem.contig(offsets, "i64")


def alt_optimize_heights_batch(xyz, elev, offsets, lambda_smooth=1.0, lambda_follow=0.0, safe_distance=50.0,
                               max_climb_rate=2.0):
    """Batched UavPathPlanner::optimizeHeights (uavPathPlanning.cpp:1575-1713).  numpy arrays (host memory) or torch CUDA
    tensors (device memory): xyz [total,3], elev [total] (NaN = no terrain sample), offsets [B+1].  Returns z [total]."""
    p = _alt_params(lambda_smooth, lambda_follow, safe_distance, max_climb_rate)
    mem, xyz, elev, offsets = _alt_inputs(xyz, elev, offsets)
    a, total = mem.addr, xyz.shape[0]
    out = mem.empty(total, "f64")
    wsp, need = _scratch(mem, _alt_ws_bytes, total)
    _check(_lib.csp_alt_optimize_heights_batch(a(xyz), a(elev), a(offsets), offsets.shape[0] - 1, ctypes.byref(p), a(out),
                                               wsp, need, mem.mem_space, mem.device_id, mem.stream()))
    mem.sync()   # the workspace is a local: it must outlive the kernel
    return out


def alt_global_smooth_batch(input_z, xyz, offsets, lambda_smooth=1.0, max_climb_rate=2.0):
    """Batched UavPathPlanner::optimizeHeightsGlobalSmooth (uavPathPlanning.cpp:1715-1827).
    Returns (z [total], solves [B]); numpy (host memory) or torch CUDA tensors (device memory)."""
    p = _alt_params(lambda_smooth, 0.0, 0.0, max_climb_rate)
    mem, xyz, input_z, offsets = _alt_inputs(xyz, input_z, offsets)
    a, total, B = mem.addr, xyz.shape[0], offsets.shape[0] - 1
    out, solves = mem.empty(total, "f64"), mem.empty(B, "i32")
    wsp, need = _scratch(mem, _alt_ws_bytes, total)
    _check(_lib.csp_alt_global_smooth_batch(a(input_z), a(xyz), a(offsets), B, ctypes.byref(p), a(out), a(solves), wsp, need,
                                            mem.mem_space, mem.device_id, mem.stream()))
    mem.sync()   # as above
    return out, solves


BEZIER_UNSAMPLEABLE = 2 ** 31 - 1   # CSP_BEZIER_UNSAMPLEABLE (include/csp_bezier.h)


def bezier_generate_batch(waypoints, offsets, resolution=1.0, min_radius=1.0, capacity=4096):
    """Batched math_util::Bezier::GenerateTrajectoryMatrix (math_util/bezier.cpp:127-190; include/csp_bezier.h).
    waypoints [total,3] (paths concatenated), offsets [B+1] point prefix sums; numpy (host) or torch CUDA tensors.
    Returns (samples [B,capacity,3], counts [B]).  With CUDA tensors the rows at and past min(counts[b], capacity) are
    zero; with numpy arrays (host memory, staged through the device) they are unspecified.  counts[b] ==
    BEZIER_UNSAMPLEABLE (INT32_MAX) marks a path with a segment of more than 2^24 samples at this resolution (a garbage
    coordinate): it is not walked, its rows are unspecified, the other paths are unaffected."""
    mem = _mem(waypoints)
    wp = mem.contig(waypoints, "f64").reshape(-1, 3)
    off = mem.contig(offsets, "i64")
    B = off.shape[0] - 1
    samples, counts = mem.zeros((B, capacity, 3), "f64"), mem.empty(B, "i32")
    _check(_lib.csp_bezier_generate_batch(mem.ptr(wp), mem.ptr(off), B, float(resolution), float(min_radius), int(capacity),
                                          mem.ptr(samples), mem.ptr(counts), mem.mem_space, mem.device_id, mem.stream()))
    return samples, counts
