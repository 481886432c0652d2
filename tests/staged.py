"""The C-ABI entries as argument tables for tests that call them through raw pointers (TEST INFRASTRUCTURE ONLY):
tests/test_gpu_edges.py (host and device forms bit-equal), tests/test_gpu_bounds.py (guard bands, stale memory, bad lanes
of the entries that take a caller's workspace) and tests/test_gpu_bounds_fast.py (the same contracts for the
workspace-free kernels, the multi-batch entry and the time-allocation / plan / sample / generate chain)."""
import numpy as np

from tests import guarded

# The five entries that stage host memory the same way: C symbol, workspace function, and per pointer argument
# (name, "in" / "out", required).  Shapes and element types are in staged_buffers.
STAGED = {
    "solve_batch": ("csp_minsnap_solve_batch", "csp_minsnap_workspace_bytes",
                    (("waypoints", "in", True), ("times", "in", True), ("bc", "in", True), ("coeffs", "out", True),
                     ("max_dev", "out", False), ("status", "out", False))),
    "solve_batch_vjp": ("csp_minsnap_solve_batch_vjp", "csp_minsnap_vjp_workspace_bytes",
                        (("waypoints", "in", True), ("times", "in", True), ("bc", "in", True), ("grad_coeffs", "in", True),
                         ("grad_waypoints", "out", False), ("grad_times", "out", False), ("grad_bc", "out", False),
                         ("status", "out", False))),
    "cost_batch": ("csp_minsnap_cost_batch", "csp_minsnap_cost_workspace_bytes",
                   (("waypoints", "in", True), ("times", "in", True), ("bc", "in", True), ("cost", "out", True),
                    ("grad_times", "out", False), ("status", "out", False))),
    "optimize_times_batch": ("csp_minsnap_optimize_times_batch", "csp_minsnap_timeopt_workspace_bytes",
                             (("waypoints", "in", True), ("times", "in", True), ("bc", "in", True), ("times_out", "out", True),
                              ("coeffs", "out", False), ("objective", "out", False), ("iterations", "out", False),
                              ("status", "out", False))),
    "solve_periodic_batch": ("csp_minsnap_solve_periodic_batch", "csp_minsnap_periodic_workspace_bytes",
                             (("waypoints", "in", True), ("times", "in", True), ("coeffs", "out", True), ("cost", "out", False),
                              ("grad_times", "out", False), ("status", "out", False))),
}

# Every entry with a caller-supplied workspace, for the memory tests: the five above (the forward solve once per
# workspace path, chosen by a descriptor flag: "generic" = CSP_FLAG_FORCE_GENERIC, "span" = CSP_FLAG_SPAN) and the
# mixed-order entry.  Rows: (C symbol, workspace function, arguments, name of the descriptor flag or None).
WORKSPACE_ENTRIES = {
    "solve_batch_generic": STAGED["solve_batch"] + ("FLAG_FORCE_GENERIC",),
    "solve_batch_span": STAGED["solve_batch"] + ("FLAG_SPAN",),
    "solve_batch_vjp": STAGED["solve_batch_vjp"] + (None,),
    "cost_batch": STAGED["cost_batch"] + (None,),
    "optimize_times_batch": STAGED["optimize_times_batch"] + (None,),
    "solve_periodic_batch": STAGED["solve_periodic_batch"] + (None,),
    "solve_mixed": ("csp_minsnap_solve_mixed", "csp_minsnap_mixed_workspace_bytes",
                    (("orders", "in", True), ("waypoints", "in", True), ("times", "in", True), ("bc", "in", True),
                     ("coeffs", "out", True), ("coeff_offsets", "out", False), ("status", "out", False)), None),
}


def staged_buffers(entry, lens, order, f32, bc_per, seed):
    """Host arrays of every pointer argument of `entry` for trajectories of `lens` segments (outputs zeroed)."""
    rng = np.random.default_rng(seed)
    io = np.float32 if f32 else np.float64
    B, total, m = len(lens), int(np.sum(lens)), 2 * order
    n_wp = total if entry == "solve_periodic_batch" else total + B   # a closed loop has no repeated end point
    b = dict(waypoints=np.cumsum(rng.normal(size=(n_wp, 3)), axis=0).astype(io), times=rng.uniform(0.5, 2.0, size=total).astype(io),
             bc=rng.normal(size=(B if bc_per else 1, 4, 3)).astype(io), grad_coeffs=rng.normal(size=(total, 3, m)).astype(io))
    b.update(coeffs=np.zeros((total, 3, m), io), grad_waypoints=np.zeros((n_wp, 3), io), grad_times=np.zeros(total, io),
             grad_bc=np.zeros_like(b["bc"]), times_out=np.zeros(total, io), max_dev=np.zeros(B), cost=np.zeros(B),
             objective=np.zeros((B, 2)), status=np.zeros(B, np.int32), iterations=np.zeros(B, np.int32))
    return b


def mixed_block_elements(orders, lens, f32):
    """Elements of every trajectory's block in csp_minsnap_solve_mixed's coefficient layout (include/csp_minsnap.h):
    6 * order * S rounded up to whole 16-byte pieces."""
    pad = 4 if f32 else 2
    e = np.asarray(lens, dtype=np.int64) * 6 * np.asarray(orders, dtype=np.int64)
    return (e + pad - 1) // pad * pad


def mixed_buffers(lens, orders, f32, bc_per, seed):
    """staged_buffers for the mixed-order entry: per-trajectory `orders`, the flat coefficient array and its offsets."""
    b = staged_buffers("solve_mixed", lens, 1, f32, bc_per, seed)
    io = np.float32 if f32 else np.float64
    total_co = int(mixed_block_elements(orders, lens, f32).sum())
    b.update(orders=np.asarray(orders, dtype=np.int32), coeffs=np.zeros(total_co, io),
             coeff_offsets=np.zeros(len(lens) + 1, np.int64))
    return b


# The entries of tests/test_gpu_bounds_fast.py that the tables above do not hold: (C symbol, workspace function or None,
# arguments).  Scalars of the C signature (v_avg, min_time_s, sample_distance, capacity) are the test's own business.
FAST_ENTRIES = {
    "solve_batch": STAGED["solve_batch"],
    "time_alloc_batch": ("csp_minsnap_time_alloc_batch", None, (("waypoints", "in", True), ("times", "out", True))),
    "plan_batch": ("csp_minsnap_plan_batch", "csp_minsnap_plan_workspace_bytes",
                   (("waypoints", "in", True), ("bc", "in", True), ("times", "out", True), ("coeffs", "out", True),
                    ("max_dev", "out", False), ("vel_zero_weight_out", "out", False), ("iterations", "out", False),
                    ("status", "out", False))),
    "sample_batch": ("csp_minsnap_sample_batch", None,
                     (("times", "in", True), ("coeffs", "in", True), ("samples", "out", True), ("counts", "out", True),
                      ("stats", "out", False))),
    "generate_batch": ("csp_minsnap_generate_batch", "csp_minsnap_plan_workspace_bytes",
                       (("waypoints", "in", True), ("bc", "in", True), ("samples", "out", True), ("counts", "out", True),
                        ("stats", "out", False), ("times", "out", True), ("coeffs", "out", True), ("max_dev", "out", False),
                        ("vel_zero_weight_out", "out", False), ("iterations", "out", False), ("status", "out", False))),
}


class Carved:
    """One pointer argument inside a guarded carve (tests/guarded.py) of exactly its size.  `shift` > 0 puts the argument
    that many bytes past the carve's (256-byte aligned) start, the carve being that much larger: the lead bytes keep the
    guard pattern and are checked with the bands.  An input holds `host`'s bytes, an output starts as `fill` bytes."""

    def __init__(self, host, device, name, fill=None, band=guarded.BAND, shift=0):
        self.host, self.shift, self.name = np.ascontiguousarray(host), int(shift), name
        self.g = guarded.Guarded(self.host.nbytes + self.shift, device, band, name=name)
        if self.shift:
            self.g.raw[:self.shift].fill_(guarded.PATTERN)
        if fill is None:
            self.put(self.host)
        else:
            self.g.raw[self.shift:].fill_(int(fill))

    def put(self, array):
        src = np.ascontiguousarray(array)
        assert src.nbytes == self.host.nbytes, (self.name, src.nbytes, self.host.nbytes)
        if src.nbytes:
            import torch
            self.g.raw[self.shift:].copy_(torch.from_numpy(src.reshape(-1).view(np.uint8).copy()))
        return self

    def data_ptr(self):
        return self.g.data_ptr() + self.shift

    def bytes(self):
        return self.g.bytes()[self.shift:]

    def numpy(self, dtype=None, shape=None):
        return self.bytes().view(self.host.dtype if dtype is None else dtype).reshape(self.host.shape if shape is None else shape)

    def check(self):
        self.g.check()
        lead = self.g.bytes()[:self.shift]
        assert (lead == guarded.PATTERN).all(), "%s: the %d bytes in front of the shifted pointer were written" % (self.name, self.shift)


def carve_args(args, host, opt, fill, device, band=guarded.BAND, shift=None):
    """({name: Carved} of the inputs, {name: Carved} of the outputs) of an argument table: every input a guarded copy of
    host[name], every required output -- and, with `opt`, every optional one (`opt` may also be a set of names) -- a
    guarded array of host[name]'s shape and type that starts as `fill` bytes.  shift: {name: bytes}, see Carved."""
    shift = shift or {}
    ins, outs = {}, {}
    for n, kind, req in args:
        if kind == "in":
            ins[n] = Carved(host[n], device, n, None, band, shift.get(n, 0))
        elif req or (n in opt if isinstance(opt, (set, frozenset)) else opt):
            outs[n] = Carved(host[n], device, n, fill, band, shift.get(n, 0))
    return ins, outs


def arg_pointers(args, ins, outs):
    """The pointer arguments in the table's order (None for an optional output that is not passed)."""
    out = []
    for n, kind, _ in args:
        g = ins.get(n) if kind == "in" else outs.get(n)
        out.append(g.data_ptr() if g is not None else None)
    return out


def check_carves(tag, carves, inputs):
    """No guard byte of any of `carves` changed, and every one of `inputs` (Carved) still holds its host bytes."""
    for g in carves:
        try:
            g.check()
        except AssertionError as e:
            raise AssertionError("%r: %s" % (tag, e)) from None
    for g in inputs:
        assert g.bytes().tobytes() == g.host.tobytes(), (tag, "input changed", g.name)
