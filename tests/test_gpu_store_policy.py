"""Store policy of the order-4 persistent solve: launches whose coefficients exceed the chip's aggregate
L2 (8 x 4 MiB) may leave through write-through stores.  The policy changes how bytes travel, never which bytes: every
launch must be bit-equal to the one-workgroup-per-slice kernel (`no_persistent=True`: ordinary stores, same arithmetic)."""
import functools

import numpy as np
import pytest

from tests import guarded, synth

pytestmark = pytest.mark.gpu

TOL_WELL = 5e-8      # HIP against the fp64 oracle, as in tests/test_gpu_parity.py
L2_BYTES = 8 * 4 * 1024 * 1024


@functools.lru_cache(maxsize=None)
def _inputs(B, S):
    """Host batch and its device copy, made once per shape and never written."""
    import torch
    wp, tm = synth.make_batch(B, S, config_id=70 + S)
    return wp, tm, torch.from_numpy(wp).cuda(), torch.from_numpy(tm).cuda()


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("S", [2, 6, 16])
@pytest.mark.parametrize("big", [False, True])
def test_default_call_is_bit_equal_to_the_one_slice_kernel(csp, oracle_mod, S, big):
    """B = 64 (2 CUs + 3) + 5: some persistent workgroups walk two slices and a ragged tail takes the one-slice kernel.
    B = 64 x 1024: the headline batch, where the write-through rule is active.  S = 6 has the middle pair that is stored
    singly, S = 2 nothing but single records."""
    import torch
    B = 64 * 1024 if big else 64 * (2 * _cus() + 3) + 5
    wp, tm, d_wp, d_tm = _inputs(B, S)
    a = csp.solve_batch(d_wp, d_tm, order=4)
    assert a.kernel == "fixed_o4_s%d_f64" % S, a.kernel
    b = csp.solve_batch(d_wp, d_tm, order=4, no_persistent=True)
    torch.cuda.synchronize()
    assert torch.equal(a.coeffs, b.coeffs)
    n_full = B // 64
    idx = np.unique(np.array([0, 63, 64, 64 * (n_full // 2) - 1, 64 * (n_full // 2), 64 * n_full - 1, B - 1]))
    ref, _ = oracle_mod.solve_batch(4, wp[idx], tm[idx])
    synth.parity_gate(a.coeffs[torch.from_numpy(idx).cuda()].cpu().numpy(), ref, TOL_WELL, ("store policy vs oracle", S, B))


@pytest.mark.parametrize("S", [6, 16])
def test_guard_bands_around_the_coefficients(csp, S):
    """The output sits between two 64 KiB sentinel bands; a launch under the write-through rule leaves them alone."""
    import torch
    B = 64 * 1024
    _, _, d_wp, d_tm = _inputs(B, S)
    assert B * S * 192 > L2_BYTES
    g = guarded.carve_array((B, S, 3, 8), torch.float64, d_wp.device, name="coeffs")
    g.fill(0xFF)
    r = csp.solve_batch(d_wp, d_tm, order=4, out=g.t)
    want = csp.solve_batch(d_wp, d_tm, order=4, no_persistent=True).coeffs
    torch.cuda.synchronize()
    g.check()
    assert r.coeffs.data_ptr() == g.data_ptr()
    assert torch.equal(g.t, want)


@pytest.mark.parametrize("B", [10922, 10923])
def test_both_sides_of_the_l2_threshold(csp, B):
    """S = 16: 3072 coefficient bytes per trajectory, so B = 10922 is 2 KiB under 32 MiB and B = 10923 1 KiB over."""
    import torch
    S = 16
    assert (B * S * 192 > L2_BYTES) == (B == 10923)
    _, _, d_wp, d_tm = _inputs(B, S)
    a = csp.solve_batch(d_wp, d_tm, order=4).coeffs
    b = csp.solve_batch(d_wp, d_tm, order=4, no_persistent=True).coeffs
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_status_and_max_dev_are_unaffected(csp):
    """The side outputs of a launch under the write-through rule equal the one-slice kernel's, also where a trajectory
    is flagged (a NaN waypoint, a negative segment time)."""
    import torch
    B, S = 64 * 1024, 16
    wp, tm, _, _ = _inputs(B, S)
    wp, tm = wp.copy(), tm.copy()
    wp[100, 3, 1] = np.nan
    tm[64 * 700 + 9, 11] = -1.0
    d_wp, d_tm = torch.from_numpy(wp).cuda(), torch.from_numpy(tm).cuda()
    a = csp.solve_batch(d_wp, d_tm, order=4, want_status=True, want_max_dev=True)
    b = csp.solve_batch(d_wp, d_tm, order=4, want_status=True, want_max_dev=True, no_persistent=True)
    torch.cuda.synchronize()
    assert a.kernel == "fixed_o4_s16_f64", a.kernel
    st = a.status.cpu().numpy()
    assert st[100] & csp.TRAJ_NONFINITE and st[64 * 700 + 9] != 0
    assert np.count_nonzero(st) == 2
    assert torch.equal(a.status, b.status)
    assert torch.equal(_bits(a.max_dev), _bits(b.max_dev))
    assert torch.equal(_bits(a.coeffs), _bits(b.coeffs))
