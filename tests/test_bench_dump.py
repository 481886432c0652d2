"""bench.py --dump-outputs on host tensors: layout, dtype, the size cap and the seeded sample (the GPU run of the flag is
tests/test_gpu_bench_flow.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(d):
    return np.load(os.path.join(d, "coeffs.npy")), np.load(os.path.join(d, "coeffs_index.npy"))


def test_dump_writes_the_whole_batch_while_it_fits(tmp_path):
    import torch
    B, S, o = 100, 16, 4
    out = torch.from_numpy(np.random.default_rng(1).normal(size=(B, S, 3, 2 * o)))
    bench.dump_outputs(str(tmp_path), out, B, S, o, False)
    co, idx = _load(tmp_path)
    assert co.dtype == np.float64 and idx.dtype == np.float64
    assert np.array_equal(co, out.numpy()) and np.array_equal(idx, np.arange(B))


def test_dump_of_a_segment_major_run_is_trajectory_major(tmp_path):
    import torch
    B, S, o = 70, 8, 3
    ref = np.random.default_rng(2).normal(size=(B, S, 3, 2 * o))
    out = torch.from_numpy(np.ascontiguousarray(ref.transpose(1, 0, 2, 3)))   # [S][B][3][2o]
    bench.dump_outputs(str(tmp_path), out, B, S, o, True)
    co, idx = _load(tmp_path)
    assert np.array_equal(co, ref) and np.array_equal(idx, np.arange(B))


def test_dump_of_a_large_batch_is_a_fixed_seeded_sample_under_64_mb(tmp_path):
    import torch
    B, S, o = 20000, 16, 4                                                       # 61 MB of coefficients
    out = torch.from_numpy(np.random.default_rng(3).normal(size=(B, S, 3, 2 * o)))
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), out, B, S, o, False)
    bench.dump_outputs(str(b), out, B, S, o, False)
    co, idx = _load(a)
    co_b, idx_b = _load(b)
    assert np.array_equal(co, co_b) and np.array_equal(idx, idx_b)              # same arguments, same sample
    n = bench.DUMP_BYTES // (S * 3 * 2 * o * 8)
    assert idx.shape == (n,) and co.shape == (n, S, 3, 2 * o) and n < B
    k = idx.astype(np.int64)
    assert np.array_equal(k, idx) and np.all(np.diff(k) > 0) and k[0] >= 0 and k[-1] < B
    assert np.array_equal(co, out.numpy()[k])
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 << 20
