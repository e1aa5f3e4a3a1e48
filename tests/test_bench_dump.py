"""bench.py --dump-outputs: the lanes it writes and the files it leaves (host side; the GPU run is bench.py itself)."""
import os

import numpy as np
import torch

import bench


def test_dump_lanes_are_all_lanes_or_a_fixed_sample_within_the_budget():
    assert np.array_equal(bench._dump_lanes(1000, 8 * 300), np.arange(1000))
    row_bytes = 8 * 300
    lanes = bench._dump_lanes(65536, row_bytes)
    assert 0 < len(lanes) < 65536 and len(lanes) * row_bytes <= bench.DUMP_MAX_BYTES
    assert np.all(np.diff(lanes) > 0) and lanes[-1] < 65536
    assert np.array_equal(lanes, bench._dump_lanes(65536, row_bytes))


def test_write_outputs_leaves_float_arrays_named_after_the_fields(tmp_path):
    lanes = np.array([0, 3, 5])
    snap = {"q": torch.arange(6, dtype=torch.float64).reshape(2, 3),
            "imu": torch.ones((1, 3), dtype=torch.float32),
            "status": torch.tensor([[0, 1, 16]], dtype=torch.int32)}
    out = str(tmp_path / "dump")
    bench.write_outputs(snap, lanes, out)
    assert sorted(os.listdir(out)) == ["imu.npy", "lanes.npy", "q.npy", "status.npy"]
    assert np.load(os.path.join(out, "q.npy")).dtype == np.float64
    assert np.load(os.path.join(out, "imu.npy")).dtype == np.float32
    status = np.load(os.path.join(out, "status.npy"))
    assert status.dtype == np.float64 and np.array_equal(status, [[0, 1, 16]])
    assert np.array_equal(np.load(os.path.join(out, "lanes.npy")), lanes)


def test_lanes_gone_non_finite_are_left_out_of_the_dump():
    lanes = np.array([2, 4, 7, 9])
    nan, inf = float("nan"), float("inf")
    snap = {"q": torch.tensor([[0.0, nan, 2.0, 3.0], [1.0, 1.0, 1.0, 1.0]], dtype=torch.float64),
            "a": torch.tensor([[0.0, 1.0, 2.0, inf]], dtype=torch.float32),
            "status": torch.tensor([[0, 1, 2, 0]], dtype=torch.int32)}
    kept, kept_lanes, dropped = bench.finite_lanes(snap, lanes)
    assert dropped == 2 and np.array_equal(kept_lanes, [2, 7])
    assert torch.equal(kept["q"], torch.tensor([[0.0, 2.0], [1.0, 1.0]], dtype=torch.float64))
    assert kept["a"].dtype == torch.float32 and torch.equal(kept["status"], torch.tensor([[0, 2]], dtype=torch.int32))
    assert all(torch.isfinite(t.double()).all() for t in kept.values())
