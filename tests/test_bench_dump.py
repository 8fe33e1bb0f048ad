"""bench.py --dump-outputs: what is written, in which types, and within which budget (host only)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402  (numpy only at import time)


def test_small_outputs_are_written_whole(tmp_path):
    y = np.arange(1000, dtype=np.float32) * 0.5
    p = np.arange(11, dtype=np.uint64)
    bench.dump_outputs(str(tmp_path), {"y": y, "rowptr": p})
    assert np.array_equal(np.load(tmp_path / "y.npy"), y) and np.load(tmp_path / "y.npy").dtype == np.float32
    r = np.load(tmp_path / "rowptr.npy")
    assert r.dtype == np.float64 and np.array_equal(r, p.astype(np.float64))
    assert sorted(os.listdir(tmp_path)) == ["rowptr.npy", "y.npy"]


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path):
    n = 10_000_000                          # config 3's y: 80 MB of float64
    y = np.linspace(-1.0, 1.0, n)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"y": y})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["y.npy", "y_positions.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BUDGET_BYTES
    pos = np.load(tmp_path / "a" / "y_positions.npy")
    assert pos.dtype == np.float64 and np.all(np.diff(pos) > 0) and pos[-1] < n and pos.size > n // 4
    assert np.array_equal(np.load(tmp_path / "a" / "y.npy"), y[pos.astype(np.int64)])
    for f in files:                         # same positions, same values: two runs compare output for output
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
