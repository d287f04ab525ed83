"""CPU tests: what bench.py --dump-outputs writes (float64 .npy files, 64 MB at most, the same sample every time)."""
import os

import numpy as np

import bench


def test_small_outputs_are_written_whole(tmp_path):
    y = np.random.RandomState(1).rand(2, 1000)
    bench.dump_outputs(str(tmp_path), {"y": y}, bench.DUMP_LIMIT_BYTES)
    assert sorted(os.listdir(tmp_path)) == ["y.npy"]
    got = np.load(tmp_path / "y.npy")
    assert got.dtype == np.float64 and np.array_equal(got, y)


def test_large_outputs_are_sampled_under_the_limit(tmp_path):
    rng = np.random.RandomState(2)
    y = rng.rand(3, 3_000_000) + 1j * rng.rand(3, 3_000_000)  # 144 MB of complex128
    res = rng.rand(50)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"y": y, "residuals": res}, bench.DUMP_LIMIT_BYTES)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["residuals.npy", "y.npy", "y_index.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_LIMIT_BYTES
    for f in files:  # the same sample on every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    got, idx = np.load(tmp_path / "a" / "y.npy"), np.load(tmp_path / "a" / "y_index.npy").astype(np.int64)
    assert got.dtype == np.float64 and got.shape == (3, len(idx), 2) and len(idx) > 1_000_000
    assert np.array_equal(got[..., 0], y.real[:, idx]) and np.array_equal(got[..., 1], y.imag[:, idx])
    assert np.array_equal(np.load(tmp_path / "a" / "residuals.npy"), res)
