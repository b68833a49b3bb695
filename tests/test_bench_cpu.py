"""CPU suite: what bench.py --dump-outputs writes, whole or as a fixed sample past its size limit."""
import numpy as np
import torch

import bench


def test_dump_writes_y_whole_or_a_fixed_sample(tmp_path, monkeypatch):
    y = torch.arange(1000, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "whole"), y)
    got = np.load(tmp_path / "whole" / "y.npy")
    assert got.dtype == np.float64 and np.array_equal(got, y.numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096 + 100 * 8)       # room for 100 doubles besides the header
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), y)
    s1 = np.load(tmp_path / "s1" / "y_sample.npy")
    assert s1.dtype == np.float64 and s1.size == 100 and np.all(np.diff(s1) > 0)   # distinct rows, in row order
    assert np.array_equal(s1, np.load(tmp_path / "s2" / "y_sample.npy"))            # the same rows every run
