"""CPU-only: bench.py's --dump-outputs writer (float64 files, the 64 MB cap, a fixed sample that keeps the columns of one
output aligned) and the options a plain and a --full run are started with."""
import os
import subprocess
import sys

import numpy as np
import torch

from conftest import ROOT

import bench


def test_small_outputs_are_written_whole_in_float64(tmp_path):
    a = torch.arange(1000, dtype=torch.int32) * 7 - 3
    b = torch.tensor([0, (1 << 40) + 1, -1], dtype=torch.int64)
    bench.dump_outputs(str(tmp_path / "d"), {"a": a, "b": b})
    ga, gb = np.load(tmp_path / "d" / "a.npy"), np.load(tmp_path / "d" / "b.npy")
    assert ga.dtype == np.float64 and gb.dtype == np.float64
    assert np.array_equal(ga, a.numpy()) and np.array_equal(gb, b.numpy())


def test_large_outputs_are_a_fixed_aligned_sample_under_64_mb(tmp_path):
    n = 5_000_000                                           # 2 x 40 MB as float64: over the cap
    x = torch.arange(n, dtype=torch.int64)
    arrays = {"x": x, "y": 3 * x + 1, "z": torch.arange(10, dtype=torch.int32)}
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    files = [tmp_path / "one" / f"{k}.npy" for k in arrays]
    assert sum(os.path.getsize(f) for f in files) <= 64 << 20
    gx, gy, gz = (np.load(f) for f in files)
    assert 0 < len(gx) < n and len(gx) == len(gy)
    assert np.array_equal(gy, 3 * gx + 1)                   # rows of one length share the drawn rows
    assert (np.diff(gx) >= 0).all()                         # kept in row order
    assert np.array_equal(gz, np.arange(10))                # a small array stays whole
    for k in arrays:                                        # the same rows from run to run
        assert np.array_equal(np.load(tmp_path / "one" / f"{k}.npy"), np.load(tmp_path / "two" / f"{k}.npy"))


def test_bench_offers_full_and_dump_outputs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout and "--steps" in p.stdout
