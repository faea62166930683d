"""-m gpu: bench.py as it is run for every change -- a plain run prints the headline line and nothing of --full, and
--dump-outputs writes the pairs of its last timed step, which equal the oracle's pairs on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_pairs_of_its_timed_step(tmp_path):
    n_probe = 2_000_000
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--probe-rows", str(n_probe), "--dump-outputs", str(tmp_path)]
    # a fresh child: this process may already hold the GPU
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "overlap-pairs/s" and out["higher_is_better"] is True and out["dtype"] == "int32"
    assert not {"ops", "cpu_baseline", "parity", "two_call_ms", "e2e", "strong"} & set(out)

    b, q = np.load(tmp_path / "build_idx.npy"), np.load(tmp_path / "probe_idx.npy")
    assert b.dtype == np.float64 and q.dtype == np.float64 and len(b) == len(q) == out["config"]["pairs_per_gpu"]
    seed = 0x5EED0000 + 2 * 2                                     # the join workload's weak-scaling seed, rank 0
    bk, bs, be = synth.gen_numpy(1_000_000, 1000, 24, seed)
    pk, ps, pe = synth.gen_numpy(n_probe, 150, 24, seed + 1)
    want = orc.pair_keys(*orc.join(bk, bs, be, pk, ps, pe, threads=min(16, os.cpu_count() or 1)))
    got = (b.astype(np.uint64) << np.uint64(32)) | q.astype(np.uint64)
    assert np.array_equal(got, want)
