"""-m gpu: intersect with contigs sharded over three ranks (`sharded.ShardedRanges.intersect`) equals the single-rank call on
the whole job, column for column.  The ranks share the box's one GPU, so the process group is gloo and the exchanged
tensors cross it through host memory (as in tests/test_gpu_multirank.py); the per-rank compute is the HIP library, the
sharding, the row translation and the splice are the lines subtract uses."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

WORLD, NK, NL, NR = 3, 6, 5000, 1500


def _job():
    import intersect_oracle as io
    return io.random_sides(np.random.default_rng(77), NL, NR, NK, span=60_000, max_len=80)


def _worker(rank, world, port, ret):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
    import torch
    import torch.distributed as dist
    import pyivx
    import shard
    import sharded
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    (lk, ls, le), (rk, rs, re) = _job()
    dev = lambda k, s, e: (torch.from_numpy(k.view(np.int32).copy()).cuda(), torch.from_numpy(s.copy()).cuda(), torch.from_numpy(e.copy()).cuda())
    rank_of = shard.assign_keys_lpt(np.bincount(lk, minlength=NK) + np.bincount(rk, minlength=NK), world)
    ml, mr = rank_of[lk] == rank, rank_of[rk] == rank
    rows_l = torch.from_numpy(np.flatnonzero(ml).astype(np.int32)).cuda()
    ctx = pyivx.Ctx(0)
    # device-mode calls return with kernels in flight on the context's stream: torch's own (as bench.py sets it), so that the
    # torch work of the splice and of the comparison below is ordered behind them
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    sr = sharded.ShardedRanges(dist, ctx, NK)
    ok = {"rows": int(ml.sum())}
    for strict in (False, True):
        got = sr.intersect(dev(lk[ml], ls[ml], le[ml]), rows_l, dev(rk[mr], rs[mr], re[mr]), strict=strict)
        want = ctx.intersect(*dev(lk, ls, le), *dev(rk, rs, re), n_keys=NK, strict=strict)
        ctx.synchronize()
        ok[f"same{strict}"] = all(g.shape == w.shape and bool((g == w).all()) for g, w in zip(got, want))
        ok[f"pieces{strict}"] = int(want[0].numel())
    ctx.close()
    flags = [None] * world
    dist.all_gather_object(flags, ok)
    if rank == 0:
        ret["flags"] = flags
    dist.destroy_process_group()


def test_three_ranks_equal_the_single_rank_result():
    import torch.multiprocessing as mp
    import intersect_oracle as io
    left, right = _job()
    n_want = {s: len(io.walk(left, right, s)[0]) for s in (False, True)}
    assert min(n_want.values()) > 500
    with mp.Manager() as m:
        ret = m.dict()
        mp.spawn(_worker, args=(WORLD, 37500 + os.getpid() % 2000, ret), nprocs=WORLD, join=True)   # fresh children: each opens the GPU itself
        flags = list(ret["flags"])
    assert len(flags) == WORLD and sum(f["rows"] for f in flags) == NL and all(f["rows"] for f in flags)
    for f in flags:
        for s in (False, True):
            assert f[f"same{s}"] and f[f"pieces{s}"] == n_want[s], f
