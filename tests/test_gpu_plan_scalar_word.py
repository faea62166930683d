"""-m gpu: the one scalar word of the context that outlives its call (csrc/ivx_scalars.hpp: SC_UNSORTED).

With the flat partition (IVX_PART=two) a region COUNT call leaves its routed probe rows in the context for the fill call that
follows, and with them a pointer to the routing pass's `unsorted` word.  Calls in between that write scalar words of their own
but take none of the routed rows' scratch slots -- bits_mark and take_fixed on device memory -- must leave that word alone:
the planned fill then returns the pairs it returns without them, which are the oracle's."""
import contextlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pair_set
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def build(ctx):
    """200 k rows of length 255 every 64 coordinates, one key (test_gpu_region_forms.py: level0_lean_build): some 50 regions"""
    n = 200_000
    s = np.arange(n, dtype=np.int64) * 64
    b = (np.zeros(n, np.uint32), s.astype(np.int32), (s + 255).astype(np.int32))
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    assert ix.layout()["nreg"] > 1
    yield b, ix
    ix.free()


@pytest.mark.parametrize("order", ["shuffled", "region_order"])
def test_planned_fill_survives_calls_that_write_scalar_words(ctx, build, order):
    import torch
    b, ix = build
    rng = np.random.default_rng(7)
    x = rng.integers(0, int(b[1].max()), 150_000)
    if order == "region_order":
        x = np.sort(x)                                  # one key: ascending starts are ascending regions, *unsorted stays 0
    p = (np.zeros(len(x), np.uint32), x.astype(np.int32), x.astype(np.int32))
    wb, wp = orc.join(*b, *p, threads=4)
    wset = pair_set(wb, wp)
    d = [torch.from_numpy(c.view(np.int32)).cuda() for c in p]
    host = lambda t: t.cpu().numpy().view(np.uint32)

    # what sits between the two calls: both raise and read back a flag word, neither takes a scratch slot
    idx = torch.from_numpy(rng.integers(0, 4096, 1000).astype(np.int32)).cuda()
    bits = torch.zeros(4096 // 32, dtype=torch.int32, device="cuda")
    src = torch.arange(4096, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                            # (the context runs on a stream of its own)

    def between():
        ctx.bits_mark(idx, bits, 4096)
        out, _ = ctx.take_fixed(src, idx)
        assert (out == idx).all()

    with env(IVX_JOIN_PATH="regions", IVX_PART="two"):
        total = ctx.overlap_count(ix, *d)
        ob0, op0 = ctx.overlap_fill(ix, *d, cap=total)              # planned, nothing in between
        ms_planned = ctx.last_kernel_ms()
        total1 = ctx.overlap_count(ix, *d)
        between()
        ob1, op1 = ctx.overlap_fill(ix, *d, cap=total)              # planned, behind the two calls
        ms_between = ctx.last_kernel_ms()
        with env(IVX_NO_PLAN=1):
            ob2, op2 = ctx.overlap_fill(ix, *d, cap=total)          # routes its rows again
    print(f"{order}: fill kernels {ms_planned:.3f} ms planned, {ms_between:.3f} ms planned behind the calls")
    assert total == total1 == len(wb)
    s0, s1, s2 = pair_set(host(ob0), host(op0)), pair_set(host(ob1), host(op1)), pair_set(host(ob2), host(op2))
    assert len(s0) == total and (s0 == wset).all()
    assert len(s1) == total and (s1 == s0).all()                    # the same pairs with and without the calls in between
    assert len(s2) == total and (s2 == wset).all()
