"""-m gpu: the join step without its copy kernels and small launches (csrc/ivx_join.hip, ivx_regions_probe.hip, ivx_capi.hip).

What the tests pin, each against the CPU oracle's pair multiset:
  * the index header reaches the host through mapped memory (k_join_layout's mirror, k_join_regdesc's HDR_SLOW), with the
    build overlap on and off and with either build tail -- and ivx_index_layout, which reads the device's header, agrees;
  * with the overlap on the host decides between the lean fill pair and the general kernel after the index's tail has run:
    an index with an over-full region (HDR_SLOW) takes the general kernel, on its first fill and on its second;
  * a bad key id still fails the build itself and leaves the context usable;
  * the lean pair's last kernel hands the pair total and the fault word to the host (k_fill_rest's done-counter): exact at
    and around the capacity edge, after a count call (the planned fill, whose counter a memset clears) and call after call;
  * the occupancy bitmap's kernel, now queued behind the header wait, still fills the bitmap before the routing pass;
  * k_fill_fast's own chunk table (the scan of the regions' row counts) at 0, 1, 8191, 8192, 8193 and 16385 routed rows per
    region, with 256 and with 1024 partition digits;
  * rows for the rest lists, so that k_fill_rest finds pairs and publishes the total in the same launch;
  * host columns and host pair buffers.
Build sides hold 66 000 .. 70 000 rows: the overlap's tail fork wants 2^16, the LDS tail 2^14.  IVX_JOIN_PATH=regions sends
the small probe batches through the region path."""
import contextlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pair_set
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu

IVX_RP_ECAP = 6144                 # ivx_internal.hpp
FP_CHUNK = 8192                    # ivx_regions.hpp


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.set_build_overlap(False)
    c.close()


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


def cols(k, s, e):
    return (np.ascontiguousarray(k, np.uint32), np.ascontiguousarray(s, np.int32), np.ascontiguousarray(e, np.int32))


def cat(*sides):
    return tuple(np.concatenate([x[i] for x in sides]) for i in range(3))


def dev(c):
    import torch
    return [torch.from_numpy(x.view(np.int32)).cuda() for x in c]


def host(t):
    return t.cpu().numpy().view(np.uint32)


def want_of(b, p):
    wb, wp = orc.join(*b, *p, threads=4)
    return pair_set(wb, wp)


def fill_dev(ctx, ix, dp, total, extra=0):
    """a region-path fill of device columns into device buffers of total + extra pairs"""
    import torch
    ob = torch.empty(max(total + extra, 1), dtype=torch.int32, device="cuda"); op = torch.empty_like(ob)
    with env(IVX_JOIN_PATH="regions"):
        gb, gp = ctx.overlap_fill(ix, *dp, out=(ob, op))
    ctx.synchronize()
    return pair_set(host(gb), host(gp))


def same(got, wset):
    return len(got) == len(wset) and bool((got == wset).all())


def uniform_probes(rng, b, nk, n, maxlen=300):
    k = rng.integers(0, nk, n)
    lo, hi = int(b[1].min()) - 1000, int(b[1].max()) + 1000
    s = rng.integers(lo, hi, n)
    return cols(k, s, s + rng.integers(0, maxlen, n))


def regions_of(lay, b, nk):
    """(key, first coordinate, coordinates) of every probe region, clipped to the key's span of starts (k_join_layout)"""
    sh0, R = lay["sh0"], lay["rcells"]
    out = []
    for k in range(nk):
        st = b[1][b[0] == k].astype(np.int64)
        if not len(st):
            continue
        origin, last = int(st.min()), int(st.max())
        cells0 = ((last - origin) >> sh0) + 1
        for rc0 in range(0, cells0, R):
            lo = origin + (rc0 << sh0)
            hi = min(origin + ((min(rc0 + R, cells0)) << sh0) - 1, last)
            out.append((k, lo, hi - lo + 1))
    assert len(out) == lay["nreg"], (len(out), lay)
    return out


def routed_region(lay, b, nk, pk, ps):
    """the region a probe row with key pk and start ps is routed to (starts inside the key's span of build starts)"""
    sh0, R = lay["sh0"], lay["rcells"]
    origin, first, nxt = np.zeros(nk, np.int64), np.zeros(nk, np.int64), 0
    for k in range(nk):
        st = b[1][b[0] == k].astype(np.int64)
        if len(st):
            origin[k], first[k] = st.min(), nxt
            nxt += (((int(st.max()) - int(st.min())) >> sh0) + 1 + R - 1) // R
    assert nxt == lay["nreg"], (nxt, lay)
    return first[pk] + ((ps.astype(np.int64) - origin[pk]) >> sh0) // R


# ------------------------------------------------------------------ 1. header mirror, both tails, overlap on and off
HEADLINE_B = synth.gen_numpy(68_000, 1000, 24, 0x5EED0100)
HEADLINE_P = synth.gen_numpy(70_000, 150, 24, 0x5EED0101)


@pytest.fixture(scope="module")
def headline_want():
    return want_of(HEADLINE_B, HEADLINE_P)


@pytest.mark.parametrize("tail", ["default", "global"])
def test_overlap_on_and_off_make_the_same_index(ctx, headline_want, tail):
    db, dp = dev(HEADLINE_B), dev(HEADLINE_P)
    kv = {"IVX_BUILD": "global"} if tail == "global" else {}
    lays = []
    try:
        for overlap in (True, False):
            ctx.set_build_overlap(overlap)
            with env(**kv):
                ix = ctx.build(pyivx.KIND_OVERLAP, *db, n_keys=24)
            assert same(fill_dev(ctx, ix, dp, len(headline_want)), headline_want), (tail, overlap)
            lays.append(ix.layout())
            ix.free()
    finally:
        ctx.set_build_overlap(False)
    assert lays[0] == lays[1], lays
    assert lays[0]["lbuild"] == (0 if tail == "global" else 1) and lays[0]["slow"] == 0 and lays[0]["nreg"] > 0, lays


# ------------------------------------------------------------------ 2. the host picks the general kernel
def overfull_build():
    """66 000 short rows spread over 60 M coordinates and 7 000 inside 1 000 coordinates of them: one region's slice holds
    more than IVX_RP_ECAP entries, whatever cells the layout picks"""
    rng = np.random.default_rng(20)
    s = np.concatenate([rng.integers(0, 60_000_000, 66_000), 30_000_000 + rng.integers(0, 1000, 7_000)])
    return cols(np.zeros(len(s)), s, s + rng.integers(0, 100, len(s)))


def test_overfull_region_takes_the_general_kernel(ctx):
    b = overfull_build()
    assert int(((b[1] >= 30_000_000) & (b[1] < 30_001_000)).sum()) > IVX_RP_ECAP
    rng = np.random.default_rng(21)
    # (few probe rows on the crowded stretch: under 3.5 pairs per probe row the call takes the ring fill, not the dense one)
    st = np.concatenate([rng.integers(-500, 60_000_500, 69_700), 30_000_000 + rng.integers(-300, 1300, 300)])
    p = cols(np.zeros(len(st)), st, st + rng.integers(0, 60, len(st)))
    wset = want_of(b, p)
    assert 300 * 100 < len(wset) < 3 * len(st)                             # (the crowded region's rows are found)
    db, dp = dev(b), dev(p)
    ctx.set_build_overlap(True)
    try:
        ix = ctx.build(pyivx.KIND_OVERLAP, *db, n_keys=1)
        # the index's first fill waits for its tail, reads HDR_SLOW = 1 on the host and launches the general kernel alone
        assert same(fill_dev(ctx, ix, dp, len(wset)), wset)
        assert same(fill_dev(ctx, ix, dp, len(wset)), wset)                # the flag is known now
        lay = ix.layout()
        assert lay["slow"] == 1 and lay["nreg"] > 1, lay
        # another index on the same context afterwards: its own flag, not this one's
        ix2 = ctx.build(pyivx.KIND_OVERLAP, *dev(HEADLINE_B), n_keys=24)
        assert same(fill_dev(ctx, ix, dp, len(wset)), wset)                # (the mirror is ix2's now: the device decides)
        p2 = HEADLINE_P
        w2 = want_of(HEADLINE_B, p2)
        assert same(fill_dev(ctx, ix2, dev(p2), len(w2)), w2)
        assert ix2.layout()["slow"] == 0
        ix.free(); ix2.free()
    finally:
        ctx.set_build_overlap(False)


# ------------------------------------------------------------------ 3. a bad key id
def test_bad_key_fails_the_build_with_the_overlap_on(ctx, headline_want):
    bad = HEADLINE_B[0].copy(); bad[33_333] = 24                          # key = n_keys
    db, dp = dev(HEADLINE_B), dev(HEADLINE_P)
    dbad = dev((bad,))[0]
    ctx.set_build_overlap(True)
    try:
        with pytest.raises(pyivx.IvxError) as ei:
            ctx.build(pyivx.KIND_OVERLAP, dbad, db[1], db[2], n_keys=24)
        assert ei.value.status == pyivx.ERR_INVALID
        ix = ctx.build(pyivx.KIND_OVERLAP, *db, n_keys=24)
        assert same(fill_dev(ctx, ix, dp, len(headline_want)), headline_want)
        ix.free()
    finally:
        ctx.set_build_overlap(False)


# ------------------------------------------------------------------ 4. / 5. totals: capacity edges, planned fills, refills
def test_capacity_edges_and_totals(ctx, headline_want):
    import torch
    db, dp = dev(HEADLINE_B), dev(HEADLINE_P)
    total = len(headline_want)
    ctx.set_build_overlap(True)
    try:
        ix = ctx.build(pyivx.KIND_OVERLAP, *db, n_keys=24)
        with env(IVX_JOIN_PATH="regions"):
            assert ctx.overlap_count(ix, *dp) == total
            # (the count call left its routed rows: this fill is the planned one, and it fails -- the plan survives)
            ob = torch.empty(total - 1, dtype=torch.int32, device="cuda"); op = torch.empty_like(ob)
            with pytest.raises(pyivx.IvxError) as ei:
                ctx.overlap_fill(ix, *dp, out=(ob, op))
            assert ei.value.status == pyivx.ERR_CAPACITY and f"need {total} pairs" in str(ei.value)
        with env(IVX_JOIN_PATH="regions", IVX_NO_PLAN=1):
            with pytest.raises(pyivx.IvxError) as ei:
                ctx.overlap_fill(ix, *dp, out=(ob, op))
            assert ei.value.status == pyivx.ERR_CAPACITY and f"need {total} pairs" in str(ei.value)
        for extra in (0, 1):
            with env(IVX_NO_PLAN=1):
                assert same(fill_dev(ctx, ix, dp, total, extra), headline_want), extra
        ix.free()
    finally:
        ctx.set_build_overlap(False)


def test_count_then_fill_then_refills(ctx, headline_want):
    import torch
    db, dp = dev(HEADLINE_B), dev(HEADLINE_P)
    total = len(headline_want)
    ctx.set_build_overlap(True)
    try:
        ix = ctx.build(pyivx.KIND_OVERLAP, *db, n_keys=24)
        ob = torch.empty(total, dtype=torch.int32, device="cuda"); op = torch.empty_like(ob)
        with env(IVX_JOIN_PATH="regions"):
            assert ctx.overlap_count(ix, *dp) == total                     # the index's first probe: a count
            for _ in range(3):                                             # the planned fill, then two that route again
                ob.zero_(); op.zero_()
                gb, gp = ctx.overlap_fill(ix, *dp, out=(ob, op))
                ctx.synchronize()
                assert same(pair_set(host(gb), host(gp)), headline_want)
            assert ctx.overlap_count(ix, *dp) == total                     # and a planned fill on the settled index
            gb, gp = ctx.overlap_fill(ix, *dp, out=(ob, op))
            ctx.synchronize()
            assert same(pair_set(host(gb), host(gp)), headline_want)
        ix.free()
    finally:
        ctx.set_build_overlap(False)


# ------------------------------------------------------------------ 6. the occupancy bitmap behind the header wait
def test_filter_forced_and_off(ctx):
    """build rows on two far-apart stretches of one key and of another: most blocks of the bitmap stay empty, and most probe
    rows fall on them"""
    rng = np.random.default_rng(60)
    n = 66_000
    k = rng.integers(0, 2, n)
    s = np.where(rng.integers(0, 2, n) == 0, rng.integers(0, 2_000_000, n), rng.integers(90_000_000, 92_000_000, n))
    b = cols(k, s, s + rng.integers(0, 200, n))
    p = uniform_probes(rng, b, 2, 70_000)
    wset = want_of(b, p)
    assert 0 < len(wset)
    db, dp = dev(b), dev(p)
    ctx.set_build_overlap(True)
    try:
        got = {}
        for mode in ("force", "0"):
            with env(IVX_FILTER=mode):
                ix = ctx.build(pyivx.KIND_OVERLAP, *db, n_keys=2)
                got[mode] = fill_dev(ctx, ix, dp, len(wset))
                lay = ix.layout()
            assert (lay["fg"] != 0xFFFFFFFF) == (mode == "force"), lay
            ix.free()
        assert same(got["force"], wset) and same(got["0"], wset)
    finally:
        ctx.set_build_overlap(False)


# ------------------------------------------------------------------ 7. k_fill_fast's own chunk table
CHUNK_COUNTS = [FP_CHUNK, 0, FP_CHUNK + 1, 1, FP_CHUNK - 1, 2 * FP_CHUNK + 1, 0]


@pytest.mark.parametrize("nk", [1, 300], ids=["one_key_256_digits", "300_keys_1024_digits"])
def test_chunk_edges(ctx, nk):
    """probe rows dealt to the regions by count: full chunk, none, one row over, one row, one row short, two chunks and a
    row, none -- repeated over the regions for one key; once, on the first regions, for 300 keys (each at least a region)"""
    rng = np.random.default_rng(70 + nk)
    n = 68_000
    k = rng.integers(0, nk, n)
    s = rng.integers(0, 40_000_000 if nk == 1 else 400_000, n)
    b = cols(k, s, s + rng.integers(0, 60, n))
    db = dev(b)
    ctx.set_build_overlap(True)
    try:
        ix = ctx.build(pyivx.KIND_OVERLAP, *db, n_keys=nk)
        lay = ix.layout()                                                  # (waits for the tail; the fill below knows the flag from its own wait)
        regs = regions_of(lay, b, nk)
        assert lay["slow"] == 0 and lay["pk24"] == 1 and len(regs) >= len(CHUNK_COUNTS), lay
        assert (len(regs) > 255) == (nk == 300), lay
        pk, ps = [], []
        for i, (key, lo, width) in enumerate(regs):
            c = CHUNK_COUNTS[i % len(CHUNK_COUNTS)] if (nk == 1 or i < len(CHUNK_COUNTS)) else (i % 3)
            pk.append(np.full(c, key)); ps.append(lo + rng.integers(0, width, c))
        pk, ps = np.concatenate(pk), np.concatenate(ps)
        # the counts really are the regions': every probe start's region again from the layout's words alone -- the key's
        # first region + (start - origin >> sh0) / cells per region, as the routing pass computes it
        want_counts = [CHUNK_COUNTS[i % len(CHUNK_COUNTS)] if (nk == 1 or i < len(CHUNK_COUNTS)) else (i % 3) for i in range(len(regs))]
        assert np.array_equal(np.bincount(routed_region(lay, b, nk, pk, ps), minlength=len(regs)), want_counts)
        for c in (0, 1, FP_CHUNK - 1, FP_CHUNK, FP_CHUNK + 1, 2 * FP_CHUNK + 1):
            assert c in want_counts
        assert any(want_counts[i - 1] >= FP_CHUNK and want_counts[i] == 0 and want_counts[i + 1] >= FP_CHUNK for i in range(1, len(regs) - 1))
        order = rng.permutation(len(pk))
        p = cols(pk[order], ps[order], ps[order] + rng.integers(0, 40, len(pk)))
        wset = want_of(b, p)
        assert len(wset) > 0
        assert same(fill_dev(ctx, ix, dev(p), len(wset)), wset)
        ix.free()
    finally:
        ctx.set_build_overlap(False)


# ------------------------------------------------------------------ 8. rows for the rest lists
def test_rest_rows_find_pairs_and_publish(ctx):
    rng = np.random.default_rng(80)
    b = HEADLINE_B
    p0 = HEADLINE_P
    # rows of length 10 000 (past their slice's halo wherever they start near a region's end), one row with end < start on a
    # build row's start, one row that starts before its key's first build start and reaches into it
    k1 = rng.integers(0, 24, 3_000)
    s1 = rng.integers(int(b[1].min()), int(b[1].max()), len(k1))
    first0 = int(b[1][b[0] == 0].min())
    x = int(b[1][b[0] == 1][0])
    special = cols([1, 0], [x + 5, first0 - 700], [x - 5, first0 + 50])
    p = cat(p0, cols(k1, s1, s1 + 10_000), special)
    wset = want_of(b, p)
    n0 = len(p0[0])
    got_rows = np.unique(wset & np.uint64(0xFFFFFFFF))
    assert (got_rows >= n0).sum() > 100 and (n0 + len(k1) + 1) in got_rows   # the long rows match, and so does the early starter
    db, dp = dev(b), dev(p)
    ctx.set_build_overlap(True)
    try:
        ix = ctx.build(pyivx.KIND_OVERLAP, *db, n_keys=24)
        assert same(fill_dev(ctx, ix, dp, len(wset)), wset)
        assert same(fill_dev(ctx, ix, dp, len(wset), 1), wset)
        assert ix.layout()["slow"] == 0
        ix.free()
    finally:
        ctx.set_build_overlap(False)


# ------------------------------------------------------------------ 9. host columns, host pair buffers
def test_host_columns_and_buffers(ctx, headline_want):
    ctx.set_build_overlap(True)                                            # (host columns build without the overlap all the same)
    try:
        ix = ctx.build(pyivx.KIND_OVERLAP, *HEADLINE_B, n_keys=24)
        with env(IVX_JOIN_PATH="regions"):
            ob, op = ctx.overlap_fill(ix, *HEADLINE_P)                     # count, then the planned fill
            assert same(pair_set(ob, op), headline_want)
            ob, op = ctx.overlap_fill(ix, *HEADLINE_P, cap=len(headline_want) + 3)
            assert same(pair_set(ob, op), headline_want)
        assert ix.layout()["slow"] == 0
        ix.free()
    finally:
        ctx.set_build_overlap(False)
