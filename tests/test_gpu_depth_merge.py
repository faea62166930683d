"""-m gpu: streaming depth() on the device (ivx_depth_profile_merge / ivx_depth_profile_blocks, csrc/ivx_depth_merge.hip),
bit-exact against tests/depth_merge_oracle.py and against the device's own one-shot calls on the inputs of both profiles.

Shapes sit where the merge kernel can go wrong.  With T = pyivx.DEPTH_MERGE_TILE elements of the virtual merged sequence per
workgroup: Sa + Sb around one and two tiles; all of A below all of B and the reverse (the partition points at their extremes);
identical position sets (every element tied, so every tile boundary splits a tie pair); thousands of keys with one or two
steps (tile boundaries on key changes: the carry is 0 there).  The blocks scan has tiles of 1024 steps."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_merge_oracle as mo  # noqa: E402
import depth_oracle as orc  # noqa: E402
import depth_per_base_oracle as pbo  # noqa: E402
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

T = pyivx.DEPTH_MERGE_TILE
M32 = 0xFFFFFFFF
BIG = 1 << 31                   # a key length no test position reaches, below 2^32 - 1: a segment's end event is clipped
DTS = (np.uint32, np.uint32, np.int32, np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


def read_both(p, ctx=None):
    """the profile's steps through both memory modes (asserted identical) -> (key, pos, cov, key_seen)"""
    host = p.read(ctx=ctx)
    dev = p.read(device=True, ctx=ctx)
    for h, d, dt in zip(host, dev, DTS):
        assert h.dtype == dt and np.array_equal(h, d.cpu().numpy().view(dt))
    return host


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def check_merge(ctx, pa, pb, whole=None, mctx=None):
    """pa + pb against the restatement on the two inputs' steps and, where given, the one-shot profile of `whole` -> the result"""
    m = pa.merge(pb, ctx=mctx)
    got = read_both(m)
    want = mo.merge_steps(read_both(pa), read_both(pb))
    same(got, want)
    assert m.steps() == len(want[0]) and m.n_keys == len(want[3])
    if whole is not None:
        p1 = ctx.depth_profile(**whole)
        assert p1.n_keys == m.n_keys
        same(got, read_both(p1))
        p1.free()
    return m


def rising(ctx, pos, n_keys=1, key=0):
    """a profile with one step per position of `pos` (distinct), coverage 1, 2, 3, ... -> (profile, kwargs)"""
    pos = np.asarray(pos, np.uint32)
    kw = dict(skey=np.full(len(pos), key, np.uint32), sstart=pos, send=np.full(len(pos), M32, np.uint32),
              sweight=np.ones(len(pos), np.int32), key_len=np.full(n_keys, BIG, np.uint32), n_keys=n_keys)
    p = ctx.depth_profile(**kw)
    assert p.steps() == len(pos)
    return p, kw


def merge_rising(ctx, pa, pb):
    a, ka = rising(ctx, pa)
    b, kb = rising(ctx, pb)
    m = check_merge(ctx, a, b, mo.concat_cases(dict(orc.pack_reads([]), **ka), dict(orc.pack_reads([]), **kb)))
    n = m.steps()
    for p in (a, b, m):
        p.free()
    return n


# ---------------------------------------------------------------------------------------------- random
@pytest.mark.parametrize("clip", [True, False])
def test_merge_random_pairs(ctx, clip):
    rng = np.random.default_rng(77 + clip)
    for _ in range(100):
        x, y = mo.random_pair(rng, max_pos=40, clip=clip)
        a, b = ctx.depth_profile(**x), ctx.depth_profile(**y)
        m = check_merge(ctx, a, b, mo.concat_cases(x, y))
        for p in (a, b, m):
            p.free()


def weighted(rng, n, n_keys=3, max_pos=3000):
    s = rng.integers(0, max_pos, n).astype(np.uint32)
    return dict(orc.pack_reads([]), skey=rng.integers(0, n_keys, n).astype(np.uint32), sstart=s,
                send=np.minimum(s + rng.integers(0, 200, n), max_pos - 1).astype(np.uint32),
                sweight=rng.integers(-4, 5, n).astype(np.int32), key_len=None, n_keys=n_keys, filter_flag=1796, min_mapq=0)


@pytest.mark.parametrize("seed", [1, 2])
def test_merge_multi_tile_with_ties(ctx, seed):
    rng = np.random.default_rng(seed)
    x, y = weighted(rng, 5000), weighted(rng, 5000)
    a, b = ctx.depth_profile(**x), ctx.depth_profile(**y)
    assert a.steps() + b.steps() > 2 * T
    m = check_merge(ctx, a, b, mo.concat_cases(x, y))
    assert m.steps() > T
    for p in (a, b, m):
        p.free()


# ---------------------------------------------------------------------------------------------- tile edges
@pytest.mark.parametrize("N", [1, T - 1, T, T + 1, 2 * T + 1])
def test_merge_tile_edges(ctx, N):
    q = 3 * np.arange(N, dtype=np.uint32)
    assert merge_rising(ctx, q[0::2], q[1::2]) == N             # interleaved position by position
    assert merge_rising(ctx, q[:N // 2], q[N // 2:]) == N       # all of A below all of B
    assert merge_rising(ctx, q[N // 2:], q[:N // 2]) == N       # ... and above


@pytest.mark.parametrize("S", [T // 2 + 1, T])
def test_merge_identical_position_sets(ctx, S):
    q = 5 + 2 * np.arange(S, dtype=np.uint32)
    assert merge_rising(ctx, q, q) == S


def test_merge_key_boundaries(ctx):
    nka, nkb = 3 * T, 3 * T - 5
    ka, kb = np.arange(nka, dtype=np.uint32), np.arange(nkb, dtype=np.uint32)
    key_len = np.full(nka, BIG, np.uint32)
    # A: one step (the end is clipped) or two per key; B: the same the other way round, with fewer keys
    x = dict(orc.pack_reads([]), skey=ka, sstart=np.full(nka, 5, np.uint32), send=np.where(ka % 2 == 0, 9, M32).astype(np.uint32),
             sweight=np.ones(nka, np.int32), key_len=key_len, n_keys=nka, filter_flag=1796, min_mapq=0)
    y = dict(orc.pack_reads([]), skey=kb, sstart=np.where(kb % 3 == 0, 5, 7).astype(np.uint32),
             send=np.where(kb % 2 == 1, 12, M32).astype(np.uint32), sweight=np.full(nkb, 2, np.int32),
             key_len=key_len[:nkb], n_keys=nkb, filter_flag=1796, min_mapq=0)
    a, b = ctx.depth_profile(**x), ctx.depth_profile(**y)
    assert a.n_keys == nka and b.n_keys == nkb and a.steps() == nka + nka // 2
    whole = mo.concat_cases(x, y)
    m = check_merge(ctx, a, b, whole)
    m2 = check_merge(ctx, b, a, whole)
    assert m.n_keys == nka and m2.n_keys == nka
    for p in (a, b, m, m2):
        p.free()


# ---------------------------------------------------------------------------------------------- values
def test_merge_with_the_negation(ctx):
    rng = np.random.default_rng(5)
    x = weighted(rng, 3000)
    y = dict(x, sweight=-x["sweight"])
    a, b = ctx.depth_profile(**x), ctx.depth_profile(**y)
    assert a.steps() > T // 2
    m = check_merge(ctx, a, b, mo.concat_cases(x, y))
    assert m.steps() == 0
    seen = m.read()[3]
    assert np.array_equal(seen, a.read()[3]) and seen.any()
    pos, cov = m.expand(1, 0, 5000)
    assert np.array_equal(pos, np.arange(5000, dtype=np.int32)) and not cov.any()
    for p in (a, b, m):
        p.free()


def test_merge_wraps_int32(ctx):
    x = dict(orc.pack_reads([]), **orc.pack_segments([(0, 5, 20, 0x7FFFFFFF)]), key_len=None, n_keys=1, filter_flag=1796, min_mapq=0)
    y = dict(orc.pack_reads([]), **orc.pack_segments([(0, 5, 20, 1), (0, 30, 40, 3)]), key_len=None, n_keys=1, filter_flag=1796, min_mapq=0)
    a, b = ctx.depth_profile(**x), ctx.depth_profile(**y)
    m = check_merge(ctx, a, b, mo.concat_cases(x, y))
    k, p, c, _ = m.read()
    assert list(zip(p.tolist(), c.tolist())) == [(5, -0x80000000), (21, 0), (30, 3), (41, 0)]
    for q in (a, b, m):
        q.free()


def test_merge_with_itself(ctx):
    # c = 1, then 1 - 2^31: doubled, the second step wraps onto the first one's value and disappears
    kw = dict(orc.pack_segments([(0, 5, M32, 1), (0, 10, M32, -0x80000000), (1, 3, 8, 7)]), key_len=np.array([BIG, BIG], np.uint32), n_keys=2)
    a = ctx.depth_profile(**kw)
    k, p, c, _ = a.read()
    assert list(zip(k.tolist(), p.tolist(), c.tolist())) == [(0, 5, 1), (0, 10, 1 - 0x80000000), (1, 3, 7), (1, 9, 0)]
    m = check_merge(ctx, a, a)
    k, p, c, _ = m.read()
    assert list(zip(k.tolist(), p.tolist(), c.tolist())) == [(0, 5, 2), (1, 3, 14), (1, 9, 0)]
    # ... and every c doubled where nothing wraps
    rng = np.random.default_rng(9)
    b = ctx.depth_profile(**weighted(rng, 4000))
    d = check_merge(ctx, b, b)
    sb, sd = b.read(), d.read()
    same(sd[:2], sb[:2])
    assert np.array_equal(sd[2], 2 * sb[2]) and np.array_equal(sd[3], sb[3])
    for q in (a, m, b, d):
        q.free()


def test_merge_empty_profiles(ctx):
    e1, _ = rising(ctx, [])
    e3 = ctx.depth_profile(**dict(orc.pack_segments([]), key_len=np.full(3, BIG, np.uint32), n_keys=3))
    a, _ = rising(ctx, [4, 9, 11], n_keys=2, key=1)
    want = read_both(a)
    for x, y, nk in ((e1, a, 2), (a, e1, 2), (e3, a, 3), (a, e3, 3)):
        m = check_merge(ctx, x, y)
        got = m.read()
        same(got[:3], want[:3])
        assert got[3].tolist() == [0, 1] + [0] * (nk - 2) and m.n_keys == nk
        assert m.expand(1, 0, 12)[1].tolist() == [0] * 4 + [1] * 5 + [2] * 2 + [3]
        m.free()
    m = check_merge(ctx, e1, e3)
    assert m.steps() == 0 and m.n_keys == 3 and m.read()[3].tolist() == [0, 0, 0]
    assert not m.expand(2, 0, 9)[1].any() and all(len(c) == 0 for c in m.blocks())
    for q in (e1, e3, a, m):
        q.free()


# ---------------------------------------------------------------------------------------------- use of the result
def test_use_of_a_merged_profile(ctx):
    rng = np.random.default_rng(12)
    cases = [weighted(rng, 2500, max_pos=20000) for _ in range(3)]
    ps = [ctx.depth_profile(**kw) for kw in cases]
    ab = check_merge(ctx, ps[0], ps[1], mo.concat_cases(cases[0], cases[1]))
    other = pyivx.Ctx(0)
    try:
        # a merge of a merge, made by a second context on the same device
        abc = check_merge(ctx, ab, ps[2], mo.concat_cases(mo.concat_cases(cases[0], cases[1]), cases[2]), mctx=other)
        assert abc.ctx is other
        st = read_both(abc, ctx=ctx)
        for key, first, n in ((0, 0, 20010), (1, 4095, 4098), (2, 19990, 40), (1, 7, 1)):
            for skip in (False, True):
                wp, wc = pbo.expand_steps(st, key, first, n, skip_pos0=skip)
                for c in (ctx, other):
                    gp, gc = abc.expand(key, first, n, skip_pos0=skip, ctx=c)
                    assert np.array_equal(gp, wp) and np.array_equal(gc, wc)
        same(abc.blocks(ctx=ctx), mo.blocks_of_steps(st))
        abc.free()
    finally:
        other.close()
    for q in ps + [ab]:
        q.free()


# ---------------------------------------------------------------------------------------------- accounting
def test_accounting_and_memory_limit():
    c = pyivx.Ctx(0)
    try:
        rng = np.random.default_rng(3)
        a, b = c.depth_profile(**weighted(rng, 3000)), c.depth_profile(**weighted(rng, 3000))
        before_metrics = c.metrics()["build_mem_used"]
        m = a.merge(b)                                              # (also grows the scratch to what this merge needs)
        nbytes = m.device_bytes
        assert nbytes >= 3 * 4 * m.steps() + 4 * 4 + 3
        assert c.metrics()["build_mem_used"] - before_metrics == nbytes
        with_m = c.reserved_bytes()
        want = m.read()
        m.free()
        base = c.reserved_bytes()
        assert with_m - base == nbytes
        c.set_memory_limit(base + nbytes - 1)
        with pytest.raises(pyivx.IvxError) as ei:
            a.merge(b)
        assert ei.value.status == pyivx.ERR_OOM and "Resources exhausted" in str(ei.value)
        assert c.reserved_bytes() == base
        c.set_memory_limit(0)
        m = a.merge(b)
        assert c.reserved_bytes() == base + nbytes
        same(m.read(), want)
        m.free()
        assert c.reserved_bytes() == base
        for q in (a, b):
            q.free()
    finally:
        c.close()


def test_wrong_handles(ctx):
    L = pyivx.lib()
    a, _ = rising(ctx, [1, 2, 3])
    ix = ctx.build(pyivx.KIND_OVERLAP, np.zeros(3, np.uint32), np.array([1, 5, 9], np.int32), np.array([4, 8, 12], np.int32), n_keys=1)
    h, m = C.c_void_p(), C.c_uint64(0)
    assert L.ivx_depth_profile_merge(ctx.h, a.h, ix.h, C.byref(h)) == pyivx.ERR_UNSUPPORTED and not h.value
    assert L.ivx_depth_profile_merge(ctx.h, ix.h, a.h, C.byref(h)) == pyivx.ERR_UNSUPPORTED and not h.value
    assert L.ivx_depth_profile_merge(ctx.h, a.h, None, C.byref(h)) == pyivx.ERR_INVALID and not h.value
    assert L.ivx_depth_profile_merge(ctx.h, None, a.h, C.byref(h)) == pyivx.ERR_INVALID and not h.value
    assert L.ivx_depth_profile_merge(ctx.h, a.h, a.h, None) == pyivx.ERR_INVALID
    assert L.ivx_depth_profile_blocks(ctx.h, ix.h, pyivx.MEM_HOST, None, None, None, None, 0, C.byref(m)) == pyivx.ERR_UNSUPPORTED
    assert L.ivx_depth_profile_blocks(ctx.h, None, pyivx.MEM_HOST, None, None, None, None, 0, C.byref(m)) == pyivx.ERR_INVALID
    assert L.ivx_depth_profile_blocks(ctx.h, a.h, pyivx.MEM_HOST, None, None, None, None, 0, None) == pyivx.ERR_INVALID
    assert L.ivx_depth_profile_blocks(ctx.h, a.h, 7, None, None, None, None, 0, C.byref(m)) == pyivx.ERR_INVALID
    ix.free()
    d = check_merge(ctx, a, a)
    assert d.read()[2].tolist() == [2, 4, 6]
    a.free()
    d.free()


# ---------------------------------------------------------------------------------------------- blocks
def check_blocks(ctx, kw):
    p = ctx.depth_profile(**kw)
    host = p.blocks()
    dev = p.blocks(device=True)
    for h, d, dt in zip(host, dev, (np.uint32, np.uint32, np.uint32, np.int32)):
        assert h.dtype == dt and np.array_equal(h, d.cpu().numpy().view(dt))
    same(host, ctx.depth(**kw))
    same(host, orc.depth_loop(**orc.oracle_kw(kw)))
    p.free()
    return host


@pytest.mark.parametrize("clip", [True, False])
def test_blocks_random(ctx, clip):
    rng = np.random.default_rng(77 + clip)                          # (the cases of test_merge_random_pairs)
    for _ in range(100):
        for kw in mo.random_pair(rng, max_pos=40, clip=clip):
            check_blocks(ctx, kw)


@pytest.mark.parametrize("S", [1, 2, 1023, 1024, 1025])
def test_blocks_scan_edges(ctx, S):
    q = 2 * np.arange(S, dtype=np.uint32)
    kw = dict(skey=np.zeros(S, np.uint32), sstart=q, send=np.full(S, M32, np.uint32), sweight=np.ones(S, np.int32),
              key_len=np.array([BIG], np.uint32), n_keys=1)
    k, s, e, c = check_blocks(ctx, kw)
    assert len(k) == S - 1 and c.tolist() == list(range(1, S))
    # ... and over two keys, the key change inside the run
    kw = dict(kw, skey=(np.arange(S) >= S // 2).astype(np.uint32), key_len=np.array([BIG, BIG], np.uint32), n_keys=2)
    assert len(check_blocks(ctx, kw)[0]) == max(S - 2, 0)


def test_blocks_open_and_cancelled_keys(ctx):
    # key 0: clipped at its length, the coverage never returns to 0 and the last open block is lost; key 1: events cancel;
    # key 2: an ordinary block
    kw = dict(orc.pack_segments([(0, 10, 19, 1), (0, 15, 80, 2), (1, 4, 9, 3), (1, 4, 9, -3), (2, 1, 2, 5)]),
              key_len=np.array([50, 50, 50], np.uint32), n_keys=3)
    k, s, e, c = check_blocks(ctx, kw)
    assert list(zip(k.tolist(), s.tolist(), e.tolist(), c.tolist())) == [(0, 10, 14, 1), (0, 15, 19, 3), (2, 1, 2, 5)]
    p = ctx.depth_profile(**kw)
    assert p.read()[3].tolist() == [1, 1, 1] and p.read()[2].tolist() == [1, 3, 2, 5, 0]
    p.free()


def test_blocks_capacity_protocol(ctx):
    kw = dict(orc.pack_segments([(0, 10, 19, 3), (0, 15, 24, -1), (1, 0, 4, -2)]), n_keys=2)
    p = ctx.depth_profile(**kw)
    want = ctx.depth(**kw)
    n = len(want[0])
    assert n == 4
    L = pyivx.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    m = C.c_uint64(0)
    assert L.ivx_depth_profile_blocks(ctx.h, p.h, pyivx.MEM_HOST, None, None, None, None, 0, C.byref(m)) == pyivx.OK and m.value == n
    bufs = [np.full(8, 77, dt) for dt in (np.uint32, np.uint32, np.uint32, np.int32)]
    m = C.c_uint64(0)
    assert L.ivx_depth_profile_blocks(ctx.h, p.h, pyivx.MEM_HOST, *map(ptr, bufs), n - 1, C.byref(m)) == pyivx.ERR_CAPACITY
    assert m.value == n and "too small" in L.ivx_last_error(ctx.h).decode() and all((b == 77).all() for b in bufs)
    with pytest.raises(pyivx.IvxError) as ei:
        p.blocks(cap=n - 1)
    assert ei.value.status == pyivx.ERR_CAPACITY and f"needed {n}" in str(ei.value)
    assert L.ivx_depth_profile_blocks(ctx.h, p.h, pyivx.MEM_HOST, *map(ptr, bufs), 8, C.byref(m)) == pyivx.OK and m.value == n
    for b, w in zip(bufs, want):
        assert np.array_equal(b[:n], w) and (b[n:] == 77).all()
    # each output NULL on its own, in both memory modes
    for i in range(4):
        outputs = tuple(j != i for j in range(4))
        for dev in (False, True):
            got = p.blocks(device=dev, outputs=outputs)
            assert got[i] is None
            for j in range(4):
                if j != i:
                    g = got[j].cpu().numpy().view(want[j].dtype) if dev else got[j]
                    assert np.array_equal(g, want[j])
    p.free()
