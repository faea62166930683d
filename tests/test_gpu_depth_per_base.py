"""-m gpu: depth profiles (ivx_depth_profile_*, csrc/ivx_depth_expand.hip) bit-exact against the CPU restatements of
tests/depth_per_base_oracle.py: the steps a build keeps, and windows expanded to (position Int32, coverage Int16) rows.

Window shapes sit where the expand kernel changes path.  With T = pyivx.DEPTH_EXPAND_TILE outputs per workgroup: a thread
owns one 16-byte line (8 coverages, 4 positions) of the OUTPUT, so the caller's pointer alignment (buffers offset by 0, 1, 3, 7
elements) and n decide which lines leave as one wide store and which element by element; a tile is a constant fill, or goes
through the LDS image when a step falls inside it; a step before the window is the carry-in."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_oracle as orc  # noqa: E402
import depth_per_base_oracle as pbo  # noqa: E402
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

T = pyivx.DEPTH_EXPAND_TILE
NULL = pyivx.NULL_IDX
M32 = 0xFFFFFFFF
op = lambda n, c: (n << 4) | c


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


def to_device(kw):
    import torch
    out = {}
    for k, v in kw.items():
        if isinstance(v, np.ndarray):
            v = torch.from_numpy(np.ascontiguousarray(v).view(np.int32) if v.dtype == np.uint32 else np.ascontiguousarray(v)).to("cuda:0")
        out[k] = v
    return out


def read_both(p):
    """the profile's steps through both memory modes (asserted identical) -> (key, pos, cov, key_seen)"""
    host = p.read()
    dev = p.read(device=True)
    for h, d, dt in zip(host, dev, (np.uint32, np.uint32, np.int32, np.uint8)):
        assert h.dtype == dt and np.array_equal(h, d.cpu().numpy().view(dt))
    return host


def check_steps(ctx, kw, device_too=True):
    want = pbo.steps(kw["n_keys"], **orc.oracle_kw(kw))
    for dev in ((False, True) if device_too else (False,)):
        p = ctx.depth_profile(**(to_device(kw) if dev else kw))
        got = read_both(p)
        assert p.steps() == len(want[0])
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        p.free()
    return want


# ---------------------------------------------------------------------------------------------- steps
@pytest.mark.parametrize("clip", [True, False])
def test_steps_random(ctx, clip):
    rng = np.random.default_rng(31 + clip)
    for i in range(100):
        check_steps(ctx, orc.random_case(rng, clip=clip, max_pos=40), device_too=i % 4 == 0)


@pytest.mark.parametrize("E", [1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097])
def test_steps_scan_edges(ctx, E):
    # E one-op reads: 2 E events, E ops -- the counts at which the scans over ops and over events change shape
    rng = np.random.default_rng(E)
    ops = ((rng.integers(0, 6, E) << 4) | np.where(rng.random(E) < 0.6, 0, rng.integers(0, 16, E))).astype(np.uint32)
    kw = dict(rkey=rng.integers(0, 2, E).astype(np.uint32), rpos=rng.integers(0, 200, E).astype(np.uint32),
              rflags=np.where(rng.random(E) < 0.1, 4, 0).astype(np.uint32), rmapq=rng.integers(0, 61, E).astype(np.uint32),
              cigar_offsets=(4 * np.arange(E + 1)).astype(np.int32), cigar_ops=ops, min_mapq=5, n_keys=2)
    check_steps(ctx, kw)
    # ... and E weighted segments: exactly 2 E events
    segs = dict(skey=rng.integers(0, 2, E).astype(np.uint32), sstart=rng.integers(0, 300, E).astype(np.uint32),
                sweight=rng.integers(-3, 4, E).astype(np.int32), n_keys=2)
    segs["send"] = (segs["sstart"] + rng.integers(0, 20, E)).astype(np.uint32)
    check_steps(ctx, segs)


def test_key_seen(ctx):
    reads = [(0, 5, 0, 60, [op(0, 0)]),                     # only a zero-length M: two events that cancel
             (1, 5, 4, 60, [op(10, 0)]), (1, 9, 0, 3, [op(10, 0)]),     # filtered: by flag, by mapq
             (2, 100, 0, 60, [op(10, 0)]),                  # beyond key_len[2]
             (3, 50, 0, 60, [op(10, 0)]),                   # starts at key_len[3] exactly: the start stays, the end is clipped
             (4, 7, 0, 60, [op(2, 0)])]
    kw = dict(orc.pack_reads(reads), key_len=np.array([50, 50, 50, 50, 50, 50], np.uint32), min_mapq=5, n_keys=6)
    k, p, c, seen = check_steps(ctx, kw)
    assert seen.tolist() == [1, 0, 0, 1, 1, 0]
    assert list(zip(k.tolist(), p.tolist(), c.tolist())) == [(3, 50, 1), (4, 7, 1), (4, 9, 0)]
    # a zero-weight segment touches its key, a skipped one touches nothing (not even key 0)
    kw = dict(orc.pack_segments([(1, 3, 9, 0), (NULL, 0, 5, 2)]), n_keys=2)
    assert check_steps(ctx, kw)[3].tolist() == [0, 1]


def test_capacity_protocol_and_empty_profile(ctx):
    kw = dict(orc.pack_segments([(0, 10, 19, 3), (0, 15, 24, -1), (1, 0, 4, -2)]), n_keys=2)
    p = ctx.depth_profile(**kw)
    L = pyivx.lib()
    m = C.c_uint64(0)
    assert L.ivx_depth_profile_read(ctx.h, p.h, pyivx.MEM_HOST, None, None, None, None, 0, C.byref(m)) == pyivx.OK and m.value == 6
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    k, q, c, seen = np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.full(8, 77, np.int32), np.full(2, 9, np.uint8)
    assert L.ivx_depth_profile_read(ctx.h, p.h, pyivx.MEM_HOST, ptr(k), ptr(q), ptr(c), ptr(seen), 5, C.byref(m)) == pyivx.ERR_CAPACITY
    assert m.value == 6 and "too small" in L.ivx_last_error(ctx.h).decode() and seen.tolist() == [1, 1] and (c == 77).all()
    assert L.ivx_depth_profile_read(ctx.h, p.h, pyivx.MEM_HOST, None, ptr(q), ptr(c), None, 8, C.byref(m)) == pyivx.OK and m.value == 6
    assert q[:6].tolist() == [10, 15, 20, 25, 0, 5] and c[:6].tolist() == [3, 2, -1, 0, -2, 0] and c[6] == 77
    assert p.device_bytes > 0
    p.free()
    # no event at all: an empty profile that still expands (to zeros)
    for ekw in (dict(n_keys=3), dict(orc.pack_reads([(0, 1, 4, 60, [op(5, 0)])]), n_keys=3), dict(orc.pack_segments([(NULL, 1, 4, 2)]), n_keys=3)):
        for dev in (False, True):
            e = ctx.depth_profile(**(to_device(ekw) if dev else ekw))
            got = read_both(e)
            assert e.steps() == 0 and all(len(g) == 0 for g in got[:3]) and got[3].tolist() == [0, 0, 0]
            pos, cov = e.expand(2, 5, 20)
            assert pos.tolist() == list(range(5, 25)) and not cov.any()
            e.free()


# ---------------------------------------------------------------------------------------------- expand
NS = [1, 2, 7, 8, 9, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]
FIRSTS = [0, 1, 3, T - 1, T, 5 * T + 5]
KEY_LEN = np.array([8 * T, 200, 100, 100, 100, 200], np.uint32)


@pytest.fixture(scope="module")
def busy():
    """one profile for the window tests, and the dense restatement's answer for it in both coordinate systems (computed once)
      key 0  one-base weighted segments on every window edge of NS x FIRSTS (first_pos - 1, first_pos, first_pos + n), around
             the multiples of T, and on EVERY position of [2T, 3T); nothing in (3T + 4, 5T + 4); left open at 30000 from 7T + 100
      key 1  a few steps, none at position 0       key 2  no event       key 3  seen, but its events cancel
      key 4  a step at position 0                   key 5  coverages beyond Int16"""
    at = set()
    for f in FIRSTS:
        for n in NS:
            at |= {max(f - 1, 0), f, f + n}
    for m in (1, 2, 6, 7):
        at |= {m * T - 1, m * T, m * T + 1}
    at |= set(range(2 * T, 3 * T))
    at = sorted(a for a in at if not 3 * T + 4 < a < 5 * T + 4)
    segs = [(0, a, a, (a * 37) % 101 - 40 or 1) for a in at]
    segs += [(0, 7 * T + 100, M32, 30000)]
    segs += [(1, 10, 20, 5), (1, 15, 30, -2)]
    segs += [(3, 5, 9, 0)]
    segs += [(4, 0, 9, 7), (4, 5, 14, 2)]
    segs += [(5, 10, 19, 32767), (5, 30, 39, 32768), (5, 50, 59, 65536), (5, 70, 79, -1), (5, 90, 99, -32769)]
    kw = dict(orc.pack_segments(segs), key_len=KEY_LEN, n_keys=6)
    okw = orc.oracle_kw(kw)
    dense = {zb: pbo.per_base_dense(zb, 6, **okw) for zb in (True, False)}
    st = pbo.steps(6, **okw)
    assert sorted(dense[True]) == [0, 1, 3, 4, 5] and st[3].tolist() == [1, 1, 0, 1, 1, 1]
    tile = st[1][(st[0] == 0) & (st[1] >= 2 * T) & (st[1] < 3 * T)]
    assert len(tile) == T                                   # every position of that stretch is a step
    return kw, dense


@pytest.fixture(scope="module")
def busy_profile(ctx, busy):
    p = ctx.depth_profile(**to_device(busy[0]))
    yield p
    p.free()


def want_window(dense, key, first_pos, n, skip_pos0):
    """the dense restatement over [first_pos, first_pos + n): the reference's 0-based emitter, or its 1-based one (which
    starts at index 1 and never adds slot 0) when skip_pos0"""
    q = (first_pos + np.arange(n, dtype=np.int64)).astype(np.int32)
    if key not in dense[True]:
        return q, np.zeros(n, np.int16)                     # an untouched contig is never emitted: the ABI pins zeros
    if skip_pos0:
        pos, cov = dense[False][key]
        assert first_pos >= 1
        lo = first_pos - 1
    else:
        pos, cov = dense[True][key]
        lo = first_pos
    assert np.array_equal(pos[lo:lo + n], q)
    return q, cov[lo:lo + n]


def expand_guarded(p, key, first_pos, n, off, skip_pos0=False, want_pos=True, want_cov=True, ctx=None):
    """expand into device buffers that start `off` elements into their allocations; the elements around the window must
    come back untouched"""
    import torch
    bp = torch.full((n + 32,), -7, dtype=torch.int32, device="cuda:0")
    bc = torch.full((n + 32,), -7, dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()                                # (the fills run on torch's stream, the expansion on the context's)
    p.expand(key, first_pos, n, skip_pos0=skip_pos0, want_pos=want_pos, want_cov=want_cov,
             out_pos=bp[off:off + n] if want_pos else None, out_cov=bc[off:off + n] if want_cov else None, ctx=ctx)
    (ctx or p.ctx).synchronize()
    hp, hc = bp.cpu().numpy(), bc.cpu().numpy()
    for h, used in ((hp, want_pos), (hc, want_cov)):
        assert (h[:off] == -7).all() and (h[off + n:] == -7).all()
        assert used or (h == -7).all()
    return hp[off:off + n], hc[off:off + n]


def check_window(p, dense, key, first_pos, n, off, skip_pos0=False, **kw):
    wp, wc = want_window(dense, key, first_pos, n, skip_pos0)
    gp, gc = expand_guarded(p, key, first_pos, n, off, skip_pos0=skip_pos0, **kw)
    if kw.get("want_pos", True):
        assert np.array_equal(gp, wp), (key, first_pos, n, off)
    if kw.get("want_cov", True):
        bad = np.flatnonzero(gc != wc)
        assert len(bad) == 0, (key, first_pos, n, off, skip_pos0, bad[:5], gc[bad[:5]], wc[bad[:5]])


@pytest.mark.parametrize("off", [0, 1, 3, 7])
def test_expand_windows(busy, busy_profile, off):
    for f in FIRSTS:
        for n in NS:
            check_window(busy_profile, busy[1], 0, f, n, off)


@pytest.mark.parametrize("off", [0, 1, 3, 7])
def test_expand_busy_empty_and_dense_tiles(busy, busy_profile, off):
    # [T, 7T): busy tiles, the tile where every position is a step, an empty stretch of 2T, busy tiles again
    check_window(busy_profile, busy[1], 0, T, 6 * T, off)
    check_window(busy_profile, busy[1], 0, 2 * T - 5, 4 * T, off)
    check_window(busy_profile, busy[1], 0, 2 * T, T, off)           # exactly the all-steps stretch
    check_window(busy_profile, busy[1], 0, 3 * T + 5, 2 * T - 2, off)   # no step inside: constant fills from the carry-in
    check_window(busy_profile, busy[1], 0, 0, 8 * T, off)           # the whole key, open at 30000 at its end
    assert expand_guarded(busy_profile, 0, 8 * T - 4, 4, off)[1].tolist() == [30000] * 4


def test_expand_keys(busy, busy_profile):
    dense = busy[1]
    for off in (0, 3):
        for key, L in ((1, 200), (2, 100), (3, 100), (4, 100), (5, 200)):
            for f, n in ((0, L), (0, 1), (7, 9), (L - 1, 1), (3, L - 3)):
                check_window(busy_profile, dense, key, f, n, off)
    # key 0 is left open at 30000; key 1 starts from 0 again
    assert not expand_guarded(busy_profile, 1, 0, 10, 1)[1].any()
    assert expand_guarded(busy_profile, 1, 8, 4, 0)[1].tolist() == [0, 0, 5, 5]
    # Int16 wrap-around of 32767, 32768, 65536, -1, -32769
    assert expand_guarded(busy_profile, 5, 0, 100, 0)[1][[10, 30, 50, 70, 90]].tolist() == [32767, -32768, 0, -1, 32767]


def test_expand_skip_pos0(busy, busy_profile):
    dense = busy[1]
    for off in (0, 1, 7):
        for key, L in ((4, 100), (1, 200), (0, 8 * T)):             # with a step at position 0; without; key 0 has one too
            for f, n in ((1, L), (1, 1), (2, 63), (9, 9)):
                check_window(busy_profile, dense, key, f, n, off, skip_pos0=True)
        check_window(busy_profile, dense, 0, T - 1, 2 * T + 3, off, skip_pos0=True)
    # position 0 itself under skip_pos0 is C(0) - c0 = 0 (the reference never emits it)
    assert expand_guarded(busy_profile, 4, 0, 3, 0, skip_pos0=True)[1].tolist() == [0, 0, 0]
    assert expand_guarded(busy_profile, 4, 0, 3, 0)[1].tolist() == [7, 7, 7]


def test_expand_one_column_and_host_mode(busy, busy_profile):
    dense = busy[1]
    for off in (0, 3):
        check_window(busy_profile, dense, 0, T - 1, T + 1, off, want_pos=False)
        check_window(busy_profile, dense, 0, T - 1, T + 1, off, want_cov=False)
    wp, wc = want_window(dense, 0, 5, 2 * T + 3, False)
    pos, cov = busy_profile.expand(0, 5, 2 * T + 3)                 # numpy outputs: IVX_MEM_HOST
    assert pos.dtype == np.int32 and cov.dtype == np.int16 and np.array_equal(pos, wp) and np.array_equal(cov, wc)
    pos, cov = busy_profile.expand(0, 5, 2 * T + 3, want_pos=False)
    assert pos is None and np.array_equal(cov, wc)
    assert busy_profile.expand(0, 5, 0) is not None                 # n = 0: a no-op


def test_expand_up_to_position_2_32(ctx):
    segs = [(0, M32 - 50, M32 - 10, 3), (0, M32 - 20, M32, 2), (0, 100, 200, 1)]
    kw = dict(orc.pack_segments(segs), n_keys=1)
    st = pbo.steps(1, **orc.oracle_kw(kw))
    p = ctx.depth_profile(**kw)
    for off in (0, 1):
        for f, n in ((M32 - 99, 100), (M32, 1), (M32 - 2 * T, 2 * T + 1), ((1 << 32) - T, T)):
            assert f + n == 1 << 32
            wp, wc = pbo.expand_steps(st, 0, f, n)
            gp, gc = expand_guarded(p, 0, f, n, off)
            assert np.array_equal(gp, wp) and np.array_equal(gc, wc)
            assert int(gp[-1]) == -1                                # (int32_t)(2^32 - 1)
    with pytest.raises(pyivx.IvxError) as ei:
        p.expand(0, M32 - 99, 101)
    assert ei.value.status == pyivx.ERR_INVALID and "2^32" in str(ei.value)
    # the argument check alone (no output asked for): first_pos + n = 2^32 passes, one more does not
    raw = lambda f, n: pyivx.lib().ivx_depth_profile_expand(ctx.h, p.h, pyivx.MEM_DEVICE, 0, f, n, 0, None, None)
    assert raw(0, 1 << 32) == pyivx.OK and raw(1, (1 << 32) - 1) == pyivx.OK
    assert raw(1, 1 << 32) == pyivx.ERR_INVALID and raw(0, (1 << 32) + 1) == pyivx.ERR_INVALID and raw(M32, 2) == pyivx.ERR_INVALID
    p.free()


def test_expand_large_window(ctx):
    # a 2^24-position window over ~10^5 random steps, compared in full
    rng = np.random.default_rng(41)
    L, n_seg = (1 << 24) + 5, 50_000
    s = rng.integers(0, L, n_seg)
    e = s + rng.integers(0, 3000, n_seg)
    w = rng.integers(-3, 9, n_seg)
    depth = np.zeros(L + 1, np.int64)
    np.add.at(depth, s, w)
    m = e + 1 <= L
    np.add.at(depth, (e + 1)[m], -w[m])
    cov = np.cumsum(depth)[:L].astype(np.int16)                     # (sums stay far inside int32)
    kw = dict(skey=np.zeros(n_seg, np.uint32), sstart=s.astype(np.uint32), send=e.astype(np.uint32), sweight=w.astype(np.int32),
              key_len=np.array([L], np.uint32), n_keys=1)
    p = ctx.depth_profile(**to_device(kw))
    assert 90_000 < p.steps() <= 2 * n_seg
    n = 1 << 24
    for f, off in ((3, 1), (0, 0)):
        gp, gc = expand_guarded(p, 0, f, n, off)
        assert np.array_equal(gc, cov[f:f + n])
        assert int(gp[0]) == f and int(gp[-1]) == f + n - 1 and (np.diff(gp) == 1).all()
    p.free()


def test_two_contexts_expand_one_profile(busy, busy_profile):
    other = pyivx.Ctx(0)
    try:
        for f, n, off in ((0, 8 * T, 0), (T - 1, T + 1, 3), (5 * T + 5, 65, 7)):
            a = expand_guarded(busy_profile, 0, f, n, off)
            b = expand_guarded(busy_profile, 0, f, n, off, ctx=other)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            check_window(busy_profile, busy[1], 0, f, n, off, ctx=other)
        k, q, c, seen = busy_profile.read(ctx=other)
        assert len(k) == busy_profile.steps() and seen.tolist() == [1, 1, 0, 1, 1, 1]
    finally:
        other.close()


def test_memory_limit_accounting(busy):
    c = pyivx.Ctx(0)
    try:
        kw = busy[0]
        p = c.depth_profile(**kw)                                   # (also grows the scratch to what this build needs)
        nbytes = p.device_bytes
        with_profile = c.reserved_bytes()
        assert nbytes >= 3 * 4 * p.steps() + 4 * 7 + 6
        p.free()
        base = c.reserved_bytes()
        assert with_profile - base == nbytes
        c.set_memory_limit(base + nbytes - 1)
        with pytest.raises(pyivx.IvxError) as ei:
            c.depth_profile(**kw)
        assert ei.value.status == pyivx.ERR_OOM and "Resources exhausted" in str(ei.value)
        assert c.reserved_bytes() == base
        c.set_memory_limit(base + nbytes)
        p = c.depth_profile(**kw)
        assert c.reserved_bytes() == base + nbytes
        # a device-mode expansion needs no scratch: it runs at the limit
        assert expand_guarded(p, 4, 0, 12, 1)[1].tolist() == [7] * 5 + [9] * 5 + [2] * 2
        assert c.reserved_bytes() == base + nbytes
        p.free()
        assert c.reserved_bytes() == base
    finally:
        c.close()


def test_refusals_leave_the_context_usable(ctx, busy, busy_profile):
    good = lambda: expand_guarded(busy_profile, 4, 0, 12, 1)[1].tolist() == [7] * 5 + [9] * 5 + [2] * 2

    def refused(f, status, text):
        with pytest.raises(pyivx.IvxError) as ei:
            f()
        assert ei.value.status == status and text in str(ei.value)
        assert good()

    assert good()
    refused(lambda: busy_profile.expand(6, 0, 4), pyivx.ERR_INVALID, "key id >= n_keys")
    refused(lambda: busy_profile.expand(0, M32, 2), pyivx.ERR_INVALID, "2^32")
    # the build refuses what ivx_depth refuses, with its texts
    for dev in (False, True):
        mk = (lambda kw: to_device(kw)) if dev else (lambda kw: kw)
        bad_key = dict(orc.pack_segments([(2, 0, 5, 1)]), n_keys=2)
        refused(lambda: ctx.depth_profile(**mk(bad_key)), pyivx.ERR_INVALID, "key id >= n_keys")
        reads = orc.pack_reads([(0, 0, 0, 60, [op(10, 0)]), (0, 5, 0, 60, [op(10, 0)])])
        refused(lambda: ctx.depth_profile(**mk(dict(reads, cigar_offsets=np.array([0, 6, 8], np.int32), n_keys=1))), pyivx.ERR_INVALID, "multiples of 4")
    # an index is not a profile, a profile is not an index
    ix = ctx.build(pyivx.KIND_OVERLAP, np.zeros(3, np.uint32), np.array([1, 5, 9], np.int32), np.array([4, 8, 12], np.int32), n_keys=1)
    m = C.c_uint64(0)
    L = pyivx.lib()
    assert L.ivx_depth_profile_read(ctx.h, ix.h, pyivx.MEM_HOST, None, None, None, None, 0, C.byref(m)) == pyivx.ERR_UNSUPPORTED
    assert L.ivx_depth_profile_steps(ix.h) == 0 and L.ivx_depth_profile_device_bytes(ix.h) == 0
    tot = C.c_uint64(0)
    q = np.array([2], np.int32)
    pq = q.ctypes.data_as(C.c_void_p)
    assert L.ivx_probe_overlap_count(ctx.h, busy_profile.h, pyivx.MEM_HOST, None, pq, pq, C.c_uint64(1), None, C.byref(tot)) == pyivx.ERR_UNSUPPORTED
    ix.free()
    assert good()
    # depth() itself is untouched by all of this
    k, s, e, cv = ctx.depth(**{k_: v for k_, v in busy[0].items()})
    want = orc.depth_loop(**orc.oracle_kw(busy[0]))
    assert np.array_equal(k, want[0]) and np.array_equal(s, want[1]) and np.array_equal(e, want[2]) and np.array_equal(cv, want[3])
