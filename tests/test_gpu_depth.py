"""-m gpu: ivx_depth (csrc/ivx_depth.hip) bit-exact against the CPU restatement (tests/depth_oracle.py), every case once
with numpy arrays (IVX_MEM_HOST) and once with torch device tensors (IVX_MEM_DEVICE).

Shapes sit where the kernels change path.  With T ops in all: a scan tile is 1024 ops (4 per thread, 64 lanes per
wavefront), one workgroup scans up to 4096 tile sums serially, beyond 4096 tiles the tile sums get a level of their own."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_oracle as orc  # noqa: E402
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

NULL = pyivx.NULL_IDX
M32 = 0xFFFFFFFF
I32_MAX = 0x7FFFFFFF
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


def from_device(out):
    return tuple(None if o is None else o.cpu().numpy().view(dt) for o, dt in zip(out, (np.uint32, np.uint32, np.uint32, np.int32)))


def both(ctx, kw):
    """the blocks through both memory modes (asserted identical)"""
    host = ctx.depth(**kw)
    dev = from_device(ctx.depth(**to_device(kw)))
    for a, b in zip(host, dev):
        assert (a is None and b is None) or (a.dtype == b.dtype and np.array_equal(a, b))
    return host


def check(ctx, kw, big=False):
    want = (orc.depth_numpy if big else orc.depth_loop)(**orc.oracle_kw(kw))
    got = both(ctx, kw)
    assert len(got[0]) == len(want[0])
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    return got


def reads_kw(reads, segs=(), **extra):
    kw = orc.pack_reads(reads)
    if segs:
        kw.update(orc.pack_segments(segs))
    kw.update(extra)
    return kw


def rows(out):
    return [tuple(int(x) for x in r) for r in zip(*out)]


# ---------------------------------------------------------------------------------------------- scan edges
def random_ops(rng, n):
    """ops of every code with short lengths (M-heavy, some of length 0)"""
    code = np.where(rng.random(n) < 0.5, 0, rng.integers(0, 16, n))
    return ((rng.integers(0, 6, n) << 4) | code).astype(np.uint32)


def layout(T, how, rng):
    ops = random_ops(rng, T)
    if how == "one_op_reads":
        cuts = list(range(T + 1))
    elif how == "one_read":
        cuts = [0, T]
    else:                       # reads that end exactly at, one before and one after ops 64, 1024 and 4096
        cuts = sorted({0, T} | {c for e in (64, 1024, 4096) for c in (e - 1, e, e + 1) if 0 < c < T})
    n = len(cuts) - 1
    kw = dict(rkey=rng.integers(0, 2, n).astype(np.uint32), rpos=rng.integers(0, 200, n).astype(np.uint32),
              rflags=np.where(rng.random(n) < 0.1, 4, 0).astype(np.uint32), rmapq=rng.integers(0, 61, n).astype(np.uint32),
              cigar_offsets=(4 * np.array(cuts)).astype(np.int32), cigar_ops=ops, min_mapq=5)
    return kw


@pytest.mark.parametrize("how", ["one_op_reads", "one_read", "reads_at_edges"])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 5 * 1024 + 3])
def test_scan_edges(ctx, T, how):
    check(ctx, layout(T, how, np.random.default_rng(T * 3 + len(how))))


@pytest.fixture(scope="module")
def big_case():
    """4 * 1024 * 1024 + 1025 ops (the tile sums need a scan level of their own) in reads of 1-7 ops; the restatement's
    answer is computed once"""
    rng = np.random.default_rng(77)
    T = 4 * 1024 * 1024 + 1025
    nops = rng.integers(1, 8, T // 3)
    cs = np.cumsum(nops)
    n = int(np.searchsorted(cs, T))
    cuts = np.r_[0, cs[:n], T] if n == 0 or cs[n - 1] < T else np.r_[0, cs[:n]]
    n = len(cuts) - 1
    code = np.where(rng.random(T) < 0.6, 0, rng.integers(0, 16, T))
    kw = dict(rkey=np.sort(rng.integers(0, 3, n)).astype(np.uint32), rpos=rng.integers(0, 3_000_000, n).astype(np.uint32),
              rflags=np.where(rng.random(n) < 0.05, 1024, 0).astype(np.uint32), rmapq=rng.integers(0, 61, n).astype(np.uint32),
              cigar_offsets=(4 * cuts).astype(np.int32), cigar_ops=((rng.integers(0, 60, T) << 4) | code).astype(np.uint32),
              min_mapq=3, n_keys=3)
    assert int(np.diff(cuts).min()) >= 1 and int(np.diff(cuts).max()) <= 7 and cuts[-1] == T
    return kw, orc.depth_numpy(**orc.oracle_kw(kw))


def test_third_scan_level(ctx, big_case):
    kw, want = big_case
    got = both(ctx, kw)
    assert len(want[0]) > 100_000
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_empty_cigar_reads(ctx):
    # reads without ops: first, last, and in runs between ops 63|64 and 1023|1024 (a wavefront's and a tile's edge)
    rng = np.random.default_rng(5)
    reads = [(0, 7, 0, 60, [])] * 3
    for i in range(1030):
        reads.append((0, int(rng.integers(0, 300)), 0, 60, [op(int(rng.integers(1, 9)), 0)]))
        if i in (63, 1023):
            reads += [(0, 11, 0, 60, [])] * 70
        if i == 500:
            reads.append((0, 5, 0, 60, []))
    reads += [(0, 9, 0, 60, [])] * 2
    check(ctx, reads_kw(reads))
    assert len(both(ctx, reads_kw([(0, 1, 0, 60, [])] * 5))[0]) == 0


# ---------------------------------------------------------------------------------------------- the read filter
def test_skip_mark_on_rkey(ctx):
    reads = [(NULL, 0, 0, 60, [op(10, 0)]), (1, 5, 0, 60, [op(10, 0)]), (NULL, 7, 0, 60, [op(3, 0), op(2, 2)]), (0, 2, 0, 60, [op(4, 0)])]
    got = check(ctx, reads_kw(reads, n_keys=2))
    assert rows(got) == [(0, 2, 5, 1), (1, 5, 14, 1)]


def test_filter_flag_bits(ctx):
    flags = [4, 256, 512, 1024, 2, 0, 4 | 2, 1796, 99, 163]
    reads = [(0, 100 * i, f, 60, [op(10, 0)]) for i, f in enumerate(flags)]
    got = check(ctx, reads_kw(reads))
    assert [r[1] for r in rows(got)] == [100 * i for i, f in enumerate(flags) if not f & 1796]
    check(ctx, reads_kw(reads, filter_flag=0))
    check(ctx, reads_kw(reads, filter_flag=2))


def test_min_mapq(ctx):
    reads = [(0, 0, 0, 29, [op(10, 0)]), (0, 100, 0, 30, [op(10, 0)]), (0, 200, 0, 60, [op(10, 0)])]
    assert rows(check(ctx, reads_kw(reads, min_mapq=30))) == [(0, 100, 109, 1), (0, 200, 209, 1)]


def test_null_flags_and_mapq(ctx):
    reads = [(0, 0, 4, 0, [op(10, 0)]), (0, 100, 0, 60, [op(10, 0)])]
    kw = reads_kw(reads, min_mapq=30)
    assert len(check(ctx, kw)[0]) == 1
    assert len(check(ctx, dict(kw, rflags=None))[0]) == 1           # the mapq of read 0 still fails
    assert len(check(ctx, dict(kw, rmapq=None))[0]) == 1            # ... and its flag
    assert len(check(ctx, dict(kw, rflags=None, rmapq=None))[0]) == 2


def test_all_op_codes(ctx):
    reads = [(0, 10, 0, 60, [op(3, c) for c in range(16)]), (0, 0, 0, 60, [op(2, c) for c in reversed(range(16))])]
    got = check(ctx, reads_kw(reads))
    # codes 0, 7, 8 cover; 2, 3 only advance: read 0 covers [10,13) [19,22) [22,25)
    assert (0, 19, 24, 1) in rows(got)


# ---------------------------------------------------------------------------------------------- sums
def test_cancellation(ctx):
    assert len(check(ctx, reads_kw([(0, 5, 0, 60, [op(0, 0)])]))[0]) == 0
    assert rows(check(ctx, reads_kw([(0, 0, 0, 60, [op(10, 0)]), (0, 10, 0, 60, [op(10, 0)])]))) == [(0, 0, 19, 1)]
    assert rows(check(ctx, reads_kw([(0, 3, 0, 60, [op(10, 0)])] * 5))) == [(0, 3, 12, 5)]
    assert rows(check(ctx, reads_kw([(0, 0, 0, 60, [op(10, 0)]), (0, 4, 0, 60, [op(0, 0)])]))) == [(0, 0, 9, 1)]


def test_saturation(ctx):
    assert rows(check(ctx, reads_kw([(0, M32 - 9, 0, 60, [op(20, 0)])]))) == [(0, M32 - 9, M32 - 1, 1)]
    # D ops that sum past 2^32 before an M: both of its events land on 2^32 - 1 and cancel
    long_d = [op((1 << 28) - 1, 2)] * 17
    got = check(ctx, reads_kw([(0, 100, 0, 60, [op(5, 0)] + long_d + [op(5, 0)]), (0, 50, 0, 60, [op(5, 0)])]))
    assert rows(got) == [(0, 50, 54, 1), (0, 100, 104, 1)]
    # ... and one that stops just short of it
    got = check(ctx, reads_kw([(0, 100, 0, 60, [op((1 << 28) - 1, 3)] * 15 + [op(1 << 27, 0), op((1 << 28) - 1, 0)])]))
    assert len(got[0]) == 1 and int(got[2][0]) == M32 - 1


# ---------------------------------------------------------------------------------------------- keys
def test_keys(ctx):
    reads = [(0, 0, 0, 60, [op(10, 0)]), (0, 5, 0, 60, [op(10, 0)])]
    kw = reads_kw(reads)
    assert rows(check(ctx, dict(kw, rkey=None))) == [(0, 0, 4, 1), (0, 5, 9, 2), (0, 10, 14, 1)]
    reads = [(2, 0, 0, 60, [op(10, 0)]), (0, 5, 0, 60, [op(10, 0)])]
    assert rows(check(ctx, reads_kw(reads, n_keys=3))) == [(0, 5, 14, 1), (2, 0, 9, 1)]


def test_many_keys(ctx):
    rng = np.random.default_rng(9)
    nk, n = 70_000, 150_000
    kw = dict(rkey=rng.integers(0, nk, n).astype(np.uint32), rpos=rng.integers(0, 50, n).astype(np.uint32),
              rflags=np.zeros(n, np.uint32), rmapq=np.full(n, 60, np.uint32),
              cigar_offsets=(4 * np.arange(n + 1)).astype(np.int32), cigar_ops=((rng.integers(1, 30, n) << 4) | 0).astype(np.uint32), n_keys=nk)
    check(ctx, kw, big=True)


def test_open_key_does_not_leak(ctx):
    # key 0 is left open by clipping (its -1 is dropped); key 1 starts from 0 again
    reads = [(0, 5, 0, 60, [op(10, 0)]), (1, 2, 0, 60, [op(4, 0)]), (1, 3, 0, 60, [op(4, 0)])]
    got = check(ctx, reads_kw(reads, key_len=np.array([7, 100], np.uint32)))
    assert rows(got) == [(1, 2, 2, 1), (1, 3, 5, 2), (1, 6, 6, 1)]


def test_clipping_edges(ctx):
    L = 50
    kl = np.array([L], np.uint32)
    one = lambda pos, n: rows(check(ctx, reads_kw([(0, pos, 0, 60, [op(n, 0)]), (0, 0, 0, 60, [op(3, 0)])], key_len=kl)))
    assert one(40, 10) == [(0, 0, 2, 1), (0, 40, 49, 1)]            # end at exactly len: kept
    assert one(40, 11) == [(0, 0, 2, 1)]                            # end at len + 1: dropped, the block stays open
    assert one(L, 5) == [(0, 0, 2, 1)]                              # start at len: kept, end dropped
    assert one(L + 1, 5) == [(0, 0, 2, 1)]                          # start at len + 1 and beyond: nothing
    assert one(L + 1000, 5) == [(0, 0, 2, 1)]
    # a later op of a read that ran past the end adds nothing either (cigar.rs:217-220)
    assert rows(check(ctx, reads_kw([(0, 45, 0, 60, [op(3, 0), op(10, 2), op(4, 0)])], key_len=kl))) == [(0, 45, 47, 1)]
    segs = [(0, 45, 49, 2), (0, 48, 50, 1), (0, 60, 70, 5)]
    assert rows(check(ctx, reads_kw([], segs, key_len=kl))) == [(0, 45, 47, 2), (0, 48, 49, 3)]


# ---------------------------------------------------------------------------------------------- weighted segments
def test_segments(ctx):
    segs = [(0, 10, 19, 3), (0, 15, 24, -1), (0, 12, 13, 0), (1, 0, 4, -2)]
    kw = reads_kw([], segs)
    assert rows(check(ctx, kw)) == [(0, 10, 14, 3), (0, 15, 19, 2), (0, 20, 24, -1), (1, 0, 4, -2)]
    assert rows(check(ctx, dict(kw, sweight=None))) == [(0, 10, 11, 1), (0, 12, 13, 2), (0, 14, 14, 1), (0, 15, 19, 2), (0, 20, 24, 1), (1, 0, 4, 1)]
    assert rows(check(ctx, reads_kw([], [(0, 0, 9, I32_MAX), (0, 0, 9, I32_MAX)]))) == [(0, 0, 9, -2)]
    assert rows(check(ctx, reads_kw([], [(0, 0, 9, -0x80000000)]))) == [(0, 0, 9, -0x80000000)]
    # end < start is not checked: (20, +1) and (11, -1)
    assert rows(check(ctx, reads_kw([], [(0, 20, 10, 1)]))) == [(0, 11, 19, -1)]
    # end = 2^32 - 1: the closing event saturates onto 2^32 - 1
    assert rows(check(ctx, reads_kw([], [(0, 5, M32, 1)]))) == [(0, 5, M32 - 1, 1)]
    assert rows(check(ctx, reads_kw([], [(NULL, 5, 9, 1), (0, 1, 2, 1)], n_keys=1))) == [(0, 1, 2, 1)]
    # reads and segments in one call
    assert rows(check(ctx, reads_kw([(0, 0, 0, 60, [op(10, 0)])], [(0, 5, 14, 2)]))) == [(0, 0, 4, 1), (0, 5, 9, 3), (0, 10, 14, 2)]


def random_reads(rng, n, n_keys=3):
    return [(int(rng.integers(0, n_keys)), int(rng.integers(0, 2000)), 0, 60,
             [op(int(rng.integers(0, 40)), int(rng.choice([0, 0, 0, 1, 2, 3, 4, 7, 8]))) for _ in range(int(rng.integers(1, 6)))]) for _ in range(n)]


def test_accumulation(ctx):
    rng = np.random.default_rng(21)
    a, b = random_reads(rng, 700), random_reads(rng, 900)
    whole = check(ctx, reads_kw(a + b, n_keys=3))
    ka, sa, ea, ca = check(ctx, reads_kw(a, n_keys=3))
    acc = both(ctx, dict(orc.pack_reads(b), skey=ka, sstart=sa, send=ea, sweight=ca, n_keys=3))
    for g, w in zip(acc, whole):
        assert np.array_equal(g, w)


def test_read_order_is_irrelevant(ctx):
    rng = np.random.default_rng(22)
    reads = random_reads(rng, 1500)
    srt = sorted(reads, key=lambda r: (r[0], r[1]))
    a, b = check(ctx, reads_kw(reads)), check(ctx, reads_kw(srt))
    for g, w in zip(a, b):
        assert np.array_equal(g, w)


def test_offsets_need_not_start_at_zero(ctx):
    kw = reads_kw([(0, 0, 0, 60, [op(4, 1)]), (0, 5, 0, 60, [op(10, 0)]), (0, 7, 0, 60, [op(2, 0), op(3, 0)])])
    sl = dict(kw, **{k: kw[k][1:] for k in ("rkey", "rpos", "rflags", "rmapq", "cigar_offsets")})
    assert rows(check(ctx, sl)) == [(0, 5, 6, 1), (0, 7, 11, 2), (0, 12, 14, 1)]


# ---------------------------------------------------------------------------------------------- the calling protocol
def raw(ctx, kw, outs, cap):
    """one ivx_depth call on host columns -> (status, n_out)"""
    g = lambda k, dt: None if kw.get(k) is None else np.ascontiguousarray(kw[k], dt)
    cols = [g("rkey", np.uint32), g("rpos", np.uint32), g("rflags", np.uint32), g("rmapq", np.uint32), g("cigar_offsets", np.int32), g("cigar_ops", np.uint32)]
    seg = [g("skey", np.uint32), g("sstart", np.uint32), g("send", np.uint32), g("sweight", np.int32)]
    n_reads = 0 if cols[1] is None else len(cols[1])
    n_seg = 0 if seg[1] is None else len(seg[1])
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    m = C.c_uint64(0)
    st = pyivx.lib().ivx_depth(ctx.h, pyivx.MEM_HOST, *[p(c) for c in cols], n_reads, *[p(s) for s in seg], n_seg, kw.get("n_keys", 1),
                               p(g("key_len", np.uint32)), kw.get("filter_flag", 1796), kw.get("min_mapq", 0), *[p(o) for o in outs], cap, C.byref(m))
    return st, m.value


def test_capacity_protocol(ctx):
    rng = np.random.default_rng(23)
    kw = reads_kw(random_reads(rng, 300, n_keys=2), [(1, 10, 500, 2)], n_keys=2)
    want = orc.depth_loop(**orc.oracle_kw(kw))
    need = len(want[0])
    assert need > 50
    ctx.reset_metrics()
    st, m = raw(ctx, kw, [None] * 4, 0)
    assert (st, m) == (pyivx.OK, need)
    bufs = lambda n: [np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.int32)]
    out = bufs(need)
    assert raw(ctx, kw, out, need) == (pyivx.OK, need)
    for g, w in zip(out, want):
        assert np.array_equal(g, w)
    mt = ctx.metrics()
    assert (mt["input_batches"], mt["input_rows"], mt["output_batches"], mt["output_rows"]) == (2, 2 * 301, 1, need)
    st, m = raw(ctx, kw, bufs(need - 1), need - 1)
    assert (st, m) == (pyivx.ERR_CAPACITY, need)
    assert "too small" in pyivx.lib().ivx_last_error(ctx.h).decode()
    # a larger buffer than needed; any output NULL on its own
    big = bufs(need + 7)
    assert raw(ctx, kw, big, need + 7) == (pyivx.OK, need)
    assert np.array_equal(big[3][:need], want[3])
    for skip in range(4):
        outs = tuple(i != skip for i in range(4))
        got = both(ctx, dict(kw, outputs=outs))
        for i in range(4):
            assert (got[i] is None) if i == skip else np.array_equal(got[i], want[i])


def test_empty_input(ctx):
    m = C.c_uint64(9)
    assert pyivx.lib().ivx_depth(ctx.h, pyivx.MEM_HOST, *[None] * 6, 0, *[None] * 4, 0, 0, None, 1796, 0, *[None] * 4, 0, C.byref(m)) == pyivx.OK
    assert m.value == 0
    e32 = np.zeros(0, np.uint32)
    kw = dict(rkey=e32, rpos=e32, rflags=e32, rmapq=e32, cigar_offsets=np.zeros(1, np.int32), cigar_ops=e32)
    assert len(ctx.depth(**kw)[0]) == 0
    # reads that all are filtered out; segments that emit nothing
    assert len(both(ctx, reads_kw([(0, 0, 4, 60, [op(5, 0)])]))[0]) == 0
    assert len(both(ctx, reads_kw([], [(0, 3, 9, 0)]))[0]) == 0


def test_refusals_leave_the_context_usable(ctx):
    good = reads_kw([(0, 0, 0, 60, [op(10, 0)]), (1, 5, 0, 60, [op(10, 0)])], n_keys=2)

    def refused(kw, text):
        for f in (lambda: ctx.depth(**kw), lambda: ctx.depth(**to_device(kw))):
            with pytest.raises(pyivx.IvxError) as ei:
                f()
            assert ei.value.status == pyivx.ERR_INVALID and text in str(ei.value)
            assert rows(both(ctx, good)) == [(0, 0, 9, 1), (1, 5, 14, 1)]

    refused(dict(good, rkey=np.array([0, 2], np.uint32)), "key id >= n_keys")
    refused(dict(reads_kw([], [(2, 0, 5, 1)]), n_keys=2), "key id >= n_keys")
    refused(dict(good, cigar_offsets=np.array([0, 6, 8], np.int32)), "multiples of 4")
    refused(dict(good, cigar_offsets=np.array([4, 0, 8], np.int32)), "multiples of 4")
