"""-m gpu: build-side match marks through the C ABI -- ivx_probe_mark_build (direct and region path), ivx_bits_mark and
ivx_bits_select.

Expected marks come from the CPU oracle's pairs: matched build rows = np.unique(orc.join(build, probe)[0]), unmatched =
the complement.  Every comparison is on the bitmap's whole words, so a bit at or past the build side's row count fails it.
The region-path cases reach each index form with the shapes tests/test_gpu_region_forms.py uses (its builders and its
restatement of the routing are imported from there) and assert the form through ivx_index_layout."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pair_set
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402
import test_gpu_region_forms as rf  # noqa: E402

pytestmark = pytest.mark.gpu

env, cols = rf.env, rf.cols


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


def words_of(rows_set, n_bits):
    """the bitmap words with exactly these bits set"""
    bits = np.zeros(((n_bits + 31) // 32) * 32, np.uint8)
    bits[np.asarray(rows_set, np.int64)] = 1
    return np.packbits(bits, bitorder="little").view(np.uint32) if len(bits) else np.zeros(0, np.uint32)


def positions(words, n_bits):
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n_bits])


def want_words(b, p, want=None):
    wb = orc.join(*b, *p, threads=4)[0] if want is None else want[0]
    return words_of(np.unique(wb), len(b[1]))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint32)


def mark(ctx, ix, p, mem, marks=None):
    """one ivx_probe_mark_build call in either memory mode; -> the bitmap's words on the host"""
    n_bits = ix.rows
    if mem == "host":
        m = pyivx.Ctx.new_marks(n_bits) if marks is None else marks.copy()
        ctx.mark_build(ix, *p, m)
        return m[: (n_bits + 31) // 32]
    m = dev(pyivx.Ctx.new_marks(n_bits) if marks is None else marks)
    ctx.mark_build(ix, *[dev(c) for c in p], m)
    ctx.synchronize()
    return host(m)[: (n_bits + 31) // 32]


# ---------------------------------------------------------------- ivx_bits_select

N_BITS = [0, 1, 31, 32, 33, 63, 64, 65, 2**16 + 1, 2**20 + 37]
PATTERNS = ["clear", "set", "random", "bit0", "last"]


def pattern_bits(pattern, n_bits):
    b = np.zeros(n_bits, np.uint8)
    if pattern == "set":
        b[:] = 1
    elif pattern == "random":
        b[:] = np.random.default_rng(n_bits).integers(0, 2, n_bits)
    elif pattern == "bit0" and n_bits:
        b[0] = 1
    elif pattern == "last" and n_bits:
        b[-1] = 1
    return b


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n_bits", N_BITS)
def test_bits_select(ctx, n_bits, pattern):
    b = pattern_bits(pattern, n_bits)
    nw = (n_bits + 31) // 32
    for want_set in (1, 0):
        # the bits at and past n_bits in the last word: ones must not be reported as set, zeros not as clear
        padded = np.full(max(nw, 1) * 32, 1 if want_set else 0, np.uint8)
        padded[:n_bits] = b
        words = np.packbits(padded, bitorder="little").view(np.uint32)
        expect = np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")[:n_bits] == want_set)
        for mem in ("host", "device"):
            w = words if mem == "host" else dev(words)
            assert ctx.bits_select(w, n_bits, want_set, count_only=True) == len(expect), (mem, want_set)
            got = ctx.bits_select(w, n_bits, want_set)
            got = got if mem == "host" else host(got)
            assert len(got) == len(expect) and (got == expect).all(), (mem, want_set)
            got = ctx.bits_select(w, n_bits, want_set, cap=len(expect) + 3)        # a roomy buffer
            got = got if mem == "host" else host(got)
            assert len(got) == len(expect) and (got == expect).all(), (mem, want_set)
            if len(expect):
                with pytest.raises(pyivx.IvxError) as ei:
                    ctx.bits_select(w, n_bits, want_set, cap=len(expect) - 1)
                assert ei.value.status == pyivx.ERR_CAPACITY and ei.value.needed == len(expect), (mem, want_set)


# ---------------------------------------------------------------- ivx_bits_mark

@pytest.mark.parametrize("mem", ["host", "device"])
def test_bits_mark(ctx, mem):
    n_bits = 1000
    rng = np.random.default_rng(11)
    pre = rng.choice(n_bits, 40, replace=False)
    base = words_of(pre, n_bits)

    def run(idx, start=base):
        idx = np.ascontiguousarray(idx, np.uint32)
        if mem == "host":
            bits = start.copy()
            ctx.bits_mark(idx, bits, n_bits)
            return bits
        bits = dev(start)
        ctx.bits_mark(dev(idx), bits, n_bits)
        ctx.synchronize()
        return host(bits)

    assert (run([]) == base).all()                                                  # n = 0
    assert (run(np.full(5000, 77)) == words_of(np.append(pre, 77), n_bits)).all()   # all indices equal
    word = np.arange(64, 96)
    assert (run(rng.permutation(word)) == words_of(np.concatenate([pre, word]), n_bits)).all()   # every bit of one word
    idx = rng.integers(0, n_bits, 3000).astype(np.uint32)
    null = rng.random(3000) < 0.3
    mixed = np.where(null, pyivx.NULL_IDX, idx).astype(np.uint32)
    assert (run(mixed) == words_of(np.concatenate([pre, idx[~null]]), n_bits)).all()             # IVX_NULL_IDX skipped, earlier bits survive
    assert (run([n_bits - 1], np.zeros_like(base)) == words_of([n_bits - 1], n_bits)).all()      # the last bit is in range
    bad = idx.copy()
    bad[1234] = n_bits                                                                           # one past it is not
    with pytest.raises(pyivx.IvxError) as ei:
        run(bad)
    assert ei.value.status == pyivx.ERR_INVALID


# ---------------------------------------------------------------- ivx_probe_mark_build, direct path

def direct_build(nb, nk, seed):
    """nb build rows over keys 0..nk-1 of an index with nk + 1 keys: the last key has no build rows.  Every tenth row
    (3, 13, ...) lies far beyond anything strict_probes generates: nobody overlaps those"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, nk, nb)
    s = rng.integers(0, 200_000, nb) + np.where(np.arange(nb) % 10 == 3, 5_000_000, 0)
    return cols(k, s, s + rng.integers(0, 400, nb))


def strict_probes(n, nk, seed):
    """probe rows as the SQL path hands them over for strict predicates (end - 1): some have qe < qs; keys 0..nk-1, the
    key without build rows (nk) and one the index does not have at all (nk + 5)"""
    rng = np.random.default_rng(seed)
    k = rng.choice(np.concatenate([np.arange(nk + 1), [nk + 5]]), n)
    s = rng.integers(-500, 201_000, n)
    return cols(k, s, s + rng.integers(-2, 120, n))


@pytest.mark.parametrize("nk", [1, 3])
@pytest.mark.parametrize("nb", [1, 33, 5000])
def test_mark_build_direct(ctx, nb, nk):
    b = direct_build(nb, nk, nb + nk)
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=nk + 1)
    assert ix.rows == nb
    nw = (nb + 31) // 32
    pre = words_of(np.arange(0, nb, 7), nb)
    union = np.zeros(nw, np.uint32)
    with env(IVX_JOIN_PATH="direct"):
        for n in (0, 1, 63, 64, 65, 8192, 100_003):
            p = strict_probes(n, nk, n + 1)
            if nb == 1 and n:
                p[0][0], p[1][0], p[2][0] = b[0][0], b[1][0], b[1][0]                     # (the single build row is hit by every non-empty batch)
            want = want_words(b, p)
            union |= want
            for mem in ("host", "device"):
                got = mark(ctx, ix, p, mem)
                assert len(got) == nw and (got == want).all(), (n, mem)        # every word: unmatched rows and the tail stay clear
                got = mark(ctx, ix, p, mem, marks=pre)
                assert (got == (want | pre)).all(), (n, mem)                    # bits set beforehand survive
        # two batches into one bitmap = the union
        p1, p2 = strict_probes(65, nk, 66), strict_probes(8192, nk, 8193)
        for mem in ("host", "device"):
            m1 = mark(ctx, ix, p1, mem)
            m12 = mark(ctx, ix, p2, mem, marks=m1)
            assert (m12 == (want_words(b, p1) | want_words(b, p2))).all(), mem
    hit = positions(union, nb)
    assert len(hit) > 0 and not (hit % 10 == 3).any()                   # build rows nobody overlaps stay clear
    if nb == 5000:
        assert len(hit) > nb // 2
    ix.free()


def test_mark_build_metrics_and_arguments(ctx):
    b = direct_build(5000, 3, 1)
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=4)
    p = strict_probes(1000, 3, 2)
    ctx.reset_metrics()
    mark(ctx, ix, p, "host")
    m = ctx.metrics()
    assert (m["input_batches"], m["input_rows"], m["output_batches"], m["output_rows"]) == (1, 1000, 0, 0), m
    cnt = ctx.build(pyivx.KIND_COUNT, *b, n_keys=4)
    with pytest.raises(pyivx.IvxError) as ei:
        ctx.mark_build(cnt, *p, pyivx.Ctx.new_marks(5000))
    assert ei.value.status == pyivx.ERR_UNSUPPORTED
    cnt.free(); ix.free()


# ---------------------------------------------------------------- ivx_probe_mark_build, region path

def both_paths(ctx, ix, b, p, mems=("host",), want=None):
    """direct and region results equal each other and the oracle's matched build rows"""
    want = want_words(b, p, want)
    for mem in mems:
        with env(IVX_JOIN_PATH="direct"):
            d = mark(ctx, ix, p, mem)
        with env(IVX_JOIN_PATH="regions"):
            r = mark(ctx, ix, p, mem)
            pre = words_of(np.arange(3, ix.rows, 11), ix.rows)
            r2 = mark(ctx, ix, p, mem, marks=pre)
        assert (d == want).all(), mem
        assert (r == want).all(), mem
        assert (r == d).all() and (r2 == (want | pre)).all(), mem
    return want


def region_path_scratch(ix, p):
    """device scratch a fresh context takes for one device-mode mark call under IVX_JOIN_PATH=regions: the direct kernel
    needs none, the region path routes the rows into scratch pages"""
    c = pyivx.Ctx(0)
    try:
        m = dev(pyivx.Ctx.new_marks(ix.rows))
        with env(IVX_JOIN_PATH="regions"):
            c.mark_build(ix, *[dev(x) for x in p], m)
        c.synchronize()
        return c.reserved_bytes()
    finally:
        c.close()


def test_mark_regions_many_regions_sorted_rows(ctx):
    """(a) three keys, several lean regions each, 1.2 million probe rows in (key, start) order: more 8192-row chunks than
    workgroups, so a workgroup's share crosses regions (flush, clear, next slice), and the two crowded regions are shared
    by many workgroups (OR, not store, into the same words)"""
    nk, per = 3, 60_000
    k = np.repeat(np.arange(nk), per)
    s = np.tile(np.arange(per, dtype=np.int64) * 512, nk)
    b = cols(k, s, s + 255)
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=nk)
    lay, geo = rf.layout_of(ix, *b, nk)
    assert lay["pk24"] == 1 and lay["slow"] == 0 and nk * 2 < lay["nreg"] <= rf.IVX_MAXREG, lay
    rng = np.random.default_rng(21)
    n_u = 400_000
    per_crowded = max(49, (270 - lay["nreg"] + 1) // 2) * rf.FP_CHUNK - 100     # rows of each crowded region: > 256 chunks in all
    n_c = 2 * per_crowded
    ku = rng.integers(0, nk, n_u); su = rng.integers(-1000, per * 512 + 1000, n_u)
    r1, r2 = geo["regs"][1], geo["regs"][len(geo["regs"]) // 2]
    kc = np.concatenate([np.full(n_c // 2, r1["k"]), np.full(n_c // 2, r2["k"])])
    sc = np.concatenate([rng.integers(r1["rbase"], r1["rend"], n_c // 2), rng.integers(r2["rbase"], r2["rend"], n_c // 2)])
    pk, ps = np.concatenate([ku, kc]), np.concatenate([su, sc])
    pe = ps + np.where(rng.random(len(ps)) < 0.5, 0, rng.integers(0, 200, len(ps)))
    order = np.lexsort((ps, pk))
    p = cols(pk[order], ps[order], pe[order])
    reg = rf.route_region(lay, b, p)
    per_reg = np.bincount(reg[reg >= 0], minlength=lay["nreg"])
    chunks = int(((per_reg + rf.FP_CHUNK - 1) // rf.FP_CHUNK).sum())
    assert chunks > 256 and (per_reg > 4 * rf.FP_CHUNK).sum() >= 2, (chunks, per_reg.max())
    want = both_paths(ctx, ix, b, p, mems=("host", "device"))
    matched = len(positions(want, len(b[1])))
    assert 0 < matched < len(b[1])
    ix.free()


@pytest.mark.parametrize("side", ["slice_6144", "slice_6145"])
def test_mark_regions_slice_capacity(ctx, side):
    """(b) region 0's slice holds exactly IVX_RP_ECAP entries: the cells that hold slice entries 0, 31, 32, 6112 and 6143
    are matched (first and last bit of the LDS bitmap's first, second and last words); one more build row and the index
    is no longer lean: the same call falls back to the direct kernel and is still right"""
    b = rf.slice_build(0 if side == "slice_6144" else 1)
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    lay, geo = rf.layout_of(ix, *b, 1)
    assert lay["sh0"] == 4 and lay["rcells"] == 1024 and lay["pk24"] == 1 and lay["levrows"] == 1, lay
    assert lay["slow"] == (0 if side == "slice_6144" else 1), lay
    assert geo["regs"][0]["ne"] == rf.IVX_RP_ECAP + (side != "slice_6144")
    s = b[1].astype(np.int64)
    in_slice = np.sort(s[s < (1024 + rf.IVX_RP_HALO) * 16])              # region 0's slice window, entries in cell order
    cells = np.unique(in_slice[[0, 31, 32, 6112, 6143]] >> 4)
    starts = in_slice[np.isin(in_slice >> 4, cells)]                     # a point probe on every row of those cells
    p = cols(np.zeros(len(starts)), starts, starts)
    want = orc.join(*b, *p, threads=4)
    hit = np.unique(want[0])
    assert 5 <= len(hit) < len(in_slice) // 4
    both_paths(ctx, ix, b, p, want=want)
    # every entry of the slice matched, and a random batch over the whole index
    allp = cols(np.zeros(len(in_slice)), in_slice, in_slice)
    both_paths(ctx, ix, b, allp)
    rng = np.random.default_rng(22)
    both_paths(ctx, ix, b, rf.edge_probes(geo, 4, rng, 60_000, -100, 3_300_000, maxlen=40))
    scratch = region_path_scratch(ix, p)
    assert (scratch > 0) == (side == "slice_6144"), scratch             # lean: routed; not lean: the direct kernel, no scratch
    ix.free()


def test_mark_regions_slow_index_falls_back(ctx):
    """(c) one build row above level 0: slow = 1, no lean form, the direct kernel answers under IVX_JOIN_PATH=regions"""
    b = rf.level0_lean_build(True)
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    lay = ix.layout()
    assert lay["slow"] == 1 and lay["levrows"] & ~1 and lay["nreg"] > 0, lay
    rng = np.random.default_rng(23)
    p = rf.points(rng, 150_000, 0, int(b[1].max()), unknown=1 / 3)
    p = rf.cat(p, cols([0, 0], [1_000_100, 1_000_256], [1_000_100, 1_000_256]))     # on the level-1 row (its last coordinate alone)
    both_paths(ctx, ix, b, p)
    assert region_path_scratch(ix, p) == 0
    ix.free()


def test_mark_regions_rest_rows(ctx):
    """(d) rows the packed form cannot carry: a span past the region's halo, qe < qs, a length at and past the packed
    maximum, rows that start before the key's first or behind its last build row -- k_lean_rest<MarkOp> marks for them"""
    b = rf.sparse_build()
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    lay, geo = rf.layout_of(ix, *b, 1)
    assert (lay["sh0"], lay["rcells"], lay["slow"], lay["pk24"], lay["fg"]) == (8, 2048, 0, 1, rf.NOFG), lay
    rng = np.random.default_rng(24)
    past, last = rf.halo_probes(geo, lay["sh0"], True), rf.halo_probes(geo, lay["sh0"], False)
    n_rand = 20_000
    f = rf.probe_form(lay, n_rand + 10_000, 1, {"IVX_JOIN_PATH": "regions"}, mode="exists")
    maxlen = f["maxlen"]
    assert f["packed"] and maxlen == 65535, f
    x = rng.integers(0, int(b[1].max()) - 200_000, 3000)
    longs = rf.cat(cols(np.zeros(1000), x[:1000], x[:1000] + maxlen - 1), cols(np.zeros(1000), x[1000:2000], x[1000:2000] + maxlen),
                   cols(np.zeros(1000), x[2000:], x[2000:] + maxlen + 70_000))
    y = rng.integers(0, int(b[1].max()), 1000)
    empty = cols(np.zeros(1000), y, y - rng.integers(1, 50, 1000))                  # qe < qs: never matches
    hi = int(b[1].max())
    outside = cols(np.zeros(6), [-5000, -300, -1, hi + 1, hi + 255, hi + 256], [100, 0, 600, hi + 300, hi + 255, hi + 9000])
    p = rf.cat(past, last, longs, empty, outside, rf.sparse_probes(b, n_rand, 25))
    assert len(p[1]) <= n_rand + 10_000
    both_paths(ctx, ix, b, p)
    # the rest rows alone (nothing for the lean walk to find)
    both_paths(ctx, ix, b, rf.cat(past, longs, empty))
    ix.free()


def test_mark_regions_no_match_and_one_row(ctx):
    """(e) a batch without any match leaves every word clear; 50 000 rows that all match build row 1234 set one bit"""
    b = rf.sparse_build()
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    assert ix.layout()["slow"] == 0
    rng = np.random.default_rng(26)
    i = rng.integers(0, len(b[1]) - 1, 50_000)
    gaps = i * 512 + rng.integers(256, 512, len(i))
    none = both_paths(ctx, ix, b, cols(np.zeros(len(i)), gaps, gaps))
    assert not none.any()
    x = 1234 * 512 + rng.integers(0, 256, 50_000)
    one = both_paths(ctx, ix, b, cols(np.zeros(len(x)), x, x))
    assert (positions(one, len(b[1])) == [1234]).all()
    ix.free()


# ---------------------------------------------------------------- concurrency and ordering

def test_mark_first_call_after_overlapped_build(ctx):
    """build overlap on, device columns: mark_build as the first call on the index waits for the build's tail"""
    b = rf.level0_lean_build(False)
    rng = np.random.default_rng(27)
    p = rf.points(rng, 150_000, 0, int(b[1].max()), unknown=1 / 3)
    want = want_words(b, p)
    dp = [dev(c) for c in p]
    ctx.set_build_overlap(True)
    try:
        for path in ("direct", "regions"):
            dcols = [dev(c) for c in b]
            ix = ctx.build(pyivx.KIND_OVERLAP, *dcols, n_keys=1)
            m = dev(pyivx.Ctx.new_marks(ix.rows))
            with env(IVX_JOIN_PATH=path):
                ctx.mark_build(ix, *dp, m)
            ctx.synchronize()
            assert (host(m)[: len(want)] == want).all(), path
            ix.free()
    finally:
        ctx.set_build_overlap(False)


def test_two_contexts_mark_one_bitmap(ctx):
    b = direct_build(5000, 3, 31)
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=4)
    p = strict_probes(60_000, 3, 32)
    half = len(p[1]) // 2
    p1, p2 = tuple(c[:half] for c in p), tuple(c[half:] for c in p)
    other = pyivx.Ctx(0)
    try:
        m = dev(pyivx.Ctx.new_marks(ix.rows))
        d1, d2 = [dev(c) for c in p1], [dev(c) for c in p2]
        ctx.mark_build(ix, *d1, m)
        other.mark_build(ix, *d2, m)                                    # both may be in flight: device-scope atomic OR
        ctx.synchronize(); other.synchronize()
        got = host(ctx.bits_select(m, ix.rows, True))
        miss = host(other.bits_select(m, ix.rows, False))
    finally:
        other.close()
    wb = np.unique(orc.join(*b, *p, threads=4)[0])
    assert len(got) == len(wb) and (got == wb).all()
    assert (miss == np.setdiff1d(np.arange(ix.rows), wb)).all()
    ix.free()


def test_mark_between_count_and_fill(ctx):
    """a total-only count of the region path leaves its routed rows for the fill; a mark call in between drops them and
    the fill still returns the oracle's pairs"""
    b = rf.sparse_build()
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    p = rf.sparse_probes(b, 200_000, 33)
    wb, wp = orc.join(*b, *p, threads=4)
    with env(IVX_JOIN_PATH="regions"):
        for mem in ("host", "device"):
            pp = p if mem == "host" else [dev(c) for c in p]
            total = ctx.overlap_count(ix, *pp)
            assert total == len(wb)
            m = pyivx.Ctx.new_marks(ix.rows) if mem == "host" else dev(pyivx.Ctx.new_marks(ix.rows))
            ctx.mark_build(ix, *pp, m)
            ob, op = ctx.overlap_fill(ix, *pp, cap=total)
            if mem == "device":
                ctx.synchronize()
                ob, op, m = host(ob), host(op), host(m)
            assert len(ob) == total and (pair_set(ob, op) == pair_set(wb, wp)).all(), mem
            assert (m[: (ix.rows + 31) // 32] == words_of(np.unique(wb), ix.rows)).all(), mem
    ix.free()
