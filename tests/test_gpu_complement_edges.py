"""-m gpu: complement where its views are cut at the merged runs' starts and ends, at the launch edges of its count and
fill kernels, and in its view bookkeeping.

For regular input (merged ends ascending) a view's output count is two partition points into the merged runs plus a
prefix sum of the non-empty gaps (k_comp_count), and the rows are filled one thread per OUTPUT row (k_comp_fill_rows);
a single input row with end < start anywhere sends every view through the serial walk (view_walk_serial) instead.  The
input decides the path, so the same views run three times: as they are, with an inverted row in another key, with one in
their own key.  Everything is compared bit-exactly with the CPU oracle, strict False and True; where the construction
makes the row count obvious it is asserted too."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

ST = 256                    # csrc/ivx_sweep.hip: threads of a workgroup (one per view, per merged run, per output row)
BIG = np.iinfo(np.int64).max


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


def cols(key, s, e):
    s = np.asarray(s, np.int64); e = np.asarray(e, np.int64)
    k = np.full(len(s), key, np.uint32) if np.isscalar(key) else np.asarray(key, np.uint32)
    return k, s, e


def cat(*sides):
    return tuple(np.concatenate([x[i] for x in sides]) for i in range(3))


EMPTY = cols(0, [], [])


def walks_serially(inp):
    """the merged runs' ends descend somewhere inside a key (both strict modes): every view takes view_walk_serial"""
    for strict in (False, True):
        k, _, e, _ = orc.merge(*inp, min_dist=0, strict=strict)
        if not ((k[1:] == k[:-1]) & (e[1:] < e[:-1])).any():
            return False
    return True


def check(ctx, inp, views, n_keys, total=None, shuffle=True):
    """both strict modes against the oracle; once more with input and views shuffled.  -> the non-strict result"""
    first = None
    rng = np.random.default_rng(3)
    for perm in ((False, True) if shuffle else (False,)):
        I, V = inp, views
        if perm:
            p = rng.permutation(len(inp[0])); I = tuple(x[p] for x in inp)
            if views is not None:
                p = rng.permutation(len(views[0])); V = tuple(x[p] for x in views)
        for strict in (False, True):
            v = V if V is not None else (None, None, None)
            got = ctx.complement(*I, *v, n_keys=n_keys, strict=strict)
            want = orc.complement(*I, *v, strict=strict)
            if total is not None:
                assert len(want[0]) == (total[strict] if isinstance(total, (tuple, list)) else total), (len(want[0]), total, strict)
            for g, w in zip(got, want):
                assert len(g) == len(w), (strict, perm, len(g), len(w))
                assert g.dtype == w.dtype and (g == w).all(), (strict, perm)
            if first is None:
                first = got
    return first


# ------------------------------------------------------------------ views cut at run boundaries

RUNS = [(1000, 2000), (2000, 3000), (5000, 6000)]       # two that touch (one run unless strict), a gap, a third


def boundary_case(key=1):
    rows = []
    for ms, me in RUNS:                                 # every run from three overlapping rows
        third = (me - ms) // 3
        rows += [(ms, ms + 2 * third), (ms + third, me), (ms + third, ms + 2 * third)]
    s, e = zip(*rows)
    pts = sorted({p + d for ms, me in RUNS for p in (ms, me) for d in (-1, 0, 1)})
    vs, ve = zip(*[(a, b) for a in pts for b in pts])   # every pair: vs >= ve and views inside one run included
    return cols(key, s, e), cols(key, vs, ve)


@pytest.mark.parametrize("inverted", ["none", "other_key", "same_key"])
def test_views_cut_at_run_starts_and_ends(ctx, inverted):
    inp, views = boundary_case()
    assert 200 <= len(views[0]) <= 400
    if inverted == "other_key":
        inp = cat(inp, cols(0, [950, 100], [400, 900]))
    elif inverted == "same_key":
        inp = cat(inp, cols(1, [4000], [2500]))           # a run of its own in the gap, ending below the run in front of it
    assert walks_serially(inp) == (inverted != "none")
    got = check(ctx, inp, views, 3)
    assert len(got[0]) > 0
    # the implicit views of key 0 (inverted == other_key) sort first
    assert (np.diff(got[0].astype(np.int64)) >= 0).all()


def test_views_cut_at_run_boundaries_far_out(ctx):
    """the same cuts with 2^40 added to every coordinate"""
    inp, views = boundary_case()
    off = 1 << 40
    check(ctx, (inp[0], inp[1] + off, inp[2] + off), (views[0], views[1] + off, views[2] + off), 2)


# ------------------------------------------------------------------ launch edges

def runs(m, key=0, width=50):
    j = np.arange(m, dtype=np.int64)
    return cols(key, 100 * j, 100 * j + width)


@pytest.mark.parametrize("gaps", [254, 255, 256, 257])
def test_one_view_across_many_gaps(ctx, gaps):
    """k_comp_fill_rows: one thread per output row, all of one view; total at ST - 2 .. ST + 3"""
    inp = runs(gaps + 1)
    inside = cols(0, [10], [100 * gaps + 20])            # from inside the first run to inside the last: the gaps alone
    check(ctx, inp, inside, 1, total=gaps)
    around = cols(0, [-5], [100 * gaps + 70])            # a head in front and a tail behind
    check(ctx, inp, around, 1, total=gaps + 2)
    odd = cat(inp, cols(0, [100 * gaps + 330], [10]))
    assert walks_serially(odd) and not walks_serially(inp)
    check(ctx, odd, around, 1, total=gaps + 2)


@pytest.mark.parametrize("nw", [1, 255, 256, 257])
def test_view_counts_around_a_workgroup(ctx, nw):
    inp = runs(40)
    i = np.arange(nw, dtype=np.int64)
    views = cols(0, 13 * i, 13 * i + 9 + i % 7)
    check(ctx, inp, views, 1)
    # views alone: they come back whole, in (start, end) order
    got = check(ctx, EMPTY, views, 1, total=nw)
    assert (got[1] == views[1]).all() and (got[2] == views[2]).all()


@pytest.mark.parametrize("m", [0, 1, 256, 257])
def test_run_counts_around_a_workgroup(ctx, m):
    """k_run_gaps and k_gap_index: one thread per merged run (and one for the slot behind them)"""
    inp = runs(m, key=0) if m else EMPTY
    views = cols(0, [-7, 10, 100 * m - 60, 100 * (m // 2) + 50, 3], [100 * m + 9, 100 * m - 80, 100 * m + 1, 100 * (m // 2) + 100, 3])
    # [-7, 100m+9): a head, m-1 gaps, a tail
    check(ctx, inp, tuple(x[:1] for x in views), 1, total=(m + 1) if m else 1)
    check(ctx, inp, views, 1)
    if m:
        odd = cat(inp, cols(0, [100 * m + 500], [5]))
        assert walks_serially(odd) and not walks_serially(inp)
        check(ctx, odd, views, 1)


# ------------------------------------------------------------------ view bookkeeping

def test_implicit_views_view_only_keys_and_keys_with_neither(ctx):
    """keys 0, 3: input and views; 1, 5: input only (implicit [0, i64::MAX)); 2, 6: views only; 4, 7: neither"""
    inp = cat(runs(5, key=0), runs(3, key=1), runs(4, key=3), runs(2, key=5))
    views = cat(cols(0, [20, 20, 0, 130], [260, 260, 1000, 170]),      # a duplicate, overlapping ones
                cols(6, [50, 5], [60, 500]), cols(3, [-10, 120], [90, 480]), cols(2, [7, 7, 1], [9, 9, 100]))
    got = check(ctx, inp, views, 8)
    k = got[0].tolist()
    with_input = [x for x in k if x in (0, 1, 3, 5)]
    # keys with input first, in key order; the view-only keys behind all of them, in key order
    assert k == sorted(with_input) + sorted(x for x in k if x in (2, 6)) and set(k) == {0, 1, 2, 3, 5, 6}
    assert k.count(2) == 3 and k.count(6) == 2                           # view-only: every view row as it is, duplicates too
    last = {key: max(i for i, x in enumerate(k) if x == key) for key in (1, 5)}
    assert got[2][last[1]] == BIG and got[2][last[5]] == BIG            # the implicit views' tails


@pytest.mark.parametrize("nkeys", [2049, 5000])
def test_more_keys_than_views(ctx, nkeys):
    """k_views_gather's grid comes from the key count: implicit views for every third key, three explicit views"""
    keys = np.arange(0, nkeys, 3, dtype=np.uint32)
    inp = cat(cols(keys, np.full(len(keys), 100), np.full(len(keys), 200)), cols(keys[::2], np.full(len(keys[::2]), 300), np.full(len(keys[::2]), 400)))
    views = cols([0, nkeys - 1, 1], [50, 1, 2], [350, 9, 8])      # key 0 has input; keys 1 and nkeys - 1 are view-only
    assert (nkeys - 1) % 3 != 0 and len(keys) + 2 > 3
    got = check(ctx, inp, views, nkeys)
    # key 0's view: [50, 100) and [200, 300); an implicit view: [0, 100), [200, BIG) or [0, 100), [200, 300), [400, BIG)
    n3 = len(keys[::2]) - 1
    assert (got[0] == 0).sum() == 2 and len(got[0]) == 2 + 3 * n3 + 2 * (len(keys) - 1 - n3) + 2
    assert got[0][-2:].tolist() == [1, nkeys - 1] and (got[2] == BIG).sum() == len(keys) - 1


def test_input_that_covers_its_implicit_view(ctx):
    inp = cat(cols(0, [0], [BIG]), cols(1, [0, 10], [5, BIG]), cols(2, [-5, 3], [4, BIG]))
    got = check(ctx, inp, None, 3, total=1)
    assert got[0].tolist() == [1] and got[1].tolist() == [5] and got[2].tolist() == [10]


def raw_complement(ctx, inp, views, n_keys, strict, cap, room):
    L = pyivx.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    inp = tuple(np.ascontiguousarray(x) for x in inp); views = tuple(np.ascontiguousarray(x) for x in views)
    args = (ctx.h, C.c_int(pyivx.MEM_HOST), p(inp[0]), p(inp[1]), p(inp[2]), C.c_uint64(len(inp[0])),
            p(views[0]), p(views[1]), p(views[2]), C.c_uint64(len(views[0])), C.c_uint32(n_keys), C.c_int(int(strict)))
    m = C.c_uint64(0)
    if room is None:
        return L.ivx_complement(*args, None, None, None, C.c_uint64(0), C.byref(m)), m.value, None
    bufs = [np.full(room, 0x5A5A5A5A, dt) for dt in (np.uint32, np.int64, np.int64)]
    st = L.ivx_complement(*args, *[p(b) for b in bufs], C.c_uint64(cap), C.byref(m))
    return st, m.value, bufs


@pytest.mark.parametrize("inverted", [False, True])
def test_count_only_and_capacity(ctx, inverted):
    inp, views = boundary_case()
    inp, views = cat(inp, runs(300, key=0)), cat(views, cols(0, [-5], [100 * 300]))      # more output rows than one workgroup fills
    if inverted:
        inp = cat(inp, cols(1, [4000], [2500]))
    assert walks_serially(inp) == inverted
    for strict in (False, True):
        want = orc.complement(*inp, *views, strict=strict)
        total = len(want[0])
        assert total > ST
        st, m, _ = raw_complement(ctx, inp, views, 2, strict, 0, None)
        assert st == pyivx.OK and m == total == len(ctx.complement(*inp, *views, n_keys=2, strict=strict)[0])
        st, m, bufs = raw_complement(ctx, inp, views, 2, strict, total - 1, total + 32)
        assert st == pyivx.ERR_CAPACITY and m == total
        for b in bufs:
            assert (b[total - 1:] == 0x5A5A5A5A).all()
        for cap in (total, total + 1):
            st, m, bufs = raw_complement(ctx, inp, views, 2, strict, cap, total + 32)
            assert st == pyivx.OK and m == total
            for b, w in zip(bufs, want):
                assert (b[:total] == w).all() and (b[total:] == 0x5A5A5A5A).all()
