"""-m gpu: ivx_probe_nearest_dir through the C ABI (include/ivx_nearest.h) -- nearest on one side only and / or within a
distance cap -- against the cursor restatement A of tests/nearest_dir_oracle.py (tied to the reference and to brute force in
tests/test_nearest_dir_cpu.py): the direct k = 1 kernel, the routed one with its gated in-place pass, and the k > 1 kernel, each
per direction with and without a cap."""
import ctypes as C
import functools
import itertools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, synth

import nearest_dir_oracle as ndo

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

NULL = pyivx.NULL_IDX
I32_MIN, I32_MAX = -2**31, 2**31 - 1
CAPS = (None, 0, 1, 50, 10**9)
PATHS = ("direct", "routed")


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def tables(seed):
    """the shapes of test_nearest_random: build 20 000 rows, probe 60 000 rows over 1, 4, 24 or 2 keys and one probe key
    without build rows; seed 3 has degenerate rows (end < start) on both sides and duplicated starts"""
    nk = [1, 4, 24, 2][seed]
    bk, bs, be = synth(20_000, 150 + seed, nkeys=nk, mean_len=[300, 3000][seed % 2], span=3_000_000)
    pk, ps, pe = synth(60_000, 160 + seed, nkeys=nk + 1, mean_len=100, span=3_000_000)
    rng = np.random.default_rng(seed)
    # some probe rows that start where a build row of their key ends (strict: reported distance 0 on the left cursor)
    m = len(ps[5::9])
    src = rng.integers(0, len(bk), m)
    pk[5::9] = bk[src]; ps[5::9] = be[src]; pe[5::9] = be[src] + 40
    if seed == 3:
        be[::17] = bs[::17] - 1 - rng.integers(0, 50, len(be[::17])).astype(np.int32)
        pe[::13] = ps[::13] - 1 - rng.integers(0, 50, len(pe[::13])).astype(np.int32)
        length = be[::23] - bs[::23]                      # duplicate starts -> tie-breaks on end / row (the rows keep their length:
        bs[::23] = bs[1::23][: len(bs[::23])]            #  a row across the whole key would make A step through the key per probe row)
        be[::23] = bs[::23] + length
    for a in (bk, bs, be, pk, ps, pe):
        a.setflags(write=False)
    return (bk, bs, be), (pk, ps, pe), nk + 1, ndo.NearIndex(bk, bs, be)


@functools.lru_cache(maxsize=4)
def want(seed, k, ovl, strict, direction, D):
    _, p, _, oix = tables(seed)
    return oix.query(*p, k=k, overlap=ovl, strict=strict, direction=direction, max_distance=D)


@pytest.fixture(scope="module")
def indexes(ctx):
    made = {}

    def get(seed):
        if seed not in made:
            b, _, nk, _ = tables(seed)
            made[seed] = ctx.build(pyivx.KIND_NEAREST, *b, n_keys=nk)
        return made[seed]
    yield get
    for ix in made.values():
        ix.free()


def run(ctx, ix, p, path=None, **kw):
    if path is None:
        return ctx.nearest_dir(ix, *p, **kw)
    os.environ["IVX_NEAREST_PATH"] = path
    try:
        return ctx.nearest_dir(ix, *p, **kw)
    finally:
        del os.environ["IVX_NEAREST_PATH"]


def same(got, exp, what, distance=True):
    assert len(got[0]) == len(exp[0]), what
    assert (got[0] == exp[0]).all() and (got[1] == exp[1]).all(), what
    if distance:
        assert (got[2] == exp[2]).all(), what
    else:
        assert got[2] is None, what


# ---------------------------------------------------------------- "any" without a cap is ivx_probe_nearest

@pytest.mark.parametrize("seed", range(4))
def test_any_without_a_cap_is_nearest(ctx, indexes, seed):
    _, p, _, _ = tables(seed)
    ix = indexes(seed)
    for k, (ovl, strict), path in itertools.product((0, 1, 3), ((True, False), (False, True)), PATHS):
        os.environ["IVX_NEAREST_PATH"] = path
        try:
            exp = ctx.nearest(ix, *p, k=k, overlap=ovl, strict=strict)
            expn = ctx.nearest(ix, *p, k=k, overlap=ovl, strict=strict, distance=False)
        finally:
            del os.environ["IVX_NEAREST_PATH"]
        same(run(ctx, ix, p, path, k=k, overlap=ovl, strict=strict), exp, (k, ovl, strict, path))
        same(run(ctx, ix, p, path, k=k, overlap=ovl, strict=strict, direction="any", max_distance=None, distance=False), expn,
             (k, ovl, strict, path), distance=False)
        same(exp, want(seed, k, ovl, strict, "any", None), (k, ovl, strict, path, "A"))


# ---------------------------------------------------------------- every direction, overlap, strict and cap

@pytest.mark.parametrize("direction", ndo.DIRECTIONS)
@pytest.mark.parametrize("seed", range(4))
def test_k1_direct_and_routed(ctx, indexes, seed, direction):
    _, p, _, _ = tables(seed)
    ix = indexes(seed)
    for ovl, strict, D in itertools.product((True, False), (False, True), CAPS):
        exp = want(seed, 1, ovl, strict, direction, D)
        for path in PATHS:
            what = (direction, ovl, strict, D, path)
            same(run(ctx, ix, p, path, overlap=ovl, strict=strict, direction=direction, max_distance=D), exp, what)
            same(run(ctx, ix, p, path, overlap=ovl, strict=strict, direction=direction, max_distance=D, distance=False), exp, what, distance=False)


@pytest.mark.parametrize("direction", ndo.DIRECTIONS)
@pytest.mark.parametrize("seed", range(4))
def test_k_above_one(ctx, indexes, seed, direction):
    _, p, _, _ = tables(seed)
    ix = indexes(seed)
    for k, ovl, strict, D in itertools.product((2, 5), (True, False), (False, True), CAPS):
        what = (direction, k, ovl, strict, D)
        same(run(ctx, ix, p, k=k, overlap=ovl, strict=strict, direction=direction, max_distance=D), want(seed, k, ovl, strict, direction, D), what)
    same(run(ctx, ix, p, k=5, direction=direction, max_distance=50, distance=False), want(seed, 5, True, False, direction, 50), direction, distance=False)


@pytest.mark.parametrize("seed", [1, 3])
def test_sorted_probe_rows_are_answered_in_place(ctx, indexes, seed):
    # probe rows already in (key, start) order: the routed path moves nothing and the gated direct kernel answers
    _, (pk, ps, pe), _, oix = tables(seed)
    o = np.lexsort((ps, pk))
    p = (pk[o].copy(), ps[o].copy(), pe[o].copy())
    ix = indexes(seed)
    for direction, (ovl, strict), D in itertools.product(ndo.DIRECTIONS, ((True, False), (False, True)), (None, 50)):
        if direction == "any" and D is None:
            continue
        exp = oix.query(*p, k=1, overlap=ovl, strict=strict, direction=direction, max_distance=D)
        same(run(ctx, ix, p, "routed", overlap=ovl, strict=strict, direction=direction, max_distance=D), exp, (direction, ovl, strict, D))


def test_aliases(ctx, indexes):
    _, p, _, _ = tables(1)
    ix = indexes(1)
    same(run(ctx, ix, p, direction="upstream", max_distance=50), want(1, 1, True, False, "before", 50), "upstream")
    same(run(ctx, ix, p, direction="downstream", overlap=False), want(1, 1, False, False, "after", None), "downstream")
    with pytest.raises(ValueError):
        ctx.nearest_dir(ix, *p, direction="left")
    with pytest.raises(ValueError):
        ctx.nearest_dir(ix, *p, max_distance=-2)


# ---------------------------------------------------------------- edge shapes

def all_forms(ctx, ix, oix, p, what, ks=(1, 3), caps=(None, 50), paths=PATHS):
    for direction, ovl, strict, D, k in itertools.product(ndo.DIRECTIONS, (True, False), (False, True), caps, ks):
        exp = oix.query(*p, k=k, overlap=ovl, strict=strict, direction=direction, max_distance=D)
        for path in (paths if k == 1 else (None,)):
            same(run(ctx, ix, p, path, k=k, overlap=ovl, strict=strict, direction=direction, max_distance=D), exp, (what, direction, ovl, strict, D, k, path))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_small_batches(ctx, indexes, n):
    _, (pk, ps, pe), _, oix = tables(1)
    all_forms(ctx, indexes(1), oix, (pk[100:100 + n].copy(), ps[100:100 + n].copy(), pe[100:100 + n].copy()), n)


@pytest.mark.parametrize("per_wave", [64, 32])
def test_keys_per_wavefront(ctx, indexes, per_wave):
    # wavefronts that hold one key take their per-key tables through the scalar unit; with two keys they fall back
    _, (pk, ps, pe), nk, oix = tables(2)
    n = 64 * 40
    key = ((np.arange(n) // per_wave) % nk).astype(np.uint32)               # (the last key has no build rows)
    all_forms(ctx, indexes(2), oix, (key, ps[:n].copy(), pe[:n].copy()), per_wave, ks=(1,), paths=("direct",))


def test_one_build_row_and_empty_index(ctx):
    _, (pk, ps, pe), _, _ = tables(0)
    p = (pk[:3000].copy(), ps[:3000].copy(), pe[:3000].copy())
    b = (np.zeros(1, np.uint32), np.array([1_500_000], np.int32), np.array([1_500_400], np.int32))
    ix = ctx.build(pyivx.KIND_NEAREST, *b, n_keys=2)
    all_forms(ctx, ix, ndo.NearIndex(*b), p, "one row", caps=(None, 100_000))
    ix.free()
    b = (np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    ix = ctx.build(pyivx.KIND_NEAREST, *b, n_keys=2)
    all_forms(ctx, ix, ndo.NearIndex(*b), p, "empty")
    got = run(ctx, ix, p, direction="after", max_distance=5)
    assert (got[0] == NULL).all() and (got[1] == np.arange(3000)).all() and (got[2] == -1).all()
    ix.free()


def test_cap_at_the_true_distance(ctx, indexes):
    _, (pk, ps, pe), _, oix = tables(1)
    ix = indexes(1)
    for direction in ("before", "after"):
        b, _, d = oix.query(pk, ps, pe, overlap=False, direction=direction)
        i = int(np.flatnonzero(d > 1)[0])
        p = (pk[i:i + 1].copy(), ps[i:i + 1].copy(), pe[i:i + 1].copy())
        for path in PATHS:
            gb, _, gd = run(ctx, ix, p, path, overlap=False, direction=direction, max_distance=int(d[i]))
            assert (int(gb[0]), int(gd[0])) == (int(b[i]), int(d[i])), (direction, path)
            gb, _, gd = run(ctx, ix, p, path, overlap=False, direction=direction, max_distance=int(d[i]) - 1)
            assert (int(gb[0]), int(gd[0])) == (NULL, -1), (direction, path)
        gb, _, gd = run(ctx, ix, p, k=2, overlap=False, direction=direction, max_distance=int(d[i]) - 1)
        assert (int(gb[0]), int(gd[0])) == (NULL, -1) and len(gb) == 1, direction


def test_extreme_coordinates_under_strict(ctx):
    # strict moves the query by one with wadd / wsub: at INT32_MAX / INT32_MIN it wraps, as the reference's wrapping_add does
    b = (np.zeros(5, np.uint32), np.array([I32_MIN, I32_MIN + 10, -5, I32_MAX - 20, I32_MAX - 3], np.int32),
         np.array([I32_MIN + 4, I32_MIN + 30, 5, I32_MAX - 10, I32_MAX], np.int32))
    ps = np.array([I32_MIN, I32_MIN, I32_MIN + 4, 0, I32_MAX, I32_MAX - 3, I32_MIN, I32_MAX - 9, I32_MIN + 5], np.int32)
    pe = np.array([I32_MIN, 3, I32_MIN + 10, I32_MAX, I32_MAX, I32_MAX, I32_MAX, I32_MAX - 4, I32_MIN + 9], np.int32)
    p = (np.zeros(len(ps), np.uint32), ps, pe)
    ix = ctx.build(pyivx.KIND_NEAREST, *b, n_keys=1)
    oix = ndo.NearIndex(*b)
    for direction, ovl, strict, D, k in itertools.product(ndo.DIRECTIONS, (True, False), (True, False), (None, 0, 6, 2**31), (1, 2, 5)):
        exp = oix.query(*p, k=k, overlap=ovl, strict=strict, direction=direction, max_distance=D)
        for path in (PATHS if k == 1 else (None,)):
            same(run(ctx, ix, p, path, k=k, overlap=ovl, strict=strict, direction=direction, max_distance=D), exp, (direction, ovl, strict, D, k, path))
    ix.free()


def test_k_beyond_the_rows_on_a_side(ctx):
    # key 0: three rows before the probe row and one behind it; k = 5
    b = (np.zeros(4, np.uint32), np.array([10, 30, 35, 100], np.int32), np.array([20, 40, 40, 110], np.int32))
    p = (np.zeros(1, np.uint32), np.array([45], np.int32), np.array([50], np.int32))
    ix = ctx.build(pyivx.KIND_NEAREST, *b, n_keys=1)
    gb, gp, gd = ctx.nearest_dir(ix, *p, k=5, direction="before")
    assert gb.tolist() == [2, 1, 0] and gp.tolist() == [0, 0, 0] and gd.tolist() == [5, 5, 25]
    gb, gp, gd = ctx.nearest_dir(ix, *p, k=5, direction="after")
    assert gb.tolist() == [3] and gd.tolist() == [50]
    gb, gp, gd = ctx.nearest_dir(ix, *p, k=5, direction="before", max_distance=5)
    assert gb.tolist() == [2, 1] and gd.tolist() == [5, 5]
    gb, gp, gd = ctx.nearest_dir(ix, *p, k=5, direction="after", max_distance=49)
    assert gb.tolist() == [NULL] and gd.tolist() == [-1]
    ix.free()


# ---------------------------------------------------------------- arguments

def raw(ctx, ix, p, n, k, direction, D, ob, op, od, cap, rows, strict=0, ovl=1):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return pyivx.lib().ivx_probe_nearest_dir(ctx.h, ix.h, pyivx.MEM_HOST, ptr(p[0]), ptr(p[1]), ptr(p[2]), n, strict, k, ovl, direction, D,
                                             ptr(ob), ptr(op), ptr(od), cap, rows)


def test_capacity_and_refusals(ctx, indexes):
    b, (pk, ps, pe), nk, oix = tables(1)
    ix = indexes(1)
    n = 2000
    p = (pk[:n].copy(), ps[:n].copy(), pe[:n].copy())

    def fresh(m):
        return np.full(m, 0xA5A5A5A5, np.uint32), np.full(m, 0xA5A5A5A5, np.uint32), np.full(m, 0x5A5A5A5A5A5A5A5A, np.int64)

    def untouched(ob, op, od):
        return (ob == 0xA5A5A5A5).all() and (op == 0xA5A5A5A5).all() and (od == 0x5A5A5A5A5A5A5A5A).all()

    # cap too small: IVX_ERR_CAPACITY with the rows it would take
    for k in (1, 3):
        exp = oix.query(*p, k=k, direction="before", max_distance=1000)
        ob, op, od = fresh(n * 3)
        rows = C.c_uint64(7)
        assert raw(ctx, ix, p, n, k, 1, 1000, ob, op, od, len(exp[0]) - 1, C.byref(rows)) == pyivx.ERR_CAPACITY, k
        assert rows.value == len(exp[0]), k
        rows = C.c_uint64(7)
        assert raw(ctx, ix, p, n, k, 1, 1000, ob, op, od, len(exp[0]), C.byref(rows)) == pyivx.OK, k
        assert rows.value == len(exp[0]) and (ob[:rows.value] == exp[0]).all() and (od[:rows.value] == exp[2]).all(), k
        assert (ob[rows.value:] == 0xA5A5A5A5).all()
    # a bad direction, a null column, another index kind: refused, nothing written
    cnt = ctx.build(pyivx.KIND_COUNT, *b, n_keys=nk)
    for status, index, direction, D, null in ((pyivx.ERR_INVALID, ix, 3, -1, None), (pyivx.ERR_INVALID, ix, -1, 10, None),
                                              (pyivx.ERR_INVALID, ix, 100, 10, None), (pyivx.ERR_INVALID, ix, 1, 10, "ob"),
                                              (pyivx.ERR_INVALID, ix, 2, -1, "op"), (pyivx.ERR_UNSUPPORTED, cnt, 1, 10, None),
                                              (pyivx.ERR_UNSUPPORTED, cnt, 0, 10, None)):
        for k in (1, 3):
            ob, op, od = fresh(n * 3)
            rows = C.c_uint64(7)
            got = raw(ctx, index, p, n, k, direction, D, None if null == "ob" else ob, None if null == "op" else op, od, n * 3, C.byref(rows))
            assert got == status, (status, direction, D, null, k)
            assert untouched(ob, op, od) and rows.value == (0 if status == pyivx.ERR_INVALID else 7), (status, direction, D, null, k)
    ob, op, od = fresh(n * 3)
    assert raw(ctx, ix, p, n, 1, 1, 10, ob, op, od, n * 3, None) == pyivx.ERR_INVALID and untouched(ob, op, od)
    with pytest.raises(pyivx.IvxError) as ei:
        ctx.nearest_dir(cnt, *p, direction="before")
    assert ei.value.status == pyivx.ERR_UNSUPPORTED
    cnt.free()
    # n = 0 is a no-op
    ob, op, od = fresh(8)
    rows = C.c_uint64(7)
    assert raw(ctx, ix, p, 0, 1, 2, 5, ob, op, od, 8, C.byref(rows)) == pyivx.OK and rows.value == 0 and untouched(ob, op, od)
