"""CPU-only: the two restatements of ivx_probe_nearest_dir that the GPU tests compare against (tests/nearest_dir_oracle.py).
A -- the contract's cursors -- with direction "any" and no cap is tied to the reference's pinned behaviour (oracle.nearest);
A equals B -- brute force -- wherever B is defined; and a hand-written table pins the rules one by one."""
import itertools

import numpy as np
import pytest

from oracle import oracle as orc

import nearest_dir_oracle as ndo

NULL = ndo.NULL_IDX


def _tables(seed, nb=2000, npr=6000, nkeys=3, span=40_000, degenerate=False):
    """random rows with many duplicated starts and ends (coordinates on a coarse lattice), a probe key without build rows"""
    rng = np.random.default_rng(seed)
    bk = rng.integers(0, nkeys, nb).astype(np.uint32)
    bs = (rng.integers(0, span // 8, nb) * 8).astype(np.int32)
    be = (bs + rng.integers(0, 40, nb) * 8).astype(np.int32)
    pk = rng.integers(0, nkeys + 1, npr).astype(np.uint32)
    ps = rng.integers(-50, span + 50, npr).astype(np.int32)
    pe = (ps + rng.integers(0, 300, npr)).astype(np.int32)
    ps[::7] = (ps[::7] // 8) * 8; pe[::5] = (pe[::5] // 8) * 8              # probe rows that touch build rows exactly
    pe = np.maximum(pe, ps)
    if degenerate:
        pe[::11] = ps[::11] - rng.integers(1, 30, len(ps[::11])).astype(np.int32)
        be[::13] = bs[::13] - 8
    return (bk, bs, be), (pk, ps, pe)


@pytest.mark.parametrize("degenerate", [False, True])
def test_any_without_a_cap_is_the_reference(degenerate):
    b, p = _tables(1 + degenerate, degenerate=degenerate)
    ix = ndo.NearIndex(*b)
    for k, ovl, strict in itertools.product((1, 2, 4), (True, False), (False, True)):
        wb, wp, wd = orc.nearest(*b, *p, k=k, overlap=ovl, strict=strict)
        gb, gp, gd = ix.query(*p, k=k, overlap=ovl, strict=strict)
        assert len(gb) == len(wb), (k, ovl, strict)
        assert (gb == wb).all() and (gp == wp).all() and (gd == wd).all(), (k, ovl, strict)
    # k = 0: one NULL row per probe row
    gb, gp, gd = ix.query(*p, k=0)
    assert (gb == NULL).all() and (gp == np.arange(len(p[0]))).all() and (gd == -1).all()


@pytest.mark.parametrize("build", ["default", "designed"])
def test_the_catalogue_case_bites(build):
    """the precondition of the catalogue's probe_nearest_dir cases (tests/entry_cases.py), on the restatement alone: on both
    builds the walks use, every one-sided call without overlaps and within the cap answers at least 100 of the 1 000 rows with
    a neighbour at distance > 0 and leaves at least 100 NULL -- a kernel that ignored the direction, the cap or
    include_overlaps would change rows of either kind.  (On the designed build every row overlaps a build row: with
    include_overlaps the cursors are never reached there.)"""
    import entry_cases as ec
    from test_gpu_entry_state import designed         # (importing the walk's module needs no GPU)
    assert ec.ivals(1000, 3)[0].dtype == np.uint32 and ec.SHAPE["cols"] is None
    b = ec.ivals(1000, 1) if build == "default" else designed()
    oix = ndo.NearIndex(*b)
    one_sided = [(d, ovl, D) for d, ovl, D in ec.NEAR_DIR_CALLS if d != "any" and not ovl and D >= 0]
    assert sorted(d for d, _, _ in one_sided) == ["after", "before"] and all(D == 32 for _, _, D in one_sided)
    for k in (1, 2):
        want = ec.nearest_dir_want(oix, 1000, k)
        assert sorted(want) == sorted(ec.near_dir_tag(*c) for c in ec.NEAR_DIR_CALLS)
        for call in one_sided:
            wb, wp, wd = want[ec.near_dir_tag(*call)]
            found = np.unique(wp[(wb != NULL) & (wd > 0)])
            nulls = wp[wb == NULL]
            assert len(found) >= 100 and len(nulls) >= 100, (build, k, call, len(found), len(nulls))
            assert (wd[wb != NULL] <= 32).all() and (wd[wb != NULL] > 0).all(), (build, k, call)
        # ... and the two sides, the cap and include_overlaps each change the answer
        t = ec.near_dir_tag
        for a, c in ((t("before", 0, 32), t("after", 0, 32)), (t("before", 0, 32), t("before", 0, -1)), (t("after", 0, -1), t("after", 1, -1))):
            assert len(want[a][0]) != len(want[c][0]) or (want[a][0] != want[c][0]).any(), (build, k, a, c)


def _as_lists(n, res):
    out = {i: [] for i in range(n)}
    for b, p, d in zip(*res):
        if b != NULL:
            out[int(p)].append((int(b), int(d)))
    return out


def test_cursors_equal_brute_force():
    b, p = _tables(3, nb=240, npr=400, span=3000)
    ix = ndo.NearIndex(*b)
    checked = 0
    for direction, ovl, strict, k, D in itertools.product(ndo.DIRECTIONS, (True, False), (False, True), (1, 3), (None, 0, 1, 50, 10**9)):
        got = _as_lists(len(p[0]), ix.query(*p, k=k, overlap=ovl, strict=strict, direction=direction, max_distance=D))
        want = ndo.brute(*b, *p, k=k, overlap=ovl, strict=strict, direction=direction, max_distance=D)
        assert len(want) > 350                                              # (a one-base row is inverted under strict: not B's)
        for i, w in want.items():
            assert got[i] == w, (direction, ovl, strict, k, D, i)
        checked += len(want)
    assert checked > 40_000


# one key's build rows, and a second key that only the probe side has
#            row:  0         1         2         3         4         5
HAND_BUILD = [(0, 10, 20), (0, 30, 40), (0, 35, 40), (0, 60, 70), (0, 60, 65), (0, 100, 110)]


def _hand(probe, **kw):
    bk, bs, be = (np.array(c) for c in zip(*HAND_BUILD))
    pk, ps, pe = (np.array([c]) for c in probe)
    b, _, d = ndo.nearest_dir(bk.astype(np.uint32), bs.astype(np.int32), be.astype(np.int32), pk.astype(np.uint32), ps.astype(np.int32),
                              pe.astype(np.int32), **kw)
    return [(int(x) if x != NULL else None, int(y)) for x, y in zip(b, d)]


def test_hand_written_table():
    none = [(None, -1)]
    # a probe row before all build rows of its key: nothing upstream, the first row downstream
    assert _hand((0, 1, 5), direction="before") == none
    assert _hand((0, 1, 5), direction="after") == [(0, 5)]
    assert _hand((0, 1, 5), direction="upstream") == none and _hand((0, 1, 5), direction="downstream") == [(0, 5)]
    # ... after all of them
    assert _hand((0, 200, 210), direction="after") == none
    assert _hand((0, 200, 210), direction="before") == [(5, 90)]
    # ... between two: each side's own, the nearer of both for "any"
    assert _hand((0, 45, 50), direction="before") == [(2, 5)]
    assert _hand((0, 45, 50), direction="after") == [(4, 10)]
    assert _hand((0, 45, 50)) == [(2, 5)]
    # equal ends with different starts: the larger start first (by_end read downwards), then the other
    assert _hand((0, 45, 50), direction="before", k=2) == [(2, 5), (1, 5)]
    # equal starts with different ends: (start, end, row) upwards
    assert _hand((0, 45, 50), direction="after", k=2) == [(4, 10), (3, 10)]
    # left before right at equal distance
    assert _hand((0, 50, 50), k=4) == [(2, 10), (1, 10), (4, 10), (3, 10)]
    # touching: an overlap when not strict -- it comes first whatever the direction, and only include_overlaps removes it
    assert _hand((0, 40, 50), direction="after") == [(1, 0)]
    assert _hand((0, 40, 50), direction="after", overlap=False) == [(4, 10)]
    assert _hand((0, 40, 50), direction="before", overlap=False) == [(0, 20)]
    # ... under strict the touching rows are upstream rows at reported distance 0, and pass a cap of 0
    assert _hand((0, 40, 50), direction="before", strict=True, overlap=False) == [(2, 0)]
    assert _hand((0, 40, 50), direction="before", strict=True, overlap=False, k=3, max_distance=0) == [(2, 0), (1, 0)]
    assert _hand((0, 40, 50), direction="after", strict=True, max_distance=0) == none
    # a cap: the distance itself passes, one less does not; an overlap always passes
    assert _hand((0, 45, 50), direction="after", max_distance=10) == [(4, 10)]
    assert _hand((0, 45, 50), direction="after", max_distance=9) == none
    assert _hand((0, 45, 50), max_distance=4) == none
    assert _hand((0, 45, 50), max_distance=5, k=4) == [(2, 5), (1, 5)]
    assert _hand((0, 38, 50), max_distance=0, k=4) == [(1, 0), (2, 0)]
    # k larger than the rows on that side
    assert _hand((0, 45, 50), direction="before", k=5) == [(2, 5), (1, 5), (0, 25)]
    assert _hand((0, 80, 90), direction="after", k=5) == [(5, 10)]
    # a key with no build rows; k = 0
    assert _hand((1, 45, 50), direction="before") == none and _hand((1, 45, 50), k=3, max_distance=10) == none
    assert _hand((0, 45, 50), direction="before", k=0) == none
