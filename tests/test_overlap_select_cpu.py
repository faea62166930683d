"""CPU-only: the numpy restatement of ivx_probe_overlap_select that the GPU tests compare against
(tests/overlap_select_oracle.py, from the oracle's pairs) agrees with an independent O(n * m) brute force, with a table
computed by hand, and with the overlap aggregates' restatement where the two say the same thing."""
import numpy as np
import pytest

import overlap_agg_oracle as agg
import overlap_select_oracle as sel

NULL = sel.NULL_IDX


def cols(k, s, e):
    return (np.ascontiguousarray(k, np.uint32), np.ascontiguousarray(s, np.int32), np.ascontiguousarray(e, np.int32))


def same(a, b, what=None):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and len(x) == len(y) and (x == y).all(), (what, x, y)


VALUES = {
    "ties": lambda rng, n: rng.integers(-1, 2, n).astype(np.int32),
    "int32_extremes": lambda rng, n: rng.choice(np.array([-2**31, 2**31 - 1, -1, 0, 1], np.int64), n).astype(np.int32),
    "int64_extremes": lambda rng, n: rng.choice(np.array([-2**63, 2**63 - 1, -2**62, 2**62, -1, 0, 3], np.int64), n),
}


def tied_sides(rng):
    """few distinct intervals, each several times, in shuffled row order: every criterion meets ties"""
    nd, n, nk = int(rng.integers(1, 12)), int(rng.integers(1, 60)), int(rng.integers(1, 4))
    ds = rng.integers(-50, 300, nd)
    de = ds + rng.integers(0, 80, nd)
    dk = rng.integers(0, nk, nd)
    pick = rng.permutation(np.repeat(np.arange(nd), rng.integers(1, 5, nd)))
    b = cols(dk[pick], ds[pick], de[pick])
    # probe rows: keys the build side may lack (nk, nk + 3), some rows with end < start, some full-range
    ps = rng.integers(-80, 330, n)
    pe = ps + rng.integers(-3, 90, n)
    wide = rng.random(n) < 0.1
    ps, pe = np.where(wide, -2**31, ps), np.where(wide, 2**31 - 1, pe)
    return b, cols(rng.choice(np.concatenate([np.arange(nk), [nk, nk + 3]]), n), ps, pe)


@pytest.mark.parametrize("values", list(VALUES))
@pytest.mark.parametrize("by", sel.BY)
@pytest.mark.parametrize("seed", range(5))
def test_restatement_equals_brute_force(seed, by, values):
    rng = np.random.default_rng(300 + seed)
    b, p = tied_sides(rng)
    val = VALUES[values](rng, len(b[1]))
    got, want = sel.select(b, p, by, val, threads=1), sel.brute(b, p, by, val)
    same(got, want, (seed, by, values))
    assert ((got[0] == NULL) <= (got[1] == 0)).all()


# build rows (key, start, end, value) and, per probe row, the (winner, score) under each criterion -- computed by hand
B_HAND = [(0, 100, 200, 5),        # 0
          (0, 150, 160, 9),        # 1: contained in row 0
          (0, 300, 400, 7),        # 2
          (0, 300, 400, 7),        # 3: row 2 again
          (0, 350, 450, 7),        # 4: rows 2, 3, 4 tie on the value
          (0, 1000, 5000, -3),     # 5: contains row 6 and the probes on it
          (0, 1100, 1200, 2),      # 6
          (1, 100, 200, 1)]        # 7: the other key
NONE = (NULL, 0)
#          probe row            min_val  max_val  max_overlap min_overlap first_row last_row
P_HAND = [((0, 120, 170),      ((0, 5), (1, 9), (0, 51), (1, 11), (0, 0), (1, 1))),
          ((0, 210, 290),      (NONE,) * 6),                                                  # in a gap
          ((0, 340, 360),      ((2, 7), (2, 7), (2, 21), (4, 11), (2, 2), (4, 4))),           # three-way value tie; rows 2, 3: 21 bases each
          ((0, 390, 410),      ((2, 7), (2, 7), (4, 21), (2, 11), (2, 2), (4, 4))),           # rows 2, 3: 11 bases each
          ((0, 1150, 1160),    ((5, -3), (6, 2), (5, 11), (5, 11), (5, 5), (6, 6))),          # contained in both matches
          ((0, 50, 6000),      ((5, -3), (1, 9), (5, 4001), (1, 11), (0, 0), (6, 6))),        # contains every build row of key 0
          ((1, 150, 150),      ((7, 1), (7, 1), (7, 1), (7, 1), (7, 7), (7, 7))),
          ((2, 100, 200),      (NONE,) * 6)]                                                  # a key the build side lacks


def hand_sides():
    b = cols(*zip(*[r[:3] for r in B_HAND]))
    p = cols(*zip(*[r[0] for r in P_HAND]))
    return b, p, np.array([r[3] for r in B_HAND], np.int32)


def hand_want(by):
    k = sel.BY.index(by)
    return (np.array([r[1][k][0] for r in P_HAND], np.uint32), np.array([r[1][k][1] for r in P_HAND], np.int64))


@pytest.mark.parametrize("by", sel.BY)
def test_hand_computed_table(by):
    b, p, val = hand_sides()
    want = hand_want(by)
    same(sel.select(b, p, by, val, threads=1), want, by)
    same(sel.brute(b, p, by, val), want, by)
    same(sel.select(b, p, by, val.astype(np.int64), threads=1), want, by)


@pytest.mark.parametrize("seed", range(4))
def test_scores_agree_with_the_aggregates(seed):
    rng = np.random.default_rng(400 + seed)
    b, p = tied_sides(rng)
    val = rng.integers(-1000, 1000, len(b[1])).astype(np.int64)
    a = agg.aggregate(b, p, val, threads=1)
    some = a["count"] > 0
    for by, name in (("max_val", "max"), ("min_val", "min")):
        idx, score = sel.select(b, p, by, val, threads=1)
        assert ((idx != NULL) == some).all()
        assert (score[some] == a[name][some]).all() and (val[idx[some]] == a[name][some]).all()
    # FIRST_ROW / LAST_ROW bracket every other winner
    first, last = sel.select(b, p, "first_row", threads=1)[0], sel.select(b, p, "last_row", threads=1)[0]
    for by in sel.BY:
        idx = sel.select(b, p, by, val, threads=1)[0]
        assert (first[some] <= idx[some]).all() and (idx[some] <= last[some]).all()


def test_overlap_scores_are_the_bases_of_single_matches():
    # disjoint build rows and probe rows that reach one of them at most: the only match's length is `bases`
    bs = np.arange(50) * 100
    b = cols(np.zeros(50), bs, bs + 40)
    rng = np.random.default_rng(5)
    ps = rng.integers(-30, 5000, 300)
    p = cols(np.zeros(300), ps, ps + rng.integers(0, 55, 300))
    a = agg.aggregate(b, p, np.zeros(50, np.int32), threads=1)
    assert a["count"].max() == 1 and (a["count"] == 0).any()
    for by in ("max_overlap", "min_overlap"):
        idx, score = sel.select(b, p, by, threads=1)
        assert (score == a["bases"]).all() and ((idx != NULL) == (a["count"] == 1)).all()
