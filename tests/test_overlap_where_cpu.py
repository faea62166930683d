"""CPU-only: the restatement of the overlap thresholds (tests/overlap_where_oracle.py) against a brute force in Python integers
and against a boundary table written out by hand -- the documented bedtools cases -f 0.5, -f 0.5 -r and -f 0.5 -F 0.5 -e, a
pair exactly on a fraction's boundary and one base short of it, min_bases at len and len + 1, and a row that spans the whole
int32 range under the largest denominator.  The GPU tests compare the library with this restatement."""
import numpy as np
import pytest

import overlap_where_oracle as wo
from overlap_where_oracle import W

THRESHOLDS = [W(min_bases=20), W(probe=(1, 2)), W(build=(1, 2)), W(probe=(1, 2), build=(1, 2)), W(probe=(1, 2), build=(1, 2), either=1),
              W(probe=(1, 1)), W(min_bases=7, probe=(2, 3)), W(min_bases=3, probe=(1, 3), build=(1, 4), either=1)]


def tables(seed, nb=60, n=90):
    """small random tables over three keys (key 2 has no build rows, key 7 is unknown to the build side); probe rows with
    lengths -2 .. 40, some with end < start"""
    rng = np.random.default_rng(seed)
    bs = rng.integers(0, 400, nb)
    b = wo.cols(rng.integers(0, 2, nb), bs, bs + rng.integers(0, 60, nb))
    ps = rng.integers(-20, 420, n)
    p = wo.cols(rng.choice([0, 1, 2, 7], n), ps, ps + rng.integers(-2, 41, n))
    return b, p


def as_set(wb, wp):
    return set(zip(np.asarray(wb).tolist(), np.asarray(wp).tolist()))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_equals_brute_force(seed):
    b, p = tables(seed)
    want = wo.Want(b, p, threads=1)
    assert (np.asarray(p[2], np.int64) < np.asarray(p[1], np.int64)).any()
    for w in [None, W()] + THRESHOLDS:
        got = want.pairs(w)
        assert len(got[0]) == len(as_set(*got))
        assert as_set(*got) == as_set(*wo.brute_pairs(w, b, p)), w


def test_identity_keeps_every_pair_including_inverted_rows():
    b, p = tables(4)
    want = wo.Want(b, p, threads=1)
    inverted = np.asarray(p[2], np.int64)[want.wp] < np.asarray(p[1], np.int64)[want.wp]
    assert inverted.any(), "the table has no matched probe row with end < start"
    for w in (None, W(), W(min_bases=0, probe=(0, 5), build=(0, 0), either=1)):
        wb, wp = want.pairs(w)
        assert (wb == want.wb).all() and (wp == want.wp).all()
    # ... and any asked condition drops exactly those pairs first
    wb, wp = want.pairs(W(min_bases=1))
    assert as_set(wb, wp) == as_set(want.wb[~inverted], want.wp[~inverted])


def test_stricter_keeps_a_subset_and_either_a_superset():
    b, p = tables(5, 200, 300)
    want = wo.Want(b, p, threads=1)
    every = as_set(want.wb, want.wp)
    prev = every
    for m in (1, 5, 20, 45, 100):
        cur = as_set(*want.pairs(W(min_bases=m)))
        assert cur <= prev
        prev = cur
    assert not prev and len(every) > 100
    prev = every
    for num in (1, 2, 3, 4):
        cur = as_set(*want.pairs(W(probe=(num, 4))))
        assert cur <= prev
        prev = cur
    both = as_set(*want.pairs(W(probe=(1, 2), build=(1, 2))))
    either = as_set(*want.pairs(W(probe=(1, 2), build=(1, 2), either=1)))
    one = as_set(*want.pairs(W(probe=(1, 2)))), as_set(*want.pairs(W(build=(1, 2))))
    assert both == one[0] & one[1] and either == one[0] | one[1] and both < either < every
    # either without two fractions changes nothing
    assert as_set(*want.pairs(W(probe=(1, 2), either=1))) == one[0]


@pytest.mark.parametrize("case", wo.HAND_CASES, ids=[c[1] for c in wo.HAND_CASES])
def test_hand_table(case):
    w, what, expected = case
    b, p = wo.HAND_BUILD, wo.HAND_PROBE
    assert as_set(*wo.brute_pairs(w, b, p)) == expected, what
    assert as_set(*wo.Want(b, p, threads=1).pairs(w)) == expected, what


def test_hand_table_reductions():
    """per-row counts, exists, marks, aggregates and select of the hand table under -f 0.5 -F 0.5 -e, written out"""
    b, p = wo.HAND_BUILD, wo.HAND_PROBE
    want = wo.Want(b, p, threads=1)
    w = W(probe=(1, 2), build=(1, 2), either=1)                          # {(0, 0), (1, 0), (1, 1), (2, 2), (3, 4), (3, 5)}
    assert want.per_row(w).tolist() == [2, 1, 1, 0, 1, 1, 0]
    assert want.exists(w).tolist() == [1, 1, 1, 0, 1, 1, 0]
    assert want.marks(w).tolist() == [0b1111] and want.marks(W(build=(1, 1))).tolist() == [0b1000]
    assert want.marks(W(build=(1, 1)), prior=np.array([0b10000, 7], np.uint32)).tolist() == [0b11000, 7]
    val = np.array([10, -3, 7, 1 << 40], np.int64)
    a = want.agg(w, val)
    assert a["count"].tolist() == [2, 1, 1, 0, 1, 1, 0] and a["sum"].tolist() == [7, -3, 7, 0, 1 << 40, 1 << 40, 0]
    assert a["bases"].tolist() == [150, 100, 5, 0, 1 << 32, 1 << 31, 0]
    assert a["min"][0] == -3 and a["max"][0] == 10 and a["min"][3] == np.iinfo(np.int64).max
    idx, score = want.select(w, "max_overlap")
    assert idx.tolist() == [1, 1, 2, wo.sel.NULL_IDX, 3, 3, wo.sel.NULL_IDX] and score.tolist() == [100, 100, 5, 0, 1 << 32, 1 << 31, 0]
    # unfiltered, probe 1 would keep build 0 as well and probe 3 would have a winner
    idx0, _ = want.select(None, "first_row")
    assert idx0.tolist() == [0, 0, 2, 2, 3, 3, 0]
