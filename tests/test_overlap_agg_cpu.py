"""CPU-only: the numpy restatement of ivx_probe_overlap_agg that the GPU tests compare against (tests/overlap_agg_oracle.py,
from the oracle's pairs) agrees with an independent O(n * m) brute force, and with a table computed by hand."""
import numpy as np
import pytest

from conftest import encode_keys
import overlap_agg_oracle as agg

I64_MAX, I64_MIN = agg.I64_MAX, agg.I64_MIN


def cols(k, s, e):
    return (np.ascontiguousarray(k, np.uint32), np.ascontiguousarray(s, np.int32), np.ascontiguousarray(e, np.int32))


def same(a, b):
    for name in agg.OUTPUTS:
        assert a[name].dtype == b[name].dtype and (a[name] == b[name]).all(), (name, a[name], b[name])


VALUES = {
    "small": lambda rng, n: rng.integers(-1000, 1000, n).astype(np.int32),
    "int32_extremes": lambda rng, n: rng.choice(np.array([-2**31, 2**31 - 1, -1, 0, 1], np.int64), n).astype(np.int32),
    "int64_extremes": lambda rng, n: rng.choice(np.array([-2**63, 2**63 - 1, -2**62, 2**62, -1, 0, 3], np.int64), n),
}


@pytest.mark.parametrize("values", list(VALUES))
@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_brute_force(seed, values):
    rng = np.random.default_rng(100 + seed)
    nb, n, nk = int(rng.integers(0, 40)), int(rng.integers(1, 60)), int(rng.integers(1, 4))
    bs = rng.integers(-50, 300, nb)
    b = cols(rng.integers(0, nk, nb), bs, bs + rng.integers(0, 80, nb))
    # probe rows: keys the build side may lack (nk, nk + 3), some rows with end < start, some full-range
    ps = rng.integers(-80, 330, n)
    pe = ps + rng.integers(-3, 90, n)
    wide = rng.random(n) < 0.1
    ps, pe = np.where(wide, -2**31, ps), np.where(wide, 2**31 - 1, pe)
    p = cols(rng.choice(np.concatenate([np.arange(nk), [nk, nk + 3]]), n), ps, pe)
    val = VALUES[values](rng, nb)
    got, want = agg.aggregate(b, p, val, threads=1), agg.brute(b, p, val)
    same(got, want)
    assert (got["count"] == 0).any() or nb > 0


def test_wrapping_and_full_range():
    # one probe and one build row over the whole int32 range: len = 2^32; four values of 2^62: the sum wraps to 0
    b = cols([0] * 4, [-2**31] * 4, [2**31 - 1] * 4)
    p = cols([0], [-2**31], [2**31 - 1])
    val = np.full(4, 2**62, np.int64)
    got = agg.aggregate(b, p, val, threads=1)
    assert got["count"][0] == 4 and got["sum"][0] == 0 and got["bases"][0] == 4 << 32 and got["wsum"][0] == 0
    assert got["min"][0] == 2**62 and got["max"][0] == 2**62
    same(got, agg.brute(b, p, val))
    # three int32 maxima: the sum passes 2^32 without wrapping
    got = agg.aggregate(tuple(c[:3] for c in b), p, np.full(3, 2**31 - 1, np.int32), threads=1)
    assert got["sum"][0] == 3 * (2**31 - 1) > 2**32


# (count, sum, min, max, bases, wsum) of the golden `targets` rows of chr1 over the golden `reads` of chr1 with values
# 1..6 in file order -- computed by hand
HAND = {
    (100, 190): (2, 3, 1, 2, 42, 43),
    (200, 290): (2, 3, 1, 2, 142, 233),
    (400, 600): (2, 7, 3, 4, 203, 710),
    (10000, 20000): (1, 6, 6, 6, 1, 6),
    (22100, 22100): (1, 5, 5, 5, 1, 5),
}


def golden_sides(golden):
    reads = [r for r in golden.rows("reads") if r[0] == "chr1"]
    targets = [r for r in golden.rows("targets") if r[0] == "chr1"] + [["chr3", 100, 190]]
    names, (b, p) = encode_keys(reads, targets)
    return names, cols(*b), cols(*p), np.arange(1, len(reads) + 1, dtype=np.int32), targets


def test_hand_computed_golden_table(golden):
    names, b, p, val, targets = golden_sides(golden)
    assert len(val) == 6 and names == ["chr1", "chr3"]
    for got in (agg.aggregate(b, p, val, threads=1), agg.brute(b, p, val), agg.aggregate(b, p, val.astype(np.int64), threads=1)):
        for i, t in enumerate(targets[:-1]):
            assert tuple(int(got[name][i]) for name in agg.OUTPUTS) == HAND[(t[1], t[2])], t
        # chr3: a key without build rows
        assert tuple(int(got[name][-1]) for name in agg.OUTPUTS) == (0, 0, I64_MAX, I64_MIN, 0, 0)
