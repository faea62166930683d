"""CPU-only: the two restatements of ivx_intersect in tests/intersect_oracle.py agree, intersect's pieces and the oracle's
subtract fragments tile every left row, and the hand-written tables of the contract (include/ivx.h) come out as written."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as orc

import intersect_oracle as io

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))


def cols(rows):
    """[(key, start, end), ...] -> (key u32, start i64, end i64)"""
    rows = list(rows)
    return (np.array([r[0] for r in rows], np.uint32), np.array([r[1] for r in rows], np.int64), np.array([r[2] for r in rows], np.int64))


def as_rows(out):
    return [tuple(int(x) for x in r) for r in zip(*out)]


def same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("strict", [False, True])
def test_restatements_agree_on_random_inputs(strict):
    rng = np.random.default_rng(20 + int(strict))
    pieces = 0
    for _ in range(400):
        left, right = io.random_sides(rng, int(rng.integers(0, 9)), int(rng.integers(0, 9)), int(rng.integers(2, 4)))
        a, b = io.walk(left, right, strict), io.from_oracle(left, right, strict)
        assert same(a, b), (left, right, as_rows(a), as_rows(b))
        pieces += len(a[0])
    assert pieces > 100                                                 # (not vacuous: the sides do overlap)


@pytest.mark.parametrize("strict", [False, True])
def test_pieces_and_subtract_fragments_tile_every_left_row(strict):
    rng = np.random.default_rng(40 + int(strict))
    rows = 0
    for _ in range(300):
        left, right = io.random_sides(rng, int(rng.integers(0, 9)), int(rng.integers(0, 9)), int(rng.integers(2, 4)))
        bad = io.check_tiling(left, io.walk(left, right, strict), orc.subtract(*left, *right, strict=strict))
        assert not bad, (strict, left, right, bad)
        rows += len(left[1])
    assert rows > 300


# (left rows, right rows, weak result, strict result); results as (key, start, end, left row)
TABLES = {
    # a right row touches the left row's START at one coordinate: a point piece when weak, nothing when strict
    "touch_at_start": ([(0, 10, 20)], [(0, 5, 10)], [(0, 10, 10, 0)], []),
    # ... and its END
    "touch_at_end": ([(0, 10, 20)], [(0, 20, 30)], [(0, 20, 20, 0)], []),
    # adjacent rights: one run when weak, two when strict
    "adjacent_rights": ([(0, 0, 10)], [(0, 1, 5), (0, 5, 9)], [(0, 1, 9, 0)], [(0, 1, 5, 0), (0, 5, 9, 0)]),
    "nested_right": ([(0, 0, 10)], [(0, 2, 8), (0, 4, 5)], [(0, 2, 8, 0)], [(0, 2, 8, 0)]),
    "left_covered_whole": ([(0, 4, 6)], [(0, 0, 10)], [(0, 4, 6, 0)], [(0, 4, 6, 0)]),
    "left_over_several_runs": ([(0, 0, 100)], [(0, 10, 20), (0, 30, 40), (0, 35, 50), (0, 90, 120)],
                               [(0, 10, 20, 0), (0, 30, 50, 0), (0, 90, 100, 0)], [(0, 10, 20, 0), (0, 30, 50, 0), (0, 90, 100, 0)]),
    "key_absent_on_the_right": ([(0, 0, 10), (1, 0, 10)], [(0, 5, 6)], [(0, 5, 6, 0)], [(0, 5, 6, 0)]),
    "key_absent_on_the_left": ([(1, 0, 10)], [(0, 5, 6), (1, 2, 3)], [(1, 2, 3, 0)], [(1, 2, 3, 0)]),
    # output order: left rows by (key, start, end, input row), whatever the input order
    "left_rows_in_sorted_order": ([(1, 5, 9), (0, 7, 8), (0, 1, 8), (0, 1, 8), (0, 1, 3)], [(0, 0, 20), (1, 0, 20)],
                                  [(0, 1, 3, 4), (0, 1, 8, 2), (0, 1, 8, 3), (0, 7, 8, 1), (1, 5, 9, 0)],
                                  [(0, 1, 3, 4), (0, 1, 8, 2), (0, 1, 8, 3), (0, 7, 8, 1), (1, 5, 9, 0)]),
    # start == end on both sides
    "points": ([(0, 5, 5)], [(0, 5, 5), (0, 7, 7)], [(0, 5, 5, 0)], []),
}


@pytest.mark.parametrize("name", sorted(TABLES))
@pytest.mark.parametrize("strict", [False, True])
def test_hand_written_tables(name, strict):
    left, right, weak, strong = TABLES[name]
    want = strong if strict else weak
    for fn in (io.walk, io.from_oracle):
        assert as_rows(fn(cols(left), cols(right), strict)) == want, fn.__name__


def test_symbol_and_methods_exist():
    import pyivx
    import sharded
    assert "ivx_intersect" in pyivx.SYMBOLS and hasattr(pyivx.lib(), "ivx_intersect") and hasattr(pyivx.lib(), "ivx_debug_intersect_paths")
    assert callable(pyivx.Ctx.intersect) and callable(pyivx.Ctx.intersect_paths)
    assert callable(sharded.ShardedRanges.intersect)
    g = pyivx.intersect_geometry()
    # the staged runs fit a workgroup's LDS budget next to seven other workgroups of a CU (160 KB): 20 bytes per run
    assert g["rows_per_wg"] == 256 and g["dbg_words"] == len(pyivx.ISECT_DBG_SLOTS)
    assert g["staged_runs"] * 20 <= 17 * 1024 and g["staged_runs"] > 256 + g["margin"]
