"""Every designed input of tests/rank_forms.py is what it claims to be -- its gaps, run lengths, bit counts and key counts --
and the classes of queries the GPU tests rely on are all there, from the oracle alone; no GPU."""
import numpy as np
import pytest

import rank_forms as rf
from oracle import oracle as orc

LO, HI = rf.LO, rf.HI


# ------------------------------------------------------------------ the rules on hand-made columns

def test_grid_rule_by_hand():
    k = np.zeros(4, np.uint32)
    assert rf.grid_form(k, [0, 1, 2, 3], 1) == (0, 4)                       # 4 cells <= 2*4 + 1
    assert rf.grid_form(k, [0, 8, 8, 8], 1) == (0, 9)                       # 9 <= 9
    assert rf.grid_form(k, [0, 9, 9, 9], 1) == (1, 5)                       # 10 > 9; (9 >> 1) + 1 = 5
    assert rf.grid_form(k, [LO, HI, 0, 0], 1) == (29, 8)                    # 2^32 values: (2^32 - 1 >> 29) + 1 = 8 <= 9
    # two keys with rows of three: spans 100 and 0; budget 2*3 + 3 = 9: sh 4 gives 7 + 1 cells
    assert rf.grid_form(np.array([0, 0, 2], np.uint32), [50, 150, 7], 3) == (4, 8)
    assert rf.grid_form(np.empty(0, np.uint32), [], 3) == (0, 0)


def test_fit_rule_by_hand():
    k = np.zeros(2, np.uint32)
    assert rf.lin_fit(k, [0, 5], [3, 9], 1) == (4, 1, True)                 # run = 10 -> bitlen(9) = 4; n = 2 -> 1
    assert rf.lin_fit(k[:1], [7], [7], 1) == (1, 1, True)                   # run = 1, n = 1: one bit each
    assert rf.lin_fit(k, [LO, 0], [0, HI], 1) == (32, 1, True)
    assert rf.lin_fit(np.array([0, 1], np.uint32), [LO, LO], [HI, HI], 2) == (33, 1, True)


def test_route_rule_by_hand():
    k = np.arange(3, dtype=np.uint32)
    assert rf.route_regions(k, [0, 5, 9], 3) == 3
    assert rf.route_regions(np.zeros(2, np.uint32), [0, 1023], 1) == 1
    assert rf.route_regions(np.zeros(2, np.uint32), [0, 1024], 1) == 2
    assert rf.route_regions(np.zeros(2, np.uint32), [0, 1024 * 1023], 1) == 512      # 1024 cells: cs = 1
    assert rf.route_regions(np.zeros(2, np.uint32), [LO, HI], 1) == 512              # 2^22 cells: cs = 13
    assert rf.route_regions(np.arange(1023, dtype=np.uint32), np.zeros(1023, np.int32), 1023) == 1023
    assert rf.route_regions(np.arange(1024, dtype=np.uint32), np.zeros(1024, np.int32), 1024) == 0
    assert rf.route_regions(np.empty(0, np.uint32), [], 4) == 0


def test_merged_nodes_is_the_oracles_merge():
    rng = np.random.default_rng(3)
    s = rng.integers(0, 3000, 500).astype(np.int32); e = (s + rng.integers(0, 20, 500)).astype(np.int32)
    nk, nf, nl = rf.merged_nodes(np.zeros(500, np.uint32), s, e)
    wf, wl = orc.merge_intervals(s, e)
    assert np.array_equal(nf, wf) and np.array_equal(nl, wl) and not nk.any()
    assert [a.tolist() for a in rf.merged_nodes([1, 0, 1], [5, 5, 6], [5, 9, 6])] == [[0, 1, 1], [5, 5, 6], [9, 5, 6]]   # touching points stay apart


# ------------------------------------------------------------------ nearest sort forms

def _run_positions(t, key, start):
    o = rf.start_order(t["bk"], t["bs"], t["be"])
    return np.flatnonzero((t["bk"][o] == key) & (t["bs"][o] == start)), o


@pytest.mark.parametrize("n", [4095, 4096])
def test_cut_table(n):
    t = rf.cut_table(n)
    assert len(t["bk"]) == n and rf.LIN_MIN_ROWS == 4096
    assert not rf.is_presorted(t["bk"], t["bs"], t["be"]) and 2 <= rf.max_run(t["bk"], t["bs"]) <= 8      # short runs only
    assert rf.lin_fit(t["bk"], t["bs"], t["be"], 3)[2]
    assert rf.nearest_form(t) == ((2, rf.FULL, 0) if n == 4095 else (1, rf.REPAIR, 0))


@pytest.mark.parametrize("run_len", [64, 65])
def test_run_table(run_len):
    t = rf.run_table(run_len)
    bk, bs, be = t["bk"], t["bs"], t["be"]
    n = len(bk)
    assert n >= 4096 and not rf.is_presorted(bk, bs, be) and rf.lin_fit(bk, bs, be, 3)[2]
    w = (bk.astype(np.int64) << 32) | (bs.astype(np.int64) - LO)
    assert sorted(np.unique(w, return_counts=True)[1].tolist())[-4:] == [1, run_len, run_len, run_len] and run_len in (rf.MAXRUN, rf.MAXRUN + 1)
    first, mid, last = (_run_positions(t, k, s)[0] for k, s in t["runs"])
    assert first[0] == 0 and last[-1] == n - 1
    assert all(len(p) == run_len and p[-1] - p[0] == run_len - 1 for p in (first, mid, last))
    assert mid[0] // rf.BLOCK != mid[-1] // rf.BLOCK                        # straddles a multiple of 256
    for k, s in t["runs"]:
        rows = np.flatnonzero((bk == k) & (bs == s))
        ends = be[rows]
        assert (np.diff(ends) <= 0).all() and (np.diff(ends) == 0).sum() == run_len // 2      # descend with the row, in pairs
        # so the sorted order of the run is NOT the row order: the last pair of rows comes first, the first rows last
        pos, o = _run_positions(t, k, s)
        assert o[pos[0]] == rows[-2] and o[pos[1]] == rows[-1] and o[pos[-1]] == rows[0 if run_len % 2 else 1]
    assert rf.nearest_form(t) == ((1, rf.REPAIR, 0) if run_len == 64 else (2, rf.FULL, rf.FB_LIN_RUN | rf.FB_SE_RUN))
    assert rf.nearest_form(t, sort2=True) == ((2, rf.REPAIR, 0) if run_len == 64 else (2, rf.FULL, rf.FB_SE_RUN))
    qk, qs, qe = t["run_probes"]
    assert len(qk) == 300 and all(((qk == k) & (qs <= s) & (qe >= s)).sum() >= 30 for k, s in t["runs"])     # probes that overlap the whole run


@pytest.mark.parametrize("n", [131072, 131073])
def test_fit_table(n):
    t = rf.fit_table(n)
    bk, bs, be = t["bk"], t["bs"], t["be"]
    assert len(bk) == n and t["nkeys"] == 32768
    cnt, lo, hi = rf.key_stats(np.concatenate([bk, bk]), np.concatenate([bs, be]), 32768)
    assert min(cnt) >= 4 and set(lo) == {LO} and set(hi) == {HI}            # run = 32768 * 2^32 = 2^47
    assert rf.lin_fit(bk, bs, be, 32768) == ((47, 17, True) if n == 131072 else (47, 18, False))
    assert rf.max_run(bk, bs) <= rf.MAXRUN and not rf.is_presorted(bk, bs, be)
    assert rf.nearest_form(t) == ((1, rf.REPAIR, 0) if n == 131072 else (2, rf.REPAIR, rf.FB_NOFIT))
    assert rf.route_regions(bk, bs, 32768) == 0


@pytest.mark.parametrize("nkeys", [2048, 2049])
def test_many_keys_table(nkeys):
    assert rf.KEYS_IN_LDS == 2048
    t = rf.many_keys_table(nkeys)
    cnt = np.bincount(t["bk"], minlength=nkeys)
    empty = np.flatnonzero(cnt == 0).tolist()
    assert empty == rf.empty_keys(nkeys) and empty[0] == 0 and empty[-1] == nkeys - 1 and set(range(0, nkeys, 3)) <= set(empty)
    assert len(t["bk"]) >= 4096 and cnt[cnt > 0].min() >= 3 and cnt.max() <= 4
    assert rf.nearest_form(t) == (1, rf.REPAIR, 0)
    assert (t["probes"][0] >= nkeys).any()
    for kind in ("count", "coverage", "nearest"):
        assert rf.expected_grids(kind, t["bk"], t["bs"], t["be"], nkeys)["nroute_nreg"] == 0      # more than 1023 keys with rows


@pytest.mark.parametrize("n", [5000, 4000])
def test_presorted_table(n):
    t = rf.presorted_table(n)
    bk, bs, be = t["bk"], t["bs"], t["be"]
    assert len(bk) == n and rf.is_presorted(bk, bs, be)
    same = (bk[1:] == bk[:-1]) & (bs[1:] == bs[:-1])
    assert (same & (be[1:] == be[:-1])).sum() >= 50 and (same & (be[1:] != be[:-1])).sum() >= 20      # exact duplicates, and equal (key, start) alone
    assert rf.nearest_form(t) == (1 if n >= 4096 else 2, rf.PRESORTED, 0)
    assert rf.nearest_form(t, sort2=True) == (2, rf.PRESORTED, 0)
    u = rf.presorted_table(n, inversion=True)
    assert not rf.is_presorted(u["bk"], u["bs"], u["be"])
    differ = np.flatnonzero((u["bk"] != bk) | (u["bs"] != bs) | (u["be"] != be))
    assert len(differ) <= 2 and differ[-1] - differ[0] == 1                # one swap of neighbours
    assert rf.nearest_form(u)[1] != rf.PRESORTED and rf.nearest_form(u, sort2=True)[1] != rf.PRESORTED


# ------------------------------------------------------------------ rank grids

@pytest.mark.parametrize("distinct", [False, True])
def test_grid_column(distinct):
    v, cell = rf.grid_column(distinct)
    n = rf.GRID_N
    assert len(v) == n and (np.diff(v.astype(np.int64)) >= 0).all()
    assert v[0] == rf.GRID_ORIGIN and v[-1] == rf.GRID_ORIGIN + rf.GRID_SPAN
    assert rf.grid_form(np.zeros(n, np.uint32), v, 1) == (4, 2 * n + 1)
    assert np.array_equal(cell, (v.astype(np.int64) - rf.GRID_ORIGIN) >> 4) and cell[-1] == 2 * n
    gaps = np.diff(cell) - 1                                                # empty cells behind row i (-1: row i + 1 shares its cell)
    assert {0, 1, 62, 63, 64, 65, 127, 128} <= set(gaps.tolist())
    assert rf.BIG_GAP == 64 and rf.WAVE == 64 and rf.BLOCK == 256
    for g in (64, 65):
        at = np.flatnonzero(gaps == g)
        assert (at % 64 == 63).any() and (at % 64 == 0).any() and (at % 256 == 255).any() and (at >= n - 3).any(), (g, at)
    assert sorted(gaps[n - 3:].tolist()) == [64, 65]
    per_cell = np.bincount(cell)
    if distinct:
        assert len(np.unique(v)) == n                                       # all values differ: coverage keeps one node a value
        assert (per_cell == 16).sum() >= 19 and per_cell.max() == 16
    else:
        assert per_cell.max() == 300 and len(set(v[rf.GRID_EQUAL[0]:rf.GRID_EQUAL[1]].tolist())) == 1
    c16 = cell[rf.GRID_SIXTEEN[0]]
    assert sorted((v[cell == c16] - rf.GRID_ORIGIN - 16 * c16).tolist()) == list(range(16))
    # the column is the grid column of all three index kinds
    k = np.zeros(n, np.uint32)
    assert rf.expected_grids("count", k, v, v, 1)["grids"] == {"starts": (4, 2001), "ends": (4, 2001)}
    assert rf.expected_grids("nearest", k, v, v, 1)["grids"] == {"by_start": (4, 2001), "by_end": (4, 2001), "pmax": (4, 2001)}
    if distinct:
        assert rf.expected_grids("coverage", k, v, v, 1)["grids"] == {"first": (4, 2001), "last": (4, 2001)}
    assert rf.route_regions(k, v, 1) == 32                                  # 32016 coordinates: 32 cells of 2^10


def test_grid_probes():
    ps, pe = rf.grid_probes()
    lo, hi = rf.GRID_ORIGIN, rf.GRID_ORIGIN + rf.GRID_SPAN
    pts = ps[:rf.GRID_SPAN + 7]
    assert np.array_equal(pts, np.arange(lo - 3, hi + 4)) and np.array_equal(pts, pe[:len(pts)])
    rs, re = ps[len(pts):].astype(np.int64), pe[len(pts):].astype(np.int64)
    assert len(rs) == 4000 and (rs <= re).all() and rs.min() >= lo and re.max() <= hi
    assert set(((rs - lo) % 16).tolist()) == {0, 15} and set(((re - lo) % 16).tolist()) == {0, 15}
    first_last = ((rs - lo) % 16 == 0) & ((re - lo) % 16 == 15)
    assert first_last.sum() >= 800 and (first_last & ((rs - lo) // 16 == (re - lo) // 16)).sum() >= 100      # one whole cell


def test_extremes_table():
    t = rf.extremes_table()
    bk, bs, be = t["bk"], t["bs"], t["be"]
    cnt = np.bincount(bk, minlength=7)
    assert t["nkeys"] == 7 and cnt[[0, 2, 6]].tolist() == [0, 0, 0] and cnt[3] == 1 and cnt[4] == 1500
    assert len(set(bs[bk == 4].tolist())) == 1 and len(set(be[bk == 4].tolist())) == 1
    for col in (bs, be):
        assert col[bk == 1].min() == LO and col[bk == 1].max() == HI
    assert (be >= bs).all() and not rf.is_presorted(bk, bs, be)
    g = rf.expected_grids("count", bk, bs, be, 7)["grids"]
    assert g["starts"][0] >= 20 and g["ends"][0] >= 20                      # key 1's 2^32 values fit the budget only in wide cells
    pk, ps, pe = t["probes"]
    assert (pk >= 7).any() and ((ps == HI) & (pk == 1)).any() and ((pe == LO) & (pk == 1)).any()


@pytest.mark.parametrize("wide", [False, True])
def test_routing_table(wide):
    for nfull, some in ((1023, True), (1024, False)):
        t = rf.routing_table(nfull, wide)
        assert rf.MAXREG_WIDE == 1023 and len(np.unique(t["bk"])) == nfull and len(t["bk"]) >= 4096
        for kind in ("count", "coverage", "nearest"):
            nreg = rf.expected_grids(kind, t["bk"], t["bs"], t["be"], t["nkeys"])["nroute_nreg"]
            assert (nreg > 0) == some
            if some:
                assert nreg == 1023                                         # one region a key (wide: only with cs > 0, below)
    if wide:
        cnt, lo, hi = rf.key_stats(t["bk"], t["bs"], t["nkeys"])
        cells = [((h - l) >> 10) + 1 for c, l, h in zip(cnt, lo, hi) if c]
        assert sum(cells) > 2 * 1023 and len(set(cells)) > 3 and min(cells) > 2      # cs = 0 and cs = 1 leave too many regions


def test_tiny_tables():
    for n in (0, 1):
        t = rf.tiny_table(n)
        assert len(t["bk"]) == len(t["bs"]) == len(t["be"]) == n
        for kind in ("count", "coverage"):
            f = rf.expected_grids(kind, t["bk"], t["bs"], t["be"], 3)
            assert f["nroute_nreg"] == n and set(f["grids"].values()) == {(0, n)}


# ------------------------------------------------------------------ coverage probe

@pytest.mark.parametrize("strict", [False, True])
def test_coverage_queries_cover_every_class(strict):
    bk, first, last = rf.coverage_nodes()
    assert len(bk) == 400 and (first[1:].astype(np.int64) - last[:-1] >= 2).all()      # disjoint and not touching: nodes = rows
    assert sorted(set((last - first).tolist())) == [0, 1, 2, 37, 98]
    nk, nf, nl = rf.merged_nodes(bk, first, last)
    assert np.array_equal(nf, first) and np.array_equal(nl, last)
    pk, ps, pe = rf.coverage_queries()
    assert len(pk) == 1500
    cls = np.bincount(orc.count_overlaps(bk, first, last, pk, ps, pe, strict=strict).astype(np.int64), minlength=6)
    assert (cls[:6] >= 150).all(), cls.tolist()
    # among the queries over three nodes and more (the prefix-sum side) some have a zero-length node strictly inside
    zero_inside = [(ps[i] < f) & (pe[i] > f) for i in range(len(ps)) for f in first[last == first] if pe[i] - ps[i] > 250]
    assert sum(zero_inside) >= 100


def test_coverage_edge_queries():
    bk, first, last = rf.coverage_nodes()
    pk, ps, pe = rf.coverage_edge_queries()
    assert ((ps == LO) | (pe == HI)).all() and (ps == LO).sum() >= 4 and (pe == HI).sum() >= 4
    assert (orc.count_overlaps(bk, first, last, pk, ps, pe) >= 200).sum() >= 4        # over hundreds of nodes
    t = rf.wide_nodes()
    assert ((t["be"].astype(np.int64) - t["bs"]) > 2**31).sum() == 1 and ((t["be"].astype(np.int64) - t["bs"]) > 2**31 - 64).sum() == 2
    cov = orc.coverage(t["bk"], t["bs"], t["be"], *t["probes"]).tolist()
    assert cov[2] < 0                                                       # the sum wraps


# ------------------------------------------------------------------ strict wrap, launch edges, k

def test_strict_wrap_table():
    t = rf.strict_wrap_table()
    pk, ps, pe = t["probes"]
    for k in range(7):
        assert ((pk == k) & (ps == HI)).sum() >= 3 and ((pk == k) & (pe == LO)).sum() >= 2
    assert np.bincount(t["bk"], minlength=6).tolist() == [0, 5, 0, 2, 0, 1]


def test_wave_key_batches():
    b = rf.wave_key_batches()
    a = b["change_at_64"][0]
    assert len(a) == 192 and len(set(a[:64].tolist())) == 1 and len(set(a[64:].tolist())) == 1 and a[63] != a[64]
    o = b["one_lane"][0]
    assert [len(set(o[w * 64:(w + 1) * 64].tolist())) for w in range(3)] == [1, 2, 1] and (o[64:128] != o[64]).sum() == 1
    assert rf.BATCH_SIZES == (1, 7, 8, 9, 255, 256, 257, 1025)


def test_small_nearest_table():
    t = rf.small_nearest_table()
    bk, bs, be = t["bk"], t["bs"], t["be"]
    assert (bk == 0).sum() == 5 and ((bs[bk == 0] <= 20) & (be[bk == 0] >= 10)).all()      # every row of key 0 overlaps [10, 20]
    pk, ps, pe = t["probes"]
    assert (pk[0], ps[0], pe[0]) == (0, 10, 20)
    wb, wp, wd = orc.nearest(bk, bs, be, pk[:1], ps[:1], pe[:1], k=1, overlap=False)
    assert wb.tolist() == [orc.NULL_IDX] and wd.tolist() == [-1]
