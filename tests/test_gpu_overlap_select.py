"""-m gpu: ivx_probe_overlap_select through the C ABI (include/ivx_select.h) -- per probe row the one best build row by a
criterion, and the criterion's value there -- on the direct path and on the region path, in host and device memory mode.

Expected values come from tests/overlap_select_oracle.py: the CPU oracle's pairs, ordered with a numpy lexsort (and, for the
hand-made edges, from its brute force in Python integers as well).  Every comparison is exact and on whole output arrays.
The region-path cases reach each index form with the shapes tests/test_gpu_region_forms.py uses (its builders are imported
from there) and assert the form through ivx_index_layout; where a case claims that the lean kernels ran, it asserts the
scratch the call reserved (the direct kernel takes none).

The default switch between the two paths is 2^23 rows, measured with tools/overlap_select_timing.py
(profiles/overlap_select_timing.txt); test_select_default_switch holds the library to it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pair_set
from oracle import oracle as orc
import overlap_select_oracle as sel

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402
import test_gpu_region_forms as rf  # noqa: E402
from entry_cases import INVALID, OK, OOM, SIZES, UNSUPPORTED, Delay, Env, LateMode, Mode, Refused, _same, cint, ivals, u32, u64  # noqa: E402
from test_gpu_entry_state import designed, inside  # noqa: E402

pytestmark = pytest.mark.gpu

env, cols = rf.env, rf.cols
BY = sel.BY
NULL = sel.NULL_IDX
PATHS = ("direct", "regions")
MEMS = ("host", "device")
I32_MAX, I32_MIN = 2**31 - 1, -2**31
I64_MAX, I64_MIN = 2**63 - 1, -2**63


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def run(ctx, ix, p, by, val=None, mem="host", score=True):
    """one ivx_probe_overlap_select call in either memory mode; -> (build_idx, score or None) as numpy columns"""
    if mem == "host":
        return ctx.overlap_select(ix, *p, by=by, val=val, score=score)
    bi, sc = ctx.overlap_select(ix, *[dev(c) for c in p], by=by, val=None if val is None else dev(val), score=score)
    ctx.synchronize()
    return bi.cpu().numpy().view(np.uint32), (None if sc is None else sc.cpu().numpy())


def same(got, want, what=None):
    for name, g, w in zip(("build_idx", "score"), got, want):
        if g is None:
            continue
        assert g.dtype == w.dtype and len(g) == len(w), (name, what)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (name, what, bad[:5], g[bad[:5]], w[bad[:5]])


class Want:
    """the oracle's pairs of (build, probe), made once; the winners under any criterion from them"""

    def __init__(self, b, p):
        self.b, self.p = b, p
        self.wb, self.wp = orc.join(*b, *p, threads=4)
        self.matched = np.zeros(len(p[1]), bool)
        self.matched[np.asarray(self.wp, np.int64)] = True

    def __call__(self, by, val=None):
        return sel.from_pairs(self.b, self.p, by, val, self.wb, self.wp)


def both_paths(ctx, ix, want, by, val=None, mems=MEMS, scores=(True,)):
    """direct and region results equal the restatement (hence each other); -> the restatement"""
    w = want(by, val)
    for mem in mems:
        for path in PATHS:
            for score in scores:
                with env(IVX_JOIN_PATH=path):
                    same(run(ctx, ix, want.p, by, val, mem, score), w, (by, mem, path, score))
    return w


def all_criteria(ctx, ix, want, val, mems=MEMS):
    """every criterion; the two by value with `val` as it is"""
    out = {}
    for by in BY:
        out[by] = both_paths(ctx, ix, want, by, val if by.endswith("_val") else None, mems)
    return out


def values(n, seed, dtype=np.int32):
    """one distinct value per build row (a shifted row -> value lookup shows), signs mixed"""
    rng = np.random.default_rng(seed)
    v = rng.permutation(n).astype(np.int64) * 3 - n
    return v.astype(dtype)


def region_path_scratch(ix, p, by="max_val", val=None):
    """device scratch a fresh context takes for one device-mode call under IVX_JOIN_PATH=regions: the direct kernel needs
    none, the region path routes the rows into scratch pages"""
    c = pyivx.Ctx(0)
    try:
        with env(IVX_JOIN_PATH="regions"):
            c.overlap_select(ix, *[dev(x) for x in p], by=by, val=None if val is None else dev(val))
        c.synchronize()
        return c.reserved_bytes()
    finally:
        c.close()


# ---------------------------------------------------------------- G1: direct path

def direct_build(nb, nk, seed):
    """nb build rows over keys 0..nk-1 of an index with nk + 1 keys: the last key has no build rows"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 200_000, nb)
    return cols(rng.integers(0, nk, nb), s, s + rng.integers(0, 400, nb))


def strict_probes(n, nk, seed):
    """probe rows as the SQL path hands them over for strict predicates (end - 1): some have qe < qs; keys 0..nk-1, the
    key without build rows (nk) and one the index does not have at all (nk + 5)"""
    rng = np.random.default_rng(seed)
    k = rng.choice(np.concatenate([np.arange(nk + 1), [nk + 5]]), n)
    s = rng.integers(-500, 201_000, n)
    return cols(k, s, s + rng.integers(-2, 120, n))


@pytest.mark.parametrize("nk", [1, 3])
@pytest.mark.parametrize("nb", [1, 33, 5000])
def test_select_direct(ctx, nb, nk):
    b = direct_build(nb, nk, nb + nk)
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=nk + 1)
    assert ix.rows == nb
    matched = 0
    for n in (0, 1, 63, 64, 65, 8192, 100_003, 300_001):                    # (the last: past the one-row-per-thread launch)
        p = strict_probes(n, nk, n + 1)
        if nb == 1 and n:
            p[0][0], p[1][0], p[2][0] = b[0][0], b[1][0], b[1][0]           # (the single build row is hit by every non-empty batch)
        want = Want(b, p)
        for by in BY:
            for dt in (np.int32, np.int64) if by.endswith("_val") else (None,):
                val = None if dt is None else np.random.default_rng(7 * nb + n).integers(-3, 4, nb).astype(dt)      # (ties)
                w = want(by, val)
                for mem in MEMS:
                    for path in PATHS if n in (65, 100_003) else PATHS[:1]:
                        with env(IVX_JOIN_PATH=path):
                            same(run(ctx, ix, p, by, val, mem), w, (n, by, dt, mem, path))
                with env(IVX_JOIN_PATH="direct"):
                    same(run(ctx, ix, p, by, val, "device", score=False), w, (n, by, dt, "no score"))
                # a probe key the build side lacks selects nothing
                assert (w[0][p[0] >= nk] == NULL).all() and (w[1][p[0] >= nk] == 0).all()
        _, per_row = ctx.overlap_count(ix, *p, per_row=True)
        assert ((per_row[:n] != 0) == want.matched).all(), n
        matched += int(want.matched.sum())
        if n >= 8192:
            assert not want.matched.all()                                   # rows without a match are in every big batch
    assert matched > 0
    ix.free()


# ---------------------------------------------------------------- G2: ties

def test_select_ties(ctx):
    """20 000 distinct intervals, 4 identical copies each, in shuffled row order, values from {-1, 0, 1}: every criterion meets
    ties on every matched row and returns the smallest tying row; FIRST_ROW / LAST_ROW the smallest / largest row of M(i)"""
    rng = np.random.default_rng(31)
    nd, copies = 20_000, 4
    ds = np.arange(nd, dtype=np.int64) * 256 + rng.integers(0, 100, nd)
    de = ds + rng.integers(0, 300, nd)
    pick = rng.permutation(np.repeat(np.arange(nd), copies))
    b = cols(np.zeros(len(pick)), ds[pick], de[pick])
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    lay = ix.layout()
    assert lay["slow"] == 0 and lay["pk24"] == 1 and lay["nreg"] > 1, lay   # lean with all 4 copies: nothing was shrunk
    n = 120_000
    x = rng.integers(-500, nd * 256 + 500, n)
    p = cols(np.zeros(n), x, x + rng.integers(0, 400, n))
    want = Want(b, p)
    val = rng.integers(-1, 2, len(pick)).astype(np.int32)
    got = all_criteria(ctx, ix, want, val)
    m = want.matched
    assert m.sum() > n // 2 and not m.all()
    wb, wp = np.asarray(want.wb, np.int64), np.asarray(want.wp, np.int64)
    lo, hi = np.full(n, 2**40), np.full(n, -1)
    np.minimum.at(lo, wp, wb); np.maximum.at(hi, wp, wb)
    assert (got["first_row"][0][m] == lo[m]).all() and (got["last_row"][0][m] == hi[m]).all()
    # the copies of an interval tie on the overlap length: the winner is the smallest row among the pairs with its score
    for by in ("max_overlap", "min_overlap", "max_val", "min_val"):
        c = sel.criterion(b, p, by, val, wb, wp)
        idx, score = got[by]
        tying = c == score[wp]
        least = np.full(n, 2**40)
        np.minimum.at(least, wp[tying], wb[tying])
        assert (idx[m] == least[m]).all(), by
        cnt = np.zeros(n, np.int64)
        np.add.at(cnt, wp[tying], 1)
        # ... and the ties are there: all copies of the winner by length; by value, of three values, on a good part of the rows
        assert (cnt[m] >= copies).all() if by.endswith("_overlap") else (cnt[m] > 1).mean() > 0.3, by
    assert region_path_scratch(ix, p, "max_val", val) > 0
    ix.free()


# ---------------------------------------------------------------- G3: sentinel edges

def edge_case(name):
    """-> (build, probe, by, val, the (build_idx, score) of probe row 0)"""
    one = cols([0], [100], [200])
    two = cols([0, 0], [100, 100], [200, 200])
    q = cols([0, 0], [150, 300], [160, 310])                                 # row 1 matches nothing
    if name == "all_int64_min_under_max":
        return two, q, "max_val", np.full(2, I64_MIN, np.int64), (0, I64_MIN)
    if name == "all_int64_max_under_min":
        return two, q, "min_val", np.full(2, I64_MAX, np.int64), (0, I64_MAX)
    if name == "one_int64_min_under_max":
        return one, q, "max_val", np.full(1, I64_MIN, np.int64), (0, I64_MIN)
    if name == "int32_min_as_4_bytes":
        return two, q, "max_val", np.full(2, I32_MIN, np.int32), (0, I32_MIN)
    if name == "int32_min_below_int32_max":
        return two, q, "min_val", np.array([I32_MAX, I32_MIN], np.int32), (1, I32_MIN)
    if name == "row_0_under_last_row":
        return one, q, "last_row", None, (0, 0)
    if name in ("len_2p32_max", "len_2p32_min"):                             # both intervals over the whole int32 range against a shorter one
        b = cols([0, 0], [0, I32_MIN], [10, I32_MAX])
        full = cols([0, 1], [I32_MIN, 300], [I32_MAX, 310])                  # (row 1: the key without build rows)
        return (b, full, "max_overlap", None, (1, 2**32)) if name == "len_2p32_max" else (b, full, "min_overlap", None, (0, 11))
    if name == "end_before_start_inside_a_build_row":                        # M(i) is the fill's: such a row is paired, its length is -9
        return two, cols([0, 0], [150, 300], [140, 310]), "max_overlap", None, (0, -9)
    assert name == "end_before_start"                                        # ... and one that no build row contains is not
    return two, cols([0, 0], [250, 300], [249, 100]), "first_row", None, (NULL, 0)


@pytest.mark.parametrize("name", ["all_int64_min_under_max", "all_int64_max_under_min", "one_int64_min_under_max", "int32_min_as_4_bytes",
                                  "int32_min_below_int32_max", "row_0_under_last_row", "len_2p32_max", "len_2p32_min", "end_before_start",
                                  "end_before_start_inside_a_build_row"])
def test_select_sentinel_edges(ctx, name):
    b, p, by, val, first = edge_case(name)
    want = sel.brute(b, p, by, val)                                         # Python integers
    same(sel.select(b, p, by, val), want, "restatement")
    assert (int(want[0][0]), int(want[1][0])) == first and (int(want[0][1]), int(want[1][1])) == (NULL, 0)
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=2)
    for path in PATHS:
        for mem in MEMS:
            for score in (True, False):
                with env(IVX_JOIN_PATH=path):
                    same(run(ctx, ix, p, by, val, mem, score), want, (path, mem, score))
    ix.free()


# ---------------------------------------------------------------- G4: slice capacity

@pytest.mark.parametrize("side", ["slice_6144", "slice_6145"])
def test_select_regions_slice_capacity(ctx, side):
    """region 0's slice holds exactly IVX_RP_ECAP entries: point probes on the cells of slice entries 0, 31, 32, 6112 and
    6143, every build row with its own value (a shifted row or value slot shows as a wrong index); one more build row and the
    index is no longer lean: the same call falls back to the direct kernel and is still right"""
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
    want = Want(b, p)
    every = Want(b, cols(np.zeros(len(in_slice)), in_slice, in_slice))   # every entry of the slice matched
    assert want.matched.all() and every.matched.all()
    for dt in (np.int32, np.int64):
        val = values(len(b[1]), 41, dt)
        got = all_criteria(ctx, ix, want, val)
        assert len(np.unique(got["max_val"][0])) > 1
        for by in ("min_val", "last_row", "max_overlap"):
            both_paths(ctx, ix, every, by, val if by == "min_val" else None, mems=("device",))
    rng = np.random.default_rng(22)
    rand = Want(b, rf.edge_probes(geo, 4, rng, 60_000, -100, 3_300_000, maxlen=40))
    all_criteria(ctx, ix, rand, val, mems=("host",))
    for by in ("max_val", "min_overlap"):
        scratch = region_path_scratch(ix, p, by, val if by == "max_val" else None)
        assert (scratch > 0) == (side == "slice_6144"), (by, scratch)   # lean: routed; not lean: the direct kernel, no scratch
    ix.free()


# ---------------------------------------------------------------- G5: rest rows

def test_select_regions_rest_rows(ctx):
    """rows the packed form cannot carry: a span past the region's halo, qe < qs, a length at and past the packed maximum,
    rows that start before the key's first or behind its last build row -- k_lean_rest<SelOp> answers them, alone and beside the
    lean walk"""
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
    empty = cols(np.zeros(1000), y, y - rng.integers(1, 50, 1000))                  # qe < qs
    hi = int(b[1].max())
    outside = cols(np.zeros(6), [-5000, -300, -1, hi + 1, hi + 255, hi + 256], [100, 0, 600, hi + 300, hi + 255, hi + 9000])
    mixed = rf.cat(past, last, longs, empty, outside, rf.sparse_probes(b, n_rand, 25))
    assert len(mixed[1]) <= n_rand + 10_000
    alone = rf.cat(past, longs, empty, outside)                                     # nothing for the lean walk to find
    for p in (alone, mixed):
        want = Want(b, p)
        assert want.matched.any() and not want.matched.all()
        for dt in (np.int32, np.int64):
            all_criteria(ctx, ix, want, values(len(b[1]), 43, dt))
        assert region_path_scratch(ix, p, "max_overlap") > 0
    ix.free()


# ---------------------------------------------------------------- G6: many regions

def test_select_regions_many_regions_sorted_rows(ctx):
    """three keys, several lean regions each, 1.2 million probe rows in (key, start) order: more 8192-row chunks than
    workgroups, so a workgroup's share crosses regions and reloads the row ids and the values with the slice"""
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
    pe = ps + np.where(rng.random(len(ps)) < 0.5, 0, rng.integers(0, 600, len(ps)))     # (some rows reach two build rows)
    order = np.lexsort((ps, pk))
    p = cols(pk[order], ps[order], pe[order])
    reg = rf.route_region(lay, b, p)
    per_reg = np.bincount(reg[reg >= 0], minlength=lay["nreg"])
    chunks = int(((per_reg + rf.FP_CHUNK - 1) // rf.FP_CHUNK).sum())
    assert chunks > 256 and (per_reg > 4 * rf.FP_CHUNK).sum() >= 2, (chunks, per_reg.max())
    want = Want(b, p)
    assert 0 < want.matched.sum() < len(p[1])
    val = values(len(b[1]), 44)
    for by in ("max_val", "min_overlap"):
        both_paths(ctx, ix, want, by, val if by == "max_val" else None)
    both_paths(ctx, ix, want, "min_val", val.astype(np.int64), mems=("device",))
    both_paths(ctx, ix, want, "last_row", mems=("device",), scores=(False,))
    ix.free()


# ---------------------------------------------------------------- G7: dropped rows and ragged tiles

def test_select_regions_occupancy_bitmap(ctx):
    """an index built under IVX_FILTER=force: probe rows in empty blocks are dropped before routing and still get
    (NULL_IDX, 0)"""
    rng = np.random.default_rng(7)
    nk = 3
    k = rng.integers(0, nk, 20_000)
    s = rng.integers(0, 50_000_000, len(k))
    b = cols(k, s, s + rng.integers(0, 300, len(k)))
    with env(IVX_FILTER="force"):
        ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=nk)
    lay, geo = rf.layout_of(ix, *b, nk)
    assert lay["fg"] != rf.NOFG and lay["slow"] == 0 and lay["pk24"] == 1, lay
    p = rf.edge_probes(geo, lay["sh0"], rng, 80_000, -100, 50_001_000)
    f = rf.probe_form(lay, len(p[1]), len(p[1]), {"IVX_JOIN_PATH": "regions"})
    assert f["filter"], f
    kept = rf.bitmap_pass(lay, b, p)
    assert 0 < int(np.count_nonzero(kept)) < len(p[1])                   # some rows are filtered out, some are routed
    val = values(len(b[1]), 45)
    for n in (len(p[1]), 3 * 8192 + 1, 3 * 8192 + 8191):                # and sizes with a ragged last 8192-row tile
        want = Want(b, tuple(c[:n] for c in p))
        got = all_criteria(ctx, ix, want, val)
        dropped = ~kept[:n]
        assert dropped.any() and want.matched.any()
        for idx, score in got.values():
            assert (idx[dropped] == NULL).all() and (score[dropped] == 0).all()
    ix.free()


@pytest.mark.parametrize("n", [5 * 8192 + 1, 5 * 8192 + 8191, 50_000])
def test_select_regions_no_match_and_ragged_tiles(ctx, n):
    """a batch without any match gives every row (NULL_IDX, 0); batch sizes with n mod 8192 in {1, 8191}"""
    b = rf.sparse_build()
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    assert ix.layout()["slow"] == 0
    rng = np.random.default_rng(26)
    i = rng.integers(0, len(b[1]) - 1, n)
    gaps = i * 512 + rng.integers(256, 512, n)
    val = values(len(b[1]), 46)
    none = Want(b, cols(np.zeros(n), gaps, gaps))
    assert not none.matched.any()
    for idx, score in all_criteria(ctx, ix, none, val).values():
        same((idx, score), sel.empty(n))
    some = Want(b, rf.sparse_probes(b, n, 27))
    assert some.matched.any()
    all_criteria(ctx, ix, some, val)
    ix.free()


# ---------------------------------------------------------------- G8: arguments and bookkeeping

def raw(ctx, ix, p, n, val, vb, by, bi, sc, mem=pyivx.MEM_HOST):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return pyivx.lib().ivx_probe_overlap_select(ctx.h, ix.h, mem, ptr(p[0]), ptr(p[1]), ptr(p[2]), n, ptr(val), vb, by, ptr(bi), ptr(sc))


def test_select_arguments_and_metrics(ctx):
    b = direct_build(5000, 3, 1)
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=4)
    n = 1000
    p = strict_probes(n, 3, 2)
    val = values(5000, 3)
    want = Want(b, p)
    ctx.reset_metrics()
    same(run(ctx, ix, p, "max_val", val), want("max_val", val))
    m = ctx.metrics()
    assert (m["input_batches"], m["input_rows"], m["output_batches"], m["output_rows"]) == (1, n, 1, n), m

    def fresh():
        return np.full(n, 0xA5A5A5A5, np.uint32), np.full(n, 0xA5A5A5A5A5A5A5A5, np.uint64).view(np.int64)

    def refused(status, text, index, v, vb, by, mem=pyivx.MEM_HOST):
        bi, sc = fresh()
        assert raw(ctx, index, p, n, v, vb, by, bi, sc, mem) == status, text
        assert text in pyivx.lib().ivx_last_error(ctx.h).decode(), pyivx.lib().ivx_last_error(ctx.h).decode()
        assert (bi == 0xA5A5A5A5).all() and (sc.view(np.uint64) == 0xA5A5A5A5A5A5A5A5).all(), text

    bi, sc = fresh()
    assert raw(ctx, ix, p, n, val, 4, 1, None, sc) == INVALID and "overlap_select: null build_idx" in pyivx.lib().ivx_last_error(ctx.h).decode()
    assert (sc.view(np.uint64) == 0xA5A5A5A5A5A5A5A5).all()
    for by in (-1, 6, 100):
        refused(INVALID, "overlap_select: unknown criterion", ix, val, 4, by)
    for by in (0, 1):
        for vb in (0, 2, 16):
            refused(INVALID, "overlap_select: val_bytes is 4 or 8", ix, val, vb, by)
        refused(INVALID, "overlap_select: null value column", ix, None, 4, by)
    refused(INVALID, "bad mem", ix, val, 4, 1, mem=7)
    cnt = ctx.build(pyivx.KIND_COUNT, *b, n_keys=4)
    refused(UNSUPPORTED, "index kind does not match", cnt, val, 4, 1)
    # the four criteria that read no value ignore val and val_bytes: null, or a width that would be refused
    for by in range(2, 6):
        for v, vb in ((None, 0), (val, 3), (None, 8)):
            bi, sc = fresh()
            assert raw(ctx, ix, p, n, v, vb, by, bi, sc) == OK, (by, vb)
            same((bi, sc), want(BY[by]), (by, vb))
    # n = 0: a no-op that leaves the buffers alone, and is still a metered batch without output
    bi, sc = fresh()
    ctx.reset_metrics()
    assert raw(ctx, ix, p, 0, val, 4, 1, bi, sc) == OK
    assert (bi == 0xA5A5A5A5).all() and (sc.view(np.uint64) == 0xA5A5A5A5A5A5A5A5).all()
    m = ctx.metrics()
    assert (m["input_batches"], m["input_rows"], m["output_batches"], m["output_rows"]) == (1, 0, 0, 0), m
    # an index without rows takes a null value column under a value criterion: every row gets the empty result
    e = ctx.build(pyivx.KIND_OVERLAP, *cols([], [], []), n_keys=4)
    same(ctx.overlap_select(e, *p, by="max_val", val=None), sel.empty(n))
    # the binding's own checks
    with pytest.raises(ValueError):
        ctx.overlap_select(ix, *p, by="median")
    with pytest.raises(ValueError):
        ctx.overlap_select(ix, *p, by="max_val", val=val.astype(np.float32))
    cnt.free(); ix.free(); e.free()


def test_select_between_count_and_fill(ctx):
    """a total-only count of the region path leaves its routed rows for the fill; a select call in between drops them and
    the fill still returns the oracle's pairs"""
    b = rf.sparse_build()
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    p = rf.sparse_probes(b, 200_000, 33)
    want = Want(b, p)
    with env(IVX_JOIN_PATH="regions"):
        for mem in MEMS:
            pp = p if mem == "host" else [dev(c) for c in p]
            total = ctx.overlap_count(ix, *pp)
            assert total == len(want.wb) and ctx.debug_state()["join_valid"] == 1
            bi, sc = ctx.overlap_select(ix, *pp, by="max_overlap")
            assert ctx.debug_state()["join_valid"] == 0
            ob, op = ctx.overlap_fill(ix, *pp, cap=total)
            if mem == "device":
                ctx.synchronize()
                ob, op = ob.cpu().numpy().view(np.uint32), op.cpu().numpy().view(np.uint32)
                bi, sc = bi.cpu().numpy().view(np.uint32), sc.cpu().numpy()
            assert len(ob) == total and (pair_set(ob, op) == pair_set(want.wb, want.wp)).all(), mem
            same((bi, sc), want("max_overlap"), mem)
    ix.free()


# ---------------------------------------------------------------- G9: the catalogue's walks, as a local case

def probe_overlap_select(E, M, n):
    """the catalogue's case (entry_cases.py): both outputs, three criteria -- an int64 value per build row, the overlap length,
    the last row -- on the catalogue's columns, through the entry itself"""
    from entry_cases import CASES, SEL_CASE_BY
    res = CASES["probe_overlap_select"](E, M, n)
    assert sorted(res) == sorted(f"{what}.{by}" for what in ("st", "idx", "score") for by in SEL_CASE_BY) and SEL_CASE_BY == ("max_val", "min_overlap", "last_row")
    return res


def spread_probes(n, seed):
    """n short rows all over the Env's one-key build (200 000 rows, some 50 regions)"""
    return inside(designed(), n, seed)


def case_run(E, M, n, path, rows=None):
    from entry_cases import shaped
    with env(IVX_JOIN_PATH=path):
        if rows is None:
            return probe_overlap_select(E, M, n)
        with shaped(cols=rows):
            return probe_overlap_select(E, M, n)


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    assert all(v == OK for k, v in want.items() if k.startswith("st.")), what
    diff = [k for k in want if not _same(got[k], want[k])]
    assert not diff, (what, {k: (got[k], want[k]) for k in diff[:2]})


@pytest.fixture(scope="module")
def E():
    e = Env(designed())
    lay = e.ix[0].layout()
    assert lay["nreg"] > 1 and lay["slow"] == 0 and lay["pk24"] == 1, lay      # the lean kernels can run
    yield e
    e.close()


@pytest.fixture(scope="module")
def host_results(E):
    """host mode on a context that is never poisoned, limited or late: (n, path) -> the case's results, held against the
    oracle once"""
    got = {}
    for n in SIZES:
        for path in PATHS:
            got[n, path] = case_run(E, Mode(False), n, path)
        assert_same(got[n, "regions"], got[n, "direct"], n)
    n = SIZES[0]
    p = ivals(n, 29, span=4000)
    val = np.random.default_rng(30).integers(-5, 6, E.n_build).astype(np.int64)
    want = Want(E.build_cols, p)
    assert want.matched.sum() > n // 10
    for by in ("max_val", "min_overlap", "last_row"):
        same((got[n, "direct"]["idx." + by], got[n, "direct"]["score." + by]), want(by, val), by)
    return got


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", SIZES)
def test_select_case_host_and_device_agree(E, host_results, n, path):
    assert_same(case_run(E, Mode(True), n, path), host_results[n, path], (n, path))


@pytest.mark.parametrize("word", [0, 1])
@pytest.mark.parametrize("devmode", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("path", PATHS)
def test_select_case_on_poisoned_state(E, host_results, path, devmode, word):
    what = pyivx.POISON_SCRATCH | pyivx.POISON_DROP_PLANS | pyivx.POISON_SCALARS | pyivx.POISON_PINNED        # everything but the pool
    for n in SIZES:
        E.ctx.synchronize()
        E.ctx.debug_poison(word, what)
        assert_same(case_run(E, Mode(devmode), n, path), host_results[n, path], (n, path, devmode, word))


@pytest.fixture(scope="module")
def late_world():
    import torch
    S = torch.cuda.Stream()
    L, H = Env(designed(), stream=S), Env(designed())
    yield S, L, H, Delay(S)
    L.close(); H.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", SIZES + [100_000])
def test_select_case_late_inputs(late_world, n, path):
    """every column still in flight on the context's stream when the entry is invoked (entry_cases.LateMode); the big size
    with rows all over the build, so that the region path routes something"""
    S, L, H, delay = late_world
    rows = spread_probes if n > 1000 else None
    want = case_run(H, Mode(False), n, path, rows)
    with LateMode(L, S, delay) as M:
        got = case_run(L, M, n, path, rows)
    assert M.calls, "no entry was called"
    assert_same(got, want, (n, path))
    if n > 1000:
        assert np.count_nonzero(want["idx.max_val"] != NULL) > n // 2


@pytest.mark.parametrize("devmode", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("path", PATHS)
def test_select_case_refused_reservations(path, devmode):
    """the memory limit stepped up from what the context holds at rest, one refused reservation at a time: IVX_ERR_OOM leaves
    the outputs untouched (host mode) and nothing reserved behind it, and the next call without the limit is right"""
    from test_gpu_entry_refusals import check_refused_call, parse
    E = Env(designed())
    try:
        ctx, n = E.ctx, SIZES[0]
        E.log = []
        want = case_run(E, Mode(devmode), n, path)
        want_log, E.log = E.log, []
        ctx.trim(0)
        L0 = ctx.reserved_bytes()
        limit, points = L0, 0
        for attempt in range(65):
            assert attempt < 64, (path, devmode, limit)
            ctx.trim(0)
            assert ctx.reserved_bytes() == L0
            ctx.set_memory_limit(limit)
            E.log, E.stop_on_oom = [], True
            got = refused = None
            try:
                got = case_run(E, Mode(devmode), n, path)
            except Refused:
                refused = E.log[-1]
            finally:
                E.stop_on_oom = False
            log, E.log = E.log, []
            assert E.L.ivx_ctx_synchronize(E.h) == OK
            if refused is None:
                assert_same(got, want, (path, devmode, "at the tightest limit", limit))
                break
            points += 1
            assert refused.st == OOM
            bts, r, lim = parse(refused.text)
            assert lim == limit and r + bts > limit, refused.text
            check_refused_call(E, refused, want_log[len(log) - 1], devmode, (path, devmode, refused.text))
            ctx.set_memory_limit(0)
            assert_same(case_run(E, Mode(devmode), n, path), want, (path, devmode, "after", refused.text))
            E.log = []
            ctx.trim(0)
            assert ctx.reserved_bytes() == L0, ("leaked after", refused.text)
            limit = r + bts
        ctx.set_memory_limit(0)
        # host mode stages its columns, the region path routes its rows: both reserve; the direct kernel on device columns does not
        assert (points > 0) == (not devmode or path == "regions"), (path, devmode, points)
    finally:
        E.ctx.set_memory_limit(0)
        E.close()


# ---------------------------------------------------------------- G10: default switch

@pytest.mark.parametrize("by", ["max_val", "min_overlap"])
def test_select_default_switch(ctx, by):
    """without IVX_JOIN_PATH the call takes the region path from 2^23 rows, the measured threshold
    (profiles/overlap_select_timing.txt: from there the region path's slowest repeat beat the direct kernel's fastest in every
    variant timed): one row below it the call reserves no scratch (the direct kernel), at it the call does.  Either way the
    result equals the other path's, and the restatement on the batch's first rows"""
    b = rf.sparse_build()
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    assert ix.layout()["slow"] == 0
    n = 1 << 23
    p = rf.sparse_probes(b, n, 71)
    val = values(len(b[1]), 72) if by == "max_val" else None
    assert "IVX_JOIN_PATH" not in os.environ
    import torch
    dp, dv = [dev(c) for c in p], None if val is None else dev(val)
    head = 50_000
    want = sel.select(b, tuple(x[:head] for x in p), by, val)
    for m, regions in ((n - 1, False), (n, True)):
        q = [c[:m] for c in dp]
        c = pyivx.Ctx(0)
        try:
            got = c.overlap_select(ix, *q, by=by, val=dv)
            c.synchronize()
            assert (c.reserved_bytes() > 0) == regions, (m, c.reserved_bytes())
            with env(IVX_JOIN_PATH="direct" if regions else "regions"):
                other = ctx.overlap_select(ix, *q, by=by, val=dv)
            ctx.synchronize()
            assert bool(torch.equal(got[0], other[0])) and bool(torch.equal(got[1], other[1])), m
            same((got[0][:head].cpu().numpy().view(np.uint32), got[1][:head].cpu().numpy()), want, m)
        finally:
            c.close()
    ix.free()
