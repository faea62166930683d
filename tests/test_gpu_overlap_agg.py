"""-m gpu: ivx_probe_overlap_agg through the C ABI -- per probe row the count, sum, min, max of a build-side value column,
the overlapped bases and the bases-weighted sum -- on the direct path and on the region path.

Expected values come from tests/overlap_agg_oracle.py: the CPU oracle's pairs reduced with numpy in 64-bit wrapping
arithmetic (and, for the hand-made arithmetic edges, from its brute force in Python integers as well).  Every comparison is
exact and on whole output arrays.  The region-path cases reach each index form with the shapes
tests/test_gpu_region_forms.py uses (its builders are imported from there) and assert the form through ivx_index_layout."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pair_set
from oracle import oracle as orc
import overlap_agg_oracle as agg

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402
import test_gpu_region_forms as rf  # noqa: E402

pytestmark = pytest.mark.gpu

env, cols = rf.env, rf.cols
OUT = agg.OUTPUTS


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


def run(ctx, ix, p, val, mem="host", outputs=OUT):
    """one ivx_probe_overlap_agg call in either memory mode; -> {name: numpy column}"""
    if mem == "host":
        return ctx.overlap_agg(ix, *p, val, outputs=outputs)
    got = ctx.overlap_agg(ix, *[dev(c) for c in p], dev(val), outputs=outputs)
    ctx.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if k == "count" else v.cpu().numpy()) for k, v in got.items()}


def same(got, want, what=None):
    assert sorted(got) == sorted(want), what
    for name in got:
        assert got[name].dtype == want[name].dtype and len(got[name]) == len(want[name]), (name, what)
        bad = np.flatnonzero(got[name] != want[name])
        assert len(bad) == 0, (name, what, bad[:5], got[name][bad[:5]], want[name][bad[:5]])


def both_paths(ctx, ix, b, p, val, mems=("host",), want=None):
    """direct and region results equal each other and the restatement"""
    want = agg.aggregate(b, p, val) if want is None else want
    for mem in mems:
        with env(IVX_JOIN_PATH="direct"):
            d = run(ctx, ix, p, val, mem)
        with env(IVX_JOIN_PATH="regions"):
            r = run(ctx, ix, p, val, mem)
        same(d, want, (mem, "direct"))
        same(r, want, (mem, "regions"))
        same(r, d, (mem, "regions against direct"))
    return want


def values(n, seed, dtype=np.int32):
    """one distinct value per build row (a shifted row -> value lookup shows), signs mixed"""
    rng = np.random.default_rng(seed)
    v = rng.permutation(n).astype(np.int64) * 3 - n
    return v.astype(dtype)


# ---------------------------------------------------------------- direct path

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
def test_agg_direct(ctx, nb, nk):
    b = direct_build(nb, nk, nb + nk)
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=nk + 1)
    assert ix.rows == nb
    matched = 0
    with env(IVX_JOIN_PATH="direct"):
        for n in (0, 1, 63, 64, 65, 8192, 100_003):
            p = strict_probes(n, nk, n + 1)
            if nb == 1 and n:
                p[0][0], p[1][0], p[2][0] = b[0][0], b[1][0], b[1][0]                 # (the single build row is hit by every non-empty batch)
            for dt in (np.int32, np.int64):
                val = values(nb, 7 * nb + n, dt)
                want = agg.aggregate(b, p, val)
                for mem in ("host", "device"):
                    got = run(ctx, ix, p, val, mem)
                    same(got, want, (n, dt, mem))
            _, per_row = ctx.overlap_count(ix, *p, per_row=True)
            assert (per_row[:n] == want["count"]).all(), n
            matched += int((want["count"] != 0).sum())
            if n >= 8192:
                assert (want["count"] == 0).any()                                     # rows without a match are in every big batch
    assert matched > 0
    ix.free()


# ---------------------------------------------------------------- arithmetic edges

I32_MAX, I32_MIN = 2**31 - 1, -2**31
I64_MAX, I64_MIN = 2**63 - 1, -2**63


def edge_case(name):
    """-> (build, probe, val): a dozen rows each, one key"""
    if name == "sum_past_2p32":                  # three and more matches of value 2^31 - 1
        bs = np.arange(12) * 10
        b = cols(np.zeros(12), bs, bs + 100)
        ps = np.arange(12) * 10 + 5
        return b, cols(np.zeros(12), ps, ps + 30), np.full(12, I32_MAX, np.int32)
    if name == "int64_wrap":                     # values near +-2^62: sum and wsum wrap
        bs = np.arange(12) * 10
        b = cols(np.zeros(12), bs, bs + 100)
        ps = np.arange(12) * 10 + 5
        val = np.array([2**62, 2**62 + 5, 2**62 - 1, 2**62, 2**62 + 9, 2**62 - 3, -2**62, -2**62 - 7, -2**62, -2**62 + 1, -2**62 - 2, 3], np.int64)
        return b, cols(np.zeros(12), ps, ps + 60), val
    if name == "int32_min":                      # the signed minimum among positives, as int32
        bs = np.arange(12) * 10
        b = cols(np.zeros(12), bs, bs + 25)
        ps = np.arange(12) * 10
        val = np.array([5, I32_MIN, 7, I32_MAX, -1, 0, I32_MIN, I32_MIN, 9, 1, I32_MAX, I32_MIN + 1], np.int32)
        return b, cols(np.zeros(12), ps, ps + 3), val
    if name == "int64_min":
        bs = np.arange(12) * 10
        b = cols(np.zeros(12), bs, bs + 25)
        ps = np.arange(12) * 10
        val = np.array([5, I64_MIN, 7, I64_MAX, -1, 0, I64_MIN, I64_MIN, 9, 1, I64_MAX, I64_MIN + 1], np.int64)
        return b, cols(np.zeros(12), ps, ps + 3), val
    if name == "len_2p24":                       # value 2^31 - 1 with an overlap of 2^24 bases
        bs = np.arange(12) * 1000
        b = cols(np.zeros(12), bs, bs + 2**24 - 1 + 5000)
        ps = np.arange(12) * 1000 + 11_000
        return b, cols(np.zeros(12), ps, ps + 2**24 - 1), np.full(12, I32_MAX, np.int32)
    if name == "len_2p32":                       # one build and one probe row over the whole int32 range
        bs = np.array([I32_MIN] + list(range(0, 110, 10)))
        be = np.array([I32_MAX] + list(range(5, 115, 10)))
        ps = np.array([I32_MIN] + list(range(2, 112, 10)))
        pe = np.array([I32_MAX] + list(range(2, 112, 10)))
        return cols(np.zeros(12), bs, be), cols(np.zeros(12), ps, pe), np.array([I32_MAX] + list(range(-5, 6)), np.int32)
    assert name == "overlap_shapes"              # contained, containing, left-partial, right-partial, point, touching ends
    b = cols(np.zeros(12), [100, 100, 100, 100, 100, 100, 1000, 1000, 2000, 2000, 3000, 3000],
             [200, 200, 200, 200, 200, 200, 1000, 1000, 2100, 2100, 3050, 3050])
    p = cols(np.zeros(12), [120, 50, 50, 150, 100, 200, 1000, 999, 2100, 1990, 3051, 2999],
             [130, 300, 150, 300, 100, 200, 1000, 1001, 2200, 2000, 3060, 2999])
    return b, p, np.arange(1, 13, dtype=np.int32) * 1001


@pytest.mark.parametrize("name", ["sum_past_2p32", "int64_wrap", "int32_min", "int64_min", "len_2p24", "len_2p32", "overlap_shapes"])
def test_agg_arithmetic_edges(ctx, name):
    b, p, val = edge_case(name)
    want = agg.brute(b, p, val)                                            # Python integers, wrapped at the end
    same(agg.aggregate(b, p, val), want, "restatement")
    if name == "sum_past_2p32":
        assert (want["count"] >= 3).all() and (want["sum"] > 2**32).all()
    if name == "int64_wrap":
        exact = np.array([sum(int(val[j]) for j in range(12) if b[1][j] <= p[2][i] and b[2][j] >= p[1][i]) for i in range(12)], object)
        assert any(int(want["sum"][i]) != exact[i] for i in range(12))     # (some sum really left the int64 range)
    if name == "len_2p32":
        assert want["bases"][0] >= 2**32 and want["count"][0] == 12
    if name == "len_2p24":
        assert (want["bases"] >= 2**24).all() and want["wsum"].max() >= I32_MAX * 2**24
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    for path in ("direct", "regions"):
        for mem in ("host", "device"):
            with env(IVX_JOIN_PATH=path):
                same(run(ctx, ix, p, val, mem), want, (path, mem))
    ix.free()


# ---------------------------------------------------------------- output selection and arguments

def test_agg_output_selection(ctx):
    b = direct_build(5000, 3, 1)
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=4)
    p = strict_probes(20_000, 3, 2)
    val = values(5000, 3)
    want = agg.aggregate(b, p, val)
    for path in ("direct", "regions"):
        with env(IVX_JOIN_PATH=path):
            for mem in ("host", "device"):
                for name in OUT:
                    same(run(ctx, ix, p, val, mem, outputs=(name,)), {name: want[name]}, (path, mem, name))
                same(run(ctx, ix, p, val, mem, outputs=("min", "wsum")), {"min": want["min"], "wsum": want["wsum"]}, (path, mem))
                same(run(ctx, ix, p, val, mem), want, (path, mem))
    ix.free()


def test_agg_arguments_and_metrics(ctx):
    b = direct_build(5000, 3, 1)
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=4)
    p = strict_probes(1000, 3, 2)
    val = values(5000, 3)
    ctx.reset_metrics()
    run(ctx, ix, p, val)
    m = ctx.metrics()
    assert (m["input_batches"], m["input_rows"], m["output_batches"], m["output_rows"]) == (1, 1000, 1, 1000), m
    with pytest.raises(pyivx.IvxError) as ei:                               # all outputs null
        ctx.overlap_agg(ix, *p, val, outputs=())
    assert ei.value.status == pyivx.ERR_INVALID
    with pytest.raises(pyivx.IvxError) as ei:                               # a null value column over a non-empty index
        ctx.overlap_agg(ix, *p, None)
    assert ei.value.status == pyivx.ERR_INVALID
    out = np.empty(1000, np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for vb in (0, 2, 16):                                                   # val_bytes is 4 or 8
        st = pyivx.lib().ivx_probe_overlap_agg(ctx.h, ix.h, pyivx.MEM_HOST, ptr(p[0]), ptr(p[1]), ptr(p[2]), 1000, ptr(val), vb,
                                               None, ptr(out), None, None, None, None)
        assert st == pyivx.ERR_INVALID, vb
    cnt = ctx.build(pyivx.KIND_COUNT, *b, n_keys=4)
    with pytest.raises(pyivx.IvxError) as ei:
        ctx.overlap_agg(cnt, *p, val)
    assert ei.value.status == pyivx.ERR_UNSUPPORTED
    # an index without rows takes a null value column: every row gets the empty result
    e = ctx.build(pyivx.KIND_OVERLAP, *cols([], [], []), n_keys=4)
    same(ctx.overlap_agg(e, *p, None), agg.empty(1000))
    cnt.free(); ix.free(); e.free()


# ---------------------------------------------------------------- region path

def region_path_scratch(ix, p, val):
    """device scratch a fresh context takes for one device-mode call under IVX_JOIN_PATH=regions: the direct kernel needs
    none, the region path routes the rows into scratch pages"""
    c = pyivx.Ctx(0)
    try:
        with env(IVX_JOIN_PATH="regions"):
            c.overlap_agg(ix, *[dev(x) for x in p], dev(val))
        c.synchronize()
        return c.reserved_bytes()
    finally:
        c.close()


@pytest.mark.parametrize("side", ["slice_6144", "slice_6145"])
def test_agg_regions_slice_capacity(ctx, side):
    """region 0's slice holds exactly IVX_RP_ECAP entries: point probes on the cells of slice entries 0, 31, 32, 6112 and
    6143, every build row with its own value (a shifted value slot shows); one more build row and the index is no longer
    lean: the same call falls back to the direct kernel and is still right"""
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
    for dt in (np.int32, np.int64):
        val = values(len(b[1]), 41, dt)
        want = both_paths(ctx, ix, b, p, val, mems=("host", "device"))
        assert (want["count"] > 0).all() and len(np.unique(want["sum"])) > 1
        # every entry of the slice matched, and a random batch over the whole index
        both_paths(ctx, ix, b, cols(np.zeros(len(in_slice)), in_slice, in_slice), val)
    rng = np.random.default_rng(22)
    both_paths(ctx, ix, b, rf.edge_probes(geo, 4, rng, 60_000, -100, 3_300_000, maxlen=40), val)
    scratch = region_path_scratch(ix, p, val)
    assert (scratch > 0) == (side == "slice_6144"), scratch             # lean: routed; not lean: the direct kernel, no scratch
    ix.free()


def test_agg_regions_slow_index_falls_back(ctx):
    """one build row above level 0: slow = 1, no lean form, the direct kernel answers under IVX_JOIN_PATH=regions"""
    b = rf.level0_lean_build(True)
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    lay = ix.layout()
    assert lay["slow"] == 1 and lay["levrows"] & ~1 and lay["nreg"] > 0, lay
    rng = np.random.default_rng(23)
    p = rf.points(rng, 150_000, 0, int(b[1].max()), unknown=1 / 3)
    p = rf.cat(p, cols([0, 0], [1_000_100, 1_000_256], [1_000_100, 1_000_256]))     # on the level-1 row (its last coordinate alone)
    val = values(len(b[1]), 42)
    both_paths(ctx, ix, b, p, val)
    assert region_path_scratch(ix, p, val) == 0
    ix.free()


def test_agg_regions_rest_rows(ctx):
    """rows the packed form cannot carry: a span past the region's halo, qe < qs, a length at and past the packed maximum,
    rows that start before the key's first or behind its last build row -- k_lean_rest<AggOp> values them"""
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
    p = rf.cat(past, last, longs, empty, outside, rf.sparse_probes(b, n_rand, 25))
    assert len(p[1]) <= n_rand + 10_000
    for dt in (np.int32, np.int64):
        val = values(len(b[1]), 43, dt)
        both_paths(ctx, ix, b, p, val, mems=("host", "device"))
        # the rest rows alone (nothing for the lean walk to find)
        both_paths(ctx, ix, b, rf.cat(past, longs, empty), val)
    ix.free()


def test_agg_regions_many_regions_sorted_rows(ctx):
    """three keys, several lean regions each, 1.2 million probe rows in (key, start) order: more 8192-row chunks than
    workgroups, so a workgroup's share crosses regions and reloads the values with the slice"""
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
    val = values(len(b[1]), 44)
    want = both_paths(ctx, ix, b, p, val, mems=("host", "device"))
    assert 0 < (want["count"] == 0).sum() < len(p[1])
    ix.free()


def test_agg_regions_occupancy_bitmap(ctx):
    """an index built under IVX_FILTER=force: probe rows in empty blocks are dropped before routing and still get count 0
    and the min / max identities"""
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
        q = tuple(c[:n] for c in p)
        want = both_paths(ctx, ix, b, q, val, mems=("host", "device"))
        none = want["count"] == 0
        assert none.any() and not none.all()
        assert (want["min"][none] == agg.I64_MAX).all() and (want["max"][none] == agg.I64_MIN).all()
    ix.free()


@pytest.mark.parametrize("n", [5 * 8192 + 1, 5 * 8192 + 8191, 50_000])
def test_agg_regions_no_match_and_ragged_tiles(ctx, n):
    """a batch without any match gives every row the empty result; batch sizes with n mod 8192 in {1, 8191}"""
    b = rf.sparse_build()
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    assert ix.layout()["slow"] == 0
    rng = np.random.default_rng(26)
    i = rng.integers(0, len(b[1]) - 1, n)
    gaps = i * 512 + rng.integers(256, 512, n)
    val = values(len(b[1]), 46)
    none = both_paths(ctx, ix, b, cols(np.zeros(n), gaps, gaps), val, mems=("host", "device"))
    same(none, agg.empty(n))
    some = both_paths(ctx, ix, b, rf.sparse_probes(b, n, 27), val, mems=("host", "device"))
    assert (some["count"] != 0).any()
    ix.free()


SWITCH = [(("count", "sum"), (1 << 23) - 1, False), (("count", "sum"), 1 << 23, True), (("sum",), 1 << 23, True),
          (("count", "sum", "min", "max"), (1 << 24) - 1, False), (("count", "sum", "min", "max"), 1 << 24, True),
          (("count", "sum", "min", "max", "bases"), 1 << 24, False), (OUT, 1 << 24, False)]


@pytest.mark.parametrize("outputs,n,regions", SWITCH, ids=[f"{len(o)}_outputs_{n}_rows" for o, n, _ in SWITCH])
def test_agg_default_switch(ctx, outputs, n, regions):
    """without IVX_JOIN_PATH the call takes the region path from 2^23 rows (at most one 8-byte output), from 2^24 rows (up
    to three) or never (more): seen by the scratch a fresh context takes, the direct kernel needs none.  Either way the
    result equals the direct kernel's, and the restatement on the batch's first rows"""
    b = rf.sparse_build()
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    assert ix.layout()["slow"] == 0
    p = rf.sparse_probes(b, n, 71)
    val = values(len(b[1]), 72)
    dp, dv = [dev(c) for c in p], dev(val)
    assert "IVX_JOIN_PATH" not in os.environ
    c = pyivx.Ctx(0)
    try:
        got = c.overlap_agg(ix, *dp, dv, outputs=outputs)
        c.synchronize()
        assert (c.reserved_bytes() > 0) == regions, c.reserved_bytes()
        with env(IVX_JOIN_PATH="direct"):
            d = ctx.overlap_agg(ix, *dp, dv, outputs=outputs)
        ctx.synchronize()
        import torch
        for name in outputs:
            assert bool(torch.equal(got[name], d[name])), name
        head = 50_000
        want = agg.aggregate(b, tuple(x[:head] for x in p), val)
        for name in outputs:
            h = got[name][:head].cpu().numpy()
            assert ((h.view(np.uint32) if name == "count" else h) == want[name]).all(), name
    finally:
        c.close()
    ix.free()


# ---------------------------------------------------------------- state

def test_agg_on_poisoned_scratch(ctx):
    b = rf.sparse_build()
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    p = rf.sparse_probes(b, 100_000, 51)
    val = values(len(b[1]), 52, np.int64)
    want = both_paths(ctx, ix, b, p, val, mems=("host", "device"))
    for word in (0, 1):
        for path in ("direct", "regions"):
            for mem in ("host", "device"):
                ctx.synchronize()
                assert ctx.debug_poison(word, pyivx.POISON_SCRATCH | pyivx.POISON_SCALARS | pyivx.POISON_DROP_PLANS) != 0
                with env(IVX_JOIN_PATH=path):
                    same(run(ctx, ix, p, val, mem), want, (word, path, mem))
    ix.free()


def test_agg_between_count_and_fill(ctx):
    """a total-only count of the region path leaves its routed rows for the fill; an agg call in between drops them and
    the fill still returns the oracle's pairs"""
    b = rf.sparse_build()
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    p = rf.sparse_probes(b, 200_000, 33)
    val = values(len(b[1]), 53)
    wb, wp = orc.join(*b, *p, threads=4)
    want = agg.from_pairs(b, p, val, wb, wp)
    with env(IVX_JOIN_PATH="regions"):
        for mem in ("host", "device"):
            pp = p if mem == "host" else [dev(c) for c in p]
            total = ctx.overlap_count(ix, *pp)
            assert total == len(wb) and ctx.debug_state()["join_valid"] == 1
            vv = val if mem == "host" else dev(val)
            got = ctx.overlap_agg(ix, *pp, vv)
            assert ctx.debug_state()["join_valid"] == 0
            ob, op = ctx.overlap_fill(ix, *pp, cap=total)
            if mem == "device":
                ctx.synchronize()
                ob, op = ob.cpu().numpy().view(np.uint32), op.cpu().numpy().view(np.uint32)
                got = {k: (v.cpu().numpy().view(np.uint32) if k == "count" else v.cpu().numpy()) for k, v in got.items()}
            assert len(ob) == total and (pair_set(ob, op) == pair_set(wb, wp)).all(), mem
            same(got, want, mem)
    ix.free()


def test_agg_first_call_after_overlapped_build(ctx):
    """build overlap on, device columns: the agg call as the first call on the index waits for the build's tail"""
    b = rf.level0_lean_build(False)
    rng = np.random.default_rng(27)
    p = rf.points(rng, 150_000, 0, int(b[1].max()), unknown=1 / 3)
    val = values(len(b[1]), 54)
    want = agg.aggregate(b, p, val)
    dp, dv = [dev(c) for c in p], dev(val)
    ctx.set_build_overlap(True)
    try:
        for path in ("direct", "regions"):
            dcols = [dev(c) for c in b]
            ix = ctx.build(pyivx.KIND_OVERLAP, *dcols, n_keys=1)
            with env(IVX_JOIN_PATH=path):
                got = ctx.overlap_agg(ix, *dp, dv)
            ctx.synchronize()
            same({k: (v.cpu().numpy().view(np.uint32) if k == "count" else v.cpu().numpy()) for k, v in got.items()}, want, path)
            ix.free()
    finally:
        ctx.set_build_overlap(False)


def test_two_contexts_agg_one_index(ctx):
    b = rf.sparse_build()
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    p1, p2 = rf.sparse_probes(b, 60_000, 61), rf.sparse_probes(b, 70_001, 62)
    val = values(len(b[1]), 55)
    other = pyivx.Ctx(0)
    d1, d2, dv = [dev(c) for c in p1], [dev(c) for c in p2], dev(val)            # (alive until both contexts are done)
    try:
        for path in ("direct", "regions"):
            with env(IVX_JOIN_PATH=path):
                g1 = ctx.overlap_agg(ix, *d1, dv)
                g2 = other.overlap_agg(ix, *d2, dv)                              # both may be in flight
            ctx.synchronize(); other.synchronize()
            for g, p in ((g1, p1), (g2, p2)):
                same({k: (v.cpu().numpy().view(np.uint32) if k == "count" else v.cpu().numpy()) for k, v in g.items()}, agg.aggregate(b, p, val), path)
    finally:
        other.close()
    ix.free()
