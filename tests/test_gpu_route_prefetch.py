"""The one-pass partition's row loads one stage ahead (k_part_onepass: the second chunk of a tile is loaded while the first
is counted, and the first chunk of a workgroup's next tile while the current tile is counted, re-ordered and written out):
every case against the CPU oracle -- the pair multiset of overlap_fill (planned and unplanned), the total, the per-row
counts and exists.

What can go wrong is a tile fed from the wrong loads, or a load past the workgroup's rows, so the cases sit on the tile
arithmetic.  With TILE rows per tile and IVX_PART_TILES = t tiles per workgroup, a tile at t0 of a workgroup that ends at
hi takes its first rows from the loads issued one tile earlier iff that earlier tile saw t0 + TILE <= hi (and the columns
are 16-byte aligned); a workgroup's first tile, a partial tile and unaligned columns load at the top of the tile.  Row counts:
    2 t TILE            every tile whole, all but the workgroups' first ones loaded ahead
    2 t TILE - 1, + 1   the last tile partial / a tile of one row in a third workgroup
    t TILE + TILE - 3   a workgroup whose partial tile follows a whole one that must not load ahead (t = 1: its first tile)
    (t + 1) TILE        the last workgroup has exactly one tile
    5                   one partial tile
for each tile size in use: 8192 (packed rows, 16 per thread in two chunks of eight), 12288 (IVX_PACK=0) and 8192 with 1024
digits (more than 255 regions, 8 per thread).  One probe side per tile size, made once with its oracle answer; a case takes
a prefix of it (the pairs of a prefix are the pairs whose probe row lies in it)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pair_set
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402
import test_gpu_region_forms as rf  # noqa: E402

pytestmark = pytest.mark.gpu
env, cols, layout_of, probe_form = rf.env, rf.cols, rf.layout_of, rf.probe_form

BASE_ENV = {"IVX_JOIN_PATH": "regions", "IVX_DENSE": "0"}
TILES = {"packed": 8192, "pack0": 12288, "wide": 8192}
SIDE_ENV = {"packed": {}, "pack0": {"IVX_PACK": "0"}, "wide": {}}
T_MAX = 4
UNKNOWN_KEY = 7


def counts_of(t, tile):
    return [2 * t * tile, 2 * t * tile - 1, 2 * t * tile + 1, t * tile + tile - 3, (t + 1) * tile, 5]


def sparse_probes(rng, n, b, dropped=0.0):
    """rows of length 0..299 all over key 0's span and a little outside; `dropped`: that share of the rows is split between an
    unknown key, the key without build rows and rows that end before key 0's first start"""
    lo, hi = int(b[1].min()), int(b[1].max())
    ps = rng.integers(lo - 2000, hi + 2000, n)
    pe = ps + rng.integers(0, 300, n)
    pk = np.zeros(n, np.int64)
    if dropped:
        kind = rng.random(n)
        pk[kind < dropped / 3] = UNKNOWN_KEY
        pk[(kind >= dropped / 3) & (kind < 2 * dropped / 3)] = 1
        early = (kind >= 2 * dropped / 3) & (kind < dropped)
        ps[early] = lo - 5000 - rng.integers(0, 1000, early.sum()); pe[early] = ps[early] + rng.integers(0, 300, early.sum())
    return cols(pk, ps, pe)


class Side:
    """a build side, its index (and one with the occupancy bitmap forced), a probe side of the largest count and the oracle's
    answer for it"""

    def __init__(self, ctx, name):
        rng = np.random.default_rng(sum(map(ord, name)))
        self.name, self.tile = name, TILES[name]
        nmax = 2 * T_MAX * self.tile + 1
        if name == "wide":
            nk, per = 300, 30                                               # one region per key: 300 regions, 1024 digits
            k = np.repeat(np.arange(nk), per)
            s = k.astype(np.int64) * 10_000 + rng.integers(0, 200, len(k))
            self.b = cols(k, s, s + rng.integers(0, 16, len(k)))
            pk = rng.integers(0, nk, nmax)
            ps = pk.astype(np.int64) * 10_000 + rng.integers(-60, 300, nmax)
            self.p = cols(pk, ps, ps + rng.integers(0, 40, nmax))
            self.nk = nk
        else:
            self.b = rf.sparse_build()                                      # key 0 of two: key 1 has no build rows
            self.p = sparse_probes(rng, nmax, self.b)
            self.nk = 2
        self.ix, self.ixf = rf.build2(ctx, self.b, self.nk)
        self.lay, _ = layout_of(self.ix, *self.b, self.nk)
        self.want = orc.join(*self.b, *self.p, per_row=True, threads=4)
        f = probe_form(self.lay, nmax, len(self.want[0]), dict(BASE_ENV, **SIDE_ENV[name]))
        # the kernel instantiation the side is there for: digits, rows per thread (packed: 16, unpacked 12, 1024 digits: 8)
        assert f["onepass"] and f["routing"] == ("1024" if name == "wide" else "256") and f["klds"] == (name != "wide"), f
        assert f["packed"] == (name == "packed") or name == "wide", f

    def free(self):
        self.ix.free(); self.ixf.free()


def prefix(want, n):
    wb, wp, wcnt = want
    sel = wp < n
    return wb[sel], wp[sel], wcnt[:n]


def host(x):
    return x.cpu().numpy() if pyivx._is_torch(x) else np.asarray(x)


def check(ctx, ix, p, want, kv, tag):
    """count, planned and unplanned fill, per-row counts, exists of probe side p (numpy columns, device tensors, or a None
    key column) against want = (build rows, probe rows, per-row counts)"""
    wb, wp, wcnt = want
    wset = pair_set(wb, wp)
    with env(**BASE_ENV, **kv):
        total = ctx.overlap_count(ix, *p)
        ob, op = ctx.overlap_fill(ix, *p, cap=total)
        with env(IVX_NO_PLAN=1):
            ob2, op2 = ctx.overlap_fill(ix, *p, cap=total)
        t2, pr = ctx.overlap_count(ix, *p, per_row=True)
        ex = ctx.exists(ix, *p)
    ob, op, ob2, op2, pr, ex = (host(x) for x in (ob, op, ob2, op2, pr, ex))
    assert total == len(wb) and t2 == total, (tag, total, t2, len(wb))
    assert len(ob) == total and (pair_set(ob.view(np.uint32), op.view(np.uint32)) == wset).all(), tag
    assert len(ob2) == total and (pair_set(ob2.view(np.uint32), op2.view(np.uint32)) == wset).all(), tag
    assert (pr.view(np.uint32).astype(np.uint64) == wcnt).all(), tag
    assert (ex.astype(bool) == (wcnt > 0)).all(), tag


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    for s in _sides.values():
        s.free()
    _sides.clear()
    c.close()


_sides = {}


def side(ctx, name):
    if name not in _sides:
        _sides[name] = Side(ctx, name)
    return _sides[name]


# ---------------------------------------------------------------- every tile size, tiles per workgroup and row count

@pytest.mark.parametrize("which", [0, 1, 2, 3, 4, 5], ids=["2tT", "2tT-1", "2tT+1", "tT+T-3", "(t+1)T", "5"])
@pytest.mark.parametrize("t", [1, 2, 4])
@pytest.mark.parametrize("name", ["packed", "pack0", "wide"])
def test_tile_edges(ctx, name, t, which):
    sd = side(ctx, name)
    n = counts_of(t, sd.tile)[which]
    p = tuple(c[:n] for c in sd.p)
    check(ctx, sd.ix, p, prefix(sd.want, n), dict(SIDE_ENV[name], IVX_PART_TILES=t), (name, t, n))


# ---------------------------------------------------------------- variants at two tiles per workgroup

VARIANT_COUNTS = [1, 3]                                     # 2 t TILE - 1 and t TILE + TILE - 3


@pytest.mark.parametrize("which", VARIANT_COUNTS)
@pytest.mark.parametrize("name", ["packed", "pack0", "wide"])
def test_unaligned_columns(ctx, name, which):
    """the columns as device views that start one element into their buffers: no 16-byte loads, and nothing loaded across
    tiles; the second chunk of a tile is still loaded ahead, element by element and checked against the workgroup's end"""
    import torch
    sd = side(ctx, name)
    n = counts_of(2, sd.tile)[which]
    p = tuple(torch.from_numpy(np.concatenate([[0], c[:n]]).astype(c.dtype).view(np.int32)).cuda()[1:] for c in sd.p)
    assert all(x.data_ptr() % 16 == 4 and x.is_contiguous() for x in p)
    check(ctx, sd.ix, p, prefix(sd.want, n), dict(SIDE_ENV[name], IVX_PART_TILES=2), (name, n))


@pytest.mark.parametrize("which", VARIANT_COUNTS)
def test_aligned_device_columns(ctx, which):
    """the same through device tensors that are aligned (the call form of the benchmark)"""
    import torch
    sd = side(ctx, "packed")
    n = counts_of(2, sd.tile)[which]
    p = tuple(torch.from_numpy(c[:n].view(np.int32)).cuda() for c in sd.p)
    assert all(x.data_ptr() % 16 == 0 for x in p)
    check(ctx, sd.ix, p, prefix(sd.want, n), dict(IVX_PART_TILES=2), n)


@pytest.mark.parametrize("which", VARIANT_COUNTS)
@pytest.mark.parametrize("name", ["packed", "wide"])
def test_filter_forced(ctx, name, which):
    """the index that carries the occupancy bitmap (built with IVX_FILTER=force): the partition's filtering instantiations"""
    sd = side(ctx, name)
    n = counts_of(2, sd.tile)[which]
    layf = sd.ixf.layout(); layf["nkeys"] = sd.nk
    assert layf["fg"] != rf.NOFG and probe_form(layf, n, n, BASE_ENV)["filter"], layf
    p = tuple(c[:n] for c in sd.p)
    check(ctx, sd.ixf, p, prefix(sd.want, n), dict(IVX_PART_TILES=2), (name, n))


@pytest.mark.parametrize("which", VARIANT_COUNTS)
@pytest.mark.parametrize("name", ["packed", "pack0"])
def test_dropped_rows(ctx, name, which):
    """a third of the rows cannot match and is dropped before the ranking (an unknown key, the key without build rows, rows that
    end before the key's first start): every tile writes out fewer rows than it read"""
    sd = side(ctx, name)
    n = counts_of(2, sd.tile)[which]
    p = sparse_probes(np.random.default_rng(40 + which), n, sd.b, dropped=0.33)
    want = orc.join(*sd.b, *p, per_row=True, threads=4)
    gone = (p[0] != 0) | (p[2] < int(sd.b[1].min()))
    assert 0.25 * n < gone.sum() < 0.40 * n and (want[2][gone] == 0).all()
    check(ctx, sd.ix, p, want, dict(SIDE_ENV[name], IVX_PART_TILES=2), (name, n))


@pytest.mark.parametrize("which", VARIANT_COUNTS)
def test_sorted_rows(ctx, which):
    """coordinate-sorted rows: whole wavefronts fall into one region and take lds_count_up4's one-atomic path"""
    sd = side(ctx, "packed")
    n = counts_of(2, sd.tile)[which]
    o = np.argsort(sd.p[1][:n], kind="stable")
    p = tuple(c[:n][o] for c in sd.p)
    want = orc.join(*sd.b, *p, per_row=True, threads=4)
    check(ctx, sd.ix, p, want, dict(IVX_PART_TILES=2), n)


@pytest.mark.parametrize("which", VARIANT_COUNTS)
def test_no_key_column(ctx, which):
    """a single-contig job: the calls without a key column (a null key pointer: every row has key 0)"""
    sd = side(ctx, "packed")
    n = counts_of(2, sd.tile)[which]
    p = (None, sd.p[1][:n], sd.p[2][:n])
    assert (sd.p[0] == 0).all()
    check(ctx, sd.ix, p, prefix(sd.want, n), dict(IVX_PART_TILES=2), n)


@pytest.mark.parametrize("which", VARIANT_COUNTS)
def test_count_and_coverage(ctx, which):
    """count_overlaps and coverage through the region partition: the values come back by tile number (vtab[tile][region]),
    so a tile fed from another tile's loads shows as wrong rows"""
    sd = side(ctx, "packed")
    n = counts_of(2, sd.tile)[which]
    p = sparse_probes(np.random.default_rng(60 + which), n, sd.b, dropped=0.1)
    with env(IVX_PART_TILES=2):
        rf.check_rowvals(ctx, sd.b, p, None, knobs=("default",))
