"""-m gpu: the one-pass partition's 16384-row tiles (k_part_onepass<..., T = 1024>, one 1024-thread workgroup per CU) for the
join's packed, unfiltered form -- fill, count and marks -- against the 8192-row form and the CPU oracle.

IVX_PART_BIG=1 takes the 16384-row tiles whatever n is and IVX_PART_BIG=0 never, where the form's conditions hold (packed
rows, no bitmap in use, 16-byte aligned columns, at most KT_MAX keys, one 256-digit pass, no un-permute table); every case
runs under both and compares, bit-exactly, the pair multiset of overlap_fill (planned by a count call, and unplanned), the
total of overlap_count and the build-side marks with the oracle's.  Which form ran is not read back (the library has no
read-back for it): where the conditions are unmet the two settings must simply agree with the oracle as well.

Shapes come from the tile's geometry.  TILE = 16384 rows, 16 per thread as quads: row ((k / 4) * 1024 + tid) * 4 + k % 4;
the rank of a row inside its region and tile has 14 bits; pages hold 2^14 rows for batches this small (lgpg = 14), so a
region's run may cross one page border inside a tile; IVX_PART_TILES = t tiles per workgroup, the first chunk of a
workgroup's next whole tile loaded ahead."""
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

TILE = 16384
PAGE = 1 << 14
BASE_ENV = {"IVX_JOIN_PATH": "regions", "IVX_DENSE": "0"}
UNKNOWN_KEY = 7
ROW_COUNTS = [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1, 3 * TILE + 5]


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    for s in _sides.values():
        s.free()
    _sides.clear()
    c.close()


def host(x):
    return x.cpu().numpy() if pyivx._is_torch(x) else np.asarray(x)


def mark_bits(rows, n_build):
    w = np.zeros((n_build + 31) // 32, np.uint32)
    r = np.unique(np.asarray(rows).astype(np.int64))
    np.bitwise_or.at(w, r >> 5, (np.uint32(1) << (r & 31).astype(np.uint32)))
    return w


def check(ctx, ix, n_build, p, want, kv, tag, device_marks=False):
    """count, planned and unplanned fill and the marks of probe side p, with the 16384-row tiles forced and with the
    8192-row tiles forced, against want = (build rows, probe rows[, ...]) of the oracle"""
    wb, wp = want[0], want[1]
    wset = pair_set(wb, wp)
    wmarks = mark_bits(wb, n_build)
    for big in ("1", "0"):
        with env(**BASE_ENV, **kv, IVX_PART_BIG=big):
            total = ctx.overlap_count(ix, *p)
            ob, op = ctx.overlap_fill(ix, *p, cap=total)
            with env(IVX_NO_PLAN=1):
                ob2, op2 = ctx.overlap_fill(ix, *p, cap=total)
            marks = ctx.mark_build(ix, *p, pyivx.Ctx.new_marks(n_build, device="cuda" if device_marks else None))
        ob, op, ob2, op2, marks = (host(x) for x in (ob, op, ob2, op2, marks))
        assert total == len(wb), (tag, big, total, len(wb))
        assert len(ob) == total and (pair_set(ob.view(np.uint32), op.view(np.uint32)) == wset).all(), (tag, big)
        assert len(ob2) == total and (pair_set(ob2.view(np.uint32), op2.view(np.uint32)) == wset).all(), (tag, big)
        assert (marks.view(np.uint32) == wmarks).all(), (tag, big)


def big_form_open(lay, n, cap):
    """the host rule's other conditions, restated: a packed, unfiltered, lean fill over one 256-digit pass with LDS key tables"""
    f = probe_form(lay, n, cap, BASE_ENV)
    return f["path"] == "regions" and f["onepass"] and f["packed"] and not f["filter"] and f["routing"] == "256" and f["klds"] and f["lean"]


# ---------------------------------------------------------------- build sides, made once

def keyed_build(rng, keys, per=30, spread=200):
    """`per` short rows inside `spread` coordinates of each key in `keys` (spread = 1: every row of a key at its first
    coordinate, a span of one cell and so ONE region per key however few keys there are)"""
    k = np.repeat(np.asarray(keys), per)
    s = k.astype(np.int64) * 10_000 + rng.integers(0, spread, len(k))
    return cols(k, s, s + rng.integers(0, 16, len(k)))


def keyed_probes(rng, keys, n):
    pk = rng.choice(np.asarray(keys), n)
    ps = pk.astype(np.int64) * 10_000 + rng.integers(-60, 300, n)
    return cols(pk, ps, ps + rng.integers(0, 40, n))


class Side:
    def __init__(self, ctx, name):
        rng = np.random.default_rng(sum(map(ord, name)))
        self.name = name
        nmax = ROW_COUNTS[-1]
        if name == "sparse":                                    # one key (of two), ~196 regions of 2^19 coordinates
            self.b, self.nk = rf.sparse_build(), 2
            lo, hi = int(self.b[1].min()), int(self.b[1].max())
            ps = rng.integers(lo - 2000, hi + 2000, nmax)
            self.p = cols(np.zeros(nmax), ps, ps + rng.integers(0, 300, nmax))
            nreg = None
        else:
            # r<N>: N keys with rows, one region each; gaps: every other key id has no build rows; keys300: 100 keys with
            # rows among 300 (more than KT_MAX keys, still one 256-digit pass)
            keys, self.nk = {"r1": ([0], 1), "r2": ([0, 1], 2), "r255": (range(255), 255), "r256": (range(256), 256),
                             "gaps": (range(0, 240, 2), 240), "keys300": (range(0, 300, 3)[:100], 300)}[name]
            keys = list(keys)
            self.b = keyed_build(rng, keys, spread=1 if len(keys) <= 2 else 200)
            self.p = keyed_probes(rng, range(self.nk), nmax)    # (rows on the keys without build rows are dropped by the pass)
            nreg = len(keys) if name[0] == "r" else None
        self.ix = ctx.build(pyivx.KIND_OVERLAP, *self.b, n_keys=self.nk)
        self.lay, self.geo = layout_of(self.ix, *self.b, self.nk)
        assert nreg is None or self.lay["nreg"] == nreg, self.lay
        assert self.lay["pk24"] == 1 and self.lay["fg"] == rf.NOFG and self.lay["slow"] == 0, self.lay
        self.n_build = len(self.b[1])
        self.want = orc.join(*self.b, *self.p, per_row=True, threads=4)
        self.open = big_form_open(self.lay, nmax, len(self.want[0]))

    def free(self):
        self.ix.free()


_sides = {}


def side(ctx, name):
    if name not in _sides:
        _sides[name] = Side(ctx, name)
    return _sides[name]


def prefix(want, n):
    wb, wp, wcnt = want
    sel = wp < n
    return wb[sel], wp[sel], wcnt[:n]


# ---------------------------------------------------------------- row counts x tiles per workgroup

@pytest.mark.parametrize("n", ROW_COUNTS, ids=["T-1", "T", "T+1", "2T-1", "2T+1", "3T+5"])
@pytest.mark.parametrize("t", [1, 2, 4])
def test_row_counts(ctx, t, n):
    """a partial last tile, a tile loaded ahead next to one that is not, a workgroup's last tile whole and partial, over
    ~196 regions (runs of ~84 rows)"""
    sd = side(ctx, "sparse")
    assert sd.open and 190 <= sd.lay["nreg"] <= 200, sd.lay
    p = tuple(c[:n] for c in sd.p)
    check(ctx, sd.ix, sd.n_build, p, prefix(sd.want, n), dict(IVX_PART_TILES=t), (t, n))


@pytest.mark.parametrize("name", ["r1", "r2", "r255", "r256", "gaps"])
def test_region_counts(ctx, name):
    """1, 2, 255 regions (the most one 256-digit pass routes), 256 regions (a 1024-digit pass: the 8192-row form whatever the
    setting), and keys without build rows between keys that have some"""
    sd = side(ctx, name)
    assert sd.open == (name != "r256") and sd.lay["nreg"] <= (256 if name == "r256" else 255), (name, sd.lay)
    n = 2 * TILE + 1
    p = tuple(c[:n] for c in sd.p)
    check(ctx, sd.ix, sd.n_build, p, prefix(sd.want, n), dict(IVX_PART_TILES=2), name)


# ---------------------------------------------------------------- the 14-bit rank

@pytest.mark.parametrize("n", [TILE, TILE + 5])
def test_one_region_takes_a_whole_tile(ctx, n):
    """every row of a tile in ONE region: whole wavefronts on one counter (lds_count_up4's one-atomic path), local ranks
    0 .. 16383 -- the largest the 14 bits beside the digit hold"""
    sd = side(ctx, "r1")
    rng = np.random.default_rng(3)
    ps = rng.integers(0, 300, n)                                # (from the key's first coordinate on: every row is routed)
    p = cols(np.zeros(n), ps, ps + rng.integers(0, 40, n))
    want = orc.join(*sd.b, *p, per_row=True, threads=4)
    assert (rf.route_region(sd.lay, sd.b, p) == 0).all()
    check(ctx, sd.ix, sd.n_build, p, want, {}, n)


def test_two_regions_alternating(ctx):
    """rows alternate between two regions: per-row LDS atomics, ranks 0 .. 8191 in each"""
    sd = side(ctx, "r2")
    rng = np.random.default_rng(4)
    n = TILE
    pk = np.arange(n) % 2
    ps = pk.astype(np.int64) * 10_000 + rng.integers(0, 300, n)
    p = cols(pk, ps, ps + rng.integers(0, 40, n))
    want = orc.join(*sd.b, *p, per_row=True, threads=4)
    reg = rf.route_region(sd.lay, sd.b, p)
    assert (reg == pk).all()
    check(ctx, sd.ix, sd.n_build, p, want, {}, "alt")


# ---------------------------------------------------------------- a page border inside one tile's run

@pytest.mark.parametrize("first", [PAGE - 1, 1, PAGE], ids=["border_at_1", "border_at_16383", "border_at_16384"])
def test_page_border_inside_a_run(ctx, first):
    """One region, one workgroup walking four tiles (its reservations come in tile order): the first tile routes `first`
    rows (the rest sit on an unknown key), the second all 16384, so the second tile's run starts at virtual row `first`
    and the page border (2^14 rows) lies at offset 16384 - first of it: 1 (the run's second row opens the page: own1, and
    the write-out's second-page look-up for all rows but one), 16383 (the last row opens it), and 16384 (the run fills its
    page; the third tile's first row opens the next: own0)."""
    sd = side(ctx, "r1")
    rng = np.random.default_rng(first)
    n = 3 * TILE + 5
    pk = np.zeros(n, np.int64)
    drop = rng.choice(TILE, TILE - first, replace=False)
    pk[drop] = UNKNOWN_KEY
    ps = rng.integers(0, 300, n)
    p = cols(pk, ps, ps + rng.integers(0, 40, n))
    reg = rf.route_region(sd.lay, sd.b, p)
    assert int((reg[:TILE] == 0).sum()) == first and (reg[TILE:] == 0).all()
    assert probe_form(sd.lay, n, n, BASE_ENV)["lgpg"] == 14
    want = orc.join(*sd.b, *p, per_row=True, threads=4)
    check(ctx, sd.ix, sd.n_build, p, want, dict(IVX_PART_TILES=4), first)


# ---------------------------------------------------------------- rows the packed form cannot carry

def test_escapes(ctx):
    """end < start, a length at and past pk_maxlen, a start before the key's first coordinate and one more than 2^24 past its
    region's: each goes to the rest list under its own row id, in every quarter of a tile (slots above 8192 k among them)"""
    sd = side(ctx, "sparse")
    n = 2 * TILE + 1
    f = probe_form(sd.lay, n, n, BASE_ENV)
    assert f["maxlen"] == 65535, f
    lo, hi = int(sd.b[1].min()), int(sd.b[1].max())
    pk, ps, pe = (c[:n].astype(np.int64) for c in sd.p)
    at = np.concatenate([np.arange(j, n, 1021) for j in range(6)])        # (1021: prime, so the slots drift through the tile)
    kind = np.arange(len(at)) % 6
    s0 = ps[at]
    ps[at] = np.select([kind == 4, kind == 5], [lo - 5 - (at % 100), hi + (1 << 24) + 1000 + at], s0)
    pe[at] = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                       [s0 - 1 - (at % 300), s0 + 65534, s0 + 65535, s0 + 65536, lo + 100, ps[at] + 10])
    assert (at >= TILE + 8192).any() and ((at % TILE) >= 8192).sum() > 10
    p = cols(pk, ps, pe)
    want = orc.join(*sd.b, *p, per_row=True, threads=4)
    check(ctx, sd.ix, sd.n_build, p, want, dict(IVX_PART_TILES=2), "escapes")


# ---------------------------------------------------------------- conditions unmet: the 8192-row form, whatever the setting

def test_unaligned_columns(ctx):
    """columns that start 4 bytes into their buffers: no 16-byte loads, so no 16384-row tiles"""
    import torch
    sd = side(ctx, "sparse")
    n = 2 * TILE + 1
    p = tuple(torch.from_numpy(np.concatenate([[0], c[:n]]).astype(c.dtype).view(np.int32)).cuda()[1:] for c in sd.p)
    assert all(x.data_ptr() % 16 == 4 and x.is_contiguous() for x in p)
    check(ctx, sd.ix, sd.n_build, p, prefix(sd.want, n), dict(IVX_PART_TILES=2), "unaligned", device_marks=True)


def test_aligned_device_columns(ctx):
    """aligned device tensors, the benchmark's call form: the 16384-row tiles straight on the caller's columns"""
    import torch
    sd = side(ctx, "sparse")
    n = 3 * TILE + 5
    p = tuple(torch.from_numpy(c[:n].view(np.int32)).cuda() for c in sd.p)
    assert all(x.data_ptr() % 16 == 0 for x in p)
    check(ctx, sd.ix, sd.n_build, p, prefix(sd.want, n), dict(IVX_PART_TILES=2), "aligned", device_marks=True)


def test_bitmap_forced(ctx):
    """an index that carries the occupancy bitmap: the filtering instantiation keeps its 8192-row tiles"""
    sd = side(ctx, "sparse")
    with env(IVX_FILTER="force"):
        ixf = ctx.build(pyivx.KIND_OVERLAP, *sd.b, n_keys=sd.nk)
    try:
        n = 2 * TILE + 1
        layf = ixf.layout(); layf["nkeys"] = sd.nk
        assert layf["fg"] != rf.NOFG and probe_form(layf, n, n, BASE_ENV)["filter"], layf
        p = tuple(c[:n] for c in sd.p)
        check(ctx, ixf, sd.n_build, p, prefix(sd.want, n), dict(IVX_PART_TILES=2), "bitmap")
    finally:
        ixf.free()


def test_more_than_kt_max_keys(ctx):
    """300 keys, 100 of them with rows: 100 regions in one 256-digit pass, but the key tables do not fit LDS"""
    sd = side(ctx, "keys300")
    assert not sd.open and not probe_form(sd.lay, TILE, TILE, BASE_ENV)["klds"], sd.lay
    n = 2 * TILE + 1
    p = tuple(c[:n] for c in sd.p)
    check(ctx, sd.ix, sd.n_build, p, prefix(sd.want, n), dict(IVX_PART_TILES=2), "keys300")


def test_per_row_values_keep_their_tiles(ctx):
    """count_overlaps, coverage, per-row counts and exists come back through the un-permute table, which is indexed by
    8192-row tiles: the setting changes nothing for them"""
    sd = side(ctx, "sparse")
    n = 2 * TILE + 1
    p = tuple(c[:n] for c in sd.p)
    wcnt = sd.want[2][:n]
    for big in ("1", "0"):
        with env(**BASE_ENV, IVX_PART_BIG=big, IVX_PART_TILES=2):
            tot, pr = ctx.overlap_count(sd.ix, *p, per_row=True)
            ex = ctx.exists(sd.ix, *p)
            rf.check_rowvals(ctx, sd.b, p, None, knobs=("default",))
        assert tot == int(wcnt.sum()) and (np.asarray(pr).view(np.uint32).astype(np.uint64) == wcnt).all(), big
        assert (np.asarray(ex).astype(bool) == (wcnt > 0)).all(), big
