"""-m gpu: the overlap thresholds through the C ABI (include/ivx_where.h) -- ivx_probe_overlap_count_where,
ivx_probe_mark_build_where, ivx_probe_overlap_agg_where, ivx_probe_overlap_select_where and ivx_pairs_where -- on the direct
path and on the region path, in host and device memory mode.

Expected values come from tests/overlap_where_oracle.py: the CPU oracle's pairs, the pass rule in numpy int64 on them, then the
existing reductions of the aggregates and select.  Every comparison is exact and on whole output arrays.  Every threshold case
first shows, on the oracle alone, that it filters something and not everything.  The region-path cases reach each index form
with the builders of tests/test_gpu_region_forms.py (imported from there): the level-0 lean build with build rows that span
region borders, probe rows that only k_lean_rest can answer and regions whose last wavefront batch is ragged; a slice of
exactly IVX_RP_ECAP entries and one more (no longer lean); the sparse build; a three-key build with the occupancy bitmap and
build rows of varying length; three keys of several regions each.  Each asserts its form through ivx_index_layout and, by the
scratch the calls reserve, whether the lean kernels took the call (the direct kernel takes none)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pair_set
import overlap_where_oracle as wo
from overlap_where_oracle import W

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402
import test_gpu_region_forms as rf  # noqa: E402
import test_gpu_overlap_select as tsel  # noqa: E402
from entry_cases import CAPACITY, INVALID, OK, OOM, SIZES, UNSUPPORTED, Delay, Env, LateMode, Mode, Refused, _same, cint, ivals, u32, u64  # noqa: E402
from test_gpu_entry_state import designed, inside  # noqa: E402

pytestmark = pytest.mark.gpu

env, cols = rf.env, rf.cols
PATHS = ("direct", "regions")
MEMS = ("host", "device")
NULL = pyivx.NULL_IDX
TILE = pyivx.PAIRS_WHERE_TILE
# the six thresholds every shape is run under
THRESHOLDS = {"min_bases_20": W(min_bases=20), "probe_half": W(probe=(1, 2)), "build_half": W(build=(1, 2)),
              "both_half": W(probe=(1, 2), build=(1, 2)), "either_half": W(probe=(1, 2), build=(1, 2), either=1),
              "probe_whole": W(probe=(1, 1))}


def test_tile_constant_is_the_kernels():
    src = open(os.path.join(ROOT, "datafusion-bio-functions_amd", "csrc", "ivx_where.hpp")).read()
    import re
    t, pi = (int(re.search(r"constexpr int " + name + r" = (\d+);", src).group(1)) for name in ("PW_T", "PW_PI"))
    assert re.search(r"constexpr int PW_TILE = PW_T \* PW_PI;", src) and t * pi == TILE and t % 64 == 0


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


dev = tsel.dev


def host(t):
    if t is None or not pyivx._is_torch(t):
        return t
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def ow(w):
    return None if w is None else pyivx.OverlapWhere(**w.kw())


def eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


class Shape:
    """a build, its index, a probe batch and the oracle's pairs; device copies made once"""

    def __init__(self, ctx, b, p, nk, val_seed=5):
        self.b, self.p, self.nk = b, p, nk
        self.ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=nk)
        self.want = wo.Want(b, p)
        rng = np.random.default_rng(val_seed)
        self.val64 = rng.integers(-(1 << 40), 1 << 40, len(b[1])).astype(np.int64)
        self.val32 = rng.integers(-50, 51, len(b[1])).astype(np.int32)
        self.dp = [dev(c) for c in p]
        self.dval = {4: dev(self.val32), 8: dev(self.val64)}
        self.prior = np.zeros((len(b[1]) + 31) // 32, np.uint32)
        self.prior[::3] = 0x00010001

    def cols(self, mem):
        return self.p if mem == "host" else self.dp

    def val(self, mem, vb=8):
        v = self.val64 if vb == 8 else self.val32
        return v if mem == "host" else self.dval[vb]


def check_entries(ctx, S, w, mem, what, agg_bytes=(8,), bys=("max_overlap",), scores=(True,), alone=False):
    """count (all three outputs), marks into a pre-set bitmap, the aggregates with all six outputs and select: each equals
    the restatement"""
    want, p, o = S.want, S.cols(mem), ow(w)
    got = ctx.overlap_count_where(S.ix, *p, where=o)
    ctx.synchronize()
    eq(host(got["per_row"]), want.per_row(w), (what, "per_row"))
    eq(host(got["exists"]), want.exists(w), (what, "exists"))
    assert got["total"] == len(want.pairs(w)[0]), (what, "total")
    if alone:
        for name in ("per_row", "exists", "total"):
            one = ctx.overlap_count_where(S.ix, *p, where=o, **{k: k == name for k in ("per_row", "exists", "total")})
            ctx.synchronize()
            assert list(one) == [name], what
            if name == "total":
                assert one[name] == got["total"], what
            else:
                eq(host(one[name]), host(got[name]), (what, name, "alone"))
    marks = S.prior.copy() if mem == "host" else dev(S.prior)
    ctx.mark_build(S.ix, *p, marks, where=o)
    ctx.synchronize()
    eq(host(marks), want.marks(w, S.prior), (what, "marks"))
    for vb in agg_bytes:
        a = ctx.overlap_agg(S.ix, *p, S.val(mem, vb), where=o)
        ctx.synchronize()
        wa = want.agg(w, S.val("host", vb))
        for name in pyivx.AGG_OUTPUTS:
            eq(host(a[name]), wa[name], (what, "agg", vb, name))
    for by in bys:
        for score in scores:
            vb = 4 if by == "min_val" else 8
            val = S.val(mem, vb) if by.endswith("_val") else None
            bi, sc = ctx.overlap_select(S.ix, *p, by=by, val=val, score=score, where=o)
            ctx.synchronize()
            wi, ws = want.select(w, by, S.val("host", vb) if by.endswith("_val") else None)
            eq(host(bi), wi, (what, "select", by))
            if score:
                eq(host(sc), ws, (what, "score", by))


def check_filters_something(S, w):
    """on the oracle alone: the threshold keeps between 1 % and 95 % of the pairs and changes a per-row count, an exists byte
    and a mark bit"""
    want = S.want
    n_all, n_kept = len(want.wb), len(want.pairs(w)[0])
    assert n_all > 0 and 0.01 * n_all <= n_kept <= 0.95 * n_all, (w, n_kept, n_all)
    assert (want.per_row(w) != want.per_row(None)).any(), w
    assert (want.exists(w) != want.exists(None)).any(), w
    assert (want.marks(w) != want.marks(None)).any(), w


# ---------------------------------------------------------------- the direct shape

@pytest.fixture(scope="module")
def small(ctx):
    """3000 build rows over 5 keys, lengths 0 .. 399; 5000 probe rows, lengths -2 .. 119, on those keys, on a key without build
    rows and on a key the index lacks (test_gpu_overlap_select.py's shape)"""
    s = Shape(ctx, tsel.direct_build(3000, 5, 11), tsel.strict_probes(5000, 5, 12), 6)
    p = s.p
    assert (p[0] == 5).any() and (p[0] == 10).any() and (p[2].astype(np.int64) < p[1].astype(np.int64)).any()
    assert 2000 < len(s.want.wb) < 4000
    yield s
    s.ix.free()


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("name", list(THRESHOLDS))
def test_where_direct(ctx, small, name, mem):
    """the direct shape.  (IVX_JOIN_PATH=regions is run on it as well, but this small index need not qualify for the lean
    kernels, and nothing here claims they ran: the region forms below assert that.)"""
    w = THRESHOLDS[name]
    check_filters_something(small, w)
    for path in PATHS:
        with env(IVX_JOIN_PATH=path):
            check_entries(ctx, small, w, mem, (name, mem, path))


@pytest.mark.parametrize("mem", MEMS)
def test_where_every_output_form(ctx, small, mem):
    """count's outputs each alone; int32 and int64 values; every criterion with and without the score"""
    with env(IVX_JOIN_PATH="direct"):
        check_entries(ctx, small, THRESHOLDS["probe_half"], mem, ("forms", mem), agg_bytes=(4, 8), bys=wo.sel.BY, scores=(True, False), alone=True)


# ---------------------------------------------------------------- the region shape

def region_probes(b, lay, geo, n_rand, seed):
    """rows all over a lean one-key build: random rows of lengths -2 .. 299 (end < start: an escape), rows from a region's last
    coordinates through its halo and one coordinate past it (the latter: k_lean_rest), rows at and past the packed length's
    maximum, rows that start before the key's first and behind its last build row, and 1300 more rows in each of two regions
    (several wavefront batches of 512 rows there, the last one ragged)"""
    rng = np.random.default_rng(seed)
    hi = int(b[1].max())
    st = rng.integers(-1000, hi + 1000, n_rand)
    rand = cols(np.zeros(n_rand), st, st + rng.integers(-2, 300, n_rand))
    f = rf.probe_form(lay, n_rand + 5000, 1, {"IVX_JOIN_PATH": "regions"}, mode="exists")
    assert f["packed"], f
    maxlen = f["maxlen"]
    x = rng.integers(0, hi - 200_000, 300)
    longs = rf.cat(cols(np.zeros(100), x[:100], x[:100] + maxlen - 1), cols(np.zeros(100), x[100:200], x[100:200] + maxlen),
                   cols(np.zeros(100), x[200:], x[200:] + maxlen + 70_000))
    outside = cols(np.zeros(6), [-5000, -300, -1, hi + 1, hi + 255, hi + 256], [100, 0, 600, hi + 300, hi + 255, hi + 9000])
    past, last = rf.halo_probes(geo, lay["sh0"], True), rf.halo_probes(geo, lay["sh0"], False)
    assert len(past[1]) and len(last[1])
    crowd = []
    for r in (geo["regs"][3], geo["regs"][len(geo["regs"]) // 2]):
        cs = rng.integers(r["rbase"], r["rend"], 1300)
        crowd.append(cols(np.zeros(1300), cs, cs + rng.integers(0, 300, 1300)))
    p = rf.cat(past, last, longs, outside, rand, *crowd)
    order = rng.permutation(len(p[1]))
    return tuple(c[order] for c in p)


@pytest.fixture(scope="module")
def lean(ctx):
    b = rf.level0_lean_build(False)
    probe_ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    lay, geo = rf.layout_of(probe_ix, *b, 1)
    probe_ix.free()
    assert lay["pk24"] == 1 and lay["slow"] == 0 and lay["nlev"] >= 1 and 8 < lay["nreg"] <= rf.IVX_MAXREG, lay
    s = Shape(ctx, b, region_probes(b, lay, geo, 60_000, 21), 1)
    s.lay, s.geo = lay, geo
    # build rows that span region borders: a row that starts in one region and ends in the next
    bs, be = b[1].astype(np.int64), b[2].astype(np.int64)
    borders = np.array([r["rend"] for r in geo["regs"][:-1]], np.int64)
    spanning = ((bs[:, None] < borders[None, :]) & (be[:, None] >= borders[None, :])).any(axis=1)
    assert spanning.sum() >= len(borders)
    assert np.isin(np.flatnonzero(spanning), s.want.wb).any()                 # ... and probe rows match them
    # regions whose routed rows end in a ragged wavefront batch (8 rows per lane, 64 lanes), some of more than one batch
    reg = rf.route_region(lay, b, s.p)
    per_reg = np.bincount(reg[reg >= 0], minlength=lay["nreg"])
    assert ((per_reg % 512 != 0) & (per_reg > 512)).sum() >= 2, per_reg
    yield s
    s.ix.free()


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("name", list(THRESHOLDS))
def test_where_regions(ctx, lean, name, mem):
    w = THRESHOLDS[name]
    check_filters_something(lean, w)
    for path in PATHS:
        with env(IVX_JOIN_PATH=path):
            check_entries(ctx, lean, w, mem, (name, mem, path), bys=("max_overlap", "max_val"))


def test_where_regions_every_output_form(ctx, lean):
    with env(IVX_JOIN_PATH="regions"):
        check_entries(ctx, lean, THRESHOLDS["either_half"], "device", "forms", agg_bytes=(4, 8), bys=wo.sel.BY, scores=(True, False), alone=True)


def test_where_region_path_reserves_scratch(lean):
    """under IVX_JOIN_PATH=regions each filtered per-row entry routes its rows (scratch pages); under =direct none of them
    reserves anything for device columns, but count's total-only form (its per-row counts live in scratch)"""
    o = ow(THRESHOLDS["probe_half"])
    p = lean.dp
    calls = {
        "count": lambda c: c.overlap_count_where(lean.ix, *p, where=o, total=False),
        "exists": lambda c: c.overlap_count_where(lean.ix, *p, where=o, per_row=False, total=False),
        "marks": lambda c: c.mark_build(lean.ix, *p, dev(lean.prior), where=o),
        "agg": lambda c: c.overlap_agg(lean.ix, *p, lean.dval[8], where=o),
        "select": lambda c: c.overlap_select(lean.ix, *p, by="max_overlap", where=o),
    }
    for name, call in calls.items():
        for path in PATHS:
            c = pyivx.Ctx(0)
            try:
                with env(IVX_JOIN_PATH=path):
                    call(c)
                c.synchronize()
                assert (c.reserved_bytes() > 0) == (path == "regions"), (name, path, c.reserved_bytes())
            finally:
                c.close()
    c = pyivx.Ctx(0)
    try:
        with env(IVX_JOIN_PATH="direct"):
            got = c.overlap_count_where(lean.ix, *p, where=o, per_row=False, exists=False)
        assert got["total"] == len(lean.want.pairs(THRESHOLDS["probe_half"])[0])
        assert c.reserved_bytes() >= 4 * len(lean.p[1])
    finally:
        c.close()


# ---------------------------------------------------------------- the index forms of tests/test_gpu_region_forms.py

def with_inverted(p, rng, share=0.03):
    """a share of the rows turned into rows with end < start (escapes: the packed form cannot carry them)"""
    k, s, e = (c.copy() for c in p)
    i = rng.random(len(s)) < share
    e[i] = s[i] - rng.integers(1, 40, int(i.sum())).astype(np.int32)
    return k, s, e


class Form(Shape):
    """a Shape on one of the region forms: `lay` / `geo` its layout as the library reports it, `lean` whether the lean kernels
    may run on it, `min_bases` the threshold that fits its row lengths, `dropped` the probe rows its occupancy bitmap drops
    before routing (or None)"""

    def __init__(self, ctx, name):
        rng = np.random.default_rng(61)
        self.name, self.lean, self.min_bases, self.dropped, build_env = name, True, 20, None, {}
        if name in ("slice_6144", "slice_6145"):
            # region 0's slice holds exactly IVX_RP_ECAP entries; one more and the index is no longer lean (the calls fall back
            # to the direct kernel).  Rows of 16 coordinates: min_bases 8
            b, nk, self.lean, self.min_bases = rf.slice_build(0 if name == "slice_6144" else 1), 1, name == "slice_6144", 8
        elif name == "sparse":
            b, nk = rf.sparse_build(), 1
        elif name == "bitmap_3keys":
            # three keys, build rows of 1 .. 300 coordinates, built with the occupancy bitmap: probe rows in empty blocks are
            # dropped before routing (the launchers' has_filter)
            r7 = np.random.default_rng(7)
            k = r7.integers(0, 3, 20_000)
            s = r7.integers(0, 50_000_000, len(k))
            b, nk, build_env = cols(k, s, s + r7.integers(0, 300, len(k))), 3, {"IVX_FILTER": "force"}
        else:
            # three keys of several lean regions each, build rows of 61 .. 256 coordinates
            assert name == "many_regions_3keys", name
            per = 60_000
            s = np.tile(np.arange(per, dtype=np.int64) * 512, 3)
            b, nk = cols(np.repeat(np.arange(3), per), s, s + rng.integers(60, 256, len(s))), 3
        with env(**build_env):
            probe_ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=nk)
        lay, geo = rf.layout_of(probe_ix, *b, nk)
        probe_ix.free()
        if name.startswith("slice"):
            assert lay["sh0"] == 4 and lay["rcells"] == 1024 and lay["pk24"] == 1 and lay["levrows"] == 1, lay
            assert lay["slow"] == (0 if self.lean else 1) and geo["regs"][0]["ne"] == rf.IVX_RP_ECAP + (not self.lean), lay
            p = with_inverted(rf.edge_probes(geo, 4, rng, 60_000, -100, 3_300_000, maxlen=40), rng)
        elif name == "sparse":
            assert (lay["sh0"], lay["rcells"], lay["slow"], lay["pk24"], lay["fg"]) == (8, 2048, 0, 1, rf.NOFG), lay
            p = rf.cat(rf.halo_probes(geo, 8, True), rf.halo_probes(geo, 8, False), rf.sparse_probes(b, 40_000, 25, lens=(-2, 300)))
        elif name == "bitmap_3keys":
            assert lay["fg"] != rf.NOFG and lay["slow"] == 0 and lay["pk24"] == 1 and lay["nreg"] >= 3, lay
            p = rf.edge_probes(geo, lay["sh0"], rng, 80_000, -100, 50_001_000)
            assert rf.probe_form(lay, len(p[1]), len(p[1]), {"IVX_JOIN_PATH": "regions"})["filter"]
            self.dropped = ~rf.bitmap_pass(lay, b, p)
            assert 0 < int(self.dropped.sum()) < len(p[1])                  # some rows are filtered out, some are routed
        else:
            assert lay["pk24"] == 1 and lay["slow"] == 0 and 6 < lay["nreg"] <= rf.IVX_MAXREG, lay
            n = 150_000
            ps = rng.integers(-1000, 60_000 * 512 + 1000, n)
            # (key 3 is unknown to the index; rows with end < start on every key: k_lean_rest finds its key by the region)
            p = cols(rng.integers(0, 4, n), ps, ps + rng.integers(-2, 600, n))
            inv = p[2].astype(np.int64) < p[1].astype(np.int64)
            assert all((inv & (p[0] == k)).any() for k in range(3))
        with env(**build_env):
            super().__init__(ctx, b, p, nk)
        assert self.ix.layout()["slow"] == lay["slow"]
        self.lay, self.geo = lay, geo
        assert len(np.unique(b[2].astype(np.int64) - b[1])) > 1 or name in ("sparse", "slice_6144", "slice_6145")
        if self.dropped is not None:
            assert not self.want.per_row(None)[self.dropped].any()          # what the bitmap drops matches nothing


FORMS = ("slice_6144", "slice_6145", "sparse", "bitmap_3keys", "many_regions_3keys")


@pytest.fixture(scope="module", params=FORMS)
def form(request, ctx):
    f = Form(ctx, request.param)
    yield f
    f.ix.free()


@pytest.mark.parametrize("mem", MEMS)
def test_where_region_forms(ctx, form, mem):
    """every threshold through every entry on each index form, both paths; on the bitmap form the rows dropped before routing
    get count 0, exists 0 and NULL_IDX (they are part of the restatement's columns, which are compared whole)"""
    th = dict(THRESHOLDS, min_bases_20=W(min_bases=form.min_bases))
    for name, w in th.items():
        check_filters_something(form, w)
        for path in PATHS:
            with env(IVX_JOIN_PATH=path):
                check_entries(ctx, form, w, mem, (form.name, name, mem, path), bys=("max_overlap", "min_val"))
    if form.dropped is not None:
        w = th["probe_half"]
        assert form.want.per_row(w)[~form.dropped].any() and (form.want.select(w, "max_overlap")[0][form.dropped] == NULL).all()


def test_where_region_forms_take_the_lean_kernels(form):
    """device columns under IVX_JOIN_PATH=regions: on a lean form every filtered per-row entry routes its rows into scratch
    (the region launcher took the call); on the form that is not lean the same calls run the direct kernel and reserve nothing"""
    o = ow(THRESHOLDS["probe_half"])
    p = form.dp
    calls = {
        "count": lambda c: c.overlap_count_where(form.ix, *p, where=o, total=False),
        "exists": lambda c: c.overlap_count_where(form.ix, *p, where=o, per_row=False, total=False),
        "marks": lambda c: c.mark_build(form.ix, *p, dev(form.prior), where=o),
        "agg": lambda c: c.overlap_agg(form.ix, *p, form.dval[8], where=o),
        "select": lambda c: c.overlap_select(form.ix, *p, by="max_overlap", where=o),
    }
    for name, call in calls.items():
        c = pyivx.Ctx(0)
        try:
            with env(IVX_JOIN_PATH="regions"):
                call(c)
            c.synchronize()
            assert (c.reserved_bytes() > 0) == form.lean, (form.name, name, c.reserved_bytes())
        finally:
            c.close()


# ---------------------------------------------------------------- identity

@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("which", ["small", "lean"])
def test_where_identity(ctx, small, lean, which, mem):
    """w = NULL and an all-zero w equal the unfiltered entries bit for bit, rows with end < start included"""
    S = small if which == "small" else lean
    p = S.cols(mem)
    assert (S.p[2].astype(np.int64) < S.p[1].astype(np.int64)).any()
    zero = pyivx.OverlapWhere()
    unasked = pyivx.OverlapWhere(probe=(0, 7), build=(0, 0), either=True)
    for path in PATHS:
        with env(IVX_JOIN_PATH=path):
            total, per_row = ctx.overlap_count(S.ix, *p, per_row=True)
            exists = ctx.exists(S.ix, *p)
            marks = ctx.mark_build(S.ix, *p, S.prior.copy() if mem == "host" else dev(S.prior))
            a = ctx.overlap_agg(S.ix, *p, S.val(mem))
            bi, sc = ctx.overlap_select(S.ix, *p, by="min_overlap")
            ctx.synchronize()
            assert total == len(S.want.wb)
            for o in (None, zero, unasked):
                got = ctx.overlap_count_where(S.ix, *p, where=o)
                gm = ctx.mark_build(S.ix, *p, S.prior.copy() if mem == "host" else dev(S.prior), where=o)
                ga = ctx.overlap_agg(S.ix, *p, S.val(mem), where=o)
                gi, gs = ctx.overlap_select(S.ix, *p, by="min_overlap", where=o)
                ctx.synchronize()
                what = (which, mem, path, o)
                eq(host(got["per_row"]), host(per_row), what); eq(host(got["exists"]), host(exists), what)
                assert got["total"] == total, what
                eq(host(gm), host(marks), what)
                for name in pyivx.AGG_OUTPUTS:
                    eq(host(ga[name]), host(a[name]), (what, name))
                eq(host(gi), host(bi), what); eq(host(gs), host(sc), what)
    # the pair filter: every pair, in order
    wb, wp = S.want.wb.astype(np.uint32), S.want.wp.astype(np.uint32)
    cols_ = (wb, wp, S.b[1], S.b[2], S.p[1], S.p[2])
    for o in (None, zero):
        ob, op = ctx.pairs_where(*(cols_ if mem == "host" else [dev(c) for c in cols_]), where=o)
        ctx.synchronize()
        eq(host(ob), wb, (which, mem, "pairs")); eq(host(op), wp, (which, mem, "pairs"))


# ---------------------------------------------------------------- the hand-made boundary table

@pytest.mark.parametrize("mem", MEMS)
def test_where_hand_table(ctx, mem):
    """the boundary table of tests/overlap_where_oracle.py -- a pair exactly on a fraction and one base short, min_bases at len
    and len + 1, the row spanning the whole int32 range under den = 2^31 - 1 -- through every entry; the oracle's pairs are the
    ones written out by hand there"""
    S = Shape(ctx, wo.HAND_BUILD, wo.HAND_PROBE, 2)
    try:
        for w, what, expected in wo.HAND_CASES:
            assert set(zip(*[x.tolist() for x in S.want.pairs(w)])) == expected, what
            for path in PATHS:
                with env(IVX_JOIN_PATH=path):
                    check_entries(ctx, S, w, mem, (what, mem, path), agg_bytes=(4, 8), bys=("max_overlap", "min_overlap", "last_row"))
            wb, wp = S.want.wb.astype(np.uint32), S.want.wp.astype(np.uint32)
            c = (wb, wp, S.b[1], S.b[2], S.p[1], S.p[2])
            ob, op = ctx.pairs_where(*(c if mem == "host" else [dev(x) for x in c]), where=ow(w))
            ctx.synchronize()
            kb, kp = S.want.pairs(w)
            eq(host(ob), kb.astype(np.uint32), what); eq(host(op), kp.astype(np.uint32), what)
    finally:
        S.ix.free()


# ---------------------------------------------------------------- ivx_pairs_where

@pytest.fixture(scope="module")
def pair_world():
    """coordinate columns of 4000 build rows (starts ascending) and 5000 probe rows, and 4 tiles + a ragged tail of (build,
    probe) index pairs in no order: a random probe row with a build row that starts near it -- the filter is computed from the
    coordinates alone, the pairs need not be matches (some are not)"""
    rng = np.random.default_rng(31)
    nb, npr, n = 4000, 5000, 4 * TILE + 37
    bs = np.sort(rng.integers(0, 100_000, nb)); ps = rng.integers(0, 100_000, npr)
    b = (bs.astype(np.int32), (bs + rng.integers(-3, 400, nb)).astype(np.int32))
    p = (ps.astype(np.int32), (ps + rng.integers(-3, 300, npr)).astype(np.int32))
    pi = rng.integers(0, npr, n)
    bi = np.clip(np.searchsorted(bs, ps[pi]) + rng.integers(-6, 4, n), 0, nb - 1)
    return b, p, bi.astype(np.uint32), pi.astype(np.uint32)


def keep_of(w, b, p, bi, pi):
    i, j = bi.astype(np.int64), pi.astype(np.int64)
    return wo.passes(w, b[0][i], b[1][i], p[0][j], p[1][j])


SIZES_PAIRS = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4 * TILE + 37]


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("n", SIZES_PAIRS)
def test_pairs_where_is_the_exact_subsequence(ctx, pair_world, n, mem):
    b, p, bi, pi = pair_world
    put = (lambda a: a) if mem == "host" else dev
    db, dp = [put(c) for c in b], [put(c) for c in p]
    for w in (W(probe=(1, 2)), W(min_bases=30, build=(1, 4)), W(probe=(1, 3), build=(1, 3), either=1), W(min_bases=10**6)):
        keep = keep_of(w, b, p, bi[:n], pi[:n])
        if n >= TILE and w.min_bases < 10**6:
            assert 0.02 * n < keep.sum() < 0.98 * n, (w, keep.sum())
        args = (put(bi[:n]), put(pi[:n]), db[0], db[1], dp[0], dp[1])
        assert ctx.pairs_where(*args, where=ow(w), count_only=True) == keep.sum()
        ob, op = ctx.pairs_where(*args, where=ow(w))
        ctx.synchronize()
        eq(host(ob), bi[:n][keep], (n, w)); eq(host(op), pi[:n][keep], (n, w))


def raw_pairs(ctx, bi, pi, n, b, nb, p, npr, w, ob, op, cap, mem=pyivx.MEM_HOST):
    ptr = lambda a: None if a is None else pyivx._ptr(a)
    m = u64(0xDEAD)
    st = pyivx.lib().ivx_pairs_where(ctx.h, mem, ptr(bi), ptr(pi), n, ptr(b[0]), ptr(b[1]), nb, ptr(p[0]), ptr(p[1]), npr,
                                     None if w is None else C.byref(w), ptr(ob), ptr(op), cap, C.byref(m))
    return st, m.value, pyivx.lib().ivx_last_error(ctx.h).decode()


def test_pairs_where_refusals(ctx, pair_world):
    b, p, bi, pi = pair_world
    n, nb, npr = len(bi), len(b[0]), len(p[0])
    w = ow(W(probe=(1, 2))).c_struct()
    need = int(keep_of(W(probe=(1, 2)), b, p, bi, pi).sum())

    def fresh(k):
        return np.full(max(k, 1), 0xA5A5A5A5, np.uint32), np.full(max(k, 1), 0xA5A5A5A5, np.uint32)

    def clean(*bufs):
        return all((x == 0xA5A5A5A5).all() for x in bufs)

    # the counting call
    assert raw_pairs(ctx, bi, pi, n, b, nb, p, npr, w, None, None, 0)[:2] == (OK, need)
    # one short: the size needed, nothing written
    ob, op = fresh(need)
    st, m, text = raw_pairs(ctx, bi, pi, n, b, nb, p, npr, w, ob, op, need - 1)
    assert (st, m) == (CAPACITY, need) and "pairs_where: output buffers too small" in text and clean(ob, op)
    st, m, _ = raw_pairs(ctx, bi, pi, n, b, nb, p, npr, w, ob, op, need)
    assert (st, m) == (OK, need) and not clean(ob)
    # an index out of range, IVX_NULL_IDX included, on either side, in the first and in the last tile: refused, outputs untouched
    for side, at, v in ((0, 5, nb), (0, n - 1, NULL), (1, TILE + 3, npr), (1, 0, NULL), (0, n - 2, 2**31)):
        cols_ = [bi.copy(), pi.copy()]
        cols_[side][at] = v
        for mem in MEMS:
            ob, op = fresh(n)
            if mem == "host":
                st, m, text = raw_pairs(ctx, cols_[0], cols_[1], n, b, nb, p, npr, w, ob, op, n)
            else:
                dob, dop = dev(ob), dev(op)
                st, m, text = raw_pairs(ctx, dev(cols_[0]), dev(cols_[1]), n, [dev(c) for c in b], nb, [dev(c) for c in p], npr, w, dob, dop, n,
                                        pyivx.MEM_DEVICE)
                ctx.synchronize()
                ob, op = host(dob), host(dop)
            assert st == INVALID and "pairs_where: index out of bounds" in text and m == 0 and clean(ob, op), (side, at, v, mem)
        # ... also by the counting call, and with nothing asked
        assert raw_pairs(ctx, cols_[0], cols_[1], n, b, nb, p, npr, None, None, None, 0)[0] == INVALID
    # aliased outputs
    big = np.zeros(2 * n, np.uint32)
    for ob, op in ((bi, fresh(n)[1]), (fresh(n)[0], pi), (fresh(n)[0], b[0].view(np.uint32)), (big[:n], big[n - 1:2 * n - 1]), (fresh(n)[0], p[1].view(np.uint32))):
        cap = min(len(ob), len(op))
        st, m, text = raw_pairs(ctx, bi, pi, n, b, nb, p, npr, w, ob, op, cap)
        assert st == INVALID and "pairs_where: an output overlaps" in text, text
    assert raw_pairs(ctx, bi, pi, n, b, nb, p, npr, w, fresh(n)[0], None, n)[0] == INVALID
    st = pyivx.lib().ivx_pairs_where(ctx.h, 0, pyivx._ptr(bi), pyivx._ptr(pi), n, pyivx._ptr(b[0]), pyivx._ptr(b[1]), nb, pyivx._ptr(p[0]),
                                     pyivx._ptr(p[1]), npr, None, None, None, 0, None)
    assert st == INVALID and "pairs_where: null n_out" in pyivx.lib().ivx_last_error(ctx.h).decode()


# ---------------------------------------------------------------- the struct's refusals, the index kind

BAD_WHERE = [
    ((-1, 0, 0, 0, 0, 0), "overlap_where: min_bases is negative"),
    ((0, 3, 2, 0, 0, 0), "overlap_where: a fraction is above 1"),
    ((0, 0, 0, 5, 4, 0), "overlap_where: a fraction is above 1"),
    ((0, 1, 0, 0, 0, 0), "overlap_where: a fraction's denominator is 0"),
    ((0, 0, 0, 1, 0, 0), "overlap_where: a fraction's denominator is 0"),
    ((0, 1, 2**31, 0, 0, 0), "overlap_where: a denominator exceeds 2^31 - 1"),
    ((0, 0, 0, 0, 2**31, 0), "overlap_where: a denominator exceeds 2^31 - 1"),
    ((0, 1, 2, 1, 2, 2), "overlap_where: either is 0 or 1"),
    ((5, 0, 0, 0, 0, 7), "overlap_where: either is 0 or 1"),
]


def every_entry(ctx, ix, p, n, val, w, nb, mem=pyivx.MEM_HOST):
    """every entry once with threshold struct w on host columns -> [(name, status, error text, output buffers)]"""
    L, ptr = pyivx.lib(), pyivx._ptr
    fill = lambda k, dt: np.full(max(k, 1) * np.dtype(dt).itemsize, 0xA5, np.uint8).view(dt)
    wp = None if w is None else C.byref(w)
    head = (ctx.h, ix.h, mem, ptr(p[0]), ptr(p[1]), ptr(p[2]), n)
    out = []
    pr, ex, tot = fill(n, np.uint32), fill(n, np.uint8), u64(0xDEAD)
    st = L.ivx_probe_overlap_count_where(*head, wp, ptr(pr), ptr(ex), C.byref(tot))
    out.append(("count", st, L.ivx_last_error(ctx.h).decode(), [pr, ex]))
    marks = fill((nb + 31) // 32, np.uint32)
    st = L.ivx_probe_mark_build_where(*head, wp, ptr(marks))
    out.append(("marks", st, L.ivx_last_error(ctx.h).decode(), [marks]))
    outs = [fill(n, np.uint32)] + [fill(n, np.int64) for _ in range(5)]
    st = L.ivx_probe_overlap_agg_where(*head, ptr(val), 8, wp, *[ptr(o) for o in outs])
    out.append(("agg", st, L.ivx_last_error(ctx.h).decode(), outs))
    bi, sc = fill(n, np.uint32), fill(n, np.int64)
    st = L.ivx_probe_overlap_select_where(*head, ptr(val), 8, 1, wp, ptr(bi), ptr(sc))
    out.append(("select", st, L.ivx_last_error(ctx.h).decode(), [bi, sc]))
    return out


def test_where_struct_refusals_and_index_kind(ctx, small, pair_world):
    S, n = small, len(small.p[1])
    for fields, text in BAD_WHERE:
        w = pyivx.OverlapWhereC(*fields)
        for name, st, err, outs in every_entry(ctx, S.ix, S.p, n, S.val64, w, len(S.b[1])):
            assert st == INVALID and text in err, (name, fields, err)
            assert all((o.view(np.uint8) == 0xA5).all() for o in outs), (name, fields)
        b, p, bi, pi = pair_world
        ob, op = np.full(len(bi), 0xA5A5A5A5, np.uint32), np.full(len(bi), 0xA5A5A5A5, np.uint32)
        st, m, err = raw_pairs(ctx, bi, pi, len(bi), b, len(b[0]), p, len(p[0]), w, ob, op, len(bi))
        assert st == INVALID and text in err and (ob == 0xA5A5A5A5).all(), (fields, err)
    # a fraction that is not asked may carry any denominator
    ok = pyivx.OverlapWhereC(0, 0, 0, 0, 2**31 - 1, 1)
    assert all(st == OK for _, st, _, _ in every_entry(ctx, S.ix, S.p, n, S.val64, ok, len(S.b[1])))
    # count: no output wanted
    st = pyivx.lib().ivx_probe_overlap_count_where(ctx.h, S.ix.h, 0, pyivx._ptr(S.p[0]), pyivx._ptr(S.p[1]), pyivx._ptr(S.p[2]), n, None, None, None, None)
    assert st == INVALID and "overlap_count_where: no output wanted" in pyivx.lib().ivx_last_error(ctx.h).decode()
    # another index kind
    cnt = ctx.build(pyivx.KIND_COUNT, *S.b, n_keys=S.nk)
    w = ow(THRESHOLDS["probe_half"]).c_struct()
    for name, st, err, outs in every_entry(ctx, cnt, S.p, n, S.val64, w, len(S.b[1])):
        assert st == UNSUPPORTED and "index kind does not match" in err, (name, err)
        assert all((o.view(np.uint8) == 0xA5).all() for o in outs), name
    # n = 0: a no-op, metered as a batch without output
    ctx.reset_metrics()
    for name, st, err, outs in every_entry(ctx, S.ix, S.p, 0, S.val64, w, len(S.b[1])):
        assert st == OK and all((o.view(np.uint8) == 0xA5).all() for o in outs), name
    m = ctx.metrics()
    assert (m["input_batches"], m["input_rows"], m["output_batches"], m["output_rows"]) == (4, 0, 0, 0), m
    ctx.reset_metrics()
    assert all(st == OK for _, st, _, _ in every_entry(ctx, S.ix, S.p, n, S.val64, w, len(S.b[1])))
    m = ctx.metrics()
    assert (m["input_batches"], m["input_rows"], m["output_rows"]) == (4, 4 * n, 3 * n), m     # (the marks make no output rows)
    cnt.free()


def test_where_count_drops_the_join_plan(ctx, lean):
    """a total-only count of the region path leaves its routed rows for the fill; a filtered count in between drops them and
    the fill still returns the oracle's pairs, which the pair filter then cuts to the filtered oracle pairs"""
    S, w = lean, THRESHOLDS["probe_half"]
    with env(IVX_JOIN_PATH="regions"):
        for mem in MEMS:
            p = S.cols(mem)
            total = ctx.overlap_count(S.ix, *p)
            assert total == len(S.want.wb) and ctx.debug_state()["join_valid"] == 1
            got = ctx.overlap_count_where(S.ix, *p, where=ow(w), per_row=False, exists=False)
            assert ctx.debug_state()["join_valid"] == 0 and got["total"] == len(S.want.pairs(w)[0])
            ob, op = ctx.overlap_fill(S.ix, *p, cap=total)
            b, q = (S.b, S.p) if mem == "host" else ([dev(c) for c in S.b], S.dp)
            fb, fp = ctx.pairs_where(ob, op, b[1], b[2], q[1], q[2], where=ow(w))
            ctx.synchronize()
            assert len(ob) == total and (pair_set(host(ob), host(op)) == pair_set(S.want.wb, S.want.wp)).all(), mem
            assert (pair_set(host(fb), host(fp)) == pair_set(*S.want.pairs(w))).all(), mem
            # stable: the filtered pairs are a subsequence of the fill's
            keep = keep_of(w, S.b[1:], S.p[1:], host(ob), host(op))
            eq(host(fb), host(ob)[keep], mem); eq(host(fp), host(op)[keep], mem)


# ---------------------------------------------------------------- the catalogue's walks, as a local case

WHERE_CASES = ("probe_overlap_count_where", "probe_mark_build_where", "probe_overlap_agg_where", "probe_overlap_select_where",
               "pairs_where")


def probe_where(E, M, n):
    """all five entries under probe 1/2 and min_bases 10: the catalogue's five cases (entry_cases.py) one after the other on
    one context, their results in one dict (the cases name their results apart)"""
    from entry_cases import CASES
    res = {}
    for name in WHERE_CASES:
        one = CASES[name](E, M, n)
        assert not set(one) & set(res), name
        res.update(one)
    # the pair filter is the catalogue's sizing / fill / one-short triple (entry_cases.sized: the fill is IVX_OK with the sizing
    # call's count, one short is IVX_ERR_CAPACITY): the sizing call's status, and what the fill wrote, under the names used below
    res["st.pairs"], res["n_out"] = res["pairs.sizing"]
    assert res["pairs.fill"] == (OK, res["n_out"]) and res.get("pairs.short", (CAPACITY, res["n_out"])) == (CAPACITY, res["n_out"]), n
    res["ob"], res["op"] = res["pairs.fill.0"], res["pairs.fill.1"]
    return res


def case_run(E, M, n, path, rows=None):
    from entry_cases import shaped
    with env(IVX_JOIN_PATH=path):
        if rows is None:
            return probe_where(E, M, n)
        with shaped(cols=rows):
            return probe_where(E, M, n)


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    assert all(v == OK for k, v in want.items() if k.startswith("st.")), (what, {k: v for k, v in want.items() if k.startswith("st.")})
    diff = [k for k in want if not _same(got[k], want[k])]
    assert not diff, (what, {k: (got[k], want[k]) for k in diff[:2]})


def spread_probes(n, seed):
    return inside(designed(), n, seed)


@pytest.fixture(scope="module")
def E():
    e = Env(designed())
    lay = e.ix[0].layout()
    assert lay["nreg"] > 1 and lay["slow"] == 0 and lay["pk24"] == 1, lay      # the lean kernels can run
    yield e
    e.close()


@pytest.fixture(scope="module")
def host_results(E):
    """host mode on a context that is never limited or late: (n, path) -> the case's results, held against the restatement"""
    got = {}
    for n in SIZES:
        for path in PATHS:
            got[n, path] = case_run(E, Mode(False), n, path)
        assert_same(got[n, "regions"], got[n, "direct"], n)
    n = SIZES[0]
    p = ivals(n, 29, span=4000)
    w = W(min_bases=10, probe=(1, 2))
    want = wo.Want(E.build_cols, p)
    g = got[n, "direct"]
    kept = len(want.pairs(w)[0])
    assert 0 < kept < len(want.wb)
    eq(g["per_row"], want.per_row(w), "case"); eq(g["exists"], want.exists(w), "case")
    assert g["total"] == g["total2"] == kept
    val = np.random.default_rng(30).integers(-5, 6, E.n_build).astype(np.int64)
    wa = want.agg(w, val)
    for name in pyivx.AGG_OUTPUTS:
        eq(g["agg." + name], wa[name], name)
    wi, ws = want.select(w, "max_overlap")
    eq(g["idx"], wi, "idx"); eq(g["score"], ws, "score")
    mine = np.zeros((E.n_build + 31) // 32, np.uint32)
    mine[::3] = 0x00010001
    eq(g["marks"], want.marks(w, mine), "marks")
    i = np.arange(n)
    keep = wo.passes(w, E.build_cols[1][:n], E.build_cols[2][:n], p[1], p[2])
    eq(g["ob"], i[keep].astype(np.uint32), "pairs"); assert g["n_out"] == keep.sum()
    return got


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", SIZES)
def test_where_case_host_and_device_agree(E, host_results, n, path):
    assert_same(case_run(E, Mode(True), n, path), host_results[n, path], (n, path))


@pytest.fixture(scope="module")
def late_world():
    import torch
    S = torch.cuda.Stream()
    L, H = Env(designed(), stream=S), Env(designed())
    yield S, L, H, Delay(S)
    L.close(); H.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", [SIZES[0], 100_000])
def test_where_case_late_inputs(late_world, n, path):
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
        assert np.count_nonzero(want["idx"] != NULL) > n // 4


@pytest.mark.parametrize("devmode", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("path", PATHS)
def test_where_case_refused_reservations(path, devmode):
    """the memory limit stepped up from what the context holds at rest, one refused reservation at a time: IVX_ERR_OOM leaves
    the outputs untouched (host mode) and nothing reserved behind it, and the same calls under no limit give the full answer"""
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
        for attempt in range(129):
            assert attempt < 128, (path, devmode, limit)
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
        assert points > 0, (path, devmode)          # (the total-only count and the pair filter reserve scratch in every mode)
    finally:
        E.ctx.set_memory_limit(0)
        E.close()
