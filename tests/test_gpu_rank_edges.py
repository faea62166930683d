"""-m gpu: count_overlaps, coverage and nearest at the edges of their index builds and probes -- the nearest build's sort
forms (the 4096-row cut, runs of 64 / 65 equal (key, start) rows, the one-word fit boundary, 2048 / 2049 keys, presorted rows),
the rank grids (a designed column with every gap length around the wavefront fill's switch, int32 extremes, empty and tiny
builds, more keys than the LDS tables, the routing view's 1023-key limit), the coverage probe's switch to prefix sums, strict
mode's wrap at the int32 extremes, probe batch sizes around the launch shapes, and nearest's k against a key's row count.

Every case compares with the CPU oracle bit for bit, and reads the form the index took (pyivx.Index.forms(), the test hook
ivx_debug_index_forms) to prove that it reached the path it names: the expected forms are the plain rules of
tests/rank_forms.py, whose designed inputs tests/test_rank_forms_cpu.py checks without a GPU."""
import os
import sys

import numpy as np
import pytest

import rank_forms as rf
from conftest import ROOT
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

LO, HI = rf.LO, rf.HI
KIND = {"count": pyivx.KIND_COUNT, "coverage": pyivx.KIND_COVERAGE, "nearest": pyivx.KIND_NEAREST}
assert (rf.PRESORTED, rf.REPAIR, rf.FULL) == (pyivx.NEAR_ORDER_PRESORTED, pyivx.NEAR_ORDER_REPAIR, pyivx.NEAR_ORDER_FULL)
assert (rf.FB_NOFIT, rf.FB_LIN_RUN, rf.FB_SE_RUN) == (pyivx.NEAR_FB_NOFIT, pyivx.NEAR_FB_LIN_RUN, pyivx.NEAR_FB_SE_RUN)
ROWVAL_PATHS = ("direct", "regions", "routed")
# nearest k = 1: (IVX_NEAREST_PATH, IVX_NEAREST_PMAX_FIRST)
NEAREST_PATHS = (("direct", None), ("routed", None), ("routed", "0"))


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


_memo = {}


def once(key, fn):
    """designed inputs, expected forms and oracle answers are made once and shared (nobody writes to them)"""
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def table(name, *args):
    return once(("table", name) + args, lambda: getattr(rf, name)(*args))


def build(ctx, kind, t):
    return ctx.build(KIND[kind], t["bk"], t["bs"], t["be"], n_keys=t["nkeys"])


def check_forms(ix, kind, t, tag):
    """the readout equals the plain rules; -> the readout"""
    f = ix.forms()
    want = once(("forms", kind, tag), lambda: rf.expected_grids(kind, t["bk"], t["bs"], t["be"], t["nkeys"]))
    assert f["kind"] == KIND[kind]
    assert f["grids"] == want["grids"], (tag, kind, f, want)
    assert f["nroute_nreg"] == want["nroute_nreg"], (tag, kind, f, want)
    if kind != "nearest":
        assert (f["near_words"], f["near_order"], f["near_fallback"]) == (0, 0, 0)
    return f


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert len(got) == len(want), (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, "rows", bad[:5].tolist(), "got", got[bad[:5]].tolist(), "want", want[bad[:5]].tolist())


def check_rowval(ctx, mp, kind, ix, t, probes, tag, stricts=(False, True), paths=ROWVAL_PATHS):
    fn, ofn = (ctx.count_overlaps, orc.count_overlaps) if kind == "count" else (ctx.coverage, orc.coverage)
    pk, ps, pe = probes
    for strict in stricts:
        want = once(("rowval", kind, tag, strict), lambda: ofn(t["bk"], t["bs"], t["be"], pk, ps, pe, strict=strict))
        for path in paths:
            mp.setenv("IVX_ROWVAL_PATH", path)
            _same(fn(ix, pk, ps, pe, strict=strict), want, (tag, kind, "strict" if strict else "weak", path))
    mp.delenv("IVX_ROWVAL_PATH")


def check_nearest1(ctx, mp, ix, t, probes, tag, overlaps=(True, False), stricts=(False, True), paths=NEAREST_PATHS):
    pk, ps, pe = probes
    for ovl in overlaps:
        for strict in stricts:
            wb, wp, wd = once(("nearest", tag, 1, ovl, strict), lambda: orc.nearest(t["bk"], t["bs"], t["be"], pk, ps, pe, k=1, overlap=ovl, strict=strict))
            for path, pmax in paths:
                mp.setenv("IVX_NEAREST_PATH", path)
                if pmax is not None:
                    mp.setenv("IVX_NEAREST_PMAX_FIRST", pmax)
                gb, gp, gd = ctx.nearest(ix, pk, ps, pe, k=1, overlap=ovl, strict=strict)
                mp.delenv("IVX_NEAREST_PMAX_FIRST", raising=False)
                what = (tag, "nearest k=1", "overlaps" if ovl else "no overlaps", "strict" if strict else "weak", path, pmax)
                _same(gb, wb, what + ("rows",)); _same(gp, wp, what + ("probe rows",)); _same(gd, wd, what + ("distances",))
    mp.delenv("IVX_NEAREST_PATH")


def check_nearestk(ctx, ix, t, probes, tag, k, overlap=True, strict=False):
    pk, ps, pe = probes
    wb, wp, wd = once(("nearest", tag, k, overlap, strict), lambda: orc.nearest(t["bk"], t["bs"], t["be"], pk, ps, pe, k=k, overlap=overlap, strict=strict))
    gb, gp, gd = ctx.nearest(ix, pk, ps, pe, k=k, overlap=overlap, strict=strict)
    what = (tag, "nearest", k, overlap, strict)
    _same(gb, wb, what + ("rows",)); _same(gp, wp, what + ("probe rows",)); _same(gd, wd, what + ("distances",))
    return gb, gp


# ====================================================================================== nearest sort forms

def nearest_form_case(ctx, mp, t, tag, expect, sort2=False, run_probes=False):
    """build (with IVX_NEAREST_SORT2 if asked), the build's form is `expect` = (words, order, fallback bits) and what the
    rules say, the grids and the routing view are what the rules say, and k = 1 on every path, k = 3 (and k = 66 on the
    long runs) equal the oracle"""
    assert rf.nearest_form(t, sort2) == expect
    if sort2:
        mp.setenv("IVX_NEAREST_SORT2", "1")
    ix = build(ctx, "nearest", t)
    mp.delenv("IVX_NEAREST_SORT2", raising=False)
    f = check_forms(ix, "nearest", t, tag)
    assert (f["near_words"], f["near_order"], f["near_fallback"]) == expect, f
    check_nearest1(ctx, mp, ix, t, t["probes"], tag)
    check_nearestk(ctx, ix, t, t["probes"], tag, 3)
    if run_probes:
        gb, gp = check_nearestk(ctx, ix, t, t["run_probes"], tag + "/runs", 66)
        # a point on a run's start overlaps the whole run: it comes back whole, in (end, row) order (rows that start
        # before the run and reach it come first, the nearest other rows fill up to k)
        qk, qs, qe = t["run_probes"]
        for key, start in t["runs"]:
            i = int(np.flatnonzero((qk == key) & (qs == start) & (qe == start))[0])
            got = gb[gp == i]
            rows = np.flatnonzero((t["bk"] == key) & (t["bs"] == start))
            order = rows[np.lexsort((rows, t["be"][rows]))]
            assert len(got) == 66 and got[np.isin(got, rows)].tolist() == order.tolist(), (tag, key, start)
    ix.free()


@pytest.mark.parametrize("n", [4095, 4096])
def test_nearest_build_at_the_4096_row_cut(ctx, monkeypatch, n):
    expect = (2, rf.FULL, 0) if n == 4095 else (1, rf.REPAIR, 0)
    nearest_form_case(ctx, monkeypatch, table("cut_table", n), f"cut{n}", expect)


@pytest.mark.parametrize("sort2", [False, True], ids=["default", "sort2"])
@pytest.mark.parametrize("run_len", [64, 65])
def test_nearest_build_runs_at_the_repair_limit(ctx, monkeypatch, run_len, sort2):
    if run_len == 64:
        expect = (2, rf.REPAIR, 0) if sort2 else (1, rf.REPAIR, 0)
    else:
        expect = (2, rf.FULL, rf.FB_SE_RUN) if sort2 else (2, rf.FULL, rf.FB_LIN_RUN | rf.FB_SE_RUN)
    nearest_form_case(ctx, monkeypatch, table("run_table", run_len), f"run{run_len}", expect, sort2=sort2, run_probes=True)


@pytest.mark.parametrize("n", [131072, 131073])
def test_nearest_build_at_the_one_word_fit_boundary(ctx, monkeypatch, n):
    t = table("fit_table", n)
    assert rf.lin_fit(t["bk"], t["bs"], t["be"], t["nkeys"]) == ((47, 17, True) if n == 131072 else (47, 18, False))
    expect = (1, rf.REPAIR, 0) if n == 131072 else (2, rf.REPAIR, rf.FB_NOFIT)
    nearest_form_case(ctx, monkeypatch, t, f"fit{n}", expect)
    assert once(("forms", "nearest", f"fit{n}"), None)["nroute_nreg"] == 0


@pytest.mark.parametrize("nkeys", [2048, 2049])
def test_nearest_build_at_the_key_table_switch(ctx, monkeypatch, nkeys):
    nearest_form_case(ctx, monkeypatch, table("many_keys_table", nkeys), f"keys{nkeys}", (1, rf.REPAIR, 0))


@pytest.mark.parametrize("variant", ["default", "sort2", "n4000", "one_inversion", "one_inversion_sort2"])
def test_nearest_build_presorted_rows(ctx, monkeypatch, variant):
    n, sort2, inv = (4000 if variant == "n4000" else 5000), variant.endswith("sort2"), variant.startswith("one_inversion")
    t = table("presorted_table", n, inv)
    if inv:
        expect = (2, rf.REPAIR, 0) if sort2 else (1, rf.REPAIR, 0)
    else:
        expect = (2 if sort2 or n < 4096 else 1, rf.PRESORTED, 0)
    nearest_form_case(ctx, monkeypatch, t, f"presorted{n}{inv}", expect, sort2=sort2)


# ====================================================================================== rank grids

def _grid_table(distinct, shuffle):
    v, _ = rf.grid_column(distinct)
    if shuffle:
        v = v[np.random.default_rng(21).permutation(len(v))]
    ps, pe = rf.grid_probes()
    return dict(bk=np.zeros(len(v), np.uint32), bs=v, be=v.copy(), nkeys=1, probes=(np.zeros(len(ps), np.uint32), ps, pe))


@pytest.mark.parametrize("kind", ["count", "coverage", "nearest"])
def test_designed_grid_column(ctx, monkeypatch, kind):
    # count builds its grids from unsorted rows (histogram, scan, scatter); coverage and nearest from sorted columns
    # (k_grid_bounds), value stride 1 and 4.  Coverage merges equal points, so its column has 16 distinct values a cell
    # where the other two have one cell of 300 equal values
    t = once(("gridtable", kind), lambda: _grid_table(kind == "coverage", kind == "count"))
    ix = build(ctx, kind, t)
    f = check_forms(ix, kind, t, "grid")
    assert set(f["grids"].values()) == {(4, 2 * rf.GRID_N + 1)}, f
    assert f["nroute_nreg"] == 32
    if kind == "nearest":
        assert (f["near_words"], f["near_order"]) == (2, rf.PRESORTED)
        check_nearest1(ctx, monkeypatch, ix, t, t["probes"], "grid")
        check_nearestk(ctx, ix, t, t["probes"], "grid", 3)
    else:
        check_rowval(ctx, monkeypatch, kind, ix, t, t["probes"], "grid")
    ix.free()


@pytest.mark.parametrize("kind", ["count", "coverage"])
def test_grids_at_the_int32_extremes(ctx, monkeypatch, kind):
    t = table("extremes_table")
    ix = build(ctx, kind, t)
    f = check_forms(ix, kind, t, "extremes")
    assert min(sh for sh, _ in f["grids"].values()) >= 20                   # key 1 spans all 2^32 values
    check_rowval(ctx, monkeypatch, kind, ix, t, t["probes"], "extremes")
    ix.free()


@pytest.mark.parametrize("n", [0, 1])
@pytest.mark.parametrize("kind", ["count", "coverage"])
def test_tiny_and_empty_builds(ctx, monkeypatch, kind, n):
    t = table("tiny_table", n)
    ix = build(ctx, kind, t)
    f = check_forms(ix, kind, t, f"tiny{n}")
    assert set(f["grids"].values()) == {(0, n)} and f["nroute_nreg"] == n
    check_rowval(ctx, monkeypatch, kind, ix, t, t["probes"], f"tiny{n}")
    ix.free()


@pytest.mark.parametrize("nkeys", [2048, 2049])
@pytest.mark.parametrize("kind", ["count", "coverage"])
def test_grids_with_more_keys_than_the_lds_table(ctx, monkeypatch, kind, nkeys):
    t = table("many_keys_table", nkeys)
    ix = build(ctx, kind, t)
    f = check_forms(ix, kind, t, f"keys{nkeys}")
    assert f["nroute_nreg"] == 0
    check_rowval(ctx, monkeypatch, kind, ix, t, t["probes"], f"keys{nkeys}")
    ix.free()


@pytest.mark.parametrize("wide", [False, True], ids=["one_cell_a_key", "cs_above_0"])
@pytest.mark.parametrize("nfull", [1023, 1024])
def test_routing_view_at_1023_keys(ctx, monkeypatch, nfull, wide):
    # 1023 keys with rows: one region a key; 1024: no routing view, and "routed" then means the direct probe
    t = table("routing_table", nfull, wide)
    tag = f"route{nfull}{wide}"
    for kind in ("count", "coverage", "nearest"):
        ix = build(ctx, kind, t)
        f = check_forms(ix, kind, t, tag)
        assert f["nroute_nreg"] == (1023 if nfull == 1023 else 0), (kind, f)
        if kind == "nearest":
            check_nearest1(ctx, monkeypatch, ix, t, t["probes"], tag, paths=NEAREST_PATHS[1:])
        else:
            check_rowval(ctx, monkeypatch, kind, ix, t, t["probes"], tag, paths=("routed",))
        ix.free()


# ====================================================================================== coverage probe

def _coverage_table():
    bk, first, last = rf.coverage_nodes()
    q, e = rf.coverage_queries(), rf.coverage_edge_queries()
    return dict(bk=bk, bs=first, be=last, nkeys=1, probes=tuple(np.concatenate([a, b]) for a, b in zip(q, e)))


def test_coverage_probe_over_0_to_6_nodes(ctx, monkeypatch):
    # adding the nodes' terms up to two overlapped nodes, prefix sums from three on, zero-length nodes inside; and queries
    # with start == INT32_MIN or end == INT32_MAX (always term by term) over hundreds of nodes
    t = once(("covtable",), _coverage_table)
    ix = build(ctx, "coverage", t)
    f = check_forms(ix, "coverage", t, "cov")
    assert f["grids"]["first"][1] >= rf.COV_NODES
    check_rowval(ctx, monkeypatch, "coverage", ix, t, t["probes"], "cov")
    ix.free()


def test_coverage_wide_nodes_and_wrapped_sums(ctx, monkeypatch):
    t = table("wide_nodes")
    ix = build(ctx, "coverage", t)
    check_forms(ix, "coverage", t, "widenodes")
    check_rowval(ctx, monkeypatch, "coverage", ix, t, t["probes"], "widenodes")
    assert ctx.coverage(ix, *t["probes"])[2] < 0                            # [-100, MAX - 7]: the int32 sum wraps, as the reference's does
    ix.free()


# ====================================================================================== strict wrap

@pytest.mark.parametrize("kind", ["count", "coverage", "nearest"])
def test_strict_wrap_at_the_int32_extremes(ctx, monkeypatch, kind):
    # start == INT32_MAX / end == INT32_MIN: start + 1 and end - 1 wrap as the reference's release build does
    t = table("strict_wrap_table")
    ix = build(ctx, kind, t)
    f = check_forms(ix, kind, t, "wrap")
    assert f["nroute_nreg"] > 0
    if kind == "nearest":
        check_nearest1(ctx, monkeypatch, ix, t, t["probes"], "wrap")
        for ovl in (True, False):
            check_nearestk(ctx, ix, t, t["probes"], "wrap", 3, overlap=ovl, strict=True)
    else:
        check_rowval(ctx, monkeypatch, kind, ix, t, t["probes"], "wrap")
    ix.free()


# ====================================================================================== probe launch edges

@pytest.mark.parametrize("kind", ["count", "coverage", "nearest"])
def test_probe_batch_sizes(ctx, monkeypatch, kind):
    t = table("cut_table", 4096)
    ix = build(ctx, kind, t)
    f = check_forms(ix, kind, t, "cut4096")
    assert f["nroute_nreg"] > 0
    for m in rf.BATCH_SIZES:
        probes = tuple(a[:m].copy() for a in t["probes"])
        if kind == "nearest":
            check_nearest1(ctx, monkeypatch, ix, t, probes, f"batch{m}")
        else:
            check_rowval(ctx, monkeypatch, kind, ix, t, probes, f"batch{m}")
    ix.free()


@pytest.mark.parametrize("kind", ["count", "coverage", "nearest"])
def test_probe_rows_already_in_region_order(ctx, monkeypatch, kind):
    # probe rows in (key, start) order through the routed path: nothing moves, the gated in-place kernel answers
    t = table("cut_table", 4096)
    pk, ps, pe = t["probes"]
    o = np.lexsort((ps, pk))
    probes = (pk[o].copy(), ps[o].copy(), pe[o].copy())
    ix = build(ctx, kind, t)
    assert check_forms(ix, kind, t, "cut4096")["nroute_nreg"] > 0
    if kind == "nearest":
        check_nearest1(ctx, monkeypatch, ix, t, probes, "sortedprobes", paths=NEAREST_PATHS[1:])
    else:
        check_rowval(ctx, monkeypatch, kind, ix, t, probes, "sortedprobes", paths=("routed",))
    ix.free()


@pytest.mark.parametrize("batch", ["change_at_64", "one_lane"])
def test_nearest_wavefronts_of_one_key_and_of_two(ctx, monkeypatch, batch):
    # k_probe_nearest1 reads a wavefront's per-key tables through the scalar unit when all its lanes have one key
    t = table("cut_table", 4096)
    ix = build(ctx, "nearest", t)
    check_forms(ix, "nearest", t, "cut4096")
    check_nearest1(ctx, monkeypatch, ix, t, rf.wave_key_batches()[batch], batch, paths=NEAREST_PATHS[:1])
    ix.free()


# ====================================================================================== nearest k

def test_nearest_k_against_the_keys_row_count(ctx):
    t = table("small_nearest_table")
    ix = build(ctx, "nearest", t)
    f = check_forms(ix, "nearest", t, "smallk")
    assert (f["near_words"], f["near_order"]) == (2, rf.FULL)
    rows0 = int((t["bk"] == 0).sum())
    pk, ps, pe = t["probes"]
    for k in (0, 2, rows0, rows0 + 1, 3, 4):                                # (3, 4: key 2's row count and one more)
        for ovl in (True, False):
            for strict in (False, True):
                gb, gp = check_nearestk(ctx, ix, t, t["probes"], "smallk", k, overlap=ovl, strict=strict)
                if k >= rows0 and ovl:
                    assert (gp == 0).sum() == rows0                         # the cursors ran out: every row of the key, once
                    assert sorted(gb[gp == 0].tolist()) == np.flatnonzero(t["bk"] == 0).tolist()
    # every row of key 0 overlaps probe row 0: without overlaps it gets one NULL row
    gb, gp, gd = ctx.nearest(ix, pk[:1], ps[:1], pe[:1], k=rows0, overlap=False)
    assert gb.tolist() == [pyivx.NULL_IDX] and gp.tolist() == [0] and gd.tolist() == [-1]
    for k in (1, rows0):
        wb, wp, _ = orc.nearest(t["bk"], t["bs"], t["be"], pk, ps, pe, k=k)
        gb, gp, gd = ctx.nearest(ix, pk, ps, pe, k=k, distance=False)
        assert gd is None
        _same(gb, wb, ("no distance", k)); _same(gp, wp, ("no distance", k))
    ix.free()
