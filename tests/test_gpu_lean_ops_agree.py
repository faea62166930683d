"""-m gpu: the per-row operators share one walk (k_lean / k_lean_rest / k_probe_rows over RvOp, MarkOp, AggOp and SelOp:
csrc/ivx_rowops.hpp), so on one batch they must agree with each other: count_overlaps, the aggregates' count, the per-row
count of the fill's pairs, where overlap select finds a winner and which, and the build rows the marks name -- on the
region path and on the direct path, each against ONE numpy brute force of the batch.

The batch is shaped for the lean kernel's batch edges: thirteen regions of a lean index receive exactly 1, 63, 64, 65, 255,
256, 257, 511, 512, 513, 8191, 8192 and 8193 rows (a wavefront batch is 64 * 4 rows for aggregates and select, 64 * 8 for
count and marks; a chunk is 8192 rows), and another region holds a handful of rows for the rest list: escapes at the packed
maximum, rows past the slice's halo, an empty row (qe < qs, placed in a gap so that the literal predicate finds nothing
either: count_overlaps defines such a row as 0, the join's predicate does not), and two absent keys."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402
import test_gpu_region_forms as rf  # noqa: E402

pytestmark = pytest.mark.gpu

env, cols = rf.env, rf.cols
ROWS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 8191, 8192, 8193)
PATHS = ("regions", "direct")


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def brute_pairs(b, p):
    """every (probe row, build row) of equal key with bs <= qe and be >= qs.  The literal predicate is tested on every build
    row that starts in [qs - L, qe], L the longest build row: a row that starts behind qe fails the first clause, one that
    starts before qs - L ends before qs.  (Build rows: one key, in start order.)"""
    assert (b[0] == 0).all() and (np.diff(b[1]) >= 0).all()
    bs, be = b[1].astype(np.int64), b[2].astype(np.int64)
    qs, qe = p[1].astype(np.int64), p[2].astype(np.int64)
    lo = np.searchsorted(bs, qs - int((be - bs).max()), "left")
    cnt = np.maximum(np.searchsorted(bs, qe, "right"), lo) - lo
    pi = np.repeat(np.arange(len(qs)), cnt)
    bi = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
    ok = (p[0][pi] == 0) & (bs[bi] <= qe[pi]) & (be[bi] >= qs[pi])
    return pi[ok], bi[ok]


def batch(lay, geo, b):
    """-> probe columns, the regions that hold ROWS rows each, the number of rest-list rows"""
    rng = np.random.default_rng(60)
    full = [i for i, r in enumerate(geo["regs"]) if r["rc1"] + rf.IVX_RP_HALO <= r["shi"]]      # regions with a whole halo
    chosen, rest_reg = full[2:2 + len(ROWS)], full[2 + len(ROWS) + 3]
    ks, ss, es = [], [], []
    for i, n in zip(chosen, ROWS):
        r = geo["regs"][i]
        # a third each: points on build rows, points in the gaps, ranges well inside the halo (0 to 3 matches)
        x = rng.integers(r["rbase"], r["rend"], n)
        kind = rng.integers(0, 3, n)
        x = np.where(kind == 0, (x // 512) * 512 + rng.integers(0, 256, n), np.where(kind == 1, (x // 512) * 512 + rng.integers(256, 512, n), x))
        ks.append(np.zeros(n)); ss.append(x); es.append(x + np.where(kind == 2, rng.integers(0, 1000, n), 0))
    n_rest = 2 + 4 + 1 + 2
    n = sum(ROWS) + n_rest
    f = rf.probe_form(lay, n, 1, {"IVX_JOIN_PATH": "regions"}, mode="exists")
    assert f["packed"] and f["maxlen"] == 65535, f
    r = geo["regs"][rest_reg]
    x0 = r["rbase"] + 1000
    halo = rf.halo_probes(dict(regs=[r]), lay["sh0"], True)                                       # four rows, one coordinate past the halo
    gap = (x0 // 512) * 512 + 300                                                                 # (build rows cover [512 i, 512 i + 255])
    rest = rf.cat(cols([0, 0], [x0, x0 + 7], [x0 + f["maxlen"], x0 + 7 + f["maxlen"] - 1]),       # the length field's escape value, and one below
                  halo, cols([0], [gap], [gap - 10]),                                             # qe < qs
                  cols([1, 9], [x0, x0], [x0 + 100, x0 + 100]))                                   # a key without build rows, a key the index lacks
    assert len(rest[0]) == n_rest
    p = rf.cat(cols(np.concatenate(ks), np.concatenate(ss), np.concatenate(es)), rest)
    order = rng.permutation(n)
    return tuple(c[order] for c in p), chosen, n_rest


@pytest.fixture(scope="module")
def side():
    ctx = pyivx.Ctx(0)
    b = rf.sparse_build()
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=2)                      # (key 1: no build rows)
    cix = ctx.build(pyivx.KIND_COUNT, *b, n_keys=2)
    lay, geo = rf.layout_of(ix, *b, 2)
    assert lay["slow"] == 0 and lay["pk24"] == 1 and 1 < lay["nreg"] <= rf.IVX_MAXREG, lay
    clay = cix.layout()
    assert {s: clay[s] for s in rf.LAYOUT_SHAPE} == {s: lay[s] for s in rf.LAYOUT_SHAPE}, (clay, lay)
    p, chosen, n_rest = batch(lay, geo, b)
    reg = rf.route_region(lay, b, p)
    assert ((reg < 0) == (p[0] != 0)).all()                              # (only the two absent keys are not routed)
    per_reg = np.bincount(reg[reg >= 0], minlength=lay["nreg"])
    assert tuple(per_reg[chosen]) == ROWS and per_reg.sum() == sum(ROWS) + n_rest - 2, per_reg[chosen]
    n, nb = len(p[1]), len(b[1])
    pi, bi = brute_pairs(b, p)
    count = np.bincount(pi, minlength=n)
    assert min((count == c).sum() for c in (0, 1, 2)) > 1000 and count.max() > 100            # (the escapes: 128 matches)
    val = (np.random.default_rng(61).permutation(nb).astype(np.int64) * 3 - nb).astype(np.int32)  # distinct: one winner per row
    first = np.full(n, pyivx.NULL_IDX, np.int64); np.minimum.at(first, pi, bi)
    by_val = np.lexsort((-val[bi].astype(np.int64), pi))                   # per probe row, the largest value first
    head = by_val[np.concatenate([[True], pi[by_val][1:] != pi[by_val][:-1]])]
    maxv = np.full(n, pyivx.NULL_IDX, np.int64); maxv[pi[head]] = bi[head]
    marked = np.zeros(nb, bool); marked[bi] = True
    want = dict(count=count, first=first, maxv=maxv, marked=marked)
    yield ctx, ix, cix, b, p, val, want
    ix.free(); cix.free(); ctx.close()


def bits(words, nb):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:nb].astype(bool)


@pytest.mark.parametrize("path", PATHS)
def test_lean_ops_agree(side, path):
    ctx, ix, cix, b, p, val, want = side
    n, nb, count = len(p[1]), len(b[1]), want["count"]
    with env(IVX_JOIN_PATH=path, IVX_ROWVAL_PATH=path):
        co = np.asarray(ctx.count_overlaps(cix, *p))
        _, per_row = ctx.overlap_count(ix, *p, per_row=True)
        a = ctx.overlap_agg(ix, *p, val, outputs=("count", "sum"))
        ob, op = ctx.overlap_fill(ix, *p)
        first, _ = ctx.overlap_select(ix, *p, by="first_row", score=False)
        maxv, score = ctx.overlap_select(ix, *p, by="max_val", val=val)
        marks = ctx.mark_build(ix, *p, ctx.new_marks(nb))
    assert (co == count).all(), np.flatnonzero(co != count)[:5]
    assert (a["count"] == count).all(), np.flatnonzero(a["count"] != count)[:5]
    assert (per_row[:n] == count).all()
    assert len(op) == count.sum() and (np.bincount(op, minlength=n) == count).all()
    for got, w in ((first, want["first"]), (maxv, want["maxv"])):
        assert ((got == pyivx.NULL_IDX) == (count == 0)).all()
        assert (got == w).all(), np.flatnonzero(got != w)[:5]
    hit = count > 0
    assert (score[hit] == val[maxv[hit]]).all() and (score[~hit] == 0).all()
    named = np.zeros(nb, bool); named[ob] = True
    assert (bits(marks, nb) == named).all() and (named == want["marked"]).all()


@pytest.mark.parametrize("op", ["count_overlaps", "agg", "select", "marks"])
def test_lean_ops_region_run_takes_scratch(side, op):
    """the region run routes the rows into scratch pages (so the lean kernels ran); the direct kernels need none"""
    _, ix, cix, b, p, val, _ = side
    d = [dev(c) for c in p]
    call = {"count_overlaps": lambda c: c.count_overlaps(cix, *d),
            "agg": lambda c: c.overlap_agg(ix, *d, dev(val), outputs=("count", "sum")),
            "select": lambda c: c.overlap_select(ix, *d, by="max_val", val=dev(val)),
            "marks": lambda c: c.mark_build(ix, *d, c.new_marks(len(b[1]), device="cuda"))}[op]
    took = {}
    for path in PATHS:
        c = pyivx.Ctx(0)
        try:
            with env(IVX_JOIN_PATH=path, IVX_ROWVAL_PATH=path):
                call(c)
            c.synchronize()
            took[path] = c.reserved_bytes()
        finally:
            c.close()
    assert took["regions"] > 0, took
    if op != "count_overlaps":                                          # (a COUNT index answers the direct call from its rank grids)
        assert took["direct"] == 0, took
