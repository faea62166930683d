"""-m gpu: the two tails of the binned overlap index build (csrc/ivx_join.hip) make the same index.

The build's tail -- cells, entries, region descriptors -- either sorts every probe region's rows in LDS (k_lbuild_tiles,
k_lbuild_regions) or runs the global counting sort (k_join_count, scan, k_join_scatter).  The device picks: the LDS tail
takes builds of 2^14 .. 2^22 rows whose rows all sit on level 0 and whose layout has at most 1023 regions of at most 8192
cells; IVX_BUILD=global forces the other one.  Every case builds both ways, reads both layouts back through
ivx_index_layout (equal word for word but for the slot that names the tail), and compares the pair multiset of a fill
through the direct probe (binstart / ent) and through the region probe (region descriptors, LDS slices) of both indexes
with the CPU oracle's.  Cases the LDS tail must decline assert that it did, and that the results are still right."""
import contextlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pair_set
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu

IVX_RP_ECAP = 6144                 # ivx_internal.hpp
IVX_RP_HALO = 8                    # ivx_internal.hpp
IVX_MAXREG_WIDE = 1023             # ivx_internal.hpp
LB_MIN_ROWS = 1 << 14              # ivx_join.hip


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def cols(k, s, e):
    return (np.ascontiguousarray(k, np.uint32), np.ascontiguousarray(s, np.int32), np.ascontiguousarray(e, np.int32))


def cat(*sides):
    return tuple(np.concatenate([x[i] for x in sides]) for i in range(3))


def both(ctx, kind, b, nk):
    """the index under the default rule and with the global tail forced, and their layouts"""
    ix = ctx.build(kind, *b, n_keys=nk)
    with env(IVX_BUILD="global"):
        ixg = ctx.build(kind, *b, n_keys=nk)
    lay, layg = ix.layout(), ixg.layout()
    assert layg["lbuild"] == 0, layg
    assert {k: v for k, v in lay.items() if k != "lbuild"} == {k: v for k, v in layg.items() if k != "lbuild"}, (lay, layg)
    return ix, ixg, lay


def check_fill(ctx, ixs, b, p):
    """fill through the direct and the region probe of every index == the oracle's pair multiset"""
    wb, wp = orc.join(*b, *p, threads=4)
    wset = pair_set(wb, wp)
    for ix in ixs:
        for path in ("direct", "regions"):
            with env(IVX_JOIN_PATH=path, IVX_NO_PLAN=1):
                ob, op = ctx.overlap_fill(ix, *p)
            assert len(ob) == len(wb) and (pair_set(ob, op) == wset).all(), path
    return len(wb)


def regions_of(lay, b, nk):
    """(key, origin, first cell, cells, cells of the key) of every probe region (k_join_layout, k_join_regdesc)"""
    sh0, R = lay["sh0"], lay["rcells"]
    out = []
    for k in range(nk):
        st = b[1][b[0] == k].astype(np.int64)
        if not len(st):
            continue
        origin, cells0 = int(st.min()), ((int(st.max()) - int(st.min())) >> sh0) + 1
        out += [(k, origin, rc0, min(R, cells0 - rc0), cells0) for rc0 in range(0, cells0, R)]
    assert len(out) == lay["nreg"], (len(out), lay)
    return out


def uniform_probes(rng, b, nk, n, maxlen=300):
    k = rng.integers(0, nk, n)
    lo, hi = int(b[1].min()) - 1000, int(b[1].max()) + 1000
    s = rng.integers(lo, hi, n)
    return cols(k, s, s + rng.integers(0, maxlen, n))


def test_headline_shape_scaled(ctx):
    """the benchmark's generator, 24 contigs, 60 k build rows of mean length 1000 against 300 k probe rows of 150"""
    b = synth.gen_numpy(60_000, 1000, 24, 0x5EED0000)
    p = synth.gen_numpy(300_000, 150, 24, 0x5EED0001)
    ix, ixg, lay = both(ctx, pyivx.KIND_OVERLAP, b, 24)
    assert lay["lbuild"] == 1 and lay["levrows"] == 1 and lay["slow"] == 0, lay
    assert check_fill(ctx, (ix, ixg), b, p) > 0
    ix.free(); ixg.free()


def test_single_contig(ctx):
    rng = np.random.default_rng(1)
    s = rng.integers(0, 40_000_000, 50_001)                               # (a ragged last tile)
    b = cols(np.zeros(len(s)), s, s + rng.integers(0, 400, len(s)))
    ix, ixg, lay = both(ctx, pyivx.KIND_OVERLAP, b, 1)
    assert lay["lbuild"] == 1, lay
    check_fill(ctx, (ix, ixg), b, uniform_probes(rng, b, 1, 200_000))
    ix.free(); ixg.free()


def test_keys_without_rows(ctx):
    """30 keys of which the first, two in the middle and the last hold no build row; probe rows on all of them"""
    rng = np.random.default_rng(2)
    nk = 30
    used = np.array([k for k in range(nk) if k not in (0, 7, 8, 29)])
    k = rng.choice(used, 40_000)
    s = rng.integers(0, 3_000_000, len(k)) + k.astype(np.int64) * 1000
    b = cols(k, s, s + rng.integers(0, 200, len(k)))
    ix, ixg, lay = both(ctx, pyivx.KIND_OVERLAP, b, nk)
    assert lay["lbuild"] == 1, lay
    check_fill(ctx, (ix, ixg), b, uniform_probes(rng, b, nk, 200_000))
    ix.free(); ixg.free()


def test_rows_on_borders(ctx):
    """build rows that start on the first and the last coordinate of every region, of cells inside it and of each key's
    last cell; probe rows on the same coordinates +- 1"""
    rng = np.random.default_rng(3)
    nk = 3
    k = rng.integers(0, nk, 60_000)
    s = rng.integers(0, 30_000_000, len(k))
    b0 = cols(k, s, s + rng.integers(0, 100, len(k)))
    ix0 = ctx.build(pyivx.KIND_OVERLAP, *b0, n_keys=nk)
    lay0 = ix0.layout()
    ix0.free()
    sh0 = lay0["sh0"]
    xs, ks = [], []
    for key, origin, rc0, nc, cells0 in regions_of(lay0, b0, nk):
        span_end = origin + ((cells0 - 1) << sh0)                         # first coordinate of the key's last cell
        for c in (rc0, rc0 + 1, rc0 + nc // 2, rc0 + nc - 1):
            for x in (origin + (c << sh0), origin + ((c + 1) << sh0) - 1):
                if origin <= x <= int(b0[1][b0[0] == key].max()):         # (inside the key's span: the layout stays as it is)
                    xs.append(x); ks.append(key)
        xs.append(span_end); ks.append(key)
    xs, ks = np.array(xs, np.int64), np.array(ks)
    b = cat(b0, cols(ks, xs, xs + np.arange(len(xs)) % 7))
    ix, ixg, lay = both(ctx, pyivx.KIND_OVERLAP, b, nk)
    assert (lay["sh0"], lay["rcells"], lay["nreg"]) == (sh0, lay0["rcells"], lay0["nreg"]) and lay["lbuild"] == 1, (lay, lay0)
    q = np.concatenate([xs - 1, xs, xs + 1])
    p = cat(cols(np.tile(ks, 3), q, q + 2), uniform_probes(rng, b, nk, 150_000))
    check_fill(ctx, (ix, ixg), b, p)
    ix.free(); ixg.free()


@pytest.mark.parametrize("extra", [0, 1], ids=["slice_6144", "slice_6145"])
def test_region_at_slice_capacity(ctx, extra):
    """200 k rows of length 15, one every 16 coordinates (sh0 = 4, R = 1024 cells), then rows added in region 0 until its
    slice window [0, R + 8) cells holds IVX_RP_ECAP entries, + extra: the lean fill goes off with the one row beyond"""
    n = 200_000
    s = np.arange(n, dtype=np.int64) * 16
    add = IVX_RP_ECAP - int((s < (1024 + IVX_RP_HALO) * 16).sum()) + extra
    s = np.concatenate([s, (np.arange(add) * 7919) % (1024 * 16)])
    b = cols(np.zeros(len(s)), s, s + 15)
    ix, ixg, lay = both(ctx, pyivx.KIND_OVERLAP, b, 1)
    assert lay["sh0"] == 4 and lay["rcells"] == 1024 and lay["slow"] == extra and lay["lbuild"] == 1, lay
    rng = np.random.default_rng(4)
    st = np.concatenate([rng.integers(-100, 40_000, 100_000), rng.integers(-100, 3_300_000, 100_000)])
    check_fill(ctx, (ix, ixg), b, cols(np.zeros(len(st)), st, st + rng.integers(0, 40, len(st))))
    ix.free(); ixg.free()


def test_declines_upper_level_rows(ctx):
    """200 k rows of length 255 every 64 coordinates (sh0 = 8) and one row of length 256, which sits on level 1"""
    s = np.arange(200_000, dtype=np.int64) * 64
    e = s + 255
    s, e = np.append(s, 1_000_000), np.append(e, 1_000_000 + 256)
    b = cols(np.zeros(len(s)), s, e)
    ix, ixg, lay = both(ctx, pyivx.KIND_OVERLAP, b, 1)
    assert lay["sh0"] == 8 and lay["levrows"] & ~1 and lay["lbuild"] == 0, lay
    rng = np.random.default_rng(5)
    check_fill(ctx, (ix, ixg), b, uniform_probes(rng, b, 1, 150_000, maxlen=20))
    ix.free(); ixg.free()


@pytest.mark.parametrize("n", [LB_MIN_ROWS - 1, LB_MIN_ROWS], ids=["below_min_rows", "min_rows"])
def test_declines_small_builds(ctx, n):
    rng = np.random.default_rng(6)
    k = rng.integers(0, 5, n)
    s = rng.integers(0, 2_000_000, n)
    b = cols(k, s, s + rng.integers(0, 100, n))
    ix, ixg, lay = both(ctx, pyivx.KIND_OVERLAP, b, 5)
    assert lay["levrows"] == 1 and lay["lbuild"] == (1 if n >= LB_MIN_ROWS else 0), lay
    check_fill(ctx, (ix, ixg), b, uniform_probes(rng, b, 5, 100_000))
    ix.free(); ixg.free()


@pytest.mark.parametrize("nk", [IVX_MAXREG_WIDE, IVX_MAXREG_WIDE + 1], ids=["regions_1023", "regions_1024"])
def test_declines_many_regions(ctx, nk):
    """nk keys with 30 rows each, every key one region (as test_gpu_region_forms.test_region_and_key_counts)"""
    rng = np.random.default_rng(nk)
    k = np.repeat(np.arange(nk), 30)
    s = k.astype(np.int64) * 10_000 + rng.integers(0, 200, len(k))
    b = cols(k, s, s + rng.integers(0, 16, len(k)))
    ix, ixg, lay = both(ctx, pyivx.KIND_OVERLAP, b, nk)
    assert lay["nreg"] == nk and lay["lbuild"] == (1 if nk <= IVX_MAXREG_WIDE else 0), lay
    m = 40 * nk
    pk = rng.integers(0, nk, m)
    ps = pk.astype(np.int64) * 10_000 + rng.integers(-60, 300, m)
    check_fill(ctx, (ix, ixg), b, cols(pk, ps, ps + rng.integers(0, 40, m)))
    ix.free(); ixg.free()


@pytest.mark.parametrize("kind", [pyivx.KIND_COUNT, pyivx.KIND_COVERAGE], ids=["count", "coverage"])
def test_count_and_coverage_indexes(ctx, kind):
    """the per-row operators build the same index: over the rows (count), over the merged rows (coverage)"""
    rng = np.random.default_rng(7)
    nk = 4
    k = rng.integers(0, nk, 80_000)
    s = rng.integers(0, 60_000_000, len(k))
    b = cols(k, s, s + rng.integers(0, 120, len(k)))                      # (sparse: merging keeps most rows)
    p = uniform_probes(rng, b, nk, 200_000, maxlen=2000)
    ix, ixg, lay = both(ctx, kind, b, nk)
    assert lay["lbuild"] == 1, lay
    fn, ofn = (ctx.count_overlaps, orc.count_overlaps) if kind == pyivx.KIND_COUNT else (ctx.coverage, orc.coverage)
    for strict in (False, True):
        want = ofn(*b, *p, strict=strict, threads=4)
        for x in (ix, ixg):
            for kv in ({}, {"IVX_ROWVAL_PATH": "regions"}):
                with env(**kv):
                    got = fn(x, *p, strict=strict)
                assert (np.asarray(got) == want).all(), (strict, kv)
    ix.free(); ixg.free()


@pytest.mark.parametrize("overlap", [False, True], ids=["build_overlap_off", "build_overlap_on"])
def test_build_overlap(ctx, overlap):
    """device columns; with the build overlap on the tail runs on the second stream beside the probe's routing pass"""
    import torch
    b = synth.gen_numpy(100_000, 1000, 24, 0x5EED0010)
    p = synth.gen_numpy(400_000, 150, 24, 0x5EED0011)
    wset = pair_set(*orc.join(*b, *p, threads=4))
    db = [torch.from_numpy(c.view(np.int32)).cuda() for c in b]
    dp = [torch.from_numpy(c.view(np.int32)).cuda() for c in p]
    ctx.set_build_overlap(overlap)
    try:
        lays = []
        for kv in ({}, {"IVX_BUILD": "global"}):
            for path in ("regions", "direct"):
                with env(**kv):
                    ix = ctx.build(pyivx.KIND_OVERLAP, *db, n_keys=24)
                ob = torch.empty(len(wset), dtype=torch.int32, device="cuda"); op = torch.empty_like(ob)
                with env(IVX_JOIN_PATH=path):
                    gb, gp = ctx.overlap_fill(ix, *dp, out=(ob, op))       # the index's first probe: waits for the tail itself
                ctx.synchronize()
                assert len(gb) == len(wset) and (pair_set(gb.cpu().numpy().view(np.uint32), gp.cpu().numpy().view(np.uint32)) == wset).all(), (kv, path)
                lays.append(ix.layout())
                ix.free()
    finally:
        ctx.set_build_overlap(False)
    assert [x["lbuild"] for x in lays] == [1, 1, 0, 0], lays
    assert all({k: v for k, v in x.items() if k != "lbuild"} == {k: v for k, v in lays[0].items() if k != "lbuild"} for x in lays), lays


@pytest.mark.parametrize("overlap", [False, True], ids=["build_overlap_off", "build_overlap_on"])
@pytest.mark.parametrize("tail", ["default", "global"])
def test_bad_key_id_fails_the_build(ctx, tail, overlap):
    """a key id >= n_keys is IVX_ERR_INVALID from either tail, also when the tail was already queued on the second stream;
    the context builds a good index right after"""
    import torch
    b = list(synth.gen_numpy(100_000, 1000, 24, 0x5EED0020))
    bad = b[0].copy(); bad[77_777] = 24
    good = [torch.from_numpy(c.view(np.int32)).cuda() for c in b]
    dbad = torch.from_numpy(bad.view(np.int32)).cuda()
    p = synth.gen_numpy(100_000, 150, 24, 0x5EED0021)
    ctx.set_build_overlap(overlap)
    try:
        with env(**({"IVX_BUILD": "global"} if tail == "global" else {})):
            with pytest.raises(pyivx.IvxError) as ei:
                ctx.build(pyivx.KIND_OVERLAP, dbad, good[1], good[2], n_keys=24)
            assert ei.value.status == pyivx.ERR_INVALID
            ix = ctx.build(pyivx.KIND_OVERLAP, *good, n_keys=24)
        check_fill(ctx, (ix,), tuple(b), p)
        ctx.synchronize()
        ix.free()
    finally:
        ctx.set_build_overlap(False)
