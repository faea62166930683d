"""-m gpu: the overlap join's region pipeline at each of the thresholds that pick its form.

The binned overlap index (csrc/ivx_join.hip) picks its layout on the device: the level-0 cell shift sh0, the cells per
probe region R (a power of two, or any integer divided by multiplication), the packed 8-byte routed rows (pk24), the lean
fill (off for the whole index when one row sits above level 0 or one slice outgrows IVX_RP_ECAP), the occupancy bitmap and
the region count.  The probe (csrc/ivx_regions_probe.hip) picks its own form from n and cap: rows-per-lane bands, dense
fill, the length field of packed rows, partition tiles, page size.  Every case below sits on one named side of one of
those thresholds; it reads the index's form back through ivx_index_layout, restates the host rules (region_geometry,
probe_form) and asserts the side it reaches before it compares bit-exactly with the CPU oracle, under the default settings
and under each knob that turns the form off.

Untested: the fallback from a non-power-of-two R to a power of two when cells * R would reach 2^40 (k_join_layout,
`s_mc * R >= 2^40`).  By the cell budget (2n + nkeys cells) it needs on the order of 2^27 build rows."""
import contextlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pair_set
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

IVX_RP_ECAP = 6144                 # ivx_internal.hpp
IVX_RP_HALO = 8                    # ivx_internal.hpp
IVX_MAXREG, IVX_MAXREG_WIDE = 255, 1023
KT_MAX = 256                       # ivx_regions_route.hip
FP_CHUNK = 8192                    # ivx_regions.hpp (RP_W * IVX_WAVE * 8)
NOFG = 0xFFFFFFFF

# knobs that turn a form off, applied to the probe calls (IVX_FILTER=force is a build-time knob: a second index)
KNOBS = {"default": {}, "fill_old": {"IVX_FILL": "old"}, "pack0": {"IVX_PACK": "0"}, "part_two": {"IVX_PART": "two"},
         "filter0": {"IVX_FILTER": "0"}, "dense0": {"IVX_DENSE": "0"}, "dense1": {"IVX_DENSE": "1"}}
FEW = ("default", "fill_old", "pack0")


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


# ---------------------------------------------------------------- the host decisions, restated

def region_geometry(layout, key, s, e, n_keys):
    """Every probe region of the index these build rows make, from the inputs and the layout's sh0 / R.
    Python ints throughout.  Each rule cites the line of csrc/ivx_join.hip it mirrors."""
    sh0, R = layout["sh0"], layout["rcells"]
    s64, e64 = s.astype(np.int64), e.astype(np.int64)
    kmin = np.full(n_keys, 2**31, np.int64); kmax = np.full(n_keys, -2**31 - 1, np.int64)
    np.minimum.at(kmin, key, s64); np.maximum.at(kmax, key, s64)
    kcnt = np.bincount(key, minlength=n_keys)
    lvl0 = (e64 - s64) < (1 << sh0)                                       # level_of (ivx_join.hpp:5): len < 2^sh0
    regs, kreg = [], []
    for k in range(n_keys):
        kreg.append(len(regs))
        if not kcnt[k] or not R:
            continue
        origin, span = int(kmin[k]), int(kmax[k] - kmin[k])               # k_join_layout :47-48
        cells0 = (span >> sh0) + 1                                        # cells_of :34
        cell = (s64[(key == k) & lvl0] - origin) >> sh0                   # cell_of (ivx_join.hpp:14)
        for rc0 in range(0, cells0, R):                                   # ceil(cells / R) regions per key :223
            rc1 = min(rc0 + R, cells0)                                    # k_join_regdesc :275
            slo = rc0 - 1 if rc0 else 0                                   # :276
            shi = min(rc1 + IVX_RP_HALO, cells0)                          # :277 (exclusive)
            regs.append(dict(k=k, origin=origin, rc0=rc0, rc1=rc1, slo=slo, shi=shi,
                             rbase=origin + (rc0 << sh0), rend=origin + (rc0 + R << sh0),   # :280
                             ne=int(((cell >= slo) & (cell < shi)).sum())))               # :279
    return dict(nreg=len(regs), regs=regs, kreg=kreg, max_ne=max([r["ne"] for r in regs], default=0))


def probe_form(layout, n, cap, env_=None, mode="fill"):
    """The form ivx_probe_overlap_* takes for a batch of n rows with pair buffers of cap (ivx_capi.hip overlap_common,
    ivx_regions_probe.hip ivx_join_probe_regions).  env_: the IVX_* settings of the call."""
    env_ = env_ or {}
    nreg = layout["nreg"]
    f = {}
    path = env_.get("IVX_JOIN_PATH")
    regions = nreg > 0 and n >= (1 << 21)                                 # overlap_common: measured crossover
    if path == "direct":
        regions = False
    elif path == "regions":
        regions = nreg > 0
    if mode in ("per_row", "exists"):
        regions = regions and nreg <= IVX_MAXREG_WIDE                     # rowval: one partition pass only
    f["path"] = "regions" if regions else "direct"
    if not regions:
        return f
    f["routing"] = "two-level" if nreg > IVX_MAXREG_WIDE else "1024" if nreg > IVX_MAXREG else "256"
    f["klds"] = layout["nkeys"] <= KT_MAX
    two_pass = env_.get("IVX_PART") == "two"
    pack_off = env_.get("IVX_PACK") == "0"
    use_filter = layout["fg"] != NOFG and env_.get("IVX_FILTER") != "0"
    onepass = f["routing"] != "two-level" and not two_pass and not (mode in ("per_row", "exists") and pack_off)
    f["onepass"] = onepass
    f["packed"] = onepass and bool(layout["pk24"]) and not pack_off
    rowbits = 1
    while rowbits < 32 and (n - 1) >> rowbits:                            # ivx_join_probe_regions: bits of the largest row id
        rowbits += 1
    if use_filter and onepass:
        rowbits = 32                                                      # (see pk_maxlen)
    f["rowbits"] = rowbits
    spare = 0 if rowbits >= 32 else 32 - rowbits
    f["maxlen"] = (1 << (8 + min(spare, 8))) - 1                          # pk_maxlen
    lgpg = 14
    while lgpg < 31 and (n >> lgpg) > 4096:
        lgpg += 1
    f["lgpg"] = lgpg
    f["part_tiles"] = 4 if n >= (16 << 20) else 2 if n >= (4 << 20) else 1
    f["filter"] = use_filter and onepass
    if mode == "fill":
        dn = env_.get("IVX_DENSE")
        f["dense"] = (int(dn) != 0) if dn is not None else cap / n > 3.5  # dense_fill_wanted
        rp = env_.get("IVX_RP_ROWS")
        per_row = cap / n
        f["rows_per_lane"] = int(rp) if rp else 8 if per_row <= 0.40 else 4 if per_row <= 0.8 else 2 if per_row <= 1.6 else 1
        if f["filter"]:
            f["rows_per_lane"] = "device"                                 # k_pick_rows: from the routed rows
        f["lean"] = (not f["dense"] and f["packed"] and not layout["slow"] and env_.get("IVX_FILL") != "old" and lgpg >= 13)
    return f


def layout_of(ix, key, s, e, n_keys):
    lay = ix.layout()
    lay["nkeys"] = n_keys
    geo = region_geometry(lay, key, s, e, n_keys)
    assert geo["nreg"] == lay["nreg"], (lay, geo["nreg"])               # the restatement agrees with the device
    return lay, geo


def key_tables(b, n_keys):
    bk, bs = b[0], b[1].astype(np.int64)
    kmin = np.full(n_keys, 2**31, np.int64); kmax = np.full(n_keys, -2**31 - 1, np.int64)
    np.minimum.at(kmin, bk, bs); np.maximum.at(kmax, bk, bs)
    return kmin, kmax - kmin, np.bincount(bk, minlength=n_keys)


def bitmap_pass(lay, b, p):
    """rows the occupancy bitmap lets through (k_join_filter, route_prep FILT): a set bit in the blocks
    [block(max(qs, origin)), block(qe)], or more than 32 blocks (routed without a test)"""
    nk, g = lay["nkeys"], lay["fg"]
    origin, span, kcnt = key_tables(b, nk)
    bk, bs, be = b[0], b[1].astype(np.int64), b[2].astype(np.int64)
    pk, ps, pe = p[0].astype(np.int64), p[1].astype(np.int64), p[2].astype(np.int64)
    out = np.zeros(len(ps), bool)
    for k in range(nk):
        if not kcnt[k]:
            continue
        o, last = int(origin[k]), (int(span[k]) >> g) + 1                # the overflow block
        sel = bk == k
        b0 = (bs[sel] - o) >> g
        b1 = np.minimum((np.maximum(be[sel], bs[sel]) - o) >> g, last)
        diff = np.zeros(last + 2, np.int64)
        np.add.at(diff, b0, 1); np.add.at(diff, b1 + 1, -1)
        setb = np.concatenate([[0], np.cumsum((np.cumsum(diff)[:last + 1] > 0).astype(np.int64))])   # set blocks before x
        q = np.nonzero(pk == k)[0]
        d, h = ps[q] - o, pe[q] - o
        c0 = np.minimum(np.where(d >= 0, d >> g, 0), last); c1 = np.minimum(np.where(h >= 0, h >> g, 0), last)
        lo, hi = np.minimum(c0, c1), np.maximum(c0, c1)
        out[q] = (h >= 0) & ((hi - lo > 31) | (setb[hi + 1] - setb[lo] > 0))
    return out


def route_region(lay, b, p):
    """the region each probe row is routed to (route_prep: the cell of its start, clamped to the key's span), -1 if none"""
    nk, sh0, R = lay["nkeys"], lay["sh0"], lay["rcells"]
    origin, span, kcnt = key_tables(b, nk)
    kreg = np.concatenate([[0], np.cumsum(np.where(kcnt > 0, ((span >> sh0) + 1 + R - 1) // R, 0))])
    pk, ps, pe = p[0].astype(np.int64), p[1].astype(np.int64), p[2].astype(np.int64)
    ok = pk < nk
    k = np.where(ok, pk, 0)
    ok &= (kcnt[k] > 0) & (pe >= origin[k])
    d = ps - origin[k]
    c = np.minimum(np.where(d >= 0, d >> sh0, 0), span[k] >> sh0)
    reg = np.where(ok, kreg[k] + c // R, -1)
    if lay["fg"] != NOFG:
        reg = np.where(bitmap_pass(lay, b, p), reg, -1)
    return reg


def assert_lean_walks(lay, b, p, cnt, cap, env_):
    """The fill with pair buffers of `cap` (what check_join passes) runs the lean kernel, and every batch of B rows per
    lane that k_fill_fast can form from a region's rows stages at most HALF = 256 pairs, whatever their order inside the
    region (the 64 * B largest counts of the region's rows): no batch is handed whole to k_fill_rest by `got > HALF`, so
    the kernel's own per-row decisions (escape length, halo) are what the comparison tests."""
    n = len(p[1])
    f = probe_form(lay, n, cap, env_)
    assert f["lean"], f
    reg = route_region(lay, b, p)
    B = f["rows_per_lane"]
    if B == "device":                                                    # k_pick_rows: pairs per ROUTED row, in float
        pr = np.float32(cap / max(int((reg >= 0).sum()), 1))
        B = 8 if pr <= np.float32(0.40) else 4 if pr <= np.float32(0.8) else 2 if pr <= np.float32(1.6) else 1
    cnt = np.asarray(cnt).astype(np.int64)
    order = np.lexsort((-cnt, reg))
    rs, cs = reg[order], cnt[order]
    starts = np.searchsorted(rs, np.unique(rs[rs >= 0]))
    for s0 in starts:
        r = rs[s0]
        s1 = np.searchsorted(rs, r, side="right")
        assert cs[s0:min(s1, s0 + 64 * B)].sum() <= 256, (int(r), B, f)
    return f, B


# ---------------------------------------------------------------- the comparisons

def check_join(ctx, ix, b, p, knobs=tuple(KNOBS), path="regions", ixf=None, want=None):
    """pairs (count-planned and unplanned fill), count, per-row counts and exists vs the oracle, under every knob"""
    (bk, bs, be), (pk, ps, pe) = b, p
    if want is None:
        want = orc.join(bk, bs, be, pk, ps, pe, per_row=True, threads=4)
    wb, wp, wcnt = want
    wset = pair_set(wb, wp)
    runs = [(name, ix, KNOBS[name]) for name in knobs]
    if ixf is not None:
        runs.append(("filter_force", ixf, {}))
    for name, x, kv in runs:
        extra = {"IVX_JOIN_PATH": path} if path else {}
        with env(**extra, **kv):
            total = ctx.overlap_count(x, pk, ps, pe)
            ob, op = ctx.overlap_fill(x, pk, ps, pe, cap=total)           # planned by the count call
            with env(IVX_NO_PLAN=1):
                ob2, op2 = ctx.overlap_fill(x, pk, ps, pe, cap=total)
            t2, pr = ctx.overlap_count(x, pk, ps, pe, per_row=True)
            ex = ctx.exists(x, pk, ps, pe)
        assert total == len(wb), name
        assert len(ob) == total and (pair_set(ob, op) == wset).all(), name
        assert len(ob2) == total and (pair_set(ob2, op2) == wset).all(), name
        assert t2 == total and (pr.astype(np.uint64) == wcnt).all(), name
        assert (ex == (wcnt > 0)).all(), name
    return want


def merged_nodes(b, nk):
    """what a COVERAGE index builds its overlap index over: every key's rows merged (first <= current.last)"""
    ks, ss, es = [], [], []
    for k in range(nk):
        sel = b[0] == k
        if sel.any():
            ms, me = orc.merge_intervals(b[1][sel].astype(np.int64), b[2][sel].astype(np.int64))
            ks.append(np.full(len(ms), k)); ss.append(ms); es.append(me)
    return cols(np.concatenate(ks), np.concatenate(ss), np.concatenate(es))


LAYOUT_SHAPE = ("sh0", "nlev", "levrows", "rcells", "rcs", "nreg", "pk24", "slow", "fg", "fbits")


def check_rowval(ctx, kind, b, p, knobs=FEW, overlap_layout=None):
    """the same build rows as a COUNT / COVERAGE index, strict both ways, through the region partition.  The index's
    readout: a COUNT index lays its rows out as the OVERLAP index of the same rows does; a COVERAGE index as the regions
    of its merged nodes make it (region_geometry)."""
    (bk, bs, be), (pk, ps, pe) = b, p
    nk = int(max(bk.max(), pk.max())) + 1
    ix = ctx.build(kind, bk, bs, be, n_keys=nk)
    lay = ix.layout()
    assert lay["kind"] == kind, lay
    if kind == pyivx.KIND_COUNT and overlap_layout is not None:
        assert {s: lay[s] for s in LAYOUT_SHAPE} == {s: overlap_layout[s] for s in LAYOUT_SHAPE}, (lay, overlap_layout)
    if kind == pyivx.KIND_COVERAGE:
        lay["nkeys"] = nk
        assert region_geometry(lay, *merged_nodes(b, nk), nk)["nreg"] == lay["nreg"], lay
    fn, ofn = (ctx.count_overlaps, orc.count_overlaps) if kind == pyivx.KIND_COUNT else (ctx.coverage, orc.coverage)
    for strict in (False, True):
        want = ofn(bk, bs, be, pk, ps, pe, strict=strict, threads=4)
        for name in knobs:
            with env(IVX_ROWVAL_PATH="regions", **KNOBS[name]):
                got = fn(ix, pk, ps, pe, strict=strict)
            assert (np.asarray(got) == want).all(), (kind, strict, name)
    ix.free()
    return lay


def check_rowvals(ctx, b, p, overlap_layout, knobs=FEW):
    check_rowval(ctx, pyivx.KIND_COUNT, b, p, knobs, overlap_layout)
    check_rowval(ctx, pyivx.KIND_COVERAGE, b, p, knobs)


def build2(ctx, b, nk):
    """the index under the default rule, and one that carries the occupancy bitmap whatever the density"""
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=nk)
    with env(IVX_FILTER="force"):
        ixf = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=nk)
    return ix, ixf


def edge_probes(geo, sh0, rng, n_rand, lo, hi, maxlen=300):
    """every region's first and last coordinate +-1, rows ending in the last halo cell and one past it, plus random rows"""
    qs, qe, qk = [], [], []
    for r in geo["regs"]:
        for x in (r["rbase"] - 1, r["rbase"], r["rbase"] + 1, r["rend"] - 2, r["rend"] - 1, r["rend"]):
            for ln in (0, 1, (1 << sh0) - 1):
                qs.append(x); qe.append(x + ln); qk.append(r["k"])
    ks = rng.integers(0, max(len(geo["kreg"]), 1), n_rand)
    st = rng.integers(lo, hi, n_rand)
    qs += st.tolist(); qe += (st + rng.integers(0, maxlen, n_rand)).tolist(); qk += ks.tolist()
    qs, qe = np.clip(np.array(qs, np.int64), -2**31 + 2, 2**31 - 3), np.clip(np.array(qe, np.int64), -2**31 + 2, 2**31 - 3)
    return cols(qk, qs, qe)


def halo_probes(geo, sh0, past):
    """from each region's last coordinate to the last coordinate of its last halo cell (past: one coordinate further)"""
    qs, qe, qk = [], [], []
    for r in geo["regs"]:
        if r["rc1"] + IVX_RP_HALO > r["shi"]:
            continue                                                      # (a key's last region: no full halo)
        last = r["origin"] + (r["rc1"] << sh0) - 1
        end = r["origin"] + ((r["rc1"] + IVX_RP_HALO) << sh0) - 1 + (1 if past else 0)
        for d in range(4):
            qs.append(last - d); qe.append(end); qk.append(r["k"])
    return cols(qk, qs, qe)


def cat(*sides):
    return tuple(np.concatenate([x[i] for x in sides]) for i in range(3))


# ---------------------------------------------------------------- index side

def level0_build(extra_level1):
    """200 k rows of length 255 every 20 coordinates: sh0 = 8 (2^8 - 1 is the longest level-0 length), 12.8 rows per
    cell; extra_level1 adds one row of length 256, which the cost model keeps in level 1 (moving sh0 up costs more)"""
    n = 200_000
    s = np.arange(n, dtype=np.int64) * 20
    e = s + 255
    if extra_level1:
        s = np.append(s, 1_000_000); e = np.append(e, 1_000_000 + 256)
    return cols(np.zeros(len(s)), s, e)


@pytest.fixture(scope="module")
def pow2_side(ctx):
    b = level0_build(False)
    ix, ixf = build2(ctx, b, 1)
    lay, geo = layout_of(ix, *b, 1)
    yield b, ix, ixf, lay, geo
    ix.free(); ixf.free()


def level0_lean_build(extra_level1):
    """200 k rows of length 255 every 64 coordinates: sh0 = 8, 4 rows per level-0 cell.  extra_level1 adds one row of
    length 256; at this occupancy the cost model keeps it in level 1 (sh0 = 9 would cost 1 + 2.2 * 8 against
    1 + 2.2 * 4 + 8 for the extra level), so the lean fill goes off for the whole index"""
    n = 200_000
    s = np.arange(n, dtype=np.int64) * 64
    e = s + 255
    if extra_level1:
        s = np.append(s, 1_000_000); e = np.append(e, 1_000_000 + 256)
    return cols(np.zeros(len(s)), s, e)


def points(rng, n, lo, hi, unknown=0.0):
    """point probes in [lo, hi); a fraction `unknown` of them on a key the index does not have (key 1)"""
    x = rng.integers(lo, hi, n)
    return cols((rng.random(n) < unknown).astype(np.uint32), x, x)


@pytest.mark.parametrize("side", ["level0_rows_only", "level0_plus_one_level1_row"])
def test_level0(ctx, side):
    """point probes match exactly 4 rows each inside the span: with a third of the rows on an unknown key the fill takes
    one row per lane (1.6 < pairs per row <= 3.5), and 64 rows stage at most 256 pairs, so k_fill_fast walks every batch"""
    import torch
    b = level0_lean_build(side != "level0_rows_only")
    ix, ixf = build2(ctx, b, 1)
    lay, geo = layout_of(ix, *b, 1)
    assert lay["sh0"] == 8 and lay["rcs"] != NOFG and lay["fg"] == NOFG, lay
    if side == "level0_rows_only":
        assert lay["slow"] == 0 and lay["levrows"] == 1, lay
    else:
        assert lay["slow"] == 1 and lay["levrows"] & ~1, lay
    # the same build from device columns with the build overlap on: the readout waits for the tail that sets `slow`
    ctx.set_build_overlap(True)
    try:
        dcols = [torch.from_numpy(c.view(np.int32)).cuda() for c in b]
        ixo = ctx.build(pyivx.KIND_OVERLAP, *dcols, n_keys=1)
        lay_o = ixo.layout()
        ctx.synchronize()
        ixo.free()
    finally:
        ctx.set_build_overlap(False)
    assert {s: lay_o[s] for s in LAYOUT_SHAPE} == {s: lay[s] for s in LAYOUT_SHAPE}, (lay_o, lay)
    rng = np.random.default_rng(1)
    p = points(rng, 150_000, 0, int(b[1].max()), unknown=1 / 3)
    want = orc.join(*b, *p, per_row=True, threads=4)
    env_ = {"IVX_JOIN_PATH": "regions"}
    if side == "level0_rows_only":
        assert want[2].max() <= 4                                          # (the level-1 row adds a fifth near it)
        f, B = assert_lean_walks(lay, b, p, want[2], len(want[0]), env_)
        assert B == 1, f
    else:
        assert not probe_form(lay, len(p[1]), len(want[0]), env_)["lean"]
    check_join(ctx, ix, b, p, ixf=ixf, want=want)
    check_rowvals(ctx, b, p, lay)
    ix.free(); ixf.free()


def slice_build(extra):
    """200 k rows of length 15, one every 16 coordinates (sh0 = 4, R = 1024 cells, a power of two), then rows added in
    region 0 until its slice window [0, R + 8) cells holds 6144 level-0 entries, + extra"""
    n = 200_000
    s = np.arange(n, dtype=np.int64) * 16
    base = int((s < (1024 + IVX_RP_HALO) * 16).sum())
    add = IVX_RP_ECAP - base + extra
    s = np.concatenate([s, (np.arange(add) * 7919) % (1024 * 16)])
    return cols(np.zeros(len(s)), s, s + 15)


@pytest.mark.parametrize("side", ["slice_6144", "slice_6145"])
def test_slice_capacity(ctx, side):
    b = slice_build(0 if side == "slice_6144" else 1)
    ix, ixf = build2(ctx, b, 1)
    lay, geo = layout_of(ix, *b, 1)
    assert lay["sh0"] == 4 and lay["rcells"] == 1024 and lay["levrows"] == 1, lay
    assert geo["max_ne"] == (IVX_RP_ECAP if side == "slice_6144" else IVX_RP_ECAP + 1) and geo["regs"][0]["ne"] == geo["max_ne"]
    assert lay["slow"] == (0 if side == "slice_6144" else 1), lay
    rng = np.random.default_rng(2)
    p = edge_probes(geo, 4, rng, 100_000, -100, 3_300_000, maxlen=40)
    check_join(ctx, ix, b, p, ixf=ixf)
    check_rowvals(ctx, b, p, lay)
    ix.free(); ixf.free()


def dense_build():
    """800 k point rows over 132096 coordinates (8256 cells of 16, ~97 rows each): the power of two that fits 255
    regions (64 cells) would overfill the LDS slice, so R = floor(0.85 * 6144 / occupancy), not a power of two"""
    n = 800_000
    s = np.arange(n, dtype=np.int64) * 132_096 // n
    return cols(np.zeros(n), s, s)


@pytest.mark.parametrize("side", ["region_width_pow2", "region_width_non_pow2"])
def test_region_width(ctx, side, pow2_side):
    if side == "region_width_pow2":
        b0 = pow2_side[0]
        sh_ln = 255
    else:
        b0 = dense_build()
        sh_ln = 15
    ix0 = ctx.build(pyivx.KIND_OVERLAP, *b0, n_keys=1)
    lay0, geo0 = layout_of(ix0, *b0, 1)
    ix0.free()
    sh0 = lay0["sh0"]
    # build rows that start one cell before each region and reach into it, and rows in each region's last halo cell
    add_s = []
    for r in geo0["regs"]:
        if r["rc0"]:
            add_s.append(r["rbase"] - (1 << sh0) + 3)
        if r["rc1"] + IVX_RP_HALO <= r["shi"]:
            add_s.append(r["origin"] + ((r["rc1"] + IVX_RP_HALO - 1) << sh0) + 1)
    add_s = np.array(add_s, np.int64)
    b = cat(b0, cols(np.zeros(len(add_s)), add_s, add_s + min(sh_ln, (1 << sh0) - 1)))
    ix, ixf = build2(ctx, b, 1)
    lay, geo = layout_of(ix, *b, 1)
    assert (lay["sh0"], lay["rcells"]) == (sh0, lay0["rcells"]), (lay, lay0)
    if side == "region_width_pow2":
        assert lay["rcs"] != NOFG and (1 << lay["rcs"]) == lay["rcells"], lay
    else:
        assert lay["rcs"] == NOFG and lay["rcells"] & (lay["rcells"] - 1), lay
        assert lay["nreg"] <= IVX_MAXREG, lay
    assert lay["slow"] == 0, lay
    rng = np.random.default_rng(3)
    hi = int(b[1].max()) + 1000
    p = edge_probes(geo, sh0, rng, 100_000, -100, hi, maxlen=(1 << sh0) if side != "region_width_pow2" else 300)
    if side == "region_width_non_pow2":
        p = (p[0], p[1], np.minimum(p[2].astype(np.int64), p[1].astype(np.int64) + 3).astype(np.int32))   # (~6 pairs per point)
    check_join(ctx, ix, b, p, ixf=ixf)
    check_rowvals(ctx, b, p, lay)
    ix.free(); ixf.free()


def sparse_build():
    """200 k rows of length 255 every 512 coordinates: sh0 = 8 (the cell budget allows no coarser grid to be cheaper),
    R = 2048 cells, a power of two, half a row per cell.  A point matches at most one row, a row up to 256 long two."""
    n = 200_000
    s = np.arange(n, dtype=np.int64) * 512
    return cols(np.zeros(n), s, s + 255)


@pytest.fixture(scope="module")
def sparse_side(ctx):
    b = sparse_build()
    ix, ixf = build2(ctx, b, 1)
    lay, geo = layout_of(ix, *b, 1)
    assert (lay["sh0"], lay["rcells"], lay["slow"], lay["pk24"], lay["fg"]) == (8, 2048, 0, 1, NOFG), lay
    layf = ixf.layout(); layf["nkeys"] = 1
    assert layf["fg"] != NOFG and {s: layf[s] for s in ("sh0", "rcells", "nreg", "slow")} == {s: lay[s] for s in ("sh0", "rcells", "nreg", "slow")}, layf
    yield b, ix, ixf, lay, layf, geo
    ix.free(); ixf.free()


def region_points(rng, b, r, hits, misses):
    """points inside region r: `hits` on build rows (one pair each), `misses` in the gaps between them (none)"""
    i = np.arange((r["rbase"] + 511) // 512, r["rend"] // 512)
    i = i[i < len(b[1])]
    on = rng.choice(i, hits) * 512 + rng.integers(0, 256, hits)
    off = rng.choice(i, misses) * 512 + rng.integers(256, 512, misses)
    return np.concatenate([on, off])


@pytest.mark.parametrize("side", ["halo_last_cell", "halo_one_past"])
def test_halo(ctx, side, sparse_side):
    """four rows per region from its last coordinate into the last halo cell (or one coordinate past it) among 200
    points that match one row and 200 that match none: every batch k_fill_fast forms stages at most 256 pairs, so each
    halo row reaches the kernel's own halo test (`bh >= ncm1`), and only the rows past the halo go to k_fill_rest"""
    b, ix, ixf, lay, layf, geo = sparse_side
    rng = np.random.default_rng(4)
    hp = halo_probes(geo, lay["sh0"], side == "halo_one_past")
    qs, qe = [], []
    for j, r in enumerate([r for r in geo["regs"] if r["rc1"] + IVX_RP_HALO <= r["shi"]]):
        x = region_points(rng, b, r, 200, 200)
        qs += [hp[1][4 * j:4 * j + 4], x]; qe += [hp[2][4 * j:4 * j + 4], x]
    qs, qe = np.concatenate(qs), np.concatenate(qe)
    p = cols(np.zeros(len(qs)), qs, qe)
    want = orc.join(*b, *p, per_row=True, threads=4)
    f, B = assert_lean_walks(lay, b, p, want[2], len(want[0]), {"IVX_JOIN_PATH": "regions"})
    assert f["maxlen"] == 65535 and (IVX_RP_HALO + 1) << lay["sh0"] < f["maxlen"], f   # packed: only the halo test diverts them
    assert_lean_walks(layf, b, p, want[2], len(want[0]), {"IVX_JOIN_PATH": "regions"})
    check_join(ctx, ix, b, p, ixf=ixf, want=want)
    check_rowvals(ctx, b, p, lay)


def wide_build(span):
    """150 k rows of length 2^14 - 1 over one key spanning `span` coordinates from -2^31: sh0 = 14; 2^32 - 2^25 keeps
    255 regions of R = 1024 cells (2^24 coordinates each), 2^32 - 1 needs R = 2048"""
    n = 150_000
    s = -2**31 + np.arange(n, dtype=np.int64) * (span - 20_000) // (n - 1)
    s[-1] = -2**31 + span
    return cols(np.zeros(n), s, np.minimum(s + 16383, 2**31 - 1))


@pytest.fixture(scope="module")
def wide_side(ctx):
    b = wide_build(2**32 - 2**25)
    with env(IVX_FILTER="0"):
        ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    lay, geo = layout_of(ix, *b, 1)
    assert lay["sh0"] == 14 and lay["rcells"] == 1024 and lay["pk24"] == 1 and lay["fg"] == NOFG and lay["slow"] == 0, lay
    yield b, ix, lay, geo
    ix.free()


@pytest.mark.parametrize("side", ["pk24_width_2p24", "pk24_wider"])
def test_pk24(ctx, side, wide_side):
    if side == "pk24_width_2p24":
        b, ix, lay, geo = wide_side
        ixf = None
        assert lay["nreg"] == IVX_MAXREG
    else:
        b = wide_build(2**32 - 1)
        ix, ixf = build2(ctx, b, 1)
        lay, geo = layout_of(ix, *b, 1)
        assert lay["sh0"] == 14 and lay["rcells"] == 2048 and lay["pk24"] == 0, lay
    rng = np.random.default_rng(5)
    p = edge_probes(geo, lay["sh0"], rng, 100_000, -2**31, 2**31 - 70_000, maxlen=60_000)
    check_join(ctx, ix, b, p, ixf=ixf)
    with env(**({"IVX_FILTER": "0"} if ixf is None else {})):            # (the wide side is built without the bitmap)
        check_rowvals(ctx, b, p, lay)
    if ixf is not None:
        ix.free(); ixf.free()


@pytest.mark.parametrize("nk", [255, 256, 257, 1023, 1024, 1025])
def test_region_and_key_counts(ctx, nk):
    """nk keys with rows, each one region: one radix digit -> 1024 digits -> two-level routing; KT_MAX keys in LDS;
    the per-row and exists modes take the partition up to 1023 regions"""
    rng = np.random.default_rng(nk)
    per = 30
    k = np.repeat(np.arange(nk), per)
    s = k.astype(np.int64) * 10_000 + rng.integers(0, 200, len(k))
    b = cols(k, s, s + rng.integers(0, 16, len(k)))
    ix, ixf = build2(ctx, b, nk)
    lay, geo = layout_of(ix, *b, nk)
    assert lay["nreg"] == nk, lay
    m = 40 * nk
    pk = rng.integers(0, nk, m)
    ps = pk.astype(np.int64) * 10_000 + rng.integers(-60, 300, m)
    p = cols(pk, ps, ps + rng.integers(0, 40, m))
    f = probe_form(lay, m, m, {"IVX_JOIN_PATH": "regions"})
    assert f["routing"] == ("256" if nk <= 255 else "1024" if nk <= 1023 else "two-level") and f["klds"] == (nk <= KT_MAX), f
    assert probe_form(lay, m, m, {"IVX_JOIN_PATH": "regions"}, mode="per_row")["path"] == ("regions" if nk <= 1023 else "direct")
    check_join(ctx, ix, b, p, ixf=ixf)
    check_rowvals(ctx, b, p, lay)
    ix.free(); ixf.free()


@pytest.mark.parametrize("side", ["bitmap_32_blocks", "bitmap_33_blocks"])
def test_bitmap_blocks(ctx, side):
    """probe rows over exactly 32 bitmap blocks (tested) against 33 (routed without a test), and rows in a key's last
    and overflow blocks; with the bitmap the packed length field ends at 255"""
    rng = np.random.default_rng(7)
    nk = 3
    k = rng.integers(0, nk, 20_000)
    s = rng.integers(0, 50_000_000, len(k))
    b = cols(k, s, s + rng.integers(0, 300, len(k)))
    with env(IVX_FILTER="force"):
        ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=nk)
    lay, geo = layout_of(ix, *b, nk)
    assert lay["fg"] != NOFG, lay
    g = lay["fg"]
    nb = 32 if side == "bitmap_32_blocks" else 33
    qs, qe, qk = [], [], []
    for key in range(nk):
        sel = b[0] == key
        o, span = int(b[1][sel].min()), int(b[1][sel].max()) - int(b[1][sel].min())
        last = span >> g
        for j in list(range(0, last + 2, max(1, last // 300))) + [last - 40, last - 32, last - 1, last, last + 1]:
            x = o + (j << g)
            qs += [x, x + 1]; qe += [x + (nb << g) - 1, x + (nb << g) - 1]; qk += [key, key]
        for x in (o + span - 1, o + span, o + span + 1, o + ((last + 1) << g), o + ((last + 1) << g) + 77):   # last / overflow block
            for ln in (0, 254, 255, 256):
                qs.append(x); qe.append(x + ln); qk.append(key)
    p = cols(qk, np.clip(qs, -2**31, 2**31 - 1), np.clip(qe, -2**31, 2**31 - 1))
    p = cat(p, edge_probes(geo, lay["sh0"], rng, 50_000, -100, 50_001_000))
    f = probe_form(lay, len(p[1]), len(p[1]), {"IVX_JOIN_PATH": "regions"})
    assert f["filter"] and f["maxlen"] == 255, f
    check_join(ctx, ix, b, p)
    ix.free()


# ---------------------------------------------------------------- probe side

def sparse_probes(b, n, seed, lens=(0, 300)):
    rng = np.random.default_rng(seed)
    lo, hi = int(b[1].min()) - 1000, int(b[1].max()) - 70_000
    st = rng.integers(lo, hi, n)
    return cols(np.zeros(n), st, st + rng.integers(*lens, n))


@pytest.mark.parametrize("side", ["crossover_2p21_minus_1", "crossover_2p21"])
def test_default_crossover(ctx, side, wide_side):
    b, ix, lay, geo = wide_side
    n = (1 << 21) - (1 if side == "crossover_2p21_minus_1" else 0)
    p = sparse_probes(b, n, 8)
    assert probe_form(lay, n, n)["path"] == ("direct" if side == "crossover_2p21_minus_1" else "regions")
    check_join(ctx, ix, b, p, knobs=("default",), path=None)


@pytest.mark.parametrize("side", ["len_65535_minus_1", "len_65535", "len_65535_plus_1"])
def test_length_field_65535(ctx, side, wide_side):
    b, ix, lay, geo = wide_side
    d = {"len_65535_minus_1": -1, "len_65535": 0, "len_65535_plus_1": 1}[side]
    p = sparse_probes(b, 200_000, 9)
    f = probe_form(lay, len(p[1]), len(p[1]), {"IVX_JOIN_PATH": "regions"})
    assert f["maxlen"] == 65535 and f["packed"] and f["lean"], f
    pe = p[2].astype(np.int64)
    pe[::3] = p[1][::3].astype(np.int64) + f["maxlen"] + d                # probe length (end - start)
    pe[1::3] = p[1][1::3].astype(np.int64) + f["maxlen"] + d + 2          # the rowval path's strict boundary (adj on both ends)
    p = (p[0], p[1], pe.astype(np.int32))
    check_join(ctx, ix, b, p)
    with env(IVX_FILTER="0"):                                              # (the wide side is built without the bitmap)
        check_rowvals(ctx, b, p, lay)


@pytest.mark.parametrize("side", ["len_255_minus_1", "len_255", "len_255_plus_1"])
def test_length_field_bitmap_255(ctx, side, sparse_side):
    """with the bitmap the length field ends at 255; rows of 254..258 coordinates match at most two build rows, so the
    two rows per lane k_pick_rows takes stage at most 256 pairs a batch and k_fill_fast tests every escape itself"""
    b, _, ixf, _, lay, _ = sparse_side
    d = {"len_255_minus_1": -1, "len_255": 0, "len_255_plus_1": 1}[side]
    rng = np.random.default_rng(10)
    n = 150_000
    st = rng.integers(-500, int(b[1].max()) + 500, n)
    ln = np.full(n, 255 + d, np.int64)
    ln[1::2] += 2                                                         # (rowval strict: 2 higher)
    p = cols(np.zeros(n), st, st + ln)
    want = orc.join(*b, *p, per_row=True, threads=4)
    assert want[2].max() <= 2
    f, B = assert_lean_walks(lay, b, p, want[2], len(want[0]), {"IVX_JOIN_PATH": "regions"})
    assert f["maxlen"] == 255 and f["filter"] and B == 2, (f, B)
    check_join(ctx, ixf, b, p, knobs=("default", "fill_old", "dense0", "pack0"), want=want)
    with env(IVX_FILTER="force"):
        check_rowvals(ctx, b, p, lay)


@pytest.mark.parametrize("side", ["len_32767_n_2p24", "len_32767_n_2p24_plus_1"])
def test_length_field_large_batch(ctx, side, wide_side):
    """n = 2^24 probe rows keep 24 row-id bits (maxlen 65535), 2^24 + 1 take 25 (maxlen 32767); 4 partition tiles"""
    b, ix, lay, geo = wide_side
    n = (1 << 24) + (0 if side == "len_32767_n_2p24" else 1)
    p = sparse_probes(b, n, 11, lens=(0, 40))
    f = probe_form(lay, n, n)
    want_max = 65535 if side == "len_32767_n_2p24" else 32767
    assert f["path"] == "regions" and f["maxlen"] == want_max and f["part_tiles"] == 4, f
    pe = p[2].astype(np.int64)
    for j, dd in enumerate((-1, 0, 1)):
        pe[j::97] = p[1][j::97].astype(np.int64) + 32767 + dd
        pe[j + 3::97] = p[1][j + 3::97].astype(np.int64) + 65535 + dd
    p = (p[0], p[1], pe.astype(np.int32))
    with env(IVX_HOST_CHUNKS=1):                                           # one call sees all n rows
        check_join(ctx, ix, b, p, knobs=("default", "fill_old"), path=None)


def lattice(m, X=1 << 18, even=False):
    """one build row per coordinate (even: per even coordinate) covering m coordinates: a point matches m rows (even: 1
    on even points, 0 on odd ones)"""
    s = np.arange(0, X, 2 if even else 1, dtype=np.int64)
    return cols(np.zeros(len(s)), s, s + m - 1)


@pytest.mark.parametrize("B,m", [(1, 4), (2, 2), (4, 1), (8, 0)])
@pytest.mark.parametrize("side", ["ring_256", "ring_257"])
def test_ring_half(ctx, side, B, m):
    """a full batch of B rows per lane stages exactly 256 pairs (the half ring), or 257 (one row matches one more:
    k_fill_fast sends the batch to the rest list).  m = 0: the even lattice, rows alternate 1 and 0 matches.  Every region
    gets 8192 probe rows, one partition tile of them, so batches are whole."""
    b0 = lattice(max(m, 1), even=(m == 0))
    ix0 = ctx.build(pyivx.KIND_OVERLAP, *b0, n_keys=1)
    lay0, geo0 = layout_of(ix0, *b0, 1)
    ix0.free()
    regs = geo0["regs"][1:17]
    # the one coordinate per region that matches one more row (an extra point row on it; odd for the even lattice)
    qstar = np.array([r["rbase"] + 1001 for r in regs], np.int64)
    b = cat(b0, cols(np.zeros(len(qstar)), qstar, qstar))
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    lay, geo = layout_of(ix, *b, 1)
    assert (lay["sh0"], lay["rcells"], lay["slow"]) == (lay0["sh0"], lay0["rcells"], 0), (lay, lay0)
    rng = np.random.default_rng(B * 10 + m)
    ps = []
    for i, r in enumerate(geo["regs"][1:17]):
        w = (r["rend"] - r["rbase"]) - 16
        x = r["rbase"] + 8 + rng.integers(0, w, FP_CHUNK)
        if m == 0:
            x = (x & ~1) + (np.arange(FP_CHUNK) & 1)                       # even, odd, even, ...
        x[x == qstar[i]] += 2
        if side == "ring_257":
            x[1 if m == 0 else 0] = qstar[i]                               # (m = 0: an odd slot, 0 matches -> 1)
        ps.append(x)
    ps = np.concatenate(ps)
    p = cols(np.zeros(len(ps)), ps, ps)
    want = orc.join(*b, *p, per_row=True, threads=4)
    per = want[2].reshape(16, FP_CHUNK)
    if m == 0:
        base = np.tile(np.array([1, 0], np.uint64), FP_CHUNK // 2)
    else:
        base = np.full(FP_CHUNK, m, np.uint64)
    extra = (per - base[None, :])
    if side == "ring_256":
        assert (extra == 0).all()
    else:
        assert (extra.sum(axis=1) == 1).all() and (extra >= 0).all()
    f = probe_form(lay, len(ps), len(ps), {"IVX_JOIN_PATH": "regions", "IVX_DENSE": "0", "IVX_RP_ROWS": str(B)})
    assert f["lean"] and f["rows_per_lane"] == B and f["part_tiles"] == 1, f
    with env(IVX_DENSE=0, IVX_RP_ROWS=B):
        check_join(ctx, ix, b, p, knobs=("default", "fill_old"), want=want)
    ix.free()


@pytest.mark.parametrize("counts", [(8191, 8192, 8193), (16383, 16384, 16385), (5000, 0, 5000, 1, 300)],
                         ids=["chunk_8192", "page_16384", "empty_and_single"])
def test_chunks_and_pages(ctx, counts, sparse_side):
    """regions holding 8192 +- 1 routed rows (FP_CHUNK) and 16384 +- 1 (a 2^14-row page), an empty region between two
    full ones, a region with one row; half the points match one row, so four rows per lane stage at most 256 pairs"""
    b, ix, ixf, lay, layf, geo = sparse_side
    rng = np.random.default_rng(sum(counts))
    ps = np.concatenate([region_points(rng, b, r, (c + 1) // 2, c // 2) for r, c in zip(geo["regs"][3:], counts)])
    rng.shuffle(ps)
    p = cols(np.zeros(len(ps)), ps, ps)
    want = orc.join(*b, *p, per_row=True, threads=4)
    reg = route_region(lay, b, p)
    assert [int((reg == r).sum()) for r in range(3, 3 + len(counts))] == list(counts)
    f, B = assert_lean_walks(lay, b, p, want[2], len(want[0]), {"IVX_JOIN_PATH": "regions"})
    assert f["lgpg"] == 14 and B == 4, (f, B)
    check_join(ctx, ix, b, p, ixf=ixf, want=want)
    check_rowvals(ctx, b, p, lay)


@pytest.mark.parametrize("band", ["0.40", "0.40+", "0.8", "0.8+", "1.6", "1.6+", "3.5", "3.5+"])
def test_density_through_cap(ctx, band, wide_side):
    """the same inputs with pair buffers of floor(x * n) against one more: rows per lane 8 / 4 / 2 / 1 and the dense
    fill past 3.5; with the bitmap on (k_pick_rows) too"""
    b, ix, lay, geo = wide_side
    n = 300_000
    p = sparse_probes(b, n, 12, lens=(0, 50))
    p = (np.where(np.arange(n) % 2 == 1, 1, 0).astype(np.uint32), p[1], p[2])   # (odd rows: a key the index does not have)
    want = orc.join(*b, *p, threads=4)
    x = float(band.rstrip("+"))
    cap = int(np.floor(x * n)) + (1 if band.endswith("+") else 0)
    assert len(want[0]) <= 0.40 * n                                       # every cap is valid
    f = probe_form(lay, n, cap, {"IVX_JOIN_PATH": "regions"})
    want_rows = {"0.40": 8, "0.40+": 4, "0.8": 4, "0.8+": 2, "1.6": 2, "1.6+": 1, "3.5": 1, "3.5+": 1}[band]
    assert f["rows_per_lane"] == want_rows and f["dense"] == (band == "3.5+") and f["lean"] == (band != "3.5+"), f
    wset = pair_set(*want)
    with env(IVX_FILTER="force"):
        ixf = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    for x_ in (ix, ixf):
        for kv in ({}, {"IVX_FILL": "old"}):
            with env(IVX_JOIN_PATH="regions", IVX_NO_PLAN=1, **kv):
                ob, op = ctx.overlap_fill(x_, *p, cap=cap)
            assert (pair_set(ob, op) == wset).all(), (band, kv)
    ixf.free()


@pytest.mark.parametrize("n", [4 * (1 << 20) - 1, 4 * (1 << 20), 37 * 8192 - 1, 37 * 8192 + 1],
                         ids=["tiles_4Mi_minus_1", "tiles_4Mi", "tiles_k8192_minus_1", "tiles_k8192_plus_1"])
def test_ragged_tiles(ctx, n, wide_side):
    b, ix, lay, geo = wide_side
    p = sparse_probes(b, n, 13, lens=(0, 3000))
    path = None if n >= (1 << 21) else "regions"
    f = probe_form(lay, n, n, {"IVX_JOIN_PATH": path} if path else {})
    assert f["path"] == "regions" and f["part_tiles"] == (2 if n == 4 << 20 else 1), f
    check_join(ctx, ix, b, p, knobs=("default", "fill_old", "pack0", "part_two") if n < (1 << 21) else ("default", "fill_old"), path=path)
