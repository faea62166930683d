"""The lean fill's drained walk (k_fill_fast: a 64-row group's walk ends once at most T lanes are still active, their
tails wait in a per-wavefront stash of 48 entries and one pass per batch walks them): the pair multiset against the oracle
with IVX_FILL_DRAIN unset (the constants: T = 12 at 8 rows per lane, 16 at 4, 0 at 2 and 1), with IVX_FILL_DRAIN=0 (the
plain walk) and, where a case says so, with a forced T.

The routed order inside a region is not deterministic, so no case places rows on lanes: what happens is either certain for
any order, or both sides of a threshold occur with near certainty -- then the case computes every row's candidate count on
the host (lean_cells_of's cells: ((rel + 1) >> sh0) - 1 .. (rel + len) >> sh0) and asserts the mix from the binomial over
a 64-row group.  That is a check on the inputs, not on the kernel.

Build sides are `striped`: rows of length 2^8 - 1 (which pins sh0 = 8, as in test_gpu_region_forms.level0_lean_build),
all at the first coordinate of their cell, in a pattern of period six cells: `a` rows in cell 6i, `c` rows in cell 6i + 2,
the other four empty.  A point's list is the cell before its own plus its own, so points in cell
    6i     have a candidates, all matching      6i + 1 have a candidates, none matching
    6i + 2 have c candidates, all matching      6i + 3 have c candidates, none matching
    6i + 4 and 6i + 5 have none.
"""
import contextlib
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402
import test_gpu_region_forms as rf  # noqa: E402

pytestmark = pytest.mark.gpu
env, cols, layout_of, probe_form, check_join = rf.env, rf.cols, rf.layout_of, rf.probe_form, rf.check_join
region_points, halo_probes, FP_CHUNK = rf.region_points, rf.halo_probes, rf.FP_CHUNK

CELL = 256                         # 2^sh0
NPERIOD = 680                      # periods of six cells: 4080 cells, 255 regions of 16
STASH = 48                         # RP_STASH (ivx_regions_probe.hip)
T_OF = {8: 12, 4: 16, 2: 0, 1: 0}   # fill_drain_of
BASE_ENV = {"IVX_JOIN_PATH": "regions", "IVX_DENSE": "0", "IVX_FILTER": "0"}


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    for sd in _sides.values():                                             # the indexes the cases shared
        sd[1].free()
    _sides.clear()
    c.close()


@contextlib.contextmanager
def drain(t):
    """IVX_FILL_DRAIN = t for the calls inside; None: unset"""
    old = os.environ.pop("IVX_FILL_DRAIN", None)
    if t is not None:
        os.environ["IVX_FILL_DRAIN"] = str(t)
    try:
        yield
    finally:
        os.environ.pop("IVX_FILL_DRAIN", None)
        if old is not None:
            os.environ["IVX_FILL_DRAIN"] = old


def striped(a, c, extra=()):
    """the build side described above; extra: (cell, rows) pairs added at the first coordinate of other cells"""
    i = np.arange(NPERIOD, dtype=np.int64)
    # (cells 1024 and up, far behind the regions the cases use, hold four more rows each: the layout takes no grid with more
    #  cells than twice the rows, and the sparsest pattern alone has a sixth of a row per cell)
    s = np.concatenate([np.repeat(6 * i * CELL, a), np.repeat((6 * i + 2) * CELL, c), np.repeat(np.arange(1024, 6 * NPERIOD, dtype=np.int64) * CELL, 4)] +
                       [np.full(n, cell * CELL, np.int64) for cell, n in extra])
    return cols(np.zeros(len(s)), s, s + CELL - 1)


_sides = {}                        # (a, c, extra) -> side, freed with the module's context


def side(ctx, a, c, extra=()):
    """(build rows, index, layout, regions 1..16, rows per cell), built once per module"""
    key = (a, c, tuple(extra))
    if key not in _sides:
        b = striped(a, c, extra)
        ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
        lay, geo = layout_of(ix, *b, 1)
        assert (lay["sh0"], lay["slow"], lay["pk24"]) == (8, 0, 1) and lay["nreg"] >= 18 and 12 <= lay["rcells"] <= 56, lay   # (regions 1..16 below cell 1024)
        _sides[key] = (b, ix, lay, geo["regs"][1:17], np.bincount(b[1] >> 8, minlength=6 * NPERIOD + 8))
    return _sides[key]


def pts(rng, reg, classes, n):
    """n points of region reg in cells whose number mod 6 is in `classes` (never a cell's last coordinate: there the list
    is the own cell alone)"""
    cells = np.arange(reg["rc0"], reg["rc1"])
    cells = cells[np.isin(cells % 6, classes)]
    assert len(cells)
    return rng.choice(cells, n) * CELL + rng.integers(0, CELL - 1, n)


def lists_of(cnt, ps, pe, sh0=8, origin=0):
    """every row's candidate count by lean_cells_of's formula"""
    cum = np.concatenate([[0], np.cumsum(cnt)])
    rel = ps.astype(np.int64) - origin
    lo = np.maximum(((rel + 1) >> sh0) - 1, 0)
    hi = np.minimum((rel + (pe.astype(np.int64) - ps.astype(np.int64))) >> sh0, len(cnt) - 1)
    return cum[hi + 1] - cum[lo]


def binom_pmf(n, f):
    return np.array([math.comb(n, k) * f ** k * (1 - f) ** (n - k) for k in range(n + 1)])


def run(ctx, sd, p, B, drains=(None, 0), want=None, n_lean=None):
    """the comparison of every case: lean form, B rows per lane, the pair multiset under each IVX_FILL_DRAIN"""
    b, ix = sd[0], sd[1]
    if want is None:
        want = orc.join(*b, *p, per_row=True, threads=4)
    kv = dict(BASE_ENV)
    if B is not None:
        kv["IVX_RP_ROWS"] = str(B)
    f = probe_form(sd[2], len(p[1]), len(want[0]), kv)
    assert f["lean"] and f["rows_per_lane"] == (B if B is not None else n_lean), f
    for t in drains:
        with env(**kv), drain(t):
            check_join(ctx, ix, b, p, knobs=("default", "fill_old"), want=want)
    return want


def as_points(x):
    return cols(np.zeros(len(x)), x, x)


# ---------------------------------------------------------------- 1. no tails

@pytest.mark.parametrize("B", [8, 4])
@pytest.mark.parametrize("L", [1, 5, 40])
def test_no_tails(ctx, L, B):
    """every routed row of a region has L candidates: all 64 lanes stay active to the end, nothing is stashed, the new loop
    test alone runs (one row in 4 L matches its L rows: 128 pairs per 512 rows on average)"""
    sd = side(ctx, L, 0)
    rng = np.random.default_rng(100 + L)
    x = []
    for r in sd[3]:
        hit = rng.random(FP_CHUNK) < 0.25 / L
        x.append(np.where(hit, pts(rng, r, [0], FP_CHUNK), pts(rng, r, [1], FP_CHUNK)))
    p = as_points(np.concatenate(x))
    assert (lists_of(sd[4], p[1], p[2]) == L).all()
    run(ctx, sd, p, B)


# ---------------------------------------------------------------- 2. tails kept before the first step

@pytest.mark.parametrize("N", [1, 8, 9, 12, 13, 64])
def test_whole_lists_stashed(ctx, N):
    """all rows of a region have empty lists but N in 8192 with 40 candidates (half of them matching all 40): whatever the
    order, a 64-row group that holds at most T of them stashes whole lists before its first step, and the tail pass runs 40
    steps"""
    sd = side(ctx, 40, 0)
    rng = np.random.default_rng(200 + N)
    x = []
    for r in sd[3]:
        v = pts(rng, r, [4, 5], FP_CHUNK)
        v[:N] = np.concatenate([pts(rng, r, [0], N - N // 2), pts(rng, r, [1], N // 2)])
        x.append(rng.permutation(v))
    p = as_points(np.concatenate(x))
    ll = lists_of(sd[4], p[1], p[2])
    assert (ll == 40).sum() == 16 * N and ((ll == 0) | (ll == 40)).all()
    run(ctx, sd, p, None, n_lean=8)


# ---------------------------------------------------------------- 3. both sides of T, 8. one pair short

def two_sided(sd, seed, thresholds):
    """lists of 1 and 6, the fraction of 6s per region set so that a 64-row group (after its first step only the 6s are
    active) falls on each side of every threshold; asserts from the binomial that at least 1 % of the 2048 groups are
    expected on each side of each"""
    rng = np.random.default_rng(seed)
    fr = [(t + 0.5) / 64 for t in thresholds]
    x, ngroups, below, above = [], 0, {t: 0.0 for t in thresholds}, {t: 0.0 for t in thresholds}
    for i, r in enumerate(sd[3]):
        f = fr[i % len(fr)]
        six = rng.random(FP_CHUNK) < f
        hit = rng.random(FP_CHUNK) < 0.05
        one = np.where(hit, pts(rng, r, [0], FP_CHUNK), pts(rng, r, [1], FP_CHUNK))
        big = np.where(hit, pts(rng, r, [2], FP_CHUNK), pts(rng, r, [3], FP_CHUNK))
        x.append(np.where(six, big, one))
        pmf = binom_pmf(64, f)
        for t in thresholds:
            below[t] += FP_CHUNK // 64 * pmf[:t + 1].sum(); above[t] += FP_CHUNK // 64 * pmf[t + 1:].sum()
        ngroups += FP_CHUNK // 64
    p = as_points(np.concatenate(x))
    ll = lists_of(sd[4], p[1], p[2])
    assert ((ll == 1) | (ll == 6)).all() and ngroups >= 2048
    for t in thresholds:
        assert below[t] >= 0.01 * ngroups and above[t] >= 0.01 * ngroups, (t, below[t], above[t])
    return p


@pytest.mark.parametrize("B,force", [(8, None), (4, None), (8, 1), (8, 63)])
def test_both_sides_of_T(ctx, B, force):
    """groups with at most T sixes drain once the ones are done (every group starts with 64 lists: three steps, then the
    test), groups with more walk on (a forced T above the stash's 48
    entries is clamped to it: regions alternate between fractions set for 63 and for 48)"""
    sd = side(ctx, 1, 6)
    T = T_OF[B] if force is None else force
    p = two_sided(sd, 300 + B + (force or 0), sorted({T, min(T, STASH)}))
    run(ctx, sd, p, B, drains=(None, 0) if force is None else (None, 0, force))


def test_one_pair_short(ctx):
    """the input of test_both_sides_of_T[8-None] into buffers one pair short: the call reports IVX_ERR_CAPACITY with the
    pairs it needs, as the plain walk does, and nothing lands behind the buffers' `cap` entries"""
    import torch
    sd = side(ctx, 1, 6)
    p = two_sided(sd, 308, [T_OF[8]])
    pairs = len(orc.join(*sd[0], *p, threads=4)[0])
    dp = [torch.from_numpy(c.view(np.int32)).cuda() for c in p]
    cap, guard = pairs - 1, 4096
    assert probe_form(sd[2], len(p[1]), cap, dict(BASE_ENV, IVX_RP_ROWS="8"))["lean"]
    for t in (None, 0):
        for no_plan in (0, 1):
            ob = torch.full((cap + guard,), -7, dtype=torch.int32, device="cuda"); op = ob.clone()
            with env(IVX_RP_ROWS=8, **({"IVX_NO_PLAN": 1} if no_plan else {}), **BASE_ENV), drain(t):
                if not no_plan:
                    assert ctx.overlap_count(sd[1], *dp) == pairs
                with pytest.raises(pyivx.IvxError) as ei:
                    ctx.overlap_fill(sd[1], *dp, out=(ob[:cap], op[:cap]))
            assert ei.value.status == pyivx.ERR_CAPACITY and f"need {pairs} pairs" in str(ei.value), (t, no_plan)
            assert bool((ob[cap:] == -7).all()) and bool((op[cap:] == -7).all()), (t, no_plan)


# ---------------------------------------------------------------- 4. stash full

def test_stash_full(ctx):
    """lists of 0 and 3 at 8 rows per lane: a group whose threes number at most min(T, room) stashes them before its first
    step; with 11 % threes at least 1 % of the batches would keep more than the stash's 48 entries were it not for the room
    rule, which leaves the lanes of the later groups walking in place"""
    sd = side(ctx, 3, 0)
    rng = np.random.default_rng(400)
    f, T = 0.11, T_OF[8]
    x = []
    for r in sd[3]:
        three = rng.random(FP_CHUNK) < f
        hit = rng.random(FP_CHUNK) < 0.3
        x.append(np.where(three, np.where(hit, pts(rng, r, [0], FP_CHUNK), pts(rng, r, [1], FP_CHUNK)), pts(rng, r, [4, 5], FP_CHUNK)))
    p = as_points(np.concatenate(x))
    ll = lists_of(sd[4], p[1], p[2])
    assert ((ll == 0) | (ll == 3)).all()
    kept = binom_pmf(64, f)                                                 # tails one group would keep with room for all: K if K <= T
    kept = np.concatenate([[kept[0] + kept[T + 1:].sum()], kept[1:T + 1]])
    tot = np.array([1.0])
    for _ in range(8):
        tot = np.convolve(tot, kept)
    assert tot[STASH + 1:].sum() >= 0.01, tot[STASH + 1:].sum()
    run(ctx, sd, p, 8)


# ---------------------------------------------------------------- 5. ring half with a deferred match

@pytest.mark.parametrize("k", [0, 1])
def test_ring_half_deferred(ctx, k):
    """4 rows per lane, batches of 256 rows: every row has one candidate, which matches, but one row per region with 12
    candidates that do not and 1 + k that do.  That row is alone after the first step, so its tail is stashed for any
    T >= 1 and its matches are staged by the tail pass: k = 0 makes its batch exactly 256 pairs (the ring half: staged),
    k = 1 makes it 257 (the batch goes to the rest list, the tail's pairs counted)"""
    star = [int(r["rc0"] + ((3 - r["rc0"]) % 6)) for r in _regs_of_plain(ctx)]          # each region's first cell 6i + 3
    sd = side(ctx, 1, 12, extra=tuple((c, 1 + k) for c in star))
    rng = np.random.default_rng(500 + k)
    x = []
    for r, c in zip(sd[3], star):
        assert r["rc0"] <= c < r["rc1"]
        v = pts(rng, r, [0], FP_CHUNK)
        v[0] = c * CELL + 100
        x.append(rng.permutation(v))
    p = as_points(np.concatenate(x))
    ll = lists_of(sd[4], p[1], p[2]).reshape(16, FP_CHUNK)
    assert ((ll == 13 + k).sum(axis=1) == 1).all() and ((ll == 1).sum(axis=1) == FP_CHUNK - 1).all()
    want = orc.join(*sd[0], *p, per_row=True, threads=4)
    per = want[2].reshape(16, FP_CHUNK)
    # only the star row's batch can pass 256 pairs: every other row has exactly one
    assert ((per == 1 + k) == (ll == 13 + k)).all() if k else (per == 1).all()
    assert ((per == 1) | (ll == 13 + k)).all()
    run(ctx, sd, p, 4, drains=(None, 0, 1), want=want)


def _regs_of_plain(ctx):
    return side(ctx, 1, 12)[3]


# ---------------------------------------------------------------- 6. short last batch, region change

def test_short_batches_and_region_change(ctx):
    """regions of 8192 k + r routed rows for r = 1, 63, 65, 511 (a last batch of every shape), then an empty region, then a
    full one; lists of 1 with a few rows of 40 candidates among them, which are stashed wherever they fall"""
    sd = side(ctx, 1, 40)
    rng = np.random.default_rng(600)
    counts = [FP_CHUNK + 1, FP_CHUNK + 63, 65, FP_CHUNK + 511, 0, FP_CHUNK]
    x = []
    for r, c in zip(sd[3], counts):
        if not c:
            continue
        hit = rng.random(c) < 0.25
        v = np.where(hit, pts(rng, r, [0], c), pts(rng, r, [1], c))
        v[:6] = np.concatenate([pts(rng, r, [2], 1), pts(rng, r, [3], 5)])
        v[-1] = pts(rng, r, [3], 1)[0]                                       # (one of them in the short last batch, if the order has it so)
        x.append(v)
    p = as_points(np.concatenate(x))
    reg = rf.route_region(sd[2], sd[0], p)
    assert [int((reg == r).sum()) for r in range(1, 1 + len(counts))] == counts
    ll = lists_of(sd[4], p[1], p[2])
    assert (ll == 40).sum() == 7 * 5 and ((ll == 1) | (ll == 40)).all()
    run(ctx, sd, p, None, n_lean=8)


# ---------------------------------------------------------------- 7. slow rows beside tails

def test_slow_rows_beside_tails(ctx):
    """rows that reach one coordinate past the slice's halo and rows longer than the packed length field (both listed by
    lean_list_slow for k_fill_rest) in the same regions, and with near certainty the same batches, as rows of 40
    candidates whose tails are stashed"""
    sd = side(ctx, 1, 40)
    rng = np.random.default_rng(700)
    n_each = 1024
    hp = halo_probes({"regs": sd[3]}, 8, past=True)
    assert len(hp[1]) == 4 * 16
    qs, qe = [hp[1].astype(np.int64)], [hp[2].astype(np.int64)]
    for r in sd[3]:
        long_ = rng.random(n_each) < 0.05
        hit = rng.random(n_each) < 0.1
        v = np.where(long_, np.where(hit, pts(rng, r, [2], n_each), pts(rng, r, [3], n_each)),
                     np.where(hit, pts(rng, r, [0], n_each), pts(rng, r, [1], n_each)))
        far = pts(rng, r, [0, 4], 2)                                          # longer than the length field holds
        qs += [v, far]; qe += [v, far + 65535 + np.array([0, 1])]
    qs, qe = np.concatenate(qs), np.concatenate(qe)
    o = rng.permutation(len(qs))
    p = cols(np.zeros(len(qs)), qs[o], qe[o])
    want = orc.join(*sd[0], *p, per_row=True, threads=4)
    f = probe_form(sd[2], len(qs), len(want[0]), dict(BASE_ENV, IVX_RP_ROWS="8"))
    assert f["maxlen"] == 65535, f
    run(ctx, sd, p, 8, want=want)


# ---------------------------------------------------------------- 9. every B

def test_every_rows_per_lane(ctx):
    """one random input of 1.4 candidates per row on average (the headline's geometry: a build row per 3100 coordinates,
    lengths 1..1999, probe lengths 1..299) at 8, 4, 2 and 1 rows per lane with IVX_FILL_DRAIN unset, 0, 8 and 16"""
    rng = np.random.default_rng(900)
    nb, n = 40_000, 100_000
    bs = np.sort(rng.integers(0, nb * 3100, nb))
    b = cols(np.zeros(nb), bs, bs + rng.integers(1, 2000, nb))
    ps = rng.integers(0, nb * 3100, n)
    p = cols(np.zeros(n), ps, ps + rng.integers(1, 300, n))
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=1)
    lay, geo = layout_of(ix, *b, 1)
    assert lay["slow"] == 0 and lay["pk24"] == 1, lay
    origin = int(b[1].min())
    ncell = ((int(b[1].max()) - origin) >> lay["sh0"]) + 1
    cnt = np.bincount((b[1].astype(np.int64) - origin) >> lay["sh0"], minlength=ncell)
    inside = (p[1] >= origin) & (p[2] < int(b[1].max()))
    ll = lists_of(cnt, p[1][inside], p[2][inside], lay["sh0"], origin)
    assert 1.2 <= ll.mean() <= 1.6 and ll.max() >= 5, (ll.mean(), ll.max(), lay)
    want = orc.join(*b, *p, per_row=True, threads=4)
    sd = (b, ix, lay)
    for B in (8, 4, 2, 1):
        run(ctx, sd, p, B, drains=(None, 0, 8, 16), want=want)
    ix.free()
