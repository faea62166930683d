"""-m gpu: depth region order statistics on the device (ivx_depth_profile_quantiles / ivx_depth_profile_window_quantiles,
csrc/ivx_depth_rank.hip), bit-exact against tests/depth_quantiles_oracle.py, in host and in device memory mode.

Profiles are made from weighted segments whose end event is clipped away, one step per segment, so that step counts and
coverage values are exact.  With T = pyivx.DEPTH_RANK_TILE steps per (min, max) tile, SEGS = pyivx.DEPTH_RANK_SEGS segments
ranked in one wavefront's registers and GRID = pyivx.DEPTH_RANK_SELECT_GRID workgroups of the select kernel, the shapes sit
where the kernels can go wrong: keys of T - 1 ... 3T + 1 steps laid end to end and one of 10T + 1 steps, regions with 0 to 9
tiles strictly between their first and last step (both sides of every power of two of the sparse table), the unique extreme
in every part of a region a different code path reads, 1 / 2 / SEGS - 1 / SEGS / SEGS + 1 segments with and without the zero
stretch, value spans on both sides of every digit count of the radix select, ranks on both sides of a segment boundary, and
more long regions in one call than the select kernel has workgroups.  (A region of more than one segment cannot have a value
span of 0: consecutive steps differ.  That span is tested on one segment.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_quantiles_oracle as dqo  # noqa: E402
import depth_regions_oracle as dro  # noqa: E402
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

T = pyivx.DEPTH_RANK_TILE
SEGS = pyivx.DEPTH_RANK_SEGS
GRID = pyivx.DEPTH_RANK_SELECT_GRID
WG = 4                          # regions (wavefronts) per workgroup of the query kernel
M32 = 0xFFFFFFFF
NULL = pyivx.NULL_IDX
BIG = 1 << 31                   # a key length no test position reaches, below 2^32 - 1: a segment's end event is clipped
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
QN, QD = (0, 1, 2, 3, 4, 2, 1), 4               # min, quartiles, max, and two repeats: seven quantiles a call
SIZES = (T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 1)
DTS = (np.int64, np.int32, np.int32, np.int32)


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


def dev_u32(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def same(got, want):
    assert len(got) == len(want) == 4
    for g, w, dt in zip(got, want, DTS):
        assert g.dtype == dt and g.shape == w.shape and np.array_equal(g, w)


def stepped(ctx, keys, pos, cov, n_keys):
    """one step per (key, position) with coverage cov from there on (per key: no two in a row equal, the first not 0)
    -> (profile, its steps as the oracle takes them)"""
    keys, pos, cov = np.asarray(keys, np.uint32), np.asarray(pos, np.uint32), np.asarray(cov, np.int64)
    prev = np.concatenate([[0], cov[:-1]])
    prev[np.concatenate([[True], keys[1:] != keys[:-1]])] = 0
    w = ((cov - prev) & M32).astype(np.uint32).view(np.int32)              # the weights: coverage differences, int32 wrap-around
    assert (w != 0).all()
    p = ctx.depth_profile(skey=keys, sstart=pos, send=np.full(len(pos), M32, np.uint32), sweight=w,
                          key_len=np.full(n_keys, BIG, np.uint32), n_keys=n_keys)
    st = p.read()
    assert p.steps() == len(pos) and np.array_equal(st[2], cov.astype(np.int32)) and np.array_equal(st[1], pos)
    return p, st


def distinct_runs(rng, lo, hi, S):
    """S values in [lo, hi], no two in a row equal, the first not 0"""
    x = rng.integers(lo, hi + 1, S).astype(np.int64)
    if S and x[0] == 0:
        x[0] = hi if hi != 0 else lo
    for j in range(1, S):
        if x[j] == x[j - 1]:
            x[j] = x[j - 1] + 1 if x[j - 1] < hi else lo
    return x


def check(p, st, qkey, qs, qe, qn=QN, qd=QD, pos_lo=0, key_hi=None, skip=False, loop_span=0, ctx=None):
    """host mode and device mode against quantiles_steps (and quantiles_loop on the regions of at most loop_span bases)"""
    qs, qe = np.asarray(qs, np.uint32), np.asarray(qe, np.uint32)
    qkey = None if qkey is None else np.asarray(qkey, np.uint32)
    want = dqo.quantiles_steps(st, qkey, qs, qe, qn, qd, pos_lo, key_hi, skip)
    if loop_span:
        m = np.flatnonzero(qe.astype(np.int64) - qs.astype(np.int64) < loop_span)
        sub = dqo.quantiles_loop(st, None if qkey is None else qkey[m], qs[m], qe[m], qn, qd, pos_lo, key_hi, skip)
        same(sub, (want[0][m], want[1][m], want[2][m], want[3][:, m]))
    host = p.quantiles(qkey, qs, qe, qn, qd, pos_lo, key_hi, skip, ctx=ctx)
    same(host, want)
    cols = [dev_u32(a) for a in (qkey, qs, qe, key_hi)]
    dev = p.quantiles(*cols[:3], qn, qd, pos_lo, cols[3], skip, ctx=ctx)
    (ctx or p.ctx).synchronize()                            # a device-mode call may return with its kernels in flight
    same([d.cpu().numpy() for d in dev], want)
    return want


def segs_of(st, qkey, qs, qe):
    return np.array([dqo.segment_count(st, int(k), int(s), int(e)) for k, s, e in zip(qkey, qs, qe)])


# ---------------------------------------------------------------------------------------------- tile edges
@pytest.fixture(scope="module")
def edges(ctx):
    """keys 0..5 with SIZES steps (key 0 all positive, key 1 all negative, the others mixed), key 6 without steps, key 7
    with three steps; key 5 has a step at position 0"""
    rng = np.random.default_rng(11)
    keys, pos, cov = [], [], []
    for k, S in enumerate(SIZES):
        first = 0 if k == 5 else 10 + k
        keys.append(np.full(S, k)); pos.append(first + 3 * np.arange(S))
        cov.append(distinct_runs(rng, *((1, 60), (-60, -1), (-40, 40), (-3, 3), (-300, 300), (-40, 40))[k], S))
    keys.append(np.full(3, 7)); pos.append(np.array([100, 200, 300])); cov.append(np.array([2, -3, 1]))
    p, st = stepped(ctx, np.concatenate(keys), np.concatenate(pos), np.concatenate(cov), 8)
    yield p, st
    p.free()


def edge_regions(st, k):
    """regions of key k around every tile boundary inside its slice of the step list"""
    g0 = int(np.searchsorted(st[0], k))
    pos = st[1][st[0] == k].astype(np.int64)
    S = len(pos)
    cand = {0, 1, S // 2, S - 2, S - 1}
    for b in range(g0 // T + 1, (g0 + S - 1) // T + 1):                   # global tile boundaries inside the key
        cand |= {b * T - g0 - 1, b * T - g0, b * T - g0 + 1}
    cand = sorted(c for c in cand if 0 <= c < S)
    qs, qe, far = [], [], 0
    for ia in cand:
        for ib in cand:
            if ib < ia:
                continue
            far = max(far, (g0 + ib) // T - (g0 + ia) // T)
            for ds in (-1, 0, 1):
                for de in (-1, 0, 1):
                    s, e = pos[ia] + ds, pos[ib] + de
                    if s >= 0:
                        qs.append(s); qe.append(e)                          # (e < s happens for ia == ib: an empty region)
    qs += [0, 0, 0, pos[-1] + 5, pos[-1], 0, pos[3] + 1, 500]
    qe += [max(pos[0] - 1, 0), 5, pos[0] + 4, pos[-1] + 1000, M32, M32, pos[3] + 1, 400]
    return np.array(qs, np.uint32), np.array(qe, np.uint32), far


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("k", range(len(SIZES)))
def test_tile_edges(edges, k, skip):
    p, st = edges
    qs, qe, far = edge_regions(st, k)
    assert far >= (3 if SIZES[k] > 3 * T else 1 if SIZES[k] > T else 0)
    check(p, st, np.full(len(qs), k, np.uint32), qs, qe, QN, QD, 1 if skip else 0, None, skip, loop_span=300)


# ---------------------------------------------------------------------------------------------- the table's levels, the extremes' places
GMAX, GMIN = 4 * T + 300, 6 * T + 700           # global step numbers of the unique largest and smallest value of the long key
TOP, BOTTOM = 1000, -1000


@pytest.fixture(scope="module")
def long_key(ctx):
    """key 0 with five steps, then key 1 with 10T + 1 steps over the tiles 0..10: values in [-50, 50] but for TOP at the
    global step GMAX and BOTTOM at GMIN"""
    rng = np.random.default_rng(12)
    S = 10 * T + 1
    cov = distinct_runs(rng, -50, 50, S)
    cov[GMAX - 5], cov[GMIN - 5] = TOP, BOTTOM
    keys = np.concatenate([np.zeros(5), np.ones(S)])
    pos = np.concatenate([20 + 4 * np.arange(5), 9 + 3 * np.arange(S)])
    p, st = stepped(ctx, keys, pos, np.concatenate([[3, 1, 4, 1, 5], cov]), 2)
    yield p, st
    p.free()


def test_tiles_strictly_between_on_both_sides_of_every_table_level(long_key):
    p, st = long_key
    gp = st[1].astype(np.int64)                             # position of a global step (the long key: steps 5 ..)
    qs, qe, between = [], [], []
    for nb in (0, 1, 2, 3, 4, 5, 7, 8, 9):
        for ta in sorted({0, 1, 10 - nb - 1}):
            if ta + nb + 1 > 10:
                continue
            for ia in {max(ta * T, 5), ta * T + 500, ta * T + T - 1}:
                for ib in {(ta + nb + 1) * T, min((ta + nb + 1) * T + 77, len(gp) - 2), min((ta + nb + 1) * T + T - 1, len(gp) - 1)}:
                    for d in (-1, 0, 1):
                        qs.append(gp[ia] + d); qe.append(gp[ib] + d)
                        between.append(ib // T - ia // T - 1)
    qs += [gp[5 + 7], gp[6], gp[T], gp[T - 1]]              # the first and last step share a step, a tile, lie in adjacent tiles
    qe += [gp[5 + 7] + 2, gp[900], gp[T] + 1, gp[T] + 1]
    assert {0, 1, 2, 3, 4, 5, 7, 8, 9} <= set(between)
    w = check(p, st, np.ones(len(qs), np.uint32), qs, qe, QN, QD, loop_span=4)
    assert (w[2] == TOP).any() and (w[1] == BOTTOM).any() and (w[2] < TOP).any() and (w[1] > BOTTOM).any()


@pytest.mark.parametrize("g,which,val", [(GMAX, 2, TOP), (GMIN, 1, BOTTOM)])
def test_where_the_unique_extreme_lies(long_key, g, which, val):
    p, st = long_key
    gp = st[1].astype(np.int64)
    assert g % T not in (0, T - 1) and st[2][g] == val
    inside = [(gp[g + 1] - 1, gp[g + 3 * T]),               # the clipped first segment, one base visible
              (gp[g - 3 * T], gp[g]),                       # the clipped last segment, one base visible
              (gp[g - 5], gp[g + 3 * T]),                   # the first tile's tail
              (gp[g - 3 * T], gp[g + 5]),                   # the last tile's head
              (gp[g - T], gp[g + 3 * T]),                   # the first tile strictly between
              (gp[g - 3 * T], gp[g + T]),                   # the last tile strictly between
              (gp[g - 2 * T], gp[g + 2 * T]),               # a middle one
              (gp[g + 1] - 1, gp[g + 1] - 1), (gp[g], gp[g + 1]), (gp[g - 1], gp[g])]
    outside = [(gp[g + 1], gp[g + 3 * T]), (gp[g - 3 * T], gp[g] - 1), (gp[g + 1], gp[g + 1]), (gp[g] - 1, gp[g] - 1),
               (gp[g + 1], gp[g + 2]), (gp[g - 1], gp[g] - 1)]
    qs, qe = zip(*(inside + outside))
    w = check(p, st, np.ones(len(qs), np.uint32), qs, qe, QN, QD)
    assert (w[which][:len(inside)] == val).all() and (w[which][len(inside):] != val).all()
    assert np.array_equal(w[3][0 if which == 1 else 4], w[which])


def test_zero_stretch_is_the_unique_extreme(edges):
    p, st = edges
    for k, which in ((0, 1), (1, 2)):                       # all positive: the 0 is the minimum; all negative: the maximum
        pos = st[1][st[0] == k].astype(np.int64)
        qs = [pos[0] - 1, 0, pos[0] - 1, 0, pos[0]]
        qe = [pos[0], pos[5], pos[2 * T // 3 * 1], M32, pos[-1]]
        w = check(p, st, np.full(5, k, np.uint32), qs, qe, QN, QD)
        assert (w[which][:4] == 0).all() and w[which][4] != 0 and (w[3 - which][:4] != 0).all()


# ---------------------------------------------------------------------------------------------- segment counts, ranks
@pytest.mark.parametrize("skip", [False, True])
def test_segment_counts_around_the_register_bound(edges, skip):
    p, st = edges
    qkey, qs, qe, want_segs = [], [], [], []
    for k in (2, 4, 5):
        pos = st[1][st[0] == k].astype(np.int64)
        for m in (1, 2, SEGS - 1, SEGS, SEGS + 1):
            for a in (10, T - 100):                      # without the zero stretch: m steps
                qkey += [k, k]; qs += [pos[a], pos[a] + 1]; qe += [pos[a + m - 1], pos[a + m - 1] + 2]; want_segs += [m, m]
            if pos[0] > 0:                                  # with it: the stretch and m - 1 steps
                qkey += [k, k]; qs += [pos[0] - 1, 0]; qe += [pos[m - 2] + 1 if m > 1 else pos[0] - 1, pos[m - 2] if m > 1 else pos[0] - 1]
                want_segs += [m, m]
    assert segs_of(st, qkey, qs, qe).tolist() == want_segs
    check(p, st, qkey, qs, qe, QN, QD, 1 if skip else 0, None, skip, loop_span=400)


@pytest.mark.parametrize("nseg", [5, SEGS, SEGS + 6])
def test_ranks_on_both_sides_of_a_segment_boundary(edges, nseg):
    p, st = edges
    k = 4
    pos = st[1][st[0] == k].astype(np.int64)
    lo, hi = int(pos[T + 3]) + 1, int(pos[T + 3 + nseg - 1]) + 1
    L = hi - lo + 1
    assert dqo.segment_count(st, k, lo, hi) == nseg and 2 <= L - 1 <= 65536
    vals, lens = dqo.segments(st, k, lo, hi)
    o = np.argsort(vals, kind="stable")
    vals, cum = vals[o], np.cumsum(lens[o])
    cuts = [int(c) for c in cum[:-1] if vals[np.searchsorted(cum, c - 1, side="right")] != vals[np.searchsorted(cum, c, side="right")]]
    assert len(cuts) >= 2
    c1, c2 = cuts[0], cuts[len(cuts) // 2]
    qn = (c1 - 1, c1, c2 - 1, c2, 0, L - 1, L - 2, 1)       # with q_den = L - 1 the rank is q_num itself
    w = check(p, st, [k], [lo], [hi], qn, L - 1)
    assert w[3][0][0] < w[3][1][0] and w[3][2][0] < w[3][3][0] and w[3][4][0] == w[1][0] and w[3][5][0] == w[2][0]


def test_median_of_odd_and_even_lengths_and_one_base(edges):
    p, st = edges
    pos = st[1][st[0] == 2].astype(np.int64)
    qs = [pos[4], pos[4], pos[4], pos[4] + 1, pos[4], pos[4]]
    qe = [pos[4], pos[4] + 1, pos[5] + 1, pos[5] + 1, pos[200], pos[200] + 1]
    w = check(p, st, np.full(6, 2), qs, qe, (1,), 2, loop_span=1000)
    assert w[0].tolist() == [1, 2, 5, 4, 3 * 196 + 1, 3 * 196 + 2]
    assert w[3][0][0] == w[1][0] == w[2][0] and w[3][0][1] == w[1][1]
    w = check(p, st, np.full(6, 2), qs, qe, (0, 1, 32768, 65535, 65536), 65536, loop_span=1000)
    assert np.array_equal(w[3][0], w[1]) and np.array_equal(w[3][4], w[2])


def test_every_position_of_the_range(ctx):
    p, st = stepped(ctx, [0], [0], [I32_MAX], 2)
    w = check(p, st, [0, 0, 1, 1], [0, 1, 0, 5], [M32, M32, M32, 5], (0, 1, 2, 65536), 65536)
    assert w[0].tolist() == [1 << 32, M32, 1 << 32, 1] and w[1].tolist() == [I32_MAX, I32_MAX, 0, 0] and not w[3][:, 2:].any()
    p.free()
    p, st = stepped(ctx, [0, 0], [5, 1 << 30], [I32_MIN, I32_MAX], 1)       # 5 zeros, -2^31 up to 2^30, then 2^31 - 1
    w = check(p, st, [0, 0], [0, 0], [M32, (1 << 31) + 8], QN, QD)
    assert w[1].tolist() == [I32_MIN] * 2 and w[2].tolist() == [I32_MAX] * 2 and w[3][1].tolist() == [0, I32_MIN] and w[3][2].tolist() == [I32_MAX, I32_MAX]
    p.free()


# ---------------------------------------------------------------------------------------------- value spans: the select's digits
SPANS = (0, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 32) - 1)
SPAN_STEPS = 200


@pytest.fixture(scope="module")
def spans(ctx):
    """key k: SPAN_STEPS steps (one for the span 0) from position 40 on whose values span exactly SPANS[k], 0 inside"""
    rng = np.random.default_rng(13)
    keys, pos, cov = [], [], []
    for k, sp in enumerate(SPANS):
        S = SPAN_STEPS if sp else 1
        lo = I32_MIN if sp == (1 << 32) - 1 else -(sp // 3) - 1
        c = distinct_runs(rng, lo, lo + sp, S)
        if sp:
            c[0], c[1] = lo, lo + sp                        # both ends of the span among the first steps, and again later
            c[130], c[131] = lo + sp, lo
            c[2] = c[2] if c[2] != c[1] else lo + sp - 1
            for j in (129, 132):
                if c[j] == c[j + 1] or c[j] == c[j - 1]:
                    c[j] = lo + 1 + (j & 1) * 2
        keys.append(np.full(S, k)); pos.append(40 + 5 * np.arange(S)); cov.append(c)
    p, st = stepped(ctx, np.concatenate(keys), np.concatenate(pos), np.concatenate(cov), len(SPANS))
    yield p, st
    p.free()


@pytest.mark.parametrize("k", range(len(SPANS)))
def test_value_spans(spans, k):
    p, st = spans
    sp = SPANS[k]
    if sp == 0:
        w = check(p, st, [k, k], [40, 45], [40, M32], QN, QD)
        assert np.array_equal(w[1], w[2])
        return
    P = lambda j: 40 + 5 * j
    qs = [P(0), P(0) + 1, P(0), 0, P(0), 0, P(100), P(60)]
    qe = [P(1), P(1) + 3, P(40), P(50), P(199) + 9, M32, P(199), P(131) + 2]
    nseg = segs_of(st, [k] * 8, qs, qe)
    assert nseg.tolist() == [2, 2, 41, 52, 200, 201, 100, 72]
    w = check(p, st, np.full(8, k), qs, qe, QN, QD)
    full = [i for i in range(8) if i != 6]
    assert ((w[2].astype(np.int64) - w[1])[full] == sp).all()       # short and long regions with exactly this span
    w = check(p, st, np.full(8, k), qs, qe, (1, 7, 100, 40000, 65535, 65536, 0, 30000), 65536)
    assert np.array_equal(w[3][5], w[2]) and np.array_equal(w[3][6], w[1])


# ---------------------------------------------------------------------------------------------- the long-region list
@pytest.mark.parametrize("n_long", [0, 1, GRID + 37])
def test_long_regions_mixed_with_short_ones(long_key, n_long):
    p, st = long_key
    gp = st[1].astype(np.int64)
    rng = np.random.default_rng(n_long)
    n = 2 * n_long + 9
    a = rng.integers(5, 9 * T, n)
    m = rng.integers(1, SEGS + 1, n)                        # short: at most SEGS segments
    is_long = np.zeros(n, bool)
    is_long[rng.choice(n, n_long, replace=False)] = True
    m[is_long] = rng.integers(SEGS + 1, 300, n_long)
    if n_long > 1:
        m[np.flatnonzero(is_long)[:3]] = (SEGS + 1, 2 * T, T + 3)
    qs, qe = gp[a] + rng.integers(0, 3, n), gp[a + m - 1] + rng.integers(0, 3, n)
    assert ((segs_of(st, np.ones(n), qs, qe) > SEGS) == is_long).all()
    check(p, st, np.ones(n, np.uint32), qs, qe, QN, QD)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, WG - 1, WG + 1])
def test_region_counts(edges, n):
    p, st = edges
    rng = np.random.default_rng(n)
    qkey = rng.integers(0, 8, n).astype(np.uint32)
    qs = rng.integers(0, 9000, n).astype(np.uint32)
    qe = (qs + rng.integers(0, 9000, n) * rng.integers(0, 2, n) + rng.integers(0, 100, n)).astype(np.uint32)
    check(p, st, qkey, qs, qe, QN, QD)


# ---------------------------------------------------------------------------------------------- what the sums' tests check, carried over
def test_key_without_steps_null_keys_and_no_key_column(edges):
    p, st = edges
    qs, qe = np.array([0, 5, 100, 250, 7, 0], np.uint32), np.array([M32, 4, 250, 250, 90, 50], np.uint32)
    w = check(p, st, [6, 6, 7, 7, NULL, NULL], qs, qe, QN, QD, loop_span=300)
    assert w[0].tolist() == [1 << 32, 0, 151, 1, 0, 0] and w[1].tolist() == [0, 0, -3, -3, 0, 0] and w[2].tolist() == [0, 0, 2, -3, 0, 0]
    assert w[3][2].tolist() == [0, 0, 2, -3, 0, 0]          # 100 bases at 2, 51 at -3: the lower median is rank 75
    check(p, st, None, qs, qe, QN, QD, loop_span=300)       # every region on key 0


def test_domain(edges):
    p, st = edges
    key_hi = np.array([50, 20000, 8, 9, 0, 3 * T, 77, 250], np.uint32)
    rng = np.random.default_rng(3)
    n = 400
    qkey = rng.integers(0, 8, n).astype(np.uint32)
    qs = rng.integers(0, 3 * T * 3 + 50, n).astype(np.uint32)
    qe = (qs + rng.integers(0, 3000, n)).astype(np.uint32)
    # pos_lo = 9: key 2's domain [9, 8] is empty; key 4's ends below pos_lo; key 7's cuts the open block at 250
    w = check(p, st, qkey, qs, qe, QN, QD, 9, key_hi, False, loop_span=400)
    assert not w[0][(qkey == 2) | (qkey == 4)].any() and (w[0][qkey == 5] > 0).any()
    w = check(p, st, [7, 7, 7, 7], [100, 240, 251, 0], [M32, 260, 300, M32], QN, QD, 1, key_hi, True, loop_span=400)
    assert w[0].tolist() == [151, 11, 0, 250] and w[2].tolist() == [2, -3, 0, 2]
    # the step at position 0 with pos_lo = 1 and skip_pos0: key 5's c0 is taken off everywhere, in the tiles too
    c0 = int(st[2][st[0] == 5][0])
    assert c0 != 0
    a = check(p, st, [5, 5], [1, 1], [3 * T * 3, 150], QN, QD, 1, None, True)
    b = check(p, st, [5, 5], [1, 1], [3 * T * 3, 150], QN, QD, 1, None, False)
    assert all(np.array_equal(x.astype(np.int64), y.astype(np.int64) - c0) for x, y in zip(a[1:], b[1:]))


def test_thousands_of_small_keys_around_a_long_one(ctx):
    rng = np.random.default_rng(21)
    nk, big = 3001, 1500
    keys, pos, cov = [], [], []
    for k in range(nk):
        S = 3 * T + 5 if k == big else (0 if k % 7 == 3 else 1 + k % 2)
        keys.append(np.full(S, k)); pos.append(50 + 7 * np.arange(S) + k % 5); cov.append(distinct_runs(rng, -9, 9, S))
    p, st = stepped(ctx, np.concatenate(keys), np.concatenate(pos), np.concatenate(cov), nk)
    g0 = int(np.searchsorted(st[0], big))
    assert g0 % T not in (0, T - 1) and (g0 + 3 * T + 5) % T != 0          # the long key starts and ends inside a tile
    qkey = np.concatenate([np.arange(nk), np.arange(nk), np.full(6, big)]).astype(np.uint32)
    qs = np.concatenate([np.zeros(nk), 50 + np.arange(nk) % 9, [0, 50, 51, 60, 50 + 7 * T, 0]]).astype(np.uint32)
    qe = np.concatenate([np.full(nk, M32), 60 + np.arange(nk) % 4, [M32, 50 + 7 * (3 * T + 4), 50 + 7 * 3 * T, 70 + 7 * 2 * T, M32, 49]]).astype(np.uint32)
    check(p, st, qkey, qs, qe, QN, QD, loop_span=100)
    p.free()


def test_empty_profile(ctx):
    p = ctx.depth_profile(n_keys=3)
    assert p.steps() == 0
    st = p.read()
    w = check(p, st, [0, 2, NULL, 1], [0, 7, 1, 9], [M32, 9, 5, 8], QN, QD)
    assert w[0].tolist() == [1 << 32, 3, 0, 0] and not w[1].any() and not w[2].any() and not w[3].any()
    for dev in (False, True):
        got = p.window_quantiles(1, 10, 30, 8, device=dev, q_num=(0, 1), q_den=1)
        p.ctx.synchronize()
        got = [g.cpu().numpy() if dev else g for g in got]
        assert got[0].tolist() == [8, 8, 5] and not got[1].any() and not got[2].any() and got[3].tolist() == [[0, 0, 0], [0, 0, 0]]
    p.free()


def test_quantile_counts_bad_fractions_and_null_outputs(edges):
    p, st = edges
    qkey, qs, qe = np.array([0, 5, 7, 6, 4], np.uint32), np.array([0, 20, 150, 3, 30], np.uint32), np.array([M32, 9000, 350, 9, 5000], np.uint32)
    w0 = check(p, st, qkey, qs, qe, (), 2)
    assert w0[3].shape == (0, 5)
    q8 = (0, 1, 2, 3, 4, 5, 6, 7)
    w8 = check(p, st, qkey, qs, qe, q8, 7, loop_span=300)
    assert w8[3].shape == (8, 5) and np.array_equal(w8[3][0], w8[1]) and np.array_equal(w8[3][7], w8[2])
    for qn, qd in ((q8 + (7,), 7), ((1,), 0), ((1,), 65537), ((3,), 2), ((0, 65536, 65537), 65536)):
        for a in ((qkey, qs, qe), tuple(dev_u32(x) for x in (qkey, qs, qe))):
            with pytest.raises(pyivx.IvxError) as ei:
                p.quantiles(*a, qn, qd)
            assert ei.value.status == pyivx.ERR_INVALID
    check(p, st, qkey, qs, qe, (65536, 0, 1), 65536)
    for mask in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
                 (False, True, True, False), (True, False, False, True)):
        for dev in (False, True):
            a = (dev_u32(qkey), dev_u32(qs), dev_u32(qe)) if dev else (qkey, qs, qe)
            got = p.quantiles(*a, q8, 7, outputs=mask)
            p.ctx.synchronize()
            for g, w, m in zip(got, w8, mask):
                assert (g is None) == (not m)
                if m:
                    assert np.array_equal(g.cpu().numpy() if dev else g, w)


# ---------------------------------------------------------------------------------------------- errors
def raw(ctx, p, mem, qkey, qs, qe, n, qn, qd, outs, pos_lo=0, key_hi=None):
    t = np.asarray(qn, np.uint32)
    return pyivx.lib().ivx_depth_profile_quantiles(ctx.h, p.h, mem, qkey, qs, qe, n, pos_lo, key_hi, 0, pyivx._ptr(t), len(t), qd, *outs)


def test_bad_key_leaves_the_outputs_untouched(ctx, edges):
    import torch
    p, _ = edges
    n = 70
    qkey = np.zeros(n, np.uint32)
    qkey[66] = 8                                                            # n_keys = 8
    qs, qe = np.zeros(n, np.uint32), np.full(n, 100, np.uint32)
    outs = [np.full(n, -7, np.int64), np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(2 * n, -7, np.int32)]
    st = raw(ctx, p, pyivx.MEM_HOST, *[pyivx._ptr(a) for a in (qkey, qs, qe)], n, (0, 1), 2, [pyivx._ptr(o) for o in outs])
    assert st == pyivx.ERR_INVALID and b"key id >= n_keys" in pyivx.lib().ivx_last_error(ctx.h)
    assert all((o == -7).all() for o in outs)
    douts = [torch.full((len(o),), -7, dtype=torch.int64 if o.dtype == np.int64 else torch.int32, device="cuda") for o in outs]
    st = raw(ctx, p, pyivx.MEM_DEVICE, *[pyivx._ptr(dev_u32(a)) for a in (qkey, qs, qe)], n, (0, 1), 2, [pyivx._ptr(o) for o in douts])
    assert st == pyivx.ERR_INVALID
    ctx.synchronize()
    assert all(bool((o == -7).all()) for o in douts)
    qkey[66] = NULL                                                         # the skip mark is no error
    assert raw(ctx, p, pyivx.MEM_HOST, *[pyivx._ptr(a) for a in (qkey, qs, qe)], n, (0, 1), 2, [pyivx._ptr(o) for o in outs]) == pyivx.OK
    assert outs[0][66] == 0 and outs[0][0] == 101 and outs[1][66] == 0 and outs[3][n + 66] == 0


def test_misaligned_device_pointers_and_other_indexes(ctx, edges):
    import torch
    p, _ = edges
    n = 8
    buf = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    al = lambda off: C.c_void_p(buf.data_ptr() + off)
    ok = [al(0), al(512), al(1024)]
    outs = [al(2048), al(2560), al(3072 + 4), al(3584)]                     # (int32 columns need 4 bytes only)
    assert raw(ctx, p, pyivx.MEM_DEVICE, *ok, n, (1,), 2, outs) == pyivx.OK
    for i in range(3):
        bad = list(ok)
        bad[i] = al(512 * i + 2)
        assert raw(ctx, p, pyivx.MEM_DEVICE, *bad, n, (1,), 2, outs) == pyivx.ERR_INVALID
    for i, off in enumerate((4, 2, 2, 2)):
        bad = list(outs)
        bad[i] = al(2048 + 512 * i + off)
        assert raw(ctx, p, pyivx.MEM_DEVICE, *ok, n, (1,), 2, bad) == pyivx.ERR_INVALID
    assert raw(ctx, p, pyivx.MEM_DEVICE, *ok, n, (1,), 2, outs, key_hi=al(3072 + 2)) == pyivx.ERR_INVALID
    ctx.synchronize()
    # any index that is not a profile
    ix = ctx.build(pyivx.KIND_COUNT, np.zeros(4, np.uint32), np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32) + 5)
    z = np.zeros(1, np.uint32)
    o = np.zeros(1, np.int64)
    L = pyivx.lib()
    assert L.ivx_depth_profile_quantiles(ctx.h, ix.h, pyivx.MEM_HOST, None, pyivx._ptr(z), pyivx._ptr(z), 1, 0, None, 0, None, 0, 2,
                                         pyivx._ptr(o), None, None, None) == pyivx.ERR_UNSUPPORTED
    assert L.ivx_depth_profile_window_quantiles(ctx.h, ix.h, pyivx.MEM_HOST, 0, 0, 10, 5, 2, 0, None, 0, 2,
                                                pyivx._ptr(o), None, None, None) == pyivx.ERR_UNSUPPORTED
    ix.free()


def test_from_another_context(edges):
    p, st = edges
    other = pyivx.Ctx(0)
    check(p, st, [5, 0, 7, 4], [0, 100, 0, 20], [M32, 5000, 400, 2000], QN, QD, ctx=other)
    other.close()


# ---------------------------------------------------------------------------------------------- windows
def check_windows(p, st, key, first, last, width, n=None, qn=QN, qd=QD, skip=False):
    host = p.window_quantiles(key, first, last, width, n, qn, qd, skip)
    nn = len(host[0])
    qs, qe = dro.windows_as_regions(first, last, width, nn)
    want = dqo.quantiles_steps(st, np.full(nn, key, np.uint32), qs, qe, qn, qd, 0, None, skip)
    same(host, want)
    dev = p.window_quantiles(key, first, last, width, n, qn, qd, skip, device=True)
    p.ctx.synchronize()
    same([d.cpu().numpy() for d in dev], want)
    return want


def test_windows(edges):
    p, st = edges
    w = check_windows(p, st, 5, 0, 3 * (3 * T + 1) + 40, 1000)             # the last window is cut; 334 segments a window
    assert w[0][-1] == (3 * (3 * T + 1) + 41) % 1000 and len(w[0]) == (3 * (3 * T + 1) + 40) // 1000 + 1
    check_windows(p, st, 5, 1, 9000, 977, skip=True)
    check_windows(p, st, 4, 0, 6000, 150)                                   # 50 or 51 segments a window
    check_windows(p, st, 0, 5, 4000, 64, n=70)                              # more windows than cover the span: empty ones
    check_windows(p, st, 6, 0, 100, 7)
    check_windows(p, st, 3, 50, 40, 10, n=3)                                # last_pos < first_pos: all empty
    check_windows(p, st, 7, M32 - 10, M32, 4, n=3)
    with pytest.raises(pyivx.IvxError) as ei:
        p.window_quantiles(7, M32 - 10, M32, 4, n=4)                        # first_pos + 3 * 4 > 2^32 - 1
    assert ei.value.status == pyivx.ERR_INVALID
    for bad in (dict(key=8, width=5), dict(key=0, width=0)):
        with pytest.raises(pyivx.IvxError) as ei:
            p.window_quantiles(bad["key"], 0, 100, bad["width"], n=2)
        assert ei.value.status == pyivx.ERR_INVALID
    for qn, qd in (((3,), 2), ((1,), 0), (tuple(range(9)), 9)):
        with pytest.raises(pyivx.IvxError) as ei:
            p.window_quantiles(0, 0, 100, 10, q_num=qn, q_den=qd)
        assert ei.value.status == pyivx.ERR_INVALID


@pytest.mark.parametrize("skip", [False, True])
def test_width_one_is_expand_in_int32(edges, skip):
    p, st = edges
    for key, first, n in ((5, 0, 2 * T + 77), (0, 3, 500), (7, 90, 300), (6, 0, 40)):
        _, cov = p.expand(key, first, n, skip_pos0=skip, want_pos=False)
        w = check_windows(p, st, key, first, first + n - 1, 1, qn=(0, 1, 2), qd=2, skip=skip)
        v = dro.values(st, key, first, n, skip)
        assert np.abs(v).max() <= 32767                                     # inside Int16: the two calls must agree
        for col in (w[1], w[2], w[3][0], w[3][1], w[3][2]):
            assert np.array_equal(col, cov.astype(np.int32))
        assert (w[0] == 1).all()


# ---------------------------------------------------------------------------------------------- merged profiles
def test_merged_profile_ranks_like_the_one_shot_profile(ctx):
    rng = np.random.default_rng(8)

    def weighted(n):
        s = rng.integers(0, 20000, n).astype(np.uint32)
        return dict(skey=rng.integers(0, 3, n).astype(np.uint32), sstart=s, send=(s + rng.integers(0, 300, n)).astype(np.uint32),
                    sweight=rng.integers(-4, 5, n).astype(np.int32), n_keys=3)
    x, y = weighted(4000), weighted(4000)
    a, b = ctx.depth_profile(**x), ctx.depth_profile(**y)
    m = a.merge(b)
    both = {k: np.concatenate([x[k], y[k]]) for k in ("skey", "sstart", "send", "sweight")}
    one = ctx.depth_profile(n_keys=3, **both)
    assert m.steps() == one.steps() > 3 * T
    n = 500
    qkey = rng.integers(0, 3, n).astype(np.uint32)
    qs = rng.integers(0, 21000, n).astype(np.uint32)
    qe = (qs + rng.integers(0, 21000, n) * rng.integers(0, 2, n)).astype(np.uint32)
    want = check(m, m.read(), qkey, qs, qe, QN, QD, loop_span=200)
    same(one.quantiles(qkey, qs, qe, QN, QD), want)
    for p in (a, b, m, one):
        p.free()
