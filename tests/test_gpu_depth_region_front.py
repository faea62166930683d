"""-m gpu: the span front of the two region statistics (csrc/ivx_depth_regions.hpp describes it and holds what they share: the
search, c0, the segment rule, the tile walk) and the two tile passes behind it, driven through both statistics on one input so
that they answer for each other:
ivx_depth_profile_summarize / _windows (sums and threshold counts) and ivx_depth_profile_quantiles / _window_quantiles
(min, max and quantiles), bit-exact against tests/depth_regions_oracle.py and tests/depth_quantiles_oracle.py.

With T = pyivx.DEPTH_REGION_TILE = pyivx.DEPTH_RANK_TILE steps per tile, key 0 has 4T + 1 steps at positions 10 + 3j and
starts the step list, so its step j is step j of the list and tile boundaries fall at j = T, 2T, ...; its coverage takes a
different range in every tile, so a tile taken or left out between a region's ends shows in the extremes.  The regions
are one per case of the front: before the first step, a zero stretch, inside one step, one tile, adjacent tiles, 2, 3 and 4
tiles apart, whole tiles, the key's last step with and without a domain end, 64 and 65 segments, and the empty ones.  A second
profile of at most 2T steps makes no aggregates and no table.  Every region goes through the table form and, one window a
call, through the windows form, in host and in device memory mode, with skip_pos0 off and on.  Windows that last_pos
does not cut, many a call, have a test of their own."""
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

T = pyivx.DEPTH_REGION_TILE
M32 = 0xFFFFFFFF
NULL = pyivx.NULL_IDX
BIG = 1 << 31                   # a key length no test position reaches, below 2^32 - 1: a segment's end event is clipped
# key 0's coverage per tile of the step list, all inside [-2, 3]; key 3's c0 is 1, so with skip_pos0 every value lies in
# [-3, 3]: the thresholds hold every region's min and max + 1, and 0
TILE_RANGES = ((1, 2), (-1, 1), (2, 3), (-2, 0), (1, 1))
THR = (-3, -2, -1, 0, 1, 2, 3, 4)
QN, QD = (0, 1, 2, 4), 4        # min, lower quartile, lower median, max


def pos0(j):
    return 10 + 3 * j           # key 0's step j covers [pos0(j), pos0(j) + 2]


def dev_u32(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def stepped(ctx, keys, pos, cov, n_keys):
    """one step per (key, position) with coverage cov from there on (per key: no two in a row equal, the first not 0)
    -> (profile, its steps as the oracles take them)"""
    keys, pos, cov = np.asarray(keys, np.uint32), np.asarray(pos, np.uint32), np.asarray(cov, np.int64)
    prev = np.concatenate([[0], cov[:-1]])
    prev[np.concatenate([[True], keys[1:] != keys[:-1]])] = 0
    w = (cov - prev).astype(np.int32)
    assert (w != 0).all()
    p = ctx.depth_profile(skey=keys, sstart=pos, send=np.full(len(pos), M32, np.uint32), sweight=w,
                          key_len=np.full(n_keys, BIG, np.uint32), n_keys=n_keys)
    st = p.read()
    assert p.steps() == len(pos) and np.array_equal(st[2], cov.astype(np.int32)) and np.array_equal(st[1], pos)
    return p, st


def key0_cov(rng, S):
    """S values, step j from TILE_RANGES[j // T], no two in a row equal"""
    x = np.zeros(S, np.int64)
    for j in range(S):
        lo, hi = TILE_RANGES[j // T]
        x[j] = rng.integers(lo, hi + 1)
        if j and x[j] == x[j - 1]:
            x[j] = x[j] + 1 if x[j] < hi else (lo if lo != x[j] else x[j] - 1)     # (a one-value range steps outside it)
    assert (np.diff(x) != 0).all() and x[0] != 0 and x.min() >= -2 and x.max() <= 3
    return x


def make(ctx, S):
    """key 0: S steps at 10 + 3j; key 1: three steps; key 2: none; key 3: five steps, the first at position 0 with coverage 1"""
    rng = np.random.default_rng(S)
    keys = np.concatenate([np.full(S, 0), np.full(3, 1), np.full(5, 3)])
    pos = np.concatenate([pos0(np.arange(S)), [100, 200, 300], [0, 7, 20, 21, 90]])
    cov = np.concatenate([key0_cov(rng, S), [2, -2, 3], [1, 3, -2, 0, 2]])
    return stepped(ctx, keys, pos, cov, 4)


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def profiles(ctx):
    assert T == pyivx.DEPTH_RANK_TILE
    tiled, flat = make(ctx, 4 * T + 1), make(ctx, T + 5)
    assert tiled[0].steps() > 2 * T >= flat[0].steps()      # aggregates and a table; neither
    yield dict(tiled=tiled, flat=flat)
    tiled[0].free(); flat[0].free()


def front_regions(S):
    """(key, start, end, case) per case of the span front that fits a key 0 of S steps"""
    L = S - 1                                               # key 0's last step
    r = [(0, 0, 9, "before the first step"), (0, 3, 5, "before the first step"),
         (0, 4, pos0(5) + 1, "zero stretch + steps"),
         (0, pos0(7) + 1, pos0(7) + 1, "inside one step"), (0, pos0(7), pos0(7) + 2, "one whole step"),
         (0, pos0(3) + 1, pos0(40), "one tile"),
         (0, pos0(T - 1), pos0(T), "adjacent tiles"), (0, pos0(T - 1) + 2, pos0(T) + 2, "adjacent tiles"),
         (0, pos0(T), pos0(T), "a tile's first step"), (0, pos0(T - 1) + 1, pos0(T) - 1, "a tile's last step"),
         (0, pos0(100), pos0(163), "64 segments"), (0, pos0(100), pos0(164) + 1, "65 segments"),
         (0, 5, pos0(62), "64 segments with the zero stretch"), (0, 5, pos0(63), "65 segments with the zero stretch"),
         (0, pos0(L) - 4, M32, "the key's last step"), (0, pos0(L) + 50, pos0(L) + 60, "inside the key's last step"),
         (0, 1, M32, "the whole key"),                   # (from 1: as a window its width is a u32)
         (1, 1, M32, "three steps"), (1, 150, 250, "three steps"), (1, 301, 400, "three steps"),
         (2, 0, 500, "a key without steps"), (2, 7, 7, "a key without steps"),
         (3, 0, 100, "a step at position 0"), (3, 0, 0, "a step at position 0"), (3, 1, 6, "a step at position 0"), (3, 5, 21, "a step at position 0"),
         (NULL, 0, 100, "the skip mark"), (0, 100, 50, "end < start"), (3, 9, 8, "end < start"),
         (2, 1, 9, "a domain that ends below pos_lo")]          # (key_hi[2] = 0: with pos_lo = 1 the domain is empty)
    if S > 4 * T:
        r += [(0, pos0(5), pos0(2 * T + 7), "2 tiles apart"), (0, pos0(T - 1), pos0(2 * T), "2 tiles apart"),
              (0, pos0(5), pos0(3 * T + 7), "3 tiles apart"), (0, pos0(T + 9) + 1, pos0(4 * T) + 1, "3 tiles apart"),
              (0, pos0(5), pos0(4 * T), "4 tiles apart"), (0, 2, pos0(4 * T) + 9, "4 tiles apart with the zero stretch"),
              (0, pos0(T), pos0(4 * T - 1) + 2, "whole tiles"), (0, pos0(0), pos0(3 * T - 1), "whole tiles"),
              (0, pos0(2 * T), pos0(3 * T - 1) + 2, "one whole tile")]
    return r


def check_cases(st, regs):
    """the regions are the cases they are named for"""
    segs = {c: dqo.segment_count(st, k, s, e) for k, s, e, c in regs if c.startswith("6")}
    assert segs == {"64 segments": 64, "65 segments": 65, "64 segments with the zero stretch": 64, "65 segments with the zero stretch": 65}
    p = st[1][st[0] == 0].astype(np.int64)
    for k, s, e, c in regs:
        if k == 0 and "tiles apart" in c:
            a, b = np.searchsorted(p, s, side="right") - 1, np.searchsorted(p, e, side="right") - 1
            assert b // T - max(a, 0) // T == int(c[0])


def run_table(p, qkey, qs, qe, pos_lo, key_hi, skip, device):
    cols = [dev_u32(a) if device else a for a in (qkey, qs, qe, key_hi)]
    sums = p.summarize(*cols[:3], THR, pos_lo, cols[3], skip)
    ranks = p.quantiles(*cols[:3], QN, QD, pos_lo, cols[3], skip)
    p.ctx.synchronize()                                     # a device-mode call may return with its kernels in flight
    return [[x.cpu().numpy() if device else x for x in out] for out in (sums, ranks)]


def run_windows(p, wins, skip, device):
    """one window a call: (key, first, last) -> the rows of both statistics, stacked"""
    sums, ranks = [], []
    for k, first, last in wins:
        width = max(last - first + 1, 1)
        sums.append(p.windows(k, first, last, width, 1, THR, skip, device=device))
        ranks.append(p.window_quantiles(k, first, last, width, 1, QN, QD, skip, device=device))
    p.ctx.synchronize()
    cat = lambda rows: [np.concatenate([(r[j].cpu().numpy() if device else r[j]) for r in rows], axis=-1) for j in range(len(rows[0]))]
    return cat(sums), cat(ranks)


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


def answer_for_each_other(sums, ranks):
    """what the sums' threshold counts and the ranks' extremes say about each other, per region with bases"""
    bases, _, ge = sums
    rb, mn, mx, q = ranks
    assert np.array_equal(bases, rb)
    m = bases > 0
    assert m.any() and not (mn[~m].any() or mx[~m].any() or q[:, ~m].any())
    assert np.array_equal(q[0][m], mn[m]) and np.array_equal(q[-1][m], mx[m])       # q_num = 0 and q_num = q_den
    assert (mn[m] >= THR[0]).all() and (mx[m] + 1 <= THR[-1]).all()                 # the thresholds hold every min and max + 1
    for j, t in enumerate(THR):
        assert np.array_equal(ge[j][m] == bases[m], mn[m] >= t)
        assert np.array_equal(ge[j][m] == 0, mx[m] < t)


@pytest.mark.parametrize("domain", [False, True])
@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("which", ["tiled", "flat"])
def test_both_statistics_through_the_front(profiles, which, skip, domain):
    p, st = profiles[which]
    S = int((st[0] == 0).sum())
    regs = front_regions(S)
    check_cases(st, regs)
    qkey, qs, qe = (np.array([r[j] for r in regs], np.uint32) for j in range(3))
    # a domain: [1, key_hi]; key 0's ends 100 positions into its last step, key 2's below pos_lo
    pos_lo, key_hi = (1, np.array([pos0(S - 1) + 100, 250, 0, 60], np.uint32)) if domain else (0, None)
    want_s = dro.summarize_prefix(st, qkey, qs, qe, THR, pos_lo, key_hi, skip)
    want_r = dqo.quantiles_steps(st, qkey, qs, qe, QN, QD, pos_lo, key_hi, skip)
    answer_for_each_other(want_s, want_r)
    # the same spans as windows: the clipped region, or a window that starts beyond its last position for an empty one
    rows = [i for i in range(len(regs)) if qkey[i] != NULL]
    clipped = [dro.clip(qkey, qs, qe, i, pos_lo, key_hi) for i in rows]
    wins = [(int(qkey[i]), 1, 0) if c is None else c for i, c in zip(rows, clipped)]
    ws, we = (np.concatenate(x) for x in zip(*[dro.windows_as_regions(f, l, max(l - f + 1, 1), 1) for _, f, l in wins]))
    wkey = np.array([w[0] for w in wins], np.uint32)
    wwant_s = dro.summarize_prefix(st, wkey, ws, we, THR, 0, None, skip)
    wwant_r = dqo.quantiles_steps(st, wkey, ws, we, QN, QD, 0, None, skip)
    same(wwant_s, (want_s[0][rows], want_s[1][rows], want_s[2][:, rows]))           # (the oracles agree that the spans are the same)
    same(wwant_r, (want_r[0][rows], want_r[1][rows], want_r[2][rows], want_r[3][:, rows]))
    for device in (False, True):
        sums, ranks = run_table(p, qkey, qs, qe, pos_lo, key_hi, skip, device)
        same(sums, want_s); same(ranks, want_r)
        answer_for_each_other(sums, ranks)
        wsums, wranks = run_windows(p, wins, skip, device)
        same(wsums, wwant_s); same(wranks, wwant_r)
        answer_for_each_other(wsums, wranks)


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("which", ["tiled", "flat"])
def test_windows_whose_ends_come_from_the_window_index(profiles, which, skip):
    """many windows a call, all but the last not cut by last_pos: the bounds are first_pos + i * width .. + width - 1"""
    p, st = profiles[which]
    S = int((st[0] == 0).sum())
    for key, first, last, width in ((0, 0, pos0(S - 1) + 500, 1000), (0, 7, pos0(S - 1), 3 * T + 1), (1, 90, 400, 100), (2, 0, 99, 10), (3, 0, 200, 7)):
        n = (last - first) // width + 2                     # one window beyond last_pos: empty
        qs, qe = dro.windows_as_regions(first, last, width, n)
        assert (qe[:-2] < last).all() and qe[-1] < qs[-1]
        qkey = np.full(n, key, np.uint32)
        want_s = dro.summarize_prefix(st, qkey, qs, qe, THR, 0, None, skip)
        want_r = dqo.quantiles_steps(st, qkey, qs, qe, QN, QD, 0, None, skip)
        for device in (False, True):
            sums = p.windows(key, first, last, width, n, THR, skip, device=device)
            ranks = p.window_quantiles(key, first, last, width, n, QN, QD, skip, device=device)
            p.ctx.synchronize()
            sums, ranks = ([x.cpu().numpy() if device else x for x in out] for out in (sums, ranks))
            same(sums, want_s); same(ranks, want_r)
            answer_for_each_other(sums, ranks)
