"""Plain statements of the layout rules behind count_overlaps / coverage / nearest, and the designed inputs of
tests/test_gpu_rank_edges.py.  No GPU and no library here: tests/test_rank_forms_cpu.py checks that every designed input
is what it claims to be, the GPU tests check that the device's readout (pyivx.Index.forms()) equals these rules.

The rules (csrc/ivx_grid.hip k_grid_layout, csrc/ivx_ops32.hip k_nlin_layout, csrc/ivx_join.hip k_nroute_layout):
  grid shift      the smallest sh in 0..31 with  sum over keys with rows of ((span_k >> sh) + 1)  <=  2n + nkeys
  one-word fit    run = sum over keys with rows of (max - min + 1) over BOTH columns; linbits = bitlen(run - 1),
                  rowbits = bitlen(n - 1) (1 for a single value); the one-word sort fits iff linbits + rowbits <= 64
  routing regions cells of 2^10 over every key's span of starts, 2^cs cells per region with the smallest cs that leaves
                  at most 1023 regions; 0 regions when none does (more than 1023 keys with rows)
"""
import numpy as np

LO, HI = -2**31, 2**31 - 1
MAXRUN = 64                     # NLIN_MAXRUN and NFIX_MAXRUN: the longest run of equal (key, start) the run repairs take
LIN_MIN_ROWS = 4096             # below it the nearest build sorts on all three fields at once
KEYS_IN_LDS = 2048              # KEYS_IN_LDS / NLIN_KEYS_LDS: key tables up to this size are privatised in LDS
MAXREG_WIDE = 1023
ROUTE_SH0 = 10
BIG_GAP = 64                    # k_grid_bounds: a stretch of this many empty cells or more is filled by the whole wavefront
WAVE, BLOCK = 64, 256
# pyivx.NEAR_ORDER_* / NEAR_FB_*
PRESORTED, REPAIR, FULL = 0, 1, 2
FB_NOFIT, FB_LIN_RUN, FB_SE_RUN = 1, 2, 4


# ---------------------------------------------------------------------------------------------------- the rules

def _bitlen_m1(x):
    return (int(x) - 1).bit_length() if x > 1 else 1


def key_stats(keys, vals, nkeys):
    """per key: rows, min, max (Python ints; min / max None for a key without rows)"""
    cnt, lo, hi = [0] * nkeys, [None] * nkeys, [None] * nkeys
    for k, v in zip(np.asarray(keys).tolist(), np.asarray(vals).tolist()):
        cnt[k] += 1
        lo[k] = v if lo[k] is None or v < lo[k] else lo[k]
        hi[k] = v if hi[k] is None or v > hi[k] else hi[k]
    return cnt, lo, hi


def grid_form(keys, vals, nkeys):
    """(shift, cells) of the rank grid over one column"""
    cnt, lo, hi = key_stats(keys, vals, nkeys)
    n = sum(cnt)
    spans = [h - l for c, l, h in zip(cnt, lo, hi) if c]
    cells = lambda sh: sum((s >> sh) + 1 for s in spans)
    sh = next((s for s in range(32) if cells(s) <= 2 * n + nkeys), 31)
    return sh, cells(sh)


def lin_fit(keys, starts, ends, nkeys):
    """(linbits, rowbits, fits) of the nearest build's one-word sort"""
    n = len(keys)
    cnt, lo, hi = key_stats(np.concatenate([keys, keys]), np.concatenate([starts, ends]), nkeys)
    run = sum(h - l + 1 for c, l, h in zip(cnt, lo, hi) if c)
    linbits, rowbits = _bitlen_m1(run), _bitlen_m1(n)
    return linbits, rowbits, linbits + rowbits <= 64


def route_regions(keys, starts, nkeys):
    """regions of the routing view over a column of starts"""
    cnt, lo, hi = key_stats(keys, starts, nkeys)
    cells = [((h - l) >> ROUTE_SH0) + 1 for c, l, h in zip(cnt, lo, hi) if c]
    for cs in range(33):
        tot = sum((c + (1 << cs) - 1) >> cs for c in cells)
        if tot <= MAXREG_WIDE:
            return tot
    return 0


def merged_nodes(keys, starts, ends):
    """coverage's merged nodes (interval_tree.rs merge_intervals: stable sort by first, `first <= current.last` merges),
    keys ascending -> (key, first, last)"""
    keys, starts, ends = (np.asarray(a).tolist() for a in (keys, starts, ends))
    rows = sorted(range(len(keys)), key=lambda i: (keys[i], starts[i]))
    out = []
    for i in rows:
        if out and out[-1][0] == keys[i] and starts[i] <= out[-1][2]:
            out[-1][2] = max(out[-1][2], ends[i])
        else:
            out.append([keys[i], starts[i], ends[i]])
    a = np.array(out, np.int64).reshape(-1, 3)
    return a[:, 0].astype(np.uint32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32)


def start_order(keys, starts, ends):
    """row numbers in the nearest index's (key, start, end, row) order"""
    return np.lexsort((np.arange(len(keys)), ends, starts, keys))


def prefix_max_ends(keys, starts, ends):
    """the running maximum of the ends within a key, rows in (key, start, end, row) order"""
    o = start_order(keys, starts, ends)
    out, run, prev = [], None, None
    for k, e in zip(np.asarray(keys)[o].tolist(), np.asarray(ends)[o].tolist()):
        run = e if k != prev or e > run else run
        prev = k
        out.append(run)
    return np.asarray(keys)[o], np.array(out, np.int64)


def max_run(keys, starts):
    """the longest run of rows with equal (key, start)"""
    if len(keys) == 0:
        return 0
    w = (np.asarray(keys).astype(np.int64) << 32) | (np.asarray(starts).astype(np.int64) - LO)
    return int(np.unique(w, return_counts=True)[1].max())


def is_presorted(keys, starts, ends):
    k, s, e = (np.asarray(a).astype(np.int64) for a in (keys, starts, ends))
    a, b = (k[:-1], s[:-1], e[:-1]), (k[1:], s[1:], e[1:])
    below = (b[0] < a[0]) | ((b[0] == a[0]) & ((b[1] < a[1]) | ((b[1] == a[1]) & (b[2] < a[2]))))
    return not below.any()


def expected_grids(kind, keys, starts, ends, nkeys):
    """what Index.forms() must say of a `kind` ("count" | "coverage" | "nearest") index: {"grids": {name: (shift, cells)},
    "nroute_nreg": regions}"""
    if kind == "count":
        g = {"starts": grid_form(keys, starts, nkeys), "ends": grid_form(keys, ends, nkeys)}
        return {"grids": g, "nroute_nreg": route_regions(keys, starts, nkeys)}
    if kind == "coverage":
        nk, nf, nl = merged_nodes(keys, starts, ends)
        g = {"first": grid_form(nk, nf, nkeys), "last": grid_form(nk, nl, nkeys)}
        return {"grids": g, "nroute_nreg": route_regions(nk, nf, nkeys)}
    pk, pm = prefix_max_ends(keys, starts, ends)
    g = {"by_start": grid_form(keys, starts, nkeys), "by_end": grid_form(keys, ends, nkeys), "pmax": grid_form(pk, pm, nkeys)}
    return {"grids": g, "nroute_nreg": route_regions(keys, starts, nkeys)}


# ---------------------------------------------------------------------------------------------------- nearest sort forms

def _probes(rng, nkeys, lo, hi, n, maxlen):
    pk = rng.integers(0, nkeys + 1, n).astype(np.uint32)             # (one probe key beyond the build's)
    ps = rng.integers(lo, hi, n)
    pe = np.minimum(ps + rng.integers(0, maxlen, n), HI)
    return pk, ps.astype(np.int32), pe.astype(np.int32)


def cut_table(n, seed=11):
    """n unsorted rows over 3 keys with a few equal-(key, start) pairs and triples: n = 4095 / 4096 straddle the cut below
    which the build sorts on all three fields"""
    rng = np.random.default_rng(seed)
    bk = rng.integers(0, 3, n).astype(np.uint32)
    bs = rng.integers(0, 400_000, n)
    for i in range(0, 60, 3):                                       # rows i, i+1 (and i+2 for every other group) share (key, start)
        bk[i + 1], bs[i + 1] = bk[i], bs[i]
        if i % 2 == 0:
            bk[i + 2], bs[i + 2] = bk[i], bs[i]
    be = bs + rng.integers(0, 300, n)
    be[1:60:3] = be[0:60:3]                                         # ... and some of them the end too
    o = rng.permutation(n)
    bk, bs, be = bk[o], bs[o].astype(np.int32), be[o].astype(np.int32)
    return dict(bk=bk, bs=bs, be=be, nkeys=3, probes=_probes(rng, 3, -1000, 401_000, 3000, 200))


def run_table(run_len, seed=12):
    """>= 4096 shuffled rows over 3 keys with three runs of exactly `run_len` rows of equal (key, start): one first in
    sorted order, one last, one whose rows straddle a multiple of 256 in sorted position.  Every other (key, start) is
    distinct.  Inside a run the ends descend with the row number and every end occurs twice (once for the first row of an
    odd run), so (end, row) decides the order.  -> dict with `runs` = [(key, start)] in that order and k = 66 probes on them"""
    rng = np.random.default_rng(seed)
    nbg = 4200
    bgk = (np.arange(nbg) % 3).astype(np.uint32)
    bgs = rng.choice(np.arange(0, 2_000_000, 4), nbg, replace=False)           # multiples of 4: distinct, and start - 1 is free
    n0 = int((bgk == 0).sum())
    s1 = np.sort(bgs[bgk == 1])
    # the middle run: j background rows of key 1 before it, so that its first row sits 30 short of a multiple of 256
    j = next(j for j in range(100, len(s1)) if (n0 + run_len + j) % BLOCK == BLOCK - 30)
    runs = [(0, -50), (1, int(s1[j]) - 1), (2, 2_000_100)]
    bk = np.concatenate([bgk] + [np.full(run_len, k, np.uint32) for k, _ in runs])
    bs = np.concatenate([bgs] + [np.full(run_len, s, np.int64) for _, s in runs])
    o = rng.permutation(len(bk))
    bk, bs = bk[o], bs[o]
    be = bs + rng.integers(0, 300, len(bk))
    for k, s in runs:
        rows = np.flatnonzero((bk == k) & (bs == s))                            # ascending row numbers
        be[rows] = s + (run_len - 1 - np.arange(run_len)) // 2 + 3
    bs, be = bs.astype(np.int32), be.astype(np.int32)
    pk, ps, pe = _probes(rng, 3, -1000, 2_001_000, 3000, 200)
    # the k = 66 probes: points and short ranges on and next to the runs' starts
    qk = np.repeat(np.array([k for k, _ in runs], np.uint32), 100)
    d = np.tile(np.arange(100) % 10 - 4, 3)
    qs = np.repeat(np.array([s for _, s in runs], np.int64), 100) + d
    qe = qs + np.tile(np.arange(100) // 10, 3) * 4
    return dict(bk=bk, bs=bs, be=be, nkeys=3, runs=runs, probes=(pk, ps, pe), run_probes=(qk, qs.astype(np.int32), qe.astype(np.int32)))


def fit_table(n, seed=13):
    """32768 keys, each with one row starting at INT32_MIN and one row ending at INT32_MAX, random rows up to n: every key
    spans 2^32 values, run = 2^47 and linbits = 47, so n = 131072 (17 row bits) fits the one-word sort exactly and
    n = 131073 (18) does not"""
    rng = np.random.default_rng(seed)
    K = 32768
    bk = np.empty(n, np.uint32); bs = np.empty(n, np.int64); be = np.empty(n, np.int64)
    bk[:K] = np.arange(K); bs[:K] = LO; be[:K] = LO + rng.integers(0, 50, K)
    bk[K:2 * K] = np.arange(K); be[K:2 * K] = HI; bs[K:2 * K] = HI - rng.integers(0, 50, K)
    m = n - 2 * K
    bk[2 * K:] = rng.integers(0, K, m); bs[2 * K:] = rng.integers(LO, HI - 2**20, m); be[2 * K:] = bs[2 * K:] + rng.integers(0, 2**20, m)
    o = rng.permutation(n)
    return dict(bk=bk[o], bs=bs[o].astype(np.int32), be=be[o].astype(np.int32), nkeys=K, probes=_probes(np.random.default_rng(5), K, LO, HI - 4096, 20000, 4096))


def empty_keys(nkeys):
    """every third key, key 0 and the last key"""
    return [k for k in range(nkeys) if k % 3 == 0 or k == nkeys - 1]


def many_keys_table(nkeys, n=4500, seed=14):
    """n >= 4096 unsorted rows dealt over the keys of [0, nkeys) that are not in empty_keys(nkeys) (about 3 rows a key):
    nkeys = 2048 / 2049 straddle the size up to which the builds keep their key tables in LDS"""
    rng = np.random.default_rng(seed)
    full = np.array(sorted(set(range(nkeys)) - set(empty_keys(nkeys))), np.uint32)
    bk = full[np.arange(n) % len(full)]
    bs = rng.integers(-20_000, 20_000, n)
    be = bs + rng.integers(0, 500, n)
    o = rng.permutation(n)
    pk, ps, pe = _probes(rng, nkeys + 2, -21_000, 21_000, 4000, 300)
    return dict(bk=bk[o], bs=bs[o].astype(np.int32), be=be[o].astype(np.int32), nkeys=nkeys, probes=(pk, ps, pe))


def presorted_table(n, inversion=False, seed=15):
    """n rows in (key, start, end) order with exact duplicates; `inversion`: two neighbouring, different rows swapped"""
    rng = np.random.default_rng(seed)
    bk = rng.integers(0, 4, n).astype(np.uint32)
    bs = rng.integers(0, 300_000, n)
    be = bs + rng.integers(0, 300, n)
    bk[5::50], bs[5::50], be[5::50] = bk[4::50][:len(bk[5::50])], bs[4::50][:len(bk[5::50])], be[4::50][:len(bk[5::50])]   # exact duplicates
    bs[7::50] = bs[6::50][:len(bs[7::50])]; bk[7::50] = bk[6::50][:len(bk[7::50])]                                           # equal (key, start) only
    o = np.lexsort((be, bs, bk))
    bk, bs, be = bk[o], bs[o], be[o]
    if inversion:
        i = next(i for i in range(n // 2, n - 1) if (bk[i], bs[i], be[i]) != (bk[i + 1], bs[i + 1], be[i + 1]))
        for a in (bk, bs, be):
            a[i], a[i + 1] = a[i + 1], a[i]
    return dict(bk=bk, bs=bs.astype(np.int32), be=be.astype(np.int32), nkeys=4, probes=_probes(rng, 4, -1000, 301_000, 3000, 200))


def nearest_form(t, sort2=False):
    """(near_words, near_order, near_fallback) the nearest build must report for table t (sort2: IVX_NEAREST_SORT2 is set)"""
    bk, bs, be, n = t["bk"], t["bs"], t["be"], len(t["bk"])
    if n == 0:
        return 0, PRESORTED, 0
    pre, long_run, fb = is_presorted(bk, bs, be), max_run(bk, bs) > MAXRUN, 0
    if n >= LIN_MIN_ROWS and not sort2:
        if not lin_fit(bk, bs, be, t["nkeys"])[2]:
            fb |= FB_NOFIT
        elif long_run:
            fb |= FB_LIN_RUN
        else:
            return 1, PRESORTED if pre else REPAIR, fb
    if pre:
        return 2, PRESORTED, fb
    if n >= LIN_MIN_ROWS and not long_run:
        return 2, REPAIR, fb
    return 2, FULL, fb | (FB_SE_RUN if n >= LIN_MIN_ROWS else 0)


# ---------------------------------------------------------------------------------------------------- rank grids

GRID_N, GRID_ORIGIN = 1000, -5000
GRID_SPAN = (2 * GRID_N + 1) * 16 - 1                   # the rule then gives shift 4 and 2001 cells for the single key
# empty cells behind (between it and its successor) the row at these sorted positions; every 64 and 65 behind a last lane,
# a first lane, the last row of a 256-row workgroup and the last rows that have a successor (behind the very last row of a
# column there is never a gap: a key's last cell holds its largest value)
GRID_GAPS = {10: 1, 20: 62, 30: 63, 40: 127, 50: 128, 200: 64, 210: 65,
             63: 64, 127: 65, 64: 65, 128: 64, 255: 64, 767: 65, GRID_N - 3: 64, GRID_N - 2: 65}
GRID_EQUAL = (300, 600)                                 # rows [300, 600): one cell of 300 equal values (distinct=False)
GRID_SIXTEEN = (600, 616)                               # rows [600, 616): one cell holding all its 16 coordinates


def grid_column(distinct=False):
    """The designed single-key column, ascending: GRID_N values over [GRID_ORIGIN, GRID_ORIGIN + GRID_SPAN], both ends
    present, GRID_GAPS empty cells behind the rows named there, single empty cells behind further rows until the last row
    lands in the last cell, every other row in the cell after its predecessor's.  distinct=True (coverage merges equal
    points into one node, which would change the column): rows [300, 600) fill 19 neighbouring cells with 16 distinct values
    each instead of sharing one value.  -> (values int32, cell of every row)"""
    same = np.zeros(GRID_N, bool)                       # same[i]: row i + 1 shares row i's cell
    same[GRID_SIXTEEN[0]:GRID_SIXTEEN[1] - 1] = True
    if distinct:
        same[GRID_EQUAL[0]:GRID_EQUAL[1] - 1] = (np.arange(GRID_EQUAL[0], GRID_EQUAL[1] - 1) - GRID_EQUAL[0]) % 16 != 15
    else:
        same[GRID_EQUAL[0]:GRID_EQUAL[1] - 1] = True
    gap = np.zeros(GRID_N, np.int64)
    for i, g in GRID_GAPS.items():
        assert not same[i]
        gap[i] = g
    ncell = 2 * GRID_N + 1
    free = (ncell - 1) - int((~same[:-1]).sum()) - int(gap.sum())      # cells still to lose to single gaps
    assert free >= 0
    fill = [i for i in range(GRID_N - 1) if i % 2 == 1 and i not in GRID_GAPS and not GRID_EQUAL[0] <= i < GRID_SIXTEEN[1]][:free]
    assert len(fill) == free
    gap[fill] = 1
    cell = np.zeros(GRID_N, np.int64)
    for i in range(GRID_N - 1):
        cell[i + 1] = cell[i] if same[i] else cell[i] + 1 + gap[i]
    off = (np.arange(GRID_N) * 7) % 16                                   # first and last coordinates of cells among them
    off[0], off[-1] = 0, 15
    off[GRID_SIXTEEN[0]:GRID_SIXTEEN[1]] = np.arange(16)
    if distinct:
        off[GRID_EQUAL[0]:GRID_EQUAL[1]] = (np.arange(GRID_EQUAL[1] - GRID_EQUAL[0])) % 16
    else:
        off[GRID_EQUAL[0]:GRID_EQUAL[1]] = 9
    v = GRID_ORIGIN + cell * 16 + off
    return v.astype(np.int32), cell


def grid_probes(seed=16):
    """every coordinate from origin - 3 to origin + span + 3 as a point query, then 4000 ranges from a cell's first or
    last coordinate to a cell's first or last coordinate -> (start, end)"""
    rng = np.random.default_rng(seed)
    x = np.arange(GRID_ORIGIN - 3, GRID_ORIGIN + GRID_SPAN + 4)
    c1 = rng.integers(0, 2 * GRID_N + 1, 4000)
    c2 = np.minimum(c1 + rng.integers(0, 200, 4000) * (rng.random(4000) < 0.8), 2 * GRID_N)
    rs = GRID_ORIGIN + c1 * 16 + 15 * rng.integers(0, 2, 4000)
    re = GRID_ORIGIN + c2 * 16 + 15 * rng.integers(0, 2, 4000)
    re = np.maximum(re, rs)                                              # (same cell, last then first coordinate: a point on the last)
    return np.concatenate([x, rs]).astype(np.int32), np.concatenate([x, re]).astype(np.int32)


def extremes_table(seed=17):
    """7 keys: 0, 2 and 6 empty, key 1 holds INT32_MIN and INT32_MAX (as starts and as ends), key 3 a single row, key 4
    1500 equal rows, key 5 ordinary rows; shuffled.  Probe keys go beyond the build's"""
    rng = np.random.default_rng(seed)
    k1s = np.array([LO, LO, -5, HI - 2, HI, LO + 1, 100], np.int64); k1e = np.array([LO, LO + 3, 7, HI, HI, LO + 1, 200], np.int64)
    r1s = rng.integers(LO, HI - 2**20, 60); r1e = r1s + rng.integers(0, 2**20, 60)
    r5s = rng.integers(-3000, 3000, 200); r5e = r5s + rng.integers(0, 40, 200)
    bk = np.concatenate([np.full(len(k1s) + 60, 1), [3], np.full(1500, 4), np.full(200, 5)]).astype(np.uint32)
    bs = np.concatenate([k1s, r1s, [77], np.full(1500, 1000), r5s])
    be = np.concatenate([k1e, r1e, [79], np.full(1500, 1010), r5e])
    o = rng.permutation(len(bk))
    # probes: the corners on every key (0..9), then random rows
    cs = np.array([LO, LO, LO, HI, HI - 1, -5, 0, 1000, 1010, 1011, 999, 77, 79, 80, LO + 1, HI - 2], np.int64)
    ce = np.array([LO, HI, LO + 1, HI, HI, 7, HI, 1000, 1010, HI, 999, 77, 79, 90, LO + 3, HI - 1], np.int64)
    pk = np.repeat(np.arange(10), len(cs)).astype(np.uint32)
    ps, pe = np.tile(cs, 10), np.tile(ce, 10)
    qk, qs, qe = _probes(rng, 8, LO, HI - 2**22, 2000, 2**22)
    tk, ts, te = _probes(rng, 8, -4000, 4000, 2000, 60)
    return dict(bk=bk[o], bs=bs[o].astype(np.int32), be=be[o].astype(np.int32), nkeys=7,
                probes=(np.concatenate([pk, qk, tk]), np.concatenate([ps, qs, ts]).astype(np.int32), np.concatenate([pe, qe, te]).astype(np.int32)))


def tiny_table(n):
    """0 rows or 1 row over 3 keys"""
    bk = np.array([1], np.uint32)[:n]; bs = np.array([40], np.int32)[:n]; be = np.array([44], np.int32)[:n]
    pk = np.array([0, 1, 1, 1, 1, 2, 3], np.uint32); ps = np.array([40, 39, 40, 44, 45, 40, 40], np.int32); pe = np.array([44, 40, 44, 50, 50, 44, 44], np.int32)
    return dict(bk=bk, bs=bs, be=be, nkeys=3, probes=(pk, ps, pe))


def routing_table(nfull, wide, seed=18):
    """5 unsorted rows for each of the first `nfull` of 1030 keys (1023 keys with rows leave a routing view, 1024 do not).
    wide=False: every key's starts span less than one 2^10 cell (one region a key); wide=True: spans of several cells
    that differ from key to key, so that regions hold 2^cs cells with cs > 0"""
    rng = np.random.default_rng(seed)
    bk = np.repeat(np.arange(nfull), 5).astype(np.uint32)
    width = (3000 + (bk % 7) * 3000) if wide else np.full(len(bk), 900)
    bs = 10_000 + (rng.random(len(bk)) * width).astype(np.int64)
    bs[0::5] = 10_000; bs[1::5] = 10_000 + width[1::5] - 1                # every key takes its whole span
    be = bs + rng.integers(0, 120, len(bk))
    o = rng.permutation(len(bk))
    pk, ps, pe = _probes(rng, 1030, 9_000, 32_000 if wide else 11_500, 6000, 150)
    return dict(bk=bk[o], bs=bs[o].astype(np.int32), be=be[o].astype(np.int32), nkeys=1030, probes=(pk, ps, pe))


# ---------------------------------------------------------------------------------------------------- coverage probe

COV_NODES, COV_STEP, COV_LENS = 400, 100, (0, 1, 2, 37, 98)


def coverage_nodes():
    """400 disjoint nodes 100 apart with lengths cycling through 0, 1, 2, 37 and 98 (none touches its successor)"""
    first = np.arange(COV_NODES) * COV_STEP
    last = first + np.tile(COV_LENS, COV_NODES // len(COV_LENS))
    return np.zeros(COV_NODES, np.uint32), first.astype(np.int32), last.astype(np.int32)


def coverage_queries():
    """from last[a] + {-2..2} to first[a + c] + {-2..2}, c = 0..5, for ten nodes a: 1500 queries that overlap 0..6 nodes,
    ends on, next to and between the nodes' ends.  Three overlapped nodes are where the probe goes over from adding the
    nodes' terms to prefix sums"""
    _, first, last = coverage_nodes()
    qs, qe = [], []
    for a in range(20, 30):
        for c in range(6):
            for ds in range(-2, 3):
                for de in range(-2, 3):
                    qs.append(int(last[a]) + ds); qe.append(int(first[a + c]) + de)
    return np.zeros(len(qs), np.uint32), np.array(qs, np.int32), np.array(qe, np.int32)


def coverage_edge_queries():
    """queries with start == INT32_MIN or end == INT32_MAX over hundreds of the nodes"""
    _, first, last = coverage_nodes()
    s = [LO, LO, LO, LO, 0, int(last[5]), int(last[5]) + 1, int(first[390]), LO, LO + 1, LO]
    e = [HI, int(first[399]), int(last[200]), -1, HI, HI, HI, HI, int(first[0]), HI, HI - 1]
    return np.zeros(len(s), np.uint32), np.array(s, np.int32), np.array(e, np.int32)


def wide_nodes():
    """nodes wider than 2^31 and sums that wrap: [MIN, 5], [10, MAX - 10], [MAX - 5, MAX] with [MIN, MAX], [0, MAX - 1],
    [-100, MAX - 7] (a wrapped, negative sum) and [MIN + 1, MAX - 1]"""
    bk = np.zeros(3, np.uint32); bs = np.array([LO, 10, HI - 5], np.int32); be = np.array([5, HI - 10, HI], np.int32)
    pk = np.zeros(4, np.uint32); ps = np.array([LO, 0, -100, LO + 1], np.int32); pe = np.array([HI, HI - 1, HI - 7, HI - 1], np.int32)
    return dict(bk=bk, bs=bs, be=be, nkeys=1, probes=(pk, ps, pe))


# ---------------------------------------------------------------------------------------------------- strict wrap, launch edges, k

def strict_wrap_table():
    """a few rows at and between the int32 extremes over keys 1, 3 and 5 of 6, and probe rows with start == INT32_MAX and
    with end == INT32_MIN: under strict start + 1 and end - 1 wrap"""
    bk = np.array([1, 1, 1, 1, 1, 3, 3, 5], np.uint32)
    bs = np.array([LO, LO + 5, -3, HI - 9, HI, 7, 7, 0], np.int32); be = np.array([LO + 2, LO + 9, 4, HI - 1, HI, 7, 9, 0], np.int32)
    ps = np.array([HI, HI, LO, 0, LO, HI - 1, HI, LO, LO + 1, 7, 6, HI, LO], np.int64)
    pe = np.array([HI, LO, LO, HI, HI, HI, HI - 1, LO + 1, LO + 1, 7, 10, 5, -5], np.int64)
    pk = np.repeat(np.arange(7), len(ps)).astype(np.uint32)
    return dict(bk=bk, bs=bs, be=be, nkeys=6, probes=(pk, np.tile(ps, 7).astype(np.int32), np.tile(pe, 7).astype(np.int32)))


BATCH_SIZES = (1, 7, 8, 9, 255, 256, 257, 1025)          # around the routed kernels' eighths, a workgroup and its grid stride


def wave_key_batches():
    """nearest k = 1 probe batches of 192 rows over cut_table's keys: the key changes exactly at row 64 (every wavefront
    has one key); exactly one lane of the second wavefront has another key"""
    rng = np.random.default_rng(19)
    ps = rng.integers(0, 400_000, 192).astype(np.int32); pe = (ps + rng.integers(0, 200, 192)).astype(np.int32)
    a = np.zeros(192, np.uint32); a[64:] = 2
    b = np.ones(192, np.uint32); b[64 + 37] = 0
    return {"change_at_64": (a, ps, pe), "one_lane": (b, ps, pe)}


def small_nearest_table():
    """key 0: five rows that all overlap [10, 20]; key 2: three rows; key 1 empty"""
    bk = np.array([0, 2, 0, 0, 2, 0, 0, 2], np.uint32)
    bs = np.array([5, 100, 10, 10, 50, 15, 20, 100], np.int32); be = np.array([12, 120, 10, 30, 60, 15, 25, 110], np.int32)
    pk = np.array([0, 0, 0, 2, 2, 1, 3, 0], np.uint32); ps = np.array([10, 0, 40, 70, 100, 5, 5, 13], np.int32); pe = np.array([20, 3, 45, 80, 100, 9, 9, 14], np.int32)
    return dict(bk=bk, bs=bs, be=be, nkeys=3, probes=(pk, ps, pe))
