"""CPU restatements of ivx_intersect (include/ivx.h): the pieces of every left row that the right side's merged runs cover.

    walk(left, right, strict)          (a) plain Python: merges the right side itself, walks the runs per left row
    from_oracle(left, right, strict)   (b) the oracle's merge of the right side, the oracle's overlap pairs of the left rows
                                           against those runs, each pair clipped, ordered by (sorted left position, ms)

Both -> (key u32, start i64, end i64, left row u32) in the contract's order: left rows by (key, start, end, input row), pieces
ascending within a row.  left / right: (key, start, end) columns; rows with end < start are the caller's to avoid (the
device call refuses them).  (b) goes through the oracle's int32 join, so it takes coordinates that fit int32 only; the CPU
tests hold the two against each other."""
import numpy as np

from oracle import oracle as orc


def _out(rows):
    if not rows:
        return np.empty(0, np.uint32), np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, np.uint32)
    k, s, e, r = zip(*rows)
    return np.array(k, np.uint32), np.array(s, np.int64), np.array(e, np.int64), np.array(r, np.uint32)


def left_order(left):
    """the input rows of the left side in (key, start, end, input row) order"""
    k, s, e = (np.asarray(c) for c in left)
    return np.lexsort((np.arange(len(s)), e, s, k))


def merged_runs(right, strict):
    """{key: [(ms, me), ...]} by the merge rule with min_dist = 0: a row joins the current run iff rs < cur_end (strict) or
    rs <= cur_end (weak)"""
    k, s, e = ([int(x) for x in np.asarray(c).tolist()] for c in right)
    runs = {}
    for kk, ss, ee in sorted(zip(k, s, e)):
        cur = runs.setdefault(kk, [])
        if cur and (ss < cur[-1][1] if strict else ss <= cur[-1][1]):
            cur[-1][1] = max(cur[-1][1], ee)
        else:
            cur.append([ss, ee])
    return runs


def walk(left, right, strict=False):
    # (every run of the row's key is tested against the predicate -- no search, no assumption that the runs' ends ascend --
    #  with the runs of a key as two int64 arrays, so that a few thousand rows against a few thousand runs stay quick)
    runs = {kk: (np.array([r[0] for r in v], np.int64), np.array([r[1] for r in v], np.int64)) for kk, v in merged_runs(right, strict).items()}
    k, s, e = ([int(x) for x in np.asarray(c).tolist()] for c in left)
    rows = []
    for i in left_order(left).tolist():
        if k[i] not in runs:
            continue
        ms, me = runs[k[i]]
        hit = (ms < e[i]) & (me > s[i]) if strict else (ms <= e[i]) & (me >= s[i])
        for j in np.flatnonzero(hit).tolist():
            rows.append((k[i], max(s[i], int(ms[j])), min(e[i], int(me[j])), i))
    return _out(rows)


def from_oracle(left, right, strict=False):
    lk, ls, le = np.asarray(left[0], np.uint32), np.asarray(left[1], np.int64), np.asarray(left[2], np.int64)
    if len(ls) == 0 or len(right[1]) == 0:
        return _out([])
    mk, ms, me, _ = orc.merge(*right, min_dist=0, strict=strict)
    wb, wp = orc.join(mk, ms, me, lk, ls, le)                           # weak pairs (run, left row)
    wb, wp = wb.astype(np.int64), wp.astype(np.int64)
    if strict:                                                          # the strict pairs are the weak ones that also overlap strictly
        keep = (ms[wb] < le[wp]) & (me[wb] > ls[wp])
        wb, wp = wb[keep], wp[keep]
    order = left_order(left)
    pos = np.empty(len(ls), np.int64)
    pos[order] = np.arange(len(ls))
    o = np.lexsort((ms[wb], pos[wp]))
    wb, wp = wb[o], wp[o]
    return (lk[wp].astype(np.uint32), np.maximum(ls[wp], ms[wb]), np.minimum(le[wp], me[wb]), wp.astype(np.uint32))


def random_sides(rng, nl, nr, nkeys, span=40, max_len=9, p_empty=0.25):
    """seeded small-coordinate sides with start <= end, rows of start == end included: -> (left, right) as (key, start, end)"""
    def side(n):
        k = rng.integers(0, nkeys, n).astype(np.uint32)
        s = rng.integers(0, span, n).astype(np.int64)
        ln = rng.integers(0, max_len, n).astype(np.int64)
        ln[rng.random(n) < p_empty] = 0
        return k, s, s + ln
    return side(nl), side(nr)


def tiles(ls, le, parts):
    """do the (start, end) parts, sorted, chain from ls to le?  (a row with ls == le may have none)"""
    parts = sorted(parts)
    if not parts:
        return ls == le
    if parts[0][0] != ls or parts[-1][1] != le:
        return False
    return all(parts[j][1] == parts[j + 1][0] for j in range(len(parts) - 1))


def check_tiling(left, isect, sub):
    """every left row's intersect pieces and subtract fragments together tile [ls, le]; isect / sub: (key, start, end, row)"""
    per = {}
    for _, s, e, r in (isect, sub):
        for ss, ee, rr in zip(np.asarray(s).tolist(), np.asarray(e).tolist(), np.asarray(r).tolist()):
            per.setdefault(rr, []).append((ss, ee))
    ls, le = np.asarray(left[1]).tolist(), np.asarray(left[2]).tolist()
    bad = [i for i in range(len(ls)) if not tiles(ls[i], le[i], per.get(i, []))]
    return bad
