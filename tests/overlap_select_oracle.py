"""CPU restatement of ivx_probe_overlap_select (include/ivx_select.h), built from the oracle's own pairs: orc.join gives M(i),
a numpy lexsort on (probe row, +-criterion, build row) orders every probe row's matches best first and the first of each
group is the winner.

    select(build, probe, by, val=None) -> (build_idx u32[n], score i64[n])      NULL_IDX / 0 where M(i) is empty

brute() is an independent O(n * m) restatement in Python integers, for tiny inputs; the CPU tests hold the two against each
other."""
import numpy as np

from oracle import oracle as orc

BY = ("min_val", "max_val", "max_overlap", "min_overlap", "first_row", "last_row")
LARGEST = ("max_val", "max_overlap", "last_row")
NULL_IDX = 0xFFFFFFFF


def empty(n):
    """the result of n rows without a match"""
    return np.full(n, NULL_IDX, np.uint32), np.zeros(n, np.int64)


def criterion(b, p, by, val, wb, wp):
    """c(b, i) of the pairs (build row wb[j], probe row wp[j]) as int64"""
    if by in ("min_val", "max_val"):
        return np.asarray(val).astype(np.int64)[wb]                     # (int32 values: sign-extended)
    if by in ("max_overlap", "min_overlap"):
        bs, be = np.asarray(b[1], np.int64)[wb], np.asarray(b[2], np.int64)[wb]
        qs, qe = np.asarray(p[1], np.int64)[wp], np.asarray(p[2], np.int64)[wp]
        return np.minimum(qe, be) - np.maximum(qs, bs) + 1              # int64, no clamp
    assert by in ("first_row", "last_row"), by
    return wb.copy()


def from_pairs(b, p, by, val, wb, wp):
    n = len(p[1])
    idx, score = empty(n)
    if len(wb) == 0:
        return idx, score
    wb, wp = np.asarray(wb, np.int64), np.asarray(wp, np.int64)
    c = criterion(b, p, by, val, wb, wp)
    # best first inside a probe row: the criterion ascending -- for the "largest" criteria its order reversed, which for
    # int64 is the bitwise complement (-c would overflow at INT64_MIN) -- then the build row ascending
    order = np.lexsort((wb, ~c if by in LARGEST else c, wp))
    first = np.ones(len(order), bool)
    first[1:] = wp[order][1:] != wp[order][:-1]
    win = order[first]
    idx[wp[win]] = wb[win].astype(np.uint32)
    score[wp[win]] = c[win]
    return idx, score


def select(b, p, by, val=None, threads=4):
    wb, wp = orc.join(*b, *p, threads=threads)
    return from_pairs(b, p, by, val, wb, wp)


def brute(b, p, by, val=None):
    """O(n * m), Python integers: same key (a key only the probe side has matches nothing), bs <= qe and be >= qs"""
    n = len(p[1])
    idx, score = empty(n)
    bk, bs, be = [np.asarray(c).tolist() for c in b]
    pk, ps, pe = [np.asarray(c).tolist() for c in p]
    vals = None if val is None else np.asarray(val).tolist()
    for i in range(n):
        best = None                                                     # (criterion, build row)
        for j in range(len(bs)):
            if bk[j] == pk[i] and bs[j] <= pe[i] and be[j] >= ps[i]:
                if by in ("min_val", "max_val"):
                    c = vals[j]
                elif by in ("max_overlap", "min_overlap"):
                    c = min(pe[i], be[j]) - max(ps[i], bs[j]) + 1
                else:
                    c = j
                # rows come in ascending order: a later row wins only when strictly better
                if best is None or (c > best[0] if by in LARGEST else c < best[0]):
                    best = (c, j)
        if best is not None:
            idx[i], score[i] = best[1], best[0]
    return idx, score
