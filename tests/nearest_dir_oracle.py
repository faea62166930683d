"""CPU restatements of ivx_probe_nearest_dir (include/ivx_nearest.h): nearest on one side only and / or within a distance cap.

A (`NearIndex.query`, `nearest_dir`) is the contract, literally: per key the two sorted orders of the reference's index
(by_start = (start, end, row), by_end = (end, start, row), nearest_index.rs:50-55, :77-82) and the running max of ends; per
probe row the overlap stage, then the left cursor going down by_end from partition_point(last < qs) and the right cursor going
up by_start from partition_point(first <= qe), their heads merged by cmp_candidate; IVX_NEAR_BEFORE / IVX_NEAR_AFTER remove a
cursor from the start, and a cap makes a cursor whose head's reported distance exceeds D count as exhausted.  Every probe row
runs that same state machine; numpy only steps all rows at once (one cursor move per row and step), so that 60 000 probe rows
take a fraction of a second.

B (`brute`) is brute force per probe row over all build rows of its key: classify (overlap / before / after, against the
strict-adjusted query), filter by direction, include_overlaps and reported distance <= D, sort by the key the tie order
implies, take k.  It is defined only for probe rows with qs <= qe after the adjustment, over build rows with start <= end
(a build row with end < start can sit on both sides of a query at once, where only the cursors say what happens)."""
import numpy as np

NULL_IDX = 0xFFFFFFFF
DIRECTIONS = ("any", "before", "after")
ALIASES = {"upstream": "before", "downstream": "after"}

_B31 = np.int64(1) << np.int64(31)


def _wrap32(v):
    """int64 values taken back into int32 the way wadd / wsub wrap"""
    return ((v + _B31) & np.int64(0xFFFFFFFF)) - _B31


def _comp(key, v):
    """(key, int32 value) as one int64 that orders like the pair"""
    return (key.astype(np.int64) << np.int64(32)) | (v.astype(np.int64) + _B31)


def _dist(qs, qe, s, e):
    """candidate_distance, nearest_index.rs:252-260"""
    return np.where(qe < s, s - qe, np.where(e < qs, qs - e, 0)).astype(np.int64)


class NearIndex:
    """the reference's NearestIntervalIndex per key, all keys in one array (positions are absolute)"""

    def __init__(self, bkey, bs, be):
        bkey = np.asarray(bkey, np.int64); bs = np.asarray(bs, np.int64); be = np.asarray(be, np.int64)
        row = np.arange(len(bkey), dtype=np.int64)
        o = np.lexsort((row, be, bs, bkey))
        self.sk, self.ss, self.se, self.srow = bkey[o], bs[o], be[o], row[o]
        o = np.lexsort((row, bs, be, bkey))
        self.es, self.ee, self.erow = bs[o], be[o], row[o]
        self.comp_s = _comp(self.sk, self.ss)
        self.comp_e = _comp(bkey[o], self.ee)
        # prefix_max_end per key (:58-63): a later key's composite is above every earlier one, so one running max serves
        self.comp_p = np.maximum.accumulate(_comp(self.sk, self.se)) if len(bkey) else np.zeros(0, np.int64)

    def query(self, pkey, ps, pe, k=1, overlap=True, strict=False, direction="any", max_distance=None):
        """-> (build_rows u32 (NULL_IDX = no answer), probe_rows u32, distance i64 (-1 = no answer)): max(1, found) rows per
        probe row in probe order, the shape of oracle.nearest"""
        direction = ALIASES.get(direction, direction)
        assert direction in DIRECTIONS
        k = int(k)
        n = len(ps)
        K = np.asarray(pkey, np.int64)
        rs = np.asarray(ps, np.int64); re = np.asarray(pe, np.int64)
        qs, qe = (_wrap32(rs + 1), _wrap32(re - 1)) if strict else (rs, re)
        W = max(k, 1)
        out = np.full((n, W), -1, np.int64); outd = np.full((n, W), -1, np.int64)
        found = np.zeros(n, np.int64)
        nb = len(self.sk)
        if k > 0 and nb > 0 and n > 0:
            off = np.searchsorted(self.sk, K, "left"); end = np.searchsorted(self.sk, K, "right")
            pend = np.searchsorted(self.comp_s, _comp(K, qe), "right")       # by_start.partition_point(first <= qe)
            lcur = np.searchsorted(self.comp_e, _comp(K, qs), "left")        # by_end.partition_point(last < qs)
            all_rows = np.arange(n)

            def take(rows, brow, s, e):
                out[rows, found[rows]] = brow
                outd[rows, found[rows]] = _dist(rs[rows], re[rows], s, e)    # reported on the raw coordinates, nearest.rs:367-374
                found[rows] += 1

            if overlap:
                # the overlapping rows in (start, end, row) order: by_start order from the first running max that reaches qs,
                # below pend, those whose end reaches qs.  k = 1 is first_overlap_by_start (:222-234): none when qe < qs
                j = np.maximum(np.searchsorted(self.comp_p, _comp(K, qs), "left"), off)
                ok = (qs <= qe) if k == 1 else np.ones(n, bool)
                while True:
                    a = all_rows[ok & (j < pend) & (found < k)]
                    if not len(a):
                        break
                    ja = j[a]
                    hit = self.se[ja] >= qs[a]
                    take(a[hit], self.srow[ja[hit]], self.ss[ja[hit]], self.se[ja[hit]])
                    j[a] += 1
            li = lcur.copy() if direction != "after" else off.copy()         # a cursor the direction removes is empty from the start
            ri = pend.copy() if direction != "before" else end.copy()
            xl = np.zeros(n, bool); xr = np.zeros(n, bool)                   # exhausted by the cap
            while True:
                hl = (li > off) & ~xl; hr = (ri < end) & ~xr
                lp = np.clip(li - 1, 0, nb - 1); rp = np.clip(ri, 0, nb - 1)
                l_s, l_e, l_row = self.es[lp], self.ee[lp], self.erow[lp]
                r_s, r_e, r_row = self.ss[rp], self.se[rp], self.srow[rp]
                if max_distance is not None:
                    xl |= hl & (_dist(rs, re, l_s, l_e) > max_distance); hl &= ~xl
                    xr |= hr & (_dist(rs, re, r_s, r_e) > max_distance); hr &= ~xr
                act = (found < k) & (hl | hr)
                if not act.any():
                    break
                dl, dr = _dist(qs, qe, l_s, l_e), _dist(qs, qe, r_s, r_e)    # cmp_candidate (:262-266): on the adjusted query
                meta_le = (l_s < r_s) | ((l_s == r_s) & ((l_e < r_e) | ((l_e == r_e) & (l_row <= r_row))))
                left = hl & (~hr | (dl < dr) | ((dl == dr) & meta_le))
                c_s, c_e, c_row = np.where(left, l_s, r_s), np.where(left, l_e, r_e), np.where(left, l_row, r_row)
                li -= (act & left); ri += (act & ~left)
                skip = np.zeros(n, bool) if (overlap or k == 1) else _dist(qs, qe, c_s, c_e) == 0    # :182-184 (nearest_k only)
                seen = (out == c_row[:, None]).any(axis=1)                   # :186
                t = all_rows[act & ~skip & ~seen]
                take(t, c_row[t], c_s[t], c_e[t])
        cnt = np.maximum(found, 1)
        probe = np.repeat(np.arange(n, dtype=np.int64), cnt)
        slot = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        b = out[probe, slot]; d = outd[probe, slot]
        return np.where(b < 0, NULL_IDX, b).astype(np.uint32), probe.astype(np.uint32), d


def nearest_dir(bkey, bs, be, pkey, ps, pe, k=1, overlap=True, strict=False, direction="any", max_distance=None):
    """A, one call"""
    return NearIndex(bkey, bs, be).query(pkey, ps, pe, k=k, overlap=overlap, strict=strict, direction=direction, max_distance=max_distance)


def brute(bkey, bs, be, pkey, ps, pe, k=1, overlap=True, strict=False, direction="any", max_distance=None):
    """B -> {probe row: [(build row, reported distance), ...]} for the probe rows it is defined for (qs <= qe after the
    adjustment); an empty list is the NULL row"""
    direction = ALIASES.get(direction, direction)
    assert direction in DIRECTIONS
    bkey = np.asarray(bkey, np.int64); bs = np.asarray(bs, np.int64); be = np.asarray(be, np.int64)
    assert (bs <= be).all()
    by_key = {}
    for kk in np.unique(bkey):
        rows = np.flatnonzero(bkey == kk)
        by_key[int(kk)] = (rows, bs[rows], be[rows])
    res = {}
    for i in range(len(ps)):
        rs, re = int(ps[i]), int(pe[i])
        qs, qe = (int(_wrap32(np.int64(rs + 1))), int(_wrap32(np.int64(re - 1)))) if strict else (rs, re)
        if qs > qe:
            continue
        cands = []
        rows, s_, e_ = by_key.get(int(pkey[i]), ((), (), ()))
        for row, s, e in zip(rows, s_, e_):
            row, s, e = int(row), int(s), int(e)
            raw = s - re if re < s else (rs - e if e < rs else 0)
            if s <= qe and e >= qs:                                         # overlap: first, in (start, end, row) order
                if overlap:
                    cands.append(((0, 0, 0, s, e, row), row, raw))
                continue
            side = 0 if e < qs else 1                                       # before / after the adjusted query
            if (side == 0 and direction == "after") or (side == 1 and direction == "before"):
                continue
            if max_distance is not None and raw > max_distance:
                continue
            adj = qs - e if side == 0 else s - qe
            # nearer first; left before right at equal distance; left rows of equal end: larger start, then larger row;
            # right rows (of equal start, then): (end, row)
            cands.append(((1, adj, side) + ((-s, -row, 0) if side == 0 else (s, e, row)), row, raw))
        cands.sort()
        res[i] = [(row, raw) for _, row, raw in cands[:int(k)]]
    return res
