"""CPU restatement of depth() for the tests: coverage blocks from reads with packed binary CIGARs and from weighted
segments, as include/ivx.h pins them for ivx_depth.

The reference (bio-function-pileup) cannot be run here (no Rust toolchain), so parity rests on two independent
restatements of its cited lines that must agree with each other and with the reference's own pinned tables
(tests/golden/pileup_golden.json):

  depth_loop   plain loops: the serial CIGAR walk with saturating adds (cigar.rs:234-254), the read filter
               (events.rs:111-137, filter.rs:31-33), the dense mode's bounds (cigar.rs:177-228: a depth array of
               len + 1 slots), and the serial block walk of events_to_coverage_blocks (coverage.rs:25-65)
  depth_numpy  vectorised, in the change-point form: segmented cumulative sums over the ops, lexsort of the events,
               sums per distinct position, running sum per key, blocks between consecutive change points

Columns are those of the C ABI: rkey/rpos/rflags/rmapq per read, cigar_offsets in BYTES into the u32 ops array,
skey/sstart/send/sweight per segment, key_len per key or None.
"""
import json
import os

import numpy as np

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pileup_golden.json")

NULL_IDX = 0xFFFFFFFF
U32_MAX = 0xFFFFFFFF
EMITS = (0, 7, 8)          # M = X
SKIPS = (2, 3)             # D N


def _wrap32(x):
    """int32 wrap-around of a Python int"""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


def pack_reads(reads):
    """[(key, pos, flags, mapq, [ops])] -> dict of the ABI's read columns"""
    n = len(reads)
    off = np.zeros(n + 1, np.int32)
    ops = []
    for i, r in enumerate(reads):
        ops.extend(r[4])
        off[i + 1] = 4 * len(ops)
    return dict(rkey=np.array([r[0] for r in reads], np.uint32), rpos=np.array([r[1] for r in reads], np.uint32),
                rflags=np.array([r[2] for r in reads], np.uint32), rmapq=np.array([r[3] for r in reads], np.uint32),
                cigar_offsets=off, cigar_ops=np.array(ops, np.uint32))


def pack_segments(segs):
    """[(key, start, end, weight)] -> dict of the ABI's segment columns"""
    return dict(skey=np.array([s[0] for s in segs], np.uint32), sstart=np.array([s[1] for s in segs], np.uint32),
                send=np.array([s[2] for s in segs], np.uint32), sweight=np.array([s[3] for s in segs], np.int32))


def events_loop(rkey=None, rpos=None, rflags=None, rmapq=None, cigar_offsets=None, cigar_ops=None,
                skey=None, sstart=None, send=None, sweight=None, key_len=None, filter_flag=1796, min_mapq=0):
    """-> {key: [(position, delta), ...]} in input order, after the filter and the dense mode's bounds"""
    ev = {}

    def add(k, pos, delta):
        if key_len is not None and pos > int(key_len[k]):
            return
        ev.setdefault(k, []).append((pos, delta))

    n_reads = 0 if rpos is None else len(rpos)
    for i in range(n_reads):
        k = 0 if rkey is None else int(rkey[i])
        if k == NULL_IDX:
            continue
        a, b = int(cigar_offsets[i]) // 4, int(cigar_offsets[i + 1]) // 4
        if a == b:
            continue
        if rflags is not None and (int(rflags[i]) & filter_flag) != 0:
            continue
        if rmapq is not None and int(rmapq[i]) < min_mapq:
            continue
        ref = int(rpos[i])
        for w in cigar_ops[a:b]:
            w = int(w)
            ln, code = w >> 4, w & 15
            if code in EMITS:
                add(k, ref, 1)
                ref = min(ref + ln, U32_MAX)
                add(k, ref, -1)
            elif code in SKIPS:
                ref = min(ref + ln, U32_MAX)
    n_seg = 0 if sstart is None else len(sstart)
    for j in range(n_seg):
        k = 0 if skey is None else int(skey[j])
        if k == NULL_IDX:
            continue
        w = 1 if sweight is None else int(sweight[j])
        add(k, int(sstart[j]), w)
        add(k, min(int(send[j]) + 1, U32_MAX), _wrap32(-w))
    return ev


def blocks_of_events(events):
    """coverage.rs:25-65 on one key's [(position, delta)] -> [(start, end, coverage)]"""
    events = sorted(events, key=lambda e: e[0])
    out = []
    cov = prev = 0
    start = 0
    i = 0
    while i < len(events):
        pos = events[i][0]
        while i < len(events) and events[i][0] == pos:
            cov = _wrap32(cov + events[i][1])
            i += 1
        if prev != 0 and cov != prev:
            out.append((start, pos - 1, prev))
            if cov != 0:
                start = pos
        elif prev == 0 and cov != 0:
            start = pos
        prev = cov
    return out


def _as_cols(blocks):
    a = np.array(blocks, np.int64).reshape(-1, 4)
    return a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32), a[:, 3].astype(np.int32)


def depth_loop(**kw):
    """-> (key u32, start u32, end u32, coverage i32), ordered by (key, start)"""
    ev = events_loop(**kw)
    rows = []
    for k in sorted(ev):
        rows += [(k, s, e, c) for s, e, c in blocks_of_events(ev[k])]
    return _as_cols(rows)


def depth_numpy(rkey=None, rpos=None, rflags=None, rmapq=None, cigar_offsets=None, cigar_ops=None,
                skey=None, sstart=None, send=None, sweight=None, key_len=None, filter_flag=1796, min_mapq=0):
    """the same blocks, vectorised (for the large cases)"""
    keys, poss, dels = [], [], []
    n_reads = 0 if rpos is None else len(rpos)
    if n_reads:
        off = np.asarray(cigar_offsets, np.int64) // 4
        nops = np.diff(off)
        ops = np.asarray(cigar_ops, np.uint32)[off[0]:off[-1]].astype(np.int64)
        rk = np.zeros(n_reads, np.int64) if rkey is None else np.asarray(rkey, np.uint32).astype(np.int64)
        keep = (rk != NULL_IDX) & (nops > 0)
        if rflags is not None:
            keep &= (np.asarray(rflags, np.uint32) & np.uint32(filter_flag)) == 0
        if rmapq is not None:
            keep &= np.asarray(rmapq, np.uint32) >= min_mapq
        rid = np.repeat(np.arange(n_reads), nops)
        ln, code = ops >> 4, ops & 15
        emits = np.isin(code, EMITS)
        adv = np.where(emits | np.isin(code, SKIPS), ln, 0)
        incl = np.cumsum(adv)
        ex = incl - adv
        excl = ex - ex[(off[:-1] - off[0])[rid]]                   # reference length before the op, inside its read
        s = np.minimum(np.asarray(rpos, np.uint32).astype(np.int64)[rid] + excl, U32_MAX)
        e = np.minimum(np.asarray(rpos, np.uint32).astype(np.int64)[rid] + excl + ln, U32_MAX)
        m = emits & keep[rid]
        keys += [rk[rid][m], rk[rid][m]]
        poss += [s[m], e[m]]
        dels += [np.ones(m.sum(), np.int64), -np.ones(m.sum(), np.int64)]
    n_seg = 0 if sstart is None else len(sstart)
    if n_seg:
        sk = np.zeros(n_seg, np.int64) if skey is None else np.asarray(skey, np.uint32).astype(np.int64)
        w = np.ones(n_seg, np.int64) if sweight is None else np.asarray(sweight, np.int32).astype(np.int64)
        m = sk != NULL_IDX
        keys += [sk[m], sk[m]]
        poss += [np.asarray(sstart, np.uint32).astype(np.int64)[m], np.minimum(np.asarray(send, np.uint32).astype(np.int64)[m] + 1, U32_MAX)]
        dels += [w[m], -w[m]]
    empty = _as_cols([])
    if not keys:
        return empty
    k, p, d = np.concatenate(keys), np.concatenate(poss), np.concatenate(dels)
    if key_len is not None:
        m = p <= np.asarray(key_len, np.uint32).astype(np.int64)[k]
        k, p, d = k[m], p[m], d[m]
    if len(k) == 0:
        return empty
    o = np.lexsort((p, k))
    k, p, d = k[o], p[o], d[o]
    head = np.r_[True, (k[1:] != k[:-1]) | (p[1:] != p[:-1])]     # first event of every (key, position) group
    hi = np.flatnonzero(head)
    wrap = lambda x: ((x + (1 << 31)) % (1 << 32)) - (1 << 31)
    g = wrap(np.add.reduceat(d, hi))
    gk, gp = k[hi], p[hi]
    cs = np.cumsum(g)
    khead = np.r_[True, gk[1:] != gk[:-1]]
    base = np.maximum.accumulate(np.where(khead, np.arange(len(g)), 0))
    c = wrap(cs - (cs - g)[base])                                   # running sum inside the key
    cp = np.flatnonzero(g != 0)                                     # change points
    if len(cp) < 2:
        return empty
    a, b = cp[:-1], cp[1:]
    m = (c[a] != 0) & (gk[a] == gk[b])
    a, b = a[m], b[m]
    return gk[a].astype(np.uint32), gp[a].astype(np.uint32), (gp[b] - 1).astype(np.uint32), c[a].astype(np.int32)


def random_case(rng, n_reads=None, n_seg=None, n_keys=None, clip=None, max_pos=60):
    """a small random input covering every op code, zero-length ops, skipped and filtered reads, clipping and
    negative / zero / INT32_MAX weights -> kwargs of depth_loop / depth_numpy / Ctx.depth"""
    n_keys = int(rng.integers(1, 4)) if n_keys is None else n_keys
    n_reads = int(rng.integers(0, 7)) if n_reads is None else n_reads
    n_seg = int(rng.integers(0, 5)) if n_seg is None else n_seg
    reads = []
    for _ in range(n_reads):
        key = NULL_IDX if rng.random() < 0.1 else int(rng.integers(0, n_keys))
        flags = int(rng.choice([0, 2, 16, 4, 256, 512, 1024, 99]))
        mapq = int(rng.choice([0, 10, 29, 30, 60]))
        nops = int(rng.integers(0, 6))
        ops = [(int(rng.integers(0, 8)) << 4) | int(rng.integers(0, 16)) for _ in range(nops)]
        pos = int(rng.integers(0, max_pos))
        if rng.random() < 0.05:
            pos = U32_MAX - int(rng.integers(0, 12))
        reads.append((key, pos, flags, mapq, ops))
    segs = []
    for _ in range(n_seg):
        key = NULL_IDX if rng.random() < 0.05 else int(rng.integers(0, n_keys))
        s = int(rng.integers(0, max_pos))
        e = s + int(rng.integers(-3, 10))
        e = min(max(e, 0), U32_MAX)
        if rng.random() < 0.05:
            e = U32_MAX
        w = int(rng.choice([1, 1, 2, -1, -3, 0, 0x7FFFFFFF, -0x80000000, 5]))
        segs.append((key, s, e, w))
    kw = dict(filter_flag=1796, min_mapq=int(rng.choice([0, 0, 30])))
    kw.update(pack_reads(reads))
    kw.update(pack_segments(segs))
    if rng.random() < 0.3:
        kw["rflags"] = None
    if rng.random() < 0.3:
        kw["rmapq"] = None
    if rng.random() < 0.2:
        kw["sweight"] = None
    use_clip = (rng.random() < 0.4) if clip is None else clip
    kw["key_len"] = rng.integers(0, max_pos + 10, n_keys).astype(np.uint32) if use_clip else None
    kw["n_keys"] = n_keys
    return kw


def oracle_kw(kw):
    """the arguments of a Ctx.depth call that the restatements take"""
    return {k: v for k, v in kw.items() if k not in ("n_keys", "cap", "outputs")}


# ---- the reference's pinned tables (tests/golden/pileup_golden.json)
def golden_cases():
    with open(GOLDEN_FILE) as f:
        return json.load(f)["cases"]


def case_columns(case):
    """a golden case -> (contig names in byte order, kwargs of the restatements)"""
    names = {r["contig"] for r in case["reads"]} | {s[0] for s in case["segments"]} | set(case["lengths"] or {})
    names = sorted(names, key=lambda s: s.encode())
    ids = {n: i for i, n in enumerate(names)}
    kw = dict(filter_flag=case["filter_flag"], min_mapq=case["min_mapq"])
    kw.update(pack_reads([(ids[r["contig"]], r["pos"], r["flags"], r["mapq"], r["ops"]) for r in case["reads"]]))
    kw.update(pack_segments([(ids[s[0]], s[1], s[2], s[3]) for s in case["segments"]]))
    kw["key_len"] = None if case["lengths"] is None else np.array([case["lengths"][n] for n in names], np.uint32)
    return names, kw


def rows_of(names, out):
    k, s, e, c = out
    return [[names[int(a)], int(b), int(d), int(f)] for a, b, d, f in zip(k, s, e, c)]
