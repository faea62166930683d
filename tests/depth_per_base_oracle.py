"""CPU restatements of per-base depth() for the tests, both built on depth_oracle.events_loop.

  per_base_dense  the reference's form (bio-function-pileup events.rs:181-206, coverage.rs:271-365): per contig a delta array
                  of len + 1 slots, touched iff an event landed in it; the emitter walks index [0, len) (zero_based) or
                  [1, len + 1) -- never adding slot 0 -- with a wrapping int32 running sum, emitted `as i16`
  steps           the form include/ivx.h pins for a depth profile: per key the positions whose summed delta is not 0, with
                  the running sum from there on, plus key_seen; expand_steps() evaluates a window of it

The reference cannot be run here (no Rust toolchain): parity rests on the two agreeing with each other on random inputs and
with the reference's own pinned tables (tests/golden/pileup_per_base_golden.json).
"""
import json
import os

import numpy as np

import depth_oracle as orc

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pileup_per_base_golden.json")
REFERENCE_ERROR = ("per_base mode requires dense accumulation (BAM header with contig lengths). "
                   "Sparse fallback (e.g. MemTable) is not supported for per_base output.")


def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def emit_dense(depth, zero_based):
    """PerBaseEmitter over one delta array (coverage.rs:294-335) -> (positions int32, coverage int16)"""
    n = len(depth)
    lo, hi = (0, n - 1) if zero_based else (1, n)
    pos, cov = [], []
    c = 0
    for idx in range(lo, hi):
        c = orc._wrap32(c + int(depth[idx]))
        pos.append(idx)
        cov.append(c)
    return np.array(pos, np.int64).astype(np.int32), np.array(cov, np.int64).astype(np.int16)


def per_base_dense(zero_based, n_keys, **kw):
    """-> {key: (positions int32, coverage int16)} for every touched key; kw as depth_oracle.events_loop, key_len required"""
    key_len = kw["key_len"]
    ev = orc.events_loop(**kw)
    out = {}
    for k in sorted(ev):
        depth = [0] * (int(key_len[k]) + 1)
        for p, d in ev[k]:
            depth[p] = orc._wrap32(depth[p] + d)
        out[k] = emit_dense(depth, zero_based)
    return out


def steps(n_keys, **kw):
    """-> (key u32, pos u32, coverage i32, key_seen u8[n_keys]) ordered by (key, position)"""
    ev = orc.events_loop(**kw)
    seen = np.zeros(n_keys, np.uint8)
    rows = []
    for k in sorted(ev):
        seen[k] = 1
        g = {}
        for p, d in ev[k]:
            g[p] = orc._wrap32(g.get(p, 0) + d)
        c = 0
        for p in sorted(g):
            if g[p] != 0:
                c = orc._wrap32(c + g[p])
                rows.append((k, p, c))
    a = np.array(rows, np.int64).reshape(-1, 3)
    return a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint32), a[:, 2].astype(np.int32), seen


def expand_steps(st, key, first_pos, n, skip_pos0=False):
    """a window of the steps form -> (positions int32, coverage int16), as ivx_depth_profile_expand defines it"""
    k, p, c, _ = st
    m = k == key
    p, c = p[m].astype(np.int64), c[m].astype(np.int64)
    c0 = int(c[0]) if (skip_pos0 and len(p) and p[0] == 0) else 0
    q = first_pos + np.arange(n, dtype=np.int64)
    j = np.searchsorted(p, q, side="right") - 1
    cov = np.where(j >= 0, c[np.maximum(j, 0)] if len(c) else 0, 0) - c0
    return q.astype(np.uint32).view(np.int32), cov.astype(np.uint32).astype(np.uint16).view(np.int16)


def per_base_steps(zero_based, n_keys, **kw):
    """the steps form emitted like the reference: every seen key over [0, len) or [1, len + 1) with skip_pos0"""
    st = steps(n_keys, **kw)
    out = {}
    for k in range(n_keys):
        if st[3][k]:
            L = int(kw["key_len"][k])
            out[k] = expand_steps(st, k, 0 if zero_based else 1, L, skip_pos0=not zero_based)
    return out
