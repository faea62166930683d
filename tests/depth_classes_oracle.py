"""CPU restatements of the depth coverage classes (include/ivx.h ivx_depth_profile_quantize / _hist) for the tests.

All take the steps form of tests/depth_per_base_oracle.py, st = (key u32, pos u32, coverage i32, key_seen); the number of
keys is len(key_seen).  quantize_* return (key u32, start u32, end u32, class u32) ordered by (key, start); hist_* return
int64 [n_keys, n_bins].

  quantize_loop / hist_loop    per position: depth_regions_oracle.values over the key's whole domain, every value classified
                               or binned on its own, run-length coded in plain Python.  Small domains only.
  quantize_steps / hist_steps  vectorised over steps: the domain's break points are its start and the steps inside it; np.
                               searchsorted on the cuts, np.diff on the classes, np.add.at for the bins.

The two of an operation share nothing but the clipping rule (depth_regions_oracle.clip) and are checked against each other,
against the reference's pinned per-base rows and against summarize_prefix in tests/test_depth_classes_cpu.py.
"""
import numpy as np

import depth_regions_oracle as dro

U32_MAX = 0xFFFFFFFF


def domain(st, k, pos_lo, key_hi, seen_only):
    """-> (lo, hi) of key k, or None when the key does not take part or its domain is empty"""
    if seen_only and not st[3][k]:
        return None
    r = dro.clip(np.array([k], np.uint32), [0], [U32_MAX], 0, pos_lo, key_hi)
    return None if r is None else (r[1], r[2])


def full_mask(n_cuts):
    return (1 << (n_cuts + 1)) - 1


def _rows(rows):
    a = np.array(rows, np.int64).reshape(-1, 4)
    return tuple(a[:, j].astype(np.uint32) for j in range(4))


# ------------------------------------------------------------------------------------------------ per position
def quantize_loop(st, cuts, emit_mask=None, pos_lo=0, key_hi=None, skip_pos0=False, seen_only=False):
    cuts = [int(c) for c in cuts]
    mask = full_mask(len(cuts)) if emit_mask is None else int(emit_mask)
    rows = []
    for k in range(len(st[3])):
        d = domain(st, k, pos_lo, key_hi, seen_only)
        if d is None:
            continue
        lo, hi = d
        cls = [sum(1 for c in cuts if c <= int(v)) for v in dro.values(st, k, lo, hi - lo + 1, skip_pos0)]
        start = 0
        for i in range(1, len(cls) + 1):
            if i == len(cls) or cls[i] != cls[start]:
                if (mask >> cls[start]) & 1:
                    rows.append((k, lo + start, lo + i - 1, cls[start]))
                start = i
    return _rows(rows)


def hist_loop(st, v_lo=0, n_bins=256, pos_lo=0, key_hi=None, skip_pos0=False, seen_only=False):
    nk = len(st[3])
    h = np.zeros((nk, n_bins), np.int64)
    for k in range(nk):
        d = domain(st, k, pos_lo, key_hi, seen_only)
        if d is None:
            continue
        for v in dro.values(st, k, d[0], d[1] - d[0] + 1, skip_pos0):
            h[k, min(max(int(v) - int(v_lo), 0), n_bins - 1)] += 1
    return h


# ------------------------------------------------------------------------------------------------ over steps
def segments(st, k, lo, hi, skip_pos0):
    """the domain [lo, hi] of key k cut at the key's steps -> (start, end, v) int64, every segment at least one base"""
    p, v = dro.key_steps(st, k, skip_pos0)
    b = np.concatenate([[lo], p[(p > lo) & (p <= hi)]]).astype(np.int64)
    e = np.concatenate([b[1:] - 1, [hi]]).astype(np.int64)
    j = np.searchsorted(p, b, side="right") - 1
    val = np.where(j >= 0, v[np.maximum(j, 0)] if len(v) else 0, 0).astype(np.int64)
    return b, e, val


def quantize_steps(st, cuts, emit_mask=None, pos_lo=0, key_hi=None, skip_pos0=False, seen_only=False):
    cuts = np.asarray(cuts, np.int64).reshape(-1)
    mask = full_mask(len(cuts)) if emit_mask is None else int(emit_mask)
    out = [[], [], [], []]
    for k in range(len(st[3])):
        d = domain(st, k, pos_lo, key_hi, seen_only)
        if d is None:
            continue
        b, e, val = segments(st, k, d[0], d[1], skip_pos0)
        cls = np.searchsorted(cuts, val, side="right")
        head = np.concatenate([[True], np.diff(cls) != 0])
        tail = np.concatenate([head[1:], [True]])
        s, t, c = b[head], e[tail], cls[head]
        keep = ((mask >> c) & 1) == 1
        for o, a in zip(out, (np.full(int(keep.sum()), k), s[keep], t[keep], c[keep])):
            o.append(a)
    return tuple(np.concatenate(o).astype(np.uint32) if o else np.zeros(0, np.uint32) for o in out)


def hist_steps(st, v_lo=0, n_bins=256, pos_lo=0, key_hi=None, skip_pos0=False, seen_only=False):
    nk = len(st[3])
    h = np.zeros((nk, n_bins), np.int64)
    for k in range(nk):
        d = domain(st, k, pos_lo, key_hi, seen_only)
        if d is None:
            continue
        b, e, val = segments(st, k, d[0], d[1], skip_pos0)
        np.add.at(h[k], np.clip(val - int(v_lo), 0, n_bins - 1), e - b + 1)
    return h


def domain_sizes(st, pos_lo=0, key_hi=None, seen_only=False):
    """|D(k)| per key, 0 for a key that does not take part"""
    out = np.zeros(len(st[3]), np.int64)
    for k in range(len(st[3])):
        d = domain(st, k, pos_lo, key_hi, seen_only)
        if d is not None:
            out[k] = d[1] - d[0] + 1
    return out
