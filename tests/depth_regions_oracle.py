"""CPU restatements of the depth region summaries (include/ivx.h ivx_depth_profile_summarize / _windows) for the tests.

Both take the steps form of tests/depth_per_base_oracle.py, st = (key u32, pos u32, coverage i32, key_seen), and return
(bases int64[n], sum int64[n], ge int64[n_thr, n]):

  summarize_loop    per position: the value of every base of the clipped region by depth_per_base_oracle.expand_steps's
                    lookup, widened to int32 (no Int16 cast), then plain Python sums and comparisons.  Small regions only.
  summarize_prefix  vectorised: per key the cumulative v * length (and, per threshold, the cumulative length where
                    v >= threshold) up to every step, two searchsorted lookups per region, F(end + 1) - F(start).

They share nothing but the clipping rule, and are checked against each other and against the reference's pinned per-base
tables in tests/test_depth_regions_cpu.py.
"""
import numpy as np

NULL_IDX = 0xFFFFFFFF
U32_MAX = 0xFFFFFFFF


def _wrap32(a):
    """int32 wrap-around of an int64 array, kept as int64"""
    return (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).astype(np.int64)


def key_steps(st, key, skip_pos0):
    """-> (positions int64, v int64) of one key: v = (int32)(c - c0)"""
    k, p, c, _ = st
    m = k == key
    p, c = p[m].astype(np.int64), c[m].astype(np.int64)
    c0 = int(c[0]) if (skip_pos0 and len(p) and p[0] == 0) else 0
    return p, _wrap32(c - c0)


def clip(qkey, qs, qe, i, pos_lo, key_hi):
    """region i -> (key, lo, hi) or None when it is empty"""
    k = 0 if qkey is None else int(qkey[i])
    s, e = int(qs[i]), int(qe[i])
    if k == NULL_IDX or e < s:
        return None
    lo, hi = max(s, int(pos_lo)), min(e, U32_MAX if key_hi is None else int(key_hi[k]))
    return (k, lo, hi) if lo <= hi else None


def values(st, key, first_pos, n, skip_pos0=False):
    """v(p) for p in [first_pos, first_pos + n): expand_steps without the Int16 cast, as int64"""
    p, v = key_steps(st, key, skip_pos0)
    q = first_pos + np.arange(n, dtype=np.int64)
    j = np.searchsorted(p, q, side="right") - 1
    return np.where(j >= 0, v[np.maximum(j, 0)] if len(v) else 0, 0).astype(np.int64)


def summarize_loop(st, qkey, qs, qe, thresholds=(), pos_lo=0, key_hi=None, skip_pos0=False):
    n = len(qs)
    ln, sm, ge = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros((len(thresholds), n), np.int64)
    for i in range(n):
        r = clip(qkey, qs, qe, i, pos_lo, key_hi)
        if r is None:
            continue
        k, lo, hi = r
        v = [int(x) for x in values(st, k, lo, hi - lo + 1, skip_pos0)]
        ln[i] = len(v)
        sm[i] = sum(v)
        for j, t in enumerate(thresholds):
            ge[j, i] = sum(1 for x in v if x >= int(t))
    return ln, sm, ge


def summarize_prefix(st, qkey, qs, qe, thresholds=(), pos_lo=0, key_hi=None, skip_pos0=False):
    n = len(qs)
    ln, sm, ge = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros((len(thresholds), n), np.int64)
    regs = {}
    for i in range(n):
        r = clip(qkey, qs, qe, i, pos_lo, key_hi)
        if r is not None:
            regs.setdefault(r[0], []).append((i, r[1], r[2]))
    for k, rows in regs.items():
        idx = np.array([r[0] for r in rows])
        lo = np.array([r[1] for r in rows], np.int64)
        hi1 = np.array([r[2] for r in rows], np.int64) + 1
        ln[idx] = hi1 - lo
        p, v = key_steps(st, k, skip_pos0)
        if len(p) == 0:
            for j, t in enumerate(thresholds):
                if int(t) <= 0:
                    ge[j, idx] = hi1 - lo
            continue
        seg = np.diff(p)                                    # length of every step but the last

        def upto(w, before_first):
            """x -> sum over positions below x of the per-base weight w[step] (before_first ahead of the first step);
            int64 wrap-around in between is exact: every difference taken fits"""
            with np.errstate(over="ignore"):
                cum = np.concatenate([[0], np.cumsum(w[:-1] * seg)])

                def f(x):
                    j = np.searchsorted(p, x, side="left") - 1              # the last step below x
                    jj = np.maximum(j, 0)
                    return np.where(j >= 0, before_first * p[0] + cum[jj] + w[jj] * (x - p[jj]), before_first * x)
                return f(hi1) - f(lo)

        sm[idx] = upto(v, 0)
        for j, t in enumerate(thresholds):
            ge[j, idx] = upto((v >= int(t)).astype(np.int64), 1 if int(t) <= 0 else 0)
    return ln, sm, ge


def windows_as_regions(first_pos, last_pos, width, n):
    """the windows of ivx_depth_profile_windows as closed regions, empty ones as end < start"""
    s = int(first_pos) + np.arange(n, dtype=np.int64) * int(width)
    e = np.minimum(s + int(width) - 1, int(last_pos))
    empty = s > int(last_pos)
    s, e = np.where(empty, 1, s), np.where(empty, 0, e)
    return s.astype(np.uint32), e.astype(np.uint32)
