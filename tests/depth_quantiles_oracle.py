"""CPU restatements of the depth region order statistics (include/ivx.h ivx_depth_profile_quantiles / _window_quantiles) for
the tests.

Both take the steps form of tests/depth_per_base_oracle.py, st = (key u32, pos u32, coverage i32, key_seen), and return
(bases int64[n], min int32[n], max int32[n], quantiles int32[n_q, n]); a region without bases gives zeros:

  quantiles_loop    per position: the value of every base of the clipped region (depth_regions_oracle.values), np.sort,
                    element floor((L - 1) * q_num / q_den).  Short regions only.
  quantiles_steps   per region the segments (value, clipped length) -- the zero stretch before the key's first step, then
                    the steps that reach into the region -- sorted by value, their cumulative lengths searched for the
                    rank.  Any length.

They share nothing but the clipping rule (depth_regions_oracle.clip) and the rank's integer arithmetic, and are checked
against each other and against the reference's pinned per-base tables in tests/test_depth_quantiles_cpu.py.
"""
import numpy as np

import depth_regions_oracle as dro


def rank(L, q_num, q_den):
    """the index into the L sorted values (Python integers: exact)"""
    return (int(L) - 1) * int(q_num) // int(q_den)


def _empty(n, n_q):
    return np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n_q, n), np.int32)


def quantiles_loop(st, qkey, qs, qe, q_num=(), q_den=2, pos_lo=0, key_hi=None, skip_pos0=False):
    n = len(qs)
    ln, mn, mx, qq = _empty(n, len(q_num))
    for i in range(n):
        r = dro.clip(qkey, qs, qe, i, pos_lo, key_hi)
        if r is None:
            continue
        k, lo, hi = r
        v = np.sort(dro.values(st, k, lo, hi - lo + 1, skip_pos0))
        ln[i], mn[i], mx[i] = len(v), v[0], v[-1]
        for j, qn in enumerate(q_num):
            qq[j, i] = v[rank(len(v), qn, q_den)]
    return ln, mn, mx, qq


def segments(st, key, lo, hi, skip_pos0=False):
    """the region [lo, hi] of `key` as (values int64, lengths int64), every length >= 1, in position order"""
    p, v = dro.key_steps(st, key, skip_pos0)
    b = int(np.searchsorted(p, hi, side="right")) - 1       # the last step at or before hi
    if b < 0:
        return np.zeros(1, np.int64), np.array([hi - lo + 1], np.int64)
    a = int(np.searchsorted(p, lo, side="right")) - 1       # the last step at or before lo
    zero = a < 0
    a = max(a, 0)
    start = np.maximum(p[a:b + 1], lo)
    end = np.concatenate([p[a + 1:b + 1] - 1, [hi]])
    vals, lens = v[a:b + 1], end - start + 1
    if zero:
        vals, lens = np.concatenate([[0], vals]), np.concatenate([[int(p[0]) - lo], lens])
    return vals.astype(np.int64), lens.astype(np.int64)


def quantiles_steps(st, qkey, qs, qe, q_num=(), q_den=2, pos_lo=0, key_hi=None, skip_pos0=False):
    n = len(qs)
    ln, mn, mx, qq = _empty(n, len(q_num))
    for i in range(n):
        r = dro.clip(qkey, qs, qe, i, pos_lo, key_hi)
        if r is None:
            continue
        k, lo, hi = r
        vals, lens = segments(st, k, lo, hi, skip_pos0)
        assert (lens >= 1).all() and int(lens.sum()) == hi - lo + 1
        o = np.argsort(vals, kind="stable")
        vals, cum = vals[o], np.cumsum(lens[o])
        ln[i], mn[i], mx[i] = cum[-1], vals[0], vals[-1]
        for j, qn in enumerate(q_num):
            qq[j, i] = vals[np.searchsorted(cum, rank(cum[-1], qn, q_den), side="right")]
    return ln, mn, mx, qq


def segment_count(st, key, lo, hi):
    return len(segments(st, key, lo, hi)[0])
