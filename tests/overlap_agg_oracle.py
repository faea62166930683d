"""CPU restatement of ivx_probe_overlap_agg (include/ivx.h), built from the oracle's own pairs: orc.join gives M(i), numpy's
unbuffered ufunc.at reduces a build-side value over it.  Everything is int64 / uint64 arithmetic, which wraps like the device.

    aggregate(build, probe, val) -> {"count": u32[n], "sum", "min", "max", "bases", "wsum": i64[n]}

brute() is an independent O(n * m) restatement in Python integers (reduced mod 2^64 at the end), for tiny inputs; the CPU
tests hold the two against each other."""
import numpy as np

from oracle import oracle as orc

OUTPUTS = ("count", "sum", "min", "max", "bases", "wsum")
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


def empty(n):
    """the result of n rows without a match"""
    return {"count": np.zeros(n, np.uint32), "sum": np.zeros(n, np.int64), "min": np.full(n, I64_MAX, np.int64),
            "max": np.full(n, I64_MIN, np.int64), "bases": np.zeros(n, np.int64), "wsum": np.zeros(n, np.int64)}


def from_pairs(b, p, val, wb, wp):
    """the aggregates of the pairs (build row wb[j], probe row wp[j]); b, p: (key, start, end) columns"""
    n = len(p[1])
    out = empty(n)
    if len(wb) == 0:
        return out
    wb, wp = np.asarray(wb, np.int64), np.asarray(wp, np.int64)
    v = np.asarray(val).astype(np.int64)[wb]                            # (int32 values: sign-extended)
    bs, be = np.asarray(b[1], np.int64)[wb], np.asarray(b[2], np.int64)[wb]
    qs, qe = np.asarray(p[1], np.int64)[wp], np.asarray(p[2], np.int64)[wp]
    length = np.minimum(qe, be) - np.maximum(qs, bs) + 1                # int64, no clamp
    cnt = np.zeros(n, np.int64)
    np.add.at(cnt, wp, 1)
    out["count"] = cnt.astype(np.uint32)
    # sums in uint64: numpy wraps silently there, as the device's two's-complement arithmetic does
    for name, term in (("sum", v.view(np.uint64)), ("bases", length.view(np.uint64)), ("wsum", v.view(np.uint64) * length.view(np.uint64))):
        acc = np.zeros(n, np.uint64)
        np.add.at(acc, wp, term)
        out[name] = acc.view(np.int64)
    np.minimum.at(out["min"], wp, v)
    np.maximum.at(out["max"], wp, v)
    return out


def aggregate(b, p, val, threads=4):
    wb, wp = orc.join(*b, *p, threads=threads)
    return from_pairs(b, p, val, wb, wp)


def _wrap(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= (1 << 63) else x


def brute(b, p, val):
    """O(n * m), Python integers: same key (a key only the probe side has matches nothing), bs <= qe and be >= qs"""
    n = len(p[1])
    out = empty(n)
    bk, bs, be = [np.asarray(c).tolist() for c in b]
    pk, ps, pe = [np.asarray(c).tolist() for c in p]
    vals = np.asarray(val).tolist()
    for i in range(n):
        c = s = ba = w = 0
        lo, hi = int(I64_MAX), int(I64_MIN)
        for j in range(len(bs)):
            if bk[j] == pk[i] and bs[j] <= pe[i] and be[j] >= ps[i]:
                ln = min(pe[i], be[j]) - max(ps[i], bs[j]) + 1
                c += 1; s += vals[j]; ba += ln; w += vals[j] * ln
                lo, hi = min(lo, vals[j]), max(hi, vals[j])
        out["count"][i] = c
        out["sum"][i], out["bases"][i], out["wsum"][i] = _wrap(s), _wrap(ba), _wrap(w)
        out["min"][i], out["max"][i] = lo, hi
    return out
