"""CPU only: the C oracle's merge / cluster / subtract / complement against a plain Python-int restatement, on small
seeded inputs at the int64 extremes.  The GPU sweeps are checked against the C oracle (tests/test_gpu_sweeps_wide.py);
this pins the oracle itself where int64 arithmetic can overflow: min_dist added with saturation, strict at INT64_MAX,
the implicit view [0, INT64_MAX), empty and inverted rows.

The restatement follows the operators' semantics as include/ivx.h states them: rows grouped by key (keys ascending),
sorted by (start, end, row) inside a key, then one serial walk per key.  Python ints do not wrap, so every sum is
exact and saturation is spelled out."""
import numpy as np
import pytest

from oracle import oracle as orc

I64_MAX = 2**63 - 1
I64_MIN = -(2**63)
L61 = 2**61


def sat_add(a, b):
    return max(I64_MIN, min(I64_MAX, a + b))


def by_key(key, s, e):
    """{key: [(start, end, row), ...] sorted by (start, end, row)}"""
    g = {}
    for i, (k, a, b) in enumerate(zip(key.tolist(), s.tolist(), e.tolist())):
        g.setdefault(k, []).append((a, b, i))
    return {k: sorted(v) for k, v in sorted(g.items())}


def merges(start, cur_end, min_dist, strict):
    boundary = sat_add(cur_end, min_dist)
    return start < boundary if strict else start <= boundary


def py_merge(key, s, e, min_dist, strict):
    out = []
    for k, rows in by_key(key, s, e).items():
        cs, ce, cn = rows[0][0], rows[0][1], 1
        for a, b, _ in rows[1:]:
            if merges(a, ce, min_dist, strict):
                ce = max(ce, b)
                cn += 1
            else:
                out.append((k, cs, ce, cn))
                cs, ce, cn = a, b, 1
        out.append((k, cs, ce, cn))
    return out


def py_cluster(key, s, e, min_dist, strict, n_keys):
    """-> per sorted row (key, start, end, row, cluster id, cluster start, cluster end), clusters per key"""
    out, per_key, next_id = [], [0] * n_keys, 0
    for k, rows in by_key(key, s, e).items():
        i = 0
        while i < len(rows):
            cs, ce, j = rows[i][0], rows[i][1], i + 1
            while j < len(rows) and merges(rows[j][0], ce, min_dist, strict):
                ce = max(ce, rows[j][1])
                j += 1
            out += [(k, a, b, r, next_id, cs, ce) for a, b, r in rows[i:j]]
            next_id += 1
            per_key[k] += 1
            i = j
    return out, per_key


def py_subtract(lkey, ls, le, rkey, rs, re, strict):
    out = []
    right = by_key(rkey, rs, re)
    for k, lrows in by_key(lkey, ls, le).items():
        rrows = right.get(k, [])
        rc = 0                                              # the right cursor only moves forward within a key
        for a, b, row in lrows:
            while rc < len(rrows) and (rrows[rc][1] <= a if strict else rrows[rc][1] < a):
                rc += 1
            cursor = a
            for x, y, _ in rrows[rc:]:
                if (x >= b) if strict else (x > b):
                    break
                if x > cursor:
                    out.append((k, cursor, x, row))
                cursor = max(cursor, y)
            if cursor < b:
                out.append((k, cursor, b, row))
    return out


def py_complement(key, s, e, vkey, vs, ve, strict):
    out = []
    views = by_key(vkey, vs, ve)
    inp = by_key(key, s, e)
    for k, rows in inp.items():
        merged = []                                         # merged with min_dist = 0, no count
        for a, b, _ in rows:
            if merged and (a < merged[-1][1] if strict else a <= merged[-1][1]):
                merged[-1][1] = max(merged[-1][1], b)
            else:
                merged.append([a, b])
        for v0, v1, _ in views.get(k, [(0, I64_MAX, 0)]):   # a key with input rows and no view: [0, INT64_MAX)
            cursor = v0
            for ms, me in merged:
                if me <= v0:
                    continue
                if ms >= v1:
                    break
                if max(ms, v0) > cursor:
                    out.append((k, cursor, max(ms, v0)))
                cursor = min(me, v1)
            if cursor < v1:
                out.append((k, cursor, v1))
    for k, vrows in views.items():                          # keys with views only: the views as they are, after the rest
        if k not in inp:
            out += [(k, v0, v1) for v0, v1, _ in vrows]
    return out


# ---------------------------------------------------------------- inputs

def _clip(x):
    return max(I64_MIN, min(I64_MAX, x))


def rows_near(rng, n, centers, n_keys):
    """n rows in clusters around the given centers: overlapping, touching, empty (end == start) and inverted
    (end < start) rows, starts and ends equal to the int64 extremes."""
    c = np.array(centers, dtype=object)[rng.integers(0, len(centers), n)]
    off = rng.integers(-300, 300, n)
    s = np.array([int(_clip(int(a) + int(b))) for a, b in zip(c, off)], dtype=object)
    ln = rng.integers(0, 120, n)
    kind = rng.random(n)
    ln = np.where(kind < 0.08, 0, ln)                       # empty rows
    ln = np.where((kind >= 0.08) & (kind < 0.12), -rng.integers(1, 50, n), ln)   # inverted rows
    e = np.array([int(_clip(int(a) + int(b))) for a, b in zip(s, ln)], dtype=object)
    at_max = rng.random(n)
    e = np.where(at_max < 0.05, I64_MAX, e)
    s = np.where(at_max > 0.97, I64_MAX, s)
    s = np.where((at_max > 0.94) & (at_max <= 0.97), I64_MIN, s)
    key = rng.integers(0, n_keys, n).astype(np.uint32)
    return key, s.astype(np.int64), e.astype(np.int64)


REGIMES = {
    "R4_full": [I64_MIN, I64_MIN + 200, -150, 0, 150, I64_MAX - 200, I64_MAX],
    "R5_small": [-L61 - 100, -L61, -L61 + 100, L61 - 100, L61, L61 + 100],
    "R8_negative": [-10**12, -5000, -600, -1],
    "R8_straddle0": [-200, 0, 200],
}
MIN_DISTS = [0, 1, 2**32, L61 - 1, L61, I64_MAX - 1, I64_MAX]


def _cases():
    for name in REGIMES:
        for seed in range(40):
            yield name, seed


def _inputs(name, seed):
    rng = np.random.default_rng([seed, list(REGIMES).index(name)])
    n = int(rng.integers(1, 201))
    n_keys = int(rng.integers(1, 4))
    return rng, n_keys, rows_near(rng, n, REGIMES[name], n_keys)


def _as_rows(*cols):
    return list(zip(*[np.asarray(c).tolist() for c in cols]))


@pytest.mark.parametrize("name,seed", list(_cases()))
def test_merge_and_cluster_exact(name, seed):
    rng, n_keys, (k, s, e) = _inputs(name, seed)
    for md in MIN_DISTS:
        for strict in (False, True):
            assert _as_rows(*orc.merge(k, s, e, min_dist=md, strict=strict)) == py_merge(k, s, e, md, strict), (md, strict)
            got = orc.cluster(k, s, e, min_dist=md, strict=strict, n_keys=n_keys)
            want, per_key = py_cluster(k, s, e, md, strict, n_keys)
            cols = ("key", "start", "end", "row", "cluster", "cluster_start", "cluster_end")
            assert _as_rows(*[got[c] for c in cols]) == want, (md, strict)
            assert got["key_clusters"].tolist() == per_key and got["n_clusters"] == sum(per_key)


@pytest.mark.parametrize("name,seed", list(_cases()))
def test_subtract_exact(name, seed):
    rng, n_keys, (lk, ls, le) = _inputs(name, seed)
    rk, rs, re = rows_near(rng, int(rng.integers(0, 201)), REGIMES[name], n_keys + 1)   # a key the left side lacks
    for strict in (False, True):
        assert _as_rows(*orc.subtract(lk, ls, le, rk, rs, re, strict=strict)) == py_subtract(lk, ls, le, rk, rs, re, strict)


@pytest.mark.parametrize("name,seed", list(_cases()))
def test_complement_exact(name, seed):
    rng, n_keys, (k, s, e) = _inputs(name, seed)
    for strict in (False, True):
        # no views: the implicit [0, INT64_MAX) clips the rows below 0
        z = np.zeros(0, np.int64)
        assert _as_rows(*orc.complement(k, s, e, strict=strict)) == py_complement(k, s, e, np.zeros(0, np.uint32), z, z, strict)
        # views of some keys only (others take the implicit view), a view-only key, views at the extremes
        nv = int(rng.integers(1, 12))
        vk = rng.integers(0, n_keys + 1, nv).astype(np.uint32)
        pts = REGIMES[name] + [I64_MIN, 0, I64_MAX]
        a = np.array([pts[i] for i in rng.integers(0, len(pts), nv)], dtype=object)
        b = np.array([pts[i] for i in rng.integers(0, len(pts), nv)], dtype=object)
        vs, ve = np.minimum(a, b).astype(np.int64), np.maximum(a, b).astype(np.int64)
        assert _as_rows(*orc.complement(k, s, e, vk, vs, ve, strict=strict)) == py_complement(k, s, e, vk, vs, ve, strict)


def test_restatement_pins():
    """Hand-checked answers, so that the restatement is not only compared with the oracle."""
    k = np.zeros(3, np.uint32)
    s = np.array([I64_MAX - 10, I64_MAX, I64_MAX], np.int64)
    e = np.array([I64_MAX, I64_MAX, I64_MAX], np.int64)
    # weak: INT64_MAX <= INT64_MAX merges; strict: INT64_MAX < sat(INT64_MAX + 0) does not
    assert py_merge(k, s, e, 0, False) == [(0, I64_MAX - 10, I64_MAX, 3)]
    assert py_merge(k, s, e, 0, True) == [(0, I64_MAX - 10, I64_MAX, 1), (0, I64_MAX, I64_MAX, 1), (0, I64_MAX, I64_MAX, 1)]
    # min_dist saturates instead of wrapping below the next start
    k2, s2, e2 = np.zeros(2, np.uint32), np.array([-5, I64_MAX - 1], np.int64), np.array([10, I64_MAX - 1], np.int64)
    assert py_merge(k2, s2, e2, I64_MAX, True) == [(0, -5, I64_MAX - 1, 2)]
    for md in (I64_MAX, I64_MAX - 1):
        assert _as_rows(*orc.merge(k2, s2, e2, min_dist=md, strict=True)) == [(0, -5, I64_MAX - 1, 2)]
    # the implicit view starts at 0: a row below 0 leaves [0, INT64_MAX) whole
    assert py_complement(np.zeros(1, np.uint32), np.array([-9], np.int64), np.array([-1], np.int64),
                         np.zeros(0, np.uint32), np.zeros(0, np.int64), np.zeros(0, np.int64), False) == [(0, 0, I64_MAX)]
    # subtract: an inverted right row [5, 3) cuts [0, 5) off and moves the cursor to its end, 3
    assert py_subtract(np.zeros(1, np.uint32), np.array([0], np.int64), np.array([20], np.int64),
                       np.zeros(1, np.uint32), np.array([5], np.int64), np.array([3], np.int64), False) == [(0, 0, 5, 0), (0, 3, 20, 0)]
