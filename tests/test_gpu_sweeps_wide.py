"""-m gpu: merge / cluster / subtract / complement on int64 coordinates whose MAGNITUDE picks the data layout.

sort64 (csrc/ivx_sweep.hip) and the packed sweep (csrc/ivx_runs.hip) choose their form from the input's ranges: narrow
32-bit sweep rows, the linearised (key, start) word, one 64-bit word or three, the packed one-pass sweep and its narrow
variant.  Every case here sits on one side of one of those thresholds, with a few hundred 4096-row tiles of rows, and
asserts (expected_form) that it reaches the form its name says.  Each is compared bit-exactly with the CPU oracle under
the default settings and under every knob that turns a form off.  The bad-key tests at the end check that a key id
>= n_keys is refused by every entry point before any per-key table is indexed with it."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

I64_MAX = 2**63 - 1
I64_MIN = -(2**63)
L61 = 2**61
SPAN32 = 2**32 - 1                        # the widest range of starts (ends) that still packs as a 32-bit offset
N_BIG, N = 1 << 20, 1 << 19               # 256 / 128 tiles of FTILE = 4096 rows (csrc/ivx_runs.hip), several radix blocks
KNOBS = [None, "IVX_FORCE_SORT", "IVX_NO_LIN", "IVX_NO_K8", "IVX_NO_NARROW_SWEEP", "IVX_NO_PACK_HIST",
         "IVX_NO_FUSED_SWEEP", "IVX_NO_NARROW_RUNS"]


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


# ---------------------------------------------------------------- the host-side decisions, restated

def _bits(x):
    return int(x).bit_length()


def expected_form(key, s, e, n_keys, min_dist=0, strict=False, no_lin=False):
    """The forms sort64 and the packed sweep take for a merge of these rows (default settings; no_lin: IVX_NO_LIN).
    Python ints throughout, so nothing wraps.  Each rule mirrors the host code named beside it."""
    n = len(s)
    min_s, max_s, min_e, max_e = int(s.min()), int(s.max()), int(e.min()), int(e.max())
    f = {}
    # sort64: narrow = both ranges fit a u32 offset; k8 also needs n_keys <= 256
    f["narrow_range"] = max_s - min_s <= 0xFFFFFFFF and max_e - min_e <= 0xFFFFFFFF
    bits_s, bits_e, bits_k = _bits(max_s - min_s), _bits(max_e - min_e), _bits(n_keys - 1 if n_keys else 0)
    # sort64 + k_lin_layout64: every key's start range (width <= 2^62), their sum <= 2^62, and fewer bits than key || start
    f["lin"] = False
    if n_keys <= 2048 and not no_lin:                                            # LIN_KEYS
        kmin = np.full(n_keys, I64_MAX, np.int64)
        kmax = np.full(n_keys, I64_MIN, np.int64)
        np.minimum.at(kmin, key, s)
        np.maximum.at(kmax, key, s)
        widths = [int(b) - int(a) + 1 for a, b in zip(kmin.tolist(), kmax.tolist()) if a <= b]
        total = sum(widths)
        usable = all(w <= 2**62 for w in widths) and 0 < total <= 2**62
        if usable and _bits(total - 1) < bits_k + bits_s:
            f["lin"] = True
            bits_s, bits_k = _bits(total - 1), 0
    # sort64: nw = 1 when key, start and end bits fit one word, else the three-word sort (k_pack64 / k_unpack64)
    f["one_word"] = bits_k + bits_s + bits_e <= 64
    f["narrow_rows"] = f["narrow_range"] and f["one_word"]
    f["k8"] = f["narrow_rows"] and n_keys <= 256
    # ivx_merge_packed_ok: well-formed rows, bits(n_keys) + bits_e <= 62, n < 2^31 - 1, lin table <= 40 KB
    malformed, has_empty = bool((e < s).any()), bool((e == s).any())
    f["packed"] = (f["one_word"] and not malformed and min_dist >= 0 and not (strict and min_dist == 0 and has_empty)
                   and n < 0x7FFFFFFF and _bits(n_keys) + bits_e <= 62
                   and not (f["lin"] and (2 * n_keys + 1) * 8 > 40 * 1024))
    # sort64: p.small = every coordinate within +-2^61 (exclusive)
    f["small"] = min_s > -L61 and max_s < L61 and min_e > -L61 and max_e < L61
    # runs_packed: narrow runs (k_pk_runs<..., true>)
    upper = bits_s if f["lin"] else bits_s + _bits(n_keys - 1 if n_keys else 0)
    f["narrow_runs"] = f["packed"] and f["small"] and bits_e <= 32 and upper <= 32 and min_dist < L61
    return f


# ---------------------------------------------------------------- inputs

def _ends(s, ln):
    """s + min(ln, INT64_MAX - s): numpy int64 wraps silently"""
    room = np.where(s >= 0, I64_MAX - np.maximum(s, 0), I64_MAX)
    return s + np.minimum(ln, room)


def local(rng, n, gap=40, max_len=250):
    """Genomic-like offsets from 0 (ascending) and lengths: dense overlapping rows, about 1 in 17 rows sharing its
    start with the row before it, a few empty rows and now and then a wide gap."""
    g = rng.integers(0, 2 * gap, n)
    g[rng.random(n) < 1 / 17] = 0
    wide = rng.random(n) < 0.004
    g[wide] += rng.integers(10 * max_len, 100 * max_len, int(wide.sum()))
    g[0] = 0
    ln = rng.integers(1, max_len, n)
    ln[rng.random(n) < 0.02] = 0
    return np.cumsum(g).astype(np.int64), ln.astype(np.int64)


def _cat(parts):
    k = np.concatenate([np.full(len(p[0]), p[2], np.uint32) for p in parts])
    return k, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def segment(rng, n, key, lo, hi):
    """n local rows of one key, every start and end inside [lo, hi] (translated, never scaled)"""
    off, ln = local(rng, n)
    assert int(off[-1]) + 300 <= hi - lo, "segment too narrow for its rows"
    s = lo + off
    e = np.minimum(_ends(s, ln), hi)
    return s, e, key


def pinned(parts, lo_key, lo, hi_key, hi):
    """the rows of parts plus two empty rows at lo and hi: the ranges of starts and of ends are then exactly hi - lo"""
    parts = parts + [(np.array([lo], np.int64), np.array([lo], np.int64), lo_key),
                     (np.array([hi], np.int64), np.array([hi], np.int64), hi_key)]
    return _cat(parts)


def order(rng, k, s, e, how):
    if how == "unsorted":
        p = rng.permutation(len(s))
    elif how == "kse":                                   # (key, start, end)-sorted
        p = np.lexsort((e, s, k))
    elif how == "ks":                                    # (key, start)-sorted, ends of equal starts unordered
        p = np.lexsort((rng.random(len(s)), s, k))
    elif how == "toolong":                               # (key, start)-sorted with runs of > 64 equal starts (FIX_MAXRUN)
        s = s.copy()
        for at in rng.choice(len(s) - 200, 6, replace=False):
            s[at:at + 100] = s[at]
        e = np.maximum(e, s)
        p = np.lexsort((rng.random(len(s)), s, k))
    else:
        raise ValueError(how)
    return k[p], s[p], e[p]


def r1(seed, above, orde, n=N_BIG):
    """R1: four keys (lin) whose starts and ends span 2^32 - 1 (narrow) or 2^32 + 1 (wide) in all"""
    rng = np.random.default_rng([1, seed])
    lo = 2**33 + 7
    hi = lo + SPAN32 + (2 if above else 0)
    q = n // 4
    parts = [segment(rng, q, 0, lo, lo + 2**28), segment(rng, q, 1, lo + 2**30, lo + 2**30 + 2**28),
             segment(rng, q, 2, lo + 2**31, lo + 2**31 + 2**28), segment(rng, q, 3, hi - 2**28, hi)]
    return order(rng, *pinned(parts, 0, lo, 3, hi), orde) + (4,)


def r1_one_key(seed, above, n=N):
    """R1 with one key: 32 + 32 bits fill the word exactly, one more bit takes the three-word sort"""
    rng = np.random.default_rng([11, seed])
    lo = -(2**35)
    hi = lo + SPAN32 + (2 if above else 0)
    q = n // 3
    parts = [segment(rng, q, 0, lo, lo + 2**28), segment(rng, q, 0, lo + 2**31, lo + 2**31 + 2**28),
             segment(rng, q, 0, hi - 2**28, hi)]
    return order(rng, *pinned(parts, 0, lo, 0, hi), "unsorted") + (1,)


def r2(seed, n=1 << 18):                                  # (more rows would need more positions than the word leaves)
    """R2: eight keys 2^40 apart, each over a narrow range: wide globally, narrow once linearised (21 bits of
    (key, start) positions and 43 of end range fill the word)"""
    rng = np.random.default_rng([2, seed])
    q = n // 8
    parts = []
    for kk in range(8):
        off, ln = local(rng, q, gap=2, max_len=20)
        s = -(2**42) + kk * 2**40 + off
        parts.append((s, _ends(s, ln), kk))
    k, s, e = _cat(parts)
    return order(rng, k, s, e, "unsorted") + (8,)


def r3_word65(seed, n=N):
    """R3: one key, 32 bits of start range and 33 of end range -- 65 bits, one more than the word holds"""
    rng = np.random.default_rng([3, seed])
    lo = 2**40
    hi = lo + SPAN32
    q = n // 2
    k, s, e = pinned([segment(rng, q, 0, lo, lo + 2**28), segment(rng, q, 0, hi - 2**28, hi)], 0, lo, 0, hi)
    e[-1] = hi + 2                                       # the end range is 2^32 + 1
    return order(rng, k, s, e, "unsorted") + (1,)


def r3_gate(seed, n_keys, n=1 << 16):
    """R3: starts within 4 positions, 61 bits of end range: bits(n_keys) + 61 = 62 (packed sweep) or 63 (not)"""
    rng = np.random.default_rng([4, seed, n_keys])
    lo = -(2**50)
    k = rng.integers(0, n_keys, n).astype(np.uint32)
    s = lo + rng.integers(0, 4, n)
    ln = rng.integers(0, 250, n)
    far = rng.random(n) < 0.01
    ln[far] = rng.integers(0, 2**60, int(far.sum()))
    e = s + ln
    s[0], e[0], k[0] = lo, lo, 0                         # min end = lo
    s[1], e[1], k[1] = lo, lo + 2**60 + 5, n_keys - 1    # max end: 61 bits of range
    return order(rng, k, s, e, "unsorted") + (n_keys,)


def r4(seed, orde, n=N_BIG):
    """R4: dense clusters near INT64_MIN, around 0 and near INT64_MAX in one key (and a second key around 0);
    starts and ends equal to INT64_MAX and INT64_MIN"""
    rng = np.random.default_rng([5, seed])
    q = n // 4
    off, ln = local(rng, q)
    a = (I64_MIN + off, _ends(I64_MIN + off, ln), 0)
    off, ln = local(rng, q)
    b = (off - off[-1] // 2, _ends(off - off[-1] // 2, ln), 0)
    off, ln = local(rng, q)
    s = I64_MAX - off[::-1]                              # the last start is INT64_MAX
    c = (s, _ends(s, ln), 0)
    off, ln = local(rng, q)
    d = (off - off[-1] // 2, _ends(off - off[-1] // 2, ln), 1)
    k, s, e = _cat([a, b, c, d])
    top = rng.random(len(s)) < 0.002
    e[top & (k == 0)] = I64_MAX                          # ends at INT64_MAX (also from far below)
    return order(rng, k, s, e, orde) + (2,)


def r5(seed, side, inside, n=N):
    """R5: 40 narrow keys next to +2^61 or -2^61; inside: every coordinate within +-2^61 (p.small), else one on it"""
    rng = np.random.default_rng([6, seed, side + 1, int(inside)])
    q = n // 40
    if side > 0:
        hi = L61 - 1 if inside else L61
        lo = hi - 2**31
    else:
        lo = -L61 + 1 if inside else -L61
        hi = lo + 2**31
    step = (hi - lo) // 40
    parts = [segment(rng, q, kk, lo + kk * step, lo + (kk + 1) * step - 1) for kk in range(40)]
    return order(rng, *pinned(parts, 0, lo, 39, hi), "unsorted") + (40,)


def r6(seed, n_keys, n=N):
    """R6: n_keys around the K8 (256), LIN_KEYS (2048) and lin-table (2559) limits; every fifth key and the last one
    without rows"""
    rng = np.random.default_rng([7, seed, n_keys])
    used = [kk for kk in range(n_keys - 1) if kk % 5 != 4]
    q = n // len(used)
    lo = 10**9
    parts = []
    for kk in used:
        off, ln = local(rng, q, gap=20, max_len=100)
        s = lo + kk * 16384 + off
        parts.append((s, _ends(s, ln), kk))
    return order(rng, *_cat(parts), "unsorted") + (n_keys,)


def r8(seed, straddle, n=N):
    """R8: every row negative, or rows straddling 0 (three keys)"""
    rng = np.random.default_rng([8, seed, straddle])
    parts = []
    for kk in range(3):
        off, ln = local(rng, n // 3)
        s = (off - off[-1] // 2) if straddle else (-(10**10) + kk * 10**8 + off)
        e = _ends(s, ln)
        if not straddle:
            e = np.minimum(e, -1)
        parts.append((s, e, kk))
    return order(rng, *_cat(parts), "unsorted") + (3,)


# name -> (builder, the forms it must reach)
CASES = {
    "R1_narrow_unsorted": (lambda: r1(0, False, "unsorted"), dict(narrow_rows=True, lin=True, packed=True, narrow_runs=True, k8=True)),
    "R1_narrow_kse": (lambda: r1(1, False, "kse"), dict(narrow_rows=True, lin=True, packed=True, narrow_runs=True)),
    "R1_narrow_ks": (lambda: r1(2, False, "ks"), dict(narrow_rows=True, lin=True, packed=True, narrow_runs=True)),
    "R1_narrow_toolong": (lambda: r1(3, False, "toolong"), dict(narrow_rows=True, lin=True, packed=True)),
    "R1_wide_unsorted": (lambda: r1(4, True, "unsorted"), dict(narrow_range=False, one_word=True, lin=True, packed=True, narrow_runs=False)),
    "R1_wide_kse": (lambda: r1(5, True, "kse"), dict(narrow_range=False, one_word=True, lin=True, packed=True, narrow_runs=False)),
    "R1_wide_ks": (lambda: r1(6, True, "ks"), dict(narrow_range=False, one_word=True, lin=True, packed=True, narrow_runs=False)),
    "R1_wide_toolong": (lambda: r1(7, True, "toolong"), dict(narrow_range=False, one_word=True, lin=True, packed=True)),
    "R1_one_key_64bits": (lambda: r1_one_key(0, False), dict(narrow_rows=True, lin=False, one_word=True, k8=True, packed=True, narrow_runs=True)),
    "R1_one_key_66bits": (lambda: r1_one_key(1, True), dict(narrow_range=False, lin=False, one_word=False, packed=False)),
    "R2_keys_2e40_apart": (lambda: r2(0), dict(narrow_range=False, lin=True, one_word=True, packed=True, narrow_runs=False)),
    "R3_word_65bits": (lambda: r3_word65(0), dict(lin=False, one_word=False, packed=False)),
    "R3_packed_gate_62": (lambda: r3_gate(0, 1), dict(one_word=True, packed=True, narrow_runs=False)),
    "R3_packed_gate_63": (lambda: r3_gate(1, 2), dict(one_word=True, packed=False)),
    "R4_full_unsorted": (lambda: r4(0, "unsorted"), dict(one_word=False, small=False, lin=False, packed=False)),
    "R4_full_kse": (lambda: r4(1, "kse"), dict(one_word=False, small=False, lin=False, packed=False)),
    "R4_full_ks": (lambda: r4(2, "ks"), dict(one_word=False, small=False, lin=False, packed=False)),
    "R4_full_toolong": (lambda: r4(3, "toolong"), dict(one_word=False, small=False, lin=False, packed=False)),
    "R5_plus_inside": (lambda: r5(0, 1, True), dict(narrow_rows=True, small=True, packed=True, narrow_runs=True)),
    "R5_plus_outside": (lambda: r5(1, 1, False), dict(narrow_rows=True, small=False, packed=True, narrow_runs=False)),
    "R5_minus_inside": (lambda: r5(2, -1, True), dict(narrow_rows=True, small=True, packed=True, narrow_runs=True)),
    "R5_minus_outside": (lambda: r5(3, -1, False), dict(narrow_rows=True, small=False, packed=True, narrow_runs=False)),
    "R6_keys_256": (lambda: r6(0, 256), dict(narrow_rows=True, k8=True, lin=True, packed=True)),
    "R6_keys_257": (lambda: r6(1, 257), dict(narrow_rows=True, k8=False, lin=True, packed=True)),
    "R6_keys_2048": (lambda: r6(2, 2048), dict(narrow_rows=True, lin=True, packed=True)),
    "R6_keys_2049": (lambda: r6(3, 2049), dict(narrow_rows=True, lin=False, packed=True)),
    # (the 40 KB lin-table gate of ivx_merge_packed_ok sits at 2559 keys, above LIN_KEYS: both take the key || start word)
    "R6_keys_2559": (lambda: r6(4, 2559), dict(narrow_rows=True, lin=False, packed=True)),
    "R6_keys_2560": (lambda: r6(5, 2560), dict(narrow_rows=True, lin=False, packed=True)),
    "R8_negative": (lambda: r8(0, False), dict(narrow_rows=True, packed=True)),
    "R8_straddle_0": (lambda: r8(1, True), dict(narrow_rows=True, packed=True)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    k, s, e, nk = CASES[name][0]()
    assert (e >= s).all(), name                          # every regime builds well-formed rows
    assert k.max() < nk
    return k, s, e, nk


@functools.lru_cache(maxsize=None)
def sub_sides(name):
    """subtract's sides: the case's rows, and for the right side a third as many of them with their starts moved a
    little.  A left row spanning most of int64 walks every right row of its key and emits a fragment per gap, and a
    right row that long keeps every later left row walking from it, so the right side takes none of them and the left
    keeps eight (ends at INT64_MAX near the top of the range are short and stay)."""
    k, s, e, nk = case(name)
    short = (e.view(np.uint64) - s.view(np.uint64)) <= 10**6       # e >= s: the unsigned difference is exact
    keep = short.copy()
    keep[np.flatnonzero(~short)[:8]] = True
    rng = np.random.default_rng([99, len(s)])
    n_right = int(short.sum()) // 3 if not name.startswith("R3_packed_gate") else 2000   # (there every row overlaps every other)
    pick = rng.choice(np.flatnonzero(short), n_right, replace=False)
    shift = rng.integers(-500, 500, len(pick))
    rs = np.where(shift > 0, s[pick] + np.minimum(shift, I64_MAX - np.maximum(s[pick], 0)), s[pick])
    return (k[keep], s[keep], e[keep]), (k[pick], rs, np.maximum(e[pick], rs))


# ---------------------------------------------------------------- comparisons

def _host(x):
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.asarray(x).astype(np.int64)


def _same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        g = _host(g)
        if w.dtype == np.uint32:
            g = g & 0xFFFFFFFF                           # (device key / row columns come back as int32)
        assert len(g) == len(w) and np.array_equal(g, w.astype(np.int64)), f"{what}: column {i}"


CLUSTER_COLS = ("key", "start", "end", "row", "cluster", "cluster_start", "cluster_end")


def _same_cluster(got, want, what):
    _same([got[c] for c in CLUSTER_COLS], [want[c] for c in CLUSTER_COLS], what)
    assert got["n_clusters"] == want["n_clusters"], what
    assert np.array_equal(_host(got["key_clusters"]), want["key_clusters"].astype(np.int64)), what


def _agrees(got, form, what):
    """the forms a merge call took (pyivx.Ctx.sweep_form(), noted by sort64 and runs_packed as they decide) against
    expected_form's restatement of them"""
    read = dict(lin=bool(got["lin"]), one_word=got["nw"] == 1, narrow_rows=bool(got["narrow_rows"]), k8=bool(got["k8"]),
                packed=got["packed"] == pyivx.SWEEP_PACKED, narrow_runs=bool(got["narrow_runs"]))
    assert read == {w: form[w] for w in read}, f"{what}: the call took {got}, expected_form says {form}"


# ---------------------------------------------------------------- every regime, every knob

@pytest.mark.parametrize("name", list(CASES))
def test_sweeps_wide_forms_and_knobs(ctx, monkeypatch, name):
    k, s, e, nk = case(name)
    form = expected_form(k, s, e, nk)
    for key_, v in CASES[name][1].items():
        assert form[key_] == v, f"{name} reaches {key_}={form[key_]} (wanted {v}): {form}"
    if name == "R2_keys_2e40_apart":                      # without lin the word is key || start: three words
        assert not expected_form(k, s, e, nk, no_lin=True)["one_word"]
    ctx.merge(k, s, e, n_keys=nk)
    _agrees(ctx.sweep_form(), form, name)                 # ... and the device's host code decided the same
    (lk, ls, le), (rk, rs, re) = sub_sides(name)
    want_m = {st: orc.merge(k, s, e, strict=st) for st in (False, True)}
    want_c = orc.cluster(k, s, e, n_keys=nk)
    want_s = orc.subtract(lk, ls, le, rk, rs, re)
    want_x = orc.complement(k, s, e)
    for knob in KNOBS:
        with monkeypatch.context() as m:
            if knob:
                m.setenv(knob, "1")
            for st in (False, True):
                _same(ctx.merge(k, s, e, n_keys=nk, strict=st), want_m[st], f"merge strict={st} {knob}")
            _same_cluster(ctx.cluster(k, s, e, n_keys=nk), want_c, f"cluster {knob}")
            _same(ctx.subtract(lk, ls, le, rk, rs, re, n_keys=nk), want_s, f"subtract {knob}")
            _same(ctx.complement(k, s, e, n_keys=nk), want_x, f"complement {knob}")
    # subtract: one call with cap, the fill without the sizing call's plan, the general (malformed-rights) sweep
    _same(ctx.subtract(lk, ls, le, rk, rs, re, n_keys=nk, cap=len(want_s[0]) + 5), want_s, "subtract cap")
    with monkeypatch.context() as m:
        m.setenv("IVX_NO_PLAN", "1")
        _same(ctx.subtract(lk, ls, le, rk, rs, re, n_keys=nk), want_s, "subtract IVX_NO_PLAN")
    with monkeypatch.context() as m:
        m.setenv("IVX_SUB_GENERAL", "1")
        _same(ctx.subtract(lk, ls, le, rk, rs, re, n_keys=nk), want_s, "subtract IVX_SUB_GENERAL")
    # strict once more for the other three
    _same_cluster(ctx.cluster(k, s, e, n_keys=nk, strict=True), orc.cluster(k, s, e, n_keys=nk, strict=True), "cluster strict")
    _same(ctx.subtract(lk, ls, le, rk, rs, re, n_keys=nk, strict=True), orc.subtract(lk, ls, le, rk, rs, re, strict=True), "subtract strict")
    _same(ctx.complement(k, s, e, n_keys=nk, strict=True), orc.complement(k, s, e, strict=True), "complement strict")


# ---------------------------------------------------------------- R7: min_dist

MIN_DISTS = [0, 1, 2**32, L61 - 1, L61, I64_MAX - 1, I64_MAX]


@pytest.mark.parametrize("name", ["R1_narrow_unsorted", "R4_full_unsorted", "R5_plus_inside", "R5_minus_outside"])
def test_min_dist_saturation(ctx, monkeypatch, name):
    """merge and cluster with min_dist up to INT64_MAX: the saturating boundary and the narrow runs' constant K"""
    k, s, e, nk = case(name)
    sub = np.random.default_rng(7).choice(len(s), len(s) // 4, replace=False)  # a quarter of the rows: 16-32 tiles
    sub.sort()
    k, s, e = k[sub], s[sub], e[sub]
    for md in MIN_DISTS:
        form = expected_form(k, s, e, nk, min_dist=md)
        if name != "R4_full_unsorted":
            assert form["packed"] and form["narrow_runs"] == (md < L61 and form["small"]), (md, form)
        for st in (False, True):
            wm = orc.merge(k, s, e, min_dist=md, strict=st)
            wc = orc.cluster(k, s, e, min_dist=md, strict=st, n_keys=nk)
            for knob in (None, "IVX_NO_NARROW_RUNS", "IVX_NO_FUSED_SWEEP", "IVX_FORCE_SORT", "IVX_NO_LIN"):
                with monkeypatch.context() as m:
                    if knob:
                        m.setenv(knob, "1")
                    _same(ctx.merge(k, s, e, n_keys=nk, min_dist=md, strict=st), wm, f"merge md={md} strict={st} {knob}")
                    if knob is None and not st:
                        _agrees(ctx.sweep_form(), form, f"{name} md={md}")
                    _same_cluster(ctx.cluster(k, s, e, n_keys=nk, min_dist=md, strict=st), wc, f"cluster md={md} strict={st} {knob}")


# ---------------------------------------------------------------- operators' extras across regimes

@pytest.mark.parametrize("left,right", [("R1_one_key_64bits", "R4_full_unsorted"), ("R4_full_unsorted", "R1_one_key_64bits"),
                                        ("R1_narrow_unsorted", "R4_full_ks")])
def test_subtract_sides_in_different_forms(ctx, monkeypatch, left, right):
    """narrow left / wide right and the reverse; then the right rows made malformed (end < start), so that the general
    sweep runs"""
    nl, nr = case(left)[3], case(right)[3]
    (lk, ls, le), _ = sub_sides(left)
    _, (rk, rs, re) = sub_sides(right)
    nk = max(nl, nr)
    rk = rk % np.uint32(nl)                              # the right rows' keys where the left has rows
    assert expected_form(lk, ls, le, nk)["one_word"] != expected_form(rk, rs, re, nk)["one_word"]
    want = orc.subtract(lk, ls, le, rk, rs, re)
    for knob in (None, "IVX_FORCE_SORT", "IVX_NO_PLAN", "IVX_NO_LIN"):
        with monkeypatch.context() as m:
            if knob:
                m.setenv(knob, "1")
            _same(ctx.subtract(lk, ls, le, rk, rs, re, n_keys=nk), want, f"subtract {left} - {right} {knob}")
    bad = np.random.default_rng(3).random(len(rs)) < 0.05
    re2 = re.copy()
    re2[bad] = np.maximum(rs[bad], I64_MIN + 1000) - 1000   # end < start
    for st in (False, True):
        _same(ctx.subtract(lk, ls, le, rk, rs, re2, n_keys=nk, strict=st), orc.subtract(lk, ls, le, rk, rs, re2, strict=st),
              f"subtract malformed rights strict={st}")


@pytest.mark.parametrize("name", ["R4_full_unsorted", "R8_negative", "R8_straddle_0", "R1_wide_unsorted"])
def test_complement_views_at_extremes(ctx, name):
    k, s, e, nk = case(name)
    vk = np.array([0, 0, 0, 1, 1, nk, nk], np.uint32)      # key nk: views without input rows; the last key: no view
    vs = np.array([I64_MIN, I64_MAX - 10**6, -5000, I64_MIN, 0, I64_MIN, 7], np.int64)
    ve = np.array([I64_MAX, I64_MAX, 5000, I64_MIN + 10**6, I64_MAX, I64_MAX, 7], np.int64)
    for st in (False, True):
        _same(ctx.complement(k, s, e, vk, vs, ve, n_keys=nk + 1, strict=st), orc.complement(k, s, e, vk, vs, ve, strict=st),
              f"complement views strict={st}")


@pytest.mark.parametrize("name", ["R1_wide_unsorted", "R4_full_unsorted", "R6_keys_2049"])
def test_cluster_key_base_across_forms(ctx, name):
    """ids from key_base per partition match one run over all rows (as test_cluster_sharded_ids_match_single_run)"""
    k, s, e, nk = case(name)
    full = ctx.cluster(k, s, e, n_keys=nk)
    _same_cluster(full, orc.cluster(k, s, e, n_keys=nk), "cluster")
    odd = (k % 2).astype(bool)
    parts = [~odd, odd]
    counts = np.zeros(nk, np.int64)
    for sel in parts:
        counts += _host(ctx.cluster(k[sel], s[sel], e[sel], n_keys=nk, rows=False)["key_clusters"])
    base = np.concatenate([[0], np.cumsum(counts)[:-1]])
    for sel in parts:
        part = ctx.cluster(k[sel], s[sel], e[sel], n_keys=nk, key_base=base)
        want = np.isin(full["key"], np.unique(k[sel]))
        for c in ("key", "start", "end", "cluster", "cluster_start", "cluster_end"):
            assert np.array_equal(_host(part[c]), _host(full[c])[want]), c
        assert np.array_equal(np.flatnonzero(sel)[part["row"]], full["row"][want])


def test_device_memory_full_int64(ctx):
    """R4 through IVX_MEM_DEVICE: torch tensors in and out"""
    import torch
    k, s, e, nk = case("R4_full_unsorted")
    (lk, ls, le), (rk, rs, re) = sub_sides("R4_full_unsorted")
    t = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    dk, ds, de, dlk, dls, dle, drk, drs, dre = map(t, (k, s, e, lk, ls, le, rk, rs, re))

    def host(cols):
        ctx.synchronize()
        return [c.cpu().numpy() for c in cols]
    for st in (False, True):
        _same(host(ctx.merge(dk, ds, de, n_keys=nk, strict=st)), orc.merge(k, s, e, strict=st), "merge device")
        _same(host(ctx.subtract(dlk, dls, dle, drk, drs, dre, n_keys=nk, strict=st)), orc.subtract(lk, ls, le, rk, rs, re, strict=st), "subtract device")
        _same(host(ctx.complement(dk, ds, de, n_keys=nk, strict=st)), orc.complement(k, s, e, strict=st), "complement device")
    got = ctx.cluster(dk, ds, de, n_keys=nk)
    ctx.synchronize()
    got = {c: (v.cpu().numpy() if hasattr(v, "cpu") else v) for c, v in got.items()}
    _same_cluster(got, orc.cluster(k, s, e, n_keys=nk), "cluster device")


# ---------------------------------------------------------------- bad key ids, every entry point

def _bad_inputs(n_keys, sorted_, n=20_000, dtype=np.int64, seed=0):
    rng = np.random.default_rng([seed, n_keys, n])
    k = rng.integers(0, n_keys, n).astype(np.uint32)
    s = rng.integers(0, 5_000_000, n).astype(dtype)
    e = (s + rng.integers(0, 2000, n)).astype(dtype)
    if sorted_:
        p = np.lexsort((e, s, k))
        k, s, e = k[p], s[p], e[p]
    return k, s, e


def _with_bad(k, bad, where):
    k = k.copy()
    k[{"first": 0, "middle": len(k) // 2, "last": len(k) - 1}[where]] = bad
    return k


def _refused(fn):
    with pytest.raises(pyivx.IvxError) as ei:
        fn()
    assert ei.value.status == pyivx.ERR_INVALID


@pytest.mark.parametrize("sorted_", [False, True], ids=["unsorted", "sorted"])
@pytest.mark.parametrize("n_keys", [24, 3000], ids=["lin", "no_lin"])
def test_bad_key_sweeps(ctx, n_keys, sorted_):
    k, s, e = _bad_inputs(n_keys, sorted_)
    rk, rs, re = _bad_inputs(n_keys, sorted_, n=8_000, seed=1)
    good_m = orc.merge(k, s, e)
    good_s = orc.subtract(k, s, e, rk, rs, re)
    vk = np.arange(n_keys, dtype=np.uint32)[: min(n_keys, 64)]
    vs, ve = np.zeros(len(vk), np.int64), np.full(len(vk), 4_000_000, np.int64)
    good_x = orc.complement(k, s, e, vk, vs, ve)
    for bad in (n_keys, 0xFFFFFFFF):
        for where in ("first", "middle", "last"):
            bk, brk, bvk = _with_bad(k, bad, where), _with_bad(rk, bad, where), _with_bad(vk, bad, where)
            _refused(lambda: ctx.merge(bk, s, e, n_keys=n_keys))
            _same(ctx.merge(k, s, e, n_keys=n_keys), good_m, "merge after a refused merge")
            _refused(lambda: ctx.cluster(bk, s, e, n_keys=n_keys))
            _same(ctx.merge(k, s, e, n_keys=n_keys), good_m, "merge after a refused cluster")
            _refused(lambda: ctx.subtract(bk, s, e, rk, rs, re, n_keys=n_keys))
            _same(ctx.subtract(k, s, e, rk, rs, re, n_keys=n_keys), good_s, "subtract after a bad left key")
            _refused(lambda: ctx.subtract(k, s, e, brk, rs, re, n_keys=n_keys))
            _same(ctx.subtract(k, s, e, rk, rs, re, n_keys=n_keys), good_s, "subtract after a bad right key")
            _refused(lambda: ctx.complement(bk, s, e, vk, vs, ve, n_keys=n_keys))
            _refused(lambda: ctx.complement(k, s, e, bvk, vs, ve, n_keys=n_keys))
            _same(ctx.complement(k, s, e, vk, vs, ve, n_keys=n_keys), good_x, "complement after a bad view key")


@pytest.mark.parametrize("sorted_", [False, True], ids=["unsorted", "sorted"])
@pytest.mark.parametrize("n_keys", [24, 3000], ids=["lin", "no_lin"])
def test_bad_key_index_builds(ctx, n_keys, sorted_):
    k, s, e = _bad_inputs(n_keys, sorted_, dtype=np.int32)
    pk, ps, pe = _bad_inputs(n_keys, False, n=30_000, dtype=np.int32, seed=2)
    want = orc.pair_keys(*orc.join(k, s, e, pk, ps, pe))
    small = slice(0, 3000)                               # nearest: n < 4096 takes the two-word sorts, more the lin build
    builds = [(pyivx.KIND_OVERLAP, slice(None)), (pyivx.KIND_COUNT, slice(None)), (pyivx.KIND_COVERAGE, slice(None)),
              (pyivx.KIND_NEAREST, slice(None)), (pyivx.KIND_NEAREST, small)]
    for bad in (n_keys, 0xFFFFFFFF):
        for where in ("first", "middle", "last"):
            for kind, rows in builds:
                bk = _with_bad(k[rows], bad, where)
                _refused(lambda: ctx.build(kind, bk, s[rows], e[rows], n_keys=n_keys))
                ix = ctx.build(pyivx.KIND_OVERLAP, k, s, e, n_keys=n_keys)
                got = orc.pair_keys(*ctx.overlap_fill(ix, pk, ps, pe))
                ix.free()
                assert np.array_equal(np.sort(got), np.sort(want)), (kind, bad, where)
