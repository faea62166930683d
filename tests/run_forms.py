"""Designed inputs for the run sweep behind merge / cluster / complement (csrc/ivx_runs.hip), the predicates that say what an
input makes the sweep do, a plain serial walk of the reference rule and the host-side form rules.  Plain numpy: no GPU and no
library here.  tests/test_run_forms_cpu.py checks that every case is what its name claims and that the serial walk equals
the C oracle; tests/test_gpu_run_edges.py runs the cases on the device and asserts the form each call took
(pyivx.Ctx.sweep_form()) against host_form() below.

Geometry (csrc/ivx_runs.hip: FT = 512 threads, FI = 8 rows each, IVX_WAVE = 64; csrc/ivx_scan.hpp: ivxscan::T_ = 256,
I_ = 4, TILE_ = 1024): the packed sweep gives a thread 8 consecutive sorted rows, a wavefront 512, a workgroup a tile of
4096; the fallback scans over unpacked rows give a thread 4, a wavefront 256, a workgroup 1024 (k_head_apply stripes them).

Builders return (key uint32, start int64, end int64, n_keys); rows are well formed (start <= end), input order is a seeded
shuffle unless a case says otherwise.  Positions are indices in stable (key, start) order, which fixes the key at every
sorted position and the position of every run head whatever the order inside equal starts."""
import functools

import numpy as np

FI, WG, FTILE = 8, 512, 4096                 # ivx_runs.hip: FI, IVX_WAVE * FI, FTILE
PACKED = (FTILE, WG, FI)
SCAN = (1024, 256, 4)                         # ivx_scan.hpp: TILE_, IVX_WAVE * I_, I_
FIX_MAXRUN = 64                               # ivx_sweep.hip: longest run of equal (key, start) the two-step sort repairs
LIN_KEYS = 2048                               # ivx_sweep.hip: most keys of the linearised (key, start) word
I64_MAX, I64_MIN, L61 = 2**63 - 1, -(2**63), 2**61
PAIRS = [(0, False), (0, True), (5, True), (5, False)]      # (min_dist, strict) of every family but F


# ---------------------------------------------------------------------------------------------------- the reference walk

def serial_sweep(key, s, e, min_dist=0, strict=False, n_keys=None):
    """The reference rule as a walk over Python ints (merge.rs:291-296, cited at csrc/ivx_runs.hip:64): rows in
    (key, start, end, row) order; a row joins the current run iff  start <= cur_end (+) min_dist  (strict: <) with a saturating
    (+), cur_end becoming max(cur_end, end); a key's first row and every other row open a run with cur_end = end.
    -> (merge rows (key, start, end, count), cluster dict as oracle.cluster gives it)"""
    key, s, e = np.asarray(key), np.asarray(s), np.asarray(e)
    n = len(s)
    order = np.lexsort((np.arange(n), e, s, key))
    ks, ss, es = key[order].tolist(), s[order].tolist(), e[order].tolist()
    nk = int(n_keys if n_keys is not None else (max(ks) + 1 if n else 0))
    mk, ms, me, mc = [], [], [], []
    cl, cs = [0] * n, [0] * n
    key_clusters = [0] * max(nk, 1)
    cur_end = 0
    for i in range(n):
        head = i == 0 or ks[i] != ks[i - 1]
        if not head:
            bound = min(cur_end + min_dist, I64_MAX)
            head = not (ss[i] < bound if strict else ss[i] <= bound)
        if head:
            mk.append(ks[i]); ms.append(ss[i]); me.append(es[i]); mc.append(1)
            key_clusters[ks[i]] += 1
            cur_end = es[i]
        else:
            cur_end = max(cur_end, es[i])
            me[-1] = cur_end
            mc[-1] += 1
        cl[i] = len(mk) - 1
        cs[i] = ms[-1]
    ce = [me[c] for c in cl]
    merge = (np.array(mk, np.uint32), np.array(ms, np.int64), np.array(me, np.int64), np.array(mc, np.int64))
    cluster = dict(key=np.array(ks, np.uint32), start=np.array(ss, np.int64), end=np.array(es, np.int64), row=order.astype(np.uint32),
                   cluster=np.array(cl, np.int64), cluster_start=np.array(cs, np.int64), cluster_end=np.array(ce, np.int64),
                   key_clusters=np.array(key_clusters[:nk], np.uint64), n_clusters=len(mk))
    return merge, cluster


# ---------------------------------------------------------------------------------------------------- predicates

def sorted_keys(key, s):
    """the key at every position of the stable (key, start) order"""
    key, s = np.asarray(key), np.asarray(s)
    return key[np.lexsort((s, key))]


def head_mask(cluster_ids):
    """run heads by sorted position, from the `cluster` column of oracle.cluster (global ids, no key_base): the oracle's
    (key, start, end, row) order differs from the stable (key, start) order only inside equal starts, and a head is the
    first position of such a group in either"""
    c = np.asarray(cluster_ids)
    h = np.ones(len(c), bool)
    h[1:] = c[1:] != c[:-1]
    return h


def fast_groups(ks, wave=WG):
    """complete wave-row groups whose rows share one key: the wavefronts that take the 32-bit path under narrow runs"""
    n = len(ks)
    return [g for g in range(n // wave) if ks[g * wave] == ks[g * wave + wave - 1]]


def opening_fast_groups(ks, wave=WG):
    """... of those, the ones whose first row is the first row of its key (group 0 included)"""
    return [g for g in fast_groups(ks, wave) if g == 0 or ks[g * wave - 1] != ks[g * wave]]


def headless(heads, size):
    """groups of `size` sorted rows (the last one may be partial) without a run head"""
    n = len(heads)
    return [g for g in range((n + size - 1) // size) if not heads[g * size:(g + 1) * size].any()]


def last_row_place(n, geom=PACKED):
    """where row n - 1 falls: (row of its thread, thread of its wavefront, wavefront of its tile, tile)"""
    tile, wave, thr = geom
    i = n - 1
    return i % thr, (i % wave) // thr, (i % tile) // wave, i // tile


# ---------------------------------------------------------------------------------------------------- the host-side forms

def _bits(x):
    return int(x).bit_length()


def range_stats(key, s, e, n_keys):
    """what k_range64 / k_lin_layout64 (csrc/ivx_sweep.hip) learn about the rows, in Python ints: the ranges, the sum of the
    keys' own start ranges (0 when the linearised word cannot be built), the row-shape flags and whether the input is in order"""
    key, s, e = np.asarray(key), np.asarray(s), np.asarray(e)
    st = dict(n=len(s), n_keys=n_keys, min_s=int(s.min()), max_s=int(s.max()), min_e=int(e.min()), max_e=int(e.max()),
              malformed=bool((e < s).any()), has_empty=bool((e == s).any()), lin_total=0)
    if n_keys <= LIN_KEYS:
        o = np.argsort(key, kind="stable")
        ko, so = key[o], s[o]
        first = np.flatnonzero(np.r_[True, ko[1:] != ko[:-1]])
        lo, hi = np.minimum.reduceat(so, first).tolist(), np.maximum.reduceat(so, first).tolist()
        widths = [b - a + 1 for a, b in zip(lo, hi)]
        total = sum(widths)
        if all(w <= 2**62 for w in widths) and 0 < total <= 2**62:
            st["lin_total"] = total
    k_ = key.astype(np.int64)
    below = (k_[1:] < k_[:-1]) | ((k_[1:] == k_[:-1]) & ((s[1:] < s[:-1]) | ((s[1:] == s[:-1]) & (e[1:] < e[:-1]))))
    st["in_order"] = not below.any()                 # (key, start, end) never below the row before
    st["ks_in_order"] = not ((k_[1:] < k_[:-1]) | ((k_[1:] == k_[:-1]) & (s[1:] < s[:-1]))).any()       # (key, start) alone
    o = np.lexsort((s, key))
    edge = np.flatnonzero(np.r_[True, (key[o][1:] != key[o][:-1]) | (s[o][1:] != s[o][:-1]), True])
    st["max_equal_starts"] = int(np.diff(edge).max())                # the longest run of equal (key, start)
    return st


def host_form(key, s, e, n_keys, min_dist=0, strict=False, op="merge", knobs=(), stats=None):
    """What sort64 (csrc/ivx_sweep.hip) and runs_packed (csrc/ivx_runs.hip) decide on the host for these rows, as the words of
    pyivx.Ctx.sweep_form() that follow from the input alone.  op: "merge" (also complement's input rows) or "cluster";
    knobs: the IVX_NO_* variables set; stats: range_stats of the rows, when the caller has them already."""
    st = stats or range_stats(key, s, e, n_keys)
    n = st["n"]
    no_lin, no_fused = "IVX_NO_LIN" in knobs, "IVX_NO_FUSED_SWEEP" in knobs
    min_s, max_s, min_e, max_e = st["min_s"], st["max_s"], st["min_e"], st["max_e"]
    bits_s, bits_e, bits_k = _bits(max_s - min_s), _bits(max_e - min_e), _bits(n_keys - 1 if n_keys else 0)
    lin = 0
    positions = (n_keys or 1) * 2.0 ** bits_s
    if st["lin_total"] and not no_lin and _bits(st["lin_total"] - 1) < bits_k + bits_s:      # fewer bits than key || start
        lin, bits_s, bits_k, positions = 1, _bits(st["lin_total"] - 1), 0, float(st["lin_total"])
    nw = 1 if bits_s + bits_e + bits_k <= 64 else 3
    # ivx_merge_packed_ok
    ok = (nw == 1 and not no_fused and not st["malformed"] and min_dist >= 0 and not (strict and min_dist == 0 and st["has_empty"])
          and n < 0x7FFFFFFF and _bits(n_keys) + bits_e <= 62 and not (lin and (2 * n_keys + 1) * 8 > 40 * 1024))
    packed = (1 if op == "merge" else 2) if ok else 0
    small = min_s > -L61 and max_s < L61 and min_e > -L61 and max_e < L61
    upper = bits_s if lin else bits_s + _bits(n_keys - 1 if n_keys else 0)
    narrow_runs = int(bool(packed and small and bits_e <= 32 and upper <= 32 and min_dist < L61 and "IVX_NO_NARROW_RUNS" not in knobs))
    f = dict(nw=nw, lin=lin, bits_s=bits_s, bits_e=bits_e, bits_k=bits_k, packed=packed, narrow_runs=narrow_runs,
             ntile=(n + FTILE - 1) // FTILE if packed else 0)
    # rows in (key, start, end) order are copied as they are (wide) unless the sweep takes the packed words instead of rows
    copied = st["in_order"] and packed != 1
    narrow_rows = (op == "merge" and not copied and nw == 1 and "IVX_NO_NARROW_SWEEP" not in knobs
                   and max_s - min_s <= 0xFFFFFFFF and max_e - min_e <= 0xFFFFFFFF)
    f["narrow_rows"] = int(narrow_rows)
    f["k8"] = int(narrow_rows and n_keys <= 256 and "IVX_NO_K8" not in knobs)
    # how the order is reached: input in order is taken as it is ((key, start) order is enough for the packed words alone); the packed
    # words are sorted on their (key, start) bits; rows on one word are sorted on those bits and the runs of equal starts repaired
    # when that pays (or nothing is sorted at all: (key, start) order) -- unless a run exceeds FIX_MAXRUN -- else on the whole word
    sorted_in = st["in_order"] or (packed == 1 and st["ks_in_order"])
    two_step = toolong = 0
    if sorted_in:
        sort_words = 0
    elif packed == 1:
        sort_words = 1
    elif nw == 3:
        sort_words = 3
    else:
        two_step = int(st["ks_in_order"] or (bits_e >= 8 and n >= 65536 and n / positions <= 0.25))
        toolong = int(two_step and st["max_equal_starts"] > FIX_MAXRUN)
        sort_words = 0 if st["ks_in_order"] and not toolong else 1
    f.update(sorted_in=int(sorted_in), two_step=two_step, toolong=toolong, sort_words=sort_words)
    return f


# ---------------------------------------------------------------------------------------------------- building blocks

class _Rows:
    """rows collected in sorted order, key by key"""

    def __init__(self):
        self.k, self.s, self.e = [], [], []
        self.key = None

    def __len__(self):
        return len(self.s)

    def open(self, key, origin):
        assert self.key is None or key > self.key
        self.key, self.origin, self.cur_end, self.prev_s = key, origin, None, None

    def at(self, s, e):
        assert e > s and (self.prev_s is None or s >= self.prev_s)
        self.k.append(self.key); self.s.append(s); self.e.append(e)
        self.cur_end = e if self.cur_end is None else max(self.cur_end, e)
        self.prev_s = s
        return len(self.s) - 1

    def head(self, length=20):
        """a row 100 beyond every earlier end of its key: a run head under every (min_dist, strict) of PAIRS"""
        s = self.origin if self.cur_end is None else self.cur_end + 100
        return self.at(s, s + length)

    def cont(self, length=20):
        """a row one past its predecessor's start, inside the current run under every pair"""
        assert self.prev_s + 1 < self.cur_end
        return self.at(self.prev_s + 1, self.prev_s + 1 + length)

    def pattern(self, count, salt=0):
        """count rows, heads at a fixed pseudo-random 1-in-11 subset (and the key's first row)"""
        for _ in range(count):
            i = len(self.s)
            if self.cur_end is None or ((i + salt) * 2654435761 % 2**32) % 11 == 0:
                self.head(12 + i % 9)
            else:
                self.cont(12 + i % 9)

    def alternate(self, count):
        """count rows, every other one a head (from the first): no thread's rows are all of one run"""
        for j in range(count):
            self.head() if j % 2 == 0 else self.cont()

    def done(self, n_keys, seed=1, perm=None):
        k, s, e = np.array(self.k, np.uint32), np.array(self.s, np.int64), np.array(self.e, np.int64)
        assert (e > s).all() and k.max() < n_keys
        if perm is None:
            perm = np.random.default_rng([77, seed, len(s)]).permutation(len(s))
        return k[perm], s[perm], e[perm], n_keys


class Case:
    """name, builder, the (min_dist, strict) pairs it runs with, the claims its name makes (test_run_forms_cpu.py checks
    them) and the settings it runs under beyond the default ones"""

    def __init__(self, name, family, build, claims=None, pairs=PAIRS, geom=PACKED, serial=True, device=False, complement=False,
                 only_knobs=None):
        self.name, self.family, self._build, self.claims, self.pairs = name, family, build, claims or {}, list(pairs)
        self.geom, self.serial, self.device, self.complement, self.only_knobs = geom, serial, device, complement, only_knobs

    @functools.lru_cache(maxsize=None)
    def rows(self):
        k, s, e, nk = self._build()
        for a in (k, s, e):
            a.setflags(write=False)
        return k, s, e, nk

    @functools.lru_cache(maxsize=None)
    def stats(self):
        return range_stats(*self.rows())


CASES = {}


def _case(name, family, build, **kw):
    assert name not in CASES, name
    CASES[name] = Case(name, family, build, **kw)


# ---------------------------------------------------------------------------------------------------- A: row counts

A_SIZES = [1, 7, 8, 9, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 4608, 8191, 8192, 8193, 12296]
A_SIZES_SCAN = [255, 256, 257, 2047, 2048, 2049]           # the fallback scans' wavefront and tile, under the two fallback settings


def a_rows(n, runs):
    """one key, n rows: every row its own run ("each"), all rows one run ("one"), heads at a 1-in-11 subset ("mix")"""
    r = _Rows()
    r.open(0, 1000)
    if runs == "mix":
        r.pattern(n)
    else:
        for i in range(n):
            r.head() if (i == 0 or runs == "each") else r.cont()
    return r.done(1, seed=n)


for _n in A_SIZES + A_SIZES_SCAN:
    for _runs in ("each", "one", "mix"):
        _scan = _n in A_SIZES_SCAN
        _geom = SCAN if _scan else PACKED
        _claims = dict(n=_n, last_row=last_row_place(_n, _geom))
        if _runs == "one":
            _claims["heads"] = [0]
            _claims["headless_tiles"] = list(range(1, (_n + _geom[0] - 1) // _geom[0]))
        if _runs == "each":
            _claims["all_heads"] = True
        _case(f"A_n{_n}_{_runs}", "A", functools.partial(a_rows, _n, _runs), claims=_claims, geom=_geom, device=True,
              only_knobs="fallback" if _scan else None)


def a_few_runs(n=1024 * 1024 + 1):
    """one key, five long runs over n rows: 1025 tiles of the fallback scans, so that scan_rec over the tile sums takes its
    second level, almost all of them without a head"""
    i = np.random.default_rng([3, n]).permutation(n).astype(np.int64)
    run = i * 5 // n
    s = 1000 + i * 3 + run * 10_000
    e = s + 40
    return np.zeros(n, np.uint32), s, e, 1


_case("A_n1048577_five_runs", "A", a_few_runs, pairs=[(0, False), (5, True)], geom=SCAN, only_knobs="fallback",
      claims=dict(n=1024 * 1024 + 1, n_heads=5, last_row=last_row_place(1024 * 1024 + 1, SCAN), min_headless_tiles=1000))


# ---------------------------------------------------------------------------------------------------- B: key boundaries

def b_rows(at, delta, prev="larger"):
    """Keys 1, 2, 4, 5 with rows; 0, 3, 6 and 7 without (n_keys = 8).  Key 1 holds at + delta rows, so the first key boundary
    falls there; key 2 holds a whole wavefront and more, so in the exact cases the wavefront behind the boundary is complete
    and single-key; its first eight rows alternate between heads and rows inside a run.  prev: the end offsets of key 1 against those of key 2 (the cur_end a fast wavefront inherits)."""
    r = _Rows()
    hi, lo = 5_000_000, 1000
    r.open(1, hi if prev == "larger" else lo)
    r.pattern(at + delta)
    r.open(2, lo if prev == "larger" else hi)
    r.alternate(FI)                                 # (heads among the rows of the thread that opens the key)
    r.pattern(WG + 37 - FI, salt=3)
    r.open(4, 70_000)
    r.pattern(100, salt=5)
    r.open(5, 20_000)
    r.pattern(50, salt=7)
    return r.done(8, seed=at * 4 + delta + 1)


for _at in (8, 512, 4096):
    for _delta in (-1, 0, 1):
        for _prev in (("larger", "smaller") if _delta == 0 and _at != 8 else ("larger",)):
            _claims = dict(key_boundary=_at + _delta, n_keys=8, empty_keys=[0, 3, 6, 7])
            if _delta == 0 and _at != 8:
                _claims["opening_fast_group"] = _at // WG
                _claims["heads_behind_boundary"] = 4
                _claims["prev_end"] = _prev
            _case(f"B_at{_at}{_delta:+d}_{_prev}", "B", functools.partial(b_rows, _at, _delta, _prev), claims=_claims, device=True,
                  complement=True)


# ---------------------------------------------------------------------------------------------------- C: long runs

def c_next_head(where, geom):
    tile, wave, thr = geom
    return {"mid": 2 * tile + wave + 3 * thr + 3, "thread": 2 * tile + wave + 5 * thr, "wave": 2 * tile + 2 * wave, "tile": 3 * tile}[where]


def c_rows(where, two_keys, geom=PACKED):
    """One run from the middle of tile 0 to the next head, which sits in or at the end of tile 2: a long first row, then
    short rows inside it -- tile 1 and the wavefronts between hold no head.  two_keys: 300 rows of another key come first (and
    keys without rows around them); positions are global either way."""
    tile, wave, thr = geom
    p0, p1 = tile // 2 + 5, c_next_head(where, geom)
    r = _Rows()
    if two_keys:
        r.open(1, 9_000_000)
        r.pattern(300, salt=1)
        r.open(3, 500)
    else:
        r.open(0, 500)
    r.pattern(p0 - len(r), salt=2)
    S = r.cur_end + 100
    assert r.at(S, S + 10**6) == p0
    while len(r) < p1:
        r.at(S + 1 + len(r), S + 11 + len(r))
    assert r.head() == p1
    r.pattern(wave + 36, salt=4)
    return r.done(5 if two_keys else 1, seed=p1 + two_keys)


for _geom, _gname in ((PACKED, ""), (SCAN, "_scan")):
    for _where in ("mid", "thread", "wave", "tile"):
        for _two in (False, True):
            _p0, _p1 = _geom[0] // 2 + 5, c_next_head(_where, _geom)
            _case(f"C_{_where}{'_key2' if _two else ''}{_gname}", "C", functools.partial(c_rows, _where, _two, _geom), geom=_geom, device=True,
                  complement=not _gname, only_knobs="fallback" if _gname else None,
                  claims=dict(heads_at=[_p0, _p1], no_heads_in=(_p0 + 1, _p1), headless_tiles=[1], min_headless_groups=_geom[0] // _geom[1],
                              next_head_place=_where))


# ---------------------------------------------------------------------------------------------------- D: where the maximum sits

def d_place(where, geom):
    tile, wave, thr = geom
    return {"key_first": wave + 5, "thread_last": wave + 5 * thr + thr - 1, "wave_last": 3 * wave - 1, "tile_last": tile - 1}[where]


D_FOLLOW = 20


def d_rows(where, geom=PACKED):
    """The row at position P ends far beyond its neighbours; the D_FOLLOW rows behind it are short, 90 apart from each other and
    inside it: each of them is a head unless P's end reaches it as cur_end.  The row after them starts a run."""
    tile, wave, thr = geom
    P = d_place(where, geom)
    r = _Rows()
    if where == "key_first":
        r.open(1, 10_000_000)                       # (the key before: larger coordinates, so its ends must not carry over)
        r.pattern(P, salt=1)
        r.open(2, 1000)
        sP = 1000
    else:
        r.open(0, 1000)
        r.pattern(P, salt=1)
        sP = r.cur_end + 100
    assert r.at(sP, sP + 5000) == P
    for j in range(1, D_FOLLOW + 1):
        r.at(sP + 100 * j, sP + 100 * j + 10)
    assert r.head() == P + D_FOLLOW + 1
    r.pattern(wave + 12, salt=6)
    return r.done(4 if where == "key_first" else 1, seed=P)


for _geom, _gname in ((PACKED, ""), (SCAN, "_scan")):
    for _where in ("key_first", "thread_last", "wave_last", "tile_last"):
        _P = d_place(_where, _geom)
        _case(f"D_{_where}{_gname}", "D", functools.partial(d_rows, _where, _geom), geom=_geom, only_knobs="fallback" if _gname else None,
              claims=dict(heads_at=[_P, _P + D_FOLLOW + 1], no_heads_in=(_P + 1, _P + D_FOLLOW + 1), max_end_place=(_where, _P)))


# ---------------------------------------------------------------------------------------------------- E: equal starts

E_GROUPS = [(1005, 6), (1516, 40), (2047, 2), (4090, 17)]    # (first position, rows): across a thread, a wavefront, a thread pair, a tile


def e_rows(largest):
    """One key; at each E_GROUPS position a group of rows sharing their start, ends all different, the largest end first, last
    or in the middle of the group's INPUT order (the packed words are sorted on (key, start) only and keep it).  The row behind
    a group starts one below the group's largest end and beyond every other end of it."""
    r = _Rows()
    r.open(0, 1000)
    members = []
    for pos, cnt in E_GROUPS:
        r.pattern(pos - len(r), salt=pos)
        s = r.cur_end + 100
        ends = [s + 10 + 3 * j for j in range(cnt - 1)] + [s + 1000]
        members.append((len(r), ends))
        for en in ends:
            r.at(s, en)
        r.at(s + 999, s + 1010)                     # inside the run only through the largest end
    r.pattern(WG + 3, salt=9)
    n = len(r)
    perm = np.random.default_rng([5, n]).permutation(n)          # input slot -> sorted row
    slot_of = np.empty(n, np.int64)
    slot_of[perm] = np.arange(n)
    for first, ends in members:
        cnt = len(ends)
        slots = np.sort(slot_of[first:first + cnt])
        big = {"first": 0, "last": cnt - 1, "middle": cnt // 2}[largest]
        rows = [first + j for j in range(cnt - 1)]
        rows.insert(big, first + cnt - 1)                           # the group's rows in input order
        perm[slots] = rows
    return r.done(1, perm=perm)


for _largest in ("first", "last", "middle"):
    _case(f"E_largest_{_largest}", "E", functools.partial(e_rows, _largest),
          claims=dict(equal_groups=E_GROUPS, largest=_largest, heads_at=[p for p, _ in E_GROUPS], no_heads_in_groups=True))


# ---------------------------------------------------------------------------------------------------- F: the threshold

F_SPOTS = {"lane0_row0": (512, 1024, 1536), "lane63_row7": (1023, 2047, 2559), "mid": (700, 1300, 1900)}   # positions for d - 1, d, d + 1
F_N = 3072 + 21


def f_rows(d, mixed, empty=False):
    """Every ordinary row starts 50 beyond cur_end; the rows at F_SPOTS start exactly d - 1, d and d + 1 beyond it.  mixed: a
    key boundary at 300 + 512 g puts one into every wavefront (they all take the generic path); else one key.  empty: one
    row with end == start, which takes strict min_dist = 0 off the packed sweep."""
    spot = {p: d - 1 + j for ps in F_SPOTS.values() for j, p in enumerate(ps)}
    r = _Rows()
    key = 1
    r.open(key, 1000)
    for i in range(F_N):
        if mixed and i >= 300 and (i - 300) % WG == 0:
            key += 1
            r.open(key, 1000 + 7 * key)
        if r.cur_end is None:
            r.head()
        elif i in spot:
            r.at(r.cur_end + spot[i], r.cur_end + spot[i] + 20)
        elif empty and i == 777:
            r.k.append(r.key); r.s.append(r.cur_end + 50); r.e.append(r.cur_end + 50)      # (not through at(): end == start)
            r.prev_s = r.cur_end = r.cur_end + 50
        else:
            r.at(r.cur_end + 50, r.cur_end + 70)
    k, s, e = np.array(r.k, np.uint32), np.array(r.s, np.int64), np.array(r.e, np.int64)
    perm = np.random.default_rng([6, d, int(mixed), int(empty)]).permutation(len(s))
    return k[perm], s[perm], e[perm], key + 2


for _d in (0, 1, 5):
    for _mixed in (False, True):
        _case(f"F_d{_d}_{'mixed' if _mixed else 'one_key'}", "F", functools.partial(f_rows, _d, _mixed), pairs=[(_d, False), (_d, True)],
              claims=dict(threshold=_d, spots=F_SPOTS, mixed=_mixed))
_case("F_d0_one_key_empty_row", "F", functools.partial(f_rows, 0, False, True), pairs=[(0, False), (0, True)],
      claims=dict(threshold=0, spots=F_SPOTS, mixed=False, has_empty=True))


# ---------------------------------------------------------------------------------------------------- G: bit widths of the word

def g_rows(n, kind):
    r = np.random.default_rng([8, n])
    i = np.arange(n, dtype=np.int64)
    if kind == "ends_equal":                        # two keys, every end the same: bits_e = 0, each key one run
        k = (i >= 1000).astype(np.uint32)
        s = 5000 + 3 * i
        e = np.full(n, int(s.max()) + 10, np.int64)
        nk = 2
    elif kind == "starts_equal":                    # one (key, start) for all rows: bits_s = 0, a run far above FIX_MAXRUN
        k = np.zeros(n, np.uint32)
        s = np.full(n, -12345, np.int64)
        e = s + 1 + i
        nk = 1
    elif kind in ("ends_2e32m1", "ends_2e32"):      # the range of ends: 2^32 - 1 (bits_e = 32, emask all ones), 2^32 (bits_e = 33)
        k = np.zeros(n, np.uint32)
        s = 7_000 + 30 * i
        e = s + 20 + (i % 3) * 15                   # gaps of 10 behind a short row, overlaps behind a long one
        e[-1] = int(e.min()) + 2**32 - (1 if kind == "ends_2e32m1" else 0)
        nk = 1
    else:                                           # four keys, bits_s = 30 or 31: key || start takes 32 or 33 bits without lin
        k = (i * 4 // n).astype(np.uint32)
        s = -2**29 + 30 * i
        e = s + 20 + (i % 3) * 15
        s[-1] = int(s.min()) + 2**30 - (1 if kind == "keystart_32" else 0)
        e[-1] = s[-1] + 5
        nk = 4
    p = r.permutation(n)
    return k[p], s[p], e[p], nk


G_FORMS = {                                        # what the case must reach under default settings / IVX_NO_LIN
    "ends_equal": dict(default=dict(bits_e=0, narrow_runs=1)),
    "starts_equal": dict(default=dict(bits_s=0, lin=0, narrow_runs=1)),
    "ends_2e32m1": dict(default=dict(bits_e=32, narrow_runs=1, narrow_rows=1)),
    "ends_2e32": dict(default=dict(bits_e=33, narrow_runs=0, packed=1, narrow_rows=0)),
    "keystart_32": dict(IVX_NO_LIN=dict(bits_s=30, bits_k=2, lin=0, narrow_runs=1)),
    "keystart_33": dict(IVX_NO_LIN=dict(bits_s=31, bits_k=2, lin=0, narrow_runs=0, packed=1)),
}
for _n in (4097, 8192):
    for _kind in G_FORMS:
        _case(f"G_n{_n}_{_kind}", "G", functools.partial(g_rows, _n, _kind), claims=dict(n=_n, forms=G_FORMS[_kind]))


# ---------------------------------------------------------------------------------------------------- H: two scan levels

H_N = 1025 * FTILE + 3
H_EDGE = 1024 * FTILE                               # first row of tile 1024: the first tile of the second scan block


def _local(rng, n, gap=40, max_len=250):
    """genomic-like offsets (ascending) and lengths, as local() of tests/test_gpu_sweeps_wide.py but without empty rows (they
    would take strict min_dist = 0 off the packed sweep): about 1 row in 17 shares its start with the row before it"""
    g = rng.integers(0, 2 * gap, n)
    g[rng.random(n) < 1 / 17] = 0
    wide = rng.random(n) < 0.004
    g[wide] += rng.integers(10 * max_len, 100 * max_len, int(wide.sum()))
    g[0] = 0
    return np.cumsum(g).astype(np.int64), rng.integers(1, max_len, n).astype(np.int64)


def h_rows(variant):
    """24 keys, H_N rows: 1026 tiles, so both tile-summary scans of runs_packed take a second level.  "run": one run is forced
    across H_EDGE; "key": a key boundary sits exactly on it, with a whole wavefront of the new key behind it."""
    rng = np.random.default_rng([9, int(variant == "key")])
    if variant == "run":
        counts = [H_N // 24] * 23
        counts.append(H_N - sum(counts))
    else:
        counts = [349525] * 11
        counts.append(H_EDGE - sum(counts))
        counts += [600] + [318] * 10
        counts.append(H_N - sum(counts))
    assert len(counts) == 24 and sum(counts) == H_N and min(counts) > 0
    ks, ss, es = [], [], []
    first = 0
    for kk, c in enumerate(counts):
        off, ln = _local(rng, c)
        if variant == "key" and first == H_EDGE:    # the thread that opens the key: eight runs of one short row each
            off, ln = off + 8000, ln.copy()
            off[:FI], ln[:FI] = 1000 * np.arange(FI), 10
        s = 1000 * (kk % 7) + off
        e = s + ln
        if variant == "run" and first <= H_EDGE < first + c:
            j = H_EDGE - first - 3
            e[j] = s[j + 40] + 1000                 # (starts ascend: the row covers the forty behind it)
        ks.append(np.full(c, kk, np.uint32)); ss.append(s); es.append(e)
        first += c
    k, s, e = np.concatenate(ks), np.concatenate(ss), np.concatenate(es)
    p = rng.permutation(H_N)
    return k[p], s[p], e[p], 24


_case("H_run_across_scan_block", "H", functools.partial(h_rows, "run"), serial=False, only_knobs="H",
      claims=dict(n=H_N, ntile=1026, no_heads_in=(H_EDGE, H_EDGE + 30)))
_case("H_key_on_scan_block", "H", functools.partial(h_rows, "key"), serial=False, only_knobs="H",
      claims=dict(n=H_N, ntile=1026, key_boundary=H_EDGE, opening_fast_group=H_EDGE // WG, heads_behind_boundary=FI))


# ---------------------------------------------------------------------------------------------------- I: many small keys

I_N = 2 * FTILE + 1


def i_rows(n_keys):
    """3 to 5 rows in most keys, none in about a fifth of them (key 0, the last key, every fifth key below 1900 and keys
    100..109 in a row): every thread's 8 rows cross keys and the per-row key walk has keys to skip.  I_N rows: one past a tile."""
    empty = {0, n_keys - 1} | {kk for kk in range(1900) if kk % 5 == 4} | set(range(100, 110))
    used = [kk for kk in range(n_keys) if kk not in empty]
    cnt = [5] * len(used)
    over, i = 5 * len(used) - I_N, 0
    assert over >= 0
    while over > 0:
        take = min(2 if i % 3 == 0 else 1, over)
        cnt[i] -= take
        over -= take
        i += 1
    r = _Rows()
    for kk, c in zip(used, cnt):
        r.open(kk, 1000 + (kk * 97) % 5000)
        for j in range(c):
            r.head(30) if j % 2 == 0 else r.cont(45)
    assert len(r) == I_N
    return r.done(n_keys, seed=n_keys)


for _nk in (2048, 2049):
    _case(f"I_keys{_nk}", "I", functools.partial(i_rows, _nk),
          claims=dict(n=I_N, n_keys=_nk, lin=int(_nk <= LIN_KEYS), last_row=last_row_place(I_N), rows_per_key=(3, 5), no_fast_groups=True,
                      empty_run=(100, 110)))
