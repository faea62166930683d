"""-m gpu: the radix sort (csrc/ivx_sort.hip) where only large inputs used to take it, bit-exact against numpy's stable sort.

A workgroup sorts a chunk of whole tiles (8192 records, 4096 for three-word records).  Below 1024 tiles of input a chunk is
one tile, so the second trip of k_scatter's tile loop, its carry gbase += tcnt, the prefetch of the next (full or partial)
tile and a short last tile behind a full one ran only in the property checks at 50 M rows and more.  IVX_SORT_CHUNK_TILES
makes a chunk k tiles at any size; every chunk test reads the geometry back from the hook (ivx_debug_sort_geom) and asserts
that a workgroup walked two tiles or more.  Two cases cross the natural switch (1024 tiles + 1 record) without the knob.

The other cases are small: fields at every bit position, pass counts of both parities, digit patterns inside one tile, the
two sides of the histogram scan's first threshold, and merge / cluster over the histogram that the sweeps' pack kernel
prepares for the sort's workgroups (k_pack1h), with chunks of two tiles.

The reference is _ref of test_gpu_sort.py: a stable argsort per field, least significant first.  Records carry their row
number in bits that are not sorted on (or in the payload), so a stable sort has exactly one right answer."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402
import test_gpu_sweeps_wide as wide  # noqa: E402

pytestmark = pytest.mark.gpu

U = np.uint64
FORMS = ["w1", "w1pay", "w2", "w3"]                   # one word (the prefetching kernel), one word + payload, two words, three
NW = {"w1": 1, "w1pay": 1, "w2": 2, "w3": 3}
TILE = {"w1": 8192, "w1pay": 8192, "w2": 8192, "w3": 4096}      # Tile<NW>::N


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


@contextlib.contextmanager
def chunk_tiles(k):
    """IVX_SORT_CHUNK_TILES = k for the calls inside; None: unset"""
    old = os.environ.pop("IVX_SORT_CHUNK_TILES", None)
    if k is not None:
        os.environ["IVX_SORT_CHUNK_TILES"] = str(k)
    try:
        yield
    finally:
        os.environ.pop("IVX_SORT_CHUNK_TILES", None)
        if old is not None:
            os.environ["IVX_SORT_CHUNK_TILES"] = old


def gpu_sort(ctx, words, fields, tight, pay=None):
    """-> (sorted words, sorted payload or None, chunk, nblk, in_b)"""
    n = len(words[0])
    arrs = [np.ascontiguousarray(w, np.uint64).copy() for w in words] + [None] * (3 - len(words))
    gp = None if pay is None else np.ascontiguousarray(pay, np.uint32).copy()
    fw = (C.c_int * len(fields))(*[f[0] for f in fields])
    fl = (C.c_int * len(fields))(*[f[1] for f in fields])
    fh = (C.c_int * len(fields))(*[f[2] for f in fields])
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    geom = (C.c_uint64 * 3)()
    st = pyivx.lib().ivx_debug_sort_geom(ctx.h, C.c_int(len(words)), p(arrs[0]), p(arrs[1]), p(arrs[2]), p(gp), C.c_uint64(n),
                                         fw, fl, fh, C.c_int(len(fields)), C.c_int(int(tight)), geom)
    assert st == 0, pyivx.lib().ivx_last_error(ctx.h)
    return arrs[:len(words)], gp, int(geom[0]), int(geom[1]), int(geom[2])


def field_of(w, lo, hi):
    if hi - lo >= 64:
        return w
    return (w >> U(lo)) & ((U(1) << U(hi - lo)) - U(1))


def ref_order(words, fields):
    order = np.arange(len(words[0]))
    for w, lo, hi in fields:                          # LSD: least significant criterion first, stable
        k = field_of(words[w][order], lo, hi)
        if hi - lo <= 16:
            k = k.astype(np.uint16)                   # (numpy's stable sort of 16-bit keys is a radix sort: the 8 M-row cases)
        order = order[np.argsort(k, kind="stable")]
    return order


def passes(words, fields, tight):
    """the scatter passes sort_impl runs: every 8-bit digit of every field when tight, else those in which a bit of the
    field varies over the input (restated from the host code)"""
    c = 0
    for w, lo, hi in fields:
        x = words[w]
        var = int(np.bitwise_or.reduce(x ^ x[0])) if len(x) else 0
        fieldmask = (1 << hi) - 1
        for sh in range(lo, hi, 8):
            window = ((1 << (sh + 8)) - 1) & ~((1 << sh) - 1) & (2**64 - 1)
            if tight or (var & window & fieldmask):
                c += 1
    return c


def check(ctx, words, fields, tight, pay=None):
    """sort, compare words and payload with the reference, assert in_b from the pass count; -> (chunk, nblk, in_b)"""
    gw, gp, chunk, nblk, in_b = gpu_sort(ctx, words, fields, tight, pay)
    n = len(words[0])
    order = ref_order(words, fields)
    for q, (g, w) in enumerate(zip(gw, words)):
        assert np.array_equal(g, w[order]), f"word {q}, tight={tight}"
    if pay is not None:
        assert np.array_equal(gp, pay[order]), f"payload, tight={tight}"
    assert nblk == (-(-n // chunk) if n else 0)
    assert in_b == (passes(words, fields, tight) & 1 if n > 1 else 0), f"in_b={in_b}, tight={tight}"
    return chunk, nblk, in_b


def tied(rng, n, bits, distinct=300):
    """n values of `bits` bits drawn from at most `distinct` different ones: heavy ties, every digit varies"""
    if bits < 64:
        pool = rng.integers(0, 1 << bits, min(distinct, 1 << bits), dtype=np.uint64)
    else:
        pool = rng.integers(0, 1 << 63, distinct, dtype=np.uint64) * U(2) + rng.integers(0, 2, distinct, dtype=np.uint64)
    pool[:2] = np.array([0, (1 << bits) - 1], np.uint64)          # (all-zeros and all-ones: every bit of the field varies)
    return pool[rng.integers(0, len(pool), n)]


def rows(n):
    return np.arange(n, dtype=np.uint64)


def records(form, rng, n):
    """(words, fields, payload): heavy ties in every field, garbage above the fields, the row number in unsorted bits"""
    junk = lambda sh: rng.integers(0, 1 << (64 - sh), n, dtype=np.uint64) << U(sh)
    if form in ("w1", "w1pay"):
        # field: bits [20, 36), two passes; the row number below it, garbage above
        w0 = (tied(rng, n, 16) << U(20)) | rows(n) | junk(36)
        return [w0], [(0, 20, 36)], (rng.integers(0, 1 << 32, n, dtype=np.uint32) if form == "w1pay" else None)
    if form == "w2":
        w0 = (tied(rng, n, 16, 40) << U(8)) | (rows(n) & U(0xFF)) | junk(24)
        w1 = (tied(rng, n, 16, 40) << U(32)) | rows(n) | junk(48)
        return [w0, w1], [(0, 8, 24), (1, 32, 48)], None
    w0 = tied(rng, n, 8, 7) | junk(8)
    w1 = (tied(rng, n, 16, 9) << U(4)) | junk(20)
    w2 = (tied(rng, n, 8, 5) << U(40)) | rows(n) | junk(48)
    return [w0, w1, w2], [(0, 0, 8), (1, 4, 20), (2, 40, 48)], None


# ---------------------------------------------------------------- chunks of several tiles under the knob

CHUNK_NS = {"k*t": lambda k, t: k * t,                             # one workgroup, k full tiles
            "k*t+1": lambda k, t: k * t + 1,                       # a second workgroup holds one record
            "2*k*t-1": lambda k, t: 2 * k * t - 1,                 # the second workgroup's last tile lacks one record
            "(k+1)*t+5": lambda k, t: (k + 1) * t + 5,             # the second workgroup: a full tile, then 5 records
            "3*k*t+t/2": lambda k, t: 3 * k * t + t // 2}          # a fourth workgroup with half a tile


@pytest.mark.parametrize("which", list(CHUNK_NS))
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("form", FORMS)
def test_chunk_of_several_tiles(ctx, form, k, which):
    t = TILE[form]
    n = CHUNK_NS[which](k, t)
    words, fields, pay = records(form, np.random.default_rng([1, FORMS.index(form), k, n]), n)
    with chunk_tiles(k):
        for tight in (0, 1):
            chunk, nblk, _ = check(ctx, words, fields, tight, pay)
            # the knob took: a workgroup's chunk is k tiles, and the first workgroup holds min(n, chunk) records of it
            assert chunk == k * t and chunk >= 2 * t and min(n, chunk) >= 2 * t and nblk == -(-n // chunk)


def test_chunk_knob_values(ctx):
    """1..8 set the chunk; anything else leaves the default (one tile at this size)"""
    n = 20_000
    words, fields, pay = records("w1pay", np.random.default_rng(2), n)
    for v, want in [("1", 8192), ("8", 65536), ("0", 8192), ("9", 8192), ("12", 8192), ("", 8192), ("x", 8192), (None, 8192)]:
        with chunk_tiles(v):
            assert check(ctx, words, fields, 1, pay)[0] == want, v


# ---------------------------------------------------------------- the natural switch, no knob

@pytest.mark.parametrize("form", ["w1pay", "w3"])
def test_chunk_natural_switch(ctx, form):
    """one record more than 1024 tiles: sort_chunk gives two tiles per workgroup on its own.  The keys vary in 16 bits only
    (two passes, and numpy sorts them by radix)"""
    t = TILE[form]
    n = 1024 * t + 1
    rng = np.random.default_rng([3, t])
    key = rng.integers(0, 1 << 16, n, dtype=np.uint64)                  # (64 and more records per value: ties)
    if form == "w1pay":
        words, fields, pay = [(key << U(24)) | (rows(n) & U(0xFFFFFF))], [(0, 24, 40)], np.arange(n, dtype=np.uint32)
    else:
        words, fields, pay = [rows(n), key << U(16), rng.integers(0, 1 << 63, n, dtype=np.uint64)], [(1, 16, 32)], None
    with chunk_tiles(None):
        chunk, nblk, in_b = check(ctx, words, fields, 1, pay)
    assert chunk == 2 * t and nblk == 513 and in_b == 0


# ---------------------------------------------------------------- fields at any bit position, pass counts

# (lo, hi): lo off the byte grid; widths 1, 7, 9, 33; hi = 64; lo = 56; one to four (and five) passes; an empty field
POSITIONS = [(3, 4), (5, 12), (13, 22), (5, 38), (31, 64), (60, 64), (56, 64), (8, 16), (8, 24), (9, 33), (8, 40), (17, 17), (0, 64)]


def positioned(form, rng, n, lo, hi):
    """records whose LAST word holds the field [lo, hi): ties in the field, the row number below lo (as much of it as
    fits; the first word or the payload holds all of it), ones between hi and the end of the field's last digit -- a
    constant that is not zero --, garbage above"""
    nw = NW[form]
    end = min(64, lo + -(-(hi - lo) // 8) * 8) if hi > lo else hi        # end of the last digit
    w = (tied(rng, n, hi - lo) << U(lo)) if hi > lo else np.zeros(n, np.uint64)
    if lo:
        w |= rows(n) & ((U(1) << U(lo)) - U(1))
    if end > hi:
        w |= ((U(1) << U(end - hi)) - U(1)) << U(hi)
    if end < 64:
        w |= rng.integers(0, 1 << (64 - end), n, dtype=np.uint64) << U(end)
    words = [rows(n) for _ in range(nw - 1)] + [w]
    return words, [(nw - 1, lo, hi)], (np.arange(n, dtype=np.uint32) if form == "w1pay" else None)


@pytest.mark.parametrize("lo,hi", POSITIONS)
@pytest.mark.parametrize("form", FORMS)
def test_field_positions(ctx, form, lo, hi):
    n = 10_007                                         # two or three workgroups, the last one partial
    words, fields, pay = positioned(form, np.random.default_rng([4, lo, hi]), n, lo, hi)
    for tight in (0, 1):
        _, _, in_b = check(ctx, words, fields, tight, pay)
        if tight:
            assert in_b == (-(-(hi - lo) // 8)) & 1    # both parities, for words and payload
        if hi == lo:
            assert in_b == 0                           # (check() has compared the order: unchanged)


@pytest.mark.parametrize("form", FORMS)
def test_two_fields_sharing_a_digit(ctx, form):
    """[4, 13) and above it [13, 20) of one word: the lower field's last digit [12, 20) reads the upper field's bits; the
    upper field's own digit [13, 21) reads bit 20, a constant"""
    n, nw = 9_001, NW[form]
    rng = np.random.default_rng(5)
    w = (tied(rng, n, 9, 20) << U(4)) | (tied(rng, n, 7, 10) << U(13)) | (rows(n) & U(0xF)) | (U(1) << U(20)) | (rng.integers(0, 1 << 40, n, dtype=np.uint64) << U(21))
    words = [rows(n) for _ in range(nw - 1)] + [w]
    for tight in (0, 1):
        check(ctx, words, [(nw - 1, 4, 13), (nw - 1, 13, 20)], tight, np.arange(n, dtype=np.uint32) if form == "w1pay" else None)


@pytest.mark.parametrize("form", FORMS)
def test_constant_digits_not_tight(ctx, form):
    """a sort that is not tight skips the digits that do not vary: none varies (no pass, the order stays), only a middle
    one does (one pass)"""
    n, nw = 12_345, NW[form]
    rng = np.random.default_rng(6)
    pay = np.arange(n, dtype=np.uint32) if form == "w1pay" else None
    other = rng.integers(0, 1 << 8, n, dtype=np.uint64) | (rng.integers(0, 1 << 24, n, dtype=np.uint64) << U(40))   # outside [8, 40)
    const = other | (U(0x5A00C3) << U(8))
    words = [rows(n) for _ in range(nw - 1)] + [const]
    _, _, in_b = check(ctx, words, [(nw - 1, 8, 40)], 0, pay)
    assert in_b == 0
    middle = other | (U(0x5A0000C3) << U(8)) | (tied(rng, n, 8, 50) << U(24))
    words = [rows(n) for _ in range(nw - 1)] + [middle]
    assert passes(words, [(nw - 1, 8, 40)], 0) == 1
    _, _, in_b = check(ctx, words, [(nw - 1, 8, 40)], 0, pay)
    assert in_b == 1


# ---------------------------------------------------------------- digit patterns inside a tile

def _digits(pattern, rng, t):
    i = np.arange(t)
    if pattern == "all_lanes_differ":                  # the 64 records of a wavefront's round: 64 different digits
        return (i % 64) * 4 + (i // 64) % 4
    if pattern == "two_alternate":
        return np.where(i % 2 == 0, 7, 200)
    if pattern == "change_mid_wave":                   # runs of 96: a whole wavefront of one digit, then a change at lane 32
        return (i // 96) % 256
    if pattern == "each_digit_equally":                # all 256, each exactly t / 256 times
        return rng.permutation(np.repeat(np.arange(256), t // 256))
    if pattern == "one_absent":
        d = rng.integers(0, 255, t)
        return np.where(d >= 77, d + 1, d)
    if pattern == "sorted_partial_last_wave":          # sorted digits, the last wavefront partial and of one digit: k_hist
        d = np.sort(rng.integers(0, 255, t + 1000 + 37))   # counts a wavefront of one digit with one lane, here with act not full
        d[-150:] = 255
        return d
    raise ValueError(pattern)


PATTERNS = ["all_lanes_differ", "two_alternate", "change_mid_wave", "each_digit_equally", "one_absent", "sorted_partial_last_wave"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("form", FORMS)
def test_digit_patterns(ctx, form, pattern):
    nw, t = NW[form], TILE[form]
    rng = np.random.default_rng([7, PATTERNS.index(pattern)])
    d = _digits(pattern, rng, t).astype(np.uint64)
    n = len(d)
    if pattern == "one_absent":
        assert 77 not in d and len(np.unique(d)) == 255
    if pattern == "each_digit_equally":
        assert (np.bincount(d.astype(np.int64), minlength=256) == t // 256).all()
    if pattern == "sorted_partial_last_wave":
        assert n % 64 and (np.diff(d.astype(np.int64)) >= 0).all() and (d[-(n % 64) - 64:] == 255).all()
    w = (d << U(8)) | (rows(n) << U(32)) | rng.integers(0, 256, n, dtype=np.uint64)
    words = [rows(n) for _ in range(nw - 1)] + [w]
    for tight in (0, 1):
        check(ctx, words, [(nw - 1, 8, 16)], tight, np.arange(n, dtype=np.uint32) if form == "w1pay" else None)


# ---------------------------------------------------------------- the histogram scan's shapes

@pytest.mark.parametrize("nblk", [16, 17])
def test_hist_scan_threshold(ctx, nblk):
    """256 * nblk histogram entries: 4096 (one workgroup scans them) and 4352 (tiles and their sums)"""
    n = 16 * 8192 + (nblk - 16)
    words, fields, pay = records("w1pay", np.random.default_rng([8, nblk]), n)
    for tight in (0, 1):
        chunk, got_nblk, _ = check(ctx, words, fields, tight, pay)
        assert chunk == 8192 and got_nblk == nblk


# ---------------------------------------------------------------- the sweeps over the prepared histogram

def test_sweeps_prepared_histogram_two_tile_chunks(ctx, monkeypatch):
    """merge (8-byte words, the prefetching kernel) and cluster (words + row ids) sort words whose first histogram the pack
    kernel k_pack1h counted, one workgroup per sort workgroup: with chunks of two tiles its inner loop and the sort's must
    still agree on the layout; IVX_NO_PACK_HIST=1 counts them with k_hist instead"""
    n = 2 * 8192 * 3 + 8192 + 5
    rng = np.random.default_rng(9)
    nk = 4
    k = rng.integers(0, nk, n).astype(np.uint32)
    s = rng.integers(-3_000_000, 3_000_000, n).astype(np.int64)
    at = np.arange(0, n - 1, 9)
    s[at] = s[at + 1]                                  # equal starts
    e = s + rng.integers(0, 400, n)
    form = wide.expected_form(k, s, e, nk)
    assert form["one_word"] and form["packed"], form    # merge sweeps the packed words, cluster sorts word + row id
    assert (np.lexsort((s, k)) != np.arange(n)).any()
    want_m = orc.merge(k, s, e)
    want_c = orc.cluster(k, s, e, n_keys=nk)
    with chunk_tiles(2):
        chunk = gpu_sort(ctx, [np.zeros(n, np.uint64)], [(0, 0, 0)], 1)[2]
        assert chunk == 2 * 8192 and n > chunk         # the geometry ivx_sort_geometry1 hands the pack kernel
        for knob in (None, "IVX_NO_PACK_HIST"):
            with monkeypatch.context() as m:
                if knob:
                    m.setenv(knob, "1")
                wide._same(ctx.merge(k, s, e, n_keys=nk), want_m, f"merge {knob}")
                wide._same_cluster(ctx.cluster(k, s, e, n_keys=nk), want_c, f"cluster {knob}")
