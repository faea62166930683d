"""-m gpu: subtract at the edges of its count pass's LDS window, of its workgroups and of its fill pass.

k_frag_count<SubOp> (csrc/ivx_sweep.hip) stages for every workgroup of ST sorted left rows the stretch of the right side its rows'
searches touch -- heads [h0, h1), rights [r0, r1), sized from the two brackets brk[b], brk[b+1] plus SUB_MARGIN -- when it
fits SUB_HW heads and SUB_RW rights; a row whose searches leave the stretch raises `esc` and is planned again from global
memory.  Every window case here reads what the pass did (ivx_debug_subtract_paths, between the sizing and the fill call)
and asserts the edge it names: hn, rn, lds, the escaped rows.  A case whose readout does not show its edge fails.

Construction: rights on a lattice, right j = [100j+10, 100j+60) in one key, so every right is a gap head and hj[h] = h;
nested rights inside a head's run where a case needs several rights per head.  A left row that starts at 100q+5 has q
heads at or below its start.  Lefts are given sorted (key, start, end) where a case reasons about workgroups, so a row's
sorted position is its index; every case runs once more with its lefts shuffled (output only), with strict False and True,
and the well-formed window cases once more with 2^40 added to every coordinate.  All four output columns are compared
bit-exactly with the CPU oracle; where the lattice makes the fragment count obvious it is asserted too.

k_frag_fill has no capacity guard of its own: a fill with total > cap is refused on the host before the launch; the
capacity cases check that refusal, the canaries behind the rows and the call that follows."""
import bisect
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

pytestmark = pytest.mark.gpu

# csrc/ivx_sweep.hip: ST (rows of a workgroup), SUB_HW / SUB_RW (heads / rights the LDS stretch holds), SUB_MARGIN
ST, SUB_HW, SUB_RW, SUB_MARGIN = 256, 256, 640, 48
# words of a workgroup in the readout (frag_dbg_words<SubOp>)
W_B0, W_B1, W_H0, W_HN, W_R0, W_RN, W_LDS, W_ESC = range(8)
KEY = 1                     # the key of the lattice and of the lefts; keys 0 and 2 hold what a mode adds
MODES = ["wf", "env", "inv"]  # two-search plan; five-point plan by IVX_SUB_GENERAL; five-point plan by an inverted right in another key
OFF = 1 << 40


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


# ------------------------------------------------------------------ rows

def cols(key, s, e):
    s = np.asarray(s, np.int64); e = np.asarray(e, np.int64)
    k = np.full(len(s), key, np.uint32) if np.isscalar(key) else np.asarray(key, np.uint32)
    return k, s, e


def cat(*sides):
    return tuple(np.concatenate([x[i] for x in sides]) for i in range(3))


def lattice(n, key=KEY, first=0):
    j = np.arange(first, first + n, dtype=np.int64)
    return cols(key, 100 * j + 10, 100 * j + 60)


def nested(h, m, key=KEY):
    """m rights inside the run of lattice head h (none of them a head)"""
    t = np.arange(m, dtype=np.int64)
    s = 100 * h + 20 + t % 30
    return cols(key, s, s + 5)


def sort_rows(side):
    o = np.lexsort((side[2], side[1], side[0]))
    return tuple(x[o] for x in side)


def is_sorted(side):
    o = np.lexsort((side[2], side[1], side[0]))
    return all((x[o] == x).all() for x in side)


def shifted(side, off):
    return side[0], side[1] + off, side[2] + off


def with_mode(right, mode, inv_side):
    """-> (right side, environment) of a mode; "inv": wf == 0 arises from one right with end < start in the key below / above"""
    if mode == "inv":
        right = cat(right, cols(0 if inv_side == "lo" else 2, [50], [20]))
    return right, ({"IVX_SUB_GENERAL": "1"} if mode == "env" else {})


@contextlib.contextmanager
def environ(env):
    os.environ.update(env)
    try:
        yield
    finally:
        for v in env:
            os.environ.pop(v, None)


# ------------------------------------------------------------------ the count pass, restated

def heads_of(right):
    """the right side sorted, and its gap heads (key, start, index of the right) as k_gap_flags / k_gap_compact make them"""
    rk, rs, re = sort_rows(right)
    hk, hrs, hj = [], [], []
    mx = 0
    for j in range(len(rk)):
        first = j == 0 or rk[j] != rk[j - 1]
        if first or rs[j] > mx:
            hk.append(int(rk[j])); hrs.append(int(rs[j])); hj.append(j)
        mx = int(re[j]) if first else max(mx, int(re[j]))
    return (rk, rs, re), hk, hrs, hj


def model(left, right):
    """words 0..6 of every workgroup for SORTED lefts, from the window rule of SubOp (csrc/ivx_sweep.hip)"""
    lk, ls, _ = left
    nl = len(lk)
    (rk, _, _), hk, hrs, hj = heads_of(right)
    nh, nr = len(hk), len(rk)
    keys = list(zip(hk, hrs))
    rank = lambda i: bisect.bisect_right(keys, (int(lk[i]), int(ls[i])))
    nwg = (nl + 1 + ST - 1) // ST
    brk = [rank(b * ST) if b * ST < nl else nh for b in range(nwg)] + [rank(nl - 1)]
    out = np.zeros((nwg, 8), np.uint32)
    for b in range(nwg):
        if b * ST >= nl:
            continue
        s0, s1 = brk[b], brk[b + 1]
        h0 = s0 - SUB_MARGIN - 1 if s0 > SUB_MARGIN + 1 else 0
        h1 = s1 + SUB_MARGIN if nh - s1 > SUB_MARGIN else nh
        r0 = hj[h0] if h0 < nh else nr
        r1 = hj[h1] if h1 < nh else nr
        r1 = r1 + SUB_MARGIN if nr - r1 > SUB_MARGIN else nr
        hn, rn = h1 - h0, max(r1 - r0, 0)
        out[b, :7] = [s0, s1, h0, hn, min(r0, r1), rn, int(hn <= SUB_HW and rn <= SUB_RW)]
    return out


def head_counts(left, right, strict):
    """per left row: heads of its key that start at or below its end (strict: below): the row's h_hi, as an index into all heads"""
    _, hk, hrs, _ = heads_of(right)
    keys = list(zip(hk, hrs))
    f = bisect.bisect_left if strict else bisect.bisect_right
    return np.array([f(keys, (int(k), int(e))) for k, e in zip(left[0], left[2])])


# ------------------------------------------------------------------ calls

def read_paths(ctx):
    """(words[nwg, 8], esc[nl]) of the sizing call that just ran; also the hook's own failure modes"""
    L = pyivx.lib()
    nwg, nrows = C.c_uint64(0), C.c_uint64(0)
    st = L.ivx_debug_subtract_paths(ctx.h, None, C.c_uint64(0), None, C.c_uint64(0), C.byref(nwg), C.byref(nrows))
    assert st == pyivx.ERR_CAPACITY, st
    wg = np.full((nwg.value, 8), 0xDEAD, np.uint32); esc = np.full(nrows.value, 7, np.uint8)
    for _ in range(2):                                      # the second run finds the plan still there
        st = L.ivx_debug_subtract_paths(ctx.h, wg.ctypes.data_as(C.c_void_p), C.c_uint64(len(wg)), esc.ctypes.data_as(C.c_void_p),
                                        C.c_uint64(len(esc)), C.byref(nwg), C.byref(nrows))
        assert st == pyivx.OK, L.ivx_last_error(ctx.h)
    assert nwg.value == len(wg) and nrows.value == len(esc)
    assert ((esc == 0) | (esc == 1)).all()
    return wg, esc


def subtract_read(ctx, left, right, n_keys, strict):
    seen = []
    got = ctx.subtract(*left, *right, n_keys=n_keys, strict=strict, between=lambda: seen.append(read_paths(ctx)))
    assert len(seen) == 1
    return got, seen[0][0], seen[0][1]


def same(got, want, what=None):
    for g, w in zip(got, want):
        assert len(g) == len(w), (what, len(g), len(w))
        assert g.dtype == w.dtype and (g == w).all(), what


def run_case(ctx, left, right, mode="wf", inv_side="hi", expect=None, total=None, n_keys=3, offsets=None):
    """left sorted.  Output against the oracle and the readout against model(); expect(wg, esc, strict, left, right) asserts
    the case's own edge; total: the closed-form fragment count."""
    assert is_sorted(left)
    right, env = with_mode(right, mode, inv_side)
    for off in (offsets if offsets is not None else ((0, OFF) if mode == "wf" else (0,))):
        L, R = shifted(left, off), shifted(right, off)
        want_wg = model(L, R)
        for strict in (False, True):
            want = orc.subtract(*L, *R, strict=strict)
            if total is not None:
                assert len(want[0]) == total, (len(want[0]), total)
            with environ(env):
                got, wg, esc = subtract_read(ctx, L, R, n_keys, strict)
            same(got, want, (mode, off, strict))
            assert wg.shape == want_wg.shape and (wg[:, :7] == want_wg[:, :7]).all(), (mode, off, strict, wg, want_wg)
            per_wg = np.add.reduceat(esc.astype(np.int64), np.arange(0, len(esc), ST))
            assert (wg[:len(per_wg), W_ESC] == per_wg).all() and (wg[len(per_wg):, W_ESC] == 0).all()
            assert (esc[np.repeat(wg[:, W_LDS] == 0, ST)[:len(esc)]] == 0).all()      # no LDS plan, no escape
            if expect is not None:
                expect(wg, esc, strict, L, R)
    run_shuffled(ctx, left, right, env, n_keys)


def run_shuffled(ctx, left, right, env, n_keys, seed=5):
    p = np.random.default_rng(seed).permutation(len(left[0]))
    L = tuple(x[p] for x in left)
    for strict in (False, True):
        with environ(env):
            got = ctx.subtract(*L, *right, n_keys=n_keys, strict=strict)
        same(got, orc.subtract(*L, *right, strict=strict), ("shuffled", strict))


# ------------------------------------------------------------------ window cases

def three_workgroups(q0, q1):
    """700 sorted lefts, every one of them ONE fragment.  Workgroup 1 (rows 256..511) starts at a row with q0 lattice heads
    at or below its start and is followed by a row with q1; its rows spread over q0..q1 and are, in turn: clear of every
    right, ending inside a right, ending at a right's end, ending at a right's start."""
    i = np.arange(ST, dtype=np.int64)
    s0 = np.full(ST, 100 * q0 + 1); e0 = s0 + 1 + i // 100
    q = q0 + (i * (q1 - q0)) // (ST - 1)
    s1 = 100 * q + 5
    e1 = np.choose(i % 4, [s1 + 3, 100 * q + 40, 100 * q + 60, 100 * q + 10])
    j = np.arange(700 - 2 * ST, dtype=np.int64)
    s2 = np.full(len(j), 100 * q1 + 6); e2 = s2 + 1 + j // 100
    mid = sort_rows(cols(KEY, s1, e1))
    return cat(cols(KEY, s0, e0), mid, cols(KEY, s2, e2))


def base_of(mode, inv_side):
    return 1 if mode == "inv" and inv_side == "lo" else 0           # heads in front of the lattice's


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("apart,hn,lds", [(159, 256, 1), (160, 257, 0)])
def test_head_window_full_and_one_over(ctx, mode, apart, hn, lds):
    """a middle workgroup whose brackets are 159 / 160 heads apart: hn = apart + 97"""
    left, right = three_workgroups(100, 100 + apart), lattice(400)

    def expect(wg, esc, strict, L, R):
        assert wg[1, W_B1] - wg[1, W_B0] == apart
        assert wg[1, W_HN] == hn and wg[1, W_LDS] == lds and wg[1, W_RN] <= SUB_RW
        assert wg[0, W_LDS] == 1 and wg[2, W_LDS] == 1
    run_case(ctx, left, right, mode, "hi", expect, total=700)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("b0,h0", [(0, 0), (49, 0), (50, 1)])
def test_head_window_front_clamp(ctx, mode, b0, h0):
    left, right = three_workgroups(b0, b0 + 20), lattice(400)

    def expect(wg, esc, strict, L, R):
        assert wg[1, W_B0] == b0 and wg[1, W_H0] == h0 and wg[1, W_LDS] == 1
        assert wg[1, W_R0] == h0                               # hj[h] = h
    run_case(ctx, left, right, mode, "hi", expect, total=700)   # the other key's head sorts behind: brk stays as named


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("back,reaches_end", [(0, True), (48, True), (49, False)])
def test_head_window_back_clamp(ctx, mode, back, reaches_end):
    nh = 400
    left, right = three_workgroups(nh - back - 20, nh - back), lattice(nh)

    def expect(wg, esc, strict, L, R):
        nh_all = nh + (mode == "inv")
        assert nh_all - wg[1, W_B1] == back and wg[1, W_LDS] == 1
        h1 = wg[1, W_H0] + wg[1, W_HN]
        assert (h1 == nh_all) == reaches_end and (reaches_end or h1 == nh_all - 1)
        if reaches_end:
            assert wg[1, W_R0] + wg[1, W_RN] == nh_all         # h1 == nh forces r1 = nr
    run_case(ctx, left, right, mode, "lo", expect, total=700)   # the other key's head sorts in front: nh - brk stays as named


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("extra,rn,lds", [(475, 640, 1), (476, 641, 0)])
def test_rights_window_full_and_one_over(ctx, mode, extra, rn, lds):
    """brackets 100 and 120: heads [51, 168), 117 of them; `extra` rights nested in head 110: rn = 117 + extra + 48"""
    left, right = three_workgroups(100, 120), cat(lattice(400), nested(110, extra))

    def expect(wg, esc, strict, L, R):
        assert wg[1, W_RN] == rn and wg[1, W_LDS] == lds and wg[1, W_HN] == 117 <= SUB_HW
    run_case(ctx, left, right, mode, "hi", expect, total=700)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("back,reaches_end", [(48, True), (49, False)])
def test_rights_window_back_clamp(ctx, mode, back, reaches_end):
    """nr - hj[h1] at 48 / 49 with h1 = brk[b+1] + 48 < nh: r1 = nr or nr - 1"""
    nh = 400
    q1 = nh - back - SUB_MARGIN
    left, right = three_workgroups(q1 - 20, q1), lattice(nh)

    def expect(wg, esc, strict, L, R):
        nr = nh + (mode == "inv")
        h1 = wg[1, W_H0] + wg[1, W_HN]
        assert h1 == wg[1, W_B1] + SUB_MARGIN and nr - h1 == back      # hj[h1] = h1
        assert wg[1, W_R0] + wg[1, W_RN] == (nr if reaches_end else nr - 1) and wg[1, W_LDS] == 1
    run_case(ctx, left, right, mode, "lo", expect, total=700)


@pytest.mark.parametrize("mode", MODES)
def test_rights_window_to_the_end_behind_the_last_head(ctx, mode):
    """h1 == nh: r1 = nr, whatever follows the last head (60 rights nested in it)"""
    nh = 300
    left, right = three_workgroups(nh - 30, nh - 10), cat(lattice(nh), nested(nh - 1, 60))

    def expect(wg, esc, strict, L, R):
        nr = nh + 60 + (mode == "inv")
        assert wg[1, W_H0] + wg[1, W_HN] == nh + (mode == "inv")
        assert wg[1, W_R0] + wg[1, W_RN] == nr and wg[1, W_LDS] == 1
    run_case(ctx, left, right, mode, "lo", expect, total=700)


# ------------------------------------------------------------------ escaping rows

Q0, Q1, NH = 100, 120, 400


def escape_rows():
    """one workgroup, brackets Q0 and Q1.  kind 0: rows that cross no head; kind d > 0: rows whose last head is d heads
    beyond the upper bracket (47: the last staged head, 48: the first one not staged); kind -1: rows across everything"""
    rows = [(100 * q + 5, 100 * q + 8, 0) for q in range(Q0, Q1 + 1)]
    for d in (1, 47, 48, 49):
        rows += [(100 * q + 5, 100 * (Q1 + d - 1) + 40, d) for q in (Q0, Q0 + 10, Q1)]
    rows += [(100 * q + 5, 100 * NH + 1000, -1) for q in (Q0, Q1)]
    rows.sort()
    s, e, kind = (np.array(x, np.int64) for x in zip(*rows))
    return cols(KEY, s, e), kind


@pytest.mark.parametrize("mode,inv_side", [("wf", "hi"), ("env", "hi"), ("inv", "hi"), ("inv", "lo")])
def test_rows_that_leave_the_staged_stretch(ctx, mode, inv_side):
    left, kind = escape_rows()
    base = base_of(mode, inv_side)

    def expect(wg, esc, strict, L, R):
        assert len(wg) == 1 and wg[0, W_LDS] == 1
        assert wg[0, W_B0] == Q0 + base and wg[0, W_B1] == Q1 + base
        h1 = int(wg[0, W_H0] + wg[0, W_HN])
        assert h1 == Q1 + base + SUB_MARGIN < NH
        hhi = head_counts(L, R, strict)
        assert (hhi[kind == 0] <= Q1 + base).all() and (esc[kind == 0] == 0).all()
        assert (hhi[kind == 47] == h1 - 1).all() and (hhi[kind == 48] == h1).all() and (hhi[kind == -1] >= NH).all()
        assert (esc[hhi >= h1] == 1).all() and (hhi >= h1).sum() == 8
        assert 0 < wg[0, W_ESC] < ST and wg[0, W_ESC] == esc.sum()
    run_case(ctx, left, lattice(NH), mode, inv_side, expect)


def _inverted_at(R, j):
    (rk, rs, re), _, _, _ = heads_of(R)
    return re[j] < rs[j]


def test_general_plan_early_right_with_a_huge_end(ctx):
    """right [10515, 20070) swallows the rights 106..200 (no heads any more), one inverted right nested in head 103 makes
    wf == 0: rows that start under the long right find their cursor far below their own start"""
    right = cat(lattice(NH), cols(KEY, [100 * 105 + 15, 100 * 103 + 30], [100 * 200 + 70, 100 * 103 + 12]))
    rows = []
    for q in range(Q0, Q1 + 1):
        rows += [(100 * q + 5, 100 * q + 8), (100 * q + 5, 100 * q + 40), (100 * q + 5, 100 * (q + 3) + 40), (100 * q + 5, 100 * 205 + 40)]
    rows.sort()
    left = cols(KEY, *zip(*rows))

    def expect(wg, esc, strict, L, R):
        _, hk, hrs, hj = heads_of(R)
        assert len(hk) == NH - 95 and wg[0, W_LDS] == 1 and wg[0, W_RN] > wg[0, W_HN] + SUB_MARGIN
    run_case(ctx, left, right, "wf", expect=expect, offsets=(0, OFF))      # ("wf": nothing added; the right side itself has the inverted row)


def test_general_plan_inverted_rights_at_both_ends_of_the_stretch(ctx):
    """inverted rights (heads: they start in a gap) exactly at the first and at the last staged right, and one right behind
    the start of the rows at 11005: the head above them has a running max below their start, so their cursor search runs
    to the end of the right side and leaves the stretch at its first probe"""
    inv = cols(KEY, [100 * 52 + 5, 100 * 215 + 5, 100 * 110 + 7], [100 * 52 - 15, 100 * 215 - 15, 100 * 110 - 13])
    right = cat(lattice(NH), inv)
    left, kind = escape_rows()

    def expect(wg, esc, strict, L, R):
        r0, rn = int(wg[0, W_R0]), int(wg[0, W_RN])
        assert wg[0, W_LDS] == 1 and _inverted_at(R, r0) and _inverted_at(R, r0 + rn - 1)
        odd = L[1] - (L[1][0] - 100 * Q0 - 5) == 100 * 110 + 5
        assert odd.sum() == 5 and (esc[odd] == 1).all() and (esc[(kind == 0) & ~odd] == 0).all() and 0 < wg[0, W_ESC] < ST
    run_case(ctx, left, right, "wf", expect=expect, offsets=(0, OFF))


# ------------------------------------------------------------------ rows and workgroups

def spread_lefts(nl, nh, key=KEY, seed=1):
    rng = np.random.default_rng(seed)
    s = np.sort(rng.integers(0, 100 * nh + 200, nl)).astype(np.int64)
    e = s + rng.integers(0, 260, nl)
    e[::9] = s[::9]                                           # empty lefts
    return sort_rows(cols(key, s, e))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nl", [1, 255, 256, 257, 512, 513])
def test_left_row_counts_around_a_workgroup(ctx, mode, nl):
    nh = 60
    left = spread_lefts(nl, nh)

    def expect(wg, esc, strict, L, R):
        assert len(wg) == nl // ST + 1
        if nl % ST == 0:                                       # the extra workgroup owns cnt[nl] alone
            assert (wg[-1] == 0).all() and wg[-1, W_LDS] == 0
            assert wg[-2, W_B1] == nh + (mode == "inv") and wg[-2, W_LDS] == 1
        assert (wg[: (nl + ST - 1) // ST, W_LDS] == 1).all()
    run_case(ctx, left, lattice(nh), mode, "hi", expect)


@pytest.mark.parametrize("nr", [0, 1])
def test_no_right_and_one_right(ctx, nr):
    left = spread_lefts(300, 3)
    right = lattice(nr)

    def expect(wg, esc, strict, L, R):
        assert (wg[:2, W_LDS] == 1).all() and (wg[:2, W_HN] == nr).all() and (wg[:2, W_RN] == nr).all() and esc.sum() == 0
    run_case(ctx, left, right, "wf", expect=expect, total=None if nr else int((left[2] > left[1]).sum()), offsets=(0,))


def test_one_head_many_rights(ctx):
    """nh == 1: every right sits in the first one's run"""
    right = cat(cols(KEY, [10], [5000]), nested(1, 300))

    def expect(wg, esc, strict, L, R):
        assert (wg[:2, W_HN] == 1).all() and (wg[:2, W_RN] == 301).all() and (wg[:2, W_LDS] == 1).all()
    run_case(ctx, spread_lefts(300, 60), right, "wf", expect=expect)


@pytest.mark.parametrize("mode", MODES)
def test_lefts_in_keys_without_rights(ctx, mode):
    left = cat(spread_lefts(200, 20, key=0, seed=2), spread_lefts(200, 20, key=2, seed=3))
    right = cat(lattice(40), cols(KEY, [33], [2])) if mode == "inv" else lattice(40)
    whole = int((left[2] > left[1]).sum())                    # every non-empty left comes back as it is

    def expect(wg, esc, strict, L, R):
        assert (wg[:2, W_LDS] == 1).all() and esc.sum() == 0
    with environ({"IVX_SUB_GENERAL": "1"} if mode == "env" else {}):
        run_case(ctx, left, right, "wf", expect=expect, total=whole, offsets=(0,))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("where", ["below", "beyond"])
def test_lefts_all_on_one_side_of_the_heads(ctx, mode, where):
    nl = 600
    i = np.arange(nl, dtype=np.int64)
    if where == "below":                                      # the first head starts at 5210
        right, s = lattice(300, first=52), 5000 + i // 3
    else:                                                     # the last right ends at 34960
        right, s = lattice(350), 35000 + i // 3
    left = cols(KEY, s, s + 1 + i % 3)

    def expect(wg, esc, strict, L, R):
        want = base_of(mode, "lo") + (0 if where == "below" else 350)
        assert (wg[:3, W_B0] == want).all() and (wg[:3, W_B1] == want).all() and (wg[:3, W_LDS] == 1).all() and esc.sum() == 0
    run_case(ctx, left, right, mode, "lo", expect, total=nl)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cut", [1, 128, 255])
def test_key_changes_inside_a_workgroup(ctx, mode, cut):
    """sorted positions cut-1 -> cut hold the last row of key 0 and the first of key 1; both keys have rights"""
    a = spread_lefts(cut, 30, key=0, seed=4)
    b = spread_lefts(300 - cut, 30, key=1, seed=5)
    left = cat(a, b)
    right = cat(lattice(30, key=0), lattice(30, key=1), nested(7, 3, key=0))
    if mode == "inv":
        right = cat(right, cols(2, [50], [20]))

    def expect(wg, esc, strict, L, R):
        assert wg[0, W_B0] <= 30 and wg[0, W_B1] >= 30 and (wg[:2, W_LDS] == 1).all()
    with environ({"IVX_SUB_GENERAL": "1"} if mode == "env" else {}):
        run_case(ctx, left, right, "wf", expect=expect, offsets=(0,))


@pytest.mark.parametrize("mode", MODES)
def test_keys_with_rights_and_no_lefts_in_between(ctx, mode):
    left = cat(*[spread_lefts(150, 40, key=k, seed=6 + k) for k in (0, 2, 4)])
    right = cat(*[lattice(40, key=k) for k in range(5)])
    if mode == "inv":
        right = cat(right, cols(3, [155], [120]))
    with environ({"IVX_SUB_GENERAL": "1"} if mode == "env" else {}):
        run_case(ctx, left, right, "wf", n_keys=5, offsets=(0,))


# ------------------------------------------------------------------ fill pass

def test_workgroup_that_emits_nothing_between_two_that_do(ctx):
    i = np.arange(ST, dtype=np.int64)
    a = cols(KEY, 100 * (i // 8) + 61 + i % 8, 100 * (i // 8) + 70 + i % 8)          # in the gaps: whole
    b = cols(KEY, 100 * (40 + i // 8) + 10 + i % 8, 100 * (40 + i // 8) + 28 + i % 32)  # inside rights: covered
    c = cols(KEY, 100 * (80 + i // 8) + 61 + i % 8, 100 * (80 + i // 8) + 70 + i % 8)
    left = cat(a, sort_rows(b), c)

    def expect(wg, esc, strict, L, R):
        assert len(wg) == 4 and (wg[:3, W_LDS] == 1).all()
    run_case(ctx, left, lattice(130), expect=expect, total=2 * ST)
    run_case(ctx, left, lattice(130), "env", total=2 * ST)


@pytest.mark.parametrize("frags", [255, 256, 257, 512, 513])
@pytest.mark.parametrize("tail", [False, True])
def test_one_row_with_many_fragments(ctx, frags, tail):
    """k_frag_fill's o += ST loop: a row's fragments spread over one, two and three trips; alone and between other rows"""
    right = lattice(600)
    long_row = (5, 100 * (frags - 2) + 80) if tail else (5, 100 * (frags - 1) + 30)    # frags-1 heads and a tail / frags heads
    alone = cols(KEY, [long_row[0]], [long_row[1]])
    for mode in ("wf", "env"):
        run_case(ctx, alone, right, mode, total=frags, offsets=(0,))
    others = sort_rows(cols(KEY, [0, 1, 5, 5, 7, 100 * 599 + 70], [3, 8, 9, long_row[1] + 100, 40, 100 * 599 + 90]))
    left = sort_rows(cat(alone, others))
    run_case(ctx, left, right, "wf", total=frags + 1 + 1 + 1 + (frags + 1) + 1 + 1)


def test_rows_with_heads_tail_both_neither_and_empty(ctx):
    rows = [(100 * 3 + 5, 100 * 3 + 40),          # a head fragment only
            (100 * 3 + 5, 100 * 3 + 60),          # ... ending at the right's end: tail_from == end, no tail
            (100 * 4 + 30, 100 * 4 + 90),         # tail only
            (100 * 5 + 5, 100 * 6 + 80),          # two heads and a tail
            (100 * 7 + 20, 100 * 7 + 50),         # covered: neither
            (100 * 7 + 10, 100 * 7 + 60),         # exactly a right: neither
            (100 * 8 + 5, 100 * 8 + 5),           # empty, in a gap
            (100 * 8 + 30, 100 * 8 + 30),         # empty, inside a right
            (100 * 9 + 60, 100 * 9 + 110),        # from a right's end to the next one's start
            (100 * 9 + 10, 100 * 10 + 10)]        # from a right's start to the next one's start
    rows.sort()
    left = cols(KEY, *zip(*rows))
    for mode in MODES:
        run_case(ctx, left, lattice(20), mode, total=1 + 1 + 1 + 3 + 0 + 0 + 0 + 0 + 1 + 1)


CANARY = 0x5A5A5A5A


def raw_subtract(ctx, left, right, strict, cap, room, sizing_first):
    """ivx_subtract into canary-filled host buffers of `room` rows with capacity `cap` -> (status, n_out, buffers)"""
    L = pyivx.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = (ctx.h, C.c_int(pyivx.MEM_HOST), p(left[0]), p(left[1]), p(left[2]), C.c_uint64(len(left[0])),
            p(right[0]), p(right[1]), p(right[2]), C.c_uint64(len(right[0])), C.c_uint32(3), C.c_int(int(strict)))
    m = C.c_uint64(0)
    if sizing_first:
        assert L.ivx_subtract(*args, None, None, None, None, C.c_uint64(0), C.byref(m)) == pyivx.OK
    bufs = [np.full(room, CANARY, dt) for dt in (np.uint32, np.int64, np.int64, np.uint32)]
    st = L.ivx_subtract(*args, *[p(b) for b in bufs], C.c_uint64(cap), C.byref(m))
    return st, m.value, bufs


@pytest.mark.parametrize("sizing_first", [False, True])
def test_capacity_at_and_around_the_total(ctx, sizing_first):
    left = tuple(np.ascontiguousarray(x) for x in spread_lefts(700, 60))
    right = tuple(np.ascontiguousarray(x) for x in lattice(60))
    for strict in (False, True):
        want = orc.subtract(*left, *right, strict=strict)
        total = len(want[0])
        assert total > 2 * ST
        for cap in (total, total + 1):
            st, m, bufs = raw_subtract(ctx, left, right, strict, cap, total + 64, sizing_first)
            assert st == pyivx.OK and m == total
            for b, w in zip(bufs, want):
                assert (b[:total] == w).all() and (b[total:] == CANARY).all()
        st, m, bufs = raw_subtract(ctx, left, right, strict, total - 1, total + 64, sizing_first)
        assert st == pyivx.ERR_CAPACITY and m == total
        for b in bufs:
            assert (b[total - 1:] == CANARY).all()
        st, m, bufs = raw_subtract(ctx, left, right, strict, total, total + 64, False)      # (after a sizing call: still its plan)
        assert st == pyivx.OK and m == total
        for b, w in zip(bufs, want):
            assert (b[:total] == w).all() and (b[total:] == CANARY).all()


def test_hook_without_a_plan(ctx):
    """no sizing call before it, and after the fill call consumed the plan: IVX_ERR_INVALID"""
    L = pyivx.lib()
    left, right = spread_lefts(300, 20), lattice(20)
    n = C.c_uint64(0)
    call = lambda: L.ivx_debug_subtract_paths(ctx.h, None, C.c_uint64(0), None, C.c_uint64(0), C.byref(n), C.byref(n))
    ctx.subtract(*left, *right, n_keys=3, cap=2000)            # one call: leaves no plan
    assert call() == pyivx.ERR_INVALID
    subtract_read(ctx, left, right, 3, False)
    assert call() == pyivx.ERR_INVALID
