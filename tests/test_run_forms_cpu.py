"""No GPU: every designed input of tests/run_forms.py is what its name claims -- the predicates over the oracle's run heads put
the key boundaries, the head-free tiles and wavefronts, the last row and the threshold rows where the case says they are --
and the serial walk of the reference rule equals the C oracle on all of them (merge rows, every cluster column, the counts).
Family H (4.2 M rows) is checked by its predicates only, with the heads taken from the C oracle."""
import numpy as np
import pytest

import run_forms as rf
from oracle import oracle as orc

SMALL = [n for n, c in rf.CASES.items() if c.family != "H"]
LAST_ROW = {1: (0, 0, 0, 0), 7: (6, 0, 0, 0), 8: (7, 0, 0, 0), 9: (0, 1, 0, 0), 511: (6, 63, 0, 0), 512: (7, 63, 0, 0), 513: (0, 0, 1, 0),
            1023: (6, 63, 1, 0), 1024: (7, 63, 1, 0), 1025: (0, 0, 2, 0), 4095: (6, 63, 7, 0), 4096: (7, 63, 7, 0), 4097: (0, 0, 0, 1),
            4608: (7, 63, 0, 1), 8191: (6, 63, 7, 1), 8192: (7, 63, 7, 1), 8193: (0, 0, 0, 2), 12296: (7, 0, 0, 3)}
LAST_ROW_SCAN = {255: (2, 63, 0, 0), 256: (3, 63, 0, 0), 257: (0, 0, 1, 0), 2047: (2, 63, 3, 1), 2048: (3, 63, 3, 1), 2049: (0, 0, 0, 2),
                 1024 * 1024 + 1: (0, 0, 0, 1024)}


def test_families_are_complete():
    fam = lambda f: [c for c in rf.CASES.values() if c.family == f]
    assert sorted({c.claims["n"] for c in fam("A") if c.geom == rf.PACKED}) == sorted(rf.A_SIZES)
    assert sorted({c.claims["n"] for c in fam("A") if c.geom == rf.SCAN}) == sorted(rf.A_SIZES_SCAN + [1024 * 1024 + 1])
    for n in rf.A_SIZES + rf.A_SIZES_SCAN:
        assert {f"A_n{n}_{r}" for r in ("each", "one", "mix")} <= set(rf.CASES)
    assert {c.claims["key_boundary"] for c in fam("B")} == {a + d for a in (8, 512, 4096) for d in (-1, 0, 1)}
    assert {(c.claims["opening_fast_group"], c.claims["prev_end"]) for c in fam("B") if "prev_end" in c.claims} == \
        {(1, "larger"), (1, "smaller"), (8, "larger"), (8, "smaller")}
    assert {c.claims["next_head_place"] for c in fam("C")} == {"mid", "thread", "wave", "tile"}
    assert {c.claims["max_end_place"][0] for c in fam("D")} == {"key_first", "thread_last", "wave_last", "tile_last"}
    assert {c.claims["largest"] for c in fam("E")} == {"first", "last", "middle"}
    assert {(c.claims["threshold"], c.claims["mixed"]) for c in fam("F")} == {(d, m) for d in (0, 1, 5) for m in (False, True)}
    assert {tuple(c.pairs) for c in fam("F") if c.claims["threshold"] == 5} == {((5, False), (5, True))}
    assert len(fam("G")) == 12 and len(fam("H")) == 2 and {c.claims["n_keys"] for c in fam("I")} == {2048, 2049}
    for c in rf.CASES.values():                              # (the 1 M-row case: two pairs, the Python walk takes seconds there)
        assert c.pairs == rf.PAIRS or c.family == "F" or c.name == "A_n1048577_five_runs", c.name


def _cur_end_before(ks, ss, es):
    """the largest end among the earlier rows of the key (the rows are well formed: that is cur_end), None at a key's first row"""
    out, run = [], None
    for i in range(len(ks)):
        if i == 0 or ks[i] != ks[i - 1]:
            run = None
        out.append(run)
        run = es[i] if run is None else max(run, es[i])
    return out


def check_claims(c, k, s, e, nk, heads, md, strict):
    """heads: run heads by sorted position under (md, strict), from the oracle"""
    tile, wave, thr = c.geom
    n = len(s)
    ks = rf.sorted_keys(k, s)
    cl = c.claims
    hpos = np.flatnonzero(heads)
    assert (e >= s).all() and int(k.max()) < nk
    if "n" in cl:
        assert n == cl["n"]
    if "last_row" in cl:
        table = LAST_ROW if c.geom == rf.PACKED else LAST_ROW_SCAN
        assert rf.last_row_place(n, c.geom) == cl["last_row"] == table[n], c.name
    if "heads" in cl:
        assert hpos.tolist() == cl["heads"]
    if cl.get("all_heads"):
        assert heads.all()
    if "n_heads" in cl:
        assert len(hpos) == cl["n_heads"]
    if "headless_tiles" in cl:
        assert set(cl["headless_tiles"]) <= set(rf.headless(heads, tile)), c.name
    if "min_headless_tiles" in cl:
        assert len(rf.headless(heads, tile)) >= cl["min_headless_tiles"]
    if "min_headless_groups" in cl:
        assert len(rf.headless(heads, wave)) >= cl["min_headless_groups"]
    if "key_boundary" in cl:
        b = cl["key_boundary"]
        assert ks[b - 1] != ks[b] and heads[b]
    if "n_keys" in cl:
        assert nk == cl["n_keys"] and nk > int(k.max()) + 1
    if "empty_keys" in cl:
        assert sorted(set(range(nk)) - set(k.tolist())) == cl["empty_keys"]
    if "opening_fast_group" in cl:
        g = cl["opening_fast_group"]
        assert g > 0 and g in rf.opening_fast_groups(ks), c.name
    if "heads_behind_boundary" in cl:                            # in the eight rows of the thread that opens the key
        b = cl["key_boundary"]
        assert b % rf.FI == 0 and int(heads[b:b + rf.FI].sum()) == cl["heads_behind_boundary"], c.name
    if "prev_end" in cl:
        # the end offset (end - smallest end) the wavefront inherits from the key before against its own first row's
        b = cl["key_boundary"]
        o = np.lexsort((s, k))
        before, own = int(e[o][:b][ks[:b] == ks[b - 1]].max()), int(e[o][b])
        assert (before > own) == (cl["prev_end"] == "larger") and before != own
    for p in cl.get("heads_at", ()):
        assert heads[p], (c.name, p)
    if "no_heads_in" in cl:
        lo, hi = cl["no_heads_in"]
        assert lo < hi and not heads[lo:hi].any(), c.name
    if "next_head_place" in cl:
        p1 = cl["heads_at"][1]
        want = {"mid": p1 % thr == 3 and p1 % wave != 3, "thread": p1 % thr == 0 and p1 % wave != 0, "wave": p1 % wave == 0 and p1 % tile != 0,
                "tile": p1 % tile == 0}[cl["next_head_place"]]
        assert want and cl["heads_at"][0] // tile == 0 and (p1 - 1) // tile == 2, c.name
    if "max_end_place" in cl:
        where, P = cl["max_end_place"]
        want = {"key_first": ks[P - 1] != ks[P], "thread_last": P % thr == thr - 1 and P % wave != wave - 1,
                "wave_last": P % wave == wave - 1 and P % tile != tile - 1, "tile_last": P % tile == tile - 1}[where]
        o = np.lexsort((s, k))
        ss, es = s[o], e[o]
        assert want and int(es[P]) == int(es[:P + rf.D_FOLLOW + 1][ks[:P + rf.D_FOLLOW + 1] == ks[P]].max())
        for j in range(P + 2, P + rf.D_FOLLOW + 1):           # without P's end every row behind it starts beyond the ones before it
            assert int(ss[j]) - int(es[P + 1:j].max()) > 5
    if "equal_groups" in cl:
        o = np.lexsort((s, k))                                   # stable: equal starts stay in input order
        ss, es = s[o], e[o]
        for p, cnt in cl["equal_groups"]:
            assert len(set(ss[p:p + cnt].tolist())) == 1 and ss[p - 1] < ss[p] < ss[p + cnt] and len(set(es[p:p + cnt].tolist())) == cnt
            at = int(np.argmax(es[p:p + cnt]))
            assert at == {"first": 0, "last": cnt - 1, "middle": cnt // 2}[cl["largest"]], (c.name, p)
            assert not heads[p + 1:p + cnt + 1].any() and int(ss[p + cnt]) > int(np.sort(es[p:p + cnt])[-2]) + 5
        assert any(p // thr != (p + cnt - 1) // thr and p // wave == (p + cnt - 1) // wave for p, cnt in cl["equal_groups"])
        assert any(p // wave != (p + cnt - 1) // wave and p // tile == (p + cnt - 1) // tile for p, cnt in cl["equal_groups"])
        assert any(p // tile != (p + cnt - 1) // tile for p, cnt in cl["equal_groups"])
        assert min(cnt for _, cnt in cl["equal_groups"]) == 2 and max(cnt for _, cnt in cl["equal_groups"]) == 40
    if "threshold" in cl:
        d = cl["threshold"]
        assert md == d
        o = np.lexsort((s, k))
        ss, es = s[o].tolist(), e[o].tolist()
        ce = _cur_end_before(ks.tolist(), ss, es)
        sp = cl["spots"]
        assert all(p % rf.WG == 0 for p in sp["lane0_row0"]) and all(p % rf.WG == rf.WG - 1 for p in sp["lane63_row7"])
        assert all(p % rf.WG not in (0, rf.WG - 1) and 0 < p % rf.FI < rf.FI - 1 for p in sp["mid"])
        fast = rf.fast_groups(ks)
        for ps in sp.values():
            for j, p in enumerate(ps):
                assert ss[p] - ce[p] == d - 1 + j, (c.name, p)
                assert bool(heads[p]) == (j == 2 or (j == 1 and strict)), (c.name, p, md, strict)
                assert (p // rf.WG in fast) == (not cl["mixed"]), (c.name, p)
        assert bool((e == s).any()) == bool(cl.get("has_empty"))
    if "forms" in cl:
        for setting, want in cl["forms"].items():
            f = rf.host_form(k, s, e, nk, md, strict, knobs=() if setting == "default" else (setting,), stats=c.stats())
            assert {w: f[w] for w in want} == want, (c.name, setting, f)
    if "ntile" in cl:
        assert rf.host_form(k, s, e, nk, md, strict, stats=c.stats())["ntile"] == cl["ntile"] > 1024
    if "lin" in cl:
        assert rf.host_form(k, s, e, nk, md, strict, stats=c.stats())["lin"] == cl["lin"]
    if "rows_per_key" in cl:
        cnt = np.bincount(k, minlength=nk)
        lo, hi = cl["rows_per_key"]
        assert set(cnt[cnt > 0].tolist()) == set(range(lo, hi + 1))
        assert 0.18 < (cnt == 0).mean() < 0.22 and cnt[0] == 0 and cnt[-1] == 0
        a, b = cl["empty_run"]
        assert not cnt[a:b].any()
    if cl.get("no_fast_groups"):
        assert rf.fast_groups(ks) == []
    # every case but the bit-width ones reaches the packed sweep with narrow runs under default settings
    if c.family not in "G":
        f = rf.host_form(k, s, e, nk, md, strict, stats=c.stats())
        fallback = bool(cl.get("has_empty")) and strict and md == 0
        assert (f["packed"], f["narrow_runs"]) == ((0, 0) if fallback else (1, 1)), (c.name, f)


@pytest.mark.parametrize("name", SMALL)
def test_case_claims_and_serial_walk(name):
    c = rf.CASES[name]
    k, s, e, nk = c.rows()
    for md, strict in c.pairs:
        want_m = orc.merge(k, s, e, min_dist=md, strict=strict)
        want_c = orc.cluster(k, s, e, min_dist=md, strict=strict, n_keys=nk)
        check_claims(c, k, s, e, nk, rf.head_mask(want_c["cluster"]), md, strict)
        got_m, got_c = rf.serial_sweep(k, s, e, md, strict, n_keys=nk)
        for i, (g, w) in enumerate(zip(got_m, want_m)):
            assert g.dtype == w.dtype and np.array_equal(g, w), (name, md, strict, "merge column", i)
        for col in ("key", "start", "end", "row", "cluster", "cluster_start", "cluster_end", "key_clusters"):
            assert np.array_equal(got_c[col].astype(np.int64), want_c[col].astype(np.int64)), (name, md, strict, col)
        assert got_c["n_clusters"] == want_c["n_clusters"] == len(want_m[0])


@pytest.mark.parametrize("name", [n for n, c in rf.CASES.items() if c.family == "H"])
def test_two_level_case_claims(name):
    """(under strict min_dist = 0, the pair that merges least: a head-free stretch there is head-free under the other three)"""
    c = rf.CASES[name]
    k, s, e, nk = c.rows()
    assert (0, True) in c.pairs
    heads = rf.head_mask(orc.cluster(k, s, e, min_dist=0, strict=True, n_keys=nk)["cluster"])
    check_claims(c, k, s, e, nk, heads, 0, True)


def test_serial_walk_saturates_and_orders_equal_starts():
    """the walk's own corners: cur_end + min_dist saturates at INT64_MAX, strict never merges at it, ends of equal starts
    are taken in ascending order"""
    big = rf.I64_MAX
    k = np.zeros(5, np.uint32)
    s = np.array([0, 100, big - 10, big, 5], np.int64)
    e = np.array([50, 200, big, big, 5], np.int64)
    for md in (0, 7, big):
        for strict in (False, True):
            m, cl = rf.serial_sweep(k, s, e, md, strict, n_keys=1)
            for g, w in zip(m, orc.merge(k, s, e, min_dist=md, strict=strict)):
                assert np.array_equal(g, w), (md, strict)
            w = orc.cluster(k, s, e, min_dist=md, strict=strict, n_keys=1)
            assert all(np.array_equal(cl[col].astype(np.int64), w[col].astype(np.int64)) for col in ("row", "cluster", "cluster_start", "cluster_end"))
