"""CPU-only: the two restatements of the depth coverage classes (tests/depth_classes_oracle.py) agree with each other on
seeded profiles, with the run-length coding and the value counts of the reference's pinned per-base rows
(tests/golden/pileup_per_base_golden.json) and with depth_regions_oracle.summarize_prefix; and the constants pyivx exports
are those of the kernel source and the header."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_classes_oracle as dco  # noqa: E402
import depth_oracle as orc  # noqa: E402
import depth_per_base_oracle as pbo  # noqa: E402
import depth_regions_oracle as dro  # noqa: E402
import pyivx  # noqa: E402

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
CUTS3 = (-1, 1, 3)
CUTS31 = tuple(range(-15, 16))
CUT_SETS = ((), (0,), CUTS3, (I32_MIN,), (I32_MAX,), (I32_MIN, 0, I32_MAX), CUTS31)


def same_rows(a, b):
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert x.dtype == y.dtype == np.uint32 and x.shape == y.shape and np.array_equal(x, y)


def same_hist(a, b):
    assert a.dtype == b.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b)


def test_restatements_agree_on_random_cases():
    rng = np.random.default_rng(9)
    seen = dict(negative=0, nosteps=0, unseen=0, empty_domain=0, pos0=0, merged_zero=0, split_zero=0, clamped_lo=0, clamped_hi=0)
    for it in range(300):
        clip = bool(it & 1)
        kw = orc.random_case(rng, clip=clip, max_pos=40)
        nk = kw["n_keys"]
        st = pbo.steps(nk, **orc.oracle_kw(kw))
        for skip in (False, True):
            pos_lo = 1 if skip else int(rng.integers(0, 3))
            key_hi = rng.integers(0, 60, nk).astype(np.uint32) if clip else np.full(nk, 70, np.uint32)
            seen_only = bool(it & 2)
            dom = (pos_lo, key_hi, skip, seen_only)
            for cuts in CUT_SETS:
                a = dco.quantize_loop(st, cuts, None, *dom)
                same_rows(a, dco.quantize_steps(st, cuts, None, *dom))
                # a full mask tiles every domain: the runs of a key add up to |D(k)|
                size = np.zeros(nk, np.int64)
                np.add.at(size, a[0], a[2].astype(np.int64) - a[1].astype(np.int64) + 1)
                assert np.array_equal(size, dco.domain_sizes(st, pos_lo, key_hi, seen_only))
            for mask in range(16):                          # every emit_mask of a 3-cut set
                same_rows(dco.quantize_loop(st, CUTS3, mask, *dom), dco.quantize_steps(st, CUTS3, mask, *dom))
            for v_lo, nb in ((0, 4), (-3, 7), (-40, 1), (I32_MIN, 2), (I32_MAX, 3), (-2, 64)):
                h = dco.hist_loop(st, v_lo, nb, *dom)
                same_hist(h, dco.hist_steps(st, v_lo, nb, *dom))
                assert np.array_equal(h.sum(axis=1), dco.domain_sizes(st, pos_lo, key_hi, seen_only))
            h = dco.hist_steps(st, -2, 5, *dom)
            seen["clamped_lo"] += int((st[2] < -2).any()); seen["clamped_hi"] += int((st[2] > 2).any())
            zero = dco.quantize_steps(st, (1,), None, *dom)
            for k in range(nk):
                p, v = dro.key_steps(st, k, skip)
                d = dco.domain(st, k, pos_lo, key_hi, seen_only)
                seen["unseen"] += int(seen_only and not st[3][k])
                seen["empty_domain"] += int(int(key_hi[k]) < pos_lo)
                if d is None:
                    continue
                seen["nosteps"] += int(len(p) == 0)
                seen["negative"] += int((v < 0).any())
                seen["pos0"] += int(skip and len(p) and p[0] == 0)
                if len(p) and d[0] < p[0] <= d[1]:
                    first = zero[2][zero[0] == k][0]
                    seen["merged_zero"] += int(first >= p[0]); seen["split_zero"] += int(first == p[0] - 1)
    assert all(x > 0 for x in seen.values()), seen


def test_hist_matches_summarize_prefix():
    """sum over the bins from t - v_lo on = the bases at or above t of the whole-domain region"""
    rng = np.random.default_rng(21)
    for it in range(60):
        kw = orc.random_case(rng, clip=bool(it & 1), max_pos=40)
        nk = kw["n_keys"]
        st = pbo.steps(nk, **orc.oracle_kw(kw))
        skip = bool(it & 2)
        pos_lo, key_hi = (1 if skip else 0), rng.integers(0, 1 << 20, nk).astype(np.uint32)
        v_lo, nb = -6, 14
        h = dco.hist_steps(st, v_lo, nb, pos_lo, key_hi, skip)
        thr = tuple(range(v_lo + 1, v_lo + nb))             # (bin 0 and the last bin are clamped: t from the second bin on)
        ln, _, ge = dro.summarize_prefix(st, np.arange(nk, dtype=np.uint32), np.zeros(nk, np.uint32), np.full(nk, 0xFFFFFFFF, np.uint32),
                                         thr, pos_lo, key_hi, skip)
        assert np.array_equal(h.sum(axis=1), ln)
        for j, t in enumerate(thr):
            assert np.array_equal(h[:, t - v_lo:].sum(axis=1), ge[j])


def rle(cls):
    cls = np.asarray(cls, np.int64)
    head = np.flatnonzero(np.concatenate([[True], np.diff(cls) != 0]))
    return head, np.concatenate([head[1:] - 1, [len(cls) - 1]]), cls[head]


def check_against_rows(st, L, zero_based, pos, cov):
    """quantize and hist over the reference's domain against the classes and the value counts of the per-base rows (pos
    int32, cov int16); only where the int32 values fit the rows' Int16"""
    assert len(pos) == L and int(pos[0]) == (0 if zero_based else 1)
    first = int(pos[0])
    key_hi = np.array([first + L - 1], np.uint32)
    dom = (first, key_hi, not zero_based)
    v = dro.values(st, 0, first, L, not zero_based)
    if v.min() < -32768 or v.max() > 32767:
        return False
    c = cov.astype(np.int64)
    assert np.array_equal(v, c)
    for cuts in ((), (1,), (0, 1, 4, 100, 200), (-2, 0, 3)):
        s, e, cl = rle(np.searchsorted(np.asarray(cuts, np.int64), c, side="right"))
        got = dco.quantize_steps(st, cuts, None, *dom)
        assert np.array_equal(got[0], np.zeros(len(s))) and np.array_equal(got[1], first + s) and np.array_equal(got[2], first + e)
        assert np.array_equal(got[3], cl)
        if L <= 300:
            same_rows(got, dco.quantize_loop(st, cuts, None, *dom))
    for v_lo, nb in ((0, 256), (-3, 8), (1, 2)):
        want = np.bincount(np.clip(c - v_lo, 0, nb - 1), minlength=nb).astype(np.int64)
        got = dco.hist_steps(st, v_lo, nb, *dom)
        assert got.shape == (1, nb) and np.array_equal(got[0], want)
        if L <= 300:
            same_hist(got, dco.hist_loop(st, v_lo, nb, *dom))
    return True


@pytest.mark.parametrize("zero_based", [True, False])
@pytest.mark.parametrize("case", pbo.golden()["emitter"], ids=lambda c: c["name"])
def test_emitter_tables(case, zero_based):
    depth = [0] * case["depth_len"]
    for i, d in case["depth"]:
        depth[i] = d
    pos, cov = pbo.emit_dense(depth, zero_based)
    if zero_based == case["zero_based"]:                    # the rows are the reference's pinned ones
        for row, c in case["expect"]["coverage"]:
            assert int(cov[row]) == c
    L = case["depth_len"] - 1
    segs = [(0, i, 0xFFFFFFFF, d) for i, d in case["depth"]]
    kw = dict(orc.pack_segments(segs), key_len=np.array([L], np.uint32))
    check_against_rows(pbo.steps(1, **kw), L, zero_based, pos, cov)


@pytest.mark.parametrize("zero_based", [True, False])
def test_ovl_bam(zero_based):
    g = pbo.golden()["ovl_bam"]
    case = next(c for c in orc.golden_cases() if c["name"] == g["reads_case"])
    names, kw = orc.case_columns(case)
    kw["key_len"] = np.array([g["length"]], np.uint32)
    if not zero_based:
        kw["rpos"] = kw["rpos"] + np.uint32(1)
    pos, cov = pbo.per_base_dense(zero_based, 1, **kw)[0]
    for row, c in g["zero_based" if zero_based else "one_based"]["coverage"]:
        assert int(cov[row]) == c
    assert check_against_rows(pbo.steps(1, **kw), g["length"], zero_based, pos, cov)


def test_constants_match_the_kernel_source_and_the_header():
    src = open(os.path.join(ROOT, "datafusion-bio-functions_amd", "csrc", "ivx_depth_classes.hip")).read()
    for name, want in (("DEPTH_HIST_LDS_BINS", pyivx.DEPTH_HIST_LDS_BINS), ("DEPTH_HIST_TILE_KEYS", pyivx.DEPTH_HIST_TILE_KEYS)):
        m = re.findall(r"\bconstexpr\s+u32\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert len(m) == 1 and int(m[0]) == want
    assert re.search(r"\bconstexpr\s+int\s+DEPTH_CLASS_TILE\s*=\s*ivxscan::TILE_\s*;", src)
    scan = open(os.path.join(ROOT, "datafusion-bio-functions_amd", "csrc", "ivx_scan.hpp")).read()
    t, i = (int(re.search(r"\bconstexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % n, scan).group(1)) for n in ("T_", "I_"))
    assert t * i == pyivx.DEPTH_CLASS_TILE
    hdr = open(os.path.join(ROOT, "include", "ivx.h")).read()
    assert int(re.search(r"#define\s+IVX_DEPTH_MAX_CUTS\s+(\d+)", hdr).group(1)) == pyivx.DEPTH_MAX_CUTS
    assert int(re.search(r"#define\s+IVX_DEPTH_MAX_BINS\s+(\d+)", hdr).group(1)) == pyivx.DEPTH_MAX_BINS
    assert "ivx_depth_profile_quantize" in pyivx.SYMBOLS and "ivx_depth_profile_hist" in pyivx.SYMBOLS
