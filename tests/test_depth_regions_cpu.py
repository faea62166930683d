"""CPU-only: the two restatements of the depth region summaries (tests/depth_regions_oracle.py) agree with each other on
random inputs and with the reference's pinned per-base tables (tests/golden/pileup_per_base_golden.json), and
pyivx.DEPTH_REGION_TILE is the tile constant of the kernel source."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_oracle as orc  # noqa: E402
import depth_per_base_oracle as pbo  # noqa: E402
import depth_regions_oracle as dro  # noqa: E402
import pyivx  # noqa: E402

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
THR = (I32_MIN, -2, 0, 1, 2, 3, 40000, I32_MAX)


def same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype == np.int64 and x.shape == y.shape and np.array_equal(x, y)


def test_restatements_agree_on_random_cases():
    rng = np.random.default_rng(5)
    seen = dict(empty=0, before_first=0, open_end=0, cut=0, negative=0, pos0=0, nokey=0)
    for it in range(400):
        clip = bool(it & 1)
        kw = orc.random_case(rng, clip=clip, max_pos=40)
        nk = kw["n_keys"]
        st = pbo.steps(nk, **orc.oracle_kw(kw))
        n = 12
        qkey = rng.integers(0, nk, n).astype(np.uint32)
        qkey[rng.random(n) < 0.1] = dro.NULL_IDX
        qs = rng.integers(0, 50, n).astype(np.uint32)
        qe = (qs.astype(np.int64) + rng.integers(-2, 30, n)).clip(0).astype(np.uint32)
        for skip in (False, True):
            pos_lo = 1 if skip else int(rng.integers(0, 3))
            key_hi = rng.integers(0, 60, nk).astype(np.uint32) if clip else None
            a = dro.summarize_loop(st, qkey, qs, qe, THR, pos_lo, key_hi, skip)
            b = dro.summarize_prefix(st, qkey, qs, qe, THR, pos_lo, key_hi, skip)
            same(a, b)
            if it % 7 == 0:
                same(dro.summarize_loop(st, None, qs, qe, THR[:2], pos_lo, key_hi, skip), dro.summarize_prefix(st, None, qs, qe, THR[:2], pos_lo, key_hi, skip))
            for i in range(n):
                r = dro.clip(qkey, qs, qe, i, pos_lo, key_hi)
                seen["empty"] += int(r is None)
                if r is None:
                    continue
                p, v = dro.key_steps(st, r[0], skip)
                seen["nokey"] += int(len(p) == 0)
                seen["cut"] += int(r[2] < int(qe[i]))
                seen["negative"] += int(a[1][i] < 0)
                if len(p):
                    seen["before_first"] += int(r[1] < p[0])
                    seen["open_end"] += int(r[2] > p[-1] and v[-1] != 0)
                    seen["pos0"] += int(skip and p[0] == 0)
    assert all(x > 0 for x in seen.values()), seen


def regions_of(L, zero_based, rng):
    """the whole contig, every single position, seeded spans -> (start, end), in the coordinates of the per-base rows"""
    first = 0 if zero_based else 1
    allp = first + np.arange(L, dtype=np.int64)
    if L > 300:                                             # (every position of a long contig: a seeded sample and both ends)
        allp = np.unique(np.concatenate([allp[:100], allp[-100:], first + rng.integers(0, L, 100)]))
    a = first + rng.integers(0, L, 24)
    b = first + rng.integers(0, L, 24)
    s = np.concatenate([[first], allp, np.minimum(a, b)])
    e = np.concatenate([[first + L - 1], allp, np.maximum(a, b)])
    return s.astype(np.uint32), e.astype(np.uint32)


def check_against_rows(st, key, L, zero_based, pos, cov, rng):
    """both restatements over the reference's domain against sums of the per-base rows (pos int32, cov int16)"""
    assert len(pos) == L and int(pos[0]) == (0 if zero_based else 1)
    s, e = regions_of(L, zero_based, rng)
    key_hi = np.zeros(key + 1, np.uint32)
    key_hi[key] = L - 1 if zero_based else L
    qkey = np.full(len(s), key, np.uint32)
    args = (st, qkey, s, e, (1, 2), 0 if zero_based else 1, key_hi, not zero_based)
    got = dro.summarize_prefix(*args)
    if L <= 300:
        same(got, dro.summarize_loop(*args))
    c = cov.astype(np.int64)
    for i in range(len(s)):
        w = c[int(s[i]) - int(pos[0]): int(e[i]) - int(pos[0]) + 1]
        assert got[0][i] == len(w) and got[1][i] == w.sum()
        assert got[2][0][i] == (w >= 1).sum() and got[2][1][i] == (w >= 2).sum()
    # beyond the domain nothing is counted
    out = dro.summarize_prefix(st, qkey[:1], np.array([L + 1], np.uint32), np.array([L + 50], np.uint32), (0,), args[5], key_hi, args[7])
    assert out[0][0] == 0 and out[1][0] == 0 and out[2][0][0] == 0


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
    st = pbo.steps(1, **kw)
    check_against_rows(st, 0, L, zero_based, pos, cov, np.random.default_rng(L))


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
    check_against_rows(pbo.steps(1, **kw), 0, g["length"], zero_based, pos, cov, np.random.default_rng(3))


def test_windows_as_regions():
    s, e = dro.windows_as_regions(10, 35, 10, 4)
    assert s.tolist()[:3] == [10, 20, 30] and e.tolist()[:3] == [19, 29, 35] and e[3] < s[3]


def test_tile_constant_matches_the_kernel_source():
    src = open(os.path.join(ROOT, "datafusion-bio-functions_amd", "csrc", "ivx_depth_regions.hip")).read()
    m = re.findall(r"\bconstexpr\s+int\s+DEPTH_REGION_TILE\s*=\s*(\d+)\s*;", src)
    assert len(m) == 1
    assert int(m[0]) == pyivx.DEPTH_REGION_TILE
    hdr = open(os.path.join(ROOT, "include", "ivx.h")).read()
    assert int(re.search(r"#define\s+IVX_DEPTH_MAX_THRESHOLDS\s+(\d+)", hdr).group(1)) == pyivx.DEPTH_MAX_THRESHOLDS
