"""CPU-only: the two restatements of the depth region order statistics (tests/depth_quantiles_oracle.py) agree with each
other on random inputs and give the min, max and median of the reference's pinned per-base tables
(tests/golden/pileup_per_base_golden.json); the constants pyivx exports are those of the kernel source."""
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
import depth_quantiles_oracle as dqo  # noqa: E402
import depth_regions_oracle as dro  # noqa: E402
import pyivx  # noqa: E402

QN, QD = (0, 1, 2, 3, 4, 1, 3), 4            # min, quartiles, max; repeats


def same(a, b):
    assert len(a) == len(b) == 4
    for x, y, dt in zip(a, b, (np.int64, np.int32, np.int32, np.int32)):
        assert x.dtype == y.dtype == dt and x.shape == y.shape and np.array_equal(x, y)


def test_rank_is_the_lower_quantile():
    assert [dqo.rank(L, 1, 2) for L in (1, 2, 3, 4, 5)] == [0, 0, 1, 1, 2]
    assert dqo.rank(1 << 32, 65536, 65536) == (1 << 32) - 1 and dqo.rank(1 << 32, 0, 7) == 0
    assert dqo.rank(10, 1, 4) == 2 and dqo.rank(10, 3, 4) == 6


def test_restatements_agree_on_random_cases():
    rng = np.random.default_rng(6)
    seen = dict(empty=0, before_first=0, open_end=0, cut=0, negative=0, pos0=0, nokey=0, even=0, spread=0)
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
            a = dqo.quantiles_loop(st, qkey, qs, qe, QN, QD, pos_lo, key_hi, skip)
            b = dqo.quantiles_steps(st, qkey, qs, qe, QN, QD, pos_lo, key_hi, skip)
            same(a, b)
            assert np.array_equal(a[3][0], a[1]) and np.array_equal(a[3][4], a[2]) and np.array_equal(a[3][1], a[3][5])
            if it % 7 == 0:
                same(dqo.quantiles_loop(st, None, qs, qe, (1,), 2, pos_lo, key_hi, skip), dqo.quantiles_steps(st, None, qs, qe, (1,), 2, pos_lo, key_hi, skip))
            for i in range(n):
                r = dro.clip(qkey, qs, qe, i, pos_lo, key_hi)
                seen["empty"] += int(r is None)
                if r is None:
                    assert a[0][i] == 0 and a[1][i] == 0 and a[2][i] == 0 and not a[3][:, i].any()
                    continue
                p, v = dro.key_steps(st, r[0], skip)
                seen["nokey"] += int(len(p) == 0)
                seen["cut"] += int(r[2] < int(qe[i]))
                seen["negative"] += int(a[1][i] < 0)
                seen["even"] += int(a[0][i] % 2 == 0)
                seen["spread"] += int(a[1][i] < a[3][2][i] < a[2][i])
                if len(p):
                    seen["before_first"] += int(r[1] < p[0])
                    seen["open_end"] += int(r[2] > p[-1] and v[-1] != 0)
                    seen["pos0"] += int(skip and p[0] == 0)
    assert all(x > 0 for x in seen.values()), seen


def test_steps_form_on_long_regions_and_wide_values():
    rng = np.random.default_rng(9)
    n_steps = 300
    pos = np.sort(rng.choice(5000, n_steps, replace=False)).astype(np.uint32) + 7
    cov = rng.integers(-(1 << 31), 1 << 31, n_steps).astype(np.int32)
    st = (np.zeros(n_steps, np.uint32), pos, cov, np.ones(1, np.uint8))
    qs = np.array([0, 7, int(pos[5]), int(pos[5]) + 1, 0], np.uint32)
    qe = np.array([6000, int(pos[-1]), int(pos[200]) - 1, int(pos[6]), 0xFFFFFFFF], np.uint32)
    a = dqo.quantiles_steps(st, None, qs, qe, (0, 1, 65536), 65536)
    same(tuple(x[..., :4] for x in a), dqo.quantiles_loop(st, None, qs[:4], qe[:4], (0, 1, 65536), 65536))
    assert a[0][4] == 1 << 32 and a[3][2][4] == a[2][4] and a[3][0][4] == a[1][4]
    assert dqo.segment_count(st, 0, 0, 6000) == n_steps + 1 and dqo.segment_count(st, 0, int(pos[0]), int(pos[1])) == 2


def regions_of(L, zero_based, rng):
    first = 0 if zero_based else 1
    allp = first + np.arange(L, dtype=np.int64)
    if L > 300:
        allp = np.unique(np.concatenate([allp[:100], allp[-100:], first + rng.integers(0, L, 100)]))
    a = first + rng.integers(0, L, 24)
    b = first + rng.integers(0, L, 24)
    s = np.concatenate([[first], allp, np.minimum(a, b)])
    e = np.concatenate([[first + L - 1], allp, np.maximum(a, b)])
    return s.astype(np.uint32), e.astype(np.uint32)


def check_against_rows(st, key, L, zero_based, pos, cov, rng):
    """both restatements over the reference's domain against np.sort of the per-base rows (pos int32, cov int16)"""
    assert len(pos) == L and int(pos[0]) == (0 if zero_based else 1)
    s, e = regions_of(L, zero_based, rng)
    key_hi = np.zeros(key + 1, np.uint32)
    key_hi[key] = L - 1 if zero_based else L
    qkey = np.full(len(s), key, np.uint32)
    args = (st, qkey, s, e, (1,), 2, 0 if zero_based else 1, key_hi, not zero_based)
    got = dqo.quantiles_steps(*args)
    if L <= 300:
        same(got, dqo.quantiles_loop(*args))
    c = cov.astype(np.int64)
    for i in range(len(s)):
        w = np.sort(c[int(s[i]) - int(pos[0]): int(e[i]) - int(pos[0]) + 1])
        assert got[0][i] == len(w) and got[1][i] == w[0] and got[2][i] == w[-1] and got[3][0][i] == w[(len(w) - 1) // 2]
    out = dqo.quantiles_steps(st, qkey[:1], np.array([L + 1], np.uint32), np.array([L + 50], np.uint32), (1,), 2, args[6], key_hi, args[8])
    assert out[0][0] == 0 and out[1][0] == 0 and out[2][0] == 0 and out[3][0][0] == 0


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


def test_constants_match_the_kernel_source():
    src = open(os.path.join(ROOT, "datafusion-bio-functions_amd", "csrc", "ivx_depth_rank.hip")).read()
    for name in ("DEPTH_RANK_TILE", "DEPTH_RANK_SEGS", "DEPTH_RANK_SELECT_GRID"):
        m = re.findall(r"\bconstexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src)
        assert len(m) == 1, name
        assert int(m[0]) == getattr(pyivx, name)
    assert pyivx.DEPTH_RANK_TILE == pyivx.DEPTH_REGION_TILE             # one tile size for the sums and the extremes
    hdr = open(os.path.join(ROOT, "include", "ivx.h")).read()
    assert int(re.search(r"#define\s+IVX_DEPTH_MAX_QUANTILES\s+(\d+)", hdr).group(1)) == pyivx.DEPTH_MAX_QUANTILES
    assert "ivx_depth_profile_quantiles" in pyivx.SYMBOLS and "ivx_depth_profile_window_quantiles" in pyivx.SYMBOLS
