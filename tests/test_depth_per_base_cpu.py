"""CPU-only: the two restatements of per-base depth() (tests/depth_per_base_oracle.py) agree with each other on random
inputs and with the reference's pinned tables (tests/golden/pileup_per_base_golden.json)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_oracle as orc  # noqa: E402
import depth_per_base_oracle as pbo  # noqa: E402


def same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        for x, y in zip(a[k], b[k]):
            assert x.dtype == y.dtype and np.array_equal(x, y)


def test_restatements_agree_on_random_cases():
    rng = np.random.default_rng(1)
    quirks = dict(cancel=0, open_end=0, pos0=0, wide=0)
    for _ in range(600):
        kw = orc.random_case(rng, clip=True, max_pos=40)
        nk = kw["n_keys"]
        okw = orc.oracle_kw(kw)
        st = pbo.steps(nk, **okw)
        for zb in (True, False):
            d = pbo.per_base_dense(zb, nk, **okw)
            same(d, pbo.per_base_steps(zb, nk, **okw))
            for k in d:
                m = st[0] == k
                quirks["cancel"] += int(not m.any())
                quirks["open_end"] += int(m.any() and st[2][m][-1] != 0)
                quirks["pos0"] += int(not zb and m.any() and st[1][m][0] == 0)
                quirks["wide"] += int(m.any() and np.abs(st[2][m].astype(np.int64)).max() > 32767)
    # the generator reaches every quirk the per-base form has over the blocks
    assert all(v > 0 for v in quirks.values()), quirks


@pytest.mark.parametrize("case", pbo.golden()["emitter"], ids=lambda c: c["name"])
def test_emitter_tables(case):
    depth = [0] * case["depth_len"]
    for i, d in case["depth"]:
        depth[i] = d
    pos, cov = pbo.emit_dense(depth, case["zero_based"])
    exp = case["expect"]
    n, bs = len(pos), case["batch_size"]
    assert [min(bs, n - i) for i in range(0, n, bs)] == exp["batch_rows"]
    assert [int(pos[0]), int(pos[-1])] == exp["positions"] and np.array_equal(np.diff(pos), np.ones(n - 1, np.int32))
    for row, c in exp["coverage"]:
        assert int(cov[row]) == c
    # the same table as weighted one-base segments through the steps form
    L = case["depth_len"] - 1
    segs = [(0, i, 0xFFFFFFFF, d) for i, d in case["depth"]]          # (i, +d) and a closing event that saturates and is clipped
    kw = dict(orc.pack_segments(segs), key_len=np.array([L], np.uint32))
    got = pbo.per_base_steps(case["zero_based"], 1, **kw)[0]
    assert np.array_equal(got[0], pos) and np.array_equal(got[1], cov)


@pytest.mark.parametrize("zero_based", [True, False])
def test_ovl_bam_pins(zero_based):
    g = pbo.golden()["ovl_bam"]
    case = next(c for c in orc.golden_cases() if c["name"] == g["reads_case"])
    names, kw = orc.case_columns(case)
    assert names == [g["contig"]]
    kw["key_len"] = np.array([g["length"]], np.uint32)
    if not zero_based:
        kw["rpos"] = kw["rpos"] + np.uint32(1)
    exp = g["zero_based" if zero_based else "one_based"]
    for f in (pbo.per_base_dense, pbo.per_base_steps):
        pos, cov = f(zero_based, 1, **kw)[0]
        assert len(pos) == exp["rows"] and int(pos[0]) == exp["first_pos"] and int(pos[-1]) == exp["last_pos"]
        for row, c in exp["coverage"]:
            assert int(cov[row]) == c
    assert pbo.REFERENCE_ERROR == g["missing_lengths_error"]
