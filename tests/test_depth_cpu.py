"""CPU-only: the two restatements of depth() (tests/depth_oracle.py) reproduce the reference's pinned tables
(tests/golden/pileup_golden.json), agree with each other on seeded random inputs, and the built libraries export the
entry points."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_oracle as orc  # noqa: E402

PKG = os.path.join(ROOT, "datafusion-bio-functions_amd")


CASES = orc.golden_cases()
case_columns, rows_of = orc.case_columns, orc.rows_of


def test_golden_file_is_data_with_provenance():
    with open(os.path.join(GOLDEN, "pileup_golden.json")) as f:
        doc = json.load(f)
    assert "bio-function-pileup" in doc["provenance"]
    assert len(doc["cases"]) >= 25
    assert {"bam_ovl", "bam_overlapping_pairs"} <= {c["name"] for c in doc["cases"]}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatements_reproduce_golden(case):
    names, kw = case_columns(case)
    exp = case["expect"]
    ev = orc.events_loop(**kw)
    if "events" in exp:
        got = {names[k]: sorted(map(list, v)) for k, v in ev.items()}
        assert got == {k: sorted(v) for k, v in exp["events"].items()}
    if "dense" in exp:
        got = {}
        for k, v in ev.items():
            slots = {}
            for p, d in v:
                slots[p] = slots.get(p, 0) + d
            got[names[k]] = {str(p): d for p, d in slots.items() if d}
        assert got == exp["dense"]
    loop, vec = orc.depth_loop(**kw), orc.depth_numpy(**kw)
    assert rows_of(names, loop) == rows_of(names, vec)
    if "blocks" in exp:
        assert rows_of(names, loop) == exp["blocks"]


def test_restatements_agree_on_random_cases():
    rng = np.random.default_rng(20240611)
    seen_codes, n_blocks, clipped, wrapped = set(), 0, 0, 0
    for _ in range(2000):
        kw = orc.oracle_kw(orc.random_case(rng))
        loop, vec = orc.depth_loop(**kw), orc.depth_numpy(**kw)
        for a, b in zip(loop, vec):
            assert a.dtype == b.dtype and np.array_equal(a, b), kw
        seen_codes |= set((kw["cigar_ops"] & 15).tolist())
        n_blocks += len(loop[0])
        clipped += kw["key_len"] is not None
        wrapped += int((np.abs(loop[3].astype(np.int64)) > 0x7FFFFFF0).any())
    assert seen_codes == set(range(16))
    assert n_blocks > 2000 and clipped > 300 and wrapped > 10


def test_restatement_pins():
    """hand-checked answers for the rules the golden tables do not reach"""
    M = 0xFFFFFFFF
    op = lambda n, c: (n << 4) | c
    # saturation: 20M at 2^32 - 10 ends at 2^32 - 1 (cigar.rs:245 saturating_add)
    kw = orc.pack_reads([(0, M - 9, 0, 60, [op(20, 0)])])
    for f in (orc.depth_loop, orc.depth_numpy):
        assert [x.tolist() for x in f(**kw)] == [[0], [M - 9], [M - 1], [1]]
    # abutting reads are one block; a 0M changes nothing
    kw = orc.pack_reads([(0, 0, 0, 60, [op(10, 0)]), (0, 10, 0, 60, [op(10, 0)]), (0, 5, 0, 60, [op(0, 0)])])
    for f in (orc.depth_loop, orc.depth_numpy):
        assert [x.tolist() for x in f(**kw)] == [[0], [0], [19], [1]]
    # clipping leaves the block open: it is lost (coverage.rs:47-56 emits a block only when the coverage changes again)
    kw = orc.pack_reads([(0, 5, 0, 60, [op(10, 0)])])
    for f in (orc.depth_loop, orc.depth_numpy):
        assert len(f(key_len=np.array([7], np.uint32), **kw)[0]) == 0
        assert [x.tolist() for x in f(key_len=np.array([15], np.uint32), **kw)] == [[0], [5], [14], [1]]
    # two INT32_MAX weights wrap to -2
    kw = orc.pack_segments([(0, 0, 9, 0x7FFFFFFF), (0, 0, 9, 0x7FFFFFFF)])
    for f in (orc.depth_loop, orc.depth_numpy):
        assert [x.tolist() for x in f(**kw)] == [[0], [0], [9], [-2]]


def test_libraries_export_depth():
    sys.path.insert(0, PKG)
    import pyivx
    assert "ivx_depth" in pyivx.SYMBOLS
    assert hasattr(pyivx.lib(), "ivx_depth")
    assert hasattr(pyivx.Ctx, "depth")
    host = ctypes.CDLL(os.path.join(PKG, "lib", "libbio_ranges_hip.so"))
    assert hasattr(host, "brh_depth")
