"""CPU-only: the restatements of the text-CIGAR tokeniser (tests/cigar_text_oracle.py) reproduce the reference's pinned
tables on text CIGARs (tests/golden/pileup_cigar_text_golden.json), the packed ops they give feed the depth() restatements
to the same events and blocks as the direct restatement of apply_cigar_to_event_list, the capped scan operator of
csrc/ivx_cigar.hip equals the byte loop under random association orders, and the built libraries export the entry points."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import cigar_text_oracle as cto  # noqa: E402
import depth_oracle as orc  # noqa: E402

PKG = os.path.join(ROOT, "datafusion-bio-functions_amd")
CASES = cto.golden_cases()


def test_golden_file_is_data_with_provenance():
    with open(os.path.join(GOLDEN, "pileup_cigar_text_golden.json")) as f:
        doc = json.load(f)
    assert "bio-function-pileup" in doc["provenance"]
    names = [c["name"] for c in doc["cases"]]
    assert len([n for n in names if n.startswith("txt_") and "dense" not in n]) == 9
    assert len([n for n in names if n.startswith("txt_dense_")]) == 7
    assert {"exec_basic_coverage", "exec_filtering", "exec_empty_input", "exec_multi_partition"} <= set(names)
    assert all("cigar.rs" in c["source"] or "physical_exec.rs" in c["source"] for c in doc["cases"])
    assert "bio-function-pileup" in open(os.path.join(GOLDEN, "pileup_cigar_text_golden.md")).read()     # the provenance note


def direct_events(cols, cigars, kw):
    """events.rs:111-165 with apply_cigar_to_event_list, after the filter and the dense mode's bounds -> {key: [(pos, delta)]}"""
    ev = {}
    for i, s in enumerate(cigars):
        k = int(cols["rkey"][i])
        if k == orc.NULL_IDX or s == b"*":
            continue
        if cols.get("rflags") is not None and (int(cols["rflags"][i]) & kw["filter_flag"]) != 0:
            continue
        if cols.get("rmapq") is not None and int(cols["rmapq"][i]) < kw["min_mapq"]:
            continue
        for pos, d in cto.events_direct(int(cols["rpos"][i]), s):
            if kw["key_len"] is not None and pos > int(kw["key_len"][k]):
                continue
            ev.setdefault(k, []).append((pos, d))
    return ev


def packed_kw(cols, cigars, kw):
    off, ops = cto.parse_reads(cigars)
    return dict(cols, cigar_offsets=off, cigar_ops=ops, **kw)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatements_reproduce_golden(case):
    names, cols, cigars, kw = cto.case_columns(case)
    exp = case["expect"]
    pk = packed_kw(cols, cigars, kw)
    ev = orc.events_loop(**pk)
    assert ev == direct_events(cols, cigars, kw)
    if "events" in exp:
        assert {names[k]: list(map(list, v)) for k, v in ev.items()} == exp["events"]      # in the reference's order
    if "dense" in exp:
        got = {}
        for k, v in ev.items():
            slots = {}
            for p, d in v:
                slots[p] = slots.get(p, 0) + d
            got[names[k]] = {str(p): d for p, d in slots.items() if d}
        assert got == exp["dense"]
    rows = orc.rows_of(names, orc.depth_loop(**pk))
    assert rows == orc.rows_of(names, orc.depth_numpy(**pk))
    if "blocks" in exp:
        assert rows == exp["blocks"]
    if "coverages" in exp:
        assert len(rows) == exp["n_rows"] and [r[3] for r in rows] == exp["coverages"]
    if "contigs" in exp:
        assert set(exp["contigs"]) <= {r[0] for r in rows}
    if "partitions" in case:
        # coverage is additive: the blocks of every partition, fed back as weighted segments, give the same rows
        segs = []
        for part in case["partitions"]:
            _, c2, g2, _ = cto.case_columns(case, part)
            k, s, e, c = orc.depth_loop(**packed_kw(c2, g2, kw))
            segs += list(zip(k.tolist(), s.tolist(), e.tolist(), c.tolist()))
        merged = orc.depth_loop(key_len=kw["key_len"], **orc.pack_segments(segs))
        assert orc.rows_of(names, merged) == rows


def random_bytes(rng, n):
    """bytes weighted towards digits and op letters, every other value included"""
    kind = rng.random(n)
    out = np.where(kind < 0.5, rng.integers(48, 58, n),
                   np.where(kind < 0.85, np.frombuffer(cto.LETTERS, np.uint8)[rng.integers(0, 9, n)], rng.integers(0, 256, n)))
    return out.astype(np.uint8).tobytes()


SPECIAL = [b"0" * 30 + b"7M", b"4294967295M", b"4294967296M", b"99999999999M", b"268435455M", b"268435456X", b"0000000000000000000004294967295=",
           b"10M5", b"3M", b"*", b"", b"12", b"M", b"=", b"5B3M", b"1 2M", b"\xc3\xa95M", b"00M", b"4294967296", b"42949672960D"]


def random_reads(rng):
    n = int(rng.integers(1, 6))
    reads = []
    for _ in range(n):
        r = rng.random()
        if r < 0.25:
            reads.append(SPECIAL[int(rng.integers(0, len(SPECIAL)))])
        elif r < 0.35:
            reads.append(b"")
        else:
            reads.append(random_bytes(rng, int(rng.integers(1, 14))))
    return reads


def test_tokenize_pins():
    """hand-checked answers for the rules of include/ivx.h ivx_cigar_parse"""
    t = cto.tokenize
    assert t(b"5M3D5M") == [(5, 0), (3, 2), (5, 0)]
    assert t(b"1M2I3D4N5S6H7P8=9X") == [(i + 1, i) for i in range(9)]
    assert t(b"M") == [(0, 0)] and t(b"007M") == [(7, 0)] and t(b"0" * 30 + b"7M") == [(7, 0)]
    assert t(b"4294967295M") == [(4294967295, 0)] and t(b"4294967296M") == [(0, 0)] and t(b"99999999999M") == [(0, 0)]
    assert t(b"*") == [] and t(b"") == [] and t(b"12") == [] and t(b"10M5") == [(10, 0)]
    assert t(b"5B3M") == [(3, 0)] and t(b"5+3M") == [(3, 0)] and t(b"5 M") == [(0, 0)] and t(b"5\xc3\xa93M") == [(3, 0)]
    assert t(b"5m") == []                                        # lower case is no op letter
    off, ops = cto.parse_reads([b"10M5", b"3M", b"", b"*", b"2S4="])
    assert off.tolist() == [0, 4, 8, 8, 8, 16] and ops.tolist() == [160, 48, (2 << 4) | 4, (4 << 4) | 7]
    assert cto.parse_reads([b"268435455M"])[1].tolist() == [(268435455 << 4)]
    with pytest.raises(cto.PackError) as ei:
        cto.parse_reads([b"1M", b"268435456M", b"4294967295M"])
    assert ei.value.read == 1
    assert cto.parse_reads([b"4294967296M"])[1].tolist() == [0]


def test_packed_ops_give_the_direct_events():
    """the tokeniser's packed ops through events_loop / depth_loop == apply_cigar_to_event_list on the text, reads near
    2^32 (saturation) and clipping included"""
    rng = np.random.default_rng(20250219)
    n_ev = 0
    for _ in range(1500):
        cigars = [s for s in random_reads(rng)]
        try:
            off, ops = cto.parse_reads(cigars)
        except cto.PackError:
            continue
        n = len(cigars)
        nk = int(rng.integers(1, 4))
        cols = dict(rkey=rng.integers(0, nk, n).astype(np.uint32),
                    rpos=np.where(rng.random(n) < 0.1, 0xFFFFFFFF - rng.integers(0, 12, n), rng.integers(0, 60, n)).astype(np.uint32),
                    rflags=rng.choice([0, 0, 4, 16, 1024], n).astype(np.uint32), rmapq=rng.choice([0, 30, 60], n).astype(np.uint32))
        kw = dict(filter_flag=1796, min_mapq=int(rng.choice([0, 30])),
                  key_len=rng.integers(0, 70, nk).astype(np.uint32) if rng.random() < 0.4 else None)
        pk = dict(cols, cigar_offsets=off, cigar_ops=ops, **kw)
        ev = orc.events_loop(**pk)
        assert ev == direct_events(cols, cigars, kw), cigars
        want = []
        for k in sorted(ev):
            want += [(k, s, e, c) for s, e, c in orc.blocks_of_events(ev[k])]
        got = orc.depth_loop(**pk)
        assert list(zip(*[x.tolist() for x in got])) == want
        n_ev += sum(len(v) for v in ev.values())
    assert n_ev > 2000


@pytest.mark.parametrize("op", [cto.combine, cto.combine_u64], ids=["stated", "u64"])
def test_scan_operator_equals_the_byte_loop(op):
    """3 000 random multi-read inputs, every exclusive prefix folded under a random association order"""
    rng = np.random.default_rng(77)
    n_ops = capped = 0
    for _ in range(3000):
        reads = random_reads(rng)
        want = [cto.tokenize(s) for s in reads]
        assert cto.scan_tokens(reads, rng, op) == want, reads
        n_ops += sum(map(len, want))
        capped += any(len(s) > 10 for s in reads)
    assert n_ops > 5000 and capped > 300


def test_scan_operator_is_associative_at_the_caps():
    rng = np.random.default_rng(5)
    vals = [0, 1, 9, 10, 429496729, 429496730, 4294967295, 1 << 32]
    pows = [1, 10, 10 ** 9, 1 << 32]
    states = [(bool(r), v, p, 0) for r in (0, 1) for v in vals for p in pows]
    for _ in range(20000):
        a, b, c = (states[int(i)] for i in rng.integers(0, len(states), 3))
        for op in (cto.combine, cto.combine_u64):
            assert op(op(a, b), c) == op(a, op(b, c))
        assert cto.combine(a, b) == cto.combine_u64(a, b)


def test_render_round_trip():
    """what the GPU tests feed the text calls: depth_oracle.random_case inputs rendered as text parse back to the same ops
    on the codes that have a letter; the codes 9..15, which depth() ignores, leave no op"""
    rng = np.random.default_rng(3)
    for _ in range(300):
        kw = orc.random_case(rng)
        cigars = cto.render_reads(kw["cigar_offsets"], kw["cigar_ops"], rng)
        off, ops = cto.parse_reads(cigars)
        keep = (kw["cigar_ops"] & 15) < 9
        assert np.array_equal(ops, kw["cigar_ops"][keep])
        pk = dict(orc.oracle_kw(kw), cigar_offsets=off, cigar_ops=ops)
        for a, b in zip(orc.depth_loop(**pk), orc.depth_loop(**orc.oracle_kw(kw))):
            assert np.array_equal(a, b)


def test_libraries_export_the_text_calls():
    sys.path.insert(0, PKG)
    import pyivx
    for s in ("ivx_cigar_parse", "ivx_depth_text", "ivx_depth_profile_build_text"):
        assert s in pyivx.SYMBOLS and hasattr(pyivx.lib(), s)
    assert hasattr(pyivx.Ctx, "cigar_parse")
    assert (pyivx.CIGAR_B, pyivx.CIGAR_TILE) == (16, 4096)
    src = open(os.path.join(PKG, "csrc", "ivx_cigar.hip")).read()
    assert "constexpr int CIGAR_B = 16;" in src and "CIGAR_TILE = ivxscan::T_ * CIGAR_B" in src
    host = ctypes.CDLL(os.path.join(PKG, "lib", "libbio_ranges_hip.so"))
    assert hasattr(host, "brh_session_set_string_cigars")
