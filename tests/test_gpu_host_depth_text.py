"""-m gpu: Session.set_string_cigars(True): depth, depth_per_base and depth_stream on pyarrow tables whose cigar column is
Utf8 / LargeUtf8 ("5M3D5M", parsed on the device) give what the same reads give as Binary; the reference's PileupExec tests
on text CIGARs (tests/golden/pileup_cigar_text_golden.json) give its asserted rows; the error texts, and the option off."""
import os
import struct
import sys

import numpy as np
import pyarrow as pa
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bio_ranges as br  # noqa: E402
import cigar_text_oracle as cto  # noqa: E402

pytestmark = pytest.mark.gpu

OLD_ERROR = "depth: string CIGAR columns are not supported, use the binary CIGAR column"
LENGTHS = {"chr1": 5000, "chr2": 3000, "MT": 900}
TEXT_TYPES = [pa.string(), pa.large_string()]


@pytest.fixture()
def sess():
    s = br.Session(0)
    s.set_string_cigars(True)
    yield s
    s.close()


def table(reads, cigar_type):
    """[(chrom, start, flags, mapq, cigar bytes)] -> a table with the reference's column names; Binary: the packed ops of
    the restatement's tokeniser"""
    if cigar_type == pa.binary():
        cig = [struct.pack("<%dI" % len(t), *[(ln << 4) | c for ln, c in t]) for t in (cto.tokenize(r[4]) for r in reads)]
    else:
        cig = [r[4].decode() for r in reads]
    return pa.table({"chrom": pa.array([r[0] for r in reads], pa.string()), "start": pa.array([r[1] for r in reads], pa.uint32()),
                     "flags": pa.array([r[2] for r in reads], pa.uint32()), "cigar": pa.array(cig, cigar_type),
                     "mapping_quality": pa.array([r[3] for r in reads], pa.uint32())})


def lengths_table(d):
    return pa.table({"name": pa.array(list(d), pa.string()), "length": pa.array(list(d.values()), pa.int64())})


def out_rows(t):
    return [list(r) for r in zip(*[t.column(c).to_pylist() for c in ("contig", "pos_start", "pos_end", "coverage")])]


def random_reads(rng, n):
    letters = "MIDNSHP=X"
    reads = []
    for _ in range(n):
        chrom = str(rng.choice(list(LENGTHS)))
        parts = []
        for _ in range(int(rng.integers(0, 6))):
            parts.append(("" if rng.random() < 0.05 else str(int(rng.integers(0, 120)))) + letters[int(rng.integers(0, 9))])
        s = "".join(parts)
        r = rng.random()
        if r < 0.05:
            s = "*"
        elif r < 0.1:
            s += "17"                   # digits without an op letter: dropped
        elif r < 0.15:
            s = "5B" + s                # a byte that only separates
        reads.append((chrom, int(rng.integers(0, LENGTHS[chrom] + 50)), int(rng.choice([0, 0, 0, 16, 4, 1024])),
                      int(rng.choice([0, 20, 60])), s.encode()))
    return reads


@pytest.mark.parametrize("cigar_type", TEXT_TYPES, ids=["utf8", "large_utf8"])
def test_depth_equals_the_binary_column(sess, cigar_type):
    reads = random_reads(np.random.default_rng(1), 600)
    for lengths in (None, lengths_table(LENGTHS)):
        want = sess.depth(table(reads, pa.binary()), lengths=lengths, min_mapq=10)
        got = sess.depth(table(reads, cigar_type), lengths=lengths, min_mapq=10)
        assert want.num_rows > 100 and got.equals(want)
    # sliced arrays, as for Binary: the offsets of the slice do not start at 0
    whole = table(reads, cigar_type)
    for lo, n in ((1, 40), (3, 1), (17, 300), (599, 1), (600, 0)):
        assert sess.depth(whole.slice(lo, n)).equals(sess.depth(table(reads[lo:lo + n], pa.binary())))
    # prior blocks are added in
    a = sess.depth(table(reads[:300], cigar_type))
    assert sess.depth(table(reads[300:], cigar_type), prior=a).equals(sess.depth(table(reads, pa.binary())))


@pytest.mark.parametrize("cigar_type", TEXT_TYPES, ids=["utf8", "large_utf8"])
def test_depth_per_base_equals_the_binary_column(sess, cigar_type):
    reads = random_reads(np.random.default_rng(2), 300)
    lengths = lengths_table(LENGTHS)
    want = list(sess.depth_per_base(table(reads, pa.binary()), lengths=lengths, zero_based=True))
    got = list(sess.depth_per_base(table(reads, cigar_type), lengths=lengths, zero_based=True))
    assert len(want) > 1 and len(got) == len(want) and all(g.equals(w) for g, w in zip(got, want))


@pytest.mark.parametrize("cigar_type", TEXT_TYPES, ids=["utf8", "large_utf8"])
def test_depth_stream_equals_the_binary_column(sess, cigar_type):
    reads = random_reads(np.random.default_rng(3), 400)
    want = sess.depth(table(reads, pa.binary()))
    with sess.depth_stream() as ds:
        for lo in range(0, 400, 90):
            ds.push(table(reads[lo:lo + 90], cigar_type if (lo // 90) % 2 == 0 else pa.binary()))      # the forms may alternate
        assert ds.finish().equals(want)
    lengths = lengths_table(LENGTHS)
    want_pb = list(sess.depth_per_base(table(reads, pa.binary()), lengths=lengths))
    with sess.depth_stream(lengths=lengths) as ds:
        for lo in range(0, 400, 150):
            ds.push(table(reads, cigar_type).slice(lo, 150))
        got_pb = list(ds.finish_per_base())
    assert len(got_pb) == len(want_pb) and all(g.equals(w) for g, w in zip(got_pb, want_pb))


EXEC_CASES = [c for c in cto.golden_cases() if c["name"].startswith("exec_")]


@pytest.mark.parametrize("case", EXEC_CASES, ids=[c["name"] for c in EXEC_CASES])
def test_pileup_exec_cases(sess, case):
    """physical_exec.rs's tests on a MemTable with a Utf8 cigar column: one partition is one pushed batch"""
    reads = [(r["contig"], r["pos"], r["flags"], r["mapq"], r["cigar"].encode()) for r in case["reads"]]
    exp = case["expect"]
    parts = case.get("partitions", [list(range(len(reads)))])
    with sess.depth_stream(filter_flag=case["filter_flag"], min_mapq=case["min_mapq"]) as ds:
        for part in parts:
            ds.push(table([reads[i] for i in part], pa.string()))
        got = out_rows(ds.finish())
    assert got == out_rows(sess.depth(table(reads, pa.string()), filter_flag=case["filter_flag"], min_mapq=case["min_mapq"]))
    if "blocks" in exp:
        assert got == exp["blocks"]
    if "coverages" in exp:
        assert len(got) == exp["n_rows"] and [r[3] for r in got] == exp["coverages"]
    if "contigs" in exp:
        assert set(exp["contigs"]) <= {r[0] for r in got}


def test_parse_errors_and_other_types(sess):
    reads = [("chr1", 0, 0, 60, b"10M"), ("chr1", 5, 4, 60, b"268435456M")]
    with pytest.raises(br.BioRangesError, match=r"2\^28.*\(read 1\)"):
        sess.depth(table(reads, pa.string()))
    for t in (pa.string_view(), pa.binary_view()):
        with pytest.raises(br.BioRangesError) as ei:
            sess.depth(pa.table({**{c: table(reads[:1], pa.string()).column(c) for c in ("chrom", "start", "flags", "mapping_quality")},
                                 "cigar": pa.array([b"10M" if t == pa.binary_view() else "10M"], t)}))
        fmt = "vu" if t == pa.string_view() else "vz"
        assert str(ei.value) == f"depth: unsupported data type {fmt} for column 'cigar'; expected Binary, Utf8 or LargeUtf8"
    assert out_rows(sess.depth(table(reads[:1], pa.string()))) == [["chr1", 0, 9, 1]]


def test_switching_the_option_off_restores_the_old_error(sess):
    reads = [("chr1", 0, 0, 60, b"10M")]
    assert out_rows(sess.depth(table(reads, pa.large_string()))) == [["chr1", 0, 9, 1]]
    sess.set_string_cigars(False)
    for t in TEXT_TYPES:
        with pytest.raises(br.BioRangesError) as ei:
            sess.depth(table(reads, t))
        assert str(ei.value) == OLD_ERROR
        with sess.depth_stream() as ds:
            with pytest.raises(br.BioRangesError) as ei:
                ds.push(table(reads, t))
            assert str(ei.value) == OLD_ERROR
        with pytest.raises(br.BioRangesError) as ei:
            next(sess.depth_per_base(table(reads, t), lengths=lengths_table(LENGTHS)))
        assert str(ei.value) == OLD_ERROR
    assert out_rows(sess.depth(table(reads, pa.binary()))) == [["chr1", 0, 9, 1]]
    sess.set_string_cigars(True)
    assert out_rows(sess.depth(table(reads, pa.string()))) == [["chr1", 0, 9, 1]]


def test_a_new_session_refuses_text_cigars():
    s = br.Session(0)
    try:
        with pytest.raises(br.BioRangesError) as ei:
            s.depth(table([("chr1", 0, 0, 60, b"10M")], pa.string()))
        assert str(ei.value) == OLD_ERROR
    finally:
        s.close()
