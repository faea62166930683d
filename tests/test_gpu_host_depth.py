"""-m gpu: Session.depth (brh_depth) on pyarrow tables: the reference's pinned tables by contig name, the output schema,
contig order, NULL rows, sliced inputs, the length table, the prior round trip and the error texts."""
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
import depth_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

op = lambda n, c: (n << 4) | c
CASES = orc.golden_cases()
case_columns, rows_of = orc.case_columns, orc.rows_of


@pytest.fixture(scope="module")
def sess():
    s = br.Session(0)
    yield s
    s.close()


def reads_table(reads, chrom_type=pa.string(), cigar_type=pa.binary()):
    """[(chrom, start, flags, mapq, [ops])] -> a table with the reference's column names (schema.rs:7-11)"""
    cig = [struct.pack("<%dI" % len(r[4]), *r[4]) for r in reads]
    if cigar_type != pa.binary():
        cig = ["10M"] * len(reads)
    return pa.table({"chrom": pa.array([r[0] for r in reads], chrom_type), "start": pa.array([r[1] for r in reads], pa.uint32()),
                     "flags": pa.array([r[2] for r in reads], pa.uint32()), "cigar": pa.array(cig, cigar_type),
                     "mapping_quality": pa.array([r[3] for r in reads], pa.uint32())})


def blocks_table(rows):
    return pa.table({"contig": pa.array([r[0] for r in rows], pa.string()), "pos_start": pa.array([r[1] for r in rows], pa.int32()),
                     "pos_end": pa.array([r[2] for r in rows], pa.int32()), "coverage": pa.array([r[3] for r in rows], pa.int16())})


def lengths_table(d):
    return pa.table({"name": pa.array(list(d), pa.string()), "length": pa.array(list(d.values()), pa.int64())})


def out_rows(t):
    return [list(r) for r in zip(*[t.column(c).to_pylist() for c in ("contig", "pos_start", "pos_end", "coverage")])]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_by_contig_name(sess, case):
    reads = reads_table([(r["contig"], r["pos"], r["flags"], r["mapq"], r["ops"]) for r in case["reads"]])
    prior = blocks_table(case["segments"]) if case["segments"] else None
    lengths = lengths_table(case["lengths"]) if case["lengths"] is not None else None
    got = out_rows(sess.depth(reads, prior=prior, lengths=lengths, filter_flag=case["filter_flag"], min_mapq=case["min_mapq"]))
    names, kw = case_columns(case)
    assert got == rows_of(names, orc.depth_loop(**kw))
    if "blocks" in case["expect"]:
        assert got == case["expect"]["blocks"]


def test_output_schema(sess):
    t = sess.depth(reads_table([("chr1", 100, 0, 60, [op(10, 0)])]))
    assert t.schema.names == ["contig", "pos_start", "pos_end", "coverage"]
    assert [f.type for f in t.schema] == [pa.string(), pa.int32(), pa.int32(), pa.int16()]
    assert out_rows(t) == [["chr1", 100, 109, 1]]
    empty = sess.depth(reads_table([]))
    assert empty.num_rows == 0 and [f.type for f in empty.schema] == [pa.string(), pa.int32(), pa.int32(), pa.int16()]


@pytest.mark.parametrize("chrom_type", [pa.string(), pa.large_string(), pa.string_view()])
def test_contigs_in_byte_order(sess, chrom_type):
    reads = [("MT", 0, 0, 60, [op(5, 0)]), ("2", 10, 0, 60, [op(5, 0)]), ("10", 20, 0, 60, [op(5, 0)]), ("2", 12, 0, 60, [op(5, 0)])]
    got = out_rows(sess.depth(reads_table(reads, chrom_type)))
    assert got == [["10", 20, 24, 1], ["2", 10, 11, 1], ["2", 12, 14, 2], ["2", 15, 16, 1], ["MT", 0, 4, 1]]


def test_null_chrom_or_start_rows_are_skipped(sess):
    t = pa.table({"chrom": pa.array([None, "chr1", "chr1", "chr1"], pa.string()), "start": pa.array([0, None, 100, 103], pa.uint32()),
                  "flags": pa.array([0, 0, 0, None], pa.uint32()), "cigar": pa.array([struct.pack("<I", op(10, 0))] * 4, pa.binary()),
                  "mapping_quality": pa.array([60, 60, None, 60], pa.uint32())})
    # (a NULL flags / mapping_quality slot is read as its value, 0 here: events.rs:119-121)
    assert out_rows(sess.depth(t)) == [["chr1", 100, 102, 1], ["chr1", 103, 109, 2], ["chr1", 110, 112, 1]]


def test_sliced_reads_table(sess):
    rng = np.random.default_rng(3)
    reads = [(str(rng.choice(["a", "b"])), int(rng.integers(0, 300)), 0, 60, [op(int(rng.integers(1, 20)), int(rng.choice([0, 2, 4]))) for _ in range(int(rng.integers(0, 4)))])
             for _ in range(200)]
    whole = reads_table(reads)
    for lo, n in ((0, 200), (7, 150), (199, 1), (64, 0)):
        got = out_rows(sess.depth(whole.slice(lo, n)))
        assert got == out_rows(sess.depth(reads_table(reads[lo:lo + n])))
        names = sorted({r[0] for r in reads[lo:lo + n]})
        kw = orc.pack_reads([(names.index(r[0]),) + r[1:] for r in reads[lo:lo + n]])
        assert got == rows_of(names, orc.depth_loop(**kw))


def test_lengths_table(sess):
    reads = [("chr1", 5, 0, 60, [op(10, 0)]), ("chr1", 40, 0, 60, [op(10, 0)]), ("chr2", 0, 0, 60, [op(10, 0)]), ("chrUn", 0, 0, 60, [op(10, 0)])]
    # chr1: the second read's end (50) is the last slot and kept; chrUn is not in the table: skipped; chr3 has no reads
    got = out_rows(sess.depth(reads_table(reads), lengths=lengths_table({"chr3": 10, "chr1": 50, "chr2": 5})))
    assert got == [["chr1", 5, 14, 1], ["chr1", 40, 49, 1]]
    # a length above 2^32 - 1 clamps instead of wrapping
    got = out_rows(sess.depth(reads_table(reads[:1]), lengths=lengths_table({"chr1": (1 << 32) + 7})))
    assert got == [["chr1", 5, 14, 1]]


def test_prior_round_trip(sess):
    rng = np.random.default_rng(4)
    mk = lambda n: [(str(rng.choice(["1", "2", "X"])), int(rng.integers(0, 500)), 0, 60, [op(int(rng.integers(1, 30)), int(rng.choice([0, 0, 2, 1]))) for _ in range(int(rng.integers(1, 4)))])
                    for _ in range(n)]
    a, b = mk(150), mk(180)
    whole = sess.depth(reads_table(a + b))
    first = sess.depth(reads_table(a))
    acc = sess.depth(reads_table(b), prior=first)
    assert acc.equals(whole)
    assert sess.depth(reads_table([]), prior=whole).equals(whole)


def test_coverage_is_truncated_to_int16(sess):
    prior = pa.table({"contig": pa.array(["c"] * 2, pa.string()), "pos_start": pa.array([0, 0], pa.int32()), "pos_end": pa.array([9, 9], pa.int32()),
                      "coverage": pa.array([20000, 20000], pa.int32())})
    assert out_rows(sess.depth(reads_table([]), prior=prior)) == [["c", 0, 9, -25536]]


def test_errors(sess):
    reads = [("chr1", 0, 0, 60, [op(10, 0)])]
    with pytest.raises(br.BioRangesError) as ei:
        sess.depth(reads_table(reads, cigar_type=pa.string()))
    assert str(ei.value) == "depth: string CIGAR columns are not supported, use the binary CIGAR column"
    with pytest.raises(br.BioRangesError, match="column 'flags' not found"):
        sess.depth(reads_table(reads).drop(["flags"]))
    with pytest.raises(br.BioRangesError, match="expected UInt32"):
        t = reads_table(reads)
        sess.depth(t.set_column(1, "start", pa.array([0], pa.int64())))
    # a ragged CIGAR (6 bytes) is refused by the device check; the session works afterwards
    t = reads_table(reads).set_column(3, "cigar", pa.array([b"\xa0\x00\x00\x00\x00\x00"], pa.binary()))
    with pytest.raises(br.BioRangesError, match="multiples of 4"):
        sess.depth(t)
    assert out_rows(sess.depth(reads_table(reads))) == [["chr1", 0, 9, 1]]
