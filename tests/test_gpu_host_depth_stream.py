"""-m gpu: Session.depth_stream (brh_depth_push_*) on pyarrow tables: reads pushed in batches give what Session.depth and
Session.depth_per_base give for all of them in one table -- a coverage beyond Int16, and what the `prior` round trip cannot do (a contig clipped at
its length, per-base output) -- and the stream's protocol."""
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
import depth_per_base_oracle as pbo  # noqa: E402

pytestmark = pytest.mark.gpu

op = lambda n, c: (n << 4) | c
BLOCK_TYPES = [pa.string(), pa.int32(), pa.int32(), pa.int16()]


@pytest.fixture(scope="module")
def sess():
    s = br.Session(0)
    yield s
    s.close()


def reads_table(reads, cigar_type=pa.binary()):
    """[(chrom, start, flags, mapq, [ops])] -> a table with the reference's column names (schema.rs:7-11)"""
    cig = [struct.pack("<%dI" % len(r[4]), *r[4]) for r in reads]
    if cigar_type != pa.binary():
        cig = ["10M"] * len(reads)
    return pa.table({"chrom": pa.array([r[0] for r in reads], pa.string()), "start": pa.array([r[1] for r in reads], pa.uint32()),
                     "flags": pa.array([r[2] for r in reads], pa.uint32()), "cigar": pa.array(cig, cigar_type),
                     "mapping_quality": pa.array([r[3] for r in reads], pa.uint32())})


def lengths_table(d):
    return pa.table({"name": pa.array(list(d), pa.string()), "length": pa.array(list(d.values()), pa.int64())})


def out_rows(t):
    return [list(r) for r in zip(*[t.column(c).to_pylist() for c in ("contig", "pos_start", "pos_end", "coverage")])]


def random_reads(rng, n, contigs=("1", "2", "X")):
    return [(str(rng.choice(contigs)), int(rng.integers(0, 500)), int(rng.choice([0, 0, 0, 4, 1024])), int(rng.choice([0, 30, 60])),
             [op(int(rng.integers(1, 30)), int(rng.choice([0, 0, 2, 1, 7]))) for _ in range(int(rng.integers(1, 4)))]) for _ in range(n)]


def split(rows, parts):
    cuts = [len(rows) * i // parts for i in range(parts + 1)]
    return [rows[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def streamed(sess, batches, **kw):
    with sess.depth_stream(**kw) as ds:
        for b in batches:
            ds.push(reads_table(b))
        return ds.finish()


LENGTHS = {"X": 300, "1": 450, "3": 100}              # "2" is not in the table: its reads are skipped; "3" has no reads


@pytest.mark.parametrize("parts", [1, 2, 7])
@pytest.mark.parametrize("dense", [False, True])
def test_batches_equal_the_whole(sess, parts, dense):
    reads = random_reads(np.random.default_rng(11), 400)
    kw = dict(min_mapq=20, lengths=lengths_table(LENGTHS) if dense else None)
    whole = sess.depth(reads_table(reads), **kw)
    assert whole.num_rows > 100
    got = streamed(sess, split(reads, parts), **kw)
    assert [f.type for f in got.schema] == BLOCK_TYPES and got.equals(whole)


def test_contigs_arrive_in_another_order(sess):
    mk = lambda c, n, seed: random_reads(np.random.default_rng(seed), n, contigs=(c,))
    batches = [mk("chrX", 60, 1), mk("chr2", 50, 2) + mk("chrX", 10, 3), mk("chr1", 40, 4), mk("chr10", 5, 5) + mk("chr2", 5, 6)]
    whole = sess.depth(reads_table(sum(batches, [])))
    got = streamed(sess, batches)
    assert got.equals(whole)
    seen = list(dict.fromkeys(got.column("contig").to_pylist()))
    assert seen == ["chr1", "chr10", "chr2", "chrX"]


# ---------------------------------------------------------------------------------------------- what prior= cannot do
def test_coverage_beyond_int16(sess):
    reads = [("c", 7, 0, 60, [op(3, 0)])] * 40000
    whole = sess.depth(reads_table(reads))
    assert out_rows(whole) == [["c", 7, 9, 40000 - 65536]]
    assert streamed(sess, [reads[:20000], reads[20000:]]).equals(whole)


def test_clipped_contig_then_a_later_read(sess):
    lengths = lengths_table({"c": 50})
    b1 = [("c", 10, 0, 60, [op(10, 0)]), ("c", 45, 0, 60, [op(10, 0)])]        # the second read's end (55) is beyond the length
    b2 = [("c", 48, 0, 60, [op(1, 0)]), ("c", 2, 0, 60, [op(3, 0)])]
    whole = sess.depth(reads_table(b1 + b2), lengths=lengths)
    assert out_rows(whole) == [["c", 2, 4, 1], ["c", 10, 19, 1], ["c", 45, 47, 1], ["c", 48, 48, 2]]
    assert streamed(sess, [b1, b2], lengths=lengths).equals(whole)
    # ... which the prior round trip loses: batch 1's open block [45, ...) is not among its blocks
    first = sess.depth(reads_table(b1), lengths=lengths)
    assert out_rows(first) == [["c", 10, 19, 1]]
    assert not sess.depth(reads_table(b2), prior=first, lengths=lengths).equals(whole)


@pytest.mark.parametrize("zero_based", [False, True])
@pytest.mark.parametrize("batch_rows", [1, 7, 8192])
def test_per_base_over_three_pushes(sess, zero_based, batch_rows):
    reads = random_reads(np.random.default_rng(21), 90)
    reads += [("3", 5, 0, 60, [op(0, 0)])]                                       # events that cancel: the contig is still emitted
    reads += [("1", 3, 0, 60, [op(10, 0)]), ("X", 60, 0, 60, [op(10, 0)])]       # (both short contigs have a read inside them)
    lengths = lengths_table(dict(LENGTHS, **{"1": 37, "X": 64}))
    kw = dict(zero_based=zero_based, batch_rows=batch_rows)
    want = list(sess.depth_per_base(reads_table(reads), lengths=lengths, **kw))
    with sess.depth_stream(lengths=lengths) as ds:
        for b in split(reads, 3):
            ds.push(reads_table(b))
        got = list(ds.finish_per_base(**kw))
    assert len(got) == len(want) and len(got) >= 3
    for g, w in zip(got, want):
        assert g.schema == w.schema and g.equals(w)
    assert {t.column("contig")[0].as_py() for t in got} == {"1", "3", "X"}


# ---------------------------------------------------------------------------------------------- protocol
def test_empty_stream_and_empty_batches(sess):
    for lengths in (None, lengths_table(LENGTHS)):
        empty = streamed(sess, [], lengths=lengths)
        assert empty.num_rows == 0 and empty.schema.names == ["contig", "pos_start", "pos_end", "coverage"]
        assert [f.type for f in empty.schema] == BLOCK_TYPES
        assert streamed(sess, [[], []], lengths=lengths).equals(empty)
    reads = random_reads(np.random.default_rng(5), 50)
    assert streamed(sess, [[], reads[:20], [], reads[20:], []]).equals(sess.depth(reads_table(reads)))
    with sess.depth_stream(lengths=lengths_table(LENGTHS)) as ds:
        assert list(ds.finish_per_base()) == []


def test_bad_batch_leaves_the_stream_usable(sess):
    reads = random_reads(np.random.default_rng(6), 40)
    with sess.depth_stream() as ds:
        ds.push(reads_table(reads[:25]))
        with pytest.raises(br.BioRangesError) as ei:
            ds.push(reads_table(reads[25:], cigar_type=pa.string()))
        assert str(ei.value) == "depth: string CIGAR columns are not supported, use the binary CIGAR column"
        with pytest.raises(br.BioRangesError, match="column 'flags' not found"):
            ds.push(reads_table(reads[25:]).drop(["flags"]))
        ds.push(reads_table(reads[25:]))
        assert ds.finish().equals(sess.depth(reads_table(reads)))


def test_finish_rules(sess):
    reads = random_reads(np.random.default_rng(7), 30)
    with sess.depth_stream() as ds:
        ds.push(reads_table(reads))
        with pytest.raises(br.BioRangesError) as ei:
            next(ds.finish_per_base())
        assert str(ei.value) == pbo.REFERENCE_ERROR
        t = ds.finish()                                                         # (the refusal did not finish the stream)
        assert t.equals(sess.depth(reads_table(reads)))
        for again in (lambda: ds.push(reads_table(reads)), ds.finish, lambda: next(ds.finish_per_base())):
            with pytest.raises(br.BioRangesError) as ei:
                again()
            assert str(ei.value) == "depth stream: already finished"
    with sess.depth_stream(lengths=lengths_table(LENGTHS)) as ds:
        ds.push(reads_table(reads))
        assert len(list(ds.finish_per_base())) >= 1
        with pytest.raises(br.BioRangesError, match="already finished"):
            ds.finish()


def test_close_returns_the_reservation(sess):
    reads = random_reads(np.random.default_rng(8), 300)
    lengths = lengths_table(LENGTHS)
    want = sess.depth(reads_table(reads))
    before = None
    for warm in (True, False):                                                  # (the first round grows the scratch to what these calls need)
        if not warm:
            before = sess.reserved_bytes()
        assert streamed(sess, split(reads, 5)).equals(want)
        ds = sess.depth_stream()
        for b in split(reads, 5)[:3]:
            ds.push(reads_table(b))
        held = sess.reserved_bytes()                                            # the profiles on the stack are reserved
        ds.close()                                                              # ... and given back without a finish
        with sess.depth_stream(lengths=lengths) as ds:
            ds.push(reads_table(reads))
            gen = ds.finish_per_base(batch_rows=100)
            next(gen)
            moved = sess.reserved_bytes()                                       # the profile lives on in the pull stream
            gen.close()
        if not warm:
            assert held > before and moved > before and sess.reserved_bytes() == before
