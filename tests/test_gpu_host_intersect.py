"""-m gpu: Session.intersect (bio_ranges.py over brh_intersect of libbio_ranges_hip.so) against restatement (a) of
tests/intersect_oracle.py plus a `take` of the extra left columns."""
import os
import sys

import numpy as np
import pyarrow as pa
import pytest

from conftest import ROOT, encode_keys

import intersect_oracle as io

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import bio_ranges as br  # noqa: E402

pytestmark = pytest.mark.gpu

# byte order: "10" < "2" < "MT" < "chrX"
CONTIGS = ["chrX", "2", "MT", "10"]


@pytest.fixture(scope="module")
def sess():
    s = br.Session(0)
    yield s
    s.close()


def rows_of(seed, n):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 3000, n)
    ln = rng.integers(0, 60, n)
    ln[rng.random(n) < 0.2] = 0
    return [[str(rng.choice(CONTIGS)), int(a), int(a + b)] for a, b in zip(s, ln)]


def table(rows, names=("contig", "pos_start", "pos_end"), extra=None):
    cols = {names[0]: pa.array([r[0] for r in rows], pa.string()), names[1]: pa.array([r[1] for r in rows], pa.int64()),
            names[2]: pa.array([r[2] for r in rows], pa.int64())}
    cols.update(extra or {})
    return pa.table(cols)


def expected(left, right, strict, gene, score):
    names, (L, R) = encode_keys(left, right)
    k, s, e, r = io.walk(L, R, strict)
    return {"contig": [names[i] for i in k.tolist()], "s": s.tolist(), "e": e.tolist(),
            "gene": [gene[i] for i in r.tolist()], "score": [score[i] for i in r.tolist()]}


@pytest.mark.parametrize("strict", [False, True])
def test_intersect_with_two_extra_left_columns(sess, strict):
    left, right = rows_of(1, 500), rows_of(2, 400)
    gene = [None if i % 17 == 0 else f"g{i * 7919 % 1000}" + "x" * (i % 5) for i in range(len(left))]
    score = [None if i % 23 == 0 else (i * 104729) % 100003 - 50000 for i in range(len(left))]
    lt = table(left, names=("chrom", "from", "to"), extra={"gene": pa.array(gene, pa.string()), "score": pa.array(score, pa.int64())})
    # (the extra columns sit between the interval columns in the schema: the output keeps the left table's column order)
    lt = lt.select(["gene", "chrom", "from", "score", "to"])
    out = sess.intersect(lt, table(right), cols_left=("chrom", "from", "to"), strict=strict)
    want = expected(left, right, strict, gene, score)
    assert out.schema.names == ["gene", "chrom", "from", "score", "to"]
    assert out.schema.field("chrom").type == pa.string() and out.schema.field("from").type == pa.int64() and out.schema.field("to").type == pa.int64()
    assert out.schema.field("gene").type == pa.string() and out.schema.field("score").type == pa.int64()
    assert len(want["s"]) > 100
    assert out.column("chrom").to_pylist() == want["contig"]
    assert out.column("from").to_pylist() == want["s"] and out.column("to").to_pylist() == want["e"]
    assert out.column("gene").to_pylist() == want["gene"] and out.column("score").to_pylist() == want["score"]


def test_contigs_come_out_in_byte_order(sess):
    left = [["chrX", 0, 10], ["2", 0, 10], ["MT", 0, 10], ["10", 0, 10], ["2", 5, 30]]
    right = [["10", 2, 3], ["MT", 4, 20], ["chrX", 9, 9], ["2", 8, 9], ["2", 20, 40]]
    out = sess.intersect(table(left), table(right))
    got = [list(r) for r in zip(*[out.column(n).to_pylist() for n in out.schema.names])]
    assert got == [["10", 2, 3], ["2", 8, 9], ["2", 8, 9], ["2", 20, 30], ["MT", 4, 10], ["chrX", 9, 9]]


def test_an_empty_right_table_gives_an_empty_result_with_the_schema(sess):
    left = table([["a", 1, 5], ["b", 2, 9]], extra={"gene": pa.array(["x", "y"], pa.string())})
    out = sess.intersect(left, table([]))
    assert out.num_rows == 0 and out.schema.names == ["contig", "pos_start", "pos_end", "gene"]
    assert [f.type for f in out.schema] == [pa.string(), pa.int64(), pa.int64(), pa.string()]
    out = sess.intersect(table([], extra={"gene": pa.array([], pa.string())}), table([["a", 1, 5]]))
    assert out.num_rows == 0 and out.schema.names == ["contig", "pos_start", "pos_end", "gene"]


def test_a_malformed_row_is_an_error_and_the_session_goes_on(sess):
    with pytest.raises(br.BioRangesError, match="intersect: a row with end < start"):
        sess.intersect(table([["a", 1, 5]]), table([["a", 7, 3]]))
    out = sess.intersect(table([["a", 1, 5]]), table([["a", 3, 9]]))
    assert [list(r) for r in zip(*[out.column(n).to_pylist() for n in out.schema.names])] == [["a", 3, 5]]
