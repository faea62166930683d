"""-m gpu: Session.overlap_aggregate (bio_ranges.py over libbio_ranges_hip.so): the overlap join grouped by probe row with a
build-side value aggregated, as Arrow Int64 columns -- against the table computed by hand in tests/test_overlap_agg_cpu.py, a
brute force over string contigs written here, and pyivx on the same data."""
import os
import sys

import numpy as np
import pyarrow as pa
import pytest

from conftest import ROOT, encode_keys
import overlap_agg_oracle as agg
from test_overlap_agg_cpu import HAND

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import bio_ranges as br  # noqa: E402
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

NULLABLE = ("sum", "min", "max", "wsum")


@pytest.fixture(scope="module")
def ses():
    s = br.Session(0)
    yield s
    s.close()


def table(rows, values=None, vtype=pa.int32()):
    cols = {"contig": pa.array([r[0] for r in rows], pa.string()),
            "pos_start": pa.array([r[1] for r in rows], pa.int64()),
            "pos_end": pa.array([r[2] for r in rows], pa.int64())}
    if values is not None:
        cols["score"] = pa.array(values, vtype)
    return pa.table(cols)


def brute(build, probe, values, strict=False):
    """{op: list with None for NULL}, in Python integers (no wrapping happens at these sizes)"""
    out = {o: [] for o in br.AGG_OPS}
    d = 1 if strict else 0
    for pc_, ps, pe in probe:
        m = [(v, min(pe - d, be - d) - max(ps, bs) + 1) for (bc, bs, be), v in zip(build, values)
             if bc == pc_ and bs <= pe - d and be - d >= ps]
        out["count"].append(len(m)); out["bases"].append(sum(ln for _, ln in m))
        out["sum"].append(sum(v for v, _ in m) if m else None)
        out["min"].append(min(v for v, _ in m) if m else None)
        out["max"].append(max(v for v, _ in m) if m else None)
        out["wsum"].append(sum(v * ln for v, ln in m) if m else None)
    return out


def check(got, want, ops=br.AGG_OPS):
    assert got.schema.names == list(ops)
    for o in ops:
        col = got.column(o)
        assert col.type == pa.int64(), o
        assert col.to_pylist() == want[o], o
        assert (col.null_count > 0) == (None in want[o]), o
        if o not in NULLABLE:
            assert col.null_count == 0


def test_golden_table_with_contig_strings(ses, golden):
    reads, targets = golden.tables["reads"], golden.tables["targets"] + [["chr3", 100, 190]]
    values = [i + 1 if r[0] == "chr1" else 100 + i for i, r in enumerate(reads)]        # chr1: 1..6 in file order
    got = ses.overlap_aggregate(table(reads, values), table(targets), "score")
    want = brute(reads, targets, values)
    check(got, want)
    for i, t in enumerate(targets):
        if t[0] == "chr1":
            assert tuple(got.column(o)[i].as_py() for o in br.AGG_OPS) == HAND[(t[1], t[2])], t
    last = {o: got.column(o)[len(targets) - 1].as_py() for o in br.AGG_OPS}             # chr3: no build rows
    assert last == {"count": 0, "sum": None, "min": None, "max": None, "bases": 0, "wsum": None}


def random_sides(seed=41):
    rng = np.random.default_rng(seed)
    shared = ["chr1", "chr10", "chr2", "chrX"]

    def side(n, names):
        c = rng.choice(names, n)
        s = rng.integers(0, 400_000, n)
        return [(str(c[i]), int(s[i]), int(s[i] + rng.integers(1, 300))) for i in range(n)]

    return side(1500, shared + ["only_in_build"]), side(2500, shared + ["only_in_probe"]), rng


@pytest.mark.parametrize("vtype", [pa.int8(), pa.int32(), pa.uint32(), pa.int64()], ids=str)
def test_value_dtypes_nulls_and_pyivx(ses, vtype):
    build, probe, rng = random_sides()
    lo, hi = {pa.int8(): (-128, 128), pa.int32(): (-2**31, 2**31), pa.uint32(): (0, 2**32), pa.int64(): (-2**40, 2**40)}[vtype]
    values = [int(v) for v in rng.integers(lo, hi, len(build))]
    values[0], values[1] = lo, hi - 1                                                   # the type's extremes
    got = ses.overlap_aggregate(table(build, values, vtype), table(probe), "score")
    want = brute(build, probe, values)
    assert 0 in want["count"] and None in want["sum"] and max(want["count"]) > 1        # NULLs where the count is 0
    check(got, want)
    # a subset of the ops, in the caller's order
    sub = ("max", "count")
    check(ses.overlap_aggregate(table(build, values, vtype), table(probe), "score", ops=sub), want, sub)
    # the same data through pyivx: equal wherever the session gives a value
    names, (b, p) = encode_keys([list(r) for r in build], [list(r) for r in probe])
    c = pyivx.Ctx(0)
    try:
        cast = lambda t: tuple(np.ascontiguousarray(x, d) for x, d in zip(t, (np.uint32, np.int32, np.int32)))
        ix = c.build(pyivx.KIND_OVERLAP, *cast(b), n_keys=len(names))
        val = np.asarray(values, np.int64 if vtype in (pa.uint32(), pa.int64()) else np.int32)
        raw = c.overlap_agg(ix, *cast(p), val)
        ix.free()
    finally:
        c.close()
    some = raw["count"] != 0
    for o in br.AGG_OPS:
        col = np.asarray(got.column(o).fill_null(0).to_pylist(), np.int64)
        keep = some if o in NULLABLE else np.ones(len(some), bool)
        assert (col[keep] == raw[o][keep].astype(np.int64)).all(), o
        if o in NULLABLE:
            assert (np.asarray(got.column(o).is_null()) == ~some).all(), o
    assert (raw["min"][~some] == agg.I64_MAX).all() and (raw["max"][~some] == agg.I64_MIN).all()


def test_strict_predicate_on_touching_intervals(ses):
    build = [("chr1", 100, 200), ("chr1", 200, 300), ("chr1", 300, 300), ("chr2", 100, 200)]
    probe = [("chr1", 200, 250), ("chr1", 50, 100), ("chr1", 300, 400), ("chr1", 199, 201), ("chr2", 200, 300)]
    values = [10, 20, 40, 80]
    weak = ses.overlap_aggregate(table(build, values), table(probe), "score")
    check(weak, brute(build, probe, values))
    assert weak.column("count").to_pylist() == [2, 1, 2, 2, 1]
    strict = ses.overlap_aggregate(table(build, values), table(probe), "score", strict_predicate=True)
    want = brute(build, probe, values, strict=True)
    check(strict, want)
    # touching ends no longer match; bases and wsum are on the adjusted (end - 1) coordinates
    assert want["count"] == [1, 0, 0, 2, 0] and want["bases"] == [50, 0, 0, 2, 0] and want["wsum"] == [1000, None, None, 30, None]


@pytest.mark.parametrize("case", ["uint64", "float64", "null_value", "missing"])
def test_rejections(ses, case):
    build, probe = [("chr1", 100, 200), ("chr1", 150, 250)], [("chr1", 160, 170)]
    vals, vtype, message = {
        "uint64": ([1, 2], pa.uint64(), "UInt64 values do not fit"),
        "float64": ([1.5, 2.5], pa.float64(), "float values are not supported"),
        "null_value": ([1, None], pa.int32(), "contains null values"),
        "missing": ([1, 2], pa.int32(), "not found in batch with columns"),
    }[case]
    with pytest.raises(br.BioRangesError) as ei:
        ses.overlap_aggregate(table(build, vals, vtype), table(probe), "score" if case != "missing" else "no_such_column")
    assert message in str(ei.value) and "overlap_aggregate" in str(ei.value), str(ei.value)
    with pytest.raises(br.BioRangesError):
        ses.overlap_aggregate(table(build, [1, 2]), table(probe), "score", ops=("count", "median"))
    # the session still works afterwards
    ok = ses.overlap_aggregate(table(build, [1, 2]), table(probe), "score")
    assert ok.column("sum").to_pylist() == [3]
