"""-m gpu: Session.overlap_select (bio_ranges.py over libbio_ranges_hip.so): the overlap join reduced to the one best build
row per probe row, as a nullable UInt32 build_idx and a nullable Int64 score -- against the table computed by hand in
tests/test_overlap_select_cpu.py, with the value column in every type the operator takes, and its refusals."""
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from conftest import ROOT
import overlap_select_oracle as sel
from test_overlap_select_cpu import B_HAND, P_HAND, cols, hand_want

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import bio_ranges as br  # noqa: E402

pytestmark = pytest.mark.gpu

NULL = sel.NULL_IDX
HAND_VALUES = [r[3] for r in B_HAND]


@pytest.fixture(scope="module")
def ses():
    s = br.Session(0)
    yield s
    s.close()


def table(rows, values=None, vtype=pa.int32(), payload=False):
    c = {"contig": pa.array([f"chr{r[0]}" for r in rows], pa.string()),
         "pos_start": pa.array([r[1] for r in rows], pa.int64()),
         "pos_end": pa.array([r[2] for r in rows], pa.int64())}
    if values is not None:
        c["score"] = pa.array(values, vtype)
    if payload:
        c["name"] = pa.array([f"gene{i}" for i in range(len(rows))], pa.string())
    return pa.table(c)


BUILD_ROWS = [r[:3] for r in B_HAND]
PROBE_ROWS = [r[0] for r in P_HAND]


def check(got, by, score_of=None):
    """build_idx and score against the hand table; score_of: winner row -> the score expected (None: no score column)"""
    idx, score = got
    widx, wscore = hand_want(by)
    assert idx.type == pa.uint32() and len(idx) == len(widx)
    assert idx.to_pylist() == [None if w == NULL else int(w) for w in widx], by
    assert idx.null_count == int((widx == NULL).sum()) > 0
    if score_of is None:
        assert score is None, by
        return
    assert score.type == pa.int64()
    assert score.to_pylist() == [None if w == NULL else score_of(int(w), int(c)) for w, c in zip(widx, wscore)], by
    assert score.null_count == idx.null_count


@pytest.mark.parametrize("by", sel.BY)
def test_hand_table(ses, by):
    value = "score" if by.endswith("_val") else None
    got = ses.overlap_select(table(BUILD_ROWS, HAND_VALUES), table(PROBE_ROWS), by, value=value)
    check(got, by, lambda row, c: c)


# the hand table's values through an order-preserving map into each type: the winners stay, the score is the mapped value (or
# absent where the device compares a key of the value, not the value)
TYPES = {
    "int8": (pa.int8(), lambda v: v, True),
    "int64": (pa.int64(), lambda v: v * 2**40, True),
    "uint32": (pa.uint32(), lambda v: v + 2**32 - 10, True),             # above 2^31: not an int32
    "uint64": (pa.uint64(), lambda v: v + 2**63 + 3, False),             # above 2^63: not an int64
    "uint64_small_and_large": (pa.uint64(), lambda v: v + 3 if v < 7 else 2**64 - 10 + v, False),
    "float32": (pa.float32(), lambda v: v * 0.5, False),                 # negative, fractional
    "float64": (pa.float64(), lambda v: -1e300 if v == -3 else v * 1e-3, False),
}


@pytest.mark.parametrize("by", ["min_val", "max_val"])
@pytest.mark.parametrize("kind", list(TYPES))
def test_value_column_types(ses, kind, by):
    vtype, f, exact = TYPES[kind]
    mapped = [f(v) for v in HAND_VALUES]
    assert sorted(range(8), key=lambda i: (mapped[i], i)) == sorted(range(8), key=lambda i: (HAND_VALUES[i], i))
    got = ses.overlap_select(table(BUILD_ROWS, mapped, vtype), table(PROBE_ROWS), by, value="score")
    check(got, by, (lambda row, c: mapped[row]) if exact else None)


@pytest.mark.parametrize("vtype", [pa.float32(), pa.float64()])
def test_negative_zero_orders_below_positive_zero(ses, vtype):
    build = [(0, 100, 200)] * 4
    vals = [0.0, -0.0, 0.0, -0.0]
    probe = [(0, 150, 160)]
    lo, _ = ses.overlap_select(table(build, vals, vtype), table(probe), "min_val", value="score")
    hi, _ = ses.overlap_select(table(build, vals, vtype), table(probe), "max_val", value="score")
    assert lo.to_pylist() == [1] and hi.to_pylist() == [0]
    # infinities are values like any other
    vals = [float("inf"), -1.0, float("-inf"), 3.0]
    lo, _ = ses.overlap_select(table(build, vals, vtype), table(probe), "min_val", value="score")
    hi, _ = ses.overlap_select(table(build, vals, vtype), table(probe), "max_val", value="score")
    assert lo.to_pylist() == [2] and hi.to_pylist() == [0]


@pytest.mark.parametrize("by", sel.BY)
def test_strict_predicate(ses, by):
    """end - 1 on both sides before anything else: the matches and the overlap lengths follow"""
    build = BUILD_ROWS + [(0, 170, 171), (0, 200, 230), (0, 170, 175)]   # rows that only touch probe row 0's end: gone when strict
    probe = PROBE_ROWS + [(0, 200, 210), (0, 171, 172)]
    vals = HAND_VALUES + [100, -100, -50]
    value = "score" if by.endswith("_val") else None
    b = cols(*zip(*build)); p = cols(*zip(*probe))
    weak = ses.overlap_select(table(build, vals), table(probe), by, value=value)
    strict = ses.overlap_select(table(build, vals), table(probe), by, value=value, strict_predicate=True)
    for got, d in ((weak, 0), (strict, 1)):
        widx, wscore = sel.brute((b[0], b[1], b[2] - d), (p[0], p[1], p[2] - d), by, np.array(vals, np.int32))
        assert got[0].to_pylist() == [None if w == NULL else int(w) for w in widx], (by, d)
        assert got[1].to_pylist() == [None if w == NULL else int(c) for w, c in zip(widx, wscore)], (by, d)
    assert weak[0].to_pylist() != strict[0].to_pylist() or weak[1].to_pylist() != strict[1].to_pylist(), by


def test_left_join_to_one_row(ses):
    """take_table(build, build_idx): the build columns of each probe row's winner, NULL rows where nothing overlaps"""
    build = table(BUILD_ROWS, HAND_VALUES, payload=True)
    idx, score = ses.overlap_select(build, table(PROBE_ROWS), "max_overlap")
    taken = ses.take_table(build, idx, prefix="b.")
    widx, _ = hand_want("max_overlap")
    assert list(taken) == ["b.contig", "b.pos_start", "b.pos_end", "b.score", "b.name"]
    assert taken["b.name"].to_pylist() == [None if w == NULL else f"gene{w}" for w in widx]
    assert taken["b.score"].to_pylist() == [None if w == NULL else HAND_VALUES[w] for w in widx]
    for name, col in taken.items():
        assert col.to_pylist() == pc.take(build.column(name[2:]), idx).to_pylist(), name


REFUSALS = [
    ("nan", "contains NaN values"),
    ("null", "contains null values"),
    ("missing_value", "selects by value and no value column is named"),
    ("superfluous_value", "given with a criterion that reads no value"),
    ("no_such_column", "not found in batch"),
    ("float16", "Float16 is not supported"),
    ("string", "unsupported data type"),
]


@pytest.mark.parametrize("case,message", REFUSALS, ids=[c for c, _ in REFUSALS])
def test_refusals(ses, case, message):
    build, probe = BUILD_ROWS[:2], PROBE_ROWS[:1]
    vals, vtype, by, value = [1, 2], pa.int32(), "max_val", "score"
    if case == "nan":
        vals, vtype = [1.0, float("nan")], pa.float64()
    elif case == "null":
        vals = [1, None]
    elif case == "missing_value":
        value = None
    elif case == "superfluous_value":
        by = "max_overlap"
    elif case == "no_such_column":
        value = "no_such_column"
    elif case == "float16":
        vals, vtype = np.array([1.0, 2.0], np.float16), pa.float16()
    elif case == "string":
        vals, vtype = ["a", "b"], pa.string()
    with pytest.raises(br.BioRangesError) as ei:
        ses.overlap_select(table(build, vals, vtype), table(probe), by, value=value)
    assert message in str(ei.value) and "overlap_select" in str(ei.value), str(ei.value)
    with pytest.raises(br.BioRangesError) as ei:
        ses.overlap_select(table(build, [1, 2]), table(probe), "median", value="score")
    assert "overlap_select: by is one of" in str(ei.value)
    # the session still works
    idx, score = ses.overlap_select(table(build, [1, 2]), table(probe), "max_val", value="score")
    assert idx.to_pylist() == [1] and score.to_pylist() == [2]
