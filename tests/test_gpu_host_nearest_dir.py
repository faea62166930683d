"""-m gpu: Session.nearest(direction=, max_distance=) on Arrow tables (brh_nearest_dir over ivx_probe_nearest_dir) against the
cursor restatement A of tests/nearest_dir_oracle.py; the call without the new keywords is today's call."""
import os
import sys

import numpy as np
import pyarrow as pa
import pytest

from conftest import ROOT

import nearest_dir_oracle as ndo

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import bio_ranges as br  # noqa: E402

pytestmark = pytest.mark.gpu

CONTIGS = ["chr1", "chr2", "chrX"]                          # chrX only on the probe (right) side


@pytest.fixture(scope="module")
def ses():
    s = br.Session(0)
    yield s
    s.close()


def make(n, seed, nkeys):
    rng = np.random.default_rng(seed)
    key = rng.integers(0, nkeys, n)
    start = rng.integers(0, 50_000, n)
    end = start + rng.integers(0, 400, n)
    return key, start, end


def as_table(key, start, end):
    return pa.table({"contig": pa.array([CONTIGS[k] for k in key]), "pos_start": pa.array(start, pa.int64()),
                     "pos_end": pa.array(end, pa.int64()), "id": pa.array(np.arange(len(key)), pa.int64())})


@pytest.fixture(scope="module")
def data():
    b, p = make(3000, 11, 2), make(5000, 12, 3)
    p[1][::6] = b[2][:len(p[1][::6])]; p[2][::6] = p[1][::6] + 30          # probe rows that start where a build row ends
    return b, p, as_table(*b), as_table(*p), ndo.NearIndex(*b)


def rows(out, distance=True):
    """(build row or None, probe row[, distance or None]) per output row, in output order"""
    cols = [out.column("left_id").to_pylist(), out.column("right_id").to_pylist()]
    if distance:
        cols.append(out.column("distance").to_pylist())
    return list(zip(*cols))


def expected(oix, p, distance=True, **kw):
    b, r, d = oix.query(*p, **kw)
    it = zip(b.tolist(), r.tolist(), d.tolist())
    return [((None if x == ndo.NULL_IDX else x), y) + (((None if x == ndo.NULL_IDX else z),) if distance else ()) for x, y, z in it]


@pytest.mark.parametrize("direction", ["any", "before", "after", "upstream", "downstream"])
def test_directions_and_caps(ses, data, direction):
    b, p, left, right, oix = data
    for D, k, ovl, strict in ((None, 1, True, False), (100, 1, True, False), (0, 1, False, True), (None, 2, False, False), (250, 2, True, True)):
        out = ses.nearest(left, right, k=k, overlap=ovl, strict=strict, direction=direction, max_distance=D)
        want = expected(oix, p, k=k, overlap=ovl, strict=strict, direction=direction, max_distance=D)
        assert rows(out) == want, (direction, D, k, ovl, strict)
        # NULL left rows exactly where there is no answer: every chrX row, and more under a cap
        nulls = [r for r in want if r[0] is None]
        assert out.column("left_id").null_count == len(nulls) == out.column("left_contig").null_count == out.column("distance").null_count
        assert len(nulls) >= int((p[0] == 2).sum())
        assert out.column("right_id").null_count == 0
    out = ses.nearest(left, right, k=2, compute_distance=False, direction=direction, max_distance=100)
    assert "distance" not in out.schema.names
    assert rows(out, False) == expected(oix, p, False, k=2, direction=direction, max_distance=100)


def test_defaults_are_todays_call(ses, data):
    b, p, left, right, oix = data
    for k, ovl, strict in ((1, True, False), (3, False, True)):
        plain = ses.nearest(left, right, k=k, overlap=ovl, strict=strict)
        named = ses.nearest(left, right, k=k, overlap=ovl, strict=strict, direction="any", max_distance=None)
        assert plain.equals(named)
        assert rows(plain) == expected(oix, p, k=k, overlap=ovl, strict=strict)
    # ... and the reference's own rows (integration_test.rs:906-950), as tests/test_gpu_host_api.py expects them
    l = pa.table({"contig": ["a", "a", "a"], "pos_start": [10, 30, 50], "pos_end": [20, 40, 60]})
    r = pa.table({"contig": ["a", "a", "b"], "pos_start": [22, 37, 1], "pos_end": [22, 37, 1]})
    names = ["left_contig", "left_pos_start", "left_pos_end", "right_contig", "right_pos_start", "right_pos_end", "distance"]
    want = [("a", 10, 20, "a", 22, 22, 2), ("a", 30, 40, "a", 22, 22, 8), ("a", 10, 20, "a", 37, 37, 17), ("a", 50, 60, "a", 37, 37, 13),
            (None, None, None, "b", 1, 1, None)]
    for kw in ({}, {"direction": "any", "max_distance": None}):
        out = ses.nearest(l, r, 2, False, **kw)
        assert sorted(zip(*[out.column(n).to_pylist() for n in names]), key=repr) == sorted(want, key=repr)
    # the same rows one side at a time
    out = ses.nearest(l, r, 2, False, direction="before")
    assert list(zip(out.column("left_pos_start").to_pylist(), out.column("right_pos_start").to_pylist(), out.column("distance").to_pylist())) == \
        [(10, 22, 2), (10, 37, 17), (None, 1, None)]
    out = ses.nearest(l, r, 2, False, direction="after", max_distance=10)
    assert list(zip(out.column("left_pos_start").to_pylist(), out.column("right_pos_start").to_pylist(), out.column("distance").to_pylist())) == \
        [(30, 22, 8), (None, 37, None), (None, 1, None)]


def test_bad_arguments(ses, data):
    _, _, left, right, _ = data
    with pytest.raises(ValueError):
        ses.nearest(left, right, direction="sideways")
    with pytest.raises(ValueError):
        ses.nearest(left, right, max_distance=-1)
