"""-m gpu: LeftSemi / LeftAnti / Left / Right / Full interval joins through the Arrow host layer (bio_ranges.py over
libbio_ranges_hip.so), one shot and as a stream, against a brute-force numpy outer join written here (NULL = -1).

Tables: the reference's reads.csv / targets.csv fixtures, and one seeded random pair with string contigs where one contig
exists only in the build table and one only in the probe table."""
import os
import sys

import numpy as np
import pyarrow as pa
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import bio_ranges as br  # noqa: E402

pytestmark = pytest.mark.gpu

NEW_TYPES = {"left_semi": br.JOIN_LEFT_SEMI, "left_anti": br.JOIN_LEFT_ANTI, "left": br.JOIN_LEFT, "right": br.JOIN_RIGHT,
             "full": br.JOIN_FULL}


@pytest.fixture(scope="module")
def ctx():
    s = br.Session(0)
    yield s
    s.close()


def table(rows):
    return pa.table({"contig": pa.array([r[0] for r in rows], pa.string()),
                     "pos_start": pa.array([r[1] for r in rows], pa.int64()),
                     "pos_end": pa.array([r[2] for r in rows], pa.int64())})


def random_tables():
    rng = np.random.default_rng(41)
    shared = ["chr1", "chr10", "chr2", "chrX"]

    def side(n, names):
        c = rng.choice(names, n)
        s = rng.integers(0, 400_000, n)
        return [(str(c[i]), int(s[i]), int(s[i] + rng.integers(1, 300))) for i in range(n)]

    return table(side(1500, shared + ["only_in_build"])), table(side(2500, shared + ["only_in_probe"]))


@pytest.fixture(scope="module", params=["golden", "random"])
def tables(request, golden):
    if request.param == "golden":
        return table(golden.tables["reads"]), table(golden.tables["targets"])
    return random_tables()


def cols_np(t):
    return (np.array(t.column("contig").to_pylist()), t.column("pos_start").to_numpy(), t.column("pos_end").to_numpy())


def brute_pairs(build, probe, strict):
    """every (build row, probe row) with the same contig whose closed (strict: open-ended) intervals overlap"""
    bc, bs, be = cols_np(build)
    pc_, ps, pe = cols_np(probe)
    hit = bc[:, None] == pc_[None, :]
    if strict:
        hit &= (bs[:, None] < pe[None, :]) & (be[:, None] > ps[None, :])
    else:
        hit &= (bs[:, None] <= pe[None, :]) & (be[:, None] >= ps[None, :])
    b, p = np.nonzero(hit)
    return b, p


def expected_rows(build, probe, kind, strict):
    """the join's rows as a sorted list of (build row, probe row), -1 = NULL; semi / anti: (build row, -1)"""
    b, p = brute_pairs(build, probe, strict)
    nb, np_ = build.num_rows, probe.num_rows
    lone_b = np.setdiff1d(np.arange(nb), b)
    lone_p = np.setdiff1d(np.arange(np_), p)
    if kind == "left_semi":
        return [(int(i), -1) for i in np.unique(b)]
    if kind == "left_anti":
        return [(int(i), -1) for i in lone_b]
    rows = list(zip(b.tolist(), p.tolist()))
    if kind in ("left", "full"):
        rows += [(int(i), -1) for i in lone_b]
    if kind in ("right", "full"):
        rows += [(-1, int(j)) for j in lone_p]
    return sorted(rows)


def idx(a):
    """UInt32 Arrow array -> int64 numpy, NULL = -1"""
    return np.array([-1 if v is None else v for v in a.to_pylist()], np.int64)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("kind", list(NEW_TYPES))
def test_one_shot(ctx, tables, kind, strict):
    build, probe = tables
    bi, pi = ctx.interval_join(build, probe, join_type=NEW_TYPES[kind], strict_predicate=strict)
    want = expected_rows(build, probe, kind, strict)
    b = idx(bi)
    if kind in ("left_semi", "left_anti"):
        assert len(pi) == 0 and bi.null_count == 0
        assert (np.diff(b) > 0).all()                               # ascending
        assert [(int(i), -1) for i in b] == want
        return
    p = idx(pi)
    assert sorted(zip(b.tolist(), p.tolist())) == want
    # the NULL-extended rows follow the pairs
    n_pairs = len(brute_pairs(build, probe, strict)[0])
    assert (b[:n_pairs] >= 0).all() and (p[:n_pairs] >= 0).all()
    assert ((b[n_pairs:] < 0) | (p[n_pairs:] < 0)).all()
    assert (bi.null_count > 0) == (kind in ("right", "full") and (b < 0).any())
    assert (pi.null_count > 0) == (kind in ("left", "full") and (p < 0).any())


def stream_rows(ctx, build, batches, kind, strict, coalesce):
    js = ctx.join_stream(build, strict_predicate=strict, coalesce_rows=coalesce, join_type=kind)
    results = []
    for t in batches:
        results += js.push(t)
    results += js.finish()
    js.close()
    starts = np.cumsum([0] + [t.num_rows for t in batches])
    rows = []
    for r in results:
        b, p = idx(r["build_idx"]), idx(r["probe_idx"])
        off = r["batch_offsets"].to_numpy()
        assert len(off) == r["n_batches"] + 1 and off[0] == 0
        if r["n_batches"]:
            assert len(b) == len(p)
            p = np.where(p >= 0, p + starts[r["first_batch"]], -1)
            assert (np.diff(off) == [batches[r["first_batch"] + j].num_rows for j in range(r["n_batches"])]).all()
        elif len(p) == 0:
            p = np.full(len(b), -1, np.int64)                       # semi / anti: build rows only
        rows += list(zip(b.tolist(), p.tolist()))
    return rows, results


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("kind", list(NEW_TYPES))
def test_stream(ctx, tables, kind, strict):
    build, probe = tables
    third = (probe.num_rows + 2) // 3
    batches = [probe.slice(i, third) for i in range(0, probe.num_rows, third)]
    assert len(batches) == 3
    want = expected_rows(build, probe, kind, strict)
    for coalesce, groups in ((1, 3), (third + 1, 2), (0, 1)):
        rows, results = stream_rows(ctx, build, batches, kind, strict, coalesce)
        last = results[-1]
        assert last["n_batches"] == 0 and last["batch_offsets"].to_pylist() == [0] and last["first_batch"] == 3
        assert all(r["n_batches"] > 0 for r in results[:-1])
        if kind in ("left_semi", "left_anti"):
            assert len(results) == 1                                # the groups give no result
            b = idx(last["build_idx"])
            assert (np.diff(b) > 0).all() and len(last["probe_idx"]) == 0
            assert rows == want
        else:
            assert len(results) == groups + 1
            assert sorted(rows) == want
            b, p = idx(last["build_idx"]), idx(last["probe_idx"])
            assert (np.diff(b) > 0).all() and (p == -1).all() and len(p) == len(b)
            if kind == "right":
                assert len(b) == 0
            for r in results[:-1]:                                  # inside a group, too, the NULL-extended rows follow the pairs
                gb = idx(r["build_idx"])
                first_null = np.flatnonzero(gb < 0)
                assert len(first_null) == 0 or (gb[first_null[0]:] < 0).all()
                assert r["probe_idx"].null_count == 0


def test_low_memory_mode_is_refused(ctx, tables):
    build, _ = tables
    for kind in NEW_TYPES:
        for budget in (1, 1000, "env"):
            with pytest.raises(br.BioRangesError, match="low-memory mode.*not supported"):
                ctx.join_stream(build, join_type=kind, max_output_rows=budget)
    with pytest.raises(br.BioRangesError, match="CoitreesNearest is an Inner join"):
        ctx.interval_join(build, build, join_type=br.JOIN_LEFT, nearest_algorithm=True)


def test_existing_modes_unchanged(ctx, tables):
    """Inner, RightSemi, RightAnti and the nearest algorithm (one shot and stream) still return what they did"""
    build, probe = tables
    for strict in (False, True):
        b, p = brute_pairs(build, probe, strict)
        bi, pi = ctx.interval_join(build, probe, join_type=br.JOIN_INNER, strict_predicate=strict)
        assert bi.null_count == 0 and pi.null_count == 0
        assert sorted(zip(idx(bi).tolist(), idx(pi).tolist())) == sorted(zip(b.tolist(), p.tolist()))
        matched = np.unique(p)
        bi, pi = ctx.interval_join(build, probe, join_type=br.JOIN_RIGHT_SEMI, strict_predicate=strict)
        assert len(bi) == 0 and (idx(pi) == matched).all()
        bi, pi = ctx.interval_join(build, probe, join_type=br.JOIN_RIGHT_ANTI, strict_predicate=strict)
        assert len(bi) == 0 and (idx(pi) == np.setdiff1d(np.arange(probe.num_rows), matched)).all()
        for kind, want in (("inner", sorted(zip(b.tolist(), p.tolist()))), ("right_semi", [(-1, int(j)) for j in matched])):
            js = ctx.join_stream(build, strict_predicate=strict, coalesce_rows=1, join_type=kind)
            res = js.push(probe) + js.finish()
            js.close()
            assert len(res) == 1 and res[0]["n_batches"] == 1       # no build-side result behind the last group
            gb, gp = idx(res[0]["build_idx"]), idx(res[0]["probe_idx"])
            if kind == "right_semi":
                gb = np.full(len(gp), -1)
            assert sorted(zip(gb.tolist(), gp.tolist())) == want
    # nearest: one row per probe row, at the smallest distance; NULL where the contig has no build rows
    bc, bs, be = cols_np(build)
    pc_, ps, pe = cols_np(probe)
    bi, pi = ctx.interval_join(build, probe, nearest_algorithm=True)
    js = ctx.join_stream(build, join_type="nearest")
    res = js.push(probe) + js.finish()
    js.close()
    assert len(res) == 1
    for b, p in ((idx(bi), idx(pi)), (idx(res[0]["build_idx"]), idx(res[0]["probe_idx"]))):
        assert (p == np.arange(probe.num_rows)).all()
        for j in range(probe.num_rows):
            same = np.flatnonzero(bc == pc_[j])
            if len(same) == 0:
                assert b[j] == -1
                continue
            d = np.maximum(0, np.maximum(bs[same] - pe[j], ps[j] - be[same]))
            i = b[j]
            assert i >= 0 and bc[i] == pc_[j] and max(0, bs[i] - pe[j], ps[j] - be[i]) == d.min()
