"""-m gpu: overlap thresholds at the table level (bio_ranges.Session over libbio_ranges_hip.so): interval_join, overlap_aggregate
and overlap_select with where= -- every join type over the same filtered matches -- against tests/overlap_where_oracle.py, on
its hand-made boundary table and on a small random table; the forms a fraction may take; the refusals."""
import os
import sys
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

from conftest import ROOT, pair_set
import overlap_where_oracle as wo
from overlap_where_oracle import W
from test_overlap_where_cpu import tables

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import bio_ranges as br  # noqa: E402

pytestmark = pytest.mark.gpu

NULL = wo.sel.NULL_IDX
THRESHOLDS = {"min_bases_20": W(min_bases=20), "probe_half": W(probe=(1, 2)), "build_half": W(build=(1, 2)),
              "both_half": W(probe=(1, 2), build=(1, 2)), "either_half": W(probe=(1, 2), build=(1, 2), either=1),
              "probe_whole": W(probe=(1, 1))}


@pytest.fixture(scope="module")
def ses():
    s = br.Session(0)
    yield s
    s.close()


def table(c, values=None):
    t = {"contig": pa.array([f"chr{k}" for k in c[0].tolist()], pa.string()),
         "pos_start": pa.array(c[1].astype(np.int64)), "pos_end": pa.array(c[2].astype(np.int64))}
    if values is not None:
        t["score"] = pa.array(values, pa.int64())
    return pa.table(t)


class World:
    def __init__(self, b, p, seed=3):
        self.b, self.p = b, p
        self.val = np.random.default_rng(seed).integers(-1000, 1000, len(b[1])).astype(np.int64)
        self.B, self.P = table(b, self.val), table(p)
        self.want = wo.Want(b, p, threads=1)


WORLDS = {"hand": lambda: World(wo.HAND_BUILD, wo.HAND_PROBE), "random": lambda: World(*tables(9, 300, 400))}


@pytest.fixture(scope="module", params=list(WORLDS))
def world(request):
    return WORLDS[request.param]()


def ow(w):
    return br.OverlapWhere(**w.kw())


def u32(a):
    return a.to_numpy(zero_copy_only=False).astype(np.uint32)


def valid(a):
    return np.array([x is not None for x in a.to_pylist()], bool)


@pytest.mark.parametrize("name", list(THRESHOLDS))
def test_join_types_agree_under_a_threshold(ses, world, name):
    w, want = THRESHOLDS[name], world.want
    kb, kp = want.pairs(w)
    nb, n = want.nb, want.n
    assert len(kb) < len(want.wb), "the threshold filters nothing here"
    has_b, has_p = np.zeros(nb, bool), np.zeros(n, bool)
    has_b[kb] = True; has_p[kp] = True
    join = lambda jt: ses.interval_join(world.B, world.P, join_type=jt, where=ow(w))
    bi, pi = join(br.JOIN_INNER)
    assert len(bi) == len(kb) and (pair_set(u32(bi), u32(pi)) == pair_set(kb, kp)).all()
    assert u32(join(br.JOIN_RIGHT_SEMI)[1]).tolist() == np.flatnonzero(has_p).tolist()
    assert u32(join(br.JOIN_RIGHT_ANTI)[1]).tolist() == np.flatnonzero(~has_p).tolist()
    assert u32(join(br.JOIN_LEFT_SEMI)[0]).tolist() == np.flatnonzero(has_b).tolist()
    assert u32(join(br.JOIN_LEFT_ANTI)[0]).tolist() == np.flatnonzero(~has_b).tolist()
    # Left / Right / Full: the pairs, then exactly the rows without one
    m = len(kb)
    for jt, null_b, null_p in ((br.JOIN_LEFT, False, True), (br.JOIN_RIGHT, True, False), (br.JOIN_FULL, True, True)):
        bi, pi = join(jt)
        vb, vp = valid(bi), valid(pi)
        gb, gp = np.array([x or 0 for x in bi.to_pylist()], np.uint32), np.array([x or 0 for x in pi.to_pylist()], np.uint32)
        assert vb[:m].all() and vp[:m].all() and (pair_set(gb[:m], gp[:m]) == pair_set(kb, kp)).all(), jt
        tail_b, tail_p = ~vb[m:], ~vp[m:]
        lone_p = np.flatnonzero(~has_p) if null_b else np.zeros(0, np.int64)
        lone_b = np.flatnonzero(~has_b) if null_p else np.zeros(0, np.int64)
        assert len(bi) == m + len(lone_p) + len(lone_b), jt
        assert not (tail_b & tail_p).any()
        assert gp[m:][tail_b].tolist() == lone_p.tolist(), jt                  # probe rows without a pair: build_idx NULL
        assert gb[m:][tail_p].tolist() == lone_b.tolist(), jt                  # build rows without one: probe_idx NULL
        assert tail_b.sum() == len(lone_p) and tail_p.sum() == len(lone_b), jt


@pytest.mark.parametrize("name", list(THRESHOLDS))
def test_aggregate_and_select_under_a_threshold(ses, world, name):
    w, want = THRESHOLDS[name], world.want
    got = ses.overlap_aggregate(world.B, world.P, "score", where=ow(w))
    wa = want.agg(w, world.val)
    none = wa["count"] == 0
    assert none.any() and not none.all()
    for op in br.AGG_OPS:
        col = got.column(op).combine_chunks()
        expect = wa[op].astype(np.int64).tolist()
        if op in ("sum", "min", "max", "wsum"):
            expect = [None if z else v for v, z in zip(expect, none)]
        assert col.to_pylist() == expect, (name, op)
    for by in ("max_overlap", "min_val", "last_row"):
        idx, score = ses.overlap_select(world.B, world.P, by, value="score" if by == "min_val" else None, where=ow(w))
        wi, ws = want.select(w, by, world.val)
        assert idx.to_pylist() == [None if i == NULL else int(i) for i in wi], (name, by)
        assert score.to_pylist() == [None if i == NULL else int(s) for i, s in zip(wi, ws)], (name, by)


def test_fraction_forms_agree(ses, world):
    """a float 0.5, the pair (1, 2), Fraction(1, 2) and a dict give equal results"""
    forms = [br.OverlapWhere(probe=0.5, min_bases=2), br.OverlapWhere(probe=(1, 2), min_bases=2), br.OverlapWhere(probe=Fraction(1, 2), min_bases=2),
             {"probe": 0.5, "min_bases": 2}, br.OverlapWhere(probe=(2**29, 2**30), min_bases=2)]
    ref = None
    for f in forms:
        bi, pi = ses.interval_join(world.B, world.P, where=f)
        a = ses.overlap_aggregate(world.B, world.P, "score", where=f)
        s = ses.overlap_select(world.B, world.P, "max_overlap", where=f)
        got = (pair_set(u32(bi), u32(pi)).tolist(), a.to_pydict(), s[0].to_pylist(), s[1].to_pylist())
        if ref is None:
            ref = got
            kb, kp = world.want.pairs(W(min_bases=2, probe=(1, 2)))
            assert ref[0] == pair_set(kb, kp).tolist()
        assert got == ref, f


def test_where_none_is_the_old_call(ses, world):
    for jt in (br.JOIN_INNER, br.JOIN_RIGHT_SEMI, br.JOIN_RIGHT_ANTI, br.JOIN_LEFT_SEMI, br.JOIN_LEFT_ANTI, br.JOIN_LEFT, br.JOIN_RIGHT, br.JOIN_FULL):
        old = ses.interval_join(world.B, world.P, join_type=jt)
        for w in (None, br.OverlapWhere(), {}):
            new = ses.interval_join(world.B, world.P, join_type=jt, where=w)
            m = len(world.want.wb) if jt in (br.JOIN_INNER, br.JOIN_LEFT, br.JOIN_RIGHT, br.JOIN_FULL) else 0
            for o, g in zip(old, new):
                assert o.to_pylist()[m:] == g.to_pylist()[m:], (jt, w)
            if m:
                z = lambda a: np.array([x or 0 for x in a.to_pylist()[:m]], np.uint32)
                assert (pair_set(z(old[0]), z(old[1])) == pair_set(z(new[0]), z(new[1]))).all(), (jt, w)
    old = ses.overlap_aggregate(world.B, world.P, "score")
    sel_old = ses.overlap_select(world.B, world.P, "min_overlap")
    for w in (None, br.OverlapWhere()):
        assert ses.overlap_aggregate(world.B, world.P, "score", where=w).equals(old)
        got = ses.overlap_select(world.B, world.P, "min_overlap", where=w)
        assert got[0].equals(sel_old[0]) and got[1].equals(sel_old[1])
    # ... which still holds the pairs of rows with end < start that any asked threshold drops
    assert len(world.want.pairs(W(min_bases=1))[0]) < len(world.want.wb)
    assert len(ses.interval_join(world.B, world.P, where=br.OverlapWhere(min_bases=1))[0]) == len(world.want.pairs(W(min_bases=1))[0])


def test_refusals(ses, world):
    with pytest.raises(br.BioRangesError, match="threshold .* does not apply to Algorithm::CoitreesNearest"):
        ses.interval_join(world.B, world.P, nearest_algorithm=True, where=br.OverlapWhere(probe=(1, 2)))
    calls = [lambda w, jt=jt: ses.interval_join(world.B, world.P, join_type=jt, where=w)
             for jt in (br.JOIN_INNER, br.JOIN_RIGHT_SEMI, br.JOIN_LEFT_ANTI, br.JOIN_LEFT, br.JOIN_FULL)]
    calls += [lambda w: ses.overlap_aggregate(world.B, world.P, "score", where=w), lambda w: ses.overlap_select(world.B, world.P, "max_overlap", where=w)]
    for call in calls:
        with pytest.raises(br.BioRangesError, match="overlap_where: a fraction is above 1"):
            call(br.OverlapWhere(probe=(3, 2)))
        with pytest.raises(br.BioRangesError, match="overlap_where: a fraction is above 1"):
            call(br.OverlapWhere(build=1.5))
        with pytest.raises(br.BioRangesError, match="overlap_where: min_bases is negative"):
            call(br.OverlapWhere(min_bases=-1))
    # the session still works
    assert len(ses.interval_join(world.B, world.P)[0]) == len(world.want.wb)
