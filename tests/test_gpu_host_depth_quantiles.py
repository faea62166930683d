"""-m gpu: Session.depth_region_quantiles / DepthStream.depth_region_quantiles (brh_depth_region_quantiles,
brh_depth_push_region_quantiles) on pyarrow tables, against np.sort of the rows Session.depth_per_base emits inside each
region (all of them fit Int16 here): both coordinate systems, half-open ends, regions cut by the domain, a contig without
reads, an unknown and a NULL contig, NULLs exactly where bases is 0, the errors, and the stream form, which stays open."""
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
import depth_quantiles_oracle as dqo  # noqa: E402

pytestmark = pytest.mark.gpu

op = lambda n, c: (n << 4) | c
NAMES = ["MT", "2", "10", "chrX"]
LENS = {"chrX": 300, "MT": 450, "2": 130, "10": 259, "empty": 77}           # "empty": in the table, never read
QN, QD = (0, 1, 2, 3, 4), 4


@pytest.fixture(scope="module")
def sess():
    s = br.Session(0)
    yield s
    s.close()


def reads_table(reads):
    cig = [struct.pack("<%dI" % len(r[4]), *r[4]) for r in reads]
    return pa.table({"chrom": pa.array([r[0] for r in reads], pa.string()), "start": pa.array([r[1] for r in reads], pa.uint32()),
                     "flags": pa.array([r[2] for r in reads], pa.uint32()), "cigar": pa.array(cig, pa.binary()),
                     "mapping_quality": pa.array([r[3] for r in reads], pa.uint32())})


def lengths_table(d):
    return pa.table({"name": pa.array(list(d), pa.string()), "length": pa.array(list(d.values()), pa.int64())})


def regions_table(contig, s, e):
    return pa.table({"contig": pa.array(contig, pa.string()), "pos_start": pa.array(s, pa.int64()), "pos_end": pa.array(e, pa.int64())})


def random_reads(rng, n):
    return [(str(rng.choice(NAMES)), int(rng.integers(1, 400)), int(rng.choice([0, 0, 4])), 60,
             [op(int(rng.integers(1, 30)), int(rng.choice([0, 0, 2, 7]))) for _ in range(int(rng.integers(1, 4)))]) for _ in range(n)]


def per_base(sess, reads, zero_based):
    """contig -> (first position, coverage int16 of every position) from the per-base rows"""
    rows = {}
    for t in sess.depth_per_base(reads, lengths=lengths_table(LENS), zero_based=zero_based):
        c = t.column("contig")[0].as_py()
        rows.setdefault(c, []).append((t.column("pos").to_numpy(), t.column("coverage").to_numpy()))
    out = {}
    for c, parts in rows.items():
        pos, cov = np.concatenate([p for p, _ in parts]), np.concatenate([v for _, v in parts])
        assert np.array_equal(pos, pos[0] + np.arange(len(pos))) and pos[0] == (0 if zero_based else 1) and len(pos) == LENS[c]
        out[c] = (int(pos[0]), cov)
    return out


def want_of(rows, contig, s, e, zero_based, qn, qd):
    """per region -> (bases, min, max, quantiles), None where there is no base: np.sort of the rows inside the region"""
    first = 0 if zero_based else 1
    out = []
    for c, a, b in zip(contig, s, e):
        if c not in LENS:                                   # an unknown or NULL contig: no domain, coverage 0 everywhere
            n = max(min(b, 0xFFFFFFFF) - max(a, 0) + 1, 0)
            out.append((n,) + ((0, 0, [0] * len(qn)) if n else (None, None, [None] * len(qn))))
            continue
        a, b = max(a, first), min(b, first + LENS[c] - 1)
        if b < a:
            out.append((0, None, None, [None] * len(qn)))
            continue
        cov = rows[c][1] if c in rows else np.zeros(LENS[c], np.int16)
        w = np.sort(cov[a - first: b - first + 1].astype(np.int64))
        out.append((len(w), int(w[0]), int(w[-1]), [int(w[dqo.rank(len(w), q, qd)]) for q in qn]))
    return out


def check_table(t, want, qn, qd):
    names = ["bases", "min", "max"] + [f"q_{q}_{qd}" for q in qn]
    assert t.schema.names[3:] == names
    assert t.schema.field("bases").type == pa.int64() and t.column("bases").null_count == 0
    for nm in names[1:]:
        assert t.schema.field(nm).type == pa.int32()
    assert t.column("bases").to_pylist() == [w[0] for w in want]
    assert t.column("min").to_pylist() == [w[1] for w in want] and t.column("max").to_pylist() == [w[2] for w in want]
    for j, nm in enumerate(names[3:]):
        assert t.column(nm).to_pylist() == [w[3][j] for w in want]
    for nm in names[1:]:                                    # NULL exactly where there is no base
        assert [v is None for v in t.column(nm).to_pylist()] == [w[0] == 0 for w in want]


def some_regions(rng, n, half_open):
    contig = [str(x) for x in rng.choice(NAMES + ["empty"], n)]
    s = rng.integers(0, 300, n)
    e = s + rng.integers(0, 300, n) * rng.integers(0, 2, n) + rng.integers(0, 20, n)
    contig += ["MT", "MT", "2", "2", "chrQ", None, "chrQ", "empty", "10"]
    s = np.concatenate([s, [0, 451, 100, 1, 10, 1, 9, 0, 5]])
    e = np.concatenate([e, [10 ** 6, 10 ** 6, 99, 130, 19, 4, 3, 10 ** 6, 5]])      # the whole contig, beyond it, end < start, ...
    return contig, s.tolist(), (e + (1 if half_open else 0)).tolist(), e.tolist()


@pytest.mark.parametrize("end_exclusive", [False, True])
@pytest.mark.parametrize("zero_based", [True, False])
def test_against_the_sorted_per_base_rows(sess, zero_based, end_exclusive):
    rng = np.random.default_rng(5 + zero_based)
    reads = reads_table(random_reads(rng, 260))
    rows = per_base(sess, reads, zero_based)
    assert set(rows) == set(NAMES) and max(int(v.max()) for _, v in rows.values()) > 4
    contig, s, e_given, e = some_regions(rng, 150, end_exclusive)
    t = sess.depth_region_quantiles(reads, regions_table(contig, s, e_given), lengths=lengths_table(LENS), zero_based=zero_based,
                                    end_exclusive=end_exclusive, q_num=QN, q_den=QD)
    want = want_of(rows, contig, s, e, zero_based, QN, QD)
    assert sum(w[0] == 0 for w in want) >= 4 and sum(w[0] > 0 and w[1] != w[2] for w in want) > 50
    check_table(t, want, QN, QD)
    assert t.column("contig").to_pylist() == contig and t.column("pos_start").to_pylist() == s
    t = sess.depth_region_quantiles(reads, regions_table(contig, s, e_given), lengths=lengths_table(LENS), zero_based=zero_based,
                                    end_exclusive=end_exclusive)                        # the default: the lower median alone
    check_table(t, want_of(rows, contig, s, e, zero_based, (1,), 2), (1,), 2)
    t = sess.depth_region_quantiles(reads, regions_table(contig, s, e_given), lengths=lengths_table(LENS), zero_based=zero_based,
                                    end_exclusive=end_exclusive, q_num=())
    check_table(t, want_of(rows, contig, s, e, zero_based, (), 2), (), 2)


def test_errors(sess):
    reads = reads_table([("a", 5, 0, 60, [op(10, 0)])])
    reg = regions_table(["a", "a"], [1, None], [9, 9])
    with pytest.raises(br.BioRangesError, match="coordinate column contains null values"):
        sess.depth_region_quantiles(reads, reg)
    reg = regions_table(["a"], [1], [9])
    with pytest.raises(br.BioRangesError, match="more than 8 quantiles"):
        sess.depth_region_quantiles(reads, reg, q_num=range(9), q_den=9)
    for qn, qd in (((3,), 2), ((1,), 0), ((1,), 65537)):
        with pytest.raises(br.BioRangesError, match="q_den|q_num"):
            sess.depth_region_quantiles(reads, reg, q_num=qn, q_den=qd)
    with pytest.raises(br.BioRangesError, match="not found"):
        sess.depth_region_quantiles(reads, reg, cols=("contig", "from", "pos_end"))
    t = sess.depth_region_quantiles(reads, reg.slice(0, 0), q_num=(1,))                 # no regions: empty columns
    assert t.num_rows == 0 and t.schema.names[3:] == ["bases", "min", "max", "q_1_2"]
    t = sess.depth_region_quantiles(reads, regions_table(["a", "a", "b"], [0, 5, 1], [4, 14, 3]), q_num=(0, 65536), q_den=65536)
    assert t.column("bases").to_pylist() == [5, 10, 3] and t.column("min").to_pylist() == [0, 1, 0] and t.column("max").to_pylist() == [0, 1, 0]
    assert t.column("q_0_65536").to_pylist() == [0, 1, 0] and t.column("q_65536_65536").to_pylist() == [0, 1, 0]


@pytest.mark.parametrize("dense", [True, False])
def test_stream_equals_the_one_shot_call_and_stays_open(sess, dense):
    rng = np.random.default_rng(41 + dense)
    batches = [random_reads(rng, 150), random_reads(rng, 20), random_reads(rng, 90)]
    L = lengths_table(LENS) if dense else None
    contig, s, e_given, _ = some_regions(rng, 120, True)
    reg = regions_table(contig, s, e_given)
    kw = dict(q_num=QN, q_den=QD, zero_based=False, end_exclusive=True)
    with sess.depth_stream(lengths=L) as ds:
        for b in batches[:2]:
            ds.push(reads_table(b))
        two = ds.depth_region_quantiles(reg, **kw)
        assert two.equals(sess.depth_region_quantiles(reads_table(batches[0] + batches[1]), reg, lengths=L, **kw))
        assert two.equals(ds.depth_region_quantiles(reg, **kw))             # asking again changes nothing
        ds.push(reads_table(batches[2]))                                    # the stream still takes a push ...
        three = ds.depth_region_quantiles(reg, **kw)
        allr = reads_table(batches[0] + batches[1] + batches[2])
        assert three.equals(sess.depth_region_quantiles(allr, reg, lengths=L, **kw)) and not three.equals(two)
        if dense:
            check_table(three, want_of(per_base(sess, allr, False), contig, s, [x - 1 for x in e_given], False, QN, QD), QN, QD)
        assert ds.finish().equals(sess.depth(allr, lengths=L))              # ... and finishes to the blocks it always gave
        with pytest.raises(br.BioRangesError, match="depth stream: already finished"):
            ds.depth_region_quantiles(reg, **kw)
    with sess.depth_stream(lengths=L) as ds:                                # nothing pushed: zeros and lengths
        t = ds.depth_region_quantiles(regions_table(["MT", "chrQ", "MT"], [5, 5, 9], [9, 9, 5]), q_num=(1,))
        assert t.column("bases").to_pylist() == [5, 5, 0] and t.column("min").to_pylist() == [0, 0, None] and t.column("q_1_2").to_pylist() == [0, 0, None]
