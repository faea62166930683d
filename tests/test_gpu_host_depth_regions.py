"""-m gpu: Session.depth_regions / DepthStream.depth_regions (brh_depth_regions, brh_depth_push_regions) on pyarrow tables:
the reference's pinned per-base tables summed over regions in both coordinate systems, every position and contig type,
sliced region arrays, half-open ends, unknown contigs, the NULL coordinate error, and the stream form."""
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
import depth_per_base_oracle as pbo  # noqa: E402
import depth_regions_oracle as dro  # noqa: E402

pytestmark = pytest.mark.gpu

op = lambda n, c: (n << 4) | c
GOLDEN = pbo.golden()


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


def blocks_table(rows):
    return pa.table({"contig": pa.array([r[0] for r in rows], pa.string()), "pos_start": pa.array([r[1] for r in rows], pa.int32()),
                     "pos_end": pa.array([r[2] for r in rows], pa.int32()), "coverage": pa.array([r[3] for r in rows], pa.int16())})


def lengths_table(d):
    return pa.table({"name": pa.array(list(d), pa.string()), "length": pa.array(list(d.values()), pa.int64())})


def regions_table(contig, s, e, pos_type=pa.int64(), contig_type=pa.string()):
    return pa.table({"contig": pa.array(contig, contig_type), "pos_start": pa.array(s, pos_type), "pos_end": pa.array(e, pos_type)})


def cols_of(t, thr):
    assert t.schema.names[3:] == ["bases", "sum"] + [f"bases_ge_{x}" for x in thr]
    for name in t.schema.names[3:]:
        assert t.schema.field(name).type == pa.int64() and t.column(name).null_count == 0
    return [t.column(n).to_numpy() for n in t.schema.names[3:]]


def rows_regions(L, first, rng):
    """the whole contig, every single position (a sample of a long contig), seeded spans; closed, inside [first, first + L)"""
    allp = first + np.arange(L)
    if L > 300:
        allp = np.unique(np.concatenate([allp[:60], allp[-60:], first + rng.integers(0, L, 80)]))
    a, b = first + rng.integers(0, L, 30), first + rng.integers(0, L, 30)
    return np.concatenate([[first], allp, np.minimum(a, b)]), np.concatenate([[first + L - 1], allp, np.maximum(a, b)])


def check_rows(got, s, e, pos, cov, thr):
    """the summary columns against sums of the per-base rows (pos int32 ascending by 1, cov int16)"""
    c = cov.astype(np.int64)
    for i in range(len(s)):
        w = c[int(s[i]) - int(pos[0]): int(e[i]) - int(pos[0]) + 1]
        assert got[0][i] == len(w) and got[1][i] == w.sum()
        for j, t in enumerate(thr):
            assert got[2 + j][i] == (w >= t).sum()


# ---------------------------------------------------------------------------------------------- the golden per-base cases
@pytest.mark.parametrize("zero_based", [True, False])
@pytest.mark.parametrize("case", GOLDEN["emitter"], ids=lambda c: c["name"])
def test_emitter_tables(sess, case, zero_based):
    L = case["depth_len"] - 1
    run, rows, last = 0, [], 0
    deltas = dict((i, d) for i, d in case["depth"])
    for i in range(case["depth_len"]):                      # the delta array as prior blocks, as tests/test_gpu_host_depth_per_base.py
        if i in deltas:
            if run:
                rows.append(("chr1", last, i - 1, run))
            run += deltas[i]
            last = i
    depth = [0] * case["depth_len"]
    for i, d in case["depth"]:
        depth[i] = d
    pos, cov = pbo.emit_dense(depth, zero_based)
    if zero_based == case["zero_based"]:
        for row, c in case["expect"]["coverage"]:
            assert int(cov[row]) == c
    thr = (1, 2, -1)
    s, e = rows_regions(L, 0 if zero_based else 1, np.random.default_rng(L))
    t = sess.depth_regions(reads_table([]), regions_table(["chr1"] * len(s), s, e), prior=blocks_table(rows), lengths=lengths_table({"chr1": L}),
                           zero_based=zero_based, thresholds=thr)
    check_rows(cols_of(t, thr), s, e, pos, cov, thr)


def ovl_reads(shift):
    case = next(c for c in orc.golden_cases() if c["name"] == GOLDEN["ovl_bam"]["reads_case"])
    return [(r["contig"], r["pos"] + shift, r["flags"], r["mapq"], r["ops"]) for r in case["reads"]]


def ovl_rows(zero_based):
    g = GOLDEN["ovl_bam"]
    case = next(c for c in orc.golden_cases() if c["name"] == g["reads_case"])
    names, kw = orc.case_columns(case)
    kw["key_len"] = np.array([g["length"]], np.uint32)
    if not zero_based:
        kw["rpos"] = kw["rpos"] + np.uint32(1)
    pos, cov = pbo.per_base_dense(zero_based, 1, **kw)[0]
    for row, c in g["zero_based" if zero_based else "one_based"]["coverage"]:
        assert int(cov[row]) == c
    return pos, cov


@pytest.mark.parametrize("zero_based", [True, False])
def test_ovl_bam(sess, zero_based):
    g = GOLDEN["ovl_bam"]
    pos, cov = ovl_rows(zero_based)
    first = 0 if zero_based else 1
    s, e = rows_regions(g["length"], first, np.random.default_rng(2))
    lengths = lengths_table({g["contig"]: g["length"], "GL000207.1": 4262})
    thr = (1, 2, 3)
    t = sess.depth_regions(reads_table(ovl_reads(first)), regions_table([g["contig"]] * len(s), s, e), lengths=lengths, zero_based=zero_based, thresholds=thr)
    got = cols_of(t, thr)
    check_rows(got, s, e, pos, cov, thr)
    assert t.column("contig").to_pylist() == [g["contig"]] * len(s) and np.array_equal(t.column("pos_start").to_numpy(), s)
    # a region is cut to the positions the per-base rows have; a contig of the table without reads has coverage 0
    t = sess.depth_regions(reads_table(ovl_reads(first)), regions_table([g["contig"], g["contig"], "GL000207.1"], [0, g["length"] + 5, 0], [10 ** 6, 10 ** 6, 10 ** 6]),
                           lengths=lengths, zero_based=zero_based, thresholds=(0, 1))
    got = cols_of(t, (0, 1))
    assert got[0].tolist() == [g["length"], 0, 4262] and got[1].tolist() == [int(cov.astype(np.int64).sum()), 0, 0]
    assert got[2].tolist() == [g["length"], 0, 4262] and got[3].tolist() == [int((cov >= 1).sum()), 0, 0]


# ---------------------------------------------------------------------------------------------- column types
@pytest.fixture(scope="module")
def ovl_one_based():
    return ovl_rows(False)


@pytest.mark.parametrize("pos_type", [pa.int32(), pa.int64(), pa.uint32(), pa.uint64()], ids=str)
@pytest.mark.parametrize("contig_type", [pa.string(), pa.large_string(), pa.string_view()], ids=str)
def test_position_and_contig_types_sliced(sess, ovl_one_based, pos_type, contig_type):
    g = GOLDEN["ovl_bam"]
    pos, cov = ovl_one_based
    s, e = rows_regions(g["length"], 1, np.random.default_rng(4))
    pad = 3                                                 # rows in front that the slice cuts away
    reg = regions_table(["nowhere"] * pad + [g["contig"]] * len(s), [7] * pad + list(s), [9] * pad + list(e), pos_type, contig_type).slice(pad)
    t = sess.depth_regions(reads_table(ovl_reads(1)), reg, lengths=lengths_table({g["contig"]: g["length"]}), thresholds=(2,))
    check_rows(cols_of(t, (2,)), s, e, pos, cov, (2,))


def test_clamping_end_exclusive_and_unknown_contigs(sess, ovl_one_based):
    g = GOLDEN["ovl_bam"]
    pos, cov = ovl_one_based
    c64 = cov.astype(np.int64)
    reads, lengths = reads_table(ovl_reads(1)), lengths_table({g["contig"]: g["length"]})
    # values outside [0, 2^32 - 1] are clamped
    reg = regions_table([g["contig"]] * 2, [-5, 1], [40, 1 << 40])
    got = cols_of(sess.depth_regions(reads, reg, lengths=lengths, thresholds=(1,)), (1,))
    assert got[0].tolist() == [40, g["length"]] and got[1].tolist() == [int(c64[:40].sum()), int(c64.sum())]
    reg = regions_table([g["contig"]], [3], [(1 << 64) - 1], pa.uint64())
    assert cols_of(sess.depth_regions(reads, reg, lengths=lengths), ())[0].tolist() == [g["length"] - 2]
    # half-open ends
    s, e = rows_regions(g["length"], 1, np.random.default_rng(6))
    reg = regions_table([g["contig"]] * (len(s) + 2), list(s) + [5, 9], list(e + 1) + [5, 2])
    got = cols_of(sess.depth_regions(reads, reg, lengths=lengths, end_exclusive=True, thresholds=(1, 2)), (1, 2))
    check_rows([x[:len(s)] for x in got], s, e, pos, cov, (1, 2))
    assert all(x[len(s):].tolist() == [0, 0] for x in got)          # end <= start: empty
    # a contig the dictionary lacks: coverage 0 everywhere, with and without a length table; a NULL contig likewise
    reg = regions_table(["chrZ", None, g["contig"], "chrZ"], [10, 1, 1, 9], [19, 4, 6, 3])
    for L in (lengths, None):
        got = cols_of(sess.depth_regions(reads, reg, lengths=L, thresholds=(0, 1)), (0, 1))
        assert got[0].tolist() == [10, 4, 6, 0] and got[1].tolist() == [0, 0, int(c64[:6].sum()), 0]
        assert got[2].tolist() == [10, 4, 6, 0] and got[3].tolist() == [0, 0, int((c64[:6] >= 1).sum()), 0]


def test_sparse_mode_matches_the_restatement(sess):
    rng = np.random.default_rng(12)
    names = ["MT", "2", "10"]
    order = sorted(names, key=lambda s: s.encode())
    reads = [(str(rng.choice(names)), int(rng.integers(0, 400)), int(rng.choice([0, 0, 4])), 60,
              [op(int(rng.integers(1, 30)), int(rng.choice([0, 0, 2, 3, 7]))) for _ in range(int(rng.integers(1, 4)))]) for _ in range(200)]
    st = pbo.steps(3, **orc.pack_reads([(order.index(r[0]),) + r[1:] for r in reads]))
    n = 120
    qk = rng.integers(0, 3, n)
    qs = rng.integers(0, 500, n)
    qe = qs + rng.integers(0, 300, n)
    thr = (1, 3, 5, 0)
    want = dro.summarize_loop(st, qk.astype(np.uint32), qs.astype(np.uint32), qe.astype(np.uint32), thr)
    t = sess.depth_regions(reads_table(reads), regions_table([order[k] for k in qk], qs, qe), thresholds=thr)
    got = cols_of(t, thr)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(np.stack(got[2:]), want[2])


def test_errors(sess):
    reads = reads_table([("a", 5, 0, 60, [op(10, 0)])])
    reg = regions_table(["a", "a"], [1, None], [9, 9])
    with pytest.raises(br.BioRangesError, match="coordinate column contains null values"):
        sess.depth_regions(reads, reg)
    reg = regions_table(["a"], [1], [9])
    with pytest.raises(br.BioRangesError, match="more than 8 thresholds"):
        sess.depth_regions(reads, reg, thresholds=range(9))
    with pytest.raises(br.BioRangesError, match="not found"):
        sess.depth_regions(reads, reg, cols=("contig", "from", "pos_end"))
    bad = pa.table({"contig": pa.array(["a"]), "pos_start": pa.array([1.0]), "pos_end": pa.array([9])})
    with pytest.raises(br.BioRangesError, match="unsupported data type"):
        sess.depth_regions(reads, bad)
    t = sess.depth_regions(reads, reg.slice(0, 0), thresholds=(1,))         # no regions: empty columns
    assert t.num_rows == 0 and t.schema.names[3:] == ["bases", "sum", "bases_ge_1"]


# ---------------------------------------------------------------------------------------------- the stream
@pytest.mark.parametrize("dense", [True, False])
def test_stream_equals_the_one_shot_call_and_stays_open(sess, dense):
    rng = np.random.default_rng(31 + dense)
    names = ["MT", "2", "10", "chrX"]
    lens = {"chrX": 300, "MT": 450, "2": 130, "10": 259}
    mk = lambda n: [(str(rng.choice(names)), int(rng.integers(1, 400)), int(rng.choice([0, 0, 4])), 60,
                     [op(int(rng.integers(1, 30)), int(rng.choice([0, 0, 2, 7]))) for _ in range(int(rng.integers(1, 4)))]) for _ in range(n)]
    batches = [mk(150), mk(20), mk(90)]
    L = lengths_table(lens) if dense else None
    n = 150
    reg = regions_table([str(x) for x in rng.choice(names + ["chrQ"], n)], rng.integers(0, 300, n), rng.integers(100, 600, n))
    thr = (1, 10, 20)
    kw = dict(thresholds=thr, zero_based=False, end_exclusive=True)
    with sess.depth_stream(lengths=L) as ds:
        for b in batches[:2]:
            ds.push(reads_table(b))
        two = ds.depth_regions(reg, **kw)
        assert two.equals(sess.depth_regions(reads_table(batches[0] + batches[1]), reg, lengths=L, **kw))
        assert two.equals(ds.depth_regions(reg, **kw))                      # asking again changes nothing
        ds.push(reads_table(batches[2]))                                    # the stream still takes a push ...
        three = ds.depth_regions(reg, **kw)
        allr = reads_table(batches[0] + batches[1] + batches[2])
        assert three.equals(sess.depth_regions(allr, reg, lengths=L, **kw)) and not three.equals(two)
        assert ds.finish().equals(sess.depth(allr, lengths=L))              # ... and finishes to the blocks it always gave
        with pytest.raises(br.BioRangesError, match="depth stream: already finished"):
            ds.depth_regions(reg, **kw)
    with sess.depth_stream(lengths=L) as ds:                                # nothing pushed: zeros and lengths
        got = cols_of(ds.depth_regions(regions_table(["MT", "chrQ"], [5, 5], [9, 9]), thresholds=(0, 1)), (0, 1))
        assert got[0].tolist() == [5, 5] and got[1].tolist() == [0, 0] and got[2].tolist() == [5, 5] and got[3].tolist() == [0, 0]
