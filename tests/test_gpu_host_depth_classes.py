"""-m gpu: Session.depth_quantize / depth_dist and the same two on a DepthStream (brh_depth_quantize, brh_depth_dist and their
push forms) on pyarrow tables, against the vectorised restatements of tests/depth_classes_oracle.py: the golden BAM-derived
reads in all four zero_based x end_exclusive forms, with and without a length table, with touched_only; and a stream after
two pushes, which stays usable."""
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
import depth_classes_oracle as dco  # noqa: E402
import depth_oracle as orc  # noqa: E402
import depth_per_base_oracle as pbo  # noqa: E402

pytestmark = pytest.mark.gpu

op = lambda n, c: (n << 4) | c
GOLDEN = pbo.golden()
CUTS = (0, 1, 4, 100, 200)                                  # mosdepth --quantize 0:1:4:100:200:


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


def restated(reads, lens, zero_based):
    """-> (steps, contigs in key order, pos_lo, key_hi, skip_pos0): the profile and the domain the host library takes"""
    if lens is not None:
        order = sorted(lens, key=lambda s: s.encode())
        kept = [r for r in reads if r[0] in lens]
        key_len = np.array([lens[n] for n in order], np.uint32)
        st = pbo.steps(len(order), key_len=key_len, **orc.pack_reads([(order.index(r[0]),) + tuple(r[1:]) for r in kept]))
        key_hi = np.where(key_len > 0, key_len - 1, 0).astype(np.uint32) if zero_based else key_len
        return st, order, (0 if zero_based else 1), key_hi, not zero_based
    order = sorted({r[0] for r in reads}, key=lambda s: s.encode())
    st = pbo.steps(len(order), **orc.pack_reads([(order.index(r[0]),) + tuple(r[1:]) for r in reads]))
    return st, order, 0, None, False


def dropped(order, lens, zero_based):
    """the keys of contigs of length 0 when zero_based: [0, -1] is no domain, and key_hi alone cannot say so"""
    return [k for k, n in enumerate(order) if lens is not None and zero_based and lens[n] == 0]


def check_quantize(t, reads, lens, zero_based, end_exclusive, touched_only, cuts, mask=None):
    st, order, pos_lo, key_hi, skip = restated(reads, lens, zero_based)
    k, s, e, c = dco.quantize_steps(st, cuts, mask, pos_lo, key_hi, skip, touched_only)
    keep = ~np.isin(k, dropped(order, lens, zero_based))
    k, s, e, c = k[keep], s[keep], e[keep], c[keep]
    assert t.schema.names == ["contig", "start", "end", "bin"]
    assert [t.schema.field(i).type for i in range(4)] == [pa.string(), pa.int64(), pa.int64(), pa.int32()]
    assert all(t.column(i).null_count == 0 for i in range(4))
    assert t.column("contig").to_pylist() == [order[x] for x in k]
    assert np.array_equal(t.column("start").to_numpy(), s.astype(np.int64))
    assert np.array_equal(t.column("end").to_numpy(), e.astype(np.int64) + int(end_exclusive))
    assert np.array_equal(t.column("bin").to_numpy(), c.astype(np.int32))
    return len(k)


def check_dist(t, reads, lens, zero_based, touched_only, v_lo, n_bins):
    st, order, pos_lo, key_hi, skip = restated(reads, lens, zero_based)
    h = dco.hist_steps(st, v_lo, n_bins, pos_lo, key_hi, skip, touched_only)
    h[dropped(order, lens, zero_based)] = 0
    k, b = np.nonzero(h)
    assert t.schema.names == ["contig", "coverage", "bases"]
    assert [t.schema.field(i).type for i in range(3)] == [pa.string(), pa.int32(), pa.int64()]
    assert t.column("contig").to_pylist() == [order[x] for x in k]
    assert np.array_equal(t.column("coverage").to_numpy(), (v_lo + b).astype(np.int32))
    assert np.array_equal(t.column("bases").to_numpy(), h[k, b])
    return h


def ovl_reads(shift):
    case = next(c for c in orc.golden_cases() if c["name"] == GOLDEN["ovl_bam"]["reads_case"])
    return [(r["contig"], r["pos"] + shift, r["flags"], r["mapq"], r["ops"]) for r in case["reads"]]


@pytest.mark.parametrize("touched_only", [False, True])
@pytest.mark.parametrize("with_lengths", [True, False])
@pytest.mark.parametrize("end_exclusive", [False, True])
@pytest.mark.parametrize("zero_based", [True, False])
def test_ovl_bam(sess, zero_based, end_exclusive, with_lengths, touched_only):
    g = GOLDEN["ovl_bam"]
    reads = ovl_reads(0 if zero_based else 1)
    lens = {g["contig"]: g["length"], "GL000207.1": 4262, "empty": 0} if with_lengths else None
    L = lengths_table(lens) if with_lengths else None
    kw = dict(lengths=L, zero_based=zero_based, touched_only=touched_only)
    t = sess.depth_quantize(reads_table(reads), CUTS, end_exclusive=end_exclusive, **kw)
    assert check_quantize(t, reads, lens, zero_based, end_exclusive, touched_only, CUTS) >= 2    # (covered and not covered)
    if with_lengths:                                        # a contig without reads is one run of bin 1, unless only touched ones go out
        assert ("GL000207.1" in t.column("contig").to_pylist()) == (not touched_only)
        assert "empty" not in t.column("contig").to_pylist()           # a contig of length 0 has no position
    t = sess.depth_quantize(reads_table(reads), (2,), emit=(1,), end_exclusive=end_exclusive, **kw)     # "the intervals at 2x or more"
    check_quantize(t, reads, lens, zero_based, end_exclusive, touched_only, (2,), 0b10)
    assert set(t.column("bin").to_pylist()) == {1}
    for v_lo, n_bins in ((0, 256), (1, 2), (-2, 4)):
        h = check_dist(sess.depth_dist(reads_table(reads), v_lo, n_bins, **kw), reads, lens, zero_based, touched_only, v_lo, n_bins)
    if with_lengths:
        assert h[sorted(lens, key=lambda s: s.encode()).index(g["contig"])].sum() == g["length"]


def test_errors(sess):
    reads = reads_table([("a", 5, 0, 60, [op(10, 0)])])
    with pytest.raises(br.BioRangesError, match="cuts not strictly ascending"):
        sess.depth_quantize(reads, (3, 3))
    with pytest.raises(br.BioRangesError, match="more than 31 cuts"):
        sess.depth_quantize(reads, range(32))
    with pytest.raises(br.BioRangesError, match="emit_mask"):
        sess.depth_quantize(reads, (1,), emit=(2,))
    with pytest.raises(br.BioRangesError, match="n_bins"):
        sess.depth_dist(reads, 0, 0)
    with pytest.raises(br.BioRangesError, match="n_bins"):
        sess.depth_dist(reads, 0, 65537)
    t = sess.depth_quantize(reads_table([]), (1,))          # no reads, no contig: no rows
    assert t.num_rows == 0 and t.schema.names == ["contig", "start", "end", "bin"]
    assert sess.depth_dist(reads_table([]), 0, 4).num_rows == 0


@pytest.mark.parametrize("dense", [True, False])
def test_stream_after_two_pushes_and_still_usable(sess, dense):
    rng = np.random.default_rng(77 + dense)
    names = ["MT", "2", "10", "chrX"]
    lens = {"chrX": 300, "MT": 450, "2": 130, "10": 259, "unplaced": 50} if dense else None
    mk = lambda n: [(str(rng.choice(names)), int(rng.integers(1, 400)), int(rng.choice([0, 0, 4])), 60,
                     [op(int(rng.integers(1, 30)), int(rng.choice([0, 0, 2, 7]))) for _ in range(int(rng.integers(1, 4)))]) for _ in range(n)]
    batches = [mk(150), mk(20), mk(90)]
    L = lengths_table(lens) if dense else None
    cuts = (1, 3, 8)
    with sess.depth_stream(lengths=L) as ds:
        for b in batches[:2]:
            ds.push(reads_table(b))
        two = batches[0] + batches[1]
        for zero_based in (False, True):
            for end_exclusive in (False, True):
                for touched in (False, True):
                    t = ds.depth_quantize(cuts, zero_based=zero_based, end_exclusive=end_exclusive, touched_only=touched)
                    check_quantize(t, two, lens, zero_based, end_exclusive, touched, cuts)
                    assert t.equals(sess.depth_quantize(reads_table(two), cuts, lengths=L, zero_based=zero_based, end_exclusive=end_exclusive,
                                                        touched_only=touched))
            t = ds.depth_dist(-1, 12, zero_based=zero_based)
            check_dist(t, two, lens, zero_based, False, -1, 12)
            assert t.equals(sess.depth_dist(reads_table(two), -1, 12, lengths=L, zero_based=zero_based))
        t = ds.depth_quantize(cuts, emit=(0, 3))
        check_quantize(t, two, lens, False, False, False, cuts, 0b1001)
        assert t.equals(ds.depth_quantize(cuts, emit=(0, 3)))                   # asking again changes nothing
        ds.push(reads_table(batches[2]))                                        # the stream still takes a push ...
        allr = two + batches[2]
        check_quantize(ds.depth_quantize(cuts), allr, lens, False, False, False, cuts)
        check_dist(ds.depth_dist(0, 256, touched_only=True), allr, lens, False, True, 0, 256)
        assert ds.finish().equals(sess.depth(reads_table(allr), lengths=L))     # ... and finishes to the blocks it always gave
        with pytest.raises(br.BioRangesError, match="depth stream: already finished"):
            ds.depth_quantize(cuts)
        with pytest.raises(br.BioRangesError, match="depth stream: already finished"):
            ds.depth_dist()
    with sess.depth_stream(lengths=L) as ds:                                    # nothing pushed: every contig of the table at depth 0
        t = ds.depth_dist(0, 4, zero_based=True)
        if dense:
            order = sorted(lens, key=lambda s: s.encode())
            assert t.column("contig").to_pylist() == order and t.column("coverage").to_pylist() == [0] * 5
            assert t.column("bases").to_pylist() == [lens[n] for n in order]
            assert ds.depth_quantize((1,), touched_only=True).num_rows == 0
        else:
            assert t.num_rows == 0
