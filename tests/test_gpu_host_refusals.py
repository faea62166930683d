"""-m gpu: the host library (bio_ranges.Session) when a device reservation is refused in the middle of an operator.  Each
operator is a sequence of several C calls with an index or a depth profile held in between; the session's memory limit is
stepped across all of them by the refusal's own text ("failed to reserve B bytes ... (R bytes reserved, limit L)": the next
limit is R + B), a fresh Session per step, as tests/test_gpu_entry_refusals.py does for the single calls.

At every refusal, on the same session: the error is BioRangesError "Resources exhausted: failed to reserve N bytes"; the
operator refused twice more at the same limit holds no more reserved bytes after the third refusal than after the second (an
index or profile left alive by the error path would add its bytes each time); with the limit off the operator then gives what
a session that never had a limit gives.  The walk ends when the operator runs through under the limit, with the same answer.
"""
import os
import re
import struct
import sys

import numpy as np
import pyarrow as pa
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import bio_ranges as br  # noqa: E402

pytestmark = pytest.mark.gpu

TEXT = re.compile(r"Resources exhausted: failed to reserve (\d+) bytes (?:of device scratch|for the index) "
                  r"\((\d+) bytes reserved, limit (\d+)\)")
MAX_ATTEMPTS = 256
CONTIGS = ["chr1", "chr10", "chr2"]


def intervals(n, seed, mean_len=300, extra=None):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 400_000, n)
    cols = {"contig": pa.array([CONTIGS[i] for i in rng.integers(0, 3, n)], pa.string()),
            "pos_start": pa.array(s, pa.int64()), "pos_end": pa.array(s + rng.integers(0, 2 * mean_len, n), pa.int64())}
    if extra:
        cols[extra] = pa.array(rng.integers(-1000, 1000, n), pa.int32())
    return pa.table(cols)


def reads(n, seed):
    """n reads of 1..3 CIGAR ops (M, I, D, N, S), a tenth of them filtered by flag"""
    rng = np.random.default_rng(seed)
    cig = []
    for _ in range(n):
        ops = [(int(rng.integers(1, 60)) << 4) | int(rng.choice([0, 0, 0, 1, 2, 3, 4])) for _ in range(int(rng.integers(1, 4)))]
        cig.append(struct.pack("<%dI" % len(ops), *ops))
    return pa.table({"chrom": pa.array([CONTIGS[i] for i in rng.integers(0, 3, n)], pa.string()),
                     "start": pa.array(rng.integers(1, 20_000, n), pa.uint32()),
                     "flags": pa.array(np.where(rng.random(n) < 0.1, 4, 0), pa.uint32()), "cigar": pa.array(cig, pa.binary()),
                     "mapping_quality": pa.array(rng.integers(0, 61, n), pa.uint32())})


def pairs(res):
    b, p = res
    return np.sort((b.to_numpy().astype(np.uint64) << np.uint64(32)) | p.to_numpy().astype(np.uint64))


A, B = intervals(3000, 1, extra="score"), intervals(4000, 2)
R = reads(3000, 3)
REGIONS = intervals(500, 4, mean_len=40)
REGIONS = REGIONS.set_column(1, "pos_start", pa.array(REGIONS.column("pos_start").to_numpy() % 20_000 + 1, pa.int64()))
REGIONS = REGIONS.set_column(2, "pos_end", pa.array(REGIONS.column("pos_start").to_numpy() + 50, pa.int64()))

# operator -> (call on a session, canonical form of its result)
OPS = {
    "interval_join": (lambda s: s.interval_join(A, B), pairs),
    "overlap_aggregate": (lambda s: s.overlap_aggregate(A, B, "score"), None),
    "intersect": (lambda s: s.intersect(A, B), None),
    "subtract": (lambda s: s.subtract(A, B), None),
    "merge": (lambda s: s.merge(A.select(["contig", "pos_start", "pos_end"])), None),
    "depth": (lambda s: s.depth(R), None),
    "depth_regions": (lambda s: s.depth_regions(R, REGIONS, thresholds=(1, 5)), None),
    "depth_quantize": (lambda s: s.depth_quantize(R, (1, 3, 10)), None),
}


def same(got, want, canon):
    if canon is not None:
        return np.array_equal(canon(got), canon(want))
    return got.schema == want.schema and got.equals(want)


@pytest.mark.parametrize("op", sorted(OPS))
def test_refused_reservation_in_a_host_operator(op):
    call, canon = OPS[op]
    free = br.Session(0)
    try:
        want = call(free)
    finally:
        free.close()
    limit, points = 1, 0                            # (0 would mean no limit)
    for attempt in range(MAX_ATTEMPTS + 1):
        assert attempt < MAX_ATTEMPTS, (op, limit)
        s = br.Session(0)
        try:
            s.set_memory_limit(limit)
            try:
                got = call(s)
            except br.BioRangesError as ex:
                m = TEXT.search(str(ex))
                assert m and re.search(r"Resources exhausted: failed to reserve \d+ bytes", str(ex)), str(ex)
                b, r, lim = map(int, m.groups())
                assert lim == limit and r + b > limit, (op, str(ex))
                points += 1
                held = []
                for _ in range(2):                  # the same refusal twice more
                    with pytest.raises(br.BioRangesError, match=r"Resources exhausted: failed to reserve \d+ bytes"):
                        call(s)
                    held.append(s.reserved_bytes())
                assert held[1] <= held[0], (op, limit, held)
                s.set_memory_limit(0)
                assert same(call(s), want, canon), (op, "after the refusal at", limit)
                limit = r + b
                continue
            assert same(got, want, canon), (op, "under the tightest limit", limit)
            break
        finally:
            s.close()
    print(f"HOST_REFUSAL_POINTS {op} {points}")
    assert points > 0
