"""-m gpu: IVX_MEM_DEVICE calls with their inputs still in flight on the caller's stream and their outputs consumed by work
queued behind them, no host synchronisation in between -- what include/ivx.h promises of a device-mode call ("kernels run on
the ctx stream", "may return with kernels in flight") and what bench.py, sharded.py and a DataFusion caller rely on.

The harness is entry_cases.LateMode: before every entry the caller's stream gets zero bytes (a valid column of every case: key
0, position 0, offset 0, row 0, empty strings) into every buffer, one delay, the copies of the real contents and an event
`ready`; the entry is invoked at once; clones of its outputs are queued right behind it.  A kernel, memset or scalar fetch on
another stream, a build tail or probe kernel that misses its event edge, or an output written early computes from the zeros or
is covered by the output's pattern: the result differs from host mode.  Every call asserts that `ready` had NOT happened when
the entry was invoked -- otherwise the call proves nothing and fails as inconclusive.

1. Every catalogue case (one per C entry) at 1000, 0 and 1 rows on a torch stream, and at 1000 rows on HIP's default stream.
2. Teeth: ivx_probe_count and ivx_merge with the context left on its own stream while the producers run on another -- the
   caller's error the contract excludes.  The call returns before `ready` and the result differs from host mode.
3. The shapes where the library uses its second stream, a plan kept from a count call, or many launches and host round
   trips: the overlapped join build (70 000 build rows, 300 000 probe rows on the region path; a fill, a count and its planned
   fill, ivx_index_layout and a fill, a probe from ANOTHER context on its own stream -- ivx_index_build has waited for its
   stream when it returns and everything behind that is ordered by the index's `ready` event, which every probe waits for);
   the per-row family on the routed paths at 100 000 rows; the sweeps at 200 000 int64 rows; depth at 5 * 1024 + 3 CIGAR ops
   and every read-out of a merged profile.
Expected values: the same calls in host mode on a plain context on its own stream, computed once.

Measured on an MI355X (printed when the module's fixture is torn down, -s):
  torch.cuda._sleep: 2 400 038 cycles per ms (a delay of 10 ms asked for took 10.01 ms; the chain of fills was not needed).
  Host time between queuing the delay and invoking the entry: calibrated 20 us + 2.9 us a buffer (the slowest of 20 runs);
  over the module's 350 late calls, median 33 us, max 244 us.  Delays: 100 times the calibrated time, at least 10 ms -- 10 ms
  for every call but the teeth check's 60 ms, 3.72 s in all; delay / measured host time: median some 300, least 84 (the
  calibration, not each call's own time, is what the factor 100 applies to; the assertion on `ready` is what holds per
  call, and it held on all 350).  94 of the calls returned with their producer still running.  Module wall time 4.6 s
  (6.9 s with pytest's start-up), 169 tests.  No mis-ordered launch was found.
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import entry_cases as ec  # noqa: E402
from entry_cases import CASES, NK, OK, SIZES, Delay, Env, LateMode, Mode, _same, cint, pyivx, shaped, u32, u64  # noqa: E402
from test_gpu_entry_state import LOCAL_CASES, designed, inside  # noqa: E402
from test_gpu_region_forms import env  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = sorted(CASES)
TEETH_MS = 60.0                     # the teeth check's delay: an entry's whole call has to fit into it


# ------------------------------------------------------------------ set-up, once per module

class World:
    """the stream S, the Env whose context runs on it, the plain Env (the module's one extra context) that gives the
    host-mode expectations, the calibrated delay"""

    def __init__(self):
        import torch
        self.S = torch.cuda.Stream()
        self.default = torch.cuda.default_stream()
        self.L = Env(designed(), stream=self.S)
        self.H = Env(designed())
        self.delay = Delay(self.S)
        self.want = {}

    def host(self, key, run):
        """run(E, M) in host mode on the plain context, once per key"""
        if key not in self.want:
            self.want[key] = run(self.H, Mode(False))
        return self.want[key]

    def late(self, run, stream=None, ms=None):
        """run(E, M) in late mode -> (result, the mode)"""
        with LateMode(self.L, stream or self.S, self.delay, ms) as M:
            got = run(self.L, M)
        assert M.calls, "no entry was called"
        return got, M

    def on_default_stream(self):
        return _Switched(self, lambda: self.L.ctx.set_stream(None))

    def on_own_stream(self):
        return _Switched(self, self.L.ctx.use_own_stream)


class _Switched:
    def __init__(self, w, switch):
        self.w, self.switch = w, switch

    def __enter__(self):
        self.switch()

    def __exit__(self, *exc):
        self.w.L.ctx.synchronize()
        self.w.L.ctx.set_stream(self.w.S.cuda_stream)


@pytest.fixture(scope="module")
def W():
    w = World()
    # the forced paths of part 3 can be taken, or the library would answer with the direct kernels and say nothing
    # (test_gpu_entry_state.py's fixture E has the reasons)
    for e in (w.L, w.H):
        lay = e.ix[0].layout()
        assert lay["nreg"] > 1 and lay["slow"] == 0, lay
        for kind in (pyivx.KIND_COUNT, pyivx.KIND_COVERAGE):
            assert 0 < e.ix[kind].layout()["nreg"] <= 1023
        assert e.ix[pyivx.KIND_NEAREST].forms()["nroute_nreg"] > 0
    t0 = time.perf_counter()
    yield w
    w.L.close()
    w.H.close()
    # the figures of the module's docstring (shown with -s)
    log, d = w.delay.log, w.delay
    if log:
        host_us, ms = np.array([t for _, _, t, _ in log]) * 1e6, np.array([m for *_, m in log])
        print(f"\nlate calls {len(log)}, {d.n_early} of them returned with the producer still running; _sleep cycles per ms {d.cycles_per_ms:.0f} (a 10 ms delay took {d.check_ms:.2f} ms; fills of "
              f"{d.ms_per_fill:.3f} ms instead: {d.big is not None}); host time queue-to-invoke: calibrated {d.host_base * 1e6:.0f} us + "
              f"{d.host_per_buf * 1e6:.1f} us a buffer, measured median {np.median(host_us):.0f} us, max {host_us.max():.0f} us; delays "
              f"{ms.min():.1f} .. {ms.max():.1f} ms, {ms.sum() / 1e3:.2f} s in all; least delay / host time {np.min(ms * 1e3 / host_us):.0f}; "
              f"module wall time {time.perf_counter() - t0:.1f} s")


def assert_equal(got, want, what):
    got = {k: (v.cpu().numpy().view(want[k].dtype) if pyivx._is_torch(v) else v) for k, v in got.items()}
    assert sorted(got) == sorted(want), what
    assert all(want[k] == OK for k in ("st", "st0", "st1", "st2") if k in want), what
    diff = [k for k in want if not _same(want[k], got[k])]
    assert not diff, (what, {k: (want[k], got[k]) for k in diff[:3]})


# ------------------------------------------------------------------ 1. the catalogue, late

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_late_inputs_equal_host_mode(W, name, n):
    want = W.host((name, n), lambda E, M: CASES[name](E, M, n))
    got, _ = W.late(lambda E, M: CASES[name](E, M, n))
    assert_equal(got, want, (name, n))


@pytest.mark.parametrize("name", NAMES)
def test_late_inputs_on_the_default_stream(W, name):
    """the context on HIP's default stream (ivx_ctx_set_stream(ctx, NULL)), the producers on torch's default stream"""
    n = SIZES[0]
    want = W.host((name, n), lambda E, M: CASES[name](E, M, n))
    with W.on_default_stream():
        got, _ = W.late(lambda E, M: CASES[name](E, M, n), stream=W.default)
    assert_equal(got, want, (name, "default stream"))


# ------------------------------------------------------------------ 2. the walk has teeth

@pytest.mark.parametrize("name", ["probe_count", "merge"])
def test_a_context_on_another_stream_is_noticed(W, name):
    """the producers on S, the context on its own stream: nothing orders the entry's kernels behind the columns.  They read
    the zero columns (valid ones: a wrong answer, never a wrong address) and their outputs are covered by the pattern"""
    n = SIZES[0]
    want = W.host((name, n), lambda E, M: CASES[name](E, M, n))
    with W.on_own_stream():
        got, M = W.late(lambda E, M: CASES[name](E, M, n), ms=TEETH_MS)
    assert all(M.early), f"inconclusive: a call took longer than the {TEETH_MS} ms of delay ({M.calls})"
    assert any(not _same(want[k], got[k]) for k in want), "a context on the wrong stream gave host mode's result"


# ------------------------------------------------------------------ 3a. the overlapped join build

NB, NP = 70_000, 300_000            # the build overlap needs 2^16 build rows (ivx_join.hip: ivx_join_build)
JOIN_BUILD = designed(NB)
JOIN_PROBE = inside(JOIN_BUILD, NP, 81)
JOIN_CAP = 8 * NP                   # build rows of 256 every 64, probe rows under 100 long: at most 7 pairs a row


def join_sequence(seq, overlap, other=None):
    """late build columns -> ivx_index_build (nothing waited for behind it: its tail may still run) -> `seq`:
         fill    late probe columns -> ivx_probe_overlap_fill
         plan    late probe columns -> total-only count, which leaves the plan -> the fill on the same, now fixed, pointers
         layout  ivx_index_layout -> late probe columns -> fill
         other   the fill from the context `other` (an Env) on its own stream, device columns that were complete beforehand
    the build columns fixed from the build on, as the build overlap wants them"""
    def run(E, M):
        res = {}
        PE, PM = (E, M) if seq != "other" or not M.dev else (other, Mode(True))
        E.ctx.set_build_overlap(overlap)
        ix = None
        try:
            bk, bs, be = (M.put(a) for a in JOIN_BUILD)
            pk, ps, pe = (PM.put(a) for a in JOIN_PROBE)
            b, p = PM.out(JOIN_CAP, np.uint32), PM.out(JOIN_CAP, np.uint32)
            h = C.c_void_p(0xDEAD)
            st = E.call("ivx_index_build", cint(0), M.mem, bk.p, bs.p, be.p, u64(NB), u32(1), C.byref(h), handle=h, drain=False)
            assert st == OK, E.err()
            M.fixed(bk, bs, be)
            ix = pyivx.Index(E.ctx, h, pyivx.KIND_OVERLAP)
            if M.dev:
                assert E.ctx.debug_state()["tail_pending"] == int(overlap)
            if seq == "layout":
                words = (C.c_uint32 * len(pyivx.LAYOUT_SLOTS))()
                assert E.call("ivx_index_layout", ix.h, words, u32(len(words))) == OK
                res["layout"] = list(words)
                assert res["layout"][pyivx.LAYOUT_SLOTS.index("nreg")] > 1, res["layout"]     # the region path exists
            if seq == "plan":
                tot = u64(0xDEAD)
                fills = E.ctx.debug_state()["join_fills_planned"]
                res["st0"] = PE.call("ivx_probe_overlap_count", ix.h, PM.mem, pk.p, ps.p, pe.p, u64(NP), None, C.byref(tot), count=tot)
                res["count"] = tot.value
                assert E.ctx.debug_state()["join_valid"] == 1
                PM.fixed(pk, ps, pe)
            w = u64(0xDEAD)
            res["st"] = PE.call("ivx_probe_overlap_fill", ix.h, PM.mem, pk.p, ps.p, pe.p, u64(NP), b.p, p.p, u64(JOIN_CAP), C.byref(w),
                                outs=[b, p], count=w)
            if seq == "plan":
                assert E.ctx.debug_state()["join_fills_planned"] == fills + 1     # the plan served the fill
            m = res["total"] = w.value
            assert 0 < m <= JOIN_CAP
            res["pairs"] = np.sort((b.np()[:m].astype(np.uint64) << np.uint64(32)) | p.np()[:m].astype(np.uint64))
        finally:
            E.ctx.set_build_overlap(False)
            E.ctx.synchronize()
            PE.ctx.synchronize()
            if ix is not None:
                ix.free()
        return res
    return run


@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "serial"])
@pytest.mark.parametrize("seq", ["fill", "plan", "layout", "other"])
def test_late_join_build_sequences(W, seq, overlap):
    with env(IVX_JOIN_PATH="regions"):
        want = W.host(("join", seq), join_sequence(seq, False))
        got, _ = W.late(join_sequence(seq, overlap, other=W.H))
    assert_equal(got, want, (seq, overlap))
    if seq == "plan":
        assert got["count"] == got["total"]


# ------------------------------------------------------------------ 3b. the per-row family on its routed paths

N_ROWS = 100_000
PER_ROW = [("probe_overlap_count", {"IVX_JOIN_PATH": "regions"}), ("probe_exists", {"IVX_JOIN_PATH": "regions"}),
           ("probe_mark_build", {"IVX_JOIN_PATH": "regions"}), ("probe_overlap_agg", {"IVX_JOIN_PATH": "regions"}),
           ("probe_count", {"IVX_ROWVAL_PATH": "regions"}), ("probe_coverage", {"IVX_ROWVAL_PATH": "regions"}),
           ("probe_nearest_k1", {"IVX_NEAREST_PATH": "routed"}),
           ("probe_overlap_select", {"IVX_JOIN_PATH": "regions"}), ("probe_overlap_count_where", {"IVX_JOIN_PATH": "regions"}),
           ("probe_mark_build_where", {"IVX_JOIN_PATH": "regions"}), ("probe_overlap_agg_where", {"IVX_JOIN_PATH": "regions"}),
           ("probe_overlap_select_where", {"IVX_JOIN_PATH": "regions"}), ("pairs_where", {"IVX_JOIN_PATH": "regions"}),
           ("probe_nearest_dir_k1", {"IVX_NEAREST_PATH": "routed"})]
NULL = pyivx.NULL_IDX
# name -> the rows (or words) of the host-mode result that say "this row met the build", of which more than half must: a
# probe that matched nothing would compare zeros with zeros.  spread_probes' rows are 1 .. 100 long and start inside a build row
# of 256 that reaches at least 192 further: every row lies inside a build row, and passes the cases' threshold (min_bases 10,
# half of the probe row) unless it is shorter than 10 -- nine rows in ten.  One-sided nearest rows without overlaps find the
# build row that ends (starts) within 64 coordinates of them when no cap is set.
MET = {
    "probe_overlap_count": lambda w: w["per_row"] != 0, "probe_exists": lambda w: w["exists"] != 0, "probe_mark_build": lambda w: w["marks"] != 0,
    "probe_overlap_agg": lambda w: w["count"] != 0, "probe_count": lambda w: w["out0"] != 0, "probe_coverage": lambda w: w["out0"] != 0,
    "probe_nearest_k1": lambda w: w["b"] != 0,
    "probe_overlap_select": lambda w: w["idx.max_val"] != NULL, "probe_overlap_count_where": lambda w: w["per_row"] != 0,
    "probe_mark_build_where": lambda w: w["marks"] != 0, "probe_overlap_agg_where": lambda w: w["agg.count"] != 0,
    "probe_overlap_select_where": lambda w: w["idx"] != NULL,
    "probe_nearest_dir_k1": lambda w: (w["before.ovl0.d-1.b"] != NULL) & (w["after.ovl0.d-1.d"] > 0),
}


def spread_probes(n, seed):
    """n short rows all over the Env's one-key build (200 000 rows, some 50 regions)"""
    return inside(designed(), n, seed)


@pytest.mark.parametrize("name,knobs", PER_ROW, ids=[n for n, _ in PER_ROW])
def test_late_per_row_family_routed(W, name, knobs):
    case = CASES.get(name) or LOCAL_CASES[name]
    with env(**knobs), shaped(cols=spread_probes):
        want = W.host(("rows", name), lambda E, M: case(E, M, N_ROWS))
        got, _ = W.late(lambda E, M: case(E, M, N_ROWS))
    assert_equal(got, want, name)
    assert all(v == OK for k, v in want.items() if k.startswith("st.") or k.endswith(".st")), name
    # the rows met the build: a probe that matched nothing would compare zeros with zeros
    if name == "pairs_where":
        # pair i is (build row i, probe row i), the probe rows anywhere: next to none of the pairs is a match at all.  What the
        # filter must return is worked out from the columns (the threshold of entry_cases._where, restated): the passing pairs,
        # in order -- and there are some, where the decoy's zero columns (pair (0, 0), one base long) give none
        bs, be = (c[:N_ROWS].astype(np.int64) for c in W.H.build_cols[1:])
        ps, pe = (c.astype(np.int64) for c in spread_probes(N_ROWS, 29)[1:])
        length = np.minimum(pe, be) - np.maximum(ps, bs) + 1
        keep = np.flatnonzero((length >= 10) & (2 * length >= pe - ps + 1)).astype(np.uint32)
        assert len(keep) > 0 and want["pairs.fill"] == (OK, len(keep)), (len(keep), want["pairs.fill"])
        assert (want["pairs.fill.0"] == keep).all() and (want["pairs.fill.1"] == keep).all()
        return
    met = MET[name](want)
    assert np.count_nonzero(met) > len(met) // 2, name


# ------------------------------------------------------------------ 3c. the sweeps

N_SWEEP = 200_000                   # several sort tiles and scan levels; 60 coordinates per row: many runs, gaps and pieces


@pytest.mark.parametrize("name", ["merge", "cluster", "subtract", "intersect", "complement"])
def test_late_sweeps(W, name):
    """the catalogue's case at 200 000 int64 rows: subtract, intersect and complement are a sizing call and its fill on the
    same late-filled pointers (subtract's six columns fixed in between: its plan serves the fill)"""
    with shaped(spread=60):
        want = W.host(("sweep", name), lambda E, M: CASES[name](E, M, N_SWEEP))
        got, M = W.late(lambda E, M: CASES[name](E, M, N_SWEEP))
    assert_equal(got, want, name)
    rows = {"merge": "n_out", "cluster": "n_clusters"}.get(name)
    assert (want[rows] if rows else want[name + ".fill"][1]) > (1000 if name != "complement" else 0), name


# ------------------------------------------------------------------ 3d. depth

N_OPS = 5 * 1024 + 3                # more than one tile of the ops scan
N_READS = 2600                      # ... as one or two ops a read
N_REGIONS = 700


@pytest.mark.parametrize("name", ["depth", "depth_text"])
def test_late_depth(W, name):
    with shaped(ops=N_OPS):
        want = W.host(("depth", name), lambda E, M: CASES[name](E, M, N_READS))
        got, _ = W.late(lambda E, M: CASES[name](E, M, N_READS))
    assert_equal(got, want, name)
    assert want[f"ivx_{name}.fill"][1] > 1000


READ_OUTS = ["depth_profile_blocks", "depth_profile_read", "depth_profile_expand", "depth_profile_summarize", "depth_profile_quantiles",
             "depth_profile_quantize", "depth_profile_hist"]


def merged_profile_sequence(E, M):
    """two profile builds from late columns, their merge, and every read-out of the sum (the catalogue's cases, on the sum in
    place of the Env's profile) with late region columns"""
    res, made = {}, []
    keep = E.profile
    try:
        with shaped(ops=N_OPS):
            big = ec._depth_in(M, N_READS, False)
        small = ec._depth_in(M, 64, False)
        for a, cols in (big, small):                           # (args, the columns they point into)
            h = C.c_void_p(0xDEAD)
            assert E.call("ivx_depth_profile_build", *a, C.byref(h), handle=h) == OK, E.err()
            made.append(pyivx.DepthProfile(E.ctx, h, NK, None))
        h = C.c_void_p(0xDEAD)
        assert E.call("ivx_depth_profile_merge", made[0].h, made[1].h, C.byref(h), handle=h) == OK, E.err()
        made.append(pyivx.DepthProfile(E.ctx, h, NK, None))
        E.profile = made[-1]
        res["steps"] = E.profile.steps()
        for name in READ_OUTS:
            res.update({f"{name}.{k}": v for k, v in CASES[name](E, M, N_REGIONS).items()})
    finally:
        E.profile = keep
        for p in made:
            p.free()
    return res


def test_late_merged_profile(W):
    want = W.host("profile", merged_profile_sequence)
    got, M = W.late(merged_profile_sequence)
    assert_equal(got, want, "merged profile")
    assert want["steps"] > 2 * 1024
    # one region of ivx_depth_profile_quantiles has more than DEPTH_RANK_SEGS segments: k_rank_select reads the device-side
    # list counter.  (The regions: entry_cases._regions; a region's segments: the steps inside it, and the one it starts in)
    pos, key = want["depth_profile_read.%d.o1" % want["steps"]], want["depth_profile_read.%d.o0" % want["steps"]]
    qk, qs, qe, _ = (b.np() for b in ec._regions(Mode(False), N_REGIONS))
    segs = max(int(np.count_nonzero((key == k) & (pos > s) & (pos <= e))) + 1 for k, s, e in zip(qk, qs, qe))
    assert segs > pyivx.DEPTH_RANK_SEGS, segs
    assert {e for e, *_ in M.calls} >= {"ivx_" + n for n in READ_OUTS} | {"ivx_depth_profile_build", "ivx_depth_profile_merge"}
