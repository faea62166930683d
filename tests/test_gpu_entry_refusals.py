"""-m gpu: what a device reservation that is REFUSED in the middle of a call leaves behind (ivx_ctx_set_memory_limit,
IVX_ERR_OOM), entry by entry -- the walk of test_gpu_entry_state.py along the axis it leaves out.

The limit itself makes the k-th growing reservation of a call fail, deterministically, and the error text says how far to
raise it for the next attempt:
    Resources exhausted: failed to reserve B bytes of device scratch (R bytes reserved, limit L)      (ivx_ctx::get_scratch)
    Resources exhausted: failed to reserve B bytes for the index (R bytes reserved, limit L)         (ivx_index_alloc)
so no hook is needed: trim, set the limit to L0 = what the live indexes take, run the case; on a refusal check what it left
(below), raise the limit to R + B and go again, until the case runs through -- with the tightest limit that suffices, where
no reservation got its 1/8 slack -- and equals the never-limited baseline bit for bit.

R1  every catalogue case (entry_cases.py), probe_nearest_k1 and probe_nearest_dir_k1, host and device mode, the default paths and every forced
    path of test_gpu_entry_state.KNOBS, on the designed 200 000-row build (region and lean forms).  After each refused
    attempt, the limit still set: only OK / OOM / CAPACITY / INVALID statuses and a clean ivx_ctx_synchronize; the refused
    call's out-handle is NULL and its count 0 or the baseline's; in host mode its output buffers are untouched; the output
    metrics and build_mem_used are what they were before it, the input metrics count the refused batch as they count a
    served one.  Then, limit off and WITHOUT a trim, the case again on the context the refusal left: the baseline, bit for
    bit.  Then trim(0): reserved_bytes() is L0 again (a refused build, profile build or merge leaks nothing).
R2  a refusal between a sizing call and its fill (region count -> fill, subtract sizing -> fill): the limited fill is
    the oracle's answer or IVX_ERR_OOM; the unlimited fill behind it is the oracle's answer, served by the plan exactly when
    the plan was still valid after the refusal.  Stepped until the limited fill is served: every exit of a planned fill.
R3  a refusal behind the fork of an overlapped build (200 000 device rows, ivx_ctx_set_build_overlap): no handle, no
    pending tail, a good build right after it, nothing leaked.
R4  a regression test, not a race detector: after each refused build on one context, at once a build and probe on ANOTHER
    context (the pool of recycled index buffers is shared by all contexts; a refused build drains its streams before its
    buffers go there, ivx_capi.hip index_commit) -- compared with the oracle.

Every refusal here is a status the host returns before the kernel it guards is started.

Refusal points met per (case, knobs, mode), copied from one run; a row changes when an entry gains or loses a reservation:
    case                              knobs                                          host  device
    bits_mark                         default                                           3       0
    bits_select                       default                                           6       1
    cigar_parse                       default                                          10       1
    cluster                           default                                          44      22
    complement                        default                                          70      47
    depth                             default                                          44      13
    depth_profile_blocks              default                                           9       1
    depth_profile_build               default                                          42      19
    depth_profile_build_text          default                                          44      23
    depth_profile_expand              default                                           3       0
    depth_profile_hist                default                                           3       0
    depth_profile_merge               default                                           9       9
    depth_profile_quantiles           default                                          16       1
    depth_profile_quantize            default                                          15       5
    depth_profile_read                default                                           0       0
    depth_profile_summarize           default                                          12       0
    depth_profile_window_quantiles    default                                           9       1
    depth_profile_windows             default                                           5       0
    depth_text                        default                                          46      17
    index_build                       default                                          57      56
    index_build                       join_path=direct+rowval_path=direct              57      56
    index_build                       join_path=regions+part=two+rowval_path=routed    68      67
    index_build                       join_path=regions+rowval_path=regions            66      65
    intersect                         default                                          70      50
    merge                             default                                          30      16
    pairs_where                       default                                          20       3
    pairs_where                       join_path=direct                                 20       3
    pairs_where                       join_path=regions                                20       3
    pairs_where                       join_path=regions+part=two                       20       3
    probe_count                       default                                           7       0
    probe_count                       part=two+rowval_path=regions                     15       7
    probe_count                       rowval_path=direct                                7       0
    probe_count                       rowval_path=regions                              16       8
    probe_count                       rowval_path=routed                               15       7
    probe_coverage                    default                                           7       0
    probe_coverage                    part=two+rowval_path=regions                     15       7
    probe_coverage                    rowval_path=direct                                7       0
    probe_coverage                    rowval_path=regions                              15       7
    probe_coverage                    rowval_path=routed                               15       7
    probe_exists                      default                                           7       0
    probe_exists                      join_path=direct                                  7       0
    probe_exists                      join_path=regions                                16       8
    probe_exists                      join_path=regions+part=two                       15       7
    probe_mark_build                  default                                           7       0
    probe_mark_build                  join_path=direct                                  7       0
    probe_mark_build                  join_path=regions                                14       6
    probe_mark_build                  join_path=regions+part=two                        7       0
    probe_mark_build_where            default                                           7       0
    probe_mark_build_where            join_path=direct                                  7       0
    probe_mark_build_where            join_path=regions                                14       6
    probe_mark_build_where            join_path=regions+part=two                        7       0
    probe_nearest                     default                                          19       7
    probe_nearest_dir                 default                                          19       7
    probe_nearest_dir_k1              default                                          11       0
    probe_nearest_dir_k1              nearest_path=direct                              11       0
    probe_nearest_dir_k1              nearest_path=routed                              21       9
    probe_nearest_k1                  default                                          11       0
    probe_nearest_k1                  nearest_path=direct                              11       0
    probe_nearest_k1                  nearest_path=routed                              21       9
    probe_overlap_agg                 default                                          18       0
    probe_overlap_agg                 join_path=direct                                 18       0
    probe_overlap_agg                 join_path=regions                                29      10
    probe_overlap_agg                 join_path=regions+part=two                       18       0
    probe_overlap_agg_where           default                                          18       0
    probe_overlap_agg_where           join_path=direct                                 18       0
    probe_overlap_agg_where           join_path=regions                                29      10
    probe_overlap_agg_where           join_path=regions+part=two                       18       0
    probe_overlap_count               default                                           7       0
    probe_overlap_count               join_path=direct                                  7       0
    probe_overlap_count               join_path=regions                                15       7
    probe_overlap_count               join_path=regions+part=two                       15       7
    probe_overlap_count_where         default                                          11       1
    probe_overlap_count_where         join_path=direct                                 11       1
    probe_overlap_count_where         join_path=regions                                20      10
    probe_overlap_count_where         join_path=regions+part=two                       11       1
    probe_overlap_fill                default                                           9       0
    probe_overlap_fill                join_path=direct                                  9       0
    probe_overlap_fill                join_path=regions                                15       6
    probe_overlap_fill                join_path=regions+part=two                       15       5
    probe_overlap_select              default                                          10       0
    probe_overlap_select              join_path=direct                                 10       0
    probe_overlap_select              join_path=regions                                21      10
    probe_overlap_select              join_path=regions+part=two                       10       0
    probe_overlap_select_where        default                                           9       0
    probe_overlap_select_where        join_path=direct                                  9       0
    probe_overlap_select_where        join_path=regions                                20      10
    probe_overlap_select_where        join_path=regions+part=two                        9       0
    scatter_fixed                     default                                           5       0
    subtract                          default                                          72      52
    take_bits                         default                                           8       0
    take_fixed                        default                                           8       0
    take_utf8                         default                                          17       1
    take_view                         default                                          14       3
    (a point is an attempt that ended in a refusal: the same reservation counts twice where an earlier slot took its slack
     in between.  R2: region count -> fill 5 rounds host (3 refusals with a live plan), 2 device (0); subtract 8 rounds
     host (7 with a live plan), 1 device (a planned subtract fill reserves nothing).  R3: 19 refusal points with the
     per-region tail, 20 with IVX_BUILD=global -- the one more is the scan's scratch behind the fork.)
"""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import pair_set
from entry_cases import CAPACITY, CASES, INVALID, OK, OOM, Env, Mode, Refused, _same, pyivx, untouched
from test_gpu_entry_state import (KNOBS, LOCAL_CASES, MODES, N, Probe, Sub, designed, device, environ, host, inside, knob_id)

pytestmark = pytest.mark.gpu

TEXT = re.compile(r"Resources exhausted: failed to reserve (\d+) bytes (?:of device scratch|for the index) "
                  r"\((\d+) bytes reserved, limit (\d+)\)")
MAX_ATTEMPTS = 256
ALL_CASES = {**CASES, **LOCAL_CASES}
RUNS = [(name, knobs) for name in sorted(ALL_CASES) for knobs in [{}] + KNOBS.get(name, [])]

# (case, mode) that may run through at L0 without a refusal, and why.  Host mode: every other case stages a column.
NO_RESERVATION = {
    ("depth_profile_read", "host"): "ivx_depth_profile_read copies from the profile to the caller's buffers: no staging, no scratch",
    ("depth_profile_read", "device"): "the same copies, device to device",
    # direct kernels on the caller's device pointers, no scratch (test_gpu_entry_state.SUB_AFTER says the same of them)
    ("probe_exists", "device"): "ivx_join_probe: direct kernel on the caller's pointers",
    ("probe_mark_build", "device"): "ivx_mark_probe: direct kernel, ORs into the caller's bitmap",
    ("probe_overlap_agg", "device"): "ivx_agg_probe: direct kernel (ivx_agg.hip takes no scratch)",
    ("probe_overlap_count", "device"): "ivx_join_probe: direct kernel, the total through the context's scalar words",
    ("probe_overlap_fill", "device"): "ivx_join_probe: direct kernel into the caller's pair buffers",
    ("probe_count", "device"): "ivx_count_probe: direct kernel",
    ("probe_coverage", "device"): "ivx_coverage_probe: direct kernel",
    ("bits_mark", "device"): "ivx_marks.hip: one kernel on the caller's bitmap",
    ("take_fixed", "device"): "ivx_take.hip: one gather kernel", ("take_bits", "device"): "ivx_take.hip: one gather kernel",
    ("scatter_fixed", "device"): "ivx_take.hip: one scatter kernel",
    ("depth_profile_hist", "device"): "include/ivx.h: hist takes no scratch",
    ("depth_profile_expand", "device"): "ivx_depth_expand.hip ivx_depth_expand_device: one kernel, no scratch",
    ("depth_profile_summarize", "device"): "ivx_depth_regions.hip region_aggregates: a profile of at most two tiles makes no aggregates",
    ("depth_profile_windows", "device"): "the same: Env.profile has at most 2 * 1024 steps",
    ("probe_nearest_k1", "device"): "ivx_ops32.hip ivx_nearest_probe: k = 1 takes the direct kernel",
    ("probe_nearest_dir_k1", "device"): "ivx_ops32.hip nearest_probe_dir_t: k = 1 below 2^21 rows launches k_probe_nearest1_dir on the caller's pointers",
    ("probe_overlap_select", "device"): "ivx_select.hip ivx_sel_probe: ivx_direct_probe on the caller's pointers, no scratch",
    ("probe_overlap_select_where", "device"): "the same kernel behind WhereOp (ivx_capi.hip overlap_select_impl)",
    ("probe_mark_build_where", "device"): "ivx_marks.hip ivx_mark_probe: ivx_direct_probe behind WhereOp, ORs into the caller's bitmap",
    ("probe_overlap_agg_where", "device"): "ivx_agg.hip ivx_agg_probe: ivx_direct_probe behind WhereOp, no scratch",
    # (NOT probe_overlap_count_where: its total-only call takes WS_T6 in either mode; NOT pairs_where: WS_T5, WS_T6 and the scan's;
    #  NOT probe_nearest_dir: k = 2 takes WS_T2..WS_T5)
}
# forced paths that end in the direct kernel all the same: the table above applies to them
DIRECT_ALL_THE_SAME = {
    ("probe_mark_build", "join_path=regions+part=two"): "ivx_regions_probe.hip ivx_mark_probe_regions: *took = false with IVX_PART=two",
    ("probe_overlap_agg", "join_path=regions+part=two"): "ivx_regions_probe.hip ivx_agg_probe_regions: the same",
    # lean_route is the one gate of every lean launcher: the four below take it with the same arguments
    ("probe_overlap_select", "join_path=regions+part=two"): "ivx_regions_probe.hip ivx_sel_probe_regions: lean_route gives *took = false",
    ("probe_overlap_select_where", "join_path=regions+part=two"): "ivx_sel_probe_regions: the same",
    ("probe_mark_build_where", "join_path=regions+part=two"): "ivx_mark_probe_regions: the same",
    ("probe_overlap_agg_where", "join_path=regions+part=two"): "ivx_agg_probe_regions: the same",
}
# Outputs a refused call legitimately wrote BEFORE the reservation that was refused: (entry, index among the call's outputs)
# -> where the source does it.  Everything else must still hold the pattern.
WRITES_BEFORE_REFUSAL = {
    ("ivx_depth_profile_read", 3): "ivx_capi.hip ivx_depth_profile_read: key_seen goes out before anything else (it takes no scratch at all)",
}


def parse(text):
    m = TEXT.fullmatch(text)
    assert m, text
    b, r, lim = map(int, m.groups())
    return b, r, lim


class Walked:
    """one Env and its L0: what the context reserves with all scratch trimmed (its live indexes and profiles)"""

    def __init__(self):
        self.E = Env(designed())
        self.E.ctx.trim(0)
        self.L0 = self.E.ctx.reserved_bytes()
        assert self.L0 > 0


@pytest.fixture(scope="module")
def W():
    w = Walked()
    yield w
    w.E.close()


class Baseline:
    """every case on a context that never had a limit: (results, log), one run per (case, mode, knobs)"""

    def __init__(self):
        self.E = Env(designed())
        self.seen = {}

    def __call__(self, name, dev, knobs):
        key = (name, dev, tuple(sorted(knobs.items())))
        if key not in self.seen:
            self.seen[key] = run(self.E, name, dev, knobs)[:2]
        return self.seen[key]


@pytest.fixture(scope="module")
def base():
    b = Baseline()
    yield b
    b.E.close()


def run(E, name, dev, knobs, stop_on_oom=False):
    """-> (results or None, the log, the refused Call or None)"""
    E.log, E.stop_on_oom = [], stop_on_oom
    res = refused = None
    try:
        with environ(knobs):
            res = ALL_CASES[name](E, Mode(dev), N)
        res = {k: (v.cpu().numpy() if pyivx._is_torch(v) else v) for k, v in res.items()}
    except Refused:
        refused = E.log[-1]
    except pyivx.IvxError as ex:            # (index_build probes its new indexes through pyivx's wrappers)
        assert ex.status == OOM, ex
        refused = ex
    finally:
        E.stop_on_oom = False
    log, E.log = E.log, []
    return res, log, refused


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    diff = [k for k in want if not _same(got[k], want[k])]
    assert not diff, (what, {k: (got[k], want[k]) for k in diff[:2]})


IN_FIELDS = ("input_batches", "input_rows", "build_input_batches", "build_input_rows")
OUT_FIELDS = ("output_batches", "output_rows", "build_mem_used")


def check_refused_call(E, call, base_call, dev, what):
    """the refused call itself, the limit still set"""
    if call.has_handle:
        assert call.handle is None, what
    if call.count is not None:
        assert call.count in (0, base_call.count), (what, call.count, base_call.count)
    if not dev:
        for i, o in enumerate(call.outs):
            if (call.entry, i) in WRITES_BEFORE_REFUSAL:
                continue
            if isinstance(o, tuple):                            # (a buffer the entry ORs into: the caller's own bits, nothing more)
                assert np.array_equal(o[0].np(), o[1]), (what, call.entry, i)
            else:
                assert untouched(o), (what, call.entry, i)
    now = E.ctx.metrics()
    for f in OUT_FIELDS:
        assert now[f] == call.before[f], (what, call.entry, f, now[f], call.before[f])
    # the input side counts a refused batch exactly as it counts a served one (Frame::meter runs before any reservation)
    for f in IN_FIELDS:
        assert now[f] - call.before[f] == base_call.after[f] - base_call.before[f], (what, call.entry, f)


def walk(W, base, name, dev, knobs):
    """-> the number of refusal points met"""
    E, ctx = W.E, W.E.ctx
    want, want_log = base(name, dev, knobs)
    what = (name, "device" if dev else "host", knob_id(knobs))
    limit, points = W.L0, 0
    try:
        for attempt in range(MAX_ATTEMPTS + 1):
            assert attempt < MAX_ATTEMPTS, (what, "more attempts than the cap", limit)
            ctx.trim(0)
            assert ctx.reserved_bytes() == W.L0, what
            ctx.set_memory_limit(limit)
            got, log, refused = run(E, name, dev, knobs, stop_on_oom=True)
            assert all(c.st in (OK, OOM, CAPACITY, INVALID) for c in log), (what, [(c.entry, c.st, c.text) for c in log])
            assert E.L.ivx_ctx_synchronize(E.h) == OK, what
            if refused is None:
                # the tightest limit that suffices: no reservation got its slack, the answer is the same
                assert_same(got, want, what + ("at the tightest limit", limit))
                break
            points += 1
            text = refused.text if not isinstance(refused, pyivx.IvxError) else E.err()
            b, r, lim = parse(text)
            assert lim == limit and r + b > limit, (what, text, limit)
            if not isinstance(refused, pyivx.IvxError):
                check_refused_call(E, refused, want_log[len(log) - 1], dev, what + (attempt, text))
            # the context the refusal left, as it is: no trim
            ctx.set_memory_limit(0)
            again, _, r2 = run(E, name, dev, knobs)
            assert r2 is None
            assert_same(again, want, what + ("after the refusal of", text))
            ctx.trim(0)
            assert ctx.reserved_bytes() == W.L0, (what, "leaked after", text)
            limit = r + b
    finally:
        ctx.set_memory_limit(0)
    return points


@pytest.mark.parametrize("dev", MODES)
@pytest.mark.parametrize("name,knobs", RUNS, ids=[f"{n}-{knob_id(k)}" for n, k in RUNS])
def test_r1_refusal_walk(W, base, name, knobs, dev):
    mode = "device" if dev else "host"
    points = walk(W, base, name, dev, knobs)
    print(f"REFUSAL_POINTS {name} {mode} {knob_id(knobs)} {points}")       # (the docstring's table: run with -s)
    if points == 0:
        # (the table is about the direct kernels: a forced region or routed path reserves in either mode)
        assert not any(v in ("regions", "routed") for v in knobs.values()) or (name, knob_id(knobs)) in DIRECT_ALL_THE_SAME, (name, mode, knobs)
        assert (name, mode) in NO_RESERVATION, (name, mode, "ran through at L0: no reservation was refused")


def test_r1_the_tables_are_about_the_catalogue():
    """no GPU work: the exemption tables name catalogue cases and entries only"""
    assert {n for n, _ in NO_RESERVATION} <= set(ALL_CASES)
    assert {e[4:] for e, _ in WRITES_BEFORE_REFUSAL} <= set(CASES)
    assert all(NO_RESERVATION.values()) and all(WRITES_BEFORE_REFUSAL.values())
    assert all(any(knob_id(k) == kid for k in KNOBS[name]) for name, kid in DIRECT_ALL_THE_SAME)


# ------------------------------------------------------------------ R2: between a sizing call and its fill

def stepped(ctx, sizing, fill, check, valid_word, planned_word, what):
    """sizing() unlimited, then fill() under a limit that lets one reservation more through each round, then fill() unlimited
    on what the refusal left.  fill() -> the answer, or raises IvxError(OOM).  -> (rounds, refusals with a live plan)"""
    limit, live = None, 0
    try:
        for rnd in range(MAX_ATTEMPTS + 1):
            assert rnd < MAX_ATTEMPTS, what
            ctx.trim(0)
            sizing()
            assert ctx.debug_state()[valid_word] == 1, what
            held = ctx.reserved_bytes()
            if limit is None:
                limit = held                                    # exactly what is held: nothing may grow
            assert limit >= held, (what, limit, held)
            ctx.set_memory_limit(limit)
            try:
                got = fill()
            except pyivx.IvxError as ex:
                assert ex.status == OOM, ex
                got = None
                b, r, lim = parse(pyivx.lib().ivx_last_error(ctx.h).decode())           # (IvxError wraps the text in a prefix)
                assert lim == limit and r + b > limit
            st = ctx.debug_state()
            ctx.set_memory_limit(0)
            if got is not None:
                check(got, what + ("limited fill", limit))
                return rnd + 1, live
            live += int(st[valid_word])
            before = st[planned_word]
            check(fill(), what + ("unlimited fill after a refusal at", limit))
            # served by the plan exactly when the plan was still valid after the refusal
            assert ctx.debug_state()[planned_word] - before == int(st[valid_word]), (what, limit, st)
            limit = r + b
    finally:
        ctx.set_memory_limit(0)


@pytest.fixture(scope="module")
def probe(W):
    return Probe(W.E.build_cols, inside(W.E.build_cols, 20_000, 41))


@pytest.fixture(scope="module")
def sub():
    return Sub()


@pytest.mark.parametrize("dev", MODES)
@pytest.mark.parametrize("pair", ["region_count_fill", "subtract"])
def test_r2_refusal_between_sizing_and_fill(W, probe, sub, pair, dev):
    ctx = W.E.ctx
    what = (pair, "device" if dev else "host")
    if pair == "region_count_fill":
        cols, total = probe.cols(dev), []

        def sizing():
            total[:] = [ctx.overlap_count(W.E.ix[0], *cols)]

        def fill():
            return ctx.overlap_fill(W.E.ix[0], *cols, cap=total[0])

        def check(got, why):
            pairs = pair_set(host(got[0]), host(got[1]))
            assert total[0] == len(probe.want) and len(pairs) == total[0] and (pairs == probe.want).all(), why
        with environ({"IVX_JOIN_PATH": "regions"}):
            rounds, live = stepped(ctx, sizing, fill, check, "join_valid", "join_fills_planned", what)
    else:
        L, cols = pyivx.lib(), sub.cols(dev)
        args = (C.c_int(pyivx.MEM_DEVICE if dev else pyivx.MEM_HOST), *[pyivx._ptr(c) for c in cols[:3]], C.c_uint64(len(sub.l[1])),
                *[pyivx._ptr(c) for c in cols[3:]], C.c_uint64(len(sub.r[1])), C.c_uint32(5), C.c_int(0))
        m = C.c_uint64(0)

        def sizing():
            ctx._chk(L.ivx_subtract(ctx.h, *args, None, None, None, None, C.c_uint64(0), C.byref(m)))

        def fill():
            cap = m.value
            outs = [Mode(dev).out(cap, dt) for dt in (np.uint32, np.int64, np.int64, np.uint32)]
            m2 = C.c_uint64(0)
            ctx._chk(L.ivx_subtract(ctx.h, *args, *[o.p for o in outs], C.c_uint64(cap), C.byref(m2)))
            ctx.synchronize()
            return [o.np()[:m2.value] for o in outs]

        def check(got, why):
            for g, w in zip(got, sub.want):
                assert len(g) == len(w) and g.dtype == w.dtype and (g == w).all(), why
        rounds, live = stepped(ctx, sizing, fill, check, "sub_valid", "sub_fills_planned", what)
    print(f"R2 {pair} {what[1]}: {rounds} rounds, {live} refusals left a valid plan")
    ctx.trim(0)
    assert ctx.reserved_bytes() == W.L0


# ------------------------------------------------------------------ R3 / R4: refused builds

@pytest.fixture(scope="module")
def tail_build():
    """device build columns of 200 000 rows, and a probe batch with its oracle"""
    b = designed()
    b = (b[0], (b[1] + 7).astype(np.int32), (b[2] + 40).astype(np.int32))
    return device(b), Probe(b, inside(b, 20_000, 43))


def good_build(ctx, dcols, pr, what):
    """an unlimited overlap build, count and fill: the oracle's pairs"""
    ix = ctx.build(pyivx.KIND_OVERLAP, *dcols, n_keys=1)
    try:
        with environ({"IVX_JOIN_PATH": "regions"}):
            total = ctx.overlap_count(ix, *pr.d)
            ob, op = ctx.overlap_fill(ix, *pr.d, cap=total)
        pairs = pair_set(host(ob), host(op))
        assert total == len(pr.want) and len(pairs) == total and (pairs == pr.want).all(), what
        ctx.synchronize()
    finally:
        ix.free()


def walk_build(E, L0, dcols, after_refusal):
    """the limit stepped across ivx_index_build(IVX_KIND_OVERLAP) of device columns; after_refusal(text) runs after every
    refused build, the limit off.  -> refusal points"""
    ctx, L = E.ctx, E.L
    n = len(dcols[1])
    limit, points, index_points = L0, 0, 0
    try:
        for attempt in range(MAX_ATTEMPTS + 1):
            assert attempt < MAX_ATTEMPTS
            ctx.trim(0)
            assert ctx.reserved_bytes() == L0 and ctx.debug_state()["pool_free"] == 0
            ctx.set_memory_limit(limit)
            h = C.c_void_p(0xDEAD)
            st = L.ivx_index_build(ctx.h, C.c_int(pyivx.KIND_OVERLAP), C.c_int(pyivx.MEM_DEVICE), *[pyivx._ptr(c) for c in dcols],
                                   C.c_uint64(n), C.c_uint32(1), C.byref(h))
            text = E.err()
            state = ctx.debug_state()
            ctx.set_memory_limit(0)
            if st == OK:
                ctx.synchronize()
                L.ivx_index_free(h)
                break
            assert st == OOM, (st, text)
            points += 1
            b, r, lim = parse(text)
            assert lim == limit and r + b > limit
            assert h.value is None, text                        # no handle
            assert state["tail_pending"] == 0, text             # no tail left running behind the refusal
            # every buffer the refused build had got is back in the pool: an index reservation has no slack, so each of them
            # is refused exactly once, in order, and all of them come before the build's first scratch (ivx_join_build)
            assert state["pool_free"] == index_points, (text, state["pool_free"], index_points)
            index_points += "for the index" in text
            after_refusal(text)
            ctx.trim(0)
            assert ctx.reserved_bytes() == L0, ("leaked after", text)
            limit = r + b
    finally:
        ctx.set_memory_limit(0)
    return points


BUILD_KNOBS = [{}, {"IVX_BUILD": "global"}]         # the per-region LDS tail where the layout allows it; the global tail (count, scan, scatter)


@pytest.mark.parametrize("knobs", BUILD_KNOBS, ids=knob_id)
def test_r3_refusal_behind_the_fork_of_an_overlapped_build(W, tail_build, knobs):
    ctx = W.E.ctx
    dcols, pr = tail_build
    ctx.set_build_overlap(True)
    try:
        with environ(knobs):
            points = walk_build(W.E, W.L0, dcols, lambda text: good_build(ctx, dcols, pr, text))
    finally:
        ctx.set_build_overlap(False)
    print(f"R3 {knob_id(knobs)}: {points} refusal points")
    assert points > 0


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlapped"])
def test_r4_another_context_builds_right_after_a_refused_build(W, tail_build, overlap):
    """A regression test of index_commit's failure path, not a race detector: the refused build's buffers are in the shared
    pool when context B builds an index of the same size on its own stream; B's answer is the oracle's every time."""
    ctx = W.E.ctx
    dcols, pr = tail_build
    B = pyivx.Ctx(0)
    ctx.set_build_overlap(overlap)
    try:
        with environ({"IVX_BUILD": "global"}):
            points = walk_build(W.E, W.L0, dcols, lambda text: good_build(B, dcols, pr, ("context B after", text)))
    finally:
        ctx.set_build_overlap(False)
        B.close()
    assert points > 0
