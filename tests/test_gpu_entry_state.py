"""-m gpu: what a context carries from one call of the C interface to the next -- grow-only scratch, the scalar words, the two
plans (ivx_join_plan, ivx_sub_plan), a build tail still running, the pool of recycled index buffers -- entry by entry.

Every entry of the catalogue (entry_cases.py) runs on ONE shared context between the calls that leave or use such state, and
must give what it gives on a context that was never poisoned (the baseline); the calls around it must give the oracle's answer.
The test hook ivx_debug_poison writes 0 or 1 into every 32-bit word of the state nobody is entitled to read again, so that a
read-before-write, a missing clear or a slot missing from a plan's mask is a wrong answer whatever ran before.

S0  poison everything, run X.
S1  region COUNT call, X, poison all but the plan's slots, FILL call: the oracle's pairs; the plan's state after X is the
    table's (JOIN_AFTER), read off the source.
S2  the same around a subtract sizing call and its fill (SUB_AFTER).
S3  X right behind an index build whose tail still runs.
S4  builds on poisoned recycled index buffers.
"""
import contextlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pair_set, synth
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_oracle as dorc  # noqa: E402
import depth_per_base_oracle as pbo  # noqa: E402
import ctypes as C  # noqa: E402
import nearest_dir_oracle as ndo  # noqa: E402
from entry_cases import CASES, Env, Mode, _same, assert_nearest_dir, ivals, nearest_dir_calls, nearest_dir_want, pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = sorted(CASES)
N = 1000                                # rows of every catalogue case
P = pyivx
ALL_BUT_POOL = P.POISON_SCRATCH | P.POISON_DROP_PLANS | P.POISON_SCALARS | P.POISON_PINNED
AROUND_PLANS = P.POISON_SCRATCH | P.POISON_SCALARS | P.POISON_PINNED
EVERYTHING = ALL_BUT_POOL | P.POISON_POOL


@contextlib.contextmanager
def environ(kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def designed(n=200_000):
    """n rows of length 255, one every 64 coordinates, on one key (test_gpu_plan_scalar_word.py's build): a lean index of
    some 50 regions"""
    s = np.arange(n, dtype=np.int64) * 64
    return np.zeros(n, np.uint32), s.astype(np.int32), (s + 255).astype(np.int32)


def device(cols):
    import torch
    d = tuple(torch.from_numpy(np.ascontiguousarray(c).view({4: np.int32, 8: np.int64}[c.dtype.itemsize])).cuda() for c in cols)
    torch.cuda.synchronize()                # (the contexts run on streams of their own)
    return d


def host(t):
    return t.cpu().numpy().view(np.uint32) if pyivx._is_torch(t) else t


def probe_nearest_k1(E, M, n):
    """ivx_probe_nearest with k = 1, the one k that reads IVX_NEAREST_PATH (ivx_ops32.hip: ivx_nearest_probe; the catalogue's
    probe_nearest asks for k = 2) -- the catalogue's columns, through the entry itself"""
    k, s, e = (M.put(a) for a in ivals(n, 11))
    b, p, d = M.out(n, np.uint32), M.out(n, np.uint32), M.out(n, np.int64)
    rows = C.c_uint64(0xDEAD)
    st = E.call("ivx_probe_nearest", E.ix[3].h, M.mem, k.p, s.p, e.p, C.c_uint64(n), C.c_int(0), C.c_uint32(1), C.c_int(1),
                b.p, p.p, d.p, C.c_uint64(n), C.byref(rows), outs=[b, p, d], count=rows)
    r = rows.value
    return {"st": st, "rows": r, "b": b.np()[:r], "p": p.np()[:r], "d": d.np()[:r]}


def probe_nearest_dir_k1(E, M, n):
    """ivx_probe_nearest_dir with k = 1, the one k that reads IVX_NEAREST_PATH (ivx_ops32.hip: nearest_probe_dir_t; the
    catalogue's probe_nearest_dir asks for k = 2) -- the catalogue's calls on the catalogue's columns"""
    return nearest_dir_calls(E, M, n, 1)


LOCAL_CASES = {"probe_nearest_k1": probe_nearest_k1, "probe_nearest_dir_k1": probe_nearest_dir_k1}


def run_case(E, name, dev, knobs):
    with environ(knobs):
        res = (CASES.get(name) or LOCAL_CASES[name])(E, Mode(dev), N)
    return {k: (v.cpu().numpy() if pyivx._is_torch(v) else v) for k, v in res.items()}


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    diff = [k for k in want if not _same(got[k], want[k])]
    assert not diff, (what, {k: (got[k], want[k]) for k in diff[:2]})


# ------------------------------------------------------------------ set-up, once per module

class Baseline:
    """every entry on a context that is never poisoned and never holds a plan of these tests; one run per (entry, mode, knobs)"""

    def __init__(self):
        self.E = Env(designed())
        self.seen = {}

    def __call__(self, name, dev, knobs):
        key = (name, dev, tuple(sorted(knobs.items())))
        if key not in self.seen:
            self.seen[key] = run_case(self.E, name, dev, knobs)
        return self.seen[key]


@pytest.fixture(scope="module")
def base():
    b = Baseline()
    yield b
    b.E.close()


@pytest.fixture(scope="module")
def E():
    e = Env(designed())
    lay = e.ix[0].layout()
    assert lay["nreg"] > 1 and lay["slow"] == 0, lay           # several regions, every one ONE LDS-resident level: the lean probes run
    # every forced path of S0 can be taken, or the library would answer with the direct kernel and say nothing:
    # IVX_ROWVAL_PATH=regions needs 0 < regions <= 1023 on the count and coverage indexes (ivx_ops32.hip: rowval_regions_wanted;
    # its flag IVX_IXF_REGION_ROWVAL is set for every coverage index and for a count index without a row of end < start, which
    # the designed column has none of), =routed and IVX_NEAREST_PATH=routed a routing view
    for kind in (pyivx.KIND_COUNT, pyivx.KIND_COVERAGE):
        assert 0 < e.ix[kind].layout()["nreg"] <= 1023, (kind, e.ix[kind].layout())
    for kind in (pyivx.KIND_COUNT, pyivx.KIND_COVERAGE, pyivx.KIND_NEAREST):
        assert e.ix[kind].forms()["nroute_nreg"] > 0, (kind, e.ix[kind].forms())
    yield e
    e.close()


@pytest.fixture(scope="module")
def near_want(E):
    """what probe_nearest_dir_k1 and the catalogue's probe_nearest_dir (k = 2) must give on E's build: the restatement of
    tests/nearest_dir_oracle.py, computed once"""
    oix = ndo.NearIndex(*E.build_cols)
    return {"probe_nearest_dir_k1": nearest_dir_want(oix, N, 1), "probe_nearest_dir": nearest_dir_want(oix, N, 2)}


class Probe:
    """probe rows as host columns and as device tensors, and the oracle's pairs with `build`"""

    def __init__(self, build, cols):
        self.h = cols
        self.d = device(cols)
        wb, wp = orc.join(*build, *cols, threads=4)
        self.want = pair_set(wb, wp)

    def cols(self, dev):
        return self.d if dev else self.h


def inside(build, n, seed):
    """n short rows with starts inside the span of a one-key build"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, int(build[1].max()), n)
    return np.zeros(n, np.uint32), x.astype(np.int32), (x + rng.integers(0, 100, n)).astype(np.int32)


@pytest.fixture(scope="module")
def probe(E):
    return Probe(E.build_cols, inside(E.build_cols, 20_000, 41))


class Sub:
    """50 000 left and 70 000 right rows over 5 keys, in both memory modes, and the oracle's rows"""

    def __init__(self):
        self.l = synth(50_000, 51, nkeys=5, mean_len=400, span=3_000_000, dtype=np.int64)
        self.r = synth(70_000, 52, nkeys=5, mean_len=150, span=3_000_000, dtype=np.int64)
        self.dl, self.dr = device(self.l), device(self.r)
        self.want = orc.subtract(*self.l, *self.r)

    def cols(self, dev):
        return (self.dl + self.dr) if dev else (self.l + self.r)


@pytest.fixture(scope="module")
def sub():
    return Sub()


# ------------------------------------------------------------------ S0: no entry depends on stale scratch or scalar words

JOIN_KNOBS = [{"IVX_JOIN_PATH": "direct"}, {"IVX_JOIN_PATH": "regions"}, {"IVX_JOIN_PATH": "regions", "IVX_PART": "two"}]
ROWVAL_KNOBS = [{"IVX_ROWVAL_PATH": "direct"}, {"IVX_ROWVAL_PATH": "regions"}, {"IVX_ROWVAL_PATH": "regions", "IVX_PART": "two"},
                {"IVX_ROWVAL_PATH": "routed"}]
NEAREST_KNOBS = [{"IVX_NEAREST_PATH": "direct"}, {"IVX_NEAREST_PATH": "routed"}]
# the path knobs an entry's layer honours (ivx_capi.hip overlap_common / ivx_probe_mark_build; ivx_ops32.hip); index_build
# probes the overlap, count and coverage indexes it built, so it takes those two at once.  IVX_NEAREST_PATH is read for
# k = 1 alone: the catalogue's probe_nearest, probe_nearest_dir and index_build ask for k = 2 and run once, probe_nearest_k1 and
# probe_nearest_dir_k1 (above) under both.  The select and threshold entries choose their path with region_path_wanted
# (ivx_capi.hip), which reads IVX_JOIN_PATH; ivx_pairs_where has one path and reads no knob: it runs under the three all the same
KNOBS = {
    "probe_overlap_count": JOIN_KNOBS, "probe_overlap_fill": JOIN_KNOBS, "probe_exists": JOIN_KNOBS, "probe_mark_build": JOIN_KNOBS,
    "probe_overlap_agg": JOIN_KNOBS, "probe_count": ROWVAL_KNOBS, "probe_coverage": ROWVAL_KNOBS, "probe_nearest_k1": NEAREST_KNOBS,
    "index_build": [{**JOIN_KNOBS[0], **ROWVAL_KNOBS[0]}, {**JOIN_KNOBS[1], **ROWVAL_KNOBS[1]}, {**JOIN_KNOBS[2], **ROWVAL_KNOBS[3]}],
    "probe_overlap_select": JOIN_KNOBS, "probe_overlap_count_where": JOIN_KNOBS, "probe_mark_build_where": JOIN_KNOBS,
    "probe_overlap_agg_where": JOIN_KNOBS, "probe_overlap_select_where": JOIN_KNOBS, "pairs_where": JOIN_KNOBS,
    "probe_nearest_dir_k1": NEAREST_KNOBS,
}
S0_RUNS = [(name, knobs) for name in NAMES + sorted(LOCAL_CASES) for knobs in KNOBS.get(name, [{}])]


def knob_id(knobs):
    return "+".join(f"{k[4:].lower()}={v}" for k, v in sorted(knobs.items())) or "default"


MODES = [pytest.param(False, id="host"), pytest.param(True, id="device")]


@pytest.mark.parametrize("value", [0, 1])
@pytest.mark.parametrize("dev", MODES)
@pytest.mark.parametrize("name,knobs", S0_RUNS, ids=[f"{n}-{knob_id(k)}" for n, k in S0_RUNS])
def test_s0_entry_on_poisoned_state(E, base, near_want, name, knobs, dev, value):
    want = base(name, dev, knobs)
    E.ctx.synchronize()
    E.ctx.debug_poison(value, ALL_BUT_POOL)
    st = E.ctx.debug_state()
    assert not st["join_valid"] and not st["sub_valid"]
    got = run_case(E, name, dev, knobs)
    assert_same(got, want, (name, knobs, dev, value))
    if name == "probe_nearest_k1":                              # ... and the baseline is the oracle's answer, on either path
        wb, wp, wd = orc.nearest(*E.build_cols, *ivals(N, 11), k=1)
        assert got["st"] == pyivx.OK and got["rows"] == len(wb) == N
        assert (got["b"] == wb).all() and (got["p"] == wp).all() and (got["d"] == wd).all(), knobs
    if name in near_want:                                       # probe_nearest_dir_k1 on either path, the catalogue's k = 2: the restatement's
        assert_nearest_dir(got, near_want[name], (name, knobs, dev, value))


def test_poison_refuses_a_word_above_one(E):
    with pytest.raises(pyivx.IvxError) as ei:
        E.ctx.debug_poison(2, ALL_BUT_POOL)
    assert ei.value.status == pyivx.ERR_INVALID and "the word is 0 or 1" in str(ei.value)


# ------------------------------------------------------------------ the expected plan state after X

K, D = "keeps", "drops"
# What X leaves of the JOIN plan of a region COUNT call, per memory mode of X: (host, device), under IVX_JOIN_PATH=regions.
# The plan's slots (ivx_regions_route.hip, R->slots): WS_SORTHIST, WS_T0, WS_T1, WS_IN_START, WS_IN_END; the paged form and
# the two-level form WS_T2 as well; the two-level form WS_SA0, WS_SA1, WS_T4..WS_T6 on top.  An entry drops the plan by
# drop_plans() / drop_join_plan() (ivx_capi.hip), by staging a host column into one of those slots (ivx_call.hpp: the second
# and third input column of a frame go to WS_IN_START / WS_IN_END), or by its device code taking one (get_scratch).
# "K2": keeps the flat form's plan (IVX_PART=two) only -- the entry takes WS_T2 and nothing else of the plan.
K2 = "keeps-flat"
JOIN_AFTER = {
    "index_build": (D, D),                      # its probes of the new indexes stage host columns, whatever mode the build ran in
    "probe_overlap_count": (D, D),              # its own count call replaces the plan, its per-row call routes again (WS_SORTHIST ...)
    "probe_overlap_fill": (D, D),               # its own count + fill consume a plan of its own; the one-short fill routes again
    "probe_exists": (D, D),                     # the per-row region probe routes its rows
    "probe_mark_build": (D, D),                 # drop_join_plan()
    "probe_overlap_agg": (D, D),                # drop_join_plan()
    "bits_mark": (K, K),                        # host: WS_IN_KEY and WS_OUT_A only; no scratch on the device
    "bits_select": (D, D),                      # WS_T0 (ivx_marks.hip)
    "probe_count": (D, K),                      # direct kernel, no scratch; host mode stages three columns
    "probe_coverage": (D, K),
    "probe_nearest": (D, K2),                   # k = 2: WS_T2..WS_T5
    "merge": (D, D), "subtract": (D, D), "cluster": (D, D), "complement": (D, D),      # WS_T0.. (ivx_sweep.hip)
    "intersect": (D, D),                        # drop_plans()
    "depth": (D, D), "depth_text": (D, D), "depth_profile_build": (D, D), "depth_profile_build_text": (D, D), "cigar_parse": (D, D),   # drop_plans()
    "depth_profile_read": (K, K),               # copies only
    "depth_profile_expand": (D, D), "depth_profile_blocks": (D, D), "depth_profile_summarize": (D, D), "depth_profile_windows": (D, D),
    "depth_profile_quantiles": (D, D), "depth_profile_window_quantiles": (D, D),           # drop_plans()
    "depth_profile_merge": (D, D), "depth_profile_quantize": (D, D), "depth_profile_hist": (D, D),      # drop_plans()
    "take_fixed": (D, K), "scatter_fixed": (D, K), "take_bits": (D, K),                    # no scratch on the device; host mode stages WS_IN_START / WS_IN_END
    "take_utf8": (D, D), "take_view": (D, D),   # WS_T0 (ivx_take.hip)
    "probe_overlap_select": (D, D),             # drop_join_plan() (ivx_capi.hip overlap_select_impl)
    "probe_overlap_count_where": (D, D),        # drop_join_plan() (ivx_probe_overlap_count_where)
    "probe_mark_build_where": (D, D),           # drop_join_plan() (mark_build_impl)
    "probe_overlap_agg_where": (D, D),          # drop_join_plan() (overlap_agg_impl)
    "probe_overlap_select_where": (D, D),       # drop_join_plan() (overlap_select_impl)
    "pairs_where": (D, D),                      # drop_join_plan() (ivx_pairs_where); WS_T5 / WS_T6 on top (ivx_where.hip)
    "probe_nearest_dir": (D, K2),               # no drop in the entry; k = 2: WS_T2..WS_T5 (ivx_ops32.hip nearest_probe_dir_t), as probe_nearest
}
# ... and of the SUBTRACT plan of a sizing call, at the default paths (1 000 rows take every direct kernel).  The plan's slots
# (ivx_sweep.hip): WS_T0..WS_T5, WS_T7, WS_T9, WS_RA0..2, WS_RB0..2 -- no staging slot, so host mode drops no more than device mode.
SUB_AFTER = {
    "index_build": (D, D),                      # the coverage and nearest builds take WS_T0..
    "probe_overlap_count": (K, K), "probe_overlap_fill": (K, K), "probe_exists": (K, K), "probe_mark_build": (K, K),   # direct kernels, no scratch
    "probe_overlap_agg": (K, K),                # drop_join_plan() only; direct kernel, no scratch (ivx_agg.hip: ivx_agg_probe)
    "bits_mark": (K, K),
    "bits_select": (D, D),                      # WS_T0
    "probe_count": (K, K), "probe_coverage": (K, K),
    "probe_nearest": (D, D),                    # WS_T2..WS_T5
    "merge": (D, D), "subtract": (D, D), "cluster": (D, D), "complement": (D, D), "intersect": (D, D),
    "depth": (D, D), "depth_text": (D, D), "depth_profile_build": (D, D), "depth_profile_build_text": (D, D), "cigar_parse": (D, D),
    "depth_profile_read": (K, K),
    "depth_profile_expand": (D, D), "depth_profile_blocks": (D, D), "depth_profile_summarize": (D, D), "depth_profile_windows": (D, D),
    "depth_profile_quantiles": (D, D), "depth_profile_window_quantiles": (D, D),
    "depth_profile_merge": (D, D), "depth_profile_quantize": (D, D), "depth_profile_hist": (D, D),
    "take_fixed": (K, K), "scatter_fixed": (K, K), "take_bits": (K, K),
    "take_utf8": (D, D), "take_view": (D, D),
    # drop_join_plan() only, then the direct kernel on staged or caller's columns (ivx_select.hip, ivx_marks.hip, ivx_agg.hip: no scratch)
    "probe_overlap_select": (K, K), "probe_mark_build_where": (K, K), "probe_overlap_agg_where": (K, K), "probe_overlap_select_where": (K, K),
    "probe_overlap_count_where": (K, K),        # the same; its total-only form takes WS_T6, which is no slot of the plan
    "pairs_where": (D, D),                      # WS_T5 (ivx_where.hip ivx_pairs_where_device: the tile counts)
    "probe_nearest_dir": (D, D),                # WS_T2..WS_T5
}


def test_the_tables_name_every_entry_and_keep_plans_alive():
    """no GPU work: the tables cover the catalogue, and each has a keeper in device mode -- S1 and S2 do reach planned fills"""
    assert sorted(JOIN_AFTER) == NAMES and sorted(SUB_AFTER) == NAMES
    assert any(v[1] == K for v in JOIN_AFTER.values()) and any(v[1] == K for v in SUB_AFTER.values())


def join_kept(name, dev, form):
    if name is None:
        return True
    v = JOIN_AFTER[name][int(dev)]
    return v == K or (v == K2 and form == "two")


# ------------------------------------------------------------------ S1: the join plan

def join_sequence(E, base, ix, pr, form, plan_dev, name, dev, value, no_plan=False):
    ctx = E.ctx
    knobs = {"IVX_JOIN_PATH": "regions"}
    if form == "two":
        knobs["IVX_PART"] = "two"
    cols = pr.cols(plan_dev)
    with environ(knobs):
        total = ctx.overlap_count(ix, *cols)
        st = ctx.debug_state()
        assert st["join_valid"] == 1 and st["join_slots"] != 0, st
        if name is not None:
            assert_same(run_case(E, name, dev, {}), base(name, dev, knobs), (name, dev, form))
        st = ctx.debug_state()
        assert st["join_valid"] == int(join_kept(name, dev, form)), (name, dev, form, st)
        wrote = ctx.debug_poison(value, AROUND_PLANS)
        if st["join_valid"]:
            assert wrote & st["join_slots"] == 0 and wrote != 0
        before = ctx.debug_state()
        assert before["join_valid"] == st["join_valid"]                # right before the fill: a kept plan is still there
        with environ({"IVX_NO_PLAN": "1"} if no_plan else {}):
            ob, op = ctx.overlap_fill(ix, *cols, cap=total)
    # the fill was served by the plan exactly when the plan was kept (host columns: the same pointers, no second upload)
    assert ctx.debug_state()["join_fills_planned"] - before["join_fills_planned"] == int(bool(st["join_valid"]) and not no_plan)
    assert total == len(pr.want)
    got = pair_set(host(ob), host(op))
    assert len(got) == total and (got == pr.want).all(), (name, dev, form, plan_dev)
    assert ctx.debug_state()["join_valid"] == 0                         # a plan serves one fill


@pytest.mark.parametrize("dev", MODES)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("plan_dev", [pytest.param(False, id="plan_host"), pytest.param(True, id="plan_device")])
@pytest.mark.parametrize("form", ["paged", "two"])
def test_s1_join_plan(E, base, probe, form, plan_dev, name, dev):
    value = (NAMES.index(name) + int(dev) + int(plan_dev) + (form == "two")) & 1
    join_sequence(E, base, E.ix[0], probe, form, plan_dev, name, dev, value)


@pytest.mark.parametrize("no_plan", [False, True], ids=["no_x", "no_plan"])
@pytest.mark.parametrize("plan_dev", [pytest.param(False, id="plan_host"), pytest.param(True, id="plan_device")])
@pytest.mark.parametrize("form", ["paged", "two"])
def test_s1_join_plan_alone(E, base, probe, form, plan_dev, no_plan):
    join_sequence(E, base, E.ix[0], probe, form, plan_dev, None, False, int(plan_dev) ^ int(no_plan), no_plan=no_plan)


@pytest.fixture(scope="module")
def wide(E):
    """test_gpu_join.py's test_join_more_than_1023_regions build, on the shared context: the two-level routing and its slot list"""
    b = synth(7_000_000, 63, nkeys=3, mean_len=200, span=240_000_000)
    ix = E.ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=3)
    assert ix.layout()["nreg"] > 1023
    p = synth(20_000, 64, nkeys=4, mean_len=150, span=240_000_000)
    p[2][::97] = p[1][::97] + 30_000
    yield ix, Probe(b, p)
    ix.free()


@pytest.mark.parametrize("dev", MODES)
@pytest.mark.parametrize("name", ["bits_mark", "take_fixed", "probe_nearest", "probe_nearest_dir", "merge", "depth_profile_read"])
def test_s1_join_plan_two_level(E, base, wide, name, dev):
    ix, pr = wide
    join_sequence(E, base, ix, pr, "paged", True, name, dev, int(dev))


# ------------------------------------------------------------------ S2: the subtract plan

def sub_sequence(E, base, sb, plan_dev, name, dev, value, no_plan=False):
    ctx = E.ctx
    after = {}

    def between():
        st = ctx.debug_state()
        assert st["sub_valid"] == 1 and st["sub_slots"] != 0, st
        if name is not None:
            assert_same(run_case(E, name, dev, {}), base(name, dev, {}), (name, dev))
        st = ctx.debug_state()
        kept = name is None or SUB_AFTER[name][int(dev)] == K
        assert st["sub_valid"] == int(kept), (name, dev, st)
        wrote = ctx.debug_poison(value, AROUND_PLANS)
        if st["sub_valid"]:
            assert wrote & st["sub_slots"] == 0 and wrote != 0
        after.update(ctx.debug_state())

    with environ({"IVX_NO_PLAN": "1"} if no_plan else {}):
        got = ctx.subtract(*sb.cols(plan_dev), n_keys=5, between=between)
    assert after["sub_valid"] == int(name is None or SUB_AFTER[name][int(dev)] == K)
    # the fill call was served by the plan exactly when the plan was kept
    assert ctx.debug_state()["sub_fills_planned"] - after["sub_fills_planned"] == int(bool(after["sub_valid"]) and not no_plan)
    for g, w in zip(got, sb.want):
        g = g.cpu().numpy().view(w.dtype) if pyivx._is_torch(g) else g
        assert len(g) == len(w) and g.dtype == w.dtype and (g == w).all(), (name, dev, plan_dev)
    assert ctx.debug_state()["sub_valid"] == 0


@pytest.mark.parametrize("dev", MODES)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("plan_dev", [pytest.param(False, id="plan_host"), pytest.param(True, id="plan_device")])
def test_s2_subtract_plan(E, base, sub, plan_dev, name, dev):
    sub_sequence(E, base, sub, plan_dev, name, dev, (NAMES.index(name) + int(dev) + int(plan_dev)) & 1)


@pytest.mark.parametrize("no_plan", [False, True], ids=["no_x", "no_plan"])
@pytest.mark.parametrize("plan_dev", [pytest.param(False, id="plan_host"), pytest.param(True, id="plan_device")])
def test_s2_subtract_plan_alone(E, base, sub, plan_dev, no_plan):
    sub_sequence(E, base, sub, plan_dev, None, False, int(plan_dev) ^ int(no_plan), no_plan=no_plan)


# ------------------------------------------------------------------ S3: behind an overlapped build

@pytest.fixture(scope="module")
def tail_build(E):
    """device build columns of 200 000 rows (they outlive every index built from them) and a probe batch with its oracle"""
    b = designed()
    b = (b[0], (b[1] + 7).astype(np.int32), (b[2] + 40).astype(np.int32))
    return device(b), Probe(b, inside(b, 20_000, 43))


@pytest.mark.parametrize("dev", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_s3_entry_behind_a_running_build_tail(E, base, tail_build, name, dev):
    ctx = E.ctx
    dcols, pr = tail_build
    want = base(name, dev, {})
    ctx.set_build_overlap(True)
    ix = None
    try:
        ix = ctx.build(pyivx.KIND_OVERLAP, *dcols, n_keys=1)
        assert ctx.debug_state()["tail_pending"] == 1
        with pytest.raises(pyivx.IvxError) as ei:               # the poison hook refuses while the tail runs (and writes nothing)
            ctx.debug_poison(1, ALL_BUT_POOL)
        assert ei.value.status == pyivx.ERR_INVALID and "a build tail is pending" in str(ei.value)
        assert ctx.debug_state()["tail_pending"] == 1
        got = run_case(E, name, dev, {})                        # at once, on the Env's older indexes
        assert_same(got, want, (name, dev))
        with environ({"IVX_JOIN_PATH": "regions"}):
            total = ctx.overlap_count(ix, *pr.d)
            ob, op = ctx.overlap_fill(ix, *pr.d, cap=total)
        pairs = pair_set(host(ob), host(op))
        assert total == len(pr.want) and len(pairs) == total and (pairs == pr.want).all()
    finally:
        ctx.set_build_overlap(False)
        if ix is not None:
            ix.free()


# ------------------------------------------------------------------ S4: builds on poisoned recycled buffers

def _rebuild(ctx, kind, value, cols_a, cols_b, nk):
    """build, free, poison all (the pool too), build the same kind from other columns of the same size: out of the pool"""
    ix = ctx.build(kind, *cols_a, n_keys=nk)
    ix.free()
    ctx.synchronize()
    free0 = ctx.debug_state()["pool_free"]
    assert free0 > 0
    ctx.debug_poison(value, EVERYTHING)
    ix = ctx.build(kind, *cols_b, n_keys=nk)
    assert ctx.debug_state()["pool_free"] < free0               # pool_take handed the build poisoned buffers
    return ix


@pytest.mark.parametrize("value", [0, 1])
@pytest.mark.parametrize("kind", ["overlap", "count", "coverage", "nearest"])
def test_s4_build_on_poisoned_pool(E, kind, value):
    ctx = E.ctx
    nk = 4
    a = synth(30_000, 71, nkeys=nk, mean_len=300, span=3_000_000)
    b = synth(30_000, 72, nkeys=nk, mean_len=300, span=3_000_000)
    p = synth(20_000, 73, nkeys=nk + 1, mean_len=100, span=3_000_000)
    ix = _rebuild(ctx, getattr(pyivx, "KIND_" + kind.upper()), value, a, b, nk + 1)
    try:
        if kind == "overlap":
            wb, wp = orc.join(*b, *p, threads=4)
            for path in ("direct", "regions"):
                with environ({"IVX_JOIN_PATH": path}):
                    total = ctx.overlap_count(ix, *p)
                    ob, op = ctx.overlap_fill(ix, *p, cap=total)
                assert total == len(wb) and (pair_set(ob, op) == pair_set(wb, wp)).all(), path
        elif kind == "count":
            assert (ctx.count_overlaps(ix, *p) == orc.count_overlaps(*b, *p)).all()
        elif kind == "coverage":
            assert (ctx.coverage(ix, *p) == orc.coverage(*b, *p)).all()
        else:
            for k in (1, 3):
                wb, wp, wd = orc.nearest(*b, *p, k=k)
                gb, gp, gd = ctx.nearest(ix, *p, k=k)
                assert len(gb) == len(wb) and (gb == wb).all() and (gp == wp).all() and (gd == wd).all(), k
    finally:
        ix.free()


@pytest.mark.parametrize("value", [0, 1])
def test_s4_depth_profile_on_poisoned_pool(E, value):
    ctx = E.ctx
    rng = np.random.default_rng(81)
    a = dorc.random_case(rng, n_reads=300, n_seg=80, n_keys=3, max_pos=4000)
    b = dorc.random_case(rng, n_reads=300, n_seg=80, n_keys=3, max_pos=4000)
    p = ctx.depth_profile(**a)
    p.free()
    ctx.synchronize()
    free0 = ctx.debug_state()["pool_free"]
    ctx.debug_poison(value, EVERYTHING)
    p = ctx.depth_profile(**b)
    try:
        assert ctx.debug_state()["pool_free"] < free0
        want = pbo.steps(b["n_keys"], **dorc.oracle_kw(b))
        for g, w in zip(p.read(), want):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        for g, w in zip(p.blocks(), dorc.depth_loop(**dorc.oracle_kw(b))):
            assert np.array_equal(g, w)
    finally:
        p.free()
