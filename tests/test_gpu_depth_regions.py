"""-m gpu: depth region summaries on the device (ivx_depth_profile_summarize / ivx_depth_profile_windows,
csrc/ivx_depth_regions.hip), bit-exact against tests/depth_regions_oracle.py, in host and in device memory mode.

Profiles are made from weighted segments whose end event is clipped away, one step per segment, so that step counts are
exact.  With T = pyivx.DEPTH_REGION_TILE steps per tile aggregate, the shapes sit where the kernels can go wrong: keys of
T - 1 ... 3T + 1 steps laid out one after another (so the tiles, which are cut over the whole step list, straddle the key
changes), regions whose first and last step share a step, a tile, lie in adjacent tiles or three tiles apart, bounds one
below, on and one above a step, regions before the first and beyond the last step, thousands of keys of one or two steps
around one long key, keys without steps, an empty profile."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_oracle as orc  # noqa: E402
import depth_regions_oracle as dro  # noqa: E402
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

T = pyivx.DEPTH_REGION_TILE
WG = 4                          # regions (wavefronts) per workgroup of the query kernel
M32 = 0xFFFFFFFF
NULL = pyivx.NULL_IDX
BIG = 1 << 31                   # a key length no test position reaches, below 2^32 - 1: a segment's end event is clipped
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
THR = (I32_MIN, -2, 0, 1, I32_MAX)
THR8 = (I32_MIN, -3, -1, 0, 1, 2, 5, I32_MAX)
SIZES = (T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 1)


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


def dev_u32(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def same(got, want):
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w)


def stepped(ctx, keys, pos, w, n_keys):
    """one step per (key, position, weight != 0) -> (profile, its steps as the oracle takes them)"""
    keys, pos, w = np.asarray(keys, np.uint32), np.asarray(pos, np.uint32), np.asarray(w, np.int32)
    p = ctx.depth_profile(skey=keys, sstart=pos, send=np.full(len(pos), M32, np.uint32), sweight=w,
                          key_len=np.full(n_keys, BIG, np.uint32), n_keys=n_keys)
    assert p.steps() == len(pos)
    return p, p.read()


def check(p, st, qkey, qs, qe, thr=THR, pos_lo=0, key_hi=None, skip=False, loop_span=0, ctx=None):
    """host mode and device mode against summarize_prefix (and summarize_loop on the regions of at most loop_span bases)"""
    qs, qe = np.asarray(qs, np.uint32), np.asarray(qe, np.uint32)
    qkey = None if qkey is None else np.asarray(qkey, np.uint32)
    want = dro.summarize_prefix(st, qkey, qs, qe, thr, pos_lo, key_hi, skip)
    if loop_span:
        m = np.flatnonzero(qe.astype(np.int64) - qs.astype(np.int64) < loop_span)
        sub = dro.summarize_loop(st, None if qkey is None else qkey[m], qs[m], qe[m], thr, pos_lo, key_hi, skip)
        same(sub, (want[0][m], want[1][m], want[2][:, m]))
    host = p.summarize(qkey, qs, qe, thr, pos_lo, key_hi, skip, ctx=ctx)
    same(host, want)
    cols = [dev_u32(a) for a in (qkey, qs, qe, key_hi)]
    dev = p.summarize(*cols[:3], thr, pos_lo, cols[3], skip, ctx=ctx)
    (ctx or p.ctx).synchronize()                            # a device-mode call may return with its kernels in flight
    same([d.cpu().numpy() for d in dev], want)
    return want


# ---------------------------------------------------------------------------------------------- tile edges
@pytest.fixture(scope="module")
def edges(ctx):
    """keys 0..5 with SIZES steps, key 6 without steps, key 7 with three steps; key 5 has a step at position 0"""
    rng = np.random.default_rng(11)
    keys, pos, w = [], [], []
    for k, S in enumerate(SIZES):
        first = 0 if k == 5 else 10 + k
        keys.append(np.full(S, k)); pos.append(first + 3 * np.arange(S))
        x = rng.integers(1, 4, S) * rng.choice([-1, 1], S)                 # negative weights too, never 0
        w.append(x)
    keys.append(np.full(3, 7)); pos.append(np.array([100, 200, 300])); w.append(np.array([2, -5, 3]))
    p, st = stepped(ctx, np.concatenate(keys), np.concatenate(pos), np.concatenate(w), 8)
    yield p, st
    p.free()


def edge_regions(st, k):
    """regions of key k around every tile boundary inside its slice of the step list"""
    g0 = int(np.searchsorted(st[0], k))
    pos = st[1][st[0] == k].astype(np.int64)
    S = len(pos)
    cand = {0, 1, S // 2, S - 2, S - 1}
    for b in range(g0 // T + 1, (g0 + S - 1) // T + 1):                   # global tile boundaries inside the key
        cand |= {b * T - g0 - 1, b * T - g0, b * T - g0 + 1}
    cand = sorted(c for c in cand if 0 <= c < S)
    qs, qe, far = [], [], 0
    for ia in cand:
        for ib in cand:
            if ib < ia:
                continue
            far = max(far, (g0 + ib) // T - (g0 + ia) // T)
            for ds in (-1, 0, 1):
                for de in (-1, 0, 1):
                    s, e = pos[ia] + ds, pos[ib] + de
                    if s >= 0:
                        qs.append(s); qe.append(e)                          # (e < s happens for ia == ib: an empty region)
    qs += [0, 0, 0, pos[-1] + 5, pos[-1], 0, pos[3] + 1, 500]
    qe += [max(pos[0] - 1, 0), 5, pos[0] + 4, pos[-1] + 1000, M32, M32, pos[3] + 1, 400]
    return np.array(qs, np.uint32), np.array(qe, np.uint32), far


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("k", range(len(SIZES)))
def test_tile_edges(edges, k, skip):
    p, st = edges
    qs, qe, far = edge_regions(st, k)
    assert far >= (3 if SIZES[k] > 3 * T else 1 if SIZES[k] > T else 0)
    check(p, st, np.full(len(qs), k, np.uint32), qs, qe, THR, 1 if skip else 0, None, skip, loop_span=300)


def test_key_without_steps_null_keys_and_no_key_column(edges):
    p, st = edges
    qs, qe = np.array([0, 5, 100, 250, 7, 0], np.uint32), np.array([M32, 4, 250, 250, 90, 50], np.uint32)
    w = check(p, st, [6, 6, 7, 7, NULL, NULL], qs, qe, THR, loop_span=300)
    assert w[0].tolist() == [1 << 32, 0, 151, 1, 0, 0] and w[1].tolist() == [0, 0, 2 * 100 - 3 * 51, -3, 0, 0]
    assert w[2][2].tolist() == [1 << 32, 0, 100, 0, 0, 0]                   # threshold 0: the zero stretches count
    check(p, st, None, qs, qe, THR, loop_span=300)                          # every region on key 0


def test_domain(edges):
    p, st = edges
    key_hi = np.array([50, 20000, 8, 9, 0, 3 * T, 77, 250], np.uint32)
    rng = np.random.default_rng(3)
    n = 400
    qkey = rng.integers(0, 8, n).astype(np.uint32)
    qs = rng.integers(0, 3 * T * 3 + 50, n).astype(np.uint32)
    qe = (qs + rng.integers(0, 3000, n)).astype(np.uint32)
    # pos_lo = 9: key 2's domain [9, 8] is empty; key 4's ends below pos_lo; key 7's cuts the open block at 250
    w = check(p, st, qkey, qs, qe, THR, 9, key_hi, False, loop_span=400)
    assert not w[0][(qkey == 2) | (qkey == 4)].any() and (w[0][qkey == 5] > 0).any()
    w = check(p, st, [7, 7, 7, 7], [100, 240, 251, 0], [M32, 260, 300, M32], THR, 1, key_hi, True, loop_span=400)
    assert w[0].tolist() == [151, 11, 0, 250]
    # the step at position 0 with pos_lo = 1 and skip_pos0: key 5's c0 is taken off everywhere, in the aggregates too
    c0 = int(st[2][st[0] == 5][0])
    assert c0 != 0
    a = check(p, st, [5], [1], [3 * T * 3], (1,), 1, None, True)
    b = check(p, st, [5], [1], [3 * T * 3], (1,), 1, None, False)
    assert a[1][0] == b[1][0] - c0 * 3 * T * 3


# ---------------------------------------------------------------------------------------------- many keys
def test_thousands_of_small_keys_around_a_long_one(ctx):
    rng = np.random.default_rng(21)
    nk, big = 3001, 1500
    keys, pos, w = [], [], []
    for k in range(nk):
        S = 3 * T + 5 if k == big else (0 if k % 7 == 3 else 1 + k % 2)
        keys.append(np.full(S, k)); pos.append(50 + 7 * np.arange(S) + k % 5); w.append(rng.integers(1, 5, S) * rng.choice([-1, 1], S))
    p, st = stepped(ctx, np.concatenate(keys), np.concatenate(pos), np.concatenate(w), nk)
    g0 = int(np.searchsorted(st[0], big))
    assert g0 % T not in (0, T - 1) and (g0 + 3 * T + 5) % T != 0          # the long key starts and ends inside a tile
    qkey = np.concatenate([np.arange(nk), np.arange(nk), np.full(6, big)]).astype(np.uint32)
    qs = np.concatenate([np.zeros(nk), 50 + np.arange(nk) % 9, [0, 50, 51, 60, 50 + 7 * T, 0]]).astype(np.uint32)
    qe = np.concatenate([np.full(nk, M32), 60 + np.arange(nk) % 4, [M32, 50 + 7 * (3 * T + 4), 50 + 7 * 3 * T, 70 + 7 * 2 * T, M32, 49]]).astype(np.uint32)
    check(p, st, qkey, qs, qe, THR, loop_span=100)
    p.free()


# ---------------------------------------------------------------------------------------------- counts, thresholds, outputs
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, WG - 1, WG, WG + 1])
def test_region_counts(edges, n):
    p, st = edges
    rng = np.random.default_rng(n)
    qkey = rng.integers(0, 8, n).astype(np.uint32)
    qs = rng.integers(0, 9000, n).astype(np.uint32)
    qe = (qs + rng.integers(0, 9000, n)).astype(np.uint32)
    check(p, st, qkey, qs, qe, THR)


def test_threshold_counts_and_null_outputs(edges):
    p, st = edges
    qkey, qs, qe = np.array([0, 5, 7, 6], np.uint32), np.array([0, 20, 150, 3], np.uint32), np.array([M32, 9000, 350, 9], np.uint32)
    w0 = check(p, st, qkey, qs, qe, ())
    assert w0[2].shape == (0, 4)
    w8 = check(p, st, qkey, qs, qe, THR8, loop_span=300)
    assert w8[2].shape == (8, 4) and np.array_equal(w8[2][0], w8[0]) and not w8[2][7].any()
    with pytest.raises(pyivx.IvxError) as ei:
        p.summarize(qkey, qs, qe, THR8 + (7,))
    assert ei.value.status == pyivx.ERR_INVALID
    for mask in ((True, False, False), (False, True, False), (False, False, True), (False, True, True), (True, True, False)):
        for dev in (False, True):
            a = (dev_u32(qkey), dev_u32(qs), dev_u32(qe)) if dev else (qkey, qs, qe)
            got = p.summarize(*a, THR8, outputs=mask)
            p.ctx.synchronize()
            for g, w, m in zip(got, w8, mask):
                assert (g is None) == (not m)
                if m:
                    assert np.array_equal(g.cpu().numpy() if dev else g, w)


def test_int32_max_over_the_whole_position_range(ctx):
    p, st = stepped(ctx, [0], [0], [I32_MAX], 1)
    w = check(p, st, [0, 0], [0, 1], [M32, M32], THR)
    assert w[0].tolist() == [1 << 32, M32] and w[1][0] == I32_MAX << 32 and w[2][4][0] == 1 << 32
    p.free()
    p, st = stepped(ctx, [0, 0], [0, 5], [I32_MIN, I32_MAX], 1)             # -2^31 * 5, then -1 to the end
    w = check(p, st, [0], [0], [M32], THR)
    assert w[1][0] == I32_MIN * 5 - ((1 << 32) - 5) and w[2][0][0] == 1 << 32
    p.free()


def test_empty_profile(ctx):
    p = ctx.depth_profile(n_keys=3)
    assert p.steps() == 0
    st = p.read()
    w = check(p, st, [0, 2, NULL, 1], [0, 7, 1, 9], [M32, 9, 5, 8], THR)
    assert w[0].tolist() == [1 << 32, 3, 0, 0] and not w[1].any() and w[2][2].tolist() == [1 << 32, 3, 0, 0]
    for dev in (False, True):
        got = p.windows(1, 10, 30, 8, device=dev, thresholds=(0, 1))
        p.ctx.synchronize()
        got = [g.cpu().numpy() if dev else g for g in got]
        assert got[0].tolist() == [8, 8, 5] and not got[1].any() and got[2].tolist() == [[8, 8, 5], [0, 0, 0]]
    p.free()


# ---------------------------------------------------------------------------------------------- errors
def raw(ctx, p, mem, qkey, qs, qe, n, thr, outs, pos_lo=0, key_hi=None):
    t = np.asarray(thr, np.int32)
    return pyivx.lib().ivx_depth_profile_summarize(ctx.h, p.h, mem, qkey, qs, qe, n, pos_lo, key_hi, 0, pyivx._ptr(t), len(t), *outs)


def test_bad_key_leaves_the_outputs_untouched(ctx, edges):
    import torch
    p, _ = edges
    n = 70
    qkey = np.zeros(n, np.uint32)
    qkey[66] = 8                                                            # n_keys = 8
    qs, qe = np.zeros(n, np.uint32), np.full(n, 100, np.uint32)
    outs = [np.full(n, -7, np.int64), np.full(n, -7, np.int64), np.full(2 * n, -7, np.int64)]
    st = raw(ctx, p, pyivx.MEM_HOST, *[pyivx._ptr(a) for a in (qkey, qs, qe)], n, (0, 1), [pyivx._ptr(o) for o in outs])
    assert st == pyivx.ERR_INVALID and b"key id >= n_keys" in pyivx.lib().ivx_last_error(ctx.h)
    assert all((o == -7).all() for o in outs)
    douts = [torch.full((len(o),), -7, dtype=torch.int64, device="cuda") for o in outs]
    st = raw(ctx, p, pyivx.MEM_DEVICE, *[pyivx._ptr(dev_u32(a)) for a in (qkey, qs, qe)], n, (0, 1), [pyivx._ptr(o) for o in douts])
    assert st == pyivx.ERR_INVALID
    ctx.synchronize()
    assert all(bool((o == -7).all()) for o in douts)
    qkey[66] = NULL                                                         # the skip mark is no error
    assert raw(ctx, p, pyivx.MEM_HOST, *[pyivx._ptr(a) for a in (qkey, qs, qe)], n, (0, 1), [pyivx._ptr(o) for o in outs]) == pyivx.OK
    assert outs[0][66] == 0 and outs[0][0] == 101


def test_misaligned_device_pointers_and_other_indexes(ctx, edges):
    import torch
    p, _ = edges
    n = 8
    buf = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    al = lambda off: C.c_void_p(buf.data_ptr() + off)
    ok = [al(0), al(512), al(1024)]
    outs = [al(2048), al(2560), None]
    assert raw(ctx, p, pyivx.MEM_DEVICE, *ok, n, (), outs) == pyivx.OK
    for i in range(3):
        bad = list(ok)
        bad[i] = al(512 * i + 2)
        assert raw(ctx, p, pyivx.MEM_DEVICE, *bad, n, (), outs) == pyivx.ERR_INVALID
    for i in range(2):
        bad = list(outs)
        bad[i] = al(2048 + 512 * i + 4)
        assert raw(ctx, p, pyivx.MEM_DEVICE, *ok, n, (), bad) == pyivx.ERR_INVALID
    assert raw(ctx, p, pyivx.MEM_DEVICE, *ok, n, (1,), [None, None, al(3072 + 4)]) == pyivx.ERR_INVALID
    assert raw(ctx, p, pyivx.MEM_DEVICE, *ok, n, (), outs, key_hi=al(3072 + 2)) == pyivx.ERR_INVALID
    ctx.synchronize()
    # any index that is not a profile
    ix = ctx.build(pyivx.KIND_COUNT, np.zeros(4, np.uint32), np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32) + 5)
    z = np.zeros(1, np.uint32)
    o = np.zeros(1, np.int64)
    L = pyivx.lib()
    assert L.ivx_depth_profile_summarize(ctx.h, ix.h, pyivx.MEM_HOST, None, pyivx._ptr(z), pyivx._ptr(z), 1, 0, None, 0, None, 0,
                                         pyivx._ptr(o), None, None) == pyivx.ERR_UNSUPPORTED
    assert L.ivx_depth_profile_windows(ctx.h, ix.h, pyivx.MEM_HOST, 0, 0, 10, 5, 2, 0, None, 0, pyivx._ptr(o), None, None) == pyivx.ERR_UNSUPPORTED
    ix.free()


def test_from_another_context(edges):
    p, st = edges
    other = pyivx.Ctx(0)
    check(p, st, [5, 0, 7], [0, 100, 0], [M32, 5000, 400], THR, ctx=other)
    other.close()


# ---------------------------------------------------------------------------------------------- windows
def check_windows(p, st, key, first, last, width, n=None, thr=(1, 3), skip=False):
    host = p.windows(key, first, last, width, n, thr, skip)
    nn = len(host[0])
    qs, qe = dro.windows_as_regions(first, last, width, nn)
    want = dro.summarize_prefix(st, np.full(nn, key, np.uint32), qs, qe, thr, 0, None, skip)
    same(host, want)
    dev = p.windows(key, first, last, width, n, thr, skip, device=True)
    p.ctx.synchronize()
    same([d.cpu().numpy() for d in dev], want)
    return want


def test_windows(edges):
    p, st = edges
    w = check_windows(p, st, 5, 0, 3 * (3 * T + 1) + 40, 1000)             # the last window is cut
    assert w[0][-1] == (3 * (3 * T + 1) + 41) % 1000 and len(w[0]) == (3 * (3 * T + 1) + 40) // 1000 + 1
    check_windows(p, st, 5, 1, 9000, 977, skip=True)
    check_windows(p, st, 0, 5, 4000, 64, n=70)                              # more windows than cover the span: empty ones
    check_windows(p, st, 6, 0, 100, 7)
    check_windows(p, st, 3, 50, 40, 10, n=3)                                # last_pos < first_pos: all empty
    check_windows(p, st, 7, M32 - 10, M32, 4, n=3)
    with pytest.raises(pyivx.IvxError) as ei:
        p.windows(7, M32 - 10, M32, 4, n=4)                                 # first_pos + 3 * 4 > 2^32 - 1
    assert ei.value.status == pyivx.ERR_INVALID
    for bad in (dict(key=8, width=5), dict(key=0, width=0)):
        with pytest.raises(pyivx.IvxError) as ei:
            p.windows(bad["key"], 0, 100, bad["width"], n=2)
        assert ei.value.status == pyivx.ERR_INVALID


@pytest.mark.parametrize("skip", [False, True])
def test_width_one_is_expand_in_int32(edges, skip):
    p, st = edges
    for key, first, n in ((5, 0, 2 * T + 77), (0, 3, 500), (7, 90, 300), (6, 0, 40)):
        _, cov = p.expand(key, first, n, skip_pos0=skip, want_pos=False)
        w = check_windows(p, st, key, first, first + n - 1, 1, thr=(1,), skip=skip)
        v = dro.values(st, key, first, n, skip)
        assert np.abs(v).max() <= 32767                                     # inside Int16: the two calls must agree
        assert np.array_equal(w[1], cov.astype(np.int64)) and np.array_equal(w[2][0], (cov >= 1).astype(np.int64))
        assert (w[0] == 1).all()


# ---------------------------------------------------------------------------------------------- merged profiles
def test_merged_profile_summarises_like_the_one_shot_profile(ctx):
    rng = np.random.default_rng(8)

    def weighted(n):
        s = rng.integers(0, 20000, n).astype(np.uint32)
        return dict(skey=rng.integers(0, 3, n).astype(np.uint32), sstart=s, send=(s + rng.integers(0, 300, n)).astype(np.uint32),
                    sweight=rng.integers(-4, 5, n).astype(np.int32), n_keys=3)
    x, y = weighted(4000), weighted(4000)
    a, b = ctx.depth_profile(**x), ctx.depth_profile(**y)
    m = a.merge(b)
    both = {k: np.concatenate([x[k], y[k]]) for k in ("skey", "sstart", "send", "sweight")}
    one = ctx.depth_profile(n_keys=3, **both)
    assert m.steps() == one.steps() > 3 * T
    n = 500
    qkey = rng.integers(0, 3, n).astype(np.uint32)
    qs = rng.integers(0, 21000, n).astype(np.uint32)
    qe = (qs + rng.integers(0, 21000, n) * rng.integers(0, 2, n)).astype(np.uint32)
    want = check(m, m.read(), qkey, qs, qe, THR8, loop_span=200)
    same(one.summarize(qkey, qs, qe, THR8), want)
    for p in (a, b, m, one):
        p.free()
