"""-m gpu: depth coverage classes on the device (ivx_depth_profile_quantize / ivx_depth_profile_hist,
csrc/ivx_depth_classes.hip), bit-exact against the vectorised restatements of tests/depth_classes_oracle.py, in host and in
device memory mode.

Profiles are made from weighted segments whose end event is clipped away, one step per segment, so that step counts are
exact; from_cov() gives every step the coverage the test wants.  With T = pyivx.DEPTH_CLASS_TILE steps per tile of both
passes and B = pyivx.DEPTH_HIST_LDS_BINS bins in LDS, the shapes sit where the kernels can go wrong: keys of T - 1, T, T + 1
and 2T + 1 steps laid one after another (so the tiles straddle the key changes), a run whose head ends one tile and whose
tail starts the next, a run over more than three tiles, a run per step, the zero stretch joining the first step's run or
not, domains cut one below, on and one above a step, keys without steps, thousands of one-step keys around a long one, an
empty profile; bins of 1, 2, B, B + 1 and 65536.  The file carries the entry-layer checks of its two entries itself: a
second context, poisoned scratch, and a call between a subtract sizing call and its fill."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, synth
from oracle import oracle as orc

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_classes_oracle as dco  # noqa: E402
import pyivx  # noqa: E402

pytestmark = pytest.mark.gpu

T = pyivx.DEPTH_CLASS_TILE
B = pyivx.DEPTH_HIST_LDS_BINS
M32 = 0xFFFFFFFF
BIG = 1 << 31                   # a key length no test position reaches, below 2^32 - 1: a segment's end event is clipped
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
SIZES = (T - 1, T, T + 1, 2 * T + 1)
CUTS31 = tuple(range(-15, 16))
L = pyivx.lib


@pytest.fixture(scope="module")
def ctx():
    c = pyivx.Ctx(0)
    yield c
    c.close()


def dev_u32(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def stepped(ctx, keys, pos, w, n_keys):
    """one step per (key, position, weight != 0) -> (profile, its steps as the oracle takes them)"""
    keys, pos, w = np.asarray(keys, np.uint32), np.asarray(pos, np.uint32), np.asarray(w, np.int32)
    p = ctx.depth_profile(skey=keys, sstart=pos, send=np.full(len(pos), M32, np.uint32), sweight=w,
                          key_len=np.full(n_keys, BIG, np.uint32), n_keys=n_keys)
    assert p.steps() == len(pos)
    return p, p.read()


def from_cov(ctx, keys, pos, cov, n_keys):
    """steps with the given coverage (per key ascending positions; cov differs from the step before, the first from 0)"""
    keys, cov = np.asarray(keys, np.int64), np.asarray(cov, np.int64)
    first = np.concatenate([[True], keys[1:] != keys[:-1]])
    w = cov - np.where(first, 0, np.concatenate([[0], cov[:-1]]))
    assert (w != 0).all()
    p, st = stepped(ctx, keys, pos, w, n_keys)
    assert np.array_equal(st[2], cov)
    return p, st


def same_rows(got, want):
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g.dtype == np.uint32 and g.shape == w.shape and np.array_equal(g, w)


def check_q(p, st, cuts, emit=None, pos_lo=0, key_hi=None, skip=False, seen_only=False, ctx=None):
    """quantize in host mode and in device mode against quantize_steps"""
    key_hi = None if key_hi is None else np.asarray(key_hi, np.uint32)
    want = dco.quantize_steps(st, cuts, emit, pos_lo, key_hi, skip, seen_only)
    same_rows(p.quantize(cuts, emit, pos_lo, key_hi, skip, seen_only, ctx=ctx), want)
    dev = p.quantize(cuts, emit, pos_lo, dev_u32(key_hi), skip, seen_only, device=True, ctx=ctx)
    (ctx or p.ctx).synchronize()                            # a device-mode call may return with its kernels in flight
    same_rows([host_u32(d) for d in dev], want)
    return want


def check_h(p, st, v_lo=0, n_bins=256, pos_lo=0, key_hi=None, skip=False, seen_only=False, ctx=None):
    """hist in host mode and in device mode against hist_steps; the rows add up to the domains"""
    key_hi = None if key_hi is None else np.asarray(key_hi, np.uint32)
    want = dco.hist_steps(st, v_lo, n_bins, pos_lo, key_hi, skip, seen_only)
    assert np.array_equal(want.sum(axis=1), dco.domain_sizes(st, pos_lo, key_hi, seen_only))
    host = p.hist(v_lo, n_bins, pos_lo, key_hi, skip, seen_only, ctx=ctx)
    assert host.dtype == np.int64 and host.shape == want.shape and np.array_equal(host, want)
    dev = p.hist(v_lo, n_bins, pos_lo, dev_u32(key_hi), skip, seen_only, device=True, ctx=ctx)
    (ctx or p.ctx).synchronize()
    dev = dev.cpu().numpy()
    assert dev.dtype == np.int64 and dev.shape == want.shape and np.array_equal(dev, want)
    return want


# ---------------------------------------------------------------------------------------------- tile edges
@pytest.fixture(scope="module")
def edges(ctx):
    """keys 0..3 with SIZES steps, key 4 without steps, key 5 with three steps; key 3 has a step at position 0 and weights in
    the hundreds, the others small ones of both signs"""
    rng = np.random.default_rng(17)
    keys, pos, w = [], [], []
    for k, S in enumerate(SIZES):
        first = 0 if k == 3 else 10 + k
        keys.append(np.full(S, k)); pos.append(first + 3 * np.arange(S))
        w.append(rng.integers(1, 300 if k == 3 else 4, S) * rng.choice([-1, 1], S))
    keys.append(np.full(3, 5)); pos.append(np.array([100, 200, 300])); w.append(np.array([2, -5, 3]))
    p, st = stepped(ctx, np.concatenate(keys), np.concatenate(pos), np.concatenate(w), 6)
    yield p, st
    p.free()


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("cuts", [(), (1,), (-2, 0, 1, 3), (0, 1, 4, 100, 200), CUTS31, (I32_MIN, I32_MAX)], ids=lambda c: f"cuts{len(c)}")
def test_quantize_tile_edges(edges, cuts, skip):
    p, st = edges
    w = check_q(p, st, cuts, None, 1 if skip else 0, None, skip)
    assert set(w[0].tolist()) == set(range(6))              # key 4 has no steps: one run over its whole domain
    k4 = w[0] == 4
    assert k4.sum() == 1 and w[2][k4][0] == M32
    check_q(p, st, cuts, None, 0, None, skip)               # a step at position 0 inside the domain, with and without c0


def test_quantize_head_ends_a_tile_and_tail_starts_the_next(ctx):
    n = 2 * T + 7
    for at in (T - 1, T, 2 * T - 1):                        # the run of class 1 is steps at, at + 1
        cov = np.where(np.arange(n) % 2 == 0, 1, 2)
        cov[at], cov[at + 1] = 10, 11
        p, st = from_cov(ctx, np.zeros(n), 5 + 2 * np.arange(n), cov, 1)
        w = check_q(p, st, (5,))
        assert w[3].tolist() == [0, 1, 0] and w[1][1] == 5 + 2 * at and w[2][1] == 5 + 2 * (at + 2) - 1
        assert len(check_q(p, st, (5,), 0b10)[0]) == 1
        p.free()


def test_quantize_one_run_over_more_than_three_tiles_and_a_run_per_step(ctx):
    n = 3 * T + 100
    pos = 7 + 3 * np.arange(n)
    p, st = from_cov(ctx, np.zeros(n), pos, np.where(np.arange(n) % 2 == 0, 1, 2), 1)
    w = check_q(p, st, (1,))                                # the zero stretch, then every step in class 1
    assert w[1].tolist() == [0, 7] and w[2].tolist() == [6, M32] and w[3].tolist() == [0, 1]
    w = check_q(p, st, (5,))                                # ... and the zero stretch joins them
    assert w[1].tolist() == [0] and w[2].tolist() == [M32]
    w = check_q(p, st, (2,))                                # alternating classes: a run per step, the first with the zero stretch
    assert len(w[0]) == n and w[1][0] == 0 and w[1][1] == pos[1]
    w = check_q(p, st, (2,), 0b10, key_hi=[int(pos[-1])])   # the emitted half; the last step is one base long
    assert len(w[0]) == n // 2 and w[2][-1] == pos[-1]
    p.free()


def test_quantize_zero_stretch_and_position_zero(ctx):
    p, st = from_cov(ctx, [0, 0, 0, 1, 1], [0, 10, 20, 4, 9], [3, 1, 4, 2, 5], 2)
    for skip in (False, True):
        for pos_lo in (0, 1):
            for cuts in ((1,), (2,), (3,), (-1, 0), (-2, 2, 4)):
                check_q(p, st, cuts, None, pos_lo, None, skip)
                check_h(p, st, -3, 9, pos_lo, None, skip)
    w = check_q(p, st, (3,))                                # key 1: [0, 3] is 0 and joins the step at 4 (2 < 3)
    assert w[1][w[0] == 1].tolist() == [0, 9]
    w = check_q(p, st, (2,))                                # ... and does not (2 >= 2)
    assert w[1][w[0] == 1].tolist() == [0, 4]
    p.free()


def test_domain_cut_one_below_on_and_one_above_a_step(edges):
    p, st = edges
    for lo in (99, 100, 101, 199, 200, 201, 300, 301):
        check_q(p, st, (0, 1), None, lo)
        check_h(p, st, -4, 8, lo)
    for hi in (98, 99, 100, 101, 199, 200, 201, 299, 300, 301):
        key_hi = [hi, hi + 1, hi - 1, hi, hi, hi]
        w = check_q(p, st, (0, 1), None, 12, key_hi)
        check_h(p, st, -4, 8, 12, key_hi)
        assert w[2][w[0] == 5][-1] == hi
    key_hi = [5000, 8, 9, 10, 3, 250]                       # pos_lo = 9: key 1's domain [9, 8] is empty, key 2's one base, key 4's below
    w = check_q(p, st, (-1, 1), None, 9, key_hi)
    assert 1 not in w[0] and 4 not in w[0] and w[1][w[0] == 2].tolist() == [9]
    h = check_h(p, st, -2, 5, 9, key_hi)
    assert not h[1].any() and not h[4].any() and h[2].sum() == 1


def test_keys_without_steps_before_between_and_after(ctx):
    p, st = from_cov(ctx, [2, 2, 3, 6], [5, 9, 0, 7], [1, 4, 2, -1], 9)
    for cuts, emit in (((0,), None), ((0,), 0b10), ((0,), 0b01), ((1, 3), None), ((1, 3), 0b101)):
        check_q(p, st, cuts, emit)
        check_q(p, st, cuts, emit, 3, np.arange(9) + 1)     # key_hi[k] = k + 1: keys 0 and 1 end below pos_lo = 3
    assert check_q(p, st, (0,))[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 6, 7, 8]
    h = check_h(p, st, -1, 6)
    assert h[0].tolist() == [0, 1 << 32, 0, 0, 0, 0]
    check_h(p, st, 0, 3, 3, np.arange(9) + 1)
    p.free()


@pytest.fixture(scope="module")
def small_around_long(ctx):
    """1500 one-step keys, one key of 2T + 5 steps, 1500 one-step keys more"""
    rng = np.random.default_rng(4)
    nk, S = 3001, 2 * T + 5
    keys = np.concatenate([np.arange(1500), np.full(S, 1500), np.arange(1501, nk)])
    pos = np.concatenate([rng.integers(0, 50, 1500), 3 + 2 * np.arange(S), rng.integers(0, 50, 1500)])
    cov = np.concatenate([rng.integers(1, 6, 1500), np.where(np.arange(S) % 3 == 0, 2, np.where(np.arange(S) % 3 == 1, 7, 4)),
                          -rng.integers(1, 6, 1500)])
    p, st = from_cov(ctx, keys, pos, cov, nk)
    yield p, st
    p.free()


def test_thousands_of_one_step_keys_around_a_long_one(small_around_long):
    p, st = small_around_long
    check_q(p, st, (3,))
    check_q(p, st, (-2, 3, 5), 0b1010, 1, np.full(3001, 40, np.uint32), True)
    check_h(p, st, -3, 12)                                  # tiles of hundreds of keys add to memory directly
    check_h(p, st, 0, 4, 2, np.full(3001, 45, np.uint32))


def test_seen_only(ctx):
    """key 1's events cancel: seen, no steps.  Key 2 has steps.  Keys 0 and 3 kept no event."""
    keys, pos, w = [1, 1, 2, 2], [50, 50, 10, 30], [1, -1, 2, 3]
    p = ctx.depth_profile(skey=np.asarray(keys, np.uint32), sstart=np.asarray(pos, np.uint32), send=np.full(4, M32, np.uint32),
                          sweight=np.asarray(w, np.int32), key_len=np.full(4, BIG, np.uint32), n_keys=4)
    st = p.read()
    assert p.steps() == 2 and st[3].tolist() == [0, 1, 1, 0]
    assert check_q(p, st, (1,), seen_only=True)[0].tolist() == [1, 2, 2]
    assert check_q(p, st, (1,), seen_only=False)[0].tolist() == [0, 1, 2, 2, 3]
    assert check_h(p, st, 0, 3, seen_only=True).sum(axis=1).tolist() == [0, 1 << 32, 1 << 32, 0]
    check_h(p, st, 0, 3, seen_only=False)
    p.free()


def test_every_emit_mask_of_two_cuts_no_cut_and_31_cuts(edges):
    p, st = edges
    for mask in range(8):
        check_q(p, st, (-1, 2), mask, 1, None, True)
    assert len(check_q(p, st, (), 0)[0]) == 0
    assert len(check_q(p, st, (), 1)[0]) == 6               # no cut: one run per key
    w = check_q(p, st, CUTS31, 0xFFFFFFFF)
    assert w[3].max() == 31 and w[3].min() == 0
    check_q(p, st, CUTS31, 0x80000001)


def test_empty_profile(ctx):
    p = ctx.depth_profile(n_keys=3)
    assert p.steps() == 0
    st = p.read()
    w = check_q(p, st, (0,), None, 4, [9, 3, 4])
    assert [a.tolist() for a in w] == [[0, 2], [4, 4], [9, 4], [1, 1]]
    assert len(check_q(p, st, (0,), seen_only=True)[0]) == 0
    h = check_h(p, st, -1, 3, 4, [9, 3, 4])
    assert h.tolist() == [[0, 6, 0], [0, 0, 0], [0, 1, 0]]
    assert not check_h(p, st, seen_only=True).any()
    p.free()


# ---------------------------------------------------------------------------------------------- capacity and errors
def raw_q(ctx, p, mem, cuts, mask, outs, cap, key_hi=None, pos_lo=0):
    c = np.asarray(cuts, np.int32)
    m = C.c_uint64(12345)
    st = L().ivx_depth_profile_quantize(ctx.h, p.h, mem, pos_lo, key_hi, 0, 0, pyivx._ptr(c) if len(c) else None, len(c), mask, *outs, cap, C.byref(m))
    return st, m.value


def test_quantize_capacity_protocol(ctx, edges):
    import torch
    p, st = edges
    cuts = tuple(range(-30, 32, 2))
    want = dco.quantize_steps(st, cuts)
    n = len(want[0])
    assert n > T
    assert raw_q(ctx, p, pyivx.MEM_HOST, cuts, M32, [None] * 4, 0) == (pyivx.OK, n)             # count only
    assert raw_q(ctx, p, pyivx.MEM_DEVICE, cuts, M32, [None] * 4, 0) == (pyivx.OK, n)
    outs = [np.full(n, 77, np.uint32) for _ in range(4)]
    assert raw_q(ctx, p, pyivx.MEM_HOST, cuts, M32, [pyivx._ptr(o) for o in outs], n) == (pyivx.OK, n)      # exact cap
    same_rows(outs, want)
    outs = [np.full(n, 77, np.uint32) for _ in range(4)]
    assert raw_q(ctx, p, pyivx.MEM_HOST, cuts, M32, [pyivx._ptr(o) for o in outs], n - 1) == (pyivx.ERR_CAPACITY, n)
    assert all((o == 77).all() for o in outs)
    douts = [torch.full((n,), 77, dtype=torch.int32, device="cuda") for _ in range(4)]
    assert raw_q(ctx, p, pyivx.MEM_DEVICE, cuts, M32, [pyivx._ptr(o) for o in douts], n - 1) == (pyivx.ERR_CAPACITY, n)
    ctx.synchronize()
    assert all(bool((o == 77).all()) for o in douts)
    with pytest.raises(pyivx.IvxError) as ei:
        p.quantize(cuts, cap=n - 1)
    assert ei.value.status == pyivx.ERR_CAPACITY
    for j in range(4):                                      # each output alone
        for dev in (False, True):
            flags = tuple(i == j for i in range(4))
            got = p.quantize(cuts, device=dev, outputs=flags)
            ctx.synchronize()
            assert all((g is None) == (i != j) for i, g in enumerate(got))
            g = host_u32(got[j]) if dev else got[j]
            assert np.array_equal(g, want[j])
    assert raw_q(ctx, p, pyivx.MEM_HOST, cuts, M32, [None] * 4, n) == (pyivx.OK, n)             # a cap and no output: the count


def test_argument_errors(ctx, edges):
    import torch
    p, _ = edges
    none = [None] * 4
    H, D = pyivx.MEM_HOST, pyivx.MEM_DEVICE
    assert raw_q(ctx, p, H, tuple(range(32)), 1, none, 0)[0] == pyivx.ERR_INVALID
    assert raw_q(ctx, p, H, tuple(range(31)), 0xFFFFFFFF, none, 0)[0] == pyivx.OK
    assert raw_q(ctx, p, H, (1, 1), 1, none, 0)[0] == pyivx.ERR_INVALID
    assert raw_q(ctx, p, H, (2, 1), 1, none, 0)[0] == pyivx.ERR_INVALID
    assert raw_q(ctx, p, H, (1, 2), 0b1000, none, 0)[0] == pyivx.ERR_INVALID
    assert raw_q(ctx, p, H, (), 0b10, none, 0)[0] == pyivx.ERR_INVALID
    assert raw_q(ctx, p, H, (1, 2), 0b111, none, 0)[0] == pyivx.OK
    assert L().ivx_depth_profile_quantize(ctx.h, p.h, H, 0, None, 0, 0, None, 0, 1, *none, 0, None) == pyivx.ERR_INVALID      # null n_out
    assert raw_q(ctx, p, 7, (), 1, none, 0)[0] == pyivx.ERR_INVALID
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    al = lambda off: C.c_void_p(buf.data_ptr() + off)
    n = raw_q(ctx, p, D, (), 1, none, 0)[1]
    assert n == 6
    good = [al(0), al(256), al(512), al(768)]
    assert raw_q(ctx, p, D, (), 1, good, 8)[0] == pyivx.OK
    for i in range(4):
        bad = list(good)
        bad[i] = al(256 * i + 2)
        assert raw_q(ctx, p, D, (), 1, bad, 8)[0] == pyivx.ERR_INVALID
    assert raw_q(ctx, p, D, (), 1, good, 8, key_hi=al(1024 + 1))[0] == pyivx.ERR_INVALID
    hist = lambda prof, mem, n_bins, out, key_hi=None: L().ivx_depth_profile_hist(ctx.h, prof.h, mem, 0, key_hi, 0, 0, 0, n_bins, out)
    o = np.zeros(6 * 4, np.int64)
    assert hist(p, H, 4, pyivx._ptr(o)) == pyivx.OK and o.sum() == 6 << 32
    assert hist(p, H, 0, pyivx._ptr(o)) == pyivx.ERR_INVALID
    assert hist(p, H, pyivx.DEPTH_MAX_BINS + 1, pyivx._ptr(o)) == pyivx.ERR_INVALID
    assert hist(p, D, 4, al(2048)) == pyivx.OK
    assert hist(p, D, 4, al(2048 + 4)) == pyivx.ERR_INVALID
    assert hist(p, D, 4, al(2048), key_hi=al(4096 + 2)) == pyivx.ERR_INVALID
    ctx.synchronize()
    ix = ctx.build(pyivx.KIND_COUNT, np.zeros(4, np.uint32), np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32) + 5)
    assert raw_q(ctx, ix, H, (), 1, none, 0)[0] == pyivx.ERR_UNSUPPORTED
    assert hist(ix, H, 4, pyivx._ptr(o)) == pyivx.ERR_UNSUPPORTED
    ix.free()


# ---------------------------------------------------------------------------------------------- hist
@pytest.mark.parametrize("n_bins", [1, 2, B, B + 1, pyivx.DEPTH_MAX_BINS])
def test_hist_bins(edges, n_bins):
    p, st = edges
    lo, hi = int(st[2].min()), int(st[2].max())
    if n_bins < pyivx.DEPTH_MAX_BINS:                       # both clamped ends hit: key 3 spreads over more values than the LDS holds
        assert hi - lo > B + 200
        h = check_h(p, st, lo + 100, n_bins)
        assert h[3][0] > 0 and h[3][-1] > 0
        check_h(p, st, lo + 50, n_bins, 1, None, True)
    else:                                                   # ... and not hit
        assert lo > -(n_bins // 2) and hi < n_bins // 2 - 1
        h = check_h(p, st, -(n_bins // 2), n_bins)
        assert not h[:, 0].any() and not h[:, -1].any()


def test_hist_every_step_in_one_bin(ctx):
    n = 3 * T
    p, st = from_cov(ctx, np.zeros(n), 2 * np.arange(n), np.where(np.arange(n) % 2 == 0, 7, 8), 1)
    h = check_h(p, st, 0, 4, 0, [2 * n + 10])               # all of it in the clamped last bin; the last step ends at key_hi
    assert h.tolist() == [[0, 0, 0, 2 * n + 11]]
    h = check_h(p, st, 7, 2)                                # two bins; the last step reaches 2^32 - 1
    assert h[0].tolist() == [n, (1 << 32) - n]
    check_h(p, st, 7, B + 1)                                # the same steps straight to memory
    check_h(p, st, -5, 1)
    p.free()


def test_hist_negative_v_lo_and_small_keys_between_tiles(edges, small_around_long):
    p, st = edges
    check_h(p, st, -7, 16)
    check_h(p, st, -300, 512, 20, [3000, 3001, 2999, 5000, 7, 250])
    p, st = small_around_long
    check_h(p, st, -6, 14, 0, np.full(3001, 4000, np.uint32))


# ---------------------------------------------------------------------------------------------- the entry layer
def test_from_another_context(edges):
    p, st = edges
    other = pyivx.Ctx(0)
    check_q(p, st, (-2, 0, 1, 3), 0b10101, 1, None, True, ctx=other)
    check_h(p, st, -50, 100, ctx=other)
    other.close()


@pytest.mark.parametrize("word", [0, 1])
def test_on_poisoned_scratch(ctx, edges, small_around_long, word):
    what = pyivx.POISON_SCRATCH | pyivx.POISON_SCALARS | pyivx.POISON_DROP_PLANS | pyivx.POISON_PINNED
    for p, st in (edges, small_around_long):
        check_q(p, st, (0, 2))                              # (the scratch exists)
        for dev in (False, True):
            ctx.synchronize()
            assert ctx.debug_poison(word, what) != 0
            want = dco.quantize_steps(st, (0, 2), 0b101)
            got = p.quantize((0, 2), 0b101, device=dev)
            ctx.synchronize()
            same_rows([host_u32(g) for g in got] if dev else got, want)
            ctx.synchronize()
            assert ctx.debug_poison(word, what) != 0
            got = p.hist(-3, 9, device=dev)
            ctx.synchronize()
            assert np.array_equal(got.cpu().numpy() if dev else got, dco.hist_steps(st, -3, 9))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("entry", ["quantize", "hist"])
def test_between_a_subtract_sizing_call_and_its_fill(ctx, edges, entry, dev):
    """the call drops the plan the sizing call left, and the fill still gives the right fragments"""
    p, st = edges
    l = synth(50_000, 51, nkeys=5, mean_len=400, span=3_000_000, dtype=np.int64)
    r = synth(70_000, 52, nkeys=5, mean_len=150, span=3_000_000, dtype=np.int64)
    want = orc.subtract(*l, *r)
    seen = {}

    def between():
        assert ctx.debug_state()["sub_valid"] == 1
        if entry == "quantize":
            got = p.quantize((0, 2), device=dev)
            ctx.synchronize()
            same_rows([host_u32(g) for g in got] if dev else got, dco.quantize_steps(st, (0, 2)))
        else:
            got = p.hist(-3, 9, device=dev)
            ctx.synchronize()
            assert np.array_equal(got.cpu().numpy() if dev else got, dco.hist_steps(st, -3, 9))
        seen.update(ctx.debug_state())

    got = ctx.subtract(*l, *r, n_keys=5, between=between)
    assert seen["sub_valid"] == 0
    for g, w in zip(got, want):
        assert len(g) == len(w) and g.dtype == w.dtype and (g == w).all()
