"""The catalogue of the C entry layer (csrc/ivx_capi.hip), shared by the tests that walk every entry: CASES maps an entry's name
to f(E, M, n) -> dict of all its outputs, the scalar ones included, on a small seeded input of n rows -- E an Env (one context,
one index of every kind, two depth profiles), M a Mode (host arrays or device tensors).  The entries are called through
pyivx.lib() with ctypes directly: pyivx's wrappers would allocate, retry or reject first.  Importing this needs no GPU.

A third mode, LateMode, is device mode with every column still in flight on the context's stream when the entry is invoked
(tests/test_gpu_entry_stream_order.py; DESIGN.md, "What a device-mode call may assume of its stream")."""
import contextlib
import ctypes as C
import math
import os
import sys
import time
import weakref

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402
import cigar_text_oracle as cto  # noqa: E402

OK, INVALID, CAPACITY, UNSUPPORTED, OOM = pyivx.OK, pyivx.ERR_INVALID, pyivx.ERR_CAPACITY, pyivx.ERR_UNSUPPORTED, pyivx.ERR_OOM
NULL = pyivx.NULL_IDX
NK = 3                      # keys
SIZES = [1000, 0, 1]
PATTERN = 0xA5              # what every output buffer holds before a call
u32, u64, i64, cint = C.c_uint32, C.c_uint64, C.c_int64, C.c_int
_SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}


class Buf:
    """an array in one memory mode: numpy on the host, a torch tensor on the device (unsigned types as their signed bits);
    never empty, so that its pointer is never null (the element count goes to the entry separately)"""

    def __init__(self, a, dev):
        a = np.ascontiguousarray(a)
        self.dt, self.n = a.dtype, a.size
        if a.size == 0:
            a = np.zeros(1, a.dtype)
        if dev:
            import torch
            self.h = torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype)).copy()).to("cuda:0")
        else:
            self.h = a.copy()

    @property
    def p(self):
        return pyivx._ptr(self.h)

    clone = None                # LateMode: what a consumer queued right behind the last call saw of this buffer

    def np(self):
        h = self.h if self.clone is None else self.clone
        a = h.cpu().numpy() if pyivx._is_torch(h) else h
        return a.view(self.dt).reshape(-1)


class Mode:
    def __init__(self, dev):
        self.dev, self.mem = dev, cint(pyivx.MEM_DEVICE if dev else pyivx.MEM_HOST)

    def put(self, a):
        return Buf(a, self.dev)

    def out(self, n, dt):
        """an output buffer of n elements (at least one), every byte PATTERN"""
        return self.put(np.full(max(int(n), 1) * np.dtype(dt).itemsize, PATTERN, np.uint8).view(dt))

    def fixed(self, *bufs):
        """input columns that the interface wants unchanged from the next call on (between a sizing call and its fill, under
        a build tail): nothing to do unless the mode rewrites its buffers before every call (LateMode)"""


class LateBuf(Buf):
    """a device Buf of LateMode: `h`, what the entry gets, holds the decoy (zero bytes) until the real content -- `stage`,
    complete on the device before anything is queued -- is copied over it on the mode's stream"""

    def __init__(self, a):
        import torch
        a = np.ascontiguousarray(a)
        self.dt, self.n = a.dtype, a.size
        if a.size == 0:
            a = np.zeros(1, a.dtype)
        self.stage = torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype)).copy()).to("cuda:0")     # (from pageable memory: synchronous)
        self.h = torch.zeros_like(self.stage)
        self.fixed = self.delivered = False


class Delay:
    """a device-side delay of a chosen length, queued on the current stream: torch.cuda._sleep, calibrated once with two
    timing events (cycles_per_ms), or -- should _sleep not give the length asked for -- a chain of 256 MB fills.  host_cost(nb)
    is the measured host time between queuing the delay and invoking an entry with nb live buffers: nb copies, one event."""
    MIN_MS = 10.0               # no delay is shorter
    FACTOR = 100.0              # ... nor shorter than this many times the host time it has to outlast

    def __init__(self, stream):
        import torch
        self.stream = stream
        self.log = []               # every call made under a LateMode with this delay: LateMode.calls
        self.n_early = 0            # ... and how many of them returned while their producer was still running

        def timed(queue):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record()
                queue()
                e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        timed(lambda: torch.cuda._sleep(1000))
        c1 = 1_000_000
        t1 = timed(lambda: torch.cuda._sleep(c1))
        c2 = int(c1 * min(max(20.0 / max(t1, 1e-3), 2.0), 1000.0))      # some 20 ms
        t2 = timed(lambda: torch.cuda._sleep(c2))
        self.cycles_per_ms = (c2 - c1) / (t2 - t1) if t2 > t1 else 0.0
        self.big, self.ms_per_fill = None, 0.0
        t10 = timed(lambda: self.queue(10.0)) if self.cycles_per_ms > 0 else 0.0
        if not 9.0 <= t10 <= 15.0:                                      # _sleep misbehaves: fills
            self.cycles_per_ms = 0.0
            self.big = torch.empty(1 << 26, dtype=torch.int32, device="cuda:0")
            timed(lambda: self.big.fill_(0))
            self.ms_per_fill = timed(lambda: [self.big.fill_(i) for i in range(8)]) / 8
            t10 = timed(lambda: self.queue(10.0))
            assert 9.0 <= t10 <= 30.0, f"no usable device-side delay: 10 ms asked for, {t10} ms measured"
        self.check_ms = t10                                             # what a delay of 10 ms took
        # the host side: the time nb copies and an event take to queue, at 1 and at 16 buffers (the most a catalogue case has
        # alive); the slowest of twenty runs each
        src = [torch.zeros(1000, dtype=torch.int32, device="cuda:0") for _ in range(16)]
        dst = [torch.zeros_like(t) for t in src]
        cost = {1: 0.0, 16: 0.0}
        for rep in range(22):                                           # (the first two: warm-up)
            for nb in cost:
                with torch.cuda.stream(stream):
                    t0 = time.perf_counter()
                    for a, b in zip(src[:nb], dst[:nb]):
                        b.copy_(a)
                    ev = torch.cuda.Event()
                    ev.record(stream)
                    ev.query()
                    dt = time.perf_counter() - t0
                stream.synchronize()
                if rep >= 2:
                    cost[nb] = max(cost[nb], dt)
        self.host_per_buf = max(cost[16] - cost[1], 0.0) / 15
        self.host_base = cost[1]

    def host_cost(self, nb):
        return self.host_base + self.host_per_buf * max(nb - 1, 0)

    def ms_for(self, nb):
        return max(self.MIN_MS, self.FACTOR * 1e3 * self.host_cost(nb))

    def queue(self, ms):
        import torch
        if self.big is None:
            torch.cuda._sleep(int(ms * self.cycles_per_ms))
        else:
            for i in range(int(math.ceil(ms / self.ms_per_fill))):
                self.big.fill_(i)


class LateMode(Mode):
    """device mode with every column still in flight on the caller's stream when the entry is invoked.  Env.call of the Env
    this mode is entered on (`with LateMode(E, stream, delay):`; the Env's context runs on `stream`) queues on that stream,
    and nowhere else, before every entry:
      1. the decoy -- zero bytes: key 0, position 0, offset 0, row 0, empty strings, an empty bitmap, a valid column of every
         case here -- into every live buffer of the mode, inputs and outputs alike;
      2. one delay (Delay.ms_for: at least 100 times the calibrated host time of 3. and 4., at least 10 ms; `ms` sets it by hand);
      3. the copies of the real contents: the input array, the PATTERN of an output, the caller's prior bits of a bitmap;
      4. the event `ready`;
    invokes the entry at once -- `ready` must not have happened by then, or the call proves nothing and fails as such --,
    queues a clone of every buffer named in outs= behind the entry before any synchronisation, synchronises, and asserts that
    the buffers still equal their clones.  Buf.np() gives the clone: the walk's results are what a consumer queued behind the
    call saw.  Inputs are never rewritten after a call returns (half of one valid offset column and half of another is no
    valid column); columns the interface wants unchanged across calls are named with fixed() and are late once."""

    def __init__(self, E, stream, delay, ms=None):
        super().__init__(True)
        self.E, self.stream, self.delay, self.ms = E, stream, delay, ms
        self.bufs = weakref.WeakSet()
        self.ready = None
        self.calls = []             # (entry, live buffers, host seconds between queuing the delay and invoking, the delay's ms)
        self.early = []             # per call: it returned while the producer was still running (it never waited for it)

    def __enter__(self):
        self.E.late = self
        return self

    def __exit__(self, *exc):
        self.E.late = None

    def put(self, a):
        b = LateBuf(a)
        self.bufs.add(b)
        return b

    def fixed(self, *bufs):
        for b in bufs:
            b.fixed = True

    def before(self):
        import torch
        live = [b for b in self.bufs if not (b.fixed and b.delivered)]
        ms = self.ms if self.ms is not None else self.delay.ms_for(len(live))
        self.stream.wait_stream(torch.cuda.current_stream())    # (the buffers were made on torch's current stream)
        with torch.cuda.stream(self.stream):
            for b in live:
                b.clone = None
                b.h.zero_()
            self.delay.queue(ms)
            self.t0 = time.perf_counter()
            for b in live:
                b.h.copy_(b.stage)
                b.delivered = True
            self.ready = torch.cuda.Event()
            self.ready.record(self.stream)
        self.nb, self.cur_ms = len(live), ms

    def invoke(self, entry):
        """right before the entry: the validity condition of the call"""
        self.calls.append((entry, self.nb, time.perf_counter() - self.t0, self.cur_ms))
        self.delay.log.append(self.calls[-1])
        assert not self.ready.query(), \
            f"{entry}: inconclusive -- the producer of the columns ({self.cur_ms:.1f} ms of delay) had finished before the entry was invoked"

    def after(self, outs):
        """right after the entry returned, nothing synchronised yet: had it waited for the producer?; the consumer's clones"""
        import torch
        self.early.append(not self.ready.query())
        self.delay.n_early += self.early[-1]
        self.cloned = [o[0] if isinstance(o, tuple) else o for o in outs]
        with torch.cuda.stream(self.stream):
            for b in self.cloned:
                b.clone = b.h.clone()

    def settle(self, entry):
        import torch
        self.stream.synchronize()
        for i, b in enumerate(self.cloned):
            assert torch.equal(b.h, b.clone), f"{entry}: output {i} changed after the consumer queued behind the call had read it"


def untouched(buf):
    return bool((buf.np().view(np.uint8) == PATTERN).all())


SHAPE = {"spread": 0, "ops": None, "cols": None}     # see shaped()


@contextlib.contextmanager
def shaped(spread=0, ops=None, cols=None):
    """the catalogue's columns at a size of the caller's for the with-block: ivals() over at least `spread` coordinates per
    row (the default 20 000 in all make 200 000 rows one run per key), or as cols(n, seed) gives them (int32 rows that meet
    the caller's own build); reads() with exactly `ops` CIGAR ops in all"""
    old = dict(SHAPE)
    SHAPE.update(spread=spread, ops=ops, cols=cols)
    try:
        yield
    finally:
        SHAPE.update(old)


def ivals(n, seed, dt=np.int32, span=20_000):
    if SHAPE["cols"] is not None:
        key, s, e = SHAPE["cols"](n, seed)
        return key.astype(np.uint32), s.astype(dt), e.astype(dt)
    rng = np.random.default_rng(seed)
    key = rng.integers(0, NK, n).astype(np.uint32)
    span = max(span, SHAPE["spread"] * n)
    s = rng.integers(0, span, n)
    e = s + rng.integers(0, 300, n)
    return key, s.astype(dt), e.astype(dt)


def reads(n, seed):
    """n reads with 1..3 CIGAR ops each (M, I, D, N, S) and n // 4 weighted segments, as the ABI's columns"""
    rng = np.random.default_rng(seed)
    off = np.zeros(n + 1, np.int32)
    ops = []
    per_read = None
    if SHAPE["ops"] is not None and n:                      # shaped(ops=): that many ops in all, every read 1 or more
        assert n <= SHAPE["ops"]
        per_read = np.full(n, SHAPE["ops"] // n)
        per_read[:SHAPE["ops"] % n] += 1
    for i in range(n):
        for _ in range(int(rng.integers(1, 4)) if per_read is None else int(per_read[i])):
            ops.append((int(rng.integers(1, 60)) << 4) | int(rng.choice([0, 0, 0, 1, 2, 3, 4])))
        off[i + 1] = 4 * len(ops)
    ns = n // 4
    ss = rng.integers(0, 5000, ns)
    return dict(rkey=rng.integers(0, NK, n).astype(np.uint32), rpos=rng.integers(0, 5000, n).astype(np.uint32),
                rflags=np.where(rng.random(n) < 0.1, 4, 0).astype(np.uint32), rmapq=rng.integers(0, 61, n).astype(np.uint32),
                off=off, ops=np.array(ops, np.uint32).reshape(-1),
                skey=rng.integers(0, NK, ns).astype(np.uint32), ss=ss.astype(np.uint32), se=(ss + rng.integers(0, 80, ns)).astype(np.uint32),
                sw=rng.integers(-2, 4, ns).astype(np.int32))


class Refused(Exception):
    """Env.call met IVX_ERR_OOM while Env.stop_on_oom was set: the case ends at its first refused call"""


class Call:
    """one line of Env.log: the entry, its status and error text (a case makes several calls, and later ones overwrite
    ivx_last_error), the context's metrics right before and after it, and what the caller registered of its outputs -- the
    output Bufs ((Buf, array) for a buffer the entry ORs into: what it held before), the scalar count's value after the call,
    the out-handle's value after the call"""

    def __init__(self, entry, st, text, before, after, outs, count, handle):
        self.entry, self.st, self.text, self.before, self.after, self.outs = entry, st, text, before, after, tuple(outs)
        self.count = None if count is None else count.value
        self.has_handle, self.handle = handle is not None, None if handle is None else handle.value


class Env:
    """one context, one index of every kind (from build_cols, by default 1 000 seeded rows) and two depth profiles, built
    once from host columns; with `stream` (a torch stream) the context then runs on that caller's stream"""

    def __init__(self, build_cols=None, stream=None):
        import torch
        torch.zeros(1, device="cuda:0")                         # (torch's own start-up: here, not in the first case that puts a tensor)
        self.ctx = pyivx.Ctx(0)
        self.h = self.ctx.h
        self.L = pyivx.lib()
        self.build_cols = ivals(1000, 1) if build_cols is None else build_cols
        self.n_build = len(self.build_cols[1])
        self.ix = [self.ctx.build(kind, *self.build_cols, n_keys=NK) for kind in range(4)]
        r = reads(1000, 7)
        self.profile = self.ctx.depth_profile(r["rkey"], r["rpos"], r["rflags"], r["rmapq"], r["off"], r["ops"],
                                              r["skey"], r["ss"], r["se"], r["sw"], n_keys=NK)
        r = reads(64, 9)
        self.profile2 = self.ctx.depth_profile(r["rkey"], r["rpos"], r["rflags"], r["rmapq"], r["off"], r["ops"],
                                               r["skey"], r["ss"], r["se"], r["sw"], n_keys=NK)
        self.log = []                   # a Call per call() since the caller last emptied it
        self.stop_on_oom = False
        self.late = None                # the LateMode entered on this Env, if any
        self.stream = stream
        if stream is not None:
            self.ctx.set_stream(stream.cuda_stream)

    def call(self, name, *args, outs=(), count=None, handle=None, drain=True):
        """the entry's status; the context's stream drained, so that device-mode outputs can be read.  The call goes into
        the log with the outputs the caller names; with stop_on_oom set, IVX_ERR_OOM raises Refused.  Under a LateMode the
        mode's producers are queued in front of the entry and its consumers behind it (see there).  drain=False, for a call
        without output buffers: nothing is waited for (ivx_ctx_synchronize would wait for a running build tail, too)"""
        assert drain or not outs
        before = self.ctx.metrics()
        late, fn = self.late, getattr(self.L, name)
        if late is not None:
            late.before()
            late.invoke(name)
        st = fn(self.h, *args)
        if late is not None:
            late.after(outs)
        self.log.append(Call(name, st, self.err() if st != OK else "", before, self.ctx.metrics(), outs, count, handle))
        if not drain:
            return st
        assert self.L.ivx_ctx_synchronize(self.h) == OK
        if late is not None:
            late.settle(name)
        if st == OOM and self.stop_on_oom:
            raise Refused(name)
        return st

    def err(self):
        return self.L.ivx_last_error(self.h).decode()

    def close(self):
        self.profile.free()
        self.profile2.free()
        for ix in self.ix:
            ix.free()
        self.ctx.close()


# ------------------------------------------------------------------ the cases

CASES = {}


def case(f):
    CASES[f.__name__] = f
    return f


def sized(res, name, call):
    """the three calls of a sizing / fill pair.  call(cap, with_buffers) -> (status, count, [output Bufs]); the one-short
    fill must give IVX_ERR_CAPACITY (with the same count in both modes: the caller compares `res`)"""
    st, m, _ = call(0, False)
    res[name + ".sizing"] = (st, m)
    st, m1, outs = call(m, True)
    assert st == OK and m1 == m, (name, st, m1, m)
    res[name + ".fill"] = (st, m1)
    for i, o in enumerate(outs):
        res[f"{name}.fill.{i}"] = o.np()[:m]
    if m:
        st, m2, _ = call(m - 1, True)
        assert st == CAPACITY, (name, st)
        res[name + ".short"] = (st, m2)


@case
def index_build(E, M, n):
    res = {}
    k, s, e = (M.put(a) for a in ivals(n, 3))
    pk, ps, pe = ivals(200, 4)
    for kind in range(4):
        h = C.c_void_p(0xDEAD)
        st = E.call("ivx_index_build", cint(kind), M.mem, k.p, s.p, e.p, u64(n), u32(NK), C.byref(h), handle=h)
        assert st == OK, E.err()
        ix = pyivx.Index(E.ctx, h, kind)
        try:                                                    # (a refused probe must not leave the index alive)
            res[f"{kind}.rows"], res[f"{kind}.bytes"] = ix.rows, ix.device_bytes
            if n:
                if kind == pyivx.KIND_OVERLAP:
                    res["0.total"], res["0.per_row"] = E.ctx.overlap_count(ix, pk, ps, pe, per_row=True)
                elif kind == pyivx.KIND_COUNT:
                    res["1.count"] = E.ctx.count_overlaps(ix, pk, ps, pe)
                elif kind == pyivx.KIND_COVERAGE:
                    res["2.coverage"] = E.ctx.coverage(ix, pk, ps, pe)
                else:
                    res["3.b"], res["3.p"], res["3.d"] = E.ctx.nearest(ix, pk, ps, pe, k=2)
        finally:
            ix.free()
    return res


@case
def probe_overlap_count(E, M, n):
    k, s, e = (M.put(a) for a in ivals(n, 5))
    res = {}
    tot = u64(0xDEAD)
    res["st"] = E.call("ivx_probe_overlap_count", E.ix[0].h, M.mem, k.p, s.p, e.p, u64(n), None, C.byref(tot), count=tot)
    res["total"] = tot.value
    pr = M.out(n, np.uint32)
    tot2 = u64(0xDEAD)
    res["st2"] = E.call("ivx_probe_overlap_count", E.ix[0].h, M.mem, k.p, s.p, e.p, u64(n), pr.p, C.byref(tot2), outs=[pr], count=tot2)
    res["total2"], res["per_row"] = tot2.value, pr.np()[:n]
    return res


@case
def probe_overlap_fill(E, M, n):
    k, s, e = (M.put(a) for a in ivals(n, 5))
    # (no M.fixed(): without IVX_JOIN_PATH=regions a count call of fewer than 2^21 rows leaves no plan, the fill call reads the
    # three columns itself and LateMode delivers them late again; a planned fill: test_gpu_entry_stream_order.py, fixed columns)
    res = {}

    def call(cap, bufs):
        w = u64(0xDEAD)
        if not bufs:        # (the sizing call of a fill is the count call)
            st = E.call("ivx_probe_overlap_count", E.ix[0].h, M.mem, k.p, s.p, e.p, u64(n), None, C.byref(w), count=w)
            return st, w.value, []
        b, p = M.out(cap, np.uint32), M.out(cap, np.uint32)
        st = E.call("ivx_probe_overlap_fill", E.ix[0].h, M.mem, k.p, s.p, e.p, u64(n), b.p, p.p, u64(cap), C.byref(w), outs=[b, p], count=w)
        m = min(w.value, cap)
        pairs = np.sort((b.np()[:m].astype(np.uint64) << np.uint64(32)) | p.np()[:m].astype(np.uint64))   # (the order of the pairs is free)
        return st, w.value, [Buf(pairs, False)]
    sized(res, "fill", call)
    return res


@case
def probe_exists(E, M, n):
    k, s, e = (M.put(a) for a in ivals(n, 6))
    out = M.out(n, np.uint8)
    st = E.call("ivx_probe_exists", E.ix[0].h, M.mem, k.p, s.p, e.p, u64(n), out.p, outs=[out])
    return {"st": st, "exists": out.np()[:n]}


@case
def probe_mark_build(E, M, n):
    k, s, e = (M.put(a) for a in ivals(n, 6, span=4000))
    nw = (E.n_build + 31) // 32
    mine = np.zeros(nw, np.uint32)
    mine[::3] = 0x00010001                                  # bits the caller had set: they survive
    marks = M.put(mine)
    st = E.call("ivx_probe_mark_build", E.ix[0].h, M.mem, k.p, s.p, e.p, u64(n), marks.p, outs=[(marks, mine)])
    got = marks.np()
    assert ((got & mine) == mine).all()
    return {"st": st, "marks": got}


AGG_DTS = (np.uint32,) + (np.int64,) * 5                       # count, sum, vmin, vmax, bases, wsum


@case
def probe_overlap_agg(E, M, n):
    """all six outputs, an int64 value per build row"""
    k, s, e = (M.put(a) for a in ivals(n, 29, span=4000))
    val = M.put(np.random.default_rng(30).integers(-(1 << 40), 1 << 40, E.n_build).astype(np.int64))
    outs = [M.out(n, dt) for dt in AGG_DTS]
    st = E.call("ivx_probe_overlap_agg", E.ix[0].h, M.mem, k.p, s.p, e.p, u64(n), val.p, u32(8), *[o.p for o in outs], outs=outs)
    res = {"st": st}
    res.update({name: o.np()[:n] for name, o in zip(pyivx.AGG_OUTPUTS, outs)})
    return res


SEL_CASE_BY = ("max_val", "min_overlap", "last_row")


def _family_in(E, M, n):
    """what the select and threshold cases share: probe_overlap_agg's rows, a small int64 value per build row (many ties),
    and the head of the call"""
    k, s, e = (M.put(a) for a in ivals(n, 29, span=4000))
    val = M.put(np.random.default_rng(30).integers(-5, 6, E.n_build).astype(np.int64))
    return (k, s, e, val), (E.ix[0].h, M.mem, k.p, s.p, e.p, u64(n))


def _where():
    """min_bases 10 and half of the probe row"""
    return pyivx.OverlapWhereC(10, 1, 2, 0, 0, 0)


@case
def probe_overlap_select(E, M, n):
    """both outputs, three criteria: the value, the overlap length, the last row"""
    (k, s, e, val), head = _family_in(E, M, n)
    res = {}
    for by in SEL_CASE_BY:
        bi, sc = M.out(n, np.uint32), M.out(n, np.int64)
        res["st." + by] = E.call("ivx_probe_overlap_select", *head, val.p, u32(8), cint(pyivx.SEL_BY.index(by)), bi.p, sc.p, outs=[bi, sc])
        res["idx." + by], res["score." + by] = bi.np()[:n], sc.np()[:n]
    return res


@case
def probe_overlap_count_where(E, M, n):
    """all three outputs; then the total alone, whose per-row counts live in scratch and go through the device reduction"""
    (k, s, e, val), head = _family_in(E, M, n)
    w = _where()
    res = {}
    pr, ex, tot = M.out(n, np.uint32), M.out(n, np.uint8), u64(0xDEAD)
    res["st.count"] = E.call("ivx_probe_overlap_count_where", *head, C.byref(w), pr.p, ex.p, C.byref(tot), outs=[pr, ex], count=tot)
    res["per_row"], res["exists"], res["total"] = pr.np()[:n], ex.np()[:n], tot.value
    tot2 = u64(0xDEAD)
    res["st.total"] = E.call("ivx_probe_overlap_count_where", *head, C.byref(w), None, None, C.byref(tot2), count=tot2)
    res["total2"] = tot2.value
    return res


@case
def probe_mark_build_where(E, M, n):
    (k, s, e, val), head = _family_in(E, M, n)
    w = _where()
    mine = np.zeros((E.n_build + 31) // 32, np.uint32)
    mine[::3] = 0x00010001                                  # bits the caller had set: they survive
    marks = M.put(mine)
    st = E.call("ivx_probe_mark_build_where", *head, C.byref(w), marks.p, outs=[(marks, mine)])
    got = marks.np()
    assert ((got & mine) == mine).all()
    return {"st.marks": st, "marks": got}


@case
def probe_overlap_agg_where(E, M, n):
    (k, s, e, val), head = _family_in(E, M, n)
    w = _where()
    outs = [M.out(n, dt) for dt in AGG_DTS]
    res = {"st.agg": E.call("ivx_probe_overlap_agg_where", *head, val.p, u32(8), C.byref(w), *[o.p for o in outs], outs=outs)}
    res.update({"agg." + name: o.np()[:n] for name, o in zip(pyivx.AGG_OUTPUTS, outs)})
    return res


@case
def probe_overlap_select_where(E, M, n):
    (k, s, e, val), head = _family_in(E, M, n)
    w = _where()
    bi, sc = M.out(n, np.uint32), M.out(n, np.int64)
    st = E.call("ivx_probe_overlap_select_where", *head, val.p, u32(8), cint(pyivx.SEL_BY.index("max_overlap")), C.byref(w), bi.p, sc.p,
                outs=[bi, sc])
    return {"st.select": st, "idx": bi.np()[:n], "score": sc.np()[:n]}


@case
def pairs_where(E, M, n):
    """the pair filter over n pairs of (row i of the build's first n rows, probe row i): sizing, fill, one short"""
    (k, s, e, val), head = _family_in(E, M, n)
    w = _where()
    bsd, bed = M.put(E.build_cols[1][:max(n, 1)]), M.put(E.build_cols[2][:max(n, 1)])
    ids = M.put(np.arange(n, dtype=np.uint32))
    res = {}

    def call(cap, bufs):
        ob, op, m = M.out(cap, np.uint32), M.out(cap, np.uint32), u64(0xDEAD)
        give = bufs and cap > 0                               # (output columns without capacity are refused)
        st = E.call("ivx_pairs_where", M.mem, ids.p, ids.p, u64(n), bsd.p, bed.p, u64(n), s.p, e.p, u64(n), C.byref(w),
                    ob.p if give else None, op.p if give else None, u64(cap), C.byref(m), outs=[ob, op], count=m)
        return st, m.value, [ob, op]
    sized(res, "pairs", call)
    return res


@case
def bits_mark(E, M, n):
    rng = np.random.default_rng(8)
    idx = rng.integers(0, 5000, n).astype(np.uint32)
    idx[::7] = NULL
    mine = np.zeros((5000 + 31) // 32, np.uint32)
    mine[::5] = 0x80000001
    d_idx, bits = M.put(idx), M.put(mine)
    st = E.call("ivx_bits_mark", M.mem, d_idx.p, u64(n), bits.p, u64(5000), outs=[(bits, mine)])
    got = bits.np()
    assert ((got & mine) == mine).all()
    return {"st": st, "bits": got}


@case
def bits_select(E, M, n):
    rng = np.random.default_rng(9)
    bits = M.put(rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32))
    res = {}
    for want in (1, 0):
        def call(cap, bufs):
            m = u64(0xDEAD)
            out = M.out(cap, np.uint32)
            st = E.call("ivx_bits_select", M.mem, bits.p, u64(n), cint(want), out.p if bufs else None, u64(cap), C.byref(m),
                        outs=[out], count=m)
            return st, m.value, [out]
        sized(res, f"select{want}", call)
    return res


def _per_row(entry, kind):
    def f(E, M, n):
        k, s, e = (M.put(a) for a in ivals(n, 10))
        res = {}
        for strict in (0, 1):
            out = M.out(n, np.int64)
            res[f"st{strict}"] = E.call(entry, E.ix[kind].h, M.mem, k.p, s.p, e.p, u64(n), cint(strict), out.p, outs=[out])
            res[f"out{strict}"] = out.np()[:n]
        return res
    f.__name__ = entry[4:]
    return case(f)


_per_row("ivx_probe_count", pyivx.KIND_COUNT)
_per_row("ivx_probe_coverage", pyivx.KIND_COVERAGE)


@case
def probe_nearest(E, M, n):
    k, s, e = (M.put(a) for a in ivals(n, 11))
    cap = 2 * n
    b, p, d = M.out(cap, np.uint32), M.out(cap, np.uint32), M.out(cap, np.int64)
    rows = u64(0xDEAD)
    st = E.call("ivx_probe_nearest", E.ix[3].h, M.mem, k.p, s.p, e.p, u64(n), cint(0), u32(2), cint(1), b.p, p.p, d.p, u64(cap), C.byref(rows),
                outs=[b, p, d], count=rows)
    r = rows.value
    return {"st": st, "rows": r, "b": b.np()[:r], "p": p.np()[:r], "d": d.np()[:r]}


# (direction, include_overlaps, max_distance) of the nearest_dir cases: each side with and without overlaps, without a cap and
# within 32; both sides within 32.  ("any" without a cap is ivx_probe_nearest: the case above.)
NEAR_DIR_CALLS = [(d, ovl, D) for d in ("before", "after") for ovl in (1, 0) for D in (-1, 32)] + [("any", 1, 32)]


def near_dir_tag(d, ovl, D):
    return f"{d}.ovl{ovl}.d{D}"


def nearest_dir_calls(E, M, n, k):
    """ivx_probe_nearest_dir for every NEAR_DIR_CALLS on probe_nearest's rows, k answers a row at the most"""
    ks, s, e = (M.put(a) for a in ivals(n, 11))
    cap = k * n
    res = {}
    for d, ovl, D in NEAR_DIR_CALLS:
        b, p, dist = M.out(cap, np.uint32), M.out(cap, np.uint32), M.out(cap, np.int64)
        rows = u64(0xDEAD)
        st = E.call("ivx_probe_nearest_dir", E.ix[3].h, M.mem, ks.p, s.p, e.p, u64(n), cint(0), u32(k), cint(ovl),
                    cint(pyivx.NEAR_DIRECTIONS.index(d)), i64(D), b.p, p.p, dist.p, u64(cap), C.byref(rows), outs=[b, p, dist], count=rows)
        r, tag = rows.value, near_dir_tag(d, ovl, D)
        res.update({tag + ".st": st, tag + ".rows": r, tag + ".b": b.np()[:r], tag + ".p": p.np()[:r], tag + ".d": dist.np()[:r]})
    return res


def nearest_dir_want(oix, n, k):
    """tag -> (build rows, probe rows, distances) that nearest_dir_calls must give, from the restatement `oix`
    (tests/nearest_dir_oracle.NearIndex over the Env's build columns)"""
    p = ivals(n, 11)
    return {near_dir_tag(d, ovl, D): oix.query(*p, k=k, overlap=bool(ovl), direction=d, max_distance=None if D < 0 else D)
            for d, ovl, D in NEAR_DIR_CALLS}


def assert_nearest_dir(got, want, what):
    for tag, (wb, wp, wd) in want.items():
        assert got[tag + ".st"] == OK and got[tag + ".rows"] == len(wb), (what, tag, got[tag + ".st"], got[tag + ".rows"], len(wb))
        assert (got[tag + ".b"] == wb).all() and (got[tag + ".p"] == wp).all() and (got[tag + ".d"] == wd).all(), (what, tag)


@case
def probe_nearest_dir(E, M, n):
    return nearest_dir_calls(E, M, n, 2)


@case
def merge(E, M, n):
    k, s, e = (M.put(a) for a in ivals(n, 12, np.int64))
    outs = [M.out(n, dt) for dt in (np.uint32, np.int64, np.int64, np.int64)]
    m = u64(0xDEAD)
    st = E.call("ivx_merge", M.mem, k.p, s.p, e.p, u64(n), u32(NK), i64(0), cint(0), *[o.p for o in outs], u64(n), C.byref(m),
                outs=outs, count=m)
    res = {"st": st, "n_out": m.value}
    res.update({f"o{i}": o.np()[:m.value] for i, o in enumerate(outs)})
    return res


@case
def subtract(E, M, n):
    lk, ls, le = (M.put(a) for a in ivals(n, 13, np.int64))
    nr = n // 2 if n > 1 else n
    rk, rs, re = (M.put(a) for a in ivals(nr, 14, np.int64))
    M.fixed(lk, ls, le, rk, rs, re)     # the six columns must not change between the sizing call and its fill: late once
    res = {}

    def call(cap, bufs):
        outs = [M.out(cap, dt) for dt in (np.uint32, np.int64, np.int64, np.uint32)]
        m = u64(0xDEAD)
        st = E.call("ivx_subtract", M.mem, lk.p, ls.p, le.p, u64(n), rk.p, rs.p, re.p, u64(nr), u32(NK), cint(0),
                    *[o.p if bufs else None for o in outs], u64(cap), C.byref(m), outs=outs, count=m)
        return st, m.value, outs
    sized(res, "subtract", call)
    return res


@case
def intersect(E, M, n):
    lk, ls, le = (M.put(a) for a in ivals(n, 31, np.int64))
    nr = n // 2 if n > 1 else n
    rk, rs, re = (M.put(a) for a in ivals(nr, 32, np.int64))
    res = {}

    def call(cap, bufs):
        outs = [M.out(cap, dt) for dt in (np.uint32, np.int64, np.int64, np.uint32)]
        m = u64(0xDEAD)
        st = E.call("ivx_intersect", M.mem, lk.p, ls.p, le.p, u64(n), rk.p, rs.p, re.p, u64(nr), u32(NK), cint(0),
                    *[o.p if bufs else None for o in outs], u64(cap), C.byref(m), outs=outs, count=m)
        return st, m.value, outs
    sized(res, "intersect", call)
    return res


@case
def cluster(E, M, n):
    k, s, e = (M.put(a) for a in ivals(n, 15, np.int64))
    base = M.put(np.array([0, 1000, 5000], np.int64))
    dts = (np.uint32, np.int64, np.int64, np.uint32, np.int64, np.int64, np.int64)
    outs = [M.out(n, dt) for dt in dts]
    kc = M.out(NK, np.uint64)
    m = u64(0xDEAD)
    st = E.call("ivx_cluster", M.mem, k.p, s.p, e.p, u64(n), u32(NK), i64(5), cint(0), base.p, *[o.p for o in outs], kc.p, C.byref(m),
                outs=outs + [kc], count=m)
    res = {"st": st, "n_clusters": m.value, "key_clusters": kc.np()[:NK]}
    res.update({f"o{i}": o.np()[:n] for i, o in enumerate(outs)})
    return res


@case
def complement(E, M, n):
    k, s, e = (M.put(a) for a in ivals(n, 16, np.int64))
    nv = min(n, 4)
    vk, vs, ve = (M.put(a) for a in (np.arange(nv, dtype=np.uint32) % NK, np.full(nv, 100, np.int64), np.full(nv, 19_000, np.int64)))
    res = {}

    def call(cap, bufs):
        outs = [M.out(cap, dt) for dt in (np.uint32, np.int64, np.int64)]
        m = u64(0xDEAD)
        st = E.call("ivx_complement", M.mem, k.p, s.p, e.p, u64(n), vk.p, vs.p, ve.p, u64(nv), u32(NK), cint(0),
                    *[o.p if bufs else None for o in outs], u64(cap), C.byref(m), outs=outs, count=m)
        return st, m.value, outs
    sized(res, "complement", call)
    return res


def _depth_in(M, n, text, large=0):
    r = reads(n, 17)
    d = {c: M.put(r[c]) for c in ("rkey", "rpos", "rflags", "rmapq", "skey", "ss", "se", "sw")}
    if text:
        toff, ttext = cto.text_column(cto.render_reads(r["off"], r["ops"]), large=bool(large), first=3)
        d["cig"] = (M.put(toff), M.put(ttext))
        cig = (cint(large), d["cig"][0].p, d["cig"][1].p)
    else:
        d["cig"] = (M.put(r["off"]), M.put(r["ops"]))
        cig = (d["cig"][0].p, d["cig"][1].p)
    klen = M.put(np.array([4000, 6000, 5200], np.uint32))
    args = (M.mem, d["rkey"].p, d["rpos"].p, d["rflags"].p, d["rmapq"].p, *cig, n,
            d["skey"].p, d["ss"].p, d["se"].p, d["sw"].p, n // 4, NK, klen.p, 1796, 20)
    return args, (d, klen)


def _depth(entry, text):
    def f(E, M, n):
        args, keep = _depth_in(M, n, text)
        res = {}

        def call(cap, bufs):
            outs = [M.out(cap, dt) for dt in (np.uint32, np.uint32, np.uint32, np.int32)]
            m = u64(0xDEAD)
            st = E.call(entry, *args, *[o.p if bufs else None for o in outs], cap, C.byref(m), outs=outs, count=m)
            return st, m.value, outs
        sized(res, entry, call)
        return res
    f.__name__ = entry[4:]
    return case(f)


_depth("ivx_depth", False)
_depth("ivx_depth_text", True)


def _profile_build(entry, text):
    def f(E, M, n):
        args, keep = _depth_in(M, n, text, large=1 if text else 0)
        h = C.c_void_p(0xDEAD)
        st = E.call(entry, *args, C.byref(h), handle=h)
        assert st == OK, E.err()
        p = pyivx.DepthProfile(E.ctx, h, NK, None)
        try:
            key, pos, cov, seen = p.read()
            res = {"steps": p.steps(), "bytes": p.device_bytes, "key": key, "pos": pos, "cov": cov, "seen": seen}
        finally:
            p.free()
        return res
    f.__name__ = entry[4:]
    return case(f)


_profile_build("ivx_depth_profile_build", False)
_profile_build("ivx_depth_profile_build_text", True)


@case
def cigar_parse(E, M, n):
    r = reads(n, 18)
    res = {}
    for large in (0, 1):
        toff, ttext = (M.put(a) for a in cto.text_column(cto.render_reads(r["off"], r["ops"]), large=bool(large)))
        head = (M.mem, cint(large), toff.p, ttext.p, u64(n))

        def call(cap, bufs):
            off, ops = M.out(n + 1, np.int32), M.out(cap, np.uint32)
            m = u64(0xDEAD)
            st = E.call("ivx_cigar_parse", *head, off.p if bufs else None, ops.p if bufs else None, u64(cap), C.byref(m),
                        outs=[off, ops], count=m)
            if bufs and n:
                res[f"{large}.off@{cap}"] = off.np()[:n + 1]       # (the offsets go out whether the ops fitted or not)
            return st, m.value, [ops]
        sized(res, f"parse{large}", call)
    return res


@case
def depth_profile_read(E, M, n):
    steps = E.profile.steps()
    res = {}
    for cap in (steps, steps - 1):
        outs = [M.out(steps, dt) for dt in (np.uint32, np.uint32, np.int32)]
        seen = M.out(NK, np.uint8)
        m = u64(0xDEAD)
        st = E.call("ivx_depth_profile_read", E.profile.h, M.mem, *[o.p for o in outs], seen.p, u64(cap), C.byref(m),
                    outs=outs + [seen], count=m)
        assert st == (OK if cap == steps else CAPACITY)
        res[f"{cap}"] = (st, m.value)
        res[f"{cap}.seen"] = seen.np()[:NK]
        res.update({f"{cap}.o{i}": o.np() for i, o in enumerate(outs)})     # (one short: all of it still the pattern)
    return res


@case
def depth_profile_expand(E, M, n):
    pos, cov = M.out(n, np.int32), M.out(n, np.int16)
    st = E.call("ivx_depth_profile_expand", E.profile.h, M.mem, 1, 100, n, 0, pos.p, cov.p, outs=[pos, cov])
    return {"st": st, "pos": pos.np()[:n], "cov": cov.np()[:n]}


@case
def depth_profile_blocks(E, M, n):
    res = {}

    def call(cap, bufs):
        outs = [M.out(cap, dt) for dt in (np.uint32, np.uint32, np.uint32, np.int32)]
        m = u64(0xDEAD)
        st = E.call("ivx_depth_profile_blocks", E.profile.h, M.mem, *[o.p if bufs else None for o in outs], u64(cap), C.byref(m),
                    outs=outs, count=m)
        return st, m.value, outs
    sized(res, "blocks", call)
    return res


def _regions(M, n):
    rng = np.random.default_rng(19)
    qs = rng.integers(0, 5000, n)
    return [M.put(a) for a in (rng.integers(0, NK, n).astype(np.uint32), qs.astype(np.uint32), (qs + rng.integers(0, 400, n)).astype(np.uint32),
                               np.array([4000, 6000, 5200], np.uint32))]


@case
def depth_profile_summarize(E, M, n):
    qk, qs, qe, hi = _regions(M, n)
    thr = np.array([1, 3, 10], np.int32)
    outs = [M.out(n, np.int64), M.out(n, np.int64), M.out(3 * n, np.int64)]
    st = E.call("ivx_depth_profile_summarize", E.profile.h, M.mem, qk.p, qs.p, qe.p, n, 0, hi.p, 0, pyivx._ptr(thr), 3, *[o.p for o in outs],
                outs=outs)
    return {"st": st, "len": outs[0].np()[:n], "sum": outs[1].np()[:n], "ge": outs[2].np()[:3 * n]}


@case
def depth_profile_windows(E, M, n):
    thr = np.array([1, 3, 10], np.int32)
    outs = [M.out(n, np.int64), M.out(n, np.int64), M.out(3 * n, np.int64)]
    st = E.call("ivx_depth_profile_windows", E.profile.h, M.mem, 2, 50, 50 + 7 * max(n, 1) - 4, 7, n, 1, pyivx._ptr(thr), 3, *[o.p for o in outs],
                outs=outs)
    return {"st": st, "len": outs[0].np()[:n], "sum": outs[1].np()[:n], "ge": outs[2].np()[:3 * n]}


@case
def depth_profile_quantiles(E, M, n):
    qk, qs, qe, hi = _regions(M, n)
    qn = np.array([1, 3], np.uint32)
    outs = [M.out(n, np.int64), M.out(n, np.int32), M.out(n, np.int32), M.out(2 * n, np.int32)]
    st = E.call("ivx_depth_profile_quantiles", E.profile.h, M.mem, qk.p, qs.p, qe.p, n, 0, hi.p, 0, pyivx._ptr(qn), 2, 4, *[o.p for o in outs],
                outs=outs)
    return {"st": st, "len": outs[0].np()[:n], "min": outs[1].np()[:n], "max": outs[2].np()[:n], "q": outs[3].np()[:2 * n]}


@case
def depth_profile_window_quantiles(E, M, n):
    qn = np.array([1, 3], np.uint32)
    outs = [M.out(n, np.int64), M.out(n, np.int32), M.out(n, np.int32), M.out(2 * n, np.int32)]
    st = E.call("ivx_depth_profile_window_quantiles", E.profile.h, M.mem, 2, 50, 50 + 7 * max(n, 1) - 4, 7, n, 1, pyivx._ptr(qn), 2, 4,
                *[o.p for o in outs], outs=outs)
    return {"st": st, "len": outs[0].np()[:n], "min": outs[1].np()[:n], "max": outs[2].np()[:n], "q": outs[3].np()[:2 * n]}


@case
def depth_profile_merge(E, M, n):
    """E.profile + E.profile2 (one row: the other way round; the empty call: a profile with itself), the sum read back in
    mode M and freed here"""
    a, b = (E.profile, E.profile) if n == 0 else (E.profile2, E.profile) if n == 1 else (E.profile, E.profile2)
    h = C.c_void_p(0xDEAD)
    st = E.call("ivx_depth_profile_merge", a.h, b.h, C.byref(h), handle=h)
    assert st == OK, E.err()
    try:
        steps = E.L.ivx_depth_profile_steps(h)
        res = {"st": st, "steps": steps, "bytes": E.L.ivx_depth_profile_device_bytes(h)}
        outs = [M.out(steps, dt) for dt in (np.uint32, np.uint32, np.int32)]
        seen = M.out(NK, np.uint8)
        m = u64(0xDEAD)
        res["st2"] = E.call("ivx_depth_profile_read", h, M.mem, *[o.p for o in outs], seen.p, u64(steps), C.byref(m),
                            outs=outs + [seen], count=m)
        res["n_out"], res["seen"] = m.value, seen.np()[:NK]
        res.update({f"o{i}": o.np()[:steps] for i, o in enumerate(outs)})
    finally:
        E.L.ivx_depth_profile_free(h)
    return res


def _classes_in(M, n):
    """the domain arguments quantize and hist share: (pos_lo, key_hi, skip_pos0, seen_only), key_hi kept alive"""
    hi = M.put(np.array([4000, 6000, 5200], np.uint32))
    return (0, hi.p, 1, int(n & 1)), hi


@case
def depth_profile_quantize(E, M, n):
    """min(n, 3) cuts; class 1 is never emitted (its runs still separate their neighbours)"""
    cuts = np.array([1, 3, 10], np.int32)[:min(n, 3)]
    emit = 0b1101 & ((1 << (len(cuts) + 1)) - 1)
    dom, keep = _classes_in(M, n)
    res = {}

    def call(cap, bufs):
        outs = [M.out(cap, np.uint32) for _ in range(4)]
        m = u64(0xDEAD)
        st = E.call("ivx_depth_profile_quantize", E.profile.h, M.mem, *dom, pyivx._ptr(cuts) if len(cuts) else None, len(cuts), emit,
                    *[o.p if bufs else None for o in outs], u64(cap), C.byref(m), outs=outs, count=m)
        return st, m.value, outs
    sized(res, "quantize", call)
    return res


@case
def depth_profile_hist(E, M, n):
    n_bins = max(1, min(n, 16))
    dom, keep = _classes_in(M, n)
    out = M.out(NK * n_bins, np.int64)
    st = E.call("ivx_depth_profile_hist", E.profile.h, M.mem, *dom, 1, n_bins, out.p, outs=[out])
    return {"st": st, "hist": out.np()[:NK * n_bins]}


N_SRC = 300


def _take_idx(n, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N_SRC, n).astype(np.uint32)
    idx[::9] = NULL
    return idx, np.packbits(rng.random(N_SRC) < 0.9, bitorder="little")


@case
def take_fixed(E, M, n):
    idx, valid = _take_idx(n, 20)
    src, d_idx, svb = M.put(np.random.default_rng(21).integers(0, 1 << 62, N_SRC).astype(np.int64)), M.put(idx), M.put(valid)
    out, ov = M.out(n, np.int64), M.out(n, np.uint8)
    st = E.call("ivx_take_fixed", M.mem, src.p, u32(8), u64(N_SRC), svb.p, d_idx.p, u64(n), out.p, ov.p, outs=[out, ov])
    return {"st": st, "out": out.np()[:n], "valid": ov.np()[:n]}


@case
def scatter_fixed(E, M, n):
    rng = np.random.default_rng(22)
    n_out = 2000
    idx = rng.permutation(n_out)[:n].astype(np.uint32)
    src, d_idx = M.put(rng.integers(0, 1 << 30, n).astype(np.int32)), M.put(idx)
    out = M.out(n_out, np.int32)
    st = E.call("ivx_scatter_fixed", M.mem, src.p, u32(4), d_idx.p, u64(n), out.p, u64(n_out), outs=[out])
    got = out.np()
    rest = np.ones(n_out, bool)
    rest[idx] = False
    assert (got[rest].view(np.uint8) == PATTERN).all()        # rows no index names keep the caller's bytes
    return {"st": st, "out": got}


def _strings(seed):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(97, 123, int(rng.integers(0, 31)), dtype=np.uint8)) for _ in range(N_SRC)]


@case
def take_utf8(E, M, n):
    res = {}
    idx, valid = _take_idx(n, 23)
    d_idx, svb = M.put(idx), M.put(valid)
    for large in (0, 1):
        off, data = cto.text_column(_strings(24), large=bool(large))
        d_off, d_data = M.put(off), M.put(data)
        head = (M.mem, cint(large), d_off.p, d_data.p, u64(N_SRC), u64(len(data)), svb.p, d_idx.p, u64(n))

        def call(cap, bufs):
            ooff, odata, ov = M.out(n + 1, off.dtype), M.out(cap, np.uint8), M.out(n, np.uint8)
            need = u64(0xDEAD)
            st = E.call("ivx_take_utf8", *head, ooff.p, odata.p if bufs else None, u64(cap), C.byref(need), ov.p,
                        outs=[ooff, odata, ov], count=need)
            # a short data buffer (and the sizing call) still returns the offsets and the validity
            res[f"{large}.off@{cap},{bufs}"], res[f"{large}.valid@{cap},{bufs}"] = ooff.np()[:n + 1], ov.np()[:n]
            return st, need.value, [odata]
        sized(res, f"utf8_{large}", call)
    return res


@case
def take_bits(E, M, n):
    idx, valid = _take_idx(n, 25)
    src = M.put(np.packbits(np.random.default_rng(26).random(N_SRC) < 0.5, bitorder="little"))
    d_idx, svb = M.put(idx), M.put(valid)
    out, ov = M.out((n + 7) // 8, np.uint8), M.out(n, np.uint8)
    st = E.call("ivx_take_bits", M.mem, src.p, u64(N_SRC), svb.p, d_idx.p, u64(n), out.p, ov.p, outs=[out, ov])
    return {"st": st, "bits": out.np()[:(n + 7) // 8], "valid": ov.np()[:n]}


@case
def take_view(E, M, n):
    strings = _strings(27)
    views = np.zeros((N_SRC, 16), np.uint8)
    bufs = [bytearray(), bytearray()]
    for i, s in enumerate(strings):
        views[i, :4] = np.frombuffer(np.uint32(len(s)).tobytes(), np.uint8)
        if len(s) <= 12:
            views[i, 4:4 + len(s)] = np.frombuffer(s, np.uint8)
        else:
            b = i & 1
            views[i, 4:8] = np.frombuffer(s[:4], np.uint8)
            views[i, 8:16] = np.frombuffer(np.array([b, len(bufs[b])], np.uint32).tobytes(), np.uint8)
            bufs[b] += s
    idx, valid = _take_idx(n, 28)
    d_views, d_idx, svb = M.put(views.reshape(-1)), M.put(idx), M.put(valid)
    d_bufs = [M.put(np.frombuffer(bytes(b), np.uint8)) for b in bufs]
    table = (C.c_void_p * 2)(*[b.p.value for b in d_bufs])      # a host table of the buffers' pointers, in either mode
    sizes = (C.c_uint64 * 2)(*[len(b) for b in bufs])
    head = (M.mem, d_views.p, table, sizes, u32(2), u64(N_SRC), svb.p, d_idx.p, u64(n))
    res = {}

    def call(cap, with_data):
        ov16, odata, ov = M.out(16 * n, np.uint8), M.out(cap, np.uint8), M.out(n, np.uint8)
        need = u64(0xDEAD)
        st = E.call("ivx_take_view", *head, ov16.p, odata.p if with_data else None, u64(cap), C.byref(need), ov.p,
                    outs=[ov16, odata, ov], count=need)
        if not with_data and need.value:
            assert untouched(ov16)                             # the views are withheld when the data did not fit
        res[f"views@{cap},{with_data}"] = ov16.np()[:16 * n]
        if st != CAPACITY:                                     # (a short buffer: host mode copies nothing back, device mode has the validity)
            res[f"valid@{cap},{with_data}"] = ov.np()[:n]
        return st, need.value, [odata]
    sized(res, "view", call)
    return res


def _same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b
