"""Device-resident timing of depth() (ivx_depth) on two synthetic read sets from fixed seeds (1 GPU):

  short   N reads (default 50 M) of 150 bp on 24 contigs, in (contig, start) order; 90 % `150M`, 5 % `10S140M`,
          5 % `70M2D80M`
  long    reads of about 20 000 ops each (M / I / M / D ... with short lengths).  An Arrow Binary column holds at most
          2^31 bytes = 2^29 ops, so the default is 25 000 such reads (5 * 10^8 ops), not more.

For each set: a warm-up, then REPS times a sizing call plus a fill call; per call the device time the context's events
measured (ivx_ctx_last_kernel_ms), median and spread over the repeats, reads/s and events/s of the sizing + fill pair, the
algorithmic bytes per event the time implies at the 8 TB/s planning peak, and the time of the vectorised numpy
restatement (tests/depth_oracle.py) on the same columns as context (CHECK=1 also compares the blocks).  The per-kernel
split comes from a run of its own under the kernel tracer: tools/kstats.sh depth tools/depth_timing.py (set REPS=1).

  SETS=short,long  N_SHORT=50000000  N_LONG=25000  OPS_LONG=20000  REPS=5  CHECK=0  ORACLE=short (sets the restatement runs on)
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyivx  # noqa: E402

dev = torch.device("cuda:0")
M, I, D, S = 0, 1, 2, 4
PEAK_BPS = 8e12


def short_reads(n, seed):
    g = torch.Generator(device=dev); g.manual_seed(seed)
    key = torch.randint(0, 24, (n,), generator=g, device=dev, dtype=torch.int64)
    pos = torch.randint(0, 100_000_000, (n,), generator=g, device=dev, dtype=torch.int64)
    o = torch.argsort((key << 32) | pos)
    key, pos = key[o].to(torch.int32).contiguous(), pos[o].to(torch.int32).contiguous()
    del o
    kind = torch.rand(n, generator=g, device=dev)
    nops = torch.where(kind < 0.90, 1, torch.where(kind < 0.95, 2, 3)).to(torch.int64)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(nops, 0, out=off[1:])
    first = off[:-1]
    ops = torch.empty(int(off[-1]), dtype=torch.int32, device=dev)
    one, two, three = nops == 1, nops == 2, nops == 3
    ops[first[one]] = (150 << 4) | M
    ops[first[two]] = (10 << 4) | S
    ops[first[two] + 1] = (140 << 4) | M
    ops[first[three]] = (70 << 4) | M
    ops[first[three] + 1] = (2 << 4) | D
    ops[first[three] + 2] = (80 << 4) | M
    return dict(rkey=key, rpos=pos, rflags=torch.zeros(n, dtype=torch.int32, device=dev), rmapq=torch.full((n,), 60, dtype=torch.int32, device=dev),
                cigar_offsets=(4 * off).to(torch.int32).contiguous(), cigar_ops=ops, n_keys=24)


def long_reads(n, ops_each, seed):
    g = torch.Generator(device=dev); g.manual_seed(seed)
    nops = torch.randint(ops_each - ops_each // 10, ops_each + ops_each // 10, (n,), generator=g, device=dev, dtype=torch.int64)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(nops, 0, out=off[1:])
    T = int(off[-1])
    assert 4 * T < 2 ** 31, "an Arrow Binary column holds at most 2^31 bytes of CIGAR ops"
    idx = torch.arange(T, device=dev, dtype=torch.int64)
    ln = torch.randint(1, 30, (T,), generator=g, device=dev, dtype=torch.int32)
    gap = torch.where(torch.rand(T, generator=g, device=dev) < 0.5, I, D).to(torch.int32)
    ops = torch.where(idx % 2 == 0, (ln << 4) | M, ((ln % 3 + 1) << 4) | gap).to(torch.int32).contiguous()
    del idx, ln, gap
    key = torch.sort(torch.randint(0, 24, (n,), generator=g, device=dev, dtype=torch.int32)).values.contiguous()
    pos = torch.randint(0, 100_000_000, (n,), generator=g, device=dev, dtype=torch.int32)
    return dict(rkey=key, rpos=pos, rflags=torch.zeros(n, dtype=torch.int32, device=dev), rmapq=torch.full((n,), 60, dtype=torch.int32, device=dev),
                cigar_offsets=(4 * off).to(torch.int32).contiguous(), cigar_ops=ops, n_keys=24)


def n_events(kw):
    code = kw["cigar_ops"] & 15
    return 2 * int(((code == 0) | (code == 7) | (code == 8)).sum())


def measure(ctx, name, kw, reps):
    lib = pyivx.lib()
    n_reads, ev = int(kw["rpos"].numel()), n_events(kw)
    n_ops = int(kw["cigar_ops"].numel())

    def pair():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.depth(cap=None, **kw)                   # a sizing call, then the fill call
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    # the two calls apart, for their device times
    import ctypes as C
    P = lambda t: C.c_void_p(t.data_ptr())
    args = (pyivx.MEM_DEVICE, P(kw["rkey"]), P(kw["rpos"]), P(kw["rflags"]), P(kw["rmapq"]), P(kw["cigar_offsets"]), P(kw["cigar_ops"]), n_reads,
            None, None, None, None, 0, kw["n_keys"], None, 1796, 0)

    def two_calls():
        m = C.c_uint64(0)
        ctx._chk(lib.ivx_depth(ctx.h, *args, None, None, None, None, 0, C.byref(m)))
        ctx.synchronize()
        size_ms = ctx.last_kernel_ms()
        out = [torch.empty(max(m.value, 1), dtype=torch.int32, device=dev) for _ in range(4)]
        m2 = C.c_uint64(0)
        ctx._chk(lib.ivx_depth(ctx.h, *args, *[P(o) for o in out], m.value, C.byref(m2)))
        ctx.synchronize()
        return size_ms, ctx.last_kernel_ms(), m2.value, out

    two_calls()                                     # warm-up: code objects, scratch growth
    size, fill, wall, blocks = [], [], [], 0
    for _ in range(reps):
        a, b, blocks, out = two_calls()
        size.append(a); fill.append(b)
        del out
        wall.append(pair() * 1e3)
    med = lambda v: statistics.median(v)
    pair_ms = med(size) + med(fill)
    res = dict(set=name, reads=n_reads, ops=n_ops, events=ev, blocks=blocks, reps=reps,
               sizing_ms=dict(median=med(size), min=min(size), max=max(size)), fill_ms=dict(median=med(fill), min=min(fill), max=max(fill)),
               pair_wall_ms=dict(median=med(wall), min=min(wall), max=max(wall)),
               reads_per_s=n_reads / (pair_ms / 1e3), events_per_s=ev / (pair_ms / 1e3),
               bytes_per_event_at_8TBps_one_call=med(fill) / 1e3 * PEAK_BPS / max(ev, 1))
    if name in os.environ.get("ORACLE", "short").split(","):
        import depth_oracle as orc
        host = {k: (v.cpu().numpy().view(np.uint32) if k not in ("cigar_offsets",) else v.cpu().numpy()) for k, v in kw.items() if torch.is_tensor(v)}
        t0 = time.perf_counter()
        want = orc.depth_numpy(**host)
        res["numpy_restatement_s"] = time.perf_counter() - t0
        if os.environ.get("CHECK", "0") == "1":
            got = ctx.depth(**kw)
            res["matches_restatement"] = all(np.array_equal(g.cpu().numpy().view(w.dtype), w) for g, w in zip(got, want))
    print(json.dumps(res), flush=True)
    return res


def main():
    sets = os.environ.get("SETS", "short,long").split(",")
    reps = int(os.environ.get("REPS", "5"))
    ctx = pyivx.Ctx(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = []
    if "short" in sets:
        kw = short_reads(int(float(os.environ.get("N_SHORT", 50_000_000))), 0x5EED0D01)
        out.append(measure(ctx, "short", kw, reps))
        del kw
        torch.cuda.empty_cache()
    if "long" in sets:
        kw = long_reads(int(float(os.environ.get("N_LONG", 25_000))), int(float(os.environ.get("OPS_LONG", 20_000))), 0x5EED0D02)
        out.append(measure(ctx, "long", kw, reps))
    if len(out) == 2:
        r = out[0]["events_per_s"] / out[1]["events_per_s"]
        print(json.dumps(dict(short_over_long_events_per_s=r, op_parallel_within_2x=bool(0.5 <= r <= 2.0))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
