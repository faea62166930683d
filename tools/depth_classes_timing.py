"""Device-resident timing of the depth coverage classes (ivx_depth_profile_quantize / ivx_depth_profile_hist) on the short read
set of tools/depth_timing.py (1 GPU): N reads (default 50 M) of 150 bp on 24 contigs of 100 Mbp, one profile, the whole
position range as every contig's domain.

  quantize  (a) sizing + fill with the cuts 0:1:4:100:200: (mosdepth's example), every class emitted
            (b) sizing + fill with one cut at 10, only the upper class emitted ("the intervals at 10x or more")
            (c) ivx_depth_profile_blocks sizing + fill on the same profile: the same columns read, at least as many rows written
            (d) what a caller had before: ivx_depth_profile_read to device tensors, torch.bucketize on the cuts, the run heads
                by comparison with the step before, the zero stretches ahead of every contig's first step, torch.nonzero for
                the rows and the ends from the next row's start
  hist      (e) n_bins = 256 from v_lo = 0
            (f) n_bins = 65536 from v_lo = 0: more bins than a workgroup keeps in LDS, every add goes to memory
            (g) the region summaries' tile pass with four thresholds (one summarize call with one region): the same three
                columns read once
            (h) what a caller had before: 32 summarize calls of 8 thresholds (1 .. 255) over the 24 whole-contig regions,
                differenced
  check     before anything is timed: (a) and (b) equal (d) row for row; (e) equals (h); (f) equals (e) where (e) is not
            clamped, its tail adds up to (e)'s last bin, and every row of both adds up to 2^32

Warm-up + REPS repeats, min and median.  `device` is the context's event time of the calls (kernels and the wait for the
count between them); `stream` is a pair of events on the stream around everything, torch's kernels included.  Bytes are what
the device time amounts to per step at the 8 TB/s planning peak.

  N=50000000  REPS=5
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pyivx  # noqa: E402
from depth_timing import PEAK_BPS, dev, short_reads  # noqa: E402

CUTS5 = (0, 1, 4, 100, 200)
THR = (1, 10, 20, 30)
M32 = 0xFFFFFFFF


def stat(v):
    return dict(min=min(v), median=statistics.median(v))


def timed(ctx, f):
    """-> (result, device ms of the context's calls f made, stream ms around all of f)"""
    ctx.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.acc_ms = 0.0
    e0.record()
    out = f()
    e1.record()
    e1.synchronize()
    ms, ctx.acc_ms = ctx.acc_ms, None
    return out, ms, e0.elapsed_time(e1)


def repeat(ctx, f, reps):
    d, s = [], []
    for i in range(reps + 1):                               # (the first round warms up: code objects, scratch growth)
        out, ms, sm = timed(ctx, f)
        if i:
            d.append(ms); s.append(sm)
        if i < reps:
            del out
    return out, stat(d), stat(s)


def u32(t):
    return t.to(torch.int64) & M32


def old_quantize(ctx, prof, cuts, emit_mask):
    """read + torch: the runs of ivx_depth_profile_quantize over the whole position range -> (key, start, end, class) int64"""
    key, pos, cov, _ = prof.read(device=True, ctx=ctx)
    key, pos = u32(key), u32(pos)
    c = torch.tensor(cuts, dtype=torch.int32, device=dev)
    cls = torch.bucketize(cov, c, right=True)
    cls0 = int(np.searchsorted(np.asarray(cuts), 0, side="right"))
    first = torch.ones_like(key, dtype=torch.bool)
    first[1:] = key[1:] != key[:-1]
    prev = torch.empty_like(cls)
    prev[1:] = cls[:-1]
    prev[0] = cls0
    prev = torch.where(first, cls0, prev)                   # ahead of a contig's first step: the zero stretch, or nothing at position 0
    zero = first & (pos > 0)                                # the contig has a zero stretch
    head = (cls != prev) | (first & (pos == 0))
    # slot 2i: the zero stretch ahead of step i as a run of its own or joined by step i; slot 2i + 1: step i heads a run
    flags = torch.stack([zero, head], dim=1).reshape(-1)
    idx = torch.nonzero(flags).reshape(-1)
    step, is_zero = idx >> 1, (idx & 1) == 0
    rk = key[step]
    rs = torch.where(is_zero, 0, pos[step])
    rc = torch.where(is_zero, cls0, cls[step])
    re = torch.full_like(rs, M32)
    same = rk[1:] == rk[:-1]
    re[:-1] = torch.where(same, rs[1:] - 1, M32)
    keep = (torch.bitwise_right_shift(torch.full_like(rc, emit_mask), rc) & 1) == 1
    return rk[keep], rs[keep], re[keep], rc[keep]


def old_hist(ctx, prof, ck, cs, ce):
    """32 summarize calls of 8 thresholds over the whole-contig regions, differenced -> int64 [24, 256]"""
    ge = []
    bases = None
    for t0 in range(1, 256, 8):
        thr = tuple(range(t0, min(t0 + 8, 256)))
        ln, _, g = prof.summarize(ck, cs, ce, thr, ctx=ctx, outputs=(bases is None, False, True))
        bases = ln if bases is None else bases
        ge.append(g)
    ge = torch.cat([bases.reshape(1, -1)] + ge + [torch.zeros_like(bases).reshape(1, -1)])      # ge(t) for t = 0 (everything) .. 256 (nothing: see below)
    h = (ge[:-1] - ge[1:]).t().contiguous()                 # bin b = ge(b) - ge(b + 1), b < 255; bin 255 = ge(255): clamped
    return h


def main():
    n, reps = int(float(os.environ.get("N", 50_000_000))), int(os.environ.get("REPS", "5"))
    ctx = pyivx.Ctx(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    prof = ctx.depth_profile(**short_reads(n, 0x5EED0D01))
    torch.cuda.empty_cache()
    steps = prof.steps()
    res = dict(reads=n, reps=reps, steps=steps, class_tile=pyivx.DEPTH_CLASS_TILE, hist_lds_bins=pyivx.DEPTH_HIST_LDS_BINS)
    per_step = lambda st: st["median"] / 1e3 * PEAK_BPS / max(steps, 1)

    # ---- the equality checks, before anything is timed
    checks = {}
    for name, cuts, mask in (("cuts5", CUTS5, 0b111111), ("ge10", (10,), 0b10)):
        got = [u32(g) for g in prof.quantize(cuts, mask, device=True)]
        want = old_quantize(ctx, prof, cuts, mask)
        ctx.synchronize()
        checks[name + "_equals_torch"] = all(g.shape == w.shape and bool(torch.equal(g, w)) for g, w in zip(got, want))
        checks[name + "_rows"] = int(got[0].numel())
        del got, want
    ck = torch.arange(24, dtype=torch.int32, device=dev)
    cs, ce = torch.zeros(24, dtype=torch.int32, device=dev), torch.full((24,), -1, dtype=torch.int32, device=dev)     # (end = 2^32 - 1)
    h256 = prof.hist(0, 256, device=True)
    h64k = prof.hist(0, 65536, device=True)
    hold = old_hist(ctx, prof, ck, cs, ce)
    ctx.synchronize()
    checks["hist256_equals_summarize_differenced"] = bool(torch.equal(h256, hold))
    checks["hist65536_equals_hist256"] = bool(torch.equal(h64k[:, :255], h256[:, :255])) and bool(torch.equal(h64k[:, 255:].sum(1), h256[:, 255]))
    checks["rows_add_up_to_the_domain"] = bool((h256.sum(1) == 1 << 32).all()) and bool((h64k.sum(1) == 1 << 32).all())
    checks["bins_not_zero_256"] = int((h256 != 0).sum())
    checks["max_coverage"] = int(torch.nonzero(h64k.sum(0)).max())
    res["checks"] = checks
    del h256, h64k, hold
    assert all(v for k, v in checks.items() if isinstance(v, bool)), checks
    torch.cuda.empty_cache()

    # ---- quantize
    q = {}
    out, d, s = repeat(ctx, lambda: prof.quantize(CUTS5, device=True), reps)
    q["cuts5"] = dict(rows=int(out[0].numel()), device_ms=d, stream_ms=s, bytes_per_step_at_8TBps=per_step(d))
    del out
    out, d, s = repeat(ctx, lambda: prof.quantize((10,), 0b10, device=True), reps)
    q["ge10"] = dict(rows=int(out[0].numel()), device_ms=d, stream_ms=s, bytes_per_step_at_8TBps=per_step(d))
    del out
    out, d, s = repeat(ctx, lambda: prof.blocks(device=True), reps)
    q["blocks"] = dict(rows=int(out[0].numel()), device_ms=d, stream_ms=s, bytes_per_step_at_8TBps=per_step(d))
    del out
    torch.cuda.empty_cache()
    out, d, s = repeat(ctx, lambda: old_quantize(ctx, prof, CUTS5, 0b111111), reps)
    q["read_and_torch_cuts5"] = dict(rows=int(out[0].numel()), stream_ms=s)
    del out
    torch.cuda.empty_cache()
    q["cuts5_over_blocks_device"] = q["cuts5"]["device_ms"]["median"] / q["blocks"]["device_ms"]["median"]
    q["torch_over_cuts5_stream"] = q["read_and_torch_cuts5"]["stream_ms"]["median"] / q["cuts5"]["stream_ms"]["median"]
    res["quantize"] = q

    # ---- hist
    h = {}
    for name, nb in (("bins256", 256), ("bins65536", 65536)):
        out, d, s = repeat(ctx, lambda: prof.hist(0, nb, device=True), reps)
        h[name] = dict(device_ms=d, stream_ms=s, bytes_per_step_at_8TBps=per_step(d))
        del out
    out, d, s = repeat(ctx, lambda: prof.summarize(ck[:1], cs[:1], ce[:1], THR), reps)
    h["region_tile_pass_4_thresholds"] = dict(device_ms=d, stream_ms=s, bytes_per_step_at_8TBps=per_step(d))
    out, d, s = repeat(ctx, lambda: old_hist(ctx, prof, ck, cs, ce), reps)
    h["summarize_32_calls"] = dict(device_ms=d, stream_ms=s)
    del out
    h["bins256_over_tile_pass_device"] = h["bins256"]["device_ms"]["median"] / h["region_tile_pass_4_thresholds"]["device_ms"]["median"]
    h["summarize_32_calls_over_bins256_device"] = h["summarize_32_calls"]["device_ms"]["median"] / h["bins256"]["device_ms"]["median"]
    h["beats_the_old_way"] = h["bins256"]["device_ms"]["median"] < h["summarize_32_calls"]["device_ms"]["median"] and \
        h["bins256"]["stream_ms"]["median"] < h["summarize_32_calls"]["stream_ms"]["median"]
    res["hist"] = h
    print(json.dumps(res), flush=True)
    assert h["beats_the_old_way"], h
    prof.free()
    ctx.close()


if __name__ == "__main__":
    main()
