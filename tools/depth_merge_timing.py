"""Device-resident timing of streaming depth() (ivx_depth_profile_merge / ivx_depth_profile_blocks) on the short read set of
tools/depth_timing.py (1 GPU): N reads (default 50 M) of 150 bp on 24 contigs, in (contig, start) order.

  halves   the set split in two, two ways: `interleaved` (even / odd reads: both profiles span every contig, the merge
           alternates between them all the way) and `consecutive` (first / second half: the merge is nearly a concatenation)
  merge    ivx_depth_profile_merge of the two halves' profiles
  blocks   ivx_depth_profile_blocks of the result: the sizing call and the fill call apart
  build    the one-shot ivx_depth_profile_build of the whole set: what obtaining the same profile costs without a merge
  check    the merged profile's columns against the one-shot profile's, on the device, in the same run

Warm-up + REPS repeats, median [min-max] of the device time (the context's events), and what the time amounts to per input
step at the 8 TB/s planning peak.

  N=50000000  REPS=5
"""
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pyivx  # noqa: E402
from depth_timing import PEAK_BPS, dev, short_reads  # noqa: E402


def take(kw, idx):
    """the reads `idx` (ascending int64 tensor) of a read set, CIGARs included"""
    off = (kw["cigar_offsets"].to(torch.int64) // 4)
    nops = (off[1:] - off[:-1])[idx]
    noff = torch.zeros(idx.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(nops, 0, out=noff[1:])
    src = torch.repeat_interleave(off[:-1][idx] - noff[:-1], nops) + torch.arange(int(noff[-1]), device=dev)
    out = dict(kw)
    for c in ("rkey", "rpos", "rflags", "rmapq"):
        out[c] = kw[c][idx].contiguous()
    out["cigar_offsets"] = (4 * noff).to(torch.int32).contiguous()
    out["cigar_ops"] = kw["cigar_ops"][src].contiguous()
    return out


def stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    n, reps = int(float(os.environ.get("N", 50_000_000))), int(os.environ.get("REPS", "5"))
    ctx = pyivx.Ctx(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lib = pyivx.lib()
    kw = short_reads(n, 0x5EED0D01)
    res = dict(reads=n, reps=reps, merge_tile=pyivx.DEPTH_MERGE_TILE)

    b = []
    whole = None
    for i in range(reps + 1):                               # (the first one warms up: code objects, scratch growth)
        if whole is not None:
            whole.free()
        whole = ctx.depth_profile(**kw)
        if i:
            b.append(ctx.last_kernel_ms())
    res["steps"], res["profile_bytes"] = whole.steps(), whole.device_bytes
    res["one_shot_build_ms"] = stat(b)
    want = whole.read(device=True)

    ar = torch.arange(n, device=dev)
    for name, ia, ib in (("interleaved", ar[0::2], ar[1::2]), ("consecutive", ar[:n // 2], ar[n // 2:])):
        pa, pb = ctx.depth_profile(**take(kw, ia)), ctx.depth_profile(**take(kw, ib))
        torch.cuda.empty_cache()
        steps_in = pa.steps() + pb.steps()
        m, v = None, []
        for i in range(reps + 1):
            if m is not None:
                m.free()
            m = pa.merge(pb)
            if i:
                v.append(ctx.last_kernel_ms())
        got = m.read(device=True)
        same = all(g.shape == w.shape and bool(torch.equal(g, w)) for g, w in zip(got, want))
        del got
        r = dict(steps_a=pa.steps(), steps_b=pb.steps(), steps_out=m.steps(), equals_one_shot=same, merge_ms=stat(v))
        r["merge_bytes_per_input_step_at_8TBps"] = r["merge_ms"]["median"] / 1e3 * PEAK_BPS / steps_in
        r["merge_over_one_shot_build"] = r["merge_ms"]["median"] / res["one_shot_build_ms"]["median"]
        # blocks: the sizing call and the fill call apart
        size, fill, nb = [], [], 0
        for i in range(reps + 1):
            c = C.c_uint64(0)
            ctx._chk(lib.ivx_depth_profile_blocks(ctx.h, m.h, pyivx.MEM_DEVICE, None, None, None, None, 0, C.byref(c)))
            ctx.synchronize()
            s_ms = ctx.last_kernel_ms()
            out = [torch.empty(max(c.value, 1), dtype=torch.int32, device=dev) for _ in range(4)]
            c2 = C.c_uint64(0)
            ctx._chk(lib.ivx_depth_profile_blocks(ctx.h, m.h, pyivx.MEM_DEVICE, *[C.c_void_p(o.data_ptr()) for o in out], c.value, C.byref(c2)))
            ctx.synchronize()
            if i:
                size.append(s_ms); fill.append(ctx.last_kernel_ms())
            nb = c2.value
            del out
        r["blocks"] = nb
        r["blocks_sizing_ms"], r["blocks_fill_ms"] = stat(size), stat(fill)
        r["blocks_fill_bytes_per_step_at_8TBps"] = r["blocks_fill_ms"]["median"] / 1e3 * PEAK_BPS / max(m.steps(), 1)
        res[name] = r
        for p in (pa, pb, m):
            p.free()
    print(json.dumps(res), flush=True)
    whole.free()
    ctx.close()


if __name__ == "__main__":
    main()
