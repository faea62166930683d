"""Device-resident timing of per-base depth() (ivx_depth_profile_build / ivx_depth_profile_expand) on one synthetic read
set from a fixed seed (1 GPU): N reads (default 2 M) of 150 bp on the 24 GRCh38 primary contigs (their lengths as key_len),
in (contig, start) order, CIGARs as tools/depth_timing.py's short set.

  check    a 2^21-position window of key 0 against a numpy restatement (delta array + cumulative sum) in the same run
  build    the profile build; next to it ivx_depth's sizing call on the same columns (they share the front half)
  expand   key 0 over its whole length (248 956 422 positions): coverage only, and coverage + positions
  fill     tensor.zero_() over the same output bytes: the yardstick (a plain device fill)

Warm-up + REPS repeats, median [min-max] of the device time (the context's events; torch events for the fills), GB/s of
the bytes written, and the expand / fill ratio.

  N=2000000  REPS=5
"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402

dev = torch.device("cuda:0")
GRCH38 = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422, 135086622,
          133275309, 114364328, 107043718, 101991189, 90338345, 83257441, 80373285, 58617616, 64444167, 46709983, 50818468,
          156040895, 57227415]


def reads(n, seed):
    g = torch.Generator(device=dev); g.manual_seed(seed)
    lens = torch.tensor(GRCH38, dtype=torch.float64, device=dev)
    key = torch.multinomial(lens / lens.sum(), n, replacement=True, generator=g).to(torch.int64)
    pos = (torch.rand(n, generator=g, device=dev, dtype=torch.float64) * lens[key]).to(torch.int64)
    o = torch.argsort((key << 32) | pos)
    key, pos = key[o].to(torch.int32).contiguous(), pos[o].to(torch.int32).contiguous()
    kind = torch.rand(n, generator=g, device=dev)
    nops = torch.where(kind < 0.90, 1, torch.where(kind < 0.95, 2, 3)).to(torch.int64)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(nops, 0, out=off[1:])
    first = off[:-1]
    ops = torch.empty(int(off[-1]), dtype=torch.int32, device=dev)
    one, two, three = nops == 1, nops == 2, nops == 3
    ops[first[one]] = (150 << 4) | 0
    ops[first[two]] = (10 << 4) | 4
    ops[first[two] + 1] = (140 << 4) | 0
    ops[first[three]] = (70 << 4) | 0
    ops[first[three] + 1] = (2 << 4) | 2
    ops[first[three] + 2] = (80 << 4) | 0
    return dict(rkey=key, rpos=pos, rflags=torch.zeros(n, dtype=torch.int32, device=dev), rmapq=torch.full((n,), 60, dtype=torch.int32, device=dev),
                cigar_offsets=(4 * off).to(torch.int32).contiguous(), cigar_ops=ops, n_keys=24,
                key_len=torch.tensor(GRCH38, dtype=torch.int64, device=dev).to(torch.int32).contiguous())


def stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def check_window(ctx, prof, kw, n):
    """the first n positions of key 0 against a delta array + cumulative sum over the same reads"""
    k0 = (kw["rkey"] == 0).cpu().numpy()
    pos = kw["rpos"].cpu().numpy()[k0].astype(np.int64)
    off = (kw["cigar_offsets"].cpu().numpy() // 4)
    ops = kw["cigar_ops"].cpu().numpy()
    lo, hi = off[:-1][k0], off[1:][k0]
    depth = np.zeros(n + 1, np.int64)
    for j in range(3):                                      # at most three ops a read
        m = lo + j < hi
        w = ops[(lo + j)[m]].astype(np.int64)
        ln, code = w >> 4, w & 15
        s = pos[m]
        e = s + np.where(code == 4, 0, ln)
        emit = code == 0
        np.add.at(depth, s[emit & (s <= n)], 1)
        np.add.at(depth, e[emit & (e <= n)], -1)
        pos[m] = e
    want = np.cumsum(depth)[:n].astype(np.int16)
    gp, gc = prof.expand(0, 0, n, device=True)
    ctx.synchronize()
    return bool(np.array_equal(gc.cpu().numpy(), want) and np.array_equal(gp.cpu().numpy(), np.arange(n, dtype=np.int32)))


def main():
    n, reps = int(float(os.environ.get("N", 2_000_000))), int(os.environ.get("REPS", "5"))
    ctx = pyivx.Ctx(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    kw = reads(n, 0x5EED0D03)
    lib = pyivx.lib()
    res = dict(reads=n, reps=reps)

    def build():
        p = ctx.depth_profile(**kw)
        return p, ctx.last_kernel_ms()

    prof, _ = build()                                       # warm-up: code objects, scratch growth
    res["steps"], res["profile_bytes"] = prof.steps(), prof.device_bytes
    res["window_2p21_matches_numpy"] = check_window(ctx, prof, kw, 1 << 21)
    prof.free()
    b = []
    for _ in range(reps):
        p, ms = build()
        b.append(ms)
        if len(b) < reps:
            p.free()
    prof = p
    res["profile_build_ms"] = stat(b)
    # ivx_depth's sizing call on the same columns
    P = lambda t: C.c_void_p(t.data_ptr())
    args = (pyivx.MEM_DEVICE, P(kw["rkey"]), P(kw["rpos"]), P(kw["rflags"]), P(kw["rmapq"]), P(kw["cigar_offsets"]), P(kw["cigar_ops"]), n,
            None, None, None, None, 0, 24, P(kw["key_len"]), 1796, 0)
    s = []
    for i in range(reps + 1):
        m = C.c_uint64(0)
        ctx._chk(lib.ivx_depth(ctx.h, *args, None, None, None, None, 0, C.byref(m)))
        ctx.synchronize()
        if i:
            s.append(ctx.last_kernel_ms())
    res["depth_sizing_ms"] = stat(s)
    res["build_over_sizing"] = res["profile_build_ms"]["median"] / res["depth_sizing_ms"]["median"]

    L = GRCH38[0]
    cov = torch.empty(L, dtype=torch.int16, device=dev)
    pos = torch.empty(L, dtype=torch.int32, device=dev)

    def expand(with_pos):
        v = []
        for i in range(reps + 1):
            prof.expand(0, 0, L, want_pos=with_pos, out_cov=cov, out_pos=pos if with_pos else None)
            ctx.synchronize()
            if i:
                v.append(ctx.last_kernel_ms())
        return v

    def fill(tensors):
        v = []
        for i in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for t in tensors:
                t.zero_()
            e1.record()
            torch.cuda.synchronize()
            if i:
                v.append(e0.elapsed_time(e1))
        return v

    for name, with_pos, tensors, nbytes in (("coverage", False, [cov], 2 * L), ("coverage_and_positions", True, [cov, pos], 6 * L)):
        f, x = stat(fill(tensors)), stat(expand(with_pos))
        res[name] = dict(positions=L, bytes=nbytes, expand_ms=x, fill_ms=f, expand_GBps=nbytes / x["median"] / 1e6, fill_GBps=nbytes / f["median"] / 1e6,
                         expand_over_fill=x["median"] / f["median"])
    print(json.dumps(res), flush=True)
    prof.free()
    ctx.close()


if __name__ == "__main__":
    main()
