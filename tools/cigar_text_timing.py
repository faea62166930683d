"""Device-resident timing of the text-CIGAR path (ivx_cigar_parse, ivx_depth_text) on the two read sets of
tools/depth_timing.py, their CIGARs rendered as text on the device (1 GPU):

  short   N reads (default 50 M): 90 % `150M`, 5 % `10S140M`, 5 % `70M2D80M`
  long    25 000 reads of about 20 000 ops each (`17M2I23M1D...`)

For each set, after a warm-up, REPS times:
  parse        ivx_cigar_parse alone: the counting call and the call that writes offsets and ops (wall time around the call,
               which synchronises; the call is not bracketed by the context's events)
  text depth   ivx_depth_text, a sizing call plus a fill call: device time (ivx_ctx_last_kernel_ms, which covers the parse)
               and wall time
  binary depth ivx_depth on the same reads as packed ops, the same way
and from the medians: the parse's text bytes per second against the 8 TB/s planning peak, the extra time of the text pair
over the binary pair, and that extra time against two stand-alone parses (each of the two text calls parses).

  SETS=short,long  N_SHORT=50000000  N_LONG=25000  OPS_LONG=20000  REPS=5  CHECK=1 (text blocks == binary blocks)
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pyivx  # noqa: E402
from depth_timing import dev, long_reads, short_reads, PEAK_BPS  # noqa: E402

LETTERS = torch.tensor(list(b"MIDNSHP=X"), dtype=torch.uint8)


def render(kw):
    """the packed ops of a read set -> (text_offsets int32 / int64 [n + 1], text uint8) on the device"""
    ops = kw["cigar_ops"]
    ln, code = (ops >> 4).to(torch.int64), (ops & 15).to(torch.int64)
    nd = torch.ones_like(ln)
    p = 10
    while int(ln.max()) >= p:
        nd += (ln >= p).to(torch.int64)
        p *= 10
    start = torch.zeros(len(ops) + 1, dtype=torch.int64, device=dev)
    torch.cumsum(nd + 1, 0, out=start[1:])
    total = int(start[-1])
    text = torch.empty(total, dtype=torch.uint8, device=dev)
    text[start[:-1] + nd] = LETTERS.to(dev)[code]
    for d in range(int(nd.max())):
        m = nd > d
        digit = (ln[m] // (10 ** (nd[m] - 1 - d))) % 10
        text[start[:-1][m] + d] = (digit + 48).to(torch.uint8)
    off = start[(kw["cigar_offsets"].to(torch.int64) // 4)]
    return (off if total >= 2 ** 31 else off.to(torch.int32)).contiguous(), text


def med(v):
    return statistics.median(v)


def stats(v):
    return dict(median=med(v), min=min(v), max=max(v))


def measure(ctx, name, kw, reps):
    lib = pyivx.lib()
    toff, text = render(kw)
    n_reads, n_ops, n_bytes = int(kw["rpos"].numel()), int(kw["cigar_ops"].numel()), int(text.numel())
    large = int(toff.dtype == torch.int64)
    P = lambda t: C.c_void_p(t.data_ptr())
    out_off = torch.empty(n_reads + 1, dtype=torch.int32, device=dev)
    out_ops = torch.empty(n_ops, dtype=torch.int32, device=dev)

    def parse(write):
        m = C.c_uint64(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx._chk0(lib.ivx_cigar_parse(ctx.h, pyivx.MEM_DEVICE, large, P(toff), P(text), n_reads,
                                      P(out_off) if write else None, P(out_ops) if write else None, n_ops if write else 0, C.byref(m)))
        torch.cuda.synchronize()
        assert m.value == n_ops
        return (time.perf_counter() - t0) * 1e3

    head = (pyivx.MEM_DEVICE, P(kw["rkey"]), P(kw["rpos"]), P(kw["rflags"]), P(kw["rmapq"]))
    tail = (n_reads, None, None, None, None, 0, kw["n_keys"], None, 1796, 0)
    forms = dict(binary=(lib.ivx_depth, head + (P(kw["cigar_offsets"]), P(kw["cigar_ops"])) + tail),
                 text=(lib.ivx_depth_text, head + (large, P(toff), P(text)) + tail))

    def pair(form):
        fn, args = forms[form]
        m, m2 = C.c_uint64(0), C.c_uint64(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx._chk(fn(ctx.h, *args, None, None, None, None, 0, C.byref(m)))
        ctx.synchronize()
        size_ms = ctx.last_kernel_ms()
        out = [torch.empty(max(m.value, 1), dtype=torch.int32, device=dev) for _ in range(4)]
        ctx._chk(fn(ctx.h, *args, *[P(o) for o in out], m.value, C.byref(m2)))
        ctx.synchronize()
        return size_ms, ctx.last_kernel_ms(), (time.perf_counter() - t0) * 1e3, out, m2.value

    parse(False); parse(True); pair("binary"); pair("text")                 # warm-up: code objects, scratch growth
    res = dict(set=name, reads=n_reads, ops=n_ops, text_bytes=n_bytes, large_offsets=bool(large), reps=reps)
    if os.environ.get("CHECK", "1") == "1":
        assert torch.equal(out_ops, kw["cigar_ops"]) and torch.equal(out_off, kw["cigar_offsets"])
        b, t = pair("binary"), pair("text")
        res["parse_matches_the_ops"] = True
        res["text_blocks_match_binary"] = b[4] == t[4] and all(torch.equal(x[:b[4]], y[:b[4]]) for x, y in zip(b[3], t[3]))
        del b, t
    count, write = [parse(False) for _ in range(reps)], [parse(True) for _ in range(reps)]
    t = dict(binary=[], text=[])
    for _ in range(reps):                                                   # the two forms alternate
        for f in t:
            t[f].append(pair(f)[:3])
    for f in t:
        res[f + "_sizing_ms"] = stats([x[0] for x in t[f]])
        res[f + "_fill_ms"] = stats([x[1] for x in t[f]])
        res[f + "_pair_wall_ms"] = stats([x[2] for x in t[f]])
    dev_pair = {f: res[f + "_sizing_ms"]["median"] + res[f + "_fill_ms"]["median"] for f in t}
    res["parse_count_wall_ms"], res["parse_write_wall_ms"] = stats(count), stats(write)
    res["parse_text_bytes_per_s"] = n_bytes / (med(write) / 1e3)
    res["parse_fraction_of_8TBps"] = res["parse_text_bytes_per_s"] / PEAK_BPS
    res["text_minus_binary_pair_device_ms"] = dev_pair["text"] - dev_pair["binary"]
    res["text_minus_binary_pair_wall_ms"] = res["text_pair_wall_ms"]["median"] - res["binary_pair_wall_ms"]["median"]
    res["two_standalone_parses_wall_ms"] = 2 * med(write)
    print(json.dumps(res), flush=True)
    return res


def main():
    sets = os.environ.get("SETS", "short,long").split(",")
    reps = int(os.environ.get("REPS", "5"))
    ctx = pyivx.Ctx(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    if "short" in sets:
        kw = short_reads(int(float(os.environ.get("N_SHORT", 50_000_000))), 0x5EED0D01)
        measure(ctx, "short", kw, reps)
        del kw
        torch.cuda.empty_cache()
    if "long" in sets:
        kw = long_reads(int(float(os.environ.get("N_LONG", 25_000))), int(float(os.environ.get("OPS_LONG", 20_000))), 0x5EED0D02)
        measure(ctx, "long", kw, reps)
    ctx.close()


if __name__ == "__main__":
    main()
