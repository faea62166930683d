"""Device-resident timing of the overlap aggregates (ivx_probe_overlap_agg) on the headline shape of bench.py (1 GPU): N probe
rows (default 100 M, mean 150 bp) against 1 M build rows (mean 1000 bp) on 24 contigs, unsorted, from synth.py; one int32
value per build row.

  agg       ivx_probe_overlap_agg for count+sum, count+sum+min+max and all six outputs, on the path the library picks
  floor     ivx_probe_overlap_count(per_row) on the same inputs: the same walk with one u32 per row
  old way   what a caller had before: ivx_probe_overlap_count (total), ivx_probe_overlap_fill, ivx_take_fixed of the value
            column by build_idx, then a segment reduction in torch by probe_idx (index_add_ / scatter_reduce_) for
            count, sum, min and max.  Timed in the same run, alternating with agg.
  check     the old way's count, sum, min and max equal the fused call's on every row (min / max where the count is not 0)
  paths     direct against region path (IVX_JOIN_PATH) at 2^20 .. 2^25 and N rows, for the three output sets

Warm-up + REPS repeats, median [min-max] of torch events around the calls on the context's stream (kernels, the gaps
between them and, for the old way, the host round trip of its count).

  N=100000000  REPS=5   ONLY=paths: the paths part alone; ROWS=8388608,100000000: its batch sizes
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402
import synth  # noqa: E402

dev = torch.device("cuda:0")
SETS = {"count+sum": ("count", "sum"), "count+sum+min+max": ("count", "sum", "min", "max"), "all six": pyivx.AGG_OUTPUTS}
I64_MAX, I64_MIN = 2**63 - 1, -2**63


def stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def fmt(s):
    return f"{s['median']:9.3f} [{s['min']:.3f}-{s['max']:.3f}] ms"


def timed(f):
    """-> (result, ms between two events around f on the current stream)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = f()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def repeat(f, reps):
    v = []
    for i in range(reps + 1):                               # (the first round warms up: code objects, scratch growth)
        out, ms = timed(f)
        if i:
            v.append(ms)
    return out, stat(v)


def main():
    n, reps = int(float(os.environ.get("N", 100_000_000))), int(os.environ.get("REPS", "5"))
    ctx = pyivx.Ctx(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    bk, bs, be = synth.gen_torch(1_000_000, 1000, 24, 0x5EED0004, dev)
    pk, ps, pe = synth.gen_torch(n, 150, 24, 0x5EED0005, dev)
    g = torch.Generator(device=dev); g.manual_seed(0xA66)
    val = torch.randint(-1000, 1000, (1_000_000,), generator=g, device=dev, dtype=torch.int32)
    ix = ctx.build(pyivx.KIND_OVERLAP, bk, bs, be, n_keys=24)
    res = dict(probe_rows=n, build_rows=1_000_000, reps=reps, layout=ix.layout())
    os.environ.pop("IVX_JOIN_PATH", None)
    if os.environ.get("ONLY") != "paths":
        fused_floor_old(ctx, ix, pk, ps, pe, val, n, reps, res)
    sizes = {int(float(x)) for x in os.environ["ROWS"].split(",")} if os.environ.get("ROWS") else {1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24, 1 << 25, n}

    # ---- direct against regions by batch size
    res["paths"] = []
    print("  rows        outputs            direct                              regions")
    for m in sorted(sizes):
        if m > n:
            continue
        qk, qs, qe = pk[:m], ps[:m], pe[:m]
        for name in SETS:
            row = dict(rows=m, outputs=name)
            for path in ("direct", "regions"):
                os.environ["IVX_JOIN_PATH"] = path
                _, row[path] = repeat(lambda: ctx.overlap_agg(ix, qk, qs, qe, val, outputs=SETS[name]), reps)
                torch.cuda.empty_cache()
            os.environ.pop("IVX_JOIN_PATH", None)
            res["paths"].append(row)
            print(f"  {m:<11d} {name:<18} {fmt(row['direct'])}   {fmt(row['regions'])}")
    print(json.dumps(res), flush=True)
    ix.free()
    ctx.close()


def fused_floor_old(ctx, ix, pk, ps, pe, val, n, reps, res):
    """the fused call, the floor and the old way, alternating"""
    def old_way():
        total = ctx.overlap_count(ix, pk, ps, pe)
        ob, op = ctx.overlap_fill(ix, pk, ps, pe, cap=total)
        v, _ = ctx.take_fixed(val, ob, want_valid=False)
        v, rows = v.to(torch.int64), op.to(torch.int64)
        cnt = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, rows, torch.ones_like(rows))
        sm = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, rows, v)
        lo = torch.full((n,), I64_MAX, dtype=torch.int64, device=dev).scatter_reduce_(0, rows, v, "amin")
        hi = torch.full((n,), I64_MIN, dtype=torch.int64, device=dev).scatter_reduce_(0, rows, v, "amax")
        return dict(count=cnt, sum=sm, min=lo, max=hi, pairs=total)

    agg = {name: [] for name in SETS}
    floor, old = [], []
    for i in range(reps + 1):
        for name, outs in SETS.items():
            got, ms = timed(lambda: ctx.overlap_agg(ix, pk, ps, pe, val, outputs=outs))
            if i:
                agg[name].append(ms)
            if name == "count+sum+min+max":
                fused = got
            del got
        _, ms = timed(lambda: ctx.overlap_count(ix, pk, ps, pe, per_row=True))
        if i:
            floor.append(ms)
        want, ms = timed(old_way)
        if i:
            old.append(ms)
        same = (bool(torch.equal(fused["count"].to(torch.int64), want["count"])) and bool(torch.equal(fused["sum"], want["sum"])) and
                bool(torch.equal(fused["min"], want["min"])) and bool(torch.equal(fused["max"], want["max"])))
        pairs = want["pairs"]
        del want, fused
        torch.cuda.empty_cache()
    res["agg_ms"] = {name: stat(v) for name, v in agg.items()}
    res["floor_count_per_row_ms"] = stat(floor)
    res["old_way_ms"] = stat(old)
    res["old_way_equals_agg"] = same
    res["pairs"] = pairs
    print(f"probe rows {n}, build rows 1000000, pairs {pairs}, reps {reps}")
    for name in SETS:
        print(f"  agg {name:<18} {fmt(res['agg_ms'][name])}")
    print(f"  floor: count(per_row)  {fmt(res['floor_count_per_row_ms'])}")
    print(f"  old way (4 outputs)    {fmt(res['old_way_ms'])}   equal to agg: {same}")


if __name__ == "__main__":
    main()
