"""Device-resident timing of overlap select (ivx_probe_overlap_select, include/ivx_select.h) on the headline shape of bench.py
(1 GPU): N probe rows (default 100 M, mean 150 bp) against 1 M build rows (mean 1000 bp) on 24 contigs, unsorted, from
synth.py; one int32 value per build row.

  check     first, on the first CHECK rows: both paths equal each other for every variant, and the old way's winner (below)
            equals the fused call's
  select    by = max_val (int32) and max_overlap, with and without the score, on the direct kernel and on the region path
            (IVX_JOIN_PATH), at 2^20 .. 2^26 and N rows
  floor     ivx_probe_overlap_count(per_row) on the same inputs: the same walk with one u32 per row
  old way   what a caller had before: ivx_probe_overlap_count (total), ivx_probe_overlap_fill, ivx_take_fixed of the value
            column by build_idx, then an argmax per probe row in torch: one stable sort of the pairs by (probe row, value
            descending, build row) and the first of each group.  At the sizes in OLD only (it sorts every pair).

All variants of one batch size alternate in ONE loop (a warm-up round + REPS rounds), so that drift hits them alike; median
[min-max] of torch events around the calls on the context's stream.

  N=100000000  REPS=5  CHECK=2000000   ONLY=paths: no check and no old way; ROWS=8388608,100000000: the batch sizes
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
VARIANTS = [("max_val", True), ("max_val", False), ("max_overlap", True), ("max_overlap", False)]
OLD = (1 << 20, 1 << 23)                                    # batch sizes the old way is timed at, beside N itself


def stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def fmt(s):
    return f"{s['median']:8.3f} [{s['min']:.3f}-{s['max']:.3f}]"


def timed(f):
    """-> (result, ms between two events around f on the current stream)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = f()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def main():
    n, reps = int(float(os.environ.get("N", 100_000_000))), int(os.environ.get("REPS", "5"))
    check = min(n, int(float(os.environ.get("CHECK", 2_000_000))))
    ctx = pyivx.Ctx(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    bk, bs, be = synth.gen_torch(1_000_000, 1000, 24, 0x5EED0004, dev)
    pk, ps, pe = synth.gen_torch(n, 150, 24, 0x5EED0005, dev)
    g = torch.Generator(device=dev); g.manual_seed(0xA66)
    val = torch.randint(-1000, 1000, (1_000_000,), generator=g, device=dev, dtype=torch.int32)
    ix = ctx.build(pyivx.KIND_OVERLAP, bk, bs, be, n_keys=24)
    res = dict(probe_rows=n, build_rows=1_000_000, reps=reps, layout=ix.layout())

    def select(q, by, score, path):
        os.environ["IVX_JOIN_PATH"] = path
        try:
            return ctx.overlap_select(ix, *q, by=by, val=val if by == "max_val" else None, score=score)
        finally:
            os.environ.pop("IVX_JOIN_PATH", None)

    def old_way(q):
        """-> (build_idx as int64 with -1 for no match, the winner's value) by max_val"""
        m = int(q[1].numel())
        total = ctx.overlap_count(ix, *q)
        ob, op = ctx.overlap_fill(ix, *q, cap=total)
        v, _ = ctx.take_fixed(val, ob, want_valid=False)
        rows, b, v = op.to(torch.int64), ob.to(torch.int64) & 0xFFFFFFFF, v.to(torch.int64)
        # one key per pair that sorts by (probe row, value descending, build row): 32 + 11 + 20 bits
        key = (rows << 31) | ((1000 - v) << 20) | b
        key, _ = torch.sort(key)
        first = torch.ones_like(key, dtype=torch.bool)
        first[1:] = (key[1:] >> 31) != (key[:-1] >> 31)
        win = key[first]
        idx = torch.full((m,), -1, dtype=torch.int64, device=dev)
        idx[win >> 31] = win & 0xFFFFF
        return idx, total

    only_paths = os.environ.get("ONLY") == "paths"
    sizes = {int(float(x)) for x in os.environ["ROWS"].split(",")} if os.environ.get("ROWS") else {1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24, 1 << 25, 1 << 26, n}
    if not only_paths:
        results_equal(ctx, ix, pk, ps, pe, check, n, reps, select, old_way, res)
    by_size(ctx, ix, pk, ps, pe, n, reps, sizes, only_paths, select, old_way, res)
    print(json.dumps(res), flush=True)
    ix.free()
    ctx.close()


def results_equal(ctx, ix, pk, ps, pe, check, n, reps, select, old_way, res):
    """both paths equal each other for every variant, and the old way's winner equals the fused call's"""
    q = (pk[:check], ps[:check], pe[:check])
    same = True
    for by, score in VARIANTS:
        d, r = select(q, by, score, "direct"), select(q, by, score, "regions")
        same = same and bool(torch.equal(d[0], r[0])) and (not score or bool(torch.equal(d[1], r[1])))
    idx, _ = old_way(q)
    fused = select(q, "max_val", True, "direct")[0].to(torch.int64) & 0xFFFFFFFF
    fused = torch.where(fused == pyivx.NULL_IDX, torch.full_like(fused, -1), fused)
    old_same = bool(torch.equal(idx, fused))
    res["paths_equal"], res["old_way_equals_select"] = same, old_same
    print(f"probe rows {n}, build rows 1000000, reps {reps}; first {check} rows: direct == regions for every variant: {same}; old way == select: {old_same}")
    assert same and old_same
    del idx, fused, d, r
    torch.cuda.empty_cache()


def by_size(ctx, ix, pk, ps, pe, n, reps, sizes, only_paths, select, old_way, res):
    """by batch size, every variant of a size alternating in one loop"""
    res["sizes"] = []
    print("  ms, median [min-max]")
    for m in sorted(sizes):
        if m > n:
            continue
        q = (pk[:m], ps[:m], pe[:m])
        runs = {("floor",): lambda: ctx.overlap_count(ix, *q, per_row=True)}
        for by, score in VARIANTS:
            for path in ("direct", "regions"):
                runs[(by, score, path)] = (lambda by=by, score=score, path=path: select(q, by, score, path))
        if not only_paths and (m in OLD or m == n):
            runs[("old",)] = lambda: old_way(q)
        ms = {k: [] for k in runs}
        pairs = None
        for i in range(reps + 1):                           # (the first round warms up: code objects, scratch growth)
            for k, f in runs.items():
                out, t = timed(f)
                if k == ("old",):
                    pairs = out[1]
                del out
                if i:
                    ms[k].append(t)
            torch.cuda.empty_cache()
        row = dict(rows=m, pairs=pairs, floor=stat(ms[("floor",)]))
        print(f"  rows {m}: floor count(per_row) {fmt(row['floor'])}")
        for by, score in VARIANTS:
            d, r = stat(ms[(by, score, "direct")]), stat(ms[(by, score, "regions")])
            name = f"{by}{'+score' if score else ''}"
            row[name] = dict(direct=d, regions=r)
            # the region path wins when even its slowest repeat beats the direct kernel's fastest
            print(f"    {name:<18} direct {fmt(d)}   regions {fmt(r)}   regions wins beyond the spread: {r['max'] < d['min']}")
        if ("old",) in ms:
            row["old_way"] = stat(ms[("old",)])
            best = min(row["max_val+score"]["direct"]["median"], row["max_val+score"]["regions"]["median"])
            print(f"    old way (max_val)  {fmt(row['old_way'])}   pairs {pairs}   old / select: {row['old_way']['median'] / best:.1f}x")
        res["sizes"].append(row)


if __name__ == "__main__":
    main()
