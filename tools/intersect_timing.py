"""Device-resident timing of ivx_intersect on the subtract shapes of bench.py --full (1 GPU): N left rows (default 200 M)
against N / 10 right rows on 24 contigs, unsorted, int64 half-open, from synth.py -- sparse (mean lengths 20 / 8) and dense
(1000 / 150).

  intersect   Ctx.intersect: sizing call + fill call (the fill call sorts, merges and counts again: no plan is kept)
  subtract    Ctx.subtract on the same inputs in the same loop: sizing call + fill call served by the sizing call's plan
  old way     what a caller had before: merge of the right side, an overlap index on the runs, overlap count + fill,
              take_fixed of four columns (the runs' and the left rows' coordinates) and the clip in torch -- on int32
              coordinates, which the synthetic data fit.  Its pieces come in the join's order.
  passes      the sizing call alone (both sorts, the merge sweep, brackets, count pass, scan) and a fill call into buffers
              of the known size alone (all of that again + the fill pass): the difference is the fill pass
  check       first of all: intersect's pieces and the old way's, both sorted by (left row, start), are equal (asserted);
              the numbers of pieces and of subtract's fragments are printed

Warm-up + REPS repeats, median [min-max] of torch events around the calls on the context's stream (kernels, the gaps
between them and the host round trips of the counts).

  N=200000000  REPS=5  SHAPES=sparse,dense
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
SHAPES = {"sparse": (20, 8, 0x5EED000A), "dense": (1000, 150, 0x5EED0008)}      # left mean, right mean, left seed (bench.py)


def stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def fmt(s):
    return f"{s['median']:9.3f} [{s['min']:.3f}-{s['max']:.3f}] ms"


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = f()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def by_row_start(row, start, end):
    """the pieces ordered by (left row, start): a left row's pieces are disjoint, so the order is total"""
    o = torch.argsort(start, stable=True)
    o = o[torch.argsort(row[o].to(torch.int64), stable=True)]
    return row[o], start[o], end[o]


def main():
    n, reps = int(float(os.environ.get("N", 200_000_000))), int(os.environ.get("REPS", "5"))
    nr = n // 10
    ctx = pyivx.Ctx(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    res = dict(left_rows=n, right_rows=nr, reps=reps, shapes={})
    for tag in os.environ.get("SHAPES", "sparse,dense").split(","):
        mean_l, mean_r, seed = SHAPES[tag]
        lk, ls32, le32 = synth.gen_torch(n, mean_l, 24, seed, dev)
        rk, rs32, re32 = synth.gen_torch(nr, mean_r, 24, 0x5EED0009, dev)
        le32, re32 = le32 + 1, re32 + 1                                 # half-open, as bench.py's half_open64
        ls, le, rs, re = (x.to(torch.int64) for x in (ls32, le32, rs32, re32))

        def old_way():
            mk, ms, me, _ = ctx.merge(rk, rs, re, n_keys=24)
            ms32, me32 = ms.to(torch.int32), me.to(torch.int32)
            ix = ctx.build(pyivx.KIND_OVERLAP, mk, ms32, me32, n_keys=24)
            total = ctx.overlap_count(ix, lk, ls32, le32)
            ob, op = ctx.overlap_fill(ix, lk, ls32, le32, cap=total)
            a, _ = ctx.take_fixed(ms32, ob, want_valid=False)
            b, _ = ctx.take_fixed(me32, ob, want_valid=False)
            c, _ = ctx.take_fixed(ls32, op, want_valid=False)
            d, _ = ctx.take_fixed(le32, op, want_valid=False)
            out = op, torch.maximum(a, c), torch.minimum(b, d)
            ctx.synchronize()
            ix.free()
            return out

        # ---- equal first
        k, s, e, row = ctx.intersect(lk, ls, le, rk, rs, re, n_keys=24)
        pieces = int(row.numel())
        got = by_row_start(row, s, e)
        del k, s, e, row
        orow, os_, oe = old_way()
        want = by_row_start(orow, os_.to(torch.int64), oe.to(torch.int64))
        del orow, os_, oe
        assert all(g.shape == w.shape and bool(torch.equal(g, w)) for g, w in zip(got, want)), "intersect differs from the old way"
        del got, want
        frags = int(ctx.subtract(lk, ls, le, rk, rs, re, n_keys=24)[0].numel())
        torch.cuda.empty_cache()

        # ---- the three ways, alternating; then the two calls of intersect on their own
        t = {name: [] for name in ("intersect", "subtract", "old_way", "sizing_call", "fill_call")}
        for i in range(reps + 1):                                       # (the first round warms up: code objects, scratch growth)
            for name, f in (("intersect", lambda: ctx.intersect(lk, ls, le, rk, rs, re, n_keys=24)),
                            ("subtract", lambda: ctx.subtract(lk, ls, le, rk, rs, re, n_keys=24)),
                            ("old_way", old_way),
                            ("sizing_call", lambda: ctx.intersect_count(lk, ls, le, rk, rs, re, n_keys=24)),
                            ("fill_call", lambda: ctx.intersect(lk, ls, le, rk, rs, re, n_keys=24, cap=pieces))):
                out, ms = timed(f)
                del out
                if i:
                    t[name].append(ms)
            # (the caching allocator keeps the output buffers across the rounds of a shape: it is emptied between shapes only)
        r = {name: stat(v) for name, v in t.items()}
        r.update(pieces=pieces, subtract_fragments=frags, equal_to_old_way=True,
                 fill_pass_ms=r["fill_call"]["median"] - r["sizing_call"]["median"], form=ctx.sweep_form())
        res["shapes"][tag] = r
        print(f"{tag}: {n} left rows (mean {mean_l}) x {nr} right rows (mean {mean_r}); {pieces} pieces, {frags} subtract fragments; equal to the old way")
        print(f"  intersect  sizing + fill   {fmt(r['intersect'])}")
        print(f"  subtract   sizing + fill   {fmt(r['subtract'])}")
        print(f"  old way                    {fmt(r['old_way'])}")
        print(f"  intersect  sizing call     {fmt(r['sizing_call'])}   (sorts, merge sweep, brackets, count pass, scan)")
        print(f"  intersect  fill call       {fmt(r['fill_call'])}   (all of that + the fill pass: {r['fill_pass_ms']:.3f} ms)")
        del lk, ls32, le32, rk, rs32, re32, ls, le, rs, re
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
