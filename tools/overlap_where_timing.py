"""Device-resident timing of the overlap thresholds (include/ivx_where.h) on the headline shape of bench.py (1 GPU): N probe
rows (default 100 M, mean 150 bp) against 1 M build rows (mean 1000 bp) on 24 contigs, unsorted, from synth.py; one int32 value
per build row.  The threshold is probe 1/2: the overlap covers at least half of the probe row.

  check     first, on the first CHECK rows: the filtered calls on the direct kernel and on the region path equal each other,
            and each equals the old way (below) reduced in torch: per-row counts, count + sum, and select's winner and score
  per-row   count (per_row and the total, which the unfiltered entry always makes), agg (count + sum) and select
            (max_overlap, with score): the filtered call against the unfiltered entry, on the direct kernel and on the region
            path (IVX_JOIN_PATH) and with the library's own switch, at the sizes in ROWS
  inner     ivx_probe_overlap_count + ivx_probe_overlap_fill + ONE ivx_pairs_where call into buffers of the fill's size (no
            sizing call) against what a caller had before: count, fill, four ivx_take_fixed of the coordinate columns, the
            comparison and a mask in torch.  At the sizes in OLD and at N.

All variants of one batch size alternate in ONE loop (a warm-up round + REPS rounds), so that drift hits them alike; median
[min-max] of torch events around the calls on the context's stream.  Every line goes to stdout and to OUT (default
profiles/overlap_where_timing.txt).

  N=100000000  REPS=5  CHECK=2000000  ROWS=2097152,8388608,16777216,100000000  OUT=profiles/overlap_where_timing.txt
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
WHERE = pyivx.OverlapWhere(probe=(1, 2))
OLD = (1 << 21, 1 << 23)                                    # batch sizes the inner join is timed at, beside N itself
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


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


class World:
    def __init__(self, n):
        self.ctx = pyivx.Ctx(0)
        self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        self.b = synth.gen_torch(1_000_000, 1000, 24, 0x5EED0004, dev)
        self.p = synth.gen_torch(n, 150, 24, 0x5EED0005, dev)
        g = torch.Generator(device=dev); g.manual_seed(0xA66)
        self.val = torch.randint(-1000, 1000, (1_000_000,), generator=g, device=dev, dtype=torch.int32)
        self.ix = self.ctx.build(pyivx.KIND_OVERLAP, *self.b, n_keys=24)

    def under(self, path, f):
        if path is None:
            return f()
        os.environ["IVX_JOIN_PATH"] = path
        try:
            return f()
        finally:
            os.environ.pop("IVX_JOIN_PATH", None)

    # the three per-row operators, filtered (w) or not
    def count(self, q, w, path=None):
        if w is None:
            return self.under(path, lambda: self.ctx.overlap_count(self.ix, *q, per_row=True)[1])
        # (like for like: ivx_probe_overlap_count(per_row) always reduces and fetches the total as well)
        return self.under(path, lambda: self.ctx.overlap_count_where(self.ix, *q, where=w, exists=False, total=True)["per_row"])

    def agg(self, q, w, path=None):
        return self.under(path, lambda: self.ctx.overlap_agg(self.ix, *q, self.val, outputs=("count", "sum"), where=w))

    def select(self, q, w, path=None):
        return self.under(path, lambda: self.ctx.overlap_select(self.ix, *q, by="max_overlap", where=w))

    def fill(self, q):
        total = self.ctx.overlap_count(self.ix, *q)
        return self.ctx.overlap_fill(self.ix, *q, cap=total)

    def inner_new(self, q):
        """ONE ivx_pairs_where call into buffers of the fill's size (no sizing call in front of it), as the host library does"""
        ob, op = self.fill(q)
        out = (torch.empty_like(ob), torch.empty_like(op))
        return self.ctx.pairs_where(ob, op, self.b[1], self.b[2], q[1], q[2], where=WHERE, out=out)

    def inner_old(self, q):
        """what a caller had before: the pairs, the four coordinates through the pairs, the predicate and a mask in torch"""
        ob, op = self.fill(q)
        take = lambda col, idx: self.ctx.take_fixed(col, idx, want_valid=False)[0].to(torch.int64)
        bs, be, qs, qe = take(self.b[1], ob), take(self.b[2], ob), take(q[1], op), take(q[2], op)
        ln = torch.minimum(qe, be) - torch.maximum(qs, bs) + 1
        keep = (ln >= 1) & (ln * 2 >= (qe - qs + 1))
        return ob[keep], op[keep]


def results_equal(W, check, res):
    q = tuple(c[:check] for c in W.p)
    fb, fp = W.inner_old(q)
    nb = fb.to(torch.int64) & 0xFFFFFFFF
    rows = fp.to(torch.int64) & 0xFFFFFFFF
    # the old way's pairs reduced in torch: per-row count, count + sum of the value, the longest overlap and its smallest row
    want_count = torch.bincount(rows, minlength=check).to(torch.int32)
    want_sum = torch.zeros(check, dtype=torch.int64, device=dev).index_add_(0, rows, W.val.to(torch.int64)[nb])
    # ... and select's winner by the longest overlap, ties to the smallest build row, with its score: one sort of the kept pairs
    # by (probe row, length descending, build row) and the first of each group
    take = lambda col, idx: W.ctx.take_fixed(col, idx, want_valid=False)[0].to(torch.int64)
    ln = torch.minimum(take(q[2], fp), take(W.b[2], fb)) - torch.maximum(take(q[1], fp), take(W.b[1], fb)) + 1
    assert check <= (1 << 21) and int(ln.max()) < (1 << 22) and int(nb.max()) < (1 << 20)
    key, _ = torch.sort((rows << 42) | (((1 << 22) - ln) << 20) | nb)
    first = torch.ones_like(key, dtype=torch.bool)
    first[1:] = (key[1:] >> 42) != (key[:-1] >> 42)
    win = key[first]
    want_idx = torch.full((check,), pyivx.NULL_IDX, dtype=torch.int64, device=dev)
    want_idx[win >> 42] = win & 0xFFFFF
    want_score = torch.zeros(check, dtype=torch.int64, device=dev)
    want_score[win >> 42] = (1 << 22) - ((win >> 20) & 0x3FFFFF)
    same = True
    for path in ("direct", "regions"):
        c = W.count(q, WHERE, path)
        a = W.agg(q, WHERE, path)
        same = same and bool(torch.equal(c, want_count)) and bool(torch.equal(a["count"], want_count)) and bool(torch.equal(a["sum"], want_sum))
        bi, sc = W.select(q, WHERE, path)
        same = same and bool(torch.equal(bi.to(torch.int64) & 0xFFFFFFFF, want_idx)) and bool(torch.equal(sc, want_score))
        if path == "direct":
            ref = (c, a, bi, sc)
        else:
            same = same and bool(torch.equal(bi, ref[2])) and bool(torch.equal(sc, ref[3]))
    ob, op = W.inner_new(q)
    # (both filters are stable, but two fill calls may order their pairs differently: compared as sets)
    key = lambda b, p: torch.sort(((p.to(torch.int64) & 0xFFFFFFFF) << 32) | (b.to(torch.int64) & 0xFFFFFFFF))[0]
    pairs_same = bool(torch.equal(key(ob, op), key(fb, fp)))
    res["filtered_equal_old_way"], res["pairs_equal_old_way"] = same, pairs_same
    res["check_rows"], res["check_pairs_kept"] = check, int(fb.numel())
    say(f"first {check} rows: filtered count / agg / select on both paths == the old way reduced in torch: {same}; "
        f"fill + pairs_where == the old way's pairs: {pairs_same} ({int(fb.numel())} pairs kept)")
    assert same and pairs_same
    torch.cuda.empty_cache()


def by_size(W, n, reps, sizes, res):
    res["sizes"] = []
    say("  ms, median [min-max]; 'auto' = the library's own path switch")
    ops = {"count": W.count, "agg": W.agg, "select": W.select}
    for m in sorted(sizes):
        if m > n:
            continue
        q = tuple(c[:m] for c in W.p)
        runs = {}
        for name, f in ops.items():
            for path in ("direct", "regions", None):
                runs[(name, "plain", path)] = (lambda f=f, path=path: f(q, None, path))
                runs[(name, "where", path)] = (lambda f=f, path=path: f(q, WHERE, path))
        inner = m in OLD or m == n
        if inner:
            runs[("inner", "new")] = lambda: W.inner_new(q)
            runs[("inner", "old")] = lambda: W.inner_old(q)
            runs[("inner", "fill")] = lambda: W.fill(q)
        ms = {k: [] for k in runs}
        kept = None
        for i in range(reps + 1):                           # (the first round warms up: code objects, scratch growth)
            for k, f in runs.items():
                out, t = timed(f)
                if k == ("inner", "new"):
                    kept = int(out[0].numel())
                if k == ("inner", "fill"):
                    pairs = int(out[0].numel())
                del out
                if i:
                    ms[k].append(t)
            torch.cuda.empty_cache()
        row = dict(rows=m)
        say(f"  rows {m}")
        for name in ops:
            row[name] = {}
            for path in ("direct", "regions", None):
                pl, wh = stat(ms[(name, "plain", path)]), stat(ms[(name, "where", path)])
                row[name][path or "auto"] = dict(plain=pl, where=wh, ratio=wh["median"] / pl["median"])
                say(f"    {name:<7} {path or 'auto':<8} unfiltered {fmt(pl)}   probe 1/2 {fmt(wh)}   filtered / unfiltered {wh['median'] / pl['median']:.2f}")
        if inner:
            new, old, fill = stat(ms[("inner", "new")]), stat(ms[("inner", "old")]), stat(ms[("inner", "fill")])
            row["inner"] = dict(new=new, old=old, fill=fill, pairs=pairs, kept=kept)
            say(f"    inner   count + fill {fmt(fill)} ({pairs} pairs)   + pairs_where {fmt(new)} ({kept} kept)   + 4 takes, compare, mask {fmt(old)}   "
                f"old / new {old['median'] / new['median']:.2f}x   filter alone: {new['median'] - fill['median']:.3f} against {old['median'] - fill['median']:.3f} ms")
        res["sizes"].append(row)


def main():
    n, reps = int(float(os.environ.get("N", 100_000_000))), int(os.environ.get("REPS", "5"))
    check = min(n, int(float(os.environ.get("CHECK", 2_000_000))), 1 << 21)
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "overlap_where_timing.txt"))
    sizes = {int(float(x)) for x in os.environ["ROWS"].split(",")} if os.environ.get("ROWS") else {1 << 21, 1 << 23, 1 << 24, n}
    W = World(n)
    res = dict(probe_rows=n, build_rows=1_000_000, reps=reps, where="probe 1/2", layout=W.ix.layout())
    say(f"overlap thresholds, probe 1/2: probe rows {n}, build rows 1000000, reps {reps}")
    results_equal(W, check, res)
    by_size(W, n, reps, sizes, res)
    say(json.dumps(res))
    W.ix.free()
    W.ctx.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
