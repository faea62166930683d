"""Device-resident timing of nearest on one side only / within a distance cap (ivx_probe_nearest_dir, include/ivx_nearest.h)
on the nearest shape of `bench.py --full` (1 GPU): N probe rows (default 50 M, mean 150 bp) against N build rows (mean
1000 bp) on 24 contigs, unsorted, from synth.py with bench.py's seeds.

  check     first: an index over the first CHECK_BUILD build rows, probed with the first CHECK probe rows on both paths, every
            timed variant equal to the cursor restatement A (tests/nearest_dir_oracle.py)
  runs      k = 1, on the routed path and on the direct kernel (IVX_NEAREST_PATH): `before` and `after` without overlaps,
            `after` with overlaps, `any` with D = 1000 -- and ivx_probe_nearest (with and without overlaps) on the same inputs

All runs of one path alternate in ONE loop (a warm-up round + REPS rounds), so that drift hits them alike; median [min-max]
of torch events around the calls on the context's stream.  The expectation to confirm or refute: a one-sided probe without
overlaps costs no more than the two-sided one, because it makes fewer lookups.

  N=50000000  REPS=5  CHECK=200000  CHECK_BUILD=2000000
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyivx  # noqa: E402
import synth  # noqa: E402
import nearest_dir_oracle as ndo  # noqa: E402

dev = torch.device("cuda:0")
# name -> keywords of Ctx.nearest_dir; the first two are ivx_probe_nearest itself (the entry delegates)
RUNS = {
    "nearest any, no overlaps": dict(overlap=False),
    "nearest any, overlaps": dict(overlap=True),
    "before, no overlaps": dict(overlap=False, direction="before"),
    "after, no overlaps": dict(overlap=False, direction="after"),
    "after, overlaps": dict(overlap=True, direction="after"),
    "any, overlaps, D=1000": dict(overlap=True, direction="any", max_distance=1000),
}
BASE = {"before, no overlaps": "nearest any, no overlaps", "after, no overlaps": "nearest any, no overlaps",
        "after, overlaps": "nearest any, overlaps", "any, overlaps, D=1000": "nearest any, overlaps"}


def stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def fmt(s):
    return f"{s['median']:8.3f} [{s['min']:.3f}-{s['max']:.3f}]"


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = f()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def on_path(path, f):
    os.environ["IVX_NEAREST_PATH"] = path
    try:
        return f()
    finally:
        os.environ.pop("IVX_NEAREST_PATH", None)


def check(ctx, b, p, nb, n):
    """every timed variant on a smaller job of the same shape, both paths, against A"""
    hb = [x[:nb].cpu().numpy() for x in b]
    hp = [x[:n].cpu().numpy() for x in p]
    ix = ctx.build(pyivx.KIND_NEAREST, *[x[:nb] for x in b], n_keys=24)
    oix = ndo.NearIndex(*hb)
    q = [x[:n] for x in p]
    for name, kw in RUNS.items():
        wb, _, wd = oix.query(*hp, k=1, **kw)
        for path in ("routed", "direct"):
            gb, _, gd = on_path(path, lambda: ctx.nearest_dir(ix, *q, k=1, **kw))
            gb = gb.cpu().numpy().view(np.uint32); gd = gd.cpu().numpy()
            assert np.array_equal(gb, wb) and np.array_equal(gd, wd), (name, path)
    ix.free()
    print(f"check: {len(RUNS)} variants x 2 paths equal A on the first {n} probe rows x first {nb} build rows", flush=True)


def main():
    n, reps = int(float(os.environ.get("N", 50_000_000))), int(os.environ.get("REPS", "5"))
    ctx = pyivx.Ctx(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    b = synth.gen_torch(n, 1000, 24, 0x5EED0006, dev)
    p = synth.gen_torch(n, 150, 24, 0x5EED0007, dev)
    check(ctx, b, p, min(n, int(float(os.environ.get("CHECK_BUILD", 2_000_000)))), min(n, int(float(os.environ.get("CHECK", 200_000)))))
    ix = ctx.build(pyivx.KIND_NEAREST, *b, n_keys=24)
    res = dict(probe_rows=n, build_rows=n, reps=reps, paths={})
    print(f"probe rows {n}, build rows {n}, reps {reps}; ms, median [min-max]")
    for path in ("routed", "direct"):
        ms = {k: [] for k in RUNS}
        for i in range(reps + 1):                           # (the first round warms up: code objects, scratch growth)
            for name, kw in RUNS.items():
                out, t = timed(lambda: on_path(path, lambda: ctx.nearest_dir(ix, *p, k=1, **kw)))
                del out
                if i:
                    ms[name].append(t)
        row = {k: stat(v) for k, v in ms.items()}
        res["paths"][path] = row
        print(f"  {path}:")
        for name in RUNS:
            s = row[name]
            if name in BASE:
                base = row[BASE[name]]
                # "no more than": not slower beyond the repeats' spread
                print(f"    {name:<26} {fmt(s)}   vs {BASE[name]}: {s['median'] / base['median']:.2f}x, no slower beyond the spread: {s['min'] <= base['max']}")
            else:
                print(f"    {name:<26} {fmt(s)}")
    print(json.dumps(res), flush=True)
    ix.free()
    ctx.close()


if __name__ == "__main__":
    main()
