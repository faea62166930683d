"""Device-resident timing of the depth region order statistics (ivx_depth_profile_quantiles / _window_quantiles) on the short
read set of tools/depth_regions_timing.py (1 GPU): N reads (default 50 M) of 150 bp on 24 contigs of 100 Mbp, one profile,
and its three region sets.

  targets   (a) R (default 200 000) seeded target regions of 100-400 bp
  contigs   (b) 24 whole-contig regions
  windows   (c) 1000 bp windows over every contig: one call per contig, the 24 times added up
  each with  minmax      bases, min and max only (n_q = 0): the key check, the tile pass, the table and the query kernel
             quartiles   the same plus the median and both quartiles (q_num 1, 2, 3 over 4): the long-region list and the
                         select kernel on top
             summarize   ivx_depth_profile_summarize / _windows with thresholds 1, 10, 20, 30 on the same regions: the
                         yardstick, alternating with the two above in one loop
  split     tiles+table  the minmax call with ONE region: the key check, the whole tile pass, the table, one wavefront
            query        minmax less that
            select       quartiles less minmax: the ranking in registers inside the query kernel, the list and the select kernel
            long         the regions of more than 64 segments (what the select kernel takes), counted on the host from the steps
  baseline  (d) what a caller had before, for the targets: ivx_depth_profile_expand of every target into one concatenated
            Int16 buffer (one call per target), then one sort in torch of (target, coverage) and the ranks picked per
            target.  BREPS repeats (default 2).  Its min, max and three quantiles must equal (a)'s on every target.

Warm-up + REPS repeats, median [min-max].  `device` is the context's event time (kernels only), `wall` a host clock around the
calls and a final synchronise.  Bytes are what the device time amounts to at the 8 TB/s planning peak.

ONLY=targets,contigs,windows restricts the region sets (for a kernel trace of one of them: rocprofv3 --kernel-trace --stats
adds the kernels' times up by name, whatever call they came from).

  N=50000000  R=200000  REPS=5  BREPS=2  ONLY=targets,contigs,windows
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pyivx  # noqa: E402
from depth_timing import PEAK_BPS, dev, short_reads  # noqa: E402

CONTIG = 100_000_000
THR = (1, 10, 20, 30)
QN, QD = (1, 2, 3), 4


def stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def timed(ctx, f):
    """-> (result, device ms of the LAST compute call f made, wall ms of all of f and a synchronise)"""
    ctx.synchronize()
    t0 = time.perf_counter()
    out = f()
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return out, ctx.last_kernel_ms(), wall


def three_ways(ctx, reps, calls):
    """calls: name -> a function that makes the call(s) and returns (result, device ms); alternating, warm-up + reps"""
    dev_ms, wall_ms, last = {k: [] for k in calls}, {k: [] for k in calls}, {}
    for i in range(reps + 1):
        for name, f in calls.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            out, ms = f()
            ctx.synchronize()
            if i:
                dev_ms[name].append(ms); wall_ms[name].append((time.perf_counter() - t0) * 1e3)
            last[name] = out
    return {k: dict(device_ms=stat(dev_ms[k]), wall_ms=stat(wall_ms[k])) for k in calls}, last


def one_call(ctx, f):
    def h():
        out = f()
        ctx.synchronize()
        return out, ctx.last_kernel_ms()
    return h


def main():
    n, nreg = int(float(os.environ.get("N", 50_000_000))), int(float(os.environ.get("R", 200_000)))
    reps, breps = int(os.environ.get("REPS", "5")), int(os.environ.get("BREPS", "2"))
    only = os.environ.get("ONLY", "targets,contigs,windows").split(",")
    ctx = pyivx.Ctx(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lib = pyivx.lib()
    prof = ctx.depth_profile(**short_reads(n, 0x5EED0D01))
    torch.cuda.empty_cache()
    steps = prof.steps()
    res = dict(reads=n, regions=nreg, reps=reps, steps=steps, rank_tile=pyivx.DEPTH_RANK_TILE, rank_segs=pyivx.DEPTH_RANK_SEGS,
               select_grid=pyivx.DEPTH_RANK_SELECT_GRID, q_num=list(QN), q_den=QD, thresholds=list(THR))
    skey, spos, _, _ = prof.read()
    koff = np.searchsorted(skey, np.arange(25))
    del skey

    def segments(qk, qs, qe):
        """steps that reach into each region (+ 1 where the region starts before the key's first step), on the host"""
        out = np.zeros(len(qk), np.int64)
        for k in range(24):
            m = np.flatnonzero(qk == k)
            p = spos[koff[k]:koff[k + 1]]
            a = np.searchsorted(p, qs[m], side="right")
            b = np.searchsorted(p, qe[m], side="right")
            out[m] = np.where(b == 0, 1, b - np.maximum(a, 1) + 1 + (a == 0))
        return out

    g = torch.Generator(device=dev); g.manual_seed(0x7A26E75)
    qkey = torch.randint(0, 24, (nreg,), generator=g, device=dev, dtype=torch.int32)
    qs = torch.randint(0, CONTIG - 400, (nreg,), generator=g, device=dev, dtype=torch.int32)
    qlen = torch.randint(100, 401, (nreg,), generator=g, device=dev, dtype=torch.int64)
    qe = (qs + qlen - 1).to(torch.int32)

    if "targets" in only:
        # ---- (a) targets
        calls = dict(minmax=one_call(ctx, lambda: prof.quantiles(qkey, qs, qe, (), QD)),
                     quartiles=one_call(ctx, lambda: prof.quantiles(qkey, qs, qe, QN, QD)),
                     summarize=one_call(ctx, lambda: prof.summarize(qkey, qs, qe, THR)),
                     one_region=one_call(ctx, lambda: prof.quantiles(qkey[:1], qs[:1], qe[:1], (), QD)))
        t, last = three_ways(ctx, reps, calls)
        seg = segments(qkey.cpu().numpy(), qs.cpu().numpy(), qe.cpu().numpy())
        med = lambda name: t[name]["device_ms"]["median"]
        res["targets"] = dict(t, segments_mean=float(seg.mean()), segments_max=int(seg.max()), long_regions=int((seg > pyivx.DEPTH_RANK_SEGS).sum()),
                              tiles_and_table_ms=med("one_region"), query_ms=med("minmax") - med("one_region"), select_ms=med("quartiles") - med("minmax"),
                              table_bytes_per_step_at_8TBps=med("one_region") / 1e3 * PEAK_BPS / max(steps, 1),
                              bytes_per_region_at_8TBps=med("quartiles") / 1e3 * PEAK_BPS / nreg,
                              extremes_agree=bool(torch.equal(last["minmax"][1], last["quartiles"][1])) and bool(torch.equal(last["minmax"][2], last["quartiles"][2])))
        got = last["quartiles"]

        # ---- (d) the old way for the targets
        if breps:
            off = torch.zeros(nreg + 1, dtype=torch.int64, device=dev)
            torch.cumsum(qlen, 0, out=off[1:])
            total = int(off[-1])
            cov = torch.empty(total, dtype=torch.int16, device=dev)
            hk, hs, hl, ho = qkey.cpu().tolist(), qs.cpu().tolist(), qlen.cpu().tolist(), off.cpu().tolist()
            base = cov.data_ptr()
            expand = lib.ivx_depth_profile_expand
            seg_id = torch.repeat_interleave(torch.arange(nreg, device=dev, dtype=torch.int64), qlen)
            ranks = [off[:-1] + (qlen - 1) * q // QD for q in (0,) + QN + (QD,)]

            def baseline():
                for i in range(nreg):
                    st = expand(ctx.h, prof.h, pyivx.MEM_DEVICE, hk[i], hs[i], hl[i], 0, None, C.c_void_p(base + 2 * ho[i]))
                    if st != pyivx.OK:
                        ctx._chk0(st)
                word = torch.sort((seg_id << 16) | (cov.to(torch.int64) + 32768)).values
                return [((word[r] & 0xFFFF) - 32768).to(torch.int32) for r in ranks]

            d_wall = []
            for i in range(breps + 1):
                want, _, dwall = timed(ctx, baseline)
                if i:
                    d_wall.append(dwall)
            same = (bool(torch.equal(got[1], want[0])) and bool(torch.equal(got[2], want[4])) and
                    all(bool(torch.equal(got[3][j], want[1 + j])) for j in range(len(QN))) and bool(torch.equal(got[0], qlen)))
            res["baseline"] = dict(wall_ms=stat(d_wall), expand_calls=nreg, bases_sorted=total, equals_quantiles=same,
                                   wall_over_quartiles_wall=statistics.median(d_wall) / t["quartiles"]["wall_ms"]["median"])
            del cov, seg_id, want, ranks, off

    if "contigs" in only:
        # ---- (b) whole contigs
        ck = torch.arange(24, dtype=torch.int32, device=dev)
        cs, ce = torch.zeros(24, dtype=torch.int32, device=dev), torch.full((24,), CONTIG + 200, dtype=torch.int32, device=dev)
        calls = dict(minmax=one_call(ctx, lambda: prof.quantiles(ck, cs, ce, (), QD)),
                     quartiles=one_call(ctx, lambda: prof.quantiles(ck, cs, ce, QN, QD)),
                     summarize=one_call(ctx, lambda: prof.summarize(ck, cs, ce, THR)))
        t, last = three_ways(ctx, reps, calls)
        med = lambda name: t[name]["device_ms"]["median"]
        w = last["quartiles"]
        res["contigs"] = dict(t, steps_per_contig=int(steps // 24), select_ms=med("quartiles") - med("minmax"),
                              select_ns_per_step_of_one_contig=(med("quartiles") - med("minmax")) * 1e6 / max(steps // 24, 1),
                              min=int(w[1].min()), max=int(w[2].max()), medians=sorted(set(w[3][1].cpu().tolist())))

    if "windows" in only:
        # ---- (c) 1000 bp windows, a call per contig
        def per_contig(f):
            def h():
                ms, outs = 0.0, None
                for k in range(24):
                    outs = f(k)
                    ctx.synchronize()
                    ms += ctx.last_kernel_ms()
                return outs, ms
            return h
        calls = dict(minmax=per_contig(lambda k: prof.window_quantiles(k, 0, CONTIG - 1, 1000, q_num=(), q_den=QD, device=True)),
                     quartiles=per_contig(lambda k: prof.window_quantiles(k, 0, CONTIG - 1, 1000, q_num=QN, q_den=QD, device=True)),
                     summarize=per_contig(lambda k: prof.windows(k, 0, CONTIG - 1, 1000, thresholds=THR, device=True)))
        t, last = three_ways(ctx, reps, calls)
        med = lambda name: t[name]["device_ms"]["median"]
        nwin = 24 * int(last["quartiles"][0].numel())
        wk = np.full(nwin // 24, 23)
        seg = segments(wk, np.arange(nwin // 24, dtype=np.int64) * 1000, np.arange(nwin // 24, dtype=np.int64) * 1000 + 999)
        res["windows"] = dict(t, width=1000, windows=nwin, segments_mean_last_contig=float(seg.mean()), segments_max_last_contig=int(seg.max()),
                              long_windows_last_contig=int((seg > pyivx.DEPTH_RANK_SEGS).sum()), select_ms=med("quartiles") - med("minmax"),
                              bytes_per_window_at_8TBps=med("quartiles") / 1e3 * PEAK_BPS / max(nwin, 1))
    print(json.dumps(res), flush=True)
    prof.free()
    ctx.close()


if __name__ == "__main__":
    main()
