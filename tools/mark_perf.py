"""Build-side match marks on the headline workload (100 M x 1 M rows, 24 contigs, device-resident), three ways to the
same answer timed in the same run, alternating, after a warm-up round:
    mark         ivx_probe_mark_build into a zeroed bitmap
    exists       ivx_probe_exists on the same columns (the probe-side twin: same routing and walk, plus the un-permute)
    count+fill   ivx_probe_overlap_count then ivx_probe_overlap_fill: what a caller needed before to learn the matched
                 build rows (it still has to deduplicate build_idx afterwards; that part is not timed)
Host wall time around a device synchronise per call; median / min / max over REPS rounds, and the device time (hipEvents)
of the last call.  IVX_JOIN_PATH=direct|regions in the environment pins the path; NP / NB scale the sides."""
import os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "datafusion-bio-functions_amd"))
import pyivx, synth
REPS = int(os.environ.get("REPS", 7))
dev = torch.device("cuda:0")
nb, np_ = int(os.environ.get("NB", 1_000_000)), int(os.environ.get("NP", 100_000_000))
bk, bs, be = synth.gen_torch(nb, 1000, 24, 0x5EED0004, dev)
pk, ps, pe = synth.gen_torch(np_, 150, 24, 0x5EED0005, dev)
ctx = pyivx.Ctx(0); ctx.set_stream(torch.cuda.current_stream().cuda_stream)
ix = ctx.build(pyivx.KIND_OVERLAP, bk, bs, be, n_keys=24)
lay = ix.layout()
total = ctx.overlap_count(ix, pk, ps, pe)
ob = torch.empty(total + 16, dtype=torch.int32, device=dev); op = torch.empty_like(ob)
marks = pyivx.Ctx.new_marks(nb, dev)
print(f"build {nb} rows, probe {np_} rows, {total} pairs; layout nreg={lay['nreg']} pk24={lay['pk24']} slow={lay['slow']}; "
      f"IVX_JOIN_PATH={os.environ.get('IVX_JOIN_PATH', '(default)')}", flush=True)

def do_mark():
    marks.zero_()
    ctx.mark_build(ix, pk, ps, pe, marks)

def do_exists():
    ctx.exists(ix, pk, ps, pe)

def do_count_fill():
    assert ctx.overlap_count(ix, pk, ps, pe) == total
    b, _ = ctx.overlap_fill(ix, pk, ps, pe, out=(ob, op)); assert b.numel() == total

calls = (("mark", do_mark), ("exists", do_exists), ("count+fill", do_count_fill))
times = {name: [] for name, _ in calls}
kernel = {}
for rep in range(REPS + 1):                                # round 0 warms every shape up
    for name, fn in calls:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if rep:
            times[name].append(dt * 1e3)
        kernel[name] = ctx.last_kernel_ms()
for name, _ in calls:
    t = times[name]
    print(f"{name:11s} median {statistics.median(t):8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  (n={len(t)})  last call's kernels {kernel[name]:8.3f} ms", flush=True)
# the same answer: the bitmap of the mark call == the build rows the fill call's pairs name
do_mark(); do_count_fill()
from_pairs = pyivx.Ctx.new_marks(nb, dev)
ctx.bits_mark(ob[:total], from_pairs, nb)
ctx.synchronize(); torch.cuda.synchronize()
assert torch.equal(marks, from_pairs), "mark bitmap differs from the pairs' build rows"
print(f"matched build rows {ctx.bits_select(marks, nb, True, count_only=True)} of {nb}: mark bitmap == build rows of the pairs", flush=True)
