#!/usr/bin/env python3
# tools/step_trace.py KERNEL_TRACE.csv [first kernel of a step, default k_init_keystats]: the per-step kernel list of a
# rocprofv3 --kernel-trace run of bench.py -- kernel, start, duration, gap to the kernel before it, queue -- as the median over
# the steady steps (those with the most common kernel count), and the step's device span.  Times in us.
import collections, csv, re, statistics, sys
path = sys.argv[1]
first = sys.argv[2] if len(sys.argv) > 2 else "k_init_keystats"
rows = []
for r in csv.DictReader(open(path)):
    name = re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"])
    name = re.sub(r"^void ", "", name)
    depth = 0; cut = len(name)
    for i, ch in enumerate(name):
        if ch == "<": depth += 1
        elif ch == ">": depth -= 1
        elif ch == "(" and depth == 0: cut = i; break
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name[:cut], r["Queue_Id"]))
rows.sort()
steps, cur = [], None
for x in rows:
    if x[2].startswith(first):
        if cur: steps.append(cur)
        cur = []
    if cur is not None and not x[2].startswith("at::"):
        cur.append(x)
if cur: steps.append(cur)
steps = steps[:-1]                                          # (the last one runs into whatever follows the timed steps)
sig = collections.Counter(tuple(k[2] for k in s) for s in steps).most_common(1)[0][0]
use = [s for s in steps if tuple(k[2] for k in s) == sig]
print(f"steps used {len(use)} of {len(steps)}, kernels per step {len(sig)}")
print(f"{'kernel':<58}{'start_us':>10}{'dur_us':>9}{'gap_before_us':>15} queue")
for i, name in enumerate(sig):
    st = statistics.median((s[i][0] - s[0][0]) / 1e3 for s in use)
    du = statistics.median((s[i][1] - s[i][0]) / 1e3 for s in use)
    gap = statistics.median(((s[i][0] - s[i - 1][1]) / 1e3 if i else 0.0) for s in use)
    print(f"{name[:57]:<58}{st:>10.1f}{du:>9.1f}{gap:>15.1f} q{use[0][i][3]}")
span = [(max(k[1] for k in s) - s[0][0]) / 1e3 for s in use]
print(f"step device span us: median {statistics.median(span):.1f} min {min(span):.1f} max {max(span):.1f}")
