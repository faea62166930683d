#!/usr/bin/env python3
# tools/kernel_usage.py LOG... : one line per kernel (registers, spills, scratch, LDS, occupancy) from the output of
# hipcc ... -Rpass-analysis=kernel-resource-usage, keyed by the demangled name up to and including its template arguments and
# sorted, so that the tables of two builds can be compared with diff (tools/variant.sh prints such output)
import re, subprocess, sys
rows = {}
cur = None
for path in sys.argv[1:]:
    for line in open(path, errors='replace'):
        m = re.search(r'remark: Function Name: (\S+)', line)
        if m:
            cur = m.group(1); continue
        m = re.search(r'remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Dynamic Stack|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]|TgSplit|NamedBarCnt):\s+(\S+)', line)
        if m and cur:
            rows.setdefault(cur, []).append((m.group(1), m.group(2)))
names = list(rows)
dem = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
seen = {}
for mangled, d in zip(names, dem):
    d = d.replace('(anonymous namespace)::', '')
    # cut the parameter list: the last top-level '(' after the template arguments
    depth = 0; cut = len(d)
    for i, ch in enumerate(d):
        if ch == '<': depth += 1
        elif ch == '>': depth -= 1
        elif ch == '(' and depth == 0: cut = i; break
    key = d[:cut].replace('void ', '')
    if key in seen: print('TWICE', key)
    seen[key] = rows[mangled]
for key in sorted(seen):
    print(key, ' '.join('%s=%s' % (a.split(' ')[0] + ('Spill' if 'Spill' in a else ''), b) for a, b in seen[key]))
