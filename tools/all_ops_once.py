"""tools/all_ops_once.py: every operator once on small inputs through pyivx, with host and with device memory.

For comparing the HIP call sequence of two builds: run it under `rocprofv3 --hip-trace --kernel-trace --stats -- python
tools/all_ops_once.py` for each and diff the per-API and per-kernel call counts (profiles/scalar_words_*_counts_*.txt are
such tables).  IVX_TREE names the checkout whose package to load (default: this one)."""
import os
import sys

import numpy as np

TREE = os.environ.get("IVX_TREE", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(TREE, "datafusion-bio-functions_amd"))
import pyivx  # noqa: E402
import torch  # noqa: E402

print("tree", TREE, "lib", pyivx.LIB_PATH, flush=True)
rng = np.random.default_rng(3)
ctx = pyivx.Ctx(0)
NK = 5


def dev(a):
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()                # (the context runs on a stream of its own)
    return t


def iv(n, dt, span=2_000_000, maxlen=400, shuffle=True):
    k = rng.integers(0, NK, n).astype(np.uint32)
    s = rng.integers(0, span, n)
    if not shuffle:
        o = np.lexsort((s, k)); k, s = k[o], s[o]
    e = s + rng.integers(1, maxlen, n)
    return k, s.astype(dt), e.astype(dt)


def both(cols):
    return [("host", cols), ("device", [None if c is None else dev(c) for c in cols])]


def env(**kv):
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


b32 = iv(60_000, np.int32)
p32 = iv(90_000, np.int32, maxlen=200)
p32s = iv(90_000, np.int32, maxlen=200, shuffle=False)
chk = []

# ---- overlap index: builds, probes on every path
for mem, b in both(b32):
    ix = ctx.build(pyivx.KIND_OVERLAP, *b, n_keys=NK)
    for pname, pc in (("shuffled", p32), ("sorted", p32s)):
        p = pc if mem == "host" else [dev(c) for c in pc]
        for path, part in (("direct", None), ("regions", None), ("regions", "two")):
            env(IVX_JOIN_PATH=path, IVX_PART=part)
            t = ctx.overlap_count(ix, *p)
            ob, op = ctx.overlap_fill(ix, *p, cap=t)
            env(IVX_NO_PLAN="1")
            ob2, _ = ctx.overlap_fill(ix, *p, cap=t)
            env(IVX_NO_PLAN=None)
            t2, pr = ctx.overlap_count(ix, *p, per_row=True)
            ex = ctx.exists(ix, *p)
            assert len(ob) == t == len(ob2) == t2
            chk.append(("overlap", mem, pname, path, part, t))
        env(IVX_JOIN_PATH=None, IVX_PART=None)
    marks = ctx.new_marks(len(b32[0]), device="cuda" if mem == "device" else None)
    torch.cuda.synchronize()
    ctx.mark_build(ix, *(p32 if mem == "host" else [dev(c) for c in p32]), marks)
    sel = ctx.bits_select(marks, len(b32[0]))
    chk.append(("marks", mem, len(sel)))
    ix.free()
ctx.set_build_overlap(True)
d = [dev(c) for c in b32]
ix = ctx.build(pyivx.KIND_OVERLAP, *d, n_keys=NK)
env(IVX_JOIN_PATH="regions")
dp_ = [dev(c) for c in p32]
t = ctx.overlap_count(ix, *dp_)
ctx.overlap_fill(ix, *dp_, cap=t)
env(IVX_JOIN_PATH=None)
ctx.synchronize(); ix.free()
ctx.set_build_overlap(False)
chk.append(("overlap_tail", t))

# ---- count / coverage / nearest
for mem, b in both(b32):
    p = p32 if mem == "host" else [dev(c) for c in p32]
    for kind, fn in ((pyivx.KIND_COUNT, ctx.count_overlaps), (pyivx.KIND_COVERAGE, ctx.coverage)):
        ix = ctx.build(kind, *b, n_keys=NK)
        for rp in (None, "regions"):
            env(IVX_ROWVAL_PATH=rp)
            for strict in (False, True):
                r = fn(ix, *p, strict=strict)
                chk.append((kind, mem, rp, strict, int(r.sum())))
        env(IVX_ROWVAL_PATH=None)
        ix.free()
    for bb in (b, None):
        if bb is None:
            bs_ = iv(60_000, np.int32, shuffle=False)
            bb = bs_ if mem == "host" else [dev(c) for c in bs_]
        ix = ctx.build(pyivx.KIND_NEAREST, *bb, n_keys=NK)
        for k in (1, 3):
            ob, op, od = ctx.nearest(ix, *p, k=k)
            chk.append(("nearest", mem, k, len(ob)))
        ix.free()

# ---- sweeps
l64 = iv(50_000, np.int64, span=3_000_000)
r64 = iv(40_000, np.int64, span=3_000_000)
s64 = iv(50_000, np.int64, span=3_000_000, shuffle=False)
v64 = iv(300, np.int64, span=3_000_000, maxlen=50_000)
for mem in ("host", "device"):
    cv = (lambda c: c) if mem == "host" else (lambda c: [dev(x) for x in c])
    for cols in (l64, s64):
        c = cv(cols)
        m = ctx.merge(*c, n_keys=NK, min_dist=3)
        cl = ctx.cluster(*c, n_keys=NK, min_dist=3)
        cp = ctx.complement(*c, *cv(v64), n_keys=NK)
        cp2 = ctx.complement(*c, n_keys=NK)
        sb = ctx.subtract(*c, *cv(r64), n_keys=NK)
        chk.append(("sweeps", mem, len(m[0]), cl["n_clusters"], len(cp[0]), len(cp2[0]), len(sb[0])))

# ---- take, marks
src = rng.integers(0, 1 << 30, 10_000).astype(np.int32)
idx = rng.integers(0, 10_000, 5_000).astype(np.uint32)
lens = rng.integers(0, 12, 10_000)
offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
data = rng.integers(65, 90, int(offs[-1])).astype(np.uint8)
sbits = np.packbits(rng.integers(0, 2, 10_000).astype(np.uint8), bitorder="little")
for mem in ("host", "device"):
    cv = (lambda a: a) if mem == "host" else dev
    o, _ = ctx.take_fixed(cv(src), cv(idx))
    ctx.scatter_fixed(cv(src[:5000].copy()), cv(np.arange(5000, dtype=np.uint32)), cv(np.zeros(6000, np.int32)))
    u = ctx.take_utf8(cv(offs), cv(data), cv(idx))
    tb = ctx.take_bits(cv(sbits), 10_000, cv(idx))
    bits = ctx.new_marks(10_000, device="cuda" if mem == "device" else None)
    torch.cuda.synchronize()
    ctx.bits_mark(cv(idx), bits, 10_000)
    n1 = ctx.bits_select(bits, 10_000, count_only=True)
    s0 = ctx.bits_select(bits, 10_000, want_set=False)
    chk.append(("take", mem, int(np.asarray(o.cpu() if mem == "device" else o).astype(np.int64).sum()), n1, len(s0)))

# ---- depth: binary and text CIGARs, segments, profiles
nr = 20_000
rkey = rng.integers(0, NK, nr).astype(np.uint32)
rpos = rng.integers(0, 1_000_000, nr).astype(np.uint32)
rflags = np.zeros(nr, np.uint32); rmapq = np.full(nr, 30, np.uint32)
nops = rng.integers(1, 4, nr)
coff = (np.concatenate([[0], np.cumsum(nops)]) * 4).astype(np.int32)
oplen = rng.integers(1, 80, int(nops.sum())).astype(np.uint32)
opk = rng.choice(np.array([0, 2, 3, 1], np.uint32), int(nops.sum()))
cops = (oplen << np.uint32(4)) | opk
letters = np.array(list("MIDN"))
txt_parts, toff = [], [0]
j = 0
for r in range(nr):
    s = "".join(f"{int(oplen[j + q])}{letters[int(opk[j + q])]}" for q in range(int(nops[r])))
    j += int(nops[r]); txt_parts.append(s); toff.append(toff[-1] + len(s))
text = np.frombuffer("".join(txt_parts).encode(), np.uint8).copy()
toff = np.array(toff, np.int32)
seg = iv(5_000, np.int64, span=1_000_000)
skey, ss, se = seg[0], seg[1].astype(np.uint32), seg[2].astype(np.uint32)
sw = rng.integers(1, 4, len(ss)).astype(np.int32)
klen = np.full(NK, 1_100_000, np.uint32)
qk = rng.integers(0, NK, 500).astype(np.uint32); qs = rng.integers(0, 900_000, 500).astype(np.uint32); qe = qs + 5000
for mem in ("host", "device"):
    cv = (lambda a: a) if mem == "host" else dev
    rd = dict(rkey=cv(rkey), rpos=cv(rpos), rflags=cv(rflags), rmapq=cv(rmapq))
    sg = dict(skey=cv(skey), sstart=cv(ss), send=cv(se), sweight=cv(sw))
    d1 = ctx.depth(**rd, cigar_offsets=cv(coff), cigar_ops=cv(cops), **sg, key_len=cv(klen))
    d2 = ctx.depth(**rd, text_offsets=cv(toff), text=cv(text), key_len=cv(klen))
    po, pops = ctx.cigar_parse(cv(toff), cv(text))
    pa = ctx.depth_profile(**rd, cigar_offsets=cv(coff), cigar_ops=cv(cops), key_len=cv(klen))
    pb = ctx.depth_profile(**sg, key_len=cv(klen))
    pm = pa.merge(pb)
    bl = pm.blocks(device=(mem == "device"))
    xp = pm.expand(1, 1000, 50_000, device=(mem == "device"))
    sm = pm.summarize(cv(qk), cv(qs), cv(qe), thresholds=(1, 5))
    wn = pm.windows(2, 0, 999_999, 10_000, thresholds=(2,), device=(mem == "device"))
    chk.append(("depth", mem, len(d1[0]), len(d2[0]), len(pops), pm.steps(), len(bl[0])))
    pa.free(); pb.free(); pm.free()

ctx.close()
for c in chk:
    print(c)
print("ALL_OPS_DONE", flush=True)
