// ivx_depth.hip -- depth(): run-length coverage blocks from reads with packed binary CIGARs and from weighted
// intervals (the reference's bio-function-pileup: cigar.rs:1-13, :78-132, :177-230; events.rs:111-137, :181-185;
// coverage.rs:25-65).  The reference walks every read's CIGAR serially and, per partition, either sorts the events or
// adds them into a dense per-contig array; here every pass is a device-wide scan, a radix sort or a compaction, with
// work proportional to the number of CIGAR ops (a 100 000-op long read is spread over ~100 scan tiles):
//
//   k_depth_check   argument checks on the device, before anything is indexed with a value: offsets ascend and are
//                   multiples of 4, key ids are below n_keys or the skip mark
//   ops scan        one segmented scan over the OPS (k_ops_reduce / scan of the tile sums / k_ops_apply).  Element i is
//                   computed from op i and its read -- (first op of its read, reference length it consumes, events it
//                   emits) -- and never stored.  The scanned value gives an M/=/X op its start (read position + 64-bit
//                   sum of the reference lengths before it in its read, cut at 2^32-1: all addends are non-negative, so
//                   this is the serial saturating walk) and the slot of its two events.
//   events          12-byte records: word = key << 32 | position, 32-bit delta (+1 / -1 for reads, +w / -w for
//                   weighted segments: one format for both).  An event beyond key_len[key] becomes (key, 0, delta 0),
//                   which changes no sum.
//   sort            ivx_radix_sort on the position bits that vary (from the largest position written) and the key bits
//   scan 1          per event: the key's running sum c and the sum g of its (key, position) group so far, both with
//                   int32 wrap-around; kept for the last event of every group
//   scan 2          a group with g != 0 is a change point.  A change point with c - g != 0 closes the block its
//                   predecessor opened: (key, position of the latest earlier change point, own position - 1, c - g).
//                   The scan counts the blocks and carries the latest change point; its output pass writes them.
//                   (c - g != 0 implies an earlier change point in the same key: a key's sum starts at 0.)
#include "ivx_device.hpp"
#include "ivx_scan.hpp"
#include "ivx_sort.hpp"

namespace {

constexpr int DT = 256;
constexpr u64 HEADBIT = 1ull << 63;

static inline u32 dgrid(u64 n) { return (u32)((n + DT - 1) / DT); }

__device__ __forceinline__ u32 sat32(u64 x) { return x > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)x; }

__global__ __launch_bounds__(DT) void k_depth_check(const i32 *__restrict__ off, u64 n_reads, const u32 *__restrict__ rkey,
                                                    const u32 *__restrict__ skey, u64 n_seg, u32 nkeys, u64 *sc)
{
    const u64 i = (u64)blockIdx.x * DT + threadIdx.x;
    u32 bad = 0;
    if (off && i <= n_reads) {
        const i32 o = off[i];
        if (o < 0 || (o & 3) || (i > 0 && o < off[i - 1])) bad |= 1u;
        if (i == 0) sc[SC_DEPTH_OFF0] = (u64)(u32)o;
        if (i == n_reads) sc[SC_DEPTH_OFFN] = (u64)(u32)o;
    }
    if (i < n_reads) { const u32 k = rkey ? rkey[i] : 0u; if (k >= nkeys && k != IVX_NULL_IDX) bad |= 2u; }
    if (i < n_seg) { const u32 k = skey ? skey[i] : 0u; if (k >= nkeys && k != IVX_NULL_IDX) bad |= 2u; }
    if (bad) atomicOr((u32 *)(sc + SC_DEPTH_BAD), bad);
}

// ------------------------------------------------------------------------------------------------ the scan over ops
struct DepthReads {
    const u32 *rkey, *rpos, *rflags, *rmapq;
    const i32 *off;
    const u32 *ops;             // the op at byte offset off[0]
    const u32 *key_len;
    u64 n_reads;
    i64 off0;
    u32 filter_flag, min_mapq;
};

// sf: bit 63 = the range holds the first op of a read; low bits = reference length consumed since that op (or, without
// one, by the whole range).  cnt: events emitted.
struct OpState { u64 sf; u32 cnt; u32 pad; };
IVX_SC_FITS(OpState, SC_LANDING, SC_LANDING + SC_LANDING_WORDS);
struct OpScan {
    using T = OpState;
    __host__ __device__ static T identity() { T t; t.sf = 0; t.cnt = 0; t.pad = 0; return t; }
    __device__ static T combine(const T &a, const T &b)
    {
        T r; r.pad = 0;
        r.sf = (b.sf & HEADBIT) ? b.sf : a.sf + b.sf;       // (sums stay below 2^61: at most 2^29 ops of 2^28 each, plus a's head bit)
        r.cnt = a.cnt + b.cnt;
        return r;
    }
    __device__ static T shfl_up(const T &v, int d)
    {
        T r; r.sf = __shfl_up(v.sf, d, IVX_WAVE); r.cnt = __shfl_up(v.cnt, d, IVX_WAVE); r.pad = 0; return r;
    }
};

// the read that holds the op at byte offset b: the last j >= lo with off[j] <= b (reads without ops never hold one)
__device__ __forceinline__ u64 read_of(const DepthReads &R, i64 b, u64 lo)
{
    u64 a = lo, c = R.n_reads;                              // off[a] <= b < off[c]
    while (c - a > 1) { const u64 mid = a + ((c - a) >> 1); if ((i64)R.off[mid] <= b) a = mid; else c = mid; }
    return a;
}

// events.rs:111-137, filter.rs:31-33: does read r contribute at all
__device__ __forceinline__ bool read_kept(const DepthReads &R, u64 r, u32 *key)
{
    const u32 k = R.rkey ? R.rkey[r] : 0u;
    *key = k;
    if (k == IVX_NULL_IDX) return false;
    if (R.rflags && (R.rflags[r] & R.filter_flag) != 0) return false;
    if (R.rmapq && R.rmapq[r] < R.min_mapq) return false;
    return true;
}

// what a thread keeps of one op between computing its element and emitting its events
struct OpAux { u32 len, key, pos; bool emits; };

// the elements of a thread's I_ consecutive ops: ONE search for the read of the first, a step (or a search past a run of
// reads without ops) for the others
__device__ __forceinline__ void ops_load(const DepthReads &R, u64 base, u64 n, OpState (&v)[ivxscan::I_], OpAux (&x)[ivxscan::I_])
{
    u64 r = 0; u32 key = 0, pos = 0; bool kept = false; bool have = false;
#pragma unroll
    for (int i = 0; i < ivxscan::I_; i++) {
        v[i] = OpScan::identity();
        x[i].len = 0; x[i].key = 0; x[i].pos = 0; x[i].emits = false;
        const u64 idx = base + i;
        if (idx >= n) continue;
        const i64 b = R.off0 + 4 * (i64)idx;
        bool moved = !have;
        if (!have) { r = read_of(R, b, 0); have = true; }
        else if (b >= (i64)R.off[r + 1]) { r++; if (b >= (i64)R.off[r + 1]) r = read_of(R, b, r + 1); moved = true; }
        if (moved) { kept = read_kept(R, r, &key); pos = R.rpos[r]; }
        const u32 w = R.ops[idx];
        const u32 len = w >> 4, code = w & 15u;
        const bool consumes = (0x18Du >> code) & 1u;        // M D N = X   (cigar.rs:177-215)
        const bool emits = kept && ((0x181u >> code) & 1u); // M = X
        v[i].sf = (b == (i64)R.off[r] ? HEADBIT : 0ull) | (consumes ? (u64)len : 0ull);
        v[i].cnt = emits ? 2u : 0u;
        x[i].len = len; x[i].key = key; x[i].pos = pos; x[i].emits = emits;
    }
}

__global__ __launch_bounds__(ivxscan::T_) void k_ops_reduce(DepthReads R, u64 n, OpState *__restrict__ sums)
{
    using namespace ivxscan;
    __shared__ OpState lds[T_ / IVX_WAVE + 1];
    const u64 base = (u64)blockIdx.x * TILE_ + (u64)threadIdx.x * I_;
    OpState v[I_]; OpAux x[I_];
    ops_load(R, base, n, v, x);
    OpState s = OpScan::identity();
#pragma unroll
    for (int i = 0; i < I_; i++) s = OpScan::combine(s, v[i]);
    OpState tot;
    block_incl<OpScan>(s, lds, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// offs[tile] = the scan over every earlier tile.  Writes the events of the tile's ops at ev[ev0 + events before the op].
__global__ __launch_bounds__(ivxscan::T_) void k_ops_apply(DepthReads R, u64 n, const OpState *__restrict__ offs,
                                                           u64 *__restrict__ ev, u32 *__restrict__ dl, u64 ev0, u32 *maxpos,
                                                           u8 *seen)
{
    using namespace ivxscan;
    __shared__ OpState lds[T_ / IVX_WAVE + 1];
    __shared__ OpState edge[T_ / IVX_WAVE];
    __shared__ u32 wmax[T_ / IVX_WAVE];
    const u64 base = (u64)blockIdx.x * TILE_ + (u64)threadIdx.x * I_;
    OpState v[I_]; OpAux x[I_];
    ops_load(R, base, n, v, x);
    OpState s = OpScan::identity();
#pragma unroll
    for (int i = 0; i < I_; i++) s = OpScan::combine(s, v[i]);
    OpState tot;
    OpState inc = block_incl<OpScan>(s, lds, &tot);
    OpState run = offs[blockIdx.x];
    OpState prev = OpScan::shfl_up(inc, 1);
    if (lane_id() == IVX_WAVE - 1) edge[threadIdx.x / IVX_WAVE] = inc;
    __syncthreads();
    if (threadIdx.x == 0) prev = OpScan::identity();
    else if (lane_id() == 0) prev = edge[threadIdx.x / IVX_WAVE - 1];
    run = OpScan::combine(run, prev);
    u32 mp = 0;
#pragma unroll
    for (int i = 0; i < I_; i++) {
        if (x[i].emits) {
            // reference length consumed before this op in its read (0 for the read's first op)
            const u64 before = (v[i].sf & HEADBIT) ? 0ull : (run.sf & ~HEADBIT);
            const u64 s64 = (u64)x[i].pos + before;
            u32 ps = sat32(s64), pe = sat32(s64 + x[i].len);
            u32 ds = 1u, de = 0xFFFFFFFFu;
            bool left = true;                                // does one of the two events survive the clipping
            if (R.key_len) {                                 // the dense array has len + 1 slots (events.rs:181-185)
                const u32 kl = R.key_len[x[i].key];
                left = ps <= kl || pe <= kl;
                if (ps > kl) { ps = 0; ds = 0; }
                if (pe > kl) { pe = 0; de = 0; }
            }
            if (seen && left) seen[x[i].key] = 1;            // (every writer stores the same byte)
            const u64 slot = ev0 + run.cnt, kw = (u64)x[i].key << 32;
            ev[slot] = kw | ps; dl[slot] = ds;
            ev[slot + 1] = kw | pe; dl[slot + 1] = de;
            mp = pe > mp ? pe : mp; mp = ps > mp ? ps : mp;
        }
        run = OpScan::combine(run, v[i]);
    }
#pragma unroll
    for (int d = IVX_WAVE / 2; d > 0; d >>= 1) { const u32 o = __shfl_xor(mp, d, IVX_WAVE); mp = o > mp ? o : mp; }
    if (lane_id() == 0) wmax[threadIdx.x / IVX_WAVE] = mp;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j < T_ / IVX_WAVE; j++) mp = wmax[j] > mp ? wmax[j] : mp;
        if (mp) atomicMax(maxpos, mp);
    }
}

// weighted segment j -> events 2j, 2j + 1: (start, +w), (end (+) 1, -w); a skipped segment leaves two events without weight
__global__ __launch_bounds__(DT) void k_seg_events(const u32 *__restrict__ skey, const u32 *__restrict__ ss, const u32 *__restrict__ se,
                                                   const i32 *__restrict__ sw, u64 n_seg, const u32 *__restrict__ key_len,
                                                   u64 *__restrict__ ev, u32 *__restrict__ dl, u32 *maxpos, u8 *seen)
{
    const u64 j = (u64)blockIdx.x * DT + threadIdx.x;
    u32 mp = 0;
    if (j < n_seg) {
        const u32 k = skey ? skey[j] : 0u;
        u64 kw = 0; u32 ps = 0, pe = 0, ds = 0, de = 0;
        if (k != IVX_NULL_IDX) {
            kw = (u64)k << 32;
            ps = ss[j]; pe = sat32((u64)se[j] + 1ull);
            ds = sw ? (u32)sw[j] : 1u; de = 0u - ds;
            bool left = true;
            if (key_len) {
                const u32 kl = key_len[k];
                left = ps <= kl || pe <= kl;
                if (ps > kl) { ps = 0; ds = 0; }
                if (pe > kl) { pe = 0; de = 0; }
            }
            if (seen && left) seen[k] = 1;
        }
        ev[2 * j] = kw | ps; dl[2 * j] = ds;
        ev[2 * j + 1] = kw | pe; dl[2 * j + 1] = de;
        mp = ps > pe ? ps : pe;
    }
#pragma unroll
    for (int d = IVX_WAVE / 2; d > 0; d >>= 1) { const u32 o = __shfl_xor(mp, d, IVX_WAVE); mp = o > mp ? o : mp; }
    if (lane_id() == 0 && mp) atomicMax(maxpos, mp);
}

// ------------------------------------------------------------------------------- sorted events -> coverage blocks
// scan 1: k = sum of the deltas since the key's first event, g = since the (key, position) group's first (int32 wrap-around:
// associative, so the parallel sum is the serial one); f bit 0 / 1 = the range holds a key's / a group's first event
struct EvState { u32 k, g, f; };
struct EvScan {
    using T = EvState;
    __host__ __device__ static T identity() { T t; t.k = 0; t.g = 0; t.f = 0; return t; }
    __device__ static T combine(const T &a, const T &b)
    {
        T r;
        r.k = (b.f & 1u) ? b.k : a.k + b.k;
        r.g = (b.f & 2u) ? b.g : a.g + b.g;
        r.f = a.f | b.f;
        return r;
    }
    __device__ static T shfl_up(const T &v, int d)
    {
        T r; r.k = __shfl_up(v.k, d, IVX_WAVE); r.g = __shfl_up(v.g, d, IVX_WAVE); r.f = __shfl_up(v.f, d, IVX_WAVE); return r;
    }
};
struct EvIn {
    const u64 *ev; const u32 *dl;
    __device__ EvState operator()(u64 i) const
    {
        const u64 w = ev[i];
        const u64 wp = i ? ev[i - 1] : ~w;
        EvState t; t.k = t.g = dl[i];
        t.f = ((w >> 32) != (wp >> 32) ? 1u : 0u) | (w != wp ? 2u : 0u);
        return t;
    }
};
// (c, g) of every group's LAST event: all that scan 2 reads
struct EvOut {
    const u64 *ev; uint2 *cg; u64 n;
    __device__ void operator()(u64 i, const EvState &t) const
    {
        if (i + 1 == n || ev[i + 1] != ev[i]) cg[i] = make_uint2(t.k, t.g);
    }
};

// scan 2: nb = blocks closed so far, cp = (index of the latest change point among the EARLIER events) + 1
struct BlkState { u32 nb, cp; };
struct BlkScan {
    using T = BlkState;
    __host__ __device__ static T identity() { T t; t.nb = 0; t.cp = 0; return t; }
    __device__ static T combine(const T &a, const T &b) { T r; r.nb = a.nb + b.nb; r.cp = a.cp > b.cp ? a.cp : b.cp; return r; }
    __device__ static T shfl_up(const T &v, int d) { T r; r.nb = __shfl_up(v.nb, d, IVX_WAVE); r.cp = __shfl_up(v.cp, d, IVX_WAVE); return r; }
};
struct BlkIn {
    const u64 *ev; const uint2 *cg; u64 n;
    // does event i close a block, and with which coverage
    __device__ __forceinline__ bool closes(u64 i, u64 w, u32 *cov) const
    {
        if (i + 1 != n && ev[i + 1] == w) return false;
        const uint2 t = cg[i];
        *cov = t.x - t.y;
        return t.y != 0 && t.x != t.y;
    }
    __device__ BlkState operator()(u64 i) const
    {
        const u64 w = ev[i];
        BlkState t; t.nb = 0; t.cp = 0;
        if (i && ev[i - 1] != w && cg[i - 1].y != 0) t.cp = (u32)i;
        u32 cov;
        if (closes(i, w, &cov)) t.nb = 1;
        return t;
    }
};
struct BlkOut {
    BlkIn in; u32 *ok, *os, *oe; i32 *oc; u64 cap; u64 *total;
    __device__ void operator()(u64 i, const BlkState &t) const
    {
        const u64 w = in.ev[i];
        u32 cov;
        if (in.closes(i, w, &cov)) {
            const u64 id = (u64)t.nb - 1;
            if (id < cap) {
                if (ok) ok[id] = (u32)(w >> 32);
                if (os) os[id] = t.cp ? (u32)in.ev[t.cp - 1] : 0u;
                if (oe) oe[id] = (u32)w - 1u;
                if (oc) oc[id] = (i32)cov;
            }
        }
        if (i + 1 == in.n) *total = t.nb;
    }
};

}  // namespace

// The front half, up to the end of scan 1: the events sorted by (key, position) and (c, g) at the last event of every group.
// out->n = 0: the input has no event.  seen (nullable, [nkeys], zeroed by the caller): seen[k] = 1 for every key that keeps
// an event after the filter and the clipping.
// Scratch: WS_SCAN0 / WS_SCAN1 (tile sums of the scans), WS_SA0 / WS_SB0 (event words, ping and pong), WS_SA1 / WS_SB1 (their
// deltas), WS_T0 ((c, g) per event), and the sort's WS_SORTHIST.
ivx_status ivx_depth_events(ivx_ctx *ctx, const u32 *rkey, const u32 *rpos, const u32 *rflags, const u32 *rmapq,
                            const i32 *off, const u32 *ops, u64 n_reads,
                            const u32 *skey, const u32 *ss, const u32 *se, const i32 *sw, u64 n_seg,
                            u32 nkeys, const u32 *key_len, u32 filter_flag, u32 min_mapq, u8 *seen, ivx_depth_evs *out)
{
    using namespace ivxscan;
    out->n = 0; out->ev = nullptr; out->cg = nullptr;
    if (n_reads == 0 && n_seg == 0) return IVX_OK;
    hipStream_t st = ctx->stream;
    IVX_HIP(ctx, hipMemsetAsync(ctx->dword(SC_DEPTH_BAD), 0, SC_DEPTH_WORDS * sizeof(u64), st));
    const u64 nchk = (n_reads + 1 > n_seg ? n_reads + 1 : n_seg);
    hipLaunchKernelGGL(k_depth_check, dim3(dgrid(nchk)), dim3(DT), 0, st, n_reads ? off : (const i32 *)nullptr, n_reads, rkey, skey, n_seg, nkeys, ctx->d_scalars);
    IVX_HIP(ctx, hipGetLastError());
    IVX_HIP(ctx, ctx->fetch(SC_DEPTH_BAD, st, SC_DEPTH_WORDS));
    IVX_HIP(ctx, hipStreamSynchronize(st));
    const u32 bad = *ctx->hword<u32>(SC_DEPTH_BAD);
    const u64 off0 = *ctx->hword(SC_DEPTH_OFF0), offn = *ctx->hword(SC_DEPTH_OFFN);
    if (bad & 1u) return ctx->fail(IVX_ERR_INVALID, "depth: cigar_offsets must ascend and be non-negative multiples of 4");
    if (bad & 2u) return ctx->fail(IVX_ERR_INVALID, "depth: key id >= n_keys");
    const u64 n_ops = n_reads ? (offn - off0) / 4 : 0;
    if (n_ops && !ops) return ctx->fail(IVX_ERR_INVALID, "depth: null CIGAR data buffer");

    // ---- the scan over ops, first half: how many events the reads emit
    DepthReads R{rkey, rpos, rflags, rmapq, off, nullptr, key_len, n_reads, 0, filter_flag, min_mapq};
    const u64 nblk = (n_ops + TILE_ - 1) / TILE_;
    OpState *tsum = nullptr;                                // [0] = identity, [1 + t] = the scan up to and including tile t
    u64 n_rev = 0;
    if (n_ops) {
        R.off0 = (i64)off0;
        R.ops = ops + off0 / 4;
        IVX_TRY(ctx->get_scratch(WS_SCAN0, (nblk + 1) * sizeof(OpState), (void **)&tsum));
        IVX_HIP(ctx, hipMemsetAsync(tsum, 0, sizeof(OpState), st));
        hipLaunchKernelGGL(k_ops_reduce, dim3((u32)nblk), dim3(T_), 0, st, R, n_ops, tsum + 1);
        IVX_TRY((scan_rec<OpScan, true>(ctx, tsum + 1, nblk, 1, WS_SCAN0)));
        IVX_HIP(ctx, hipGetLastError());
        OpState tot;
        IVX_TRY(ctx->fetch_wait((const OpState *)tsum + nblk, st, &tot));
        n_rev = tot.cnt;
        // (the 32-bit count cannot wrap: 2^29 ops at most, two events each)
    }
    const u64 E = 2 * n_seg + n_rev;
    if (E >= 0xFFFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "depth: more than 2^32-2 events in one call");
    if (E == 0) return IVX_OK;

    // ---- events
    u64 *wa, *wb; u32 *da, *db;
    IVX_TRY(ctx->get_scratch(WS_SA0, E * sizeof(u64), (void **)&wa));
    IVX_TRY(ctx->get_scratch(WS_SB0, E * sizeof(u64), (void **)&wb));
    IVX_TRY(ctx->get_scratch(WS_SA1, E * sizeof(u32), (void **)&da));
    IVX_TRY(ctx->get_scratch(WS_SB1, E * sizeof(u32), (void **)&db));
    u32 *maxpos = ctx->dword<u32>(SC_DEPTH_MAXPOS);
    if (n_seg) hipLaunchKernelGGL(k_seg_events, dim3(dgrid(n_seg)), dim3(DT), 0, st, skey, ss, se, sw, n_seg, key_len, wa, da, maxpos, seen);
    if (n_rev) hipLaunchKernelGGL(k_ops_apply, dim3((u32)nblk), dim3(T_), 0, st, R, n_ops, (const OpState *)tsum, wa, da, 2 * n_seg, maxpos, seen);
    IVX_HIP(ctx, hipGetLastError());
    u32 hmaxpos;
    IVX_TRY(ctx->fetch_wait(SC_DEPTH_MAXPOS, st, &hmaxpos));

    // ---- sort by (key, position): only the bits that can vary
    int pbits = 0, kbits = 0;
    for (u64 x = hmaxpos; x; x >>= 1) pbits++;
    for (u64 x = nkeys ? nkeys - 1 : 0; x; x >>= 1) kbits++;
    ivx_sort_field f[2]; int nf = 0;
    if (pbits) f[nf++] = ivx_sort_field{0, 0, pbits};
    if (kbits) f[nf++] = ivx_sort_field{0, 32, 32 + kbits};
    u64 *a[1] = {wa}, *b[1] = {wb}; u32 *pay[2] = {da, db};
    int in_b = 0;
    IVX_TRY(ivx_radix_sort(ctx, 1, a, b, E, f, nf, &in_b, true, pay));
    const u64 *ev = in_b ? wb : wa; const u32 *dl = pay[in_b];

    // ---- scan 1
    uint2 *cg;
    IVX_TRY(ctx->get_scratch(WS_T0, E * sizeof(uint2), (void **)&cg));
    IVX_TRY((inclusive_f<EvScan>(ctx, EvIn{ev, dl}, EvOut{ev, cg, E}, E)));
    out->n = E; out->ev = ev; out->cg = cg;
    return IVX_OK;
}

ivx_status ivx_depth_device(ivx_ctx *ctx, const u32 *rkey, const u32 *rpos, const u32 *rflags, const u32 *rmapq,
                            const i32 *off, const u32 *ops, u64 n_reads,
                            const u32 *skey, const u32 *ss, const u32 *se, const i32 *sw, u64 n_seg,
                            u32 nkeys, const u32 *key_len, u32 filter_flag, u32 min_mapq,
                            u32 *ok, u32 *os, u32 *oe, i32 *oc, u64 cap, u64 *n_out)
{
    using namespace ivxscan;
    *n_out = 0;
    ivx_depth_evs evs;
    IVX_TRY(ivx_depth_events(ctx, rkey, rpos, rflags, rmapq, off, ops, n_reads, skey, ss, se, sw, n_seg, nkeys, key_len,
                             filter_flag, min_mapq, nullptr, &evs));
    const u64 E = evs.n;
    if (E == 0) return IVX_OK;
    hipStream_t st = ctx->stream;
    const u64 *ev = evs.ev; const uint2 *cg = evs.cg;

    // ---- scan 2 (its output pass writes the blocks)
    const BlkIn bin{ev, cg, E};
    IVX_TRY((inclusive_f<BlkScan>(ctx, bin, BlkOut{bin, ok, os, oe, oc, cap, ctx->dword(SC_DEPTH_TOTAL)}, E)));
    IVX_HIP(ctx, hipGetLastError());
    IVX_TRY(ctx->fetch_wait(SC_DEPTH_TOTAL, st, n_out));
    if (cap == 0 && !ok && !os && !oe && !oc) return IVX_OK;            // count only
    if (*n_out > cap) return ctx->fail(IVX_ERR_CAPACITY, "depth: output buffers too small");
    return IVX_OK;
}
