// ivx_depth_classes.hip -- depth coverage classes: every base of a depth profile classified by its coverage.  Quantize gives
// the maximal intervals whose coverage stays in one class (mosdepth --quantize, GATK CallableLoci, "the intervals at 10x or
// more"); hist gives, per key, the number of bases at each coverage value (bedtools genomecov, mosdepth's dist, the
// histogram of Picard CollectWgsMetrics).  include/ivx.h ivx_depth_profile_quantize / _hist; v(p), c0(k), the domain D(k),
// the zero stretch and the key's last step are those of the region summaries (ivx_depth_regions.hip).
//
//   segments  step i of key k covers [max(pos[i], pos_lo), min(pos[i + 1] - 1, hi(k))], a key's last step up to hi(k).  The
//             steps that cover nothing lie wholly below pos_lo or wholly above hi(k): a prefix and a suffix of the key's
//             steps, so the live ones are consecutive and a live step's neighbour in its run is the step next to it.  Ahead
//             of them sits the zero stretch [pos_lo, first pos - 1] (the whole domain of a key without steps), value 0.
//   quantize  a live step is a HEAD when no live segment of its key precedes it or that one has another class, a TAIL
//             likewise towards its successor; both tests read only the two neighbouring steps.  A segmented counting scan
//             over the steps (ivx_scan.hpp; the flag of a key's first step in bit 63) numbers the emitted heads inside their
//             key, the key's first step carrying the zero stretch's row along.  Count pass: a key's last step stores the
//             key's rows (the scan's last kernel runs in the tiles that hold such a step alone); a per-key kernel supplies
//             the keys without steps; one exclusive scan over the keys gives every key's first row and the total, which is
//             read back.  Write pass: the same scan again, every tile this time; a head stores key, start
//             and class at row = first row of the key + its number - 1, and a tail stores the end at the row its own scan
//             value gives: inside a run there is no other head, so it is the head's row.  No head looks forward.  The zero
//             stretch's row is the key's first; the per-key kernel writes it.
//   hist      one pass over the steps.  A workgroup takes a run of consecutive tiles and keeps the bins of ONE key in LDS
//             (n_bins <= DEPTH_HIST_LDS_BINS); they go to memory, one 64-bit atomic per bin that is not zero, when the key
//             changes and at the end of the run.  A tile whose steps span DEPTH_HIST_TILE_KEYS key ids or more, or a call
//             with more bins, adds to memory directly.  Before any add a wavefront combines its 256 steps: a round takes
//             the first pending (key, bin), every lane sums its matching lengths, one reduction, one add.  Real coverage
//             puts most steps into a few dozen bins: a few dozen rounds instead of 256 adds to the same few words.
//             Integer sums: any order gives the same bits.
#include "ivx_depth_regions.hpp"
#include "ivx_scan.hpp"

namespace {

constexpr int CT = 256;                         // threads of every kernel here (the scan's workgroup)
constexpr int DEPTH_CLASS_TILE = ivxscan::TILE_;        // steps per tile of both passes
constexpr int HS = DEPTH_CLASS_TILE / CT;       // steps per thread of the histogram pass
constexpr u32 DEPTH_HIST_LDS_BINS = 2048;       // 16 KiB of 64-bit bins: eight workgroups a CU stay inside 160 KiB
constexpr u32 DEPTH_HIST_TILE_KEYS = 8;         // a tile spanning this many key ids or more adds to memory directly
constexpr u32 HIST_MAX_WG = 2048;               // workgroups of the histogram pass: 256 CUs x 8
constexpr int MAXC = 31;
static_assert(CT == ivxscan::T_ && DEPTH_CLASS_TILE % CT == 0 && MAXC == IVX_DEPTH_MAX_CUTS, "the scan's workgroup; the header's limit");

using ull = unsigned long long;
constexpr ull SEG = 1ull << 63;                 // scan element: the step is its key's first

struct Dom { const u32 *key_hi; u32 pos_lo; int skip_pos0, seen_only; };
struct Cuts { i32 c[MAXC]; u32 n, emit; };

// hi(k), and whether key k takes part
__device__ __forceinline__ bool key_domain(const DepthProfileView &dp, const Dom &d, u32 k, u32 &dh)
{
    dh = d.key_hi ? d.key_hi[k] : 0xFFFFFFFFu;
    return dh >= d.pos_lo && !(d.seen_only && !dp.seen[k]);
}

// the segment of step i: false if it covers nothing.  follows: the key's next step is live too
__device__ __forceinline__ bool step_segment(const DepthProfileView &dp, const Dom &d, u64 i, u32 &k, u32 &lo, u32 &hi, u32 &c0, bool &follows)
{
    k = dp.key[i];
    follows = false;
    u32 dh;
    if (!key_domain(dp, d, k, dh)) return false;
    const u32 p = dp.pos[i];
    lo = p > d.pos_lo ? p : d.pos_lo;
    hi = dh;
    if (i + 1 < dp.steps && dp.key[i + 1] == k) {
        const u32 q = dp.pos[i + 1] - 1u;
        if (q < dh) { hi = q; follows = true; }
    }
    c0 = d.skip_pos0 ? key_c0(dp, dp.koff[k], 1) : 0u;
    return lo <= hi;
}

// the zero stretch of key k: false if it is empty.  follows: the key's first step is live
__device__ __forceinline__ bool zero_stretch(const DepthProfileView &dp, const Dom &d, u32 k, u32 &hi, bool &follows)
{
    follows = false;
    u32 dh;
    if (!key_domain(dp, d, k, dh)) return false;
    hi = dh;
    const u32 f = dp.koff[k];
    if (f != dp.koff[k + 1]) {
        const u32 fp = dp.pos[f];
        if (fp <= d.pos_lo) return false;
        if (fp - 1u < dh) { hi = fp - 1u; follows = true; }
    }
    return true;
}

// ------------------------------------------------------------------------------------------------ quantize
__device__ __forceinline__ u32 class_of(const Cuts &c, i32 v)
{
    u32 r = 0;
    for (u32 e = 0; e < c.n; e++) r += v >= c.c[e] ? 1u : 0u;
    return r;
}
__device__ __forceinline__ bool emitted(const Cuts &c, u32 cls) { return (c.emit >> cls) & 1u; }

struct QStep { u32 k, lo, hi, cls; bool first, live, head, tail; };

__device__ __forceinline__ QStep q_step(const DepthProfileView &dp, const Dom &d, const Cuts &c, u64 i)
{
    QStep s;
    u32 c0; bool follows;
    s.live = step_segment(dp, d, i, s.k, s.lo, s.hi, c0, follows);
    s.first = i == 0 || dp.key[i - 1] != s.k;
    s.head = s.tail = false; s.cls = 0;
    if (!s.live) return s;
    const i32 v = (i32)((u32)dp.cov[i] - c0);
    const i32 vp = s.first ? 0 : (i32)((u32)dp.cov[i - 1] - c0);            // (the zero stretch ahead of a first step)
    const i32 vn = follows ? (i32)((u32)dp.cov[i + 1] - c0) : 0;
    u32 cl = 0, cp = 0, cn = 0;
    for (u32 e = 0; e < c.n; e++) {
        const i32 t = c.c[e];
        cl += v >= t ? 1u : 0u; cp += vp >= t ? 1u : 0u; cn += vn >= t ? 1u : 0u;
    }
    s.cls = cl;
    s.head = dp.pos[i] <= d.pos_lo || cp != cl;             // at or below pos_lo: nothing live precedes it
    s.tail = !follows || cn != cl;
    return s;
}

struct SegScan {
    using T = ull;
    __host__ __device__ static T identity() { return 0ull; }
    __device__ static T combine(const T &a, const T &b) { return (b & SEG) ? b : a + b; }
    __device__ static T shfl_up(const T &v, int d) { return __shfl_up(v, d, IVX_WAVE); }
};

// element i: the emitted heads of step i (0 or 1), a key's first step with the key's flag and the zero stretch's row
struct QIn {
    DepthProfileView dp; Dom d; Cuts c;
    __device__ ull operator()(u64 i) const
    {
        const QStep s = q_step(dp, d, c, i);
        ull r = 0;
        if (s.first) {
            r = SEG;
            u32 dh;
            if (key_domain(dp, d, s.k, dh) && dp.pos[i] > d.pos_lo && emitted(c, class_of(c, 0))) r |= 1ull;
        }
        if (s.head && emitted(c, s.cls)) r += 1ull;
        return r;
    }
};
// the count pass: a key's last step stores the key's rows
struct QCount {
    const u32 *key; u64 n; ull *krows;
    __device__ void operator()(u64 i, const ull &t) const
    {
        const u32 k = key[i];
        if (i + 1 == n || key[i + 1] != k) krows[k] = t & ~SEG;
    }
};
// the write pass: heads and tails of emitted runs, each at the row its own scan value gives
struct QWrite {
    QIn in; const ull *first_row; u32 *ok, *os, *oe, *oc;
    __device__ void operator()(u64 i, const ull &t) const
    {
        const QStep s = q_step(in.dp, in.d, in.c, i);
        if (!s.live || !emitted(in.c, s.cls) || !(s.head || s.tail)) return;
        const u64 row = first_row[s.k] + (t & ~SEG) - 1ull;
        if (s.head) {
            if (ok) ok[row] = s.k;
            if (os) os[row] = s.lo;
            if (oc) oc[row] = s.cls;
        }
        if (s.tail && oe) oe[row] = s.hi;
    }
};

// The count pass's last kernel: k_apply_f of ivx_scan.hpp with QCount, run by the tiles that hold a key's last step alone.  Only
// those steps store anything, and a genome's step list has a couple of dozen of them in a hundred thousand tiles.
__global__ __launch_bounds__(CT) void k_quantize_count(QIn in, QCount out, u64 n, const ull *__restrict__ offs)
{
    using namespace ivxscan;
    using Op = SegScan;
    const u64 t0 = (u64)blockIdx.x * TILE_, past = t0 + TILE_ < n ? t0 + TILE_ : n;
    if (past < n && in.dp.key[t0] == in.dp.key[past]) return;       // no key ends inside the tile (the same for the whole workgroup)
    __shared__ ull lds[T_ / IVX_WAVE + 1];
    __shared__ ull edge[T_ / IVX_WAVE];
    const u64 base = t0 + (u64)threadIdx.x * I_;
    ull v[I_];
    ull s = Op::identity();
#pragma unroll
    for (int i = 0; i < I_; i++) { v[i] = base + i < n ? in(base + i) : Op::identity(); s = Op::combine(s, v[i]); }
    ull tot;
    ull inc = block_incl<Op>(s, lds, &tot);
    ull run = offs ? offs[blockIdx.x] : Op::identity();
    ull prev = Op::shfl_up(inc, 1);
    if (lane_id() == IVX_WAVE - 1) edge[threadIdx.x / IVX_WAVE] = inc;
    __syncthreads();
    if (threadIdx.x == 0) prev = Op::identity();
    else if (lane_id() == 0) prev = edge[threadIdx.x / IVX_WAVE - 1];
    run = Op::combine(run, prev);
#pragma unroll
    for (int i = 0; i < I_; i++) { run = Op::combine(run, v[i]); if (base + i < n) out(base + i, run); }
}

// the count pass: inclusive_f of ivx_scan.hpp with k_quantize_count as its last kernel.  Scratch: WS_SCAN*
ivx_status quantize_count(ivx_ctx *ctx, const QIn &in, const QCount &out, u64 n)
{
    using namespace ivxscan;
    if (n == 0) return IVX_OK;
    const u64 nblk = (n + TILE_ - 1) / TILE_;
    ull *sums;
    IVX_TRY(ctx->get_scratch(WS_SCAN0, nblk * sizeof(ull), (void **)&sums));
    if (nblk > 1) {
        hipLaunchKernelGGL((k_reduce_f<SegScan, QIn>), dim3((u32)nblk), dim3(T_), 0, ctx->stream, in, n, sums);
        IVX_TRY((scan_rec<SegScan, false>(ctx, sums, nblk, 1, WS_SCAN0)));
    }
    hipLaunchKernelGGL(k_quantize_count, dim3((u32)nblk), dim3(T_), 0, ctx->stream, in, out, n, nblk > 1 ? (const ull *)sums : (const ull *)nullptr);
    return IVX_OK;
}

// WRITE = false: rows[k] = the rows of key k (krows for a key with steps, the zero stretch's for one without), rows[nkeys] = 0:
// the slot the scan turns into the total.  WRITE = true: rows holds the scanned counts; the zero stretch's run goes out.
template <bool WRITE>
__global__ __launch_bounds__(CT) void k_quantize_keys(DepthProfileView dp, Dom d, Cuts c, u32 nkeys, const ull *__restrict__ krows, ull *__restrict__ rows,
                                                      u32 *__restrict__ ok, u32 *__restrict__ os, u32 *__restrict__ oe, u32 *__restrict__ oc)
{
    const u64 k64 = (u64)blockIdx.x * CT + threadIdx.x;
    if (k64 > nkeys) return;
    const u32 k = (u32)k64;
    if (k == nkeys) { if (!WRITE) rows[k] = 0ull; return; }
    u32 hi; bool follows;
    const u32 cls0 = class_of(c, 0);
    const bool zero = zero_stretch(dp, d, k, hi, follows) && emitted(c, cls0);
    const u32 f = dp.koff[k];
    if (!WRITE) { rows[k] = f != dp.koff[k + 1] ? krows[k] : (zero ? 1ull : 0ull); return; }
    if (!zero) return;
    const u64 row = rows[k];
    if (ok) ok[row] = k;
    if (os) os[row] = d.pos_lo;
    if (oc) oc[row] = cls0;
    // (c0 = 0 here: the zero stretch is not empty, so the key has no step at position 0)
    if (oe && (!follows || class_of(c, dp.cov[f]) != cls0)) oe[row] = hi;
}

// ------------------------------------------------------------------------------------------------ hist
__device__ __forceinline__ u32 bin_of(i32 v, i32 v_lo, u32 n_bins)
{
    const i64 b = (i64)v - v_lo;
    return b < 0 ? 0u : b > (i64)(n_bins - 1u) ? n_bins - 1u : (u32)b;
}

// the zero stretches and the keys without steps, after the memset and ahead of the step pass: one writer per word
__global__ __launch_bounds__(CT) void k_hist_keys(DepthProfileView dp, Dom d, i32 v_lo, u32 n_bins, u32 nkeys, ull *__restrict__ out)
{
    const u64 k = (u64)blockIdx.x * CT + threadIdx.x;
    if (k >= nkeys) return;
    u32 hi; bool follows;
    if (zero_stretch(dp, d, (u32)k, hi, follows)) out[k * n_bins + bin_of(0, v_lo, n_bins)] = (ull)hi - d.pos_lo + 1ull;
}

// One wavefront's pending adds (len != 0), combined: a round takes the first pending index, the lanes sum their matching
// lengths and one lane adds the wavefront's sum.  Every lane of the wavefront is here.
template <class Add>
__device__ __forceinline__ void wave_combine(const u64 (&idx)[HS], u64 (&len)[HS], u32 l, Add add)
{
    for (;;) {
        u64 mine = ~0ull;
#pragma unroll
        for (int j = HS - 1; j >= 0; j--)
            if (len[j]) mine = idx[j];
        const u64 pending = __ballot(mine != ~0ull);
        if (!pending) break;
        const int lead = __ffsll((long long)pending) - 1;
        const u64 cand = ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(mine >> 32), lead) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)mine, lead);
        u64 s = 0;
#pragma unroll
        for (int j = 0; j < HS; j++)
            if (len[j] && idx[j] == cand) { s += len[j]; len[j] = 0; }
        s = (u64)wave_sum((ull)s);
        if (l == 0) add(cand, s);
    }
}

__global__ __launch_bounds__(CT) void k_hist_steps(DepthProfileView dp, Dom d, i32 v_lo, u32 n_bins, u32 ntiles, u32 tiles_per_wg, ull *__restrict__ out)
{
    constexpr u32 T = DEPTH_CLASS_TILE;
    __shared__ ull bins[DEPTH_HIST_LDS_BINS];
    const u32 t = threadIdx.x, l = lane_id();
    const bool lds_ok = n_bins <= DEPTH_HIST_LDS_BINS;
    const u32 t0 = blockIdx.x * tiles_per_wg, t1 = t0 + tiles_per_wg < ntiles ? t0 + tiles_per_wg : ntiles;
    if (lds_ok)
        for (u32 b = t; b < n_bins; b += CT) bins[b] = 0ull;
    __syncthreads();
    u32 cur = IVX_NULL_IDX;                                 // the key whose bins are in LDS (the same for the whole workgroup)
    // the bins in LDS to memory, and zero again
    auto flush = [&]() {
        __syncthreads();
        for (u32 b = t; b < n_bins; b += CT) {
            const ull v = bins[b];
            if (v) { atomicAdd(out + (u64)cur * n_bins + b, v); bins[b] = 0ull; }
        }
        __syncthreads();
    };
    for (u32 tile = t0; tile < t1; tile++) {
        const u64 base = (u64)tile * T;
        const u64 last = base + T < dp.steps ? base + T - 1u : dp.steps - 1u;
        const u32 kf = dp.key[base], kl = dp.key[last];
        u32 sk[HS], sb[HS]; u64 sl[HS];
#pragma unroll
        for (int j = 0; j < HS; j++) {
            const u64 i = base + t + (u64)CT * j;
            sk[j] = 0; sb[j] = 0; sl[j] = 0;
            u32 lo, hi, c0; bool follows;
            if (i <= last && step_segment(dp, d, i, sk[j], lo, hi, c0, follows)) {
                sl[j] = (u64)hi - lo + 1u;
                sb[j] = bin_of((i32)((u32)dp.cov[i] - c0), v_lo, n_bins);
            }
        }
        u64 idx[HS], len[HS];
        if (!lds_ok || kl - kf >= DEPTH_HIST_TILE_KEYS) {
#pragma unroll
            for (int j = 0; j < HS; j++) { idx[j] = (u64)sk[j] * n_bins + sb[j]; len[j] = sl[j]; }
            wave_combine(idx, len, l, [&](u64 at, u64 s) { atomicAdd(out + at, (ull)s); });
            continue;
        }
        for (u32 k = kf;; k++) {                            // (fewer than DEPTH_HIST_TILE_KEYS rounds)
            if (k != cur) {
                if (cur != IVX_NULL_IDX) flush();
                cur = k;
            }
#pragma unroll
            for (int j = 0; j < HS; j++) { idx[j] = sb[j]; len[j] = sk[j] == k ? sl[j] : 0; }
            wave_combine(idx, len, l, [&](u64 at, u64 s) { atomicAdd(&bins[at], (ull)s); });
            if (k == kl) break;
        }
    }
    if (cur != IVX_NULL_IDX) flush();
}

Dom make_dom(u32 pos_lo, const u32 *key_hi, int skip_pos0, int seen_only) { return Dom{key_hi, pos_lo, skip_pos0 ? 1 : 0, seen_only ? 1 : 0}; }

}  // namespace

// cuts: host memory, strictly ascending, n_cuts <= 31, emit_mask < 2^(n_cuts + 1): the caller's checks; every other pointer
// on the device.  Scratch: WS_T0 (rows of the keys with steps), WS_T1 (rows per key, scanned), WS_SCAN* (both scans).  The
// count is always made and read back; the write pass runs only when the buffers hold it.
ivx_status ivx_depth_quantize_device(ivx_ctx *ctx, const DepthProfileView &dp, u32 nkeys, u32 pos_lo, const u32 *key_hi, int skip_pos0, int seen_only,
                                     const i32 *cuts, u32 n_cuts, u32 emit_mask, u32 *ok, u32 *os, u32 *oe, u32 *oc, u64 cap, u64 *n_out)
{
    using namespace ivxscan;
    *n_out = 0;
    if (nkeys == 0) return IVX_OK;
    hipStream_t st = ctx->stream;
    QIn in{dp, make_dom(pos_lo, key_hi, skip_pos0, seen_only), Cuts{}};
    in.c.n = n_cuts; in.c.emit = emit_mask;
    for (u32 e = 0; e < n_cuts; e++) in.c.c[e] = cuts[e];
    ull *krows, *rows;
    IVX_TRY(ctx->get_scratch(WS_T0, (size_t)nkeys * sizeof(ull), (void **)&krows));
    IVX_TRY(ctx->get_scratch(WS_T1, ((size_t)nkeys + 1) * sizeof(ull), (void **)&rows));
    const dim3 kgrid((u32)(((u64)nkeys + 1 + CT - 1) / CT));
    IVX_TRY(quantize_count(ctx, in, QCount{dp.key, dp.steps, krows}, dp.steps));
    hipLaunchKernelGGL((k_quantize_keys<false>), kgrid, dim3(CT), 0, st, dp, in.d, in.c, nkeys, (const ull *)krows, rows,
                       (u32 *)nullptr, (u32 *)nullptr, (u32 *)nullptr, (u32 *)nullptr);
    IVX_HIP(ctx, hipGetLastError());
    IVX_TRY(ivx_scan_exclusive_u64(ctx, (u64 *)rows, (u64)nkeys + 1));
    IVX_HIP(ctx, hipGetLastError());
    IVX_TRY(ctx->fetch_wait((const u64 *)rows + nkeys, st, n_out));
    if (cap == 0 && !ok && !os && !oe && !oc) return IVX_OK;            // count only
    if (*n_out > cap) return ctx->fail(IVX_ERR_CAPACITY, "depth profile quantize: output buffers too small");
    if (*n_out == 0 || (!ok && !os && !oe && !oc)) return IVX_OK;
    IVX_TRY((inclusive_f<SegScan>(ctx, in, QWrite{in, (const ull *)rows, ok, os, oe, oc}, dp.steps)));
    hipLaunchKernelGGL((k_quantize_keys<true>), kgrid, dim3(CT), 0, st, dp, in.d, in.c, nkeys, (const ull *)krows, rows, ok, os, oe, oc);
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}

// out: [nkeys * n_bins] on the device, every element written; 1 <= n_bins <= 65536: the caller's check.  No scratch.
ivx_status ivx_depth_hist_device(ivx_ctx *ctx, const DepthProfileView &dp, u32 nkeys, u32 pos_lo, const u32 *key_hi, int skip_pos0, int seen_only,
                                 i32 v_lo, u32 n_bins, i64 *out)
{
    if (nkeys == 0) return IVX_OK;
    hipStream_t st = ctx->stream;
    const Dom d = make_dom(pos_lo, key_hi, skip_pos0, seen_only);
    IVX_HIP(ctx, hipMemsetAsync(out, 0, (size_t)nkeys * n_bins * sizeof(i64), st));
    hipLaunchKernelGGL(k_hist_keys, dim3((u32)(((u64)nkeys + CT - 1) / CT)), dim3(CT), 0, st, dp, d, v_lo, n_bins, nkeys, (ull *)out);
    if (dp.steps) {
        const u32 ntiles = (u32)((dp.steps + DEPTH_CLASS_TILE - 1) / DEPTH_CLASS_TILE);
        const u32 per = (ntiles + HIST_MAX_WG - 1) / HIST_MAX_WG;
        hipLaunchKernelGGL(k_hist_steps, dim3((ntiles + per - 1) / per), dim3(CT), 0, st, dp, d, v_lo, n_bins, ntiles, per, (ull *)out);
    }
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}
