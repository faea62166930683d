// ivx_depth_rank.hip -- depth region order statistics: for regions (or fixed-width windows) of a depth profile, the number of
// bases, the smallest and the largest per-base coverage and up to 8 lower quantiles of it (bedtools map -o min,max, Picard
// MIN_ / MEDIAN_TARGET_COVERAGE, mosdepth --use-median; include/ivx.h ivx_depth_profile_quantiles / _window_quantiles).
//
//   profile   a sorted step list.  A region's per-base values are a list of SEGMENTS (value, length): the zero stretch before
//             the key's first step if it has length, then the steps s..b of the region's span, the first and the last one
//             clipped to the region (ivx_depth_regions.hpp: the segment rule).  Every segment has length >= 1.
//   tiles     one workgroup per tile of DEPTH_RANK_TILE consecutive steps reduces (min, max) of v over the steps the shared
//             tile walk passes (ivx_depth_regions.hpp tile_steps); a tile without one gets the neutral pair.  Over the tiles
//             a sparse table: level l, entry t = the pair of tiles t .. t + 2^l - 1, levels up to log2(tiles - 2), several
//             levels a launch.  8 bytes a tile and level.
//   query     one wavefront per region: the span front (ivx_depth_regions.hpp describes it), then (min, max) over s's tile tail,
//             b's tile head and two table look-ups for the tiles strictly between, the zero stretch's 0, a wavefront
//             reduction.  Two searches and at most two tiles of steps, whatever the region's length.
//             Quantiles of at most DEPTH_RANK_SEGS = 64 segments: one segment per lane; in as many broadcast rounds as there
//             are segments every lane adds up `below`, the bases of the segments with a smaller value, and `atmost`, the
//             same for <=; the value of rank r sits in any lane with below <= r < atmost.  Registers only.
//             More segments: lane 0 appends the region to a device list (one vector atomic add on a counter word).
//   select    DEPTH_RANK_SELECT_GRID workgroups, launched without knowing the list's length: they read it on the device and
//             take the listed regions grid-stride, one region a workgroup.  A radix select on u = (u32)v - (u32)min, only as
//             many 8-bit digits as max - min needs (1 to 4), most significant first: per pass one walk over the region's steps
//             adds the clipped lengths to 256 64-bit LDS bins (a bin can reach 2^32) per DISTINCT prefix the quantiles have
//             reached so far, a workgroup scan finds each quantile's bin.  A coverage span below 256 (the usual case) is one
//             walk for all quantiles.  Cost: linear in the region's steps, times the passes.
#include "ivx_depth_regions.hpp"

namespace {

constexpr int DEPTH_RANK_TILE = 1024;           // steps per (min, max) tile: the sums' DEPTH_REGION_TILE
constexpr int DEPTH_RANK_SEGS = 64;             // segments the query wavefront ranks in registers: one per lane
constexpr int DEPTH_RANK_SELECT_GRID = 512;     // workgroups of the select kernel: two per compute unit
constexpr int MAXQ = 8;                         // IVX_DEPTH_MAX_QUANTILES
constexpr u32 TABLE_LEVELS = 4;                 // table levels one launch makes: up to 16 reads an entry
static_assert(DEPTH_RANK_SEGS == IVX_WAVE && RT == 256, "a lane per segment; a thread per bin");
static_assert(MAXQ == IVX_DEPTH_MAX_QUANTILES, "the header's limit");

constexpr i32 I32_LO = (i32)0x80000000, I32_HI = 0x7FFFFFFF;

struct Qn { u32 num[MAXQ]; u32 n, den; };
struct LongRegion { u64 i; u32 s, b; i32 mn, mx; };        // a region for the select kernel: its index, first and last step, extremes

__device__ __forceinline__ i32 wave_min(i32 v)
{
#pragma unroll
    for (int d = IVX_WAVE / 2; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, IVX_WAVE));
    return v;
}
__device__ __forceinline__ i32 wave_max(i32 v)
{
#pragma unroll
    for (int d = IVX_WAVE / 2; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, IVX_WAVE));
    return v;
}
__device__ __forceinline__ int2 both(int2 a, int2 b) { return make_int2(min(a.x, b.x), max(a.y, b.y)); }
__device__ __forceinline__ u64 lane_u64(u64 v, u32 lane)       // lane: wave-uniform
{
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)v, (int)lane), hi = (u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), (int)lane);
    return (u64)hi << 32 | lo;
}

// ------------------------------------------------------------------------------------------------ tiles and their table
// tab[tile] = (min, max) of v over the steps tile_steps passes; the neutral pair for a skipped tile
__global__ __launch_bounds__(RT) void k_rank_tiles(DepthProfileView dp, int skip_pos0, u32 only_key, int2 *__restrict__ tab)
{
    __shared__ int2 part[RW];
    const u32 t = threadIdx.x;
    if (tile_skipped<DEPTH_RANK_TILE>(dp, only_key)) {
        if (t == 0) tab[blockIdx.x] = make_int2(I32_HI, I32_LO);
        return;
    }
    i32 mn = I32_HI, mx = I32_LO;
    tile_steps<DEPTH_RANK_TILE>(dp, skip_pos0, [&](i32 v, u64) { mn = min(mn, v); mx = max(mx, v); });
    mn = wave_min(mn); mx = wave_max(mx);
    if (lane_id() == 0) part[t / IVX_WAVE] = make_int2(mn, mx);
    __syncthreads();
    if (t == 0) {
        int2 r = part[0];
#pragma unroll
        for (int x = 1; x < RW; x++) r = both(r, part[x]);
        tab[blockIdx.x] = r;
    }
}

// levels lb + 1 .. lb + nl from level lb: entry t of level lb + j = the entries t + m * 2^lb of level lb, m < 2^j; entries
// whose tiles would run past the last one are never read and are not made
__global__ __launch_bounds__(RT) void k_rank_table(int2 *__restrict__ tab, u32 ntiles, u32 lb, u32 nl)
{
    const int2 *src = tab + (u64)lb * ntiles;
    for (u64 x = (u64)blockIdx.x * RT + threadIdx.x; x < (u64)nl * ntiles; x += (u64)gridDim.x * RT) {
        const u32 j = 1u + (u32)(x / ntiles), t = (u32)(x % ntiles);
        if ((u64)t + (1ull << (lb + j)) > ntiles) continue;
        int2 r = src[t];
        for (u32 m = 1; m < (1u << j); m++) r = both(r, src[t + ((u64)m << lb)]);
        tab[(u64)(lb + j) * ntiles + t] = r;
    }
}

// ------------------------------------------------------------------------------------------------ query
// (min, max) of v over the steps from..to, the lanes striding: every one of them lies inside the region with at least a base
__device__ __forceinline__ void walk_extremes(const DepthProfileView &dp, u64 from, u64 to, u32 c0, u32 l, i32 &mn, i32 &mx)
{
    for (u64 j = from + l; j <= to; j += IVX_WAVE) {
        const i32 v = (i32)((u32)dp.cov[j] - c0);
        mn = min(mn, v); mx = max(mx, v);
    }
}

template <typename In>
__global__ __launch_bounds__(RT) void k_rank_query(DepthProfileView dp, In in, u64 i0, u64 n, int skip_pos0, Qn q,
                                                   const int2 *__restrict__ tab, u32 ntiles,
                                                   i64 *__restrict__ out_len, i32 *__restrict__ out_min, i32 *__restrict__ out_max, i32 *__restrict__ out_q,
                                                   LongRegion *__restrict__ list, u64 *counter)
{
    constexpr u32 T = DEPTH_RANK_TILE;
    const u32 l = lane_id();
    const u64 i = query_region(i0);
    if (i >= n) return;
    u64 len = 0;
    i32 mn = 0, mx = 0, qv[MAXQ];
#pragma unroll
    for (int e = 0; e < MAXQ; e++) qv[e] = 0;
    bool listed = false;                                    // the select kernel writes this region's quantiles
    u32 k, lo, hi;
    if (in.get(i, k, lo, hi)) {
        len = (u64)hi - lo + 1u;
        const u32 klo = dp.koff[k], khi = dp.koff[k + 1];
        const u32 ub = wave_first_at_or_after(dp.pos, klo, khi - klo, (u64)hi + 1u, l);
        if (ub != klo) {                                    // (else no step at or before the end: zeros throughout)
            const u32 b = (u32)__builtin_amdgcn_readfirstlane((int)(ub - 1u));
            const u32 ua = wave_first_at_or_after(dp.pos, klo, ub - klo, (u64)lo + 1u, l);
            u32 s = ua - 1u;
            u64 zero = 0;                                   // bases before the key's first step: coverage 0, and c0 = 0 there
            if (ua == klo) { s = klo; zero = (u64)(dp.pos[klo] - lo); }     // (lo < pos[klo] <= hi)
            s = (u32)__builtin_amdgcn_readfirstlane((int)s);
            const u32 c0 = key_c0(dp, klo, skip_pos0);
            const u32 ta = s / T, tb = b / T;
            i32 a = I32_HI, z = I32_LO;
            if (tb > ta + 1u) {
                walk_extremes(dp, s, (u64)(ta + 1u) * T - 1u, c0, l, a, z);
                walk_extremes(dp, (u64)tb * T, b, c0, l, a, z);
                if (l == 0) {                               // the tiles ta + 1 .. tb - 1: two entries of the level that half covers them
                    const u32 lv = 31u - (u32)__clz(tb - ta - 1u);
                    const int2 r = both(tab[(u64)lv * ntiles + ta + 1u], tab[(u64)lv * ntiles + tb - (1u << lv)]);
                    a = min(a, r.x); z = max(z, r.y);
                }
            } else walk_extremes(dp, s, b, c0, l, a, z);
            if (zero) { a = min(a, 0); z = max(z, 0); }
            mn = wave_min(a); mx = wave_max(z);
            if (q.n && out_q) {
                const u32 zs = zero ? 1u : 0u;
                const u64 nseg = (u64)(b - s) + 1u + zs;
                if (nseg <= (u64)DEPTH_RANK_SEGS) {
                    const u32 ns = (u32)__builtin_amdgcn_readfirstlane((int)(u32)nseg);
                    i32 v = 0;
                    u64 ln = 0;                             // (a lane without a segment: no bases, and it never answers)
                    if (l < ns && !(zs && l == 0)) {
                        const StepSegment g = span_segment(dp, SpanClip{b, c0, lo, hi}, s + l - zs);
                        v = g.v; ln = g.len;
                    } else if (l == 0 && zs) ln = zero;
                    u64 below = 0, atmost = 0;
                    for (u32 r = 0; r < ns; r++) {
                        const i32 bv = __builtin_amdgcn_readlane(v, (int)r);
                        const u64 bl = lane_u64(ln, r);
                        below += bv < v ? bl : 0ull;
                        atmost += bv <= v ? bl : 0ull;
                    }
#pragma unroll
                    for (int e = 0; e < MAXQ; e++) {
                        if ((u32)e >= q.n) continue;
                        const u64 r = (len - 1u) * q.num[e] / q.den;
                        const u64 hit = __ballot(l < ns && below <= r && r < atmost);
                        if (hit) qv[e] = __builtin_amdgcn_readlane(v, __ffsll((unsigned long long)hit) - 1);
                    }
                } else {
                    listed = true;
                    if (l == 0) list[atomicAdd((unsigned long long *)counter, 1ull)] = LongRegion{i, s, b, mn, mx};
                }
            }
        }
    }
    if (l == 0) {
        if (out_len) out_len[i] = (i64)len;
        if (out_min) out_min[i] = mn;
        if (out_max) out_max[i] = mx;
        if (out_q && !listed) {
#pragma unroll
            for (int e = 0; e < MAXQ; e++)
                if ((u32)e < q.n) out_q[(u64)e * n + i] = qv[e];
        }
    }
}

// ------------------------------------------------------------------------------------------------ select
template <typename In>
__global__ __launch_bounds__(RT) void k_rank_select(DepthProfileView dp, In in, u64 n, int skip_pos0, Qn q,
                                                    const LongRegion *__restrict__ list, const u64 *__restrict__ counter, i32 *__restrict__ out_q)
{
    __shared__ u64 hist[MAXQ][RT];                          // per quantile that owns a prefix: bases per digit value
    __shared__ u64 scan_lds[RW + 1];
    __shared__ u32 prefix[MAXQ];                            // the digits of quantile e found so far
    __shared__ u64 rem[MAXQ];                               // its rank among the values with that prefix
    const u32 t = threadIdx.x;
    const u64 cnt = *counter;
    for (u64 x = blockIdx.x; x < cnt; x += gridDim.x) {
        const LongRegion R = list[x];
        u32 k, lo, hi;
        in.get(R.i, k, lo, hi);                             // (not empty: it was listed)
        const u32 klo = dp.koff[k];
        const u32 c0 = key_c0(dp, klo, skip_pos0);
        const u32 p0 = dp.pos[klo];
        const u64 zero = (R.s == klo && lo < p0) ? (u64)(p0 - lo) : 0ull;
        const u64 len = (u64)hi - lo + 1u;
        const SpanClip sp{R.b, c0, lo, hi};
        const u32 span = (u32)R.mx - (u32)R.mn;
        const int ndig = span < 256u ? 1 : span < 65536u ? 2 : span < (1u << 24) ? 3 : 4;
        if (t < q.n) { prefix[t] = 0u; rem[t] = (len - 1u) * q.num[t] / q.den; }
        for (int d = ndig - 1; d >= 0; d--) {
            for (u32 y = t; y < q.n * RT; y += RT) (&hist[0][0])[y] = 0ull;
            __syncthreads();
            u32 pf[MAXQ];
#pragma unroll
            for (int e = 0; e < MAXQ; e++) pf[e] = (u32)e < q.n ? prefix[e] : 0u;
            const bool top = d == ndig - 1;                 // no digit found yet: every value has the (empty) prefix
            auto add = [&](u32 u, u64 ln) {
                const u32 up = top ? 0u : u >> (8 * (d + 1));
#pragma unroll
                for (int e = 0; e < MAXQ; e++)              // the first quantile with this prefix owns its histogram
                    if ((u32)e < q.n && pf[e] == up) { atomicAdd((unsigned long long *)&hist[e][(u >> (8 * d)) & 255u], (unsigned long long)ln); break; }
            };
            if (t == 0 && zero) add(0u - (u32)R.mn, zero);
            for (u64 j = (u64)R.s + t; j <= R.b; j += RT) {
                const StepSegment g = span_segment(dp, sp, j);
                add((u32)g.v - (u32)R.mn, g.len);
            }
            __syncthreads();
            for (u32 e = 0; e < q.n; e++) {
                u32 o = e;                                  // the owner of e's prefix
                for (u32 f = e; f-- > 0;)
                    if (pf[f] == pf[e]) o = f;
                const u64 h = hist[o][t], r = rem[e];
                u64 total;
                const u64 ex = block_excl_scan<u64, RT>(h, scan_lds, &total);
                if (ex <= r && r < ex + h) { prefix[e] = pf[e] << 8 | t; rem[e] = r - ex; }
            }
            __syncthreads();
        }
        if (t < q.n) out_q[(u64)t * n + R.i] = (i32)((u32)R.mn + prefix[t]);
        __syncthreads();
    }
}

// Scratch: WS_T0 (the table: 8 bytes a tile and level).  A profile of at most two tiles has no tile strictly between two
// others: no table is made.
ivx_status rank_table(ivx_ctx *ctx, const DepthProfileView &dp, int skip_pos0, u32 only_key, const int2 **tab, u32 *ntiles)
{
    *tab = nullptr;
    *ntiles = (u32)((dp.steps + DEPTH_RANK_TILE - 1) / DEPTH_RANK_TILE);
    if (*ntiles <= 2) return IVX_OK;
    u32 top = 0;                                            // the highest level a region can ask for: 2^top <= tiles - 2
    while ((2ull << top) <= (u64)*ntiles - 2u) top++;
    int2 *a;
    IVX_TRY(ctx->get_scratch(WS_T0, (size_t)(top + 1u) * *ntiles * sizeof(int2), (void **)&a));
    hipLaunchKernelGGL(k_rank_tiles, dim3(*ntiles), dim3(RT), 0, ctx->stream, dp, skip_pos0, only_key, a);
    for (u32 lb = 0; lb < top; lb += TABLE_LEVELS) {
        const u32 nl = top - lb < TABLE_LEVELS ? top - lb : TABLE_LEVELS;
        hipLaunchKernelGGL(k_rank_table, dim3(ivx_stream_grid((u64)nl * *ntiles, RT)), dim3(RT), 0, ctx->stream, a, *ntiles, lb, nl);
    }
    IVX_HIP(ctx, hipGetLastError());
    *tab = a;
    return IVX_OK;
}

}  // namespace

// Scratch: rank_table's, and WS_T1 (the long-region list: 24 bytes a region) when quantiles are asked for.
ivx_status ivx_depth_region_ranks_device(ivx_ctx *ctx, const DepthProfileView &dp, u32 nkeys, const DepthRegionSrc &src,
                                         const u32 *q_num, u32 n_q, u32 q_den, i64 *out_len, i32 *out_min, i32 *out_max, i32 *out_q)
{
    const u64 n = src.n;
    if (n == 0) return IVX_OK;
    if (!src.windows) IVX_TRY(ivx_depth_regions_check_keys(ctx, src.qkey, n, nkeys));
    if (!out_len && !out_min && !out_max && !(out_q && n_q)) return IVX_OK;
    Qn q{};
    q.n = n_q; q.den = q_den;
    for (u32 e = 0; e < n_q; e++) q.num[e] = q_num[e];
    return with_region_in(src, [&](const auto &in, u32 only_key) -> ivx_status {
        using In = std::decay_t<decltype(in)>;
        const int2 *tab; u32 ntiles;
        IVX_TRY(rank_table(ctx, dp, src.skip_pos0, only_key, &tab, &ntiles));
        const bool ranks = q.n && out_q;
        LongRegion *list = nullptr;
        u64 *counter = ctx->dword(SC_RANK_LONG);
        if (ranks) {
            IVX_TRY(ctx->get_scratch(WS_T1, (size_t)n * sizeof(LongRegion), (void **)&list));
            IVX_HIP(ctx, hipMemsetAsync(counter, 0, sizeof(u64), ctx->stream));
        }
        query_chunks(n, [&](u64 i0, dim3 grid) {
            hipLaunchKernelGGL((k_rank_query<In>), grid, dim3(RT), 0, ctx->stream, dp, in, i0, n, src.skip_pos0, q,
                               tab, ntiles, out_len, out_min, out_max, out_q, list, counter);
        });
        if (ranks)
            hipLaunchKernelGGL((k_rank_select<In>), dim3(DEPTH_RANK_SELECT_GRID), dim3(RT), 0, ctx->stream, dp, in, n, src.skip_pos0, q, list, counter, out_q);
        IVX_HIP(ctx, hipGetLastError());
        return IVX_OK;
    });
}
