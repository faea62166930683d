// ivx_depth_regions.hip -- depth region summaries: for regions (or fixed-width windows) of a depth profile, the number of
// bases, the sum of the coverage over them and the number of bases at or above each of up to 8 thresholds (what samtools
// bedcov, mosdepth --by and mosdepth --thresholds report; include/ivx.h ivx_depth_profile_summarize / _windows).
//
//   profile   a sorted step list (ivx_depth_expand.hip): a region's sum is a difference of prefix sums plus two clipped end
//             segments.  A per-step prefix table would cost 8 * (1 + n_thr) bytes per step and the thresholds change with
//             the call, so the prefix sums are kept per TILE of DEPTH_REGION_TILE consecutive steps only.
//   tiles     the tile pass (ivx_depth_regions.hpp tile_steps: which steps count, and the tiles a one-key call skips) with
//             sums: v * length and, per threshold, the length where v >= threshold: 1 + n_thr words a tile, word-major,
//             then ONE exclusive scan over the whole array -- only differences inside a word's row are ever taken, and
//             sums are modulo 2^64, so the rows need no scan of their own.
//   query     one wavefront per region.  The span front (ivx_depth_regions.hpp describes it) finds the region's steps s..b and
//             its zero stretch; the lanes stride over the clipped segments of at most two tiles of steps, and the tiles
//             strictly between come from the scanned aggregates.  A wavefront reduction, and lane 0 stores the region's
//             row.  No atomics, no LDS.
#include "ivx_depth_regions.hpp"

namespace {

constexpr int DEPTH_REGION_TILE = 1024;         // steps per tile aggregate: a region walks at most two tiles of steps
constexpr int MAXT = 8;                         // IVX_DEPTH_MAX_THRESHOLDS
static_assert(1 + MAXT <= RT, "a thread per aggregate word");
static_assert(MAXT == IVX_DEPTH_MAX_THRESHOLDS, "the header's limit");

struct Thr { i32 t[MAXT]; u32 n; };

// a step (or a clipped segment) of value v over len bases: into the sum, and into every threshold's count it reaches
__device__ __forceinline__ void add_step(u64 &sum, u64 (&ge)[MAXT], const Thr &thr, i32 v, u64 len)
{
    sum += (u64)(i64)v * len;
#pragma unroll
    for (int e = 0; e < MAXT; e++)
        if ((u32)e < thr.n && v >= thr.t[e]) ge[e] += len;
}
__device__ __forceinline__ void wave_reduce(u64 &sum, u64 (&ge)[MAXT], const Thr &thr)
{
    sum = (u64)wave_sum((unsigned long long)sum);
#pragma unroll
    for (int e = 0; e < MAXT; e++)
        if ((u32)e < thr.n) ge[e] = (u64)wave_sum((unsigned long long)ge[e]);
}

// ------------------------------------------------------------------------------------------------ tile aggregates
// agg[w * ntiles + tile], w = 0: sum of v * length, w = 1 + e: length where v >= thr.t[e], over the steps tile_steps passes;
// zeros for a skipped tile
__global__ __launch_bounds__(RT) void k_region_tiles(DepthProfileView dp, int skip_pos0, Thr thr, u32 only_key, u32 ntiles, u64 *__restrict__ agg)
{
    __shared__ u64 part[RW][1 + MAXT];
    const u32 t = threadIdx.x, l = lane_id(), w = t / IVX_WAVE;
    if (tile_skipped<DEPTH_REGION_TILE>(dp, only_key)) {
        if (t <= thr.n) agg[(u64)t * ntiles + blockIdx.x] = 0;
        return;
    }
    u64 sum = 0, ge[MAXT];
#pragma unroll
    for (int e = 0; e < MAXT; e++) ge[e] = 0;
    tile_steps<DEPTH_REGION_TILE>(dp, skip_pos0, [&](i32 v, u64 len) { add_step(sum, ge, thr, v, len); });
    wave_reduce(sum, ge, thr);
    if (l == 0) {
        part[w][0] = sum;
#pragma unroll
        for (int e = 0; e < MAXT; e++) part[w][1 + e] = ge[e];
    }
    __syncthreads();
    if (t <= thr.n) {
        u64 r = 0;
#pragma unroll
        for (int x = 0; x < RW; x++) r += part[x][t];
        agg[(u64)t * ntiles + blockIdx.x] = r;
    }
}

// ------------------------------------------------------------------------------------------------ regions
// a key id >= nkeys other than the skip mark (every writer stores the same word: no atomic)
__global__ __launch_bounds__(RT) void k_region_check(const u32 *__restrict__ qkey, u64 n, u32 nkeys, u64 *sc)
{
    for (u64 i = (u64)blockIdx.x * RT + threadIdx.x; i < n; i += (u64)gridDim.x * RT) {
        const u32 k = qkey[i];
        if (k >= nkeys && k != IVX_NULL_IDX) sc[SC_REGIONS_BAD] = 1ull;
    }
}

// the lanes stride over the steps from..to of a span, each adding its clipped segment
__device__ __forceinline__ void walk_steps(const DepthProfileView &dp, u64 from, u64 to, const SpanClip &sp, const Thr &thr, u32 l,
                                           u64 &sum, u64 (&ge)[MAXT])
{
    for (u64 j = from + l; j <= to; j += IVX_WAVE) {
        const StepSegment g = span_segment(dp, sp, j);
        add_step(sum, ge, thr, g.v, g.len);
    }
}

template <typename In>
__global__ __launch_bounds__(RT) void k_region_query(DepthProfileView dp, In in, u64 i0, u64 n, int skip_pos0, Thr thr,
                                                     const u64 *__restrict__ agg, u32 ntiles,
                                                     i64 *__restrict__ out_len, i64 *__restrict__ out_sum, i64 *__restrict__ out_ge)
{
    const u32 l = lane_id();
    const u64 i = query_region(i0);
    if (i >= n) return;
    constexpr u32 T = DEPTH_REGION_TILE;
    u64 len = 0, sum = 0, ge[MAXT];
#pragma unroll
    for (int e = 0; e < MAXT; e++) ge[e] = 0;
    u32 k, lo, hi;
    if (in.get(i, k, lo, hi)) {
        len = (u64)hi - lo + 1u;
        const u32 klo = dp.koff[k], khi = dp.koff[k + 1];
        u64 zero = 0;                                       // bases before the key's first step: coverage 0, and c0 = 0 there
        const u32 ub = wave_first_at_or_after(dp.pos, klo, khi - klo, (u64)hi + 1u, l);
        if (ub == klo) zero = len;                          // no step at or before the end (or a key without steps)
        else {
            const u32 b = ub - 1u;
            const u32 ua = wave_first_at_or_after(dp.pos, klo, ub - klo, (u64)lo + 1u, l);
            u32 s = ua - 1u;
            if (ua == klo) { s = klo; zero = (u64)(dp.pos[klo] - lo); }     // (lo < pos[klo] <= hi)
            const u32 c0 = key_c0(dp, klo, skip_pos0);
            const SpanClip sp{b, c0, lo, hi};
            const u32 ta = s / T, tb = b / T;
            if (tb > ta + 1u) {
                walk_steps(dp, s, (u64)(ta + 1u) * T - 1u, sp, thr, l, sum, ge);
                walk_steps(dp, (u64)tb * T, b, sp, thr, l, sum, ge);
                if (l == 0) {
                    sum += agg[tb] - agg[ta + 1u];
#pragma unroll
                    for (int e = 0; e < MAXT; e++)
                        if ((u32)e < thr.n) ge[e] += agg[(u64)(1 + e) * ntiles + tb] - agg[(u64)(1 + e) * ntiles + ta + 1u];
                }
            } else walk_steps(dp, s, b, sp, thr, l, sum, ge);
        }
        wave_reduce(sum, ge, thr);
#pragma unroll
        for (int e = 0; e < MAXT; e++)
            if ((u32)e < thr.n && thr.t[e] <= 0) ge[e] += zero;
    }
    if (l == 0) {
        if (out_len) out_len[i] = (i64)len;
        if (out_sum) out_sum[i] = (i64)sum;
        if (out_ge) {
#pragma unroll
            for (int e = 0; e < MAXT; e++)
                if ((u32)e < thr.n) out_ge[(u64)e * n + i] = (i64)ge[e];
        }
    }
}

// Scratch: WS_T0 (the tile aggregates), WS_SCAN* (their scan).  A profile of at most two tiles has no tile strictly between
// two others: no aggregates are made.
ivx_status region_aggregates(ivx_ctx *ctx, const DepthProfileView &dp, int skip_pos0, const Thr &thr, u32 only_key, const u64 **agg, u32 *ntiles)
{
    *agg = nullptr;
    *ntiles = (u32)((dp.steps + DEPTH_REGION_TILE - 1) / DEPTH_REGION_TILE);
    if (*ntiles <= 2) return IVX_OK;
    const u64 words = (u64)(1u + thr.n) * *ntiles;
    u64 *a;
    IVX_TRY(ctx->get_scratch(WS_T0, (size_t)words * sizeof(u64), (void **)&a));
    hipLaunchKernelGGL(k_region_tiles, dim3(*ntiles), dim3(RT), 0, ctx->stream, dp, skip_pos0, thr, only_key, *ntiles, a);
    IVX_HIP(ctx, hipGetLastError());
    IVX_TRY(ivx_scan_exclusive_u64(ctx, a, words));
    IVX_HIP(ctx, hipGetLastError());
    *agg = a;
    return IVX_OK;
}

}  // namespace

// the regions' key ids (qkey nullable: every region on key 0) against nkeys, before anything is indexed with them: one word read back
ivx_status ivx_depth_regions_check_keys(ivx_ctx *ctx, const u32 *qkey, u64 n, u32 nkeys)
{
    if (qkey) {
        hipStream_t st = ctx->stream;
        IVX_HIP(ctx, hipMemsetAsync(ctx->dword(SC_REGIONS_BAD), 0, sizeof(u64), st));
        hipLaunchKernelGGL(k_region_check, dim3(ivx_stream_grid(n, RT)), dim3(RT), 0, st, qkey, n, nkeys, ctx->d_scalars);
        IVX_HIP(ctx, hipGetLastError());
        IVX_TRY(ctx->check_flag(SC_REGIONS_BAD, st, "depth profile: key id >= n_keys"));
    } else if (nkeys == 0) return ctx->fail(IVX_ERR_INVALID, "depth profile: key id >= n_keys");
    return IVX_OK;
}

ivx_status ivx_depth_region_sums_device(ivx_ctx *ctx, const DepthProfileView &dp, u32 nkeys, const DepthRegionSrc &src,
                                        const i32 *thresholds, u32 n_thr, i64 *out_len, i64 *out_sum, i64 *out_ge)
{
    if (src.n == 0) return IVX_OK;
    if (!src.windows) IVX_TRY(ivx_depth_regions_check_keys(ctx, src.qkey, src.n, nkeys));
    if (!out_len && !out_sum && !(out_ge && n_thr)) return IVX_OK;
    Thr thr{};
    thr.n = n_thr;
    for (u32 e = 0; e < n_thr; e++) thr.t[e] = thresholds[e];
    return with_region_in(src, [&](const auto &in, u32 only_key) -> ivx_status {
        using In = std::decay_t<decltype(in)>;
        const u64 *agg; u32 ntiles;
        IVX_TRY(region_aggregates(ctx, dp, src.skip_pos0, thr, only_key, &agg, &ntiles));
        query_chunks(src.n, [&](u64 i0, dim3 grid) {
            hipLaunchKernelGGL((k_region_query<In>), grid, dim3(RT), 0, ctx->stream, dp, in, i0, src.n, src.skip_pos0, thr, agg, ntiles, out_len, out_sum, out_ge);
        });
        IVX_HIP(ctx, hipGetLastError());
        return IVX_OK;
    });
}
