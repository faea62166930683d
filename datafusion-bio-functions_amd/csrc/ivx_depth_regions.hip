// ivx_depth_regions.hip -- depth region summaries: for regions (or fixed-width windows) of a depth profile, the number of
// bases, the sum of the coverage over them and the number of bases at or above each of up to 8 thresholds (what samtools
// bedcov, mosdepth --by and mosdepth --thresholds report; include/ivx.h ivx_depth_profile_summarize / _windows).
//
//   profile   a sorted step list (ivx_depth_expand.hip): a region's sum is a difference of prefix sums plus two clipped end
//             segments.  A per-step prefix table would cost 8 * (1 + n_thr) bytes per step and the thresholds change with
//             the call, so the prefix sums are kept per TILE of DEPTH_REGION_TILE consecutive steps only.
//   tiles     one workgroup per tile reduces, over its steps that have a successor with the same key, v * (next position -
//             position) and, per threshold, that length where v >= threshold: 1 + n_thr words a tile, word-major, then ONE
//             exclusive scan over the whole array -- only differences inside a word's row are ever taken, and sums are
//             modulo 2^64, so the rows need no scan of their own.  A key's last step has no length until the region's
//             domain gives it one: it adds nothing here.
//   query     one wavefront per region.  Two 64-ary wavefront searches inside the key's slice (the search of the expand
//             kernel, restated; in ivx_depth_regions.hpp with the regions' bounds, shared with ivx_depth_rank.hip) find b, the last step at or before the clipped end, and a, the last step at or before the
//             clipped start.  With a and b in one tile or in adjacent tiles the lanes stride over the steps a..b, the first
//             and the last segment clipped; otherwise they walk a's tile tail and b's tile head, and the tiles strictly
//             between come from the scanned aggregates (every step there has a same-key successor, b at the latest).  A
//             wavefront reduction, and lane 0 stores the region's row.  No atomics, no LDS.
//             The region index is made wave-uniform for the compiler, so the region's bounds and the key's slice arrive
//             through scalar loads and every branch on them is a scalar branch.
#include "ivx_depth_regions.hpp"

namespace {

constexpr int DEPTH_REGION_TILE = 1024;         // steps per tile aggregate: a region walks at most two tiles of steps
constexpr int RT = 256;                         // threads of both kernels
constexpr int RW = RT / IVX_WAVE;               // regions per workgroup of the query: one per wavefront
constexpr int RS = DEPTH_REGION_TILE / RT;      // steps per thread of the tile pass
constexpr int MAXT = 8;                         // IVX_DEPTH_MAX_THRESHOLDS
static_assert(DEPTH_REGION_TILE % RT == 0 && RT % IVX_WAVE == 0 && 1 + MAXT <= RT, "whole steps per thread; a thread per aggregate word");
static_assert(MAXT == IVX_DEPTH_MAX_THRESHOLDS, "the header's limit");

constexpr u64 QUERY_CHUNK = (u64)RW << 23;      // regions per launch: the grid times the workgroup stays below 2^32 threads

struct Thr { i32 t[MAXT]; u32 n; };

__device__ __forceinline__ void wave_reduce(u64 &sum, u64 (&ge)[MAXT], const Thr &thr)
{
    sum = (u64)wave_sum((unsigned long long)sum);
#pragma unroll
    for (int e = 0; e < MAXT; e++)
        if ((u32)e < thr.n) ge[e] = (u64)wave_sum((unsigned long long)ge[e]);
}

// ------------------------------------------------------------------------------------------------ tile aggregates
// agg[w * ntiles + tile], w = 0: sum of v * length, w = 1 + e: length where v >= thr.t[e]; over the tile's steps whose
// successor has the same key.  only_key != IVX_NULL_IDX (the windows call: every region is on that key): a tile without a step
// of the key is never read back, it gets zeros and loads nothing.
__global__ __launch_bounds__(RT) void k_region_tiles(DepthProfileView dp, int skip_pos0, Thr thr, u32 only_key, u32 ntiles, u64 *__restrict__ agg)
{
    __shared__ u64 part[RW][1 + MAXT];
    const u32 t = threadIdx.x, l = lane_id(), w = t / IVX_WAVE;
    const u64 base = (u64)blockIdx.x * DEPTH_REGION_TILE;
    if (only_key != IVX_NULL_IDX && (base >= dp.koff[only_key + 1] || base + DEPTH_REGION_TILE <= dp.koff[only_key])) {
        if (t <= thr.n) agg[(u64)t * ntiles + blockIdx.x] = 0;      // (the same for the whole workgroup)
        return;
    }
    u64 sum = 0, ge[MAXT];
#pragma unroll
    for (int e = 0; e < MAXT; e++) ge[e] = 0;
#pragma unroll
    for (int j = 0; j < RS; j++) {
        const u64 i = base + t + (u64)RT * j;
        if (i + 1 >= dp.steps) continue;
        const u32 k = dp.key[i];
        if (dp.key[i + 1] != k) continue;
        const u32 c0 = skip_pos0 ? key_c0(dp, dp.koff[k], 1) : 0u;
        const i32 v = (i32)((u32)dp.cov[i] - c0);
        const u64 len = (u64)(dp.pos[i + 1] - dp.pos[i]);
        sum += (u64)(i64)v * len;
#pragma unroll
        for (int e = 0; e < MAXT; e++)
            if ((u32)e < thr.n && v >= thr.t[e]) ge[e] += len;
    }
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

// the lanes stride over the steps from..to (from <= to <= b): step j covers [max(pos[j], lo), j < b ? pos[j + 1] - 1 : hi]
__device__ __forceinline__ void walk_steps(const DepthProfileView &dp, u64 from, u64 to, u32 b, u32 lo, u32 hi, u32 c0, const Thr &thr, u32 l,
                                           u64 &sum, u64 (&ge)[MAXT])
{
    for (u64 j = from + l; j <= to; j += IVX_WAVE) {
        const u32 p = dp.pos[j];
        const u64 start = p > lo ? p : lo;
        const u64 end = j < b ? (u64)dp.pos[j + 1] : (u64)hi + 1u;
        const u64 len = end - start;
        const i32 v = (i32)((u32)dp.cov[j] - c0);
        sum += (u64)(i64)v * len;
#pragma unroll
        for (int e = 0; e < MAXT; e++)
            if ((u32)e < thr.n && v >= thr.t[e]) ge[e] += len;
    }
}

template <typename In>
__global__ __launch_bounds__(RT) void k_region_query(DepthProfileView dp, In in, u64 i0, u64 n, int skip_pos0, Thr thr,
                                                     const u64 *__restrict__ agg, u32 ntiles,
                                                     i64 *__restrict__ out_len, i64 *__restrict__ out_sum, i64 *__restrict__ out_ge)
{
    constexpr u32 T = DEPTH_REGION_TILE;
    const u32 l = lane_id();
    const u64 i = i0 + (u64)blockIdx.x * RW + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / IVX_WAVE));
    if (i >= n) return;
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
            const u32 ta = s / T, tb = b / T;
            if (tb > ta + 1u) {
                walk_steps(dp, s, (u64)(ta + 1u) * T - 1u, b, lo, hi, c0, thr, l, sum, ge);
                walk_steps(dp, (u64)tb * T, b, b, lo, hi, c0, thr, l, sum, ge);
                if (l == 0) {
                    sum += agg[tb] - agg[ta + 1u];
#pragma unroll
                    for (int e = 0; e < MAXT; e++)
                        if ((u32)e < thr.n) ge[e] += agg[(u64)(1 + e) * ntiles + tb] - agg[(u64)(1 + e) * ntiles + ta + 1u];
                }
            } else walk_steps(dp, s, b, b, lo, hi, c0, thr, l, sum, ge);
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

template <typename In>
ivx_status region_query(ivx_ctx *ctx, const DepthProfileView &dp, const In &in, u32 only_key, u64 n, int skip_pos0, const Thr &thr,
                        i64 *out_len, i64 *out_sum, i64 *out_ge)
{
    const u64 *agg; u32 ntiles;
    IVX_TRY(region_aggregates(ctx, dp, skip_pos0, thr, only_key, &agg, &ntiles));
    for (u64 i0 = 0; i0 < n; i0 += QUERY_CHUNK) {
        const u64 m = n - i0 < QUERY_CHUNK ? n - i0 : QUERY_CHUNK;
        hipLaunchKernelGGL((k_region_query<In>), dim3((u32)((m + RW - 1) / RW)), dim3(RT), 0, ctx->stream, dp, in, i0, n, skip_pos0, thr,
                           agg, ntiles, out_len, out_sum, out_ge);
    }
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}

Thr make_thr(const i32 *thresholds, u32 n_thr)
{
    Thr t{};
    t.n = n_thr;
    for (u32 e = 0; e < n_thr; e++) t.t[e] = thresholds[e];
    return t;
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

// thresholds: host memory, n_thr <= 8; every other pointer on the device.  Reads one word back when qkey is given: a key id
// >= nkeys other than the skip mark is found before anything is indexed with it, and nothing is written then.
ivx_status ivx_depth_regions_device(ivx_ctx *ctx, const DepthProfileView &dp, u32 nkeys, const u32 *qkey, const u32 *qs, const u32 *qe, u64 n,
                                    u32 pos_lo, const u32 *key_hi, int skip_pos0, const i32 *thresholds, u32 n_thr,
                                    i64 *out_len, i64 *out_sum, i64 *out_ge)
{
    if (n == 0) return IVX_OK;
    IVX_TRY(ivx_depth_regions_check_keys(ctx, qkey, n, nkeys));
    if (!out_len && !out_sum && !(out_ge && n_thr)) return IVX_OK;
    return region_query(ctx, dp, RegionsIn{qkey, qs, qe, key_hi, pos_lo}, qkey ? IVX_NULL_IDX : 0u, n, skip_pos0, make_thr(thresholds, n_thr), out_len, out_sum, out_ge);
}

// window i = [first_pos + i * width, + width - 1], cut at last_pos; key < nkeys and first_pos + (n - 1) * width < 2^32: the caller's checks
ivx_status ivx_depth_windows_device(ivx_ctx *ctx, const DepthProfileView &dp, u32 key, u32 first_pos, u32 last_pos, u32 width, u64 n,
                                    int skip_pos0, const i32 *thresholds, u32 n_thr, i64 *out_len, i64 *out_sum, i64 *out_ge)
{
    if (n == 0 || (!out_len && !out_sum && !(out_ge && n_thr))) return IVX_OK;
    return region_query(ctx, dp, WindowsIn{key, first_pos, last_pos, width}, key, n, skip_pos0, make_thr(thresholds, n_thr), out_len, out_sum, out_ge);
}
