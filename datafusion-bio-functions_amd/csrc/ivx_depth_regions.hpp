// ivx_depth_regions.hpp -- what the kernels that read a depth profile's step list share
// (ivx_depth_regions.hip: sums and threshold counts; ivx_depth_rank.hip: min, max and quantiles; ivx_depth_expand.hip: the
// search and c0): where a region's key and bounds come from, the per-key c0, the 64-ary wavefront search inside a key's slice,
// the clipped segment of a step, the tile pass's walk over the steps with a same-key successor, and the chunked launch of one
// wavefront per region.
#pragma once
#include "ivx_device.hpp"

constexpr int RT = 256;                         // threads of the tile pass and of the query
constexpr int RW = RT / IVX_WAVE;               // regions per workgroup of the query: one per wavefront
constexpr u64 QUERY_CHUNK = (u64)RW << 23;      // regions per launch: the grid times the workgroup stays below 2^32 threads
static_assert(RT % IVX_WAVE == 0, "whole wavefronts");

// c0 of a key with steps: the coverage of its step at position 0 when skip_pos0 is set and that step exists
__device__ __forceinline__ u32 key_c0(const DepthProfileView &dp, u32 first, int skip_pos0)
{
    return (skip_pos0 && dp.pos[first] == 0u) ? (u32)dp.cov[first] : 0u;
}

// where a region's key and closed bounds come from; get() returns false for an empty region
struct RegionsIn {
    const u32 *qkey, *qs, *qe, *key_hi; u32 pos_lo;
    __device__ __forceinline__ bool get(u64 i, u32 &k, u32 &lo, u32 &hi) const
    {
        k = qkey ? qkey[i] : 0u;
        if (k == IVX_NULL_IDX) return false;
        const u32 s = qs[i], e = qe[i];
        if (e < s) return false;
        const u32 dh = key_hi ? key_hi[k] : 0xFFFFFFFFu;
        lo = s > pos_lo ? s : pos_lo;
        hi = e < dh ? e : dh;
        return lo <= hi;                                    // (false also for a domain that ends below pos_lo)
    }
};
struct WindowsIn {
    u32 key, first, last, width;
    __device__ __forceinline__ bool get(u64 i, u32 &k, u32 &lo, u32 &hi) const
    {
        k = key;
        const u64 s = (u64)first + i * width;               // (<= 2^32 - 1: checked by the caller)
        if (s > last) return false;
        const u64 e = s + width - 1u;
        lo = (u32)s;
        hi = e > last ? last : (u32)e;
        return true;
    }
};
// a table's key ids (qkey nullable: every region on key 0) against nkeys: a key id >= nkeys other than the skip mark is
// IVX_ERR_INVALID (one word read back).  ivx_depth_regions.hip; both statistics run it before anything is indexed with a key.
ivx_status ivx_depth_regions_check_keys(ivx_ctx *ctx, const u32 *qkey, u64 n, u32 nkeys);
// the host's descriptor (ivx_internal.hpp) as the one of the two a kernel takes, and the key every region is on (none: IVX_NULL_IDX)
template <typename F>
inline ivx_status with_region_in(const DepthRegionSrc &r, F &&run)
{
    if (r.windows) return run(WindowsIn{r.key, r.first_pos, r.last_pos, r.width}, r.key);
    return run(RegionsIn{r.qkey, r.qstart, r.qend, r.key_hi, r.pos_lo}, r.qkey ? IVX_NULL_IDX : 0u);
}

// the first step of [lo, lo + len) at a position >= x, lo + len if there is none: 64 probes a round, every lane of the
// wavefront with the same arguments.  (32-bit throughout: a profile holds fewer than 2^32 - 256 steps.)
__device__ __forceinline__ u32 wave_first_at_or_after(const u32 *__restrict__ pos, u32 lo, u32 len, u64 x, u32 l)
{
    while (len) {
        const u32 stride = (len + 63u) >> 6;
        const u32 off = (l + 1u) * stride - 1u;
        const bool less = off < len && (u64)pos[lo + off] < x;
        const u32 cnt = (u32)__popcll(__ballot(less));      // the probes before the answer: a prefix of the lanes
        const u32 skip = min(cnt * stride, len);            // steps known to lie before the answer
        lo += skip;
        len = min(len - skip, stride - 1u);                 // the first probe that is not before it bounds the answer
    }
    return lo;
}

// A region's span over the step list, as both queries find it (k_region_query, k_rank_query): two searches inside the key's
// slice give b, the last step at or before the clipped end hi, and s, the last step at or before the clipped start lo; without
// a b the region holds zero coverage only, and a start before the key's first step leaves a zero stretch (c0 = 0 there) and s
// = that step.  With s and b in one tile or in adjacent tiles the lanes walk the steps s..b; otherwise they walk s's tile tail
// and b's tile head, and lane 0 takes the tiles strictly between from what the tile pass left (every step there has a same-key
// successor, b at the latest).  The two kernels write this front out: as one function filling a span struct, with the tile split
// taking two callables, the sums' windows query measured 1.2 % slower than before (profiles/depth_region_front_ab.txt), and the
// instruction sequences show why not: only the written-out form compiles to the code it had.  What they share is below.

// step j of a span (s <= j <= b) covers [max(pos[j], lo), j < b ? pos[j + 1] - 1 : hi]: its value and its bases, at least one
struct SpanClip { u32 b, c0, lo, hi; };
struct StepSegment { i32 v; u64 len; };
__device__ __forceinline__ StepSegment span_segment(const DepthProfileView &dp, const SpanClip &sp, u64 j)
{
    const u32 p = dp.pos[j];
    const u64 start = p > sp.lo ? p : sp.lo;
    const u64 end = j < sp.b ? (u64)dp.pos[j + 1] : (u64)sp.hi + 1u;
    return StepSegment{(i32)((u32)dp.cov[j] - sp.c0), end - start};
}

// The tile pass that feeds the tiles strictly between: one workgroup of RT threads per tile of T consecutive steps (tiles are
// cut over the whole step list), T / RT steps a thread.  step(v, len) gets every step of the tile whose successor has the same
// key: its value (int32)(cov - c0) and its bases up to the successor.  A key's last step has no length until a region's
// domain gives it one: it is not passed.  The caller keeps its accumulator and reduces it: sums in k_region_tiles, (min, max)
// in k_rank_tiles.
// tile_skipped: only_key != IVX_NULL_IDX (the windows call: every region is on that key) and the tile holds no step of the key.
// It is never read back: the caller asks first, stores its neutral words and loads nothing (the same for the whole workgroup).
template <int T>
__device__ __forceinline__ bool tile_skipped(const DepthProfileView &dp, u32 only_key)
{
    const u64 base = (u64)blockIdx.x * T;
    return only_key != IVX_NULL_IDX && (base >= dp.koff[only_key + 1] || base + T <= dp.koff[only_key]);
}
template <int T, typename Step>
__device__ __forceinline__ void tile_steps(const DepthProfileView &dp, int skip_pos0, Step &&step)
{
    static_assert(T % RT == 0, "whole steps per thread");
    const u64 base = (u64)blockIdx.x * T;
#pragma unroll
    for (int j = 0; j < T / RT; j++) {
        const u64 i = base + threadIdx.x + (u64)RT * j;
        if (i + 1 >= dp.steps) continue;
        const u32 k = dp.key[i];
        if (dp.key[i + 1] != k) continue;
        const u32 c0 = skip_pos0 ? key_c0(dp, dp.koff[k], 1) : 0u;
        step((i32)((u32)dp.cov[i] - c0), (u64)(dp.pos[i + 1] - dp.pos[i]));
    }
}

// one wavefront per region, QUERY_CHUNK regions a launch: launch(i0, grid) for the regions from i0 on
template <typename Launch>
inline void query_chunks(u64 n, Launch &&launch)
{
    for (u64 i0 = 0; i0 < n; i0 += QUERY_CHUNK) {
        const u64 m = n - i0 < QUERY_CHUNK ? n - i0 : QUERY_CHUNK;
        launch(i0, dim3((u32)((m + RW - 1) / RW)));
    }
}
// the region a wavefront of such a launch takes, the same in every lane for the compiler too: the region's bounds and the
// key's slice arrive through scalar loads and every branch on them is a scalar branch
__device__ __forceinline__ u64 query_region(u64 i0)
{
    return i0 + (u64)blockIdx.x * RW + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / IVX_WAVE));
}
