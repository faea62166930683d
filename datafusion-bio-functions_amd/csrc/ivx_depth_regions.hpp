// ivx_depth_regions.hpp -- what the two region kernels' files share (ivx_depth_regions.hip: sums and threshold counts;
// ivx_depth_rank.hip: min, max and quantiles): where a region's key and bounds come from, the per-key c0, and the
// wavefront search inside a key's slice of the step list.
#pragma once
#include "ivx_device.hpp"

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
