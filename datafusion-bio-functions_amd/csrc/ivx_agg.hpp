// ivx_agg.hpp -- device pieces shared by the overlap-aggregate kernels (ivx_agg.hip: the direct walk; ivx_regions_probe.hip:
// k_agg_fast / k_agg_rest): what one probe row accumulates over its matches, and its store into a set of output columns
// (AggOut, ivx_internal.hpp: the caller's columns by row, or the region path's records by pool index).
#pragma once
#include "ivx_join.hpp"

// the value of build row `row`, sign-extended (VB: bytes of a value, 4 or 8)
template <int VB>
__device__ __forceinline__ i64 agg_val(const void *__restrict__ val, u32 row)
{
    return VB == 4 ? (i64)((const i32 *)val)[row] : ((const i64 *)val)[row];
}

// One probe row's aggregates.  MM: min / max wanted; WT: bases / wsum wanted (the only two that need the coordinates).
// Sums wrap: unsigned arithmetic, stored as int64.  len = min(qe, be) - max(qs, bs) + 1 in 64 bits, unclamped.
template <bool MM, bool WT>
struct AggAcc {
    u32 c = 0;
    u64 s = 0, b = 0, w = 0;
    i64 lo = INT64_MAX, hi = INT64_MIN;
    __device__ __forceinline__ void add(i64 v, i32 qs, i32 qe, i32 bs, i32 be)
    {
        c++;
        s += (u64)v;
        if (MM) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
        if (WT) {
            const u64 len = (u64)((i64)(qe < be ? qe : be) - (i64)(qs > bs ? qs : bs) + 1);
            b += len;
            w += (u64)v * len;
        }
    }
    __device__ __forceinline__ void store(const AggOut &o, u64 i) const
    {
        if (o.count) o.count[i] = c;
        if (o.sum) o.sum[i] = (i64)s;
        if (MM) { if (o.vmin) o.vmin[i] = lo; if (o.vmax) o.vmax[i] = hi; }
        if (WT) { if (o.bases) o.bases[i] = (i64)b; if (o.wsum) o.wsum[i] = (i64)w; }
    }
};
