// ivx_agg.hpp -- the overlap aggregates as a per-row operator (ivx_rowops.hpp; ivx_agg.hip runs it on the direct walk,
// ivx_regions_probe.hip on the lean kernels): what one probe row accumulates over its matches, and its store into a set of
// output columns (AggOut, ivx_internal.hpp: the caller's columns by row, or the region path's records by pool index).
#pragma once
#include <type_traits>
#include "ivx_rowops.hpp"

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

// VB: bytes of a value.  k_lean stages the slice's VALUES in LDS when a region is entered, val[j] = the value of slice entry
// j's build row, so its candidate loop reads LDS only; the other two kernels gather the value per match.  A row's result is
// up to 44 bytes and does not fit its packed word: it goes to out.*[at] -- on the region path a RECORD, one scratch array per
// wanted output indexed like the page pool, so a wavefront's stores are as contiguous as its row loads.
template <int VB, bool MM, bool WT>
struct AggOp : RowOpBase {
    using VT = typename std::conditional<VB == 4, i32, i64>::type;
    const void *val; AggOut out;
    struct Lds { VT val[RP_ECAP]; };
    // (the slice load's first barrier: nobody reads the old values any more)
    template <class S> __device__ __forceinline__ void enter(const JoinIndexView &ix, const S &sl, u32 r, Lds &l) const
    {
        slice_rows(ix, sl, r, [&](u32 j, u32 row) { l.val[j] = ((const VT *)val)[row]; });
    }
    struct Row : AggAcc<MM, WT> {
        __device__ __forceinline__ void hit(const AggOp &, const Lds &l, u32 j, i32 qs, i32 qe, i32 xs, i32 xe) { this->add((i64)l.val[j], qs, qe, xs, xe); }
        __device__ __forceinline__ void hit(const AggOp &op, const ivx_ent &x, i32 qs, i32 qe) { this->add(agg_val<VB>(op.val, x.row), qs, qe, x.s, x.e); }
        __device__ __forceinline__ void done(const AggOp &op, const u64 *, u64 at, u32) const { this->store(op.out, at); }
    };
};
