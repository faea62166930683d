// ivx_select.hpp -- overlap select as a per-row operator (ivx_rowops.hpp; ivx_select.hip runs it on the direct walk,
// ivx_regions_probe.hip on the lean kernels): the criterion value of one match, the best match one probe row has seen so far,
// and its store into the output columns (SelOut, ivx_internal.hpp: the caller's columns by row, or the region path's records
// by pool index).
#pragma once
#include "ivx_agg.hpp"

// BY: an IVX_SEL_* criterion (include/ivx_select.h)
template <int BY> constexpr bool sel_by_val = BY == IVX_SEL_MIN_VAL || BY == IVX_SEL_MAX_VAL;
template <int BY> constexpr bool sel_by_len = BY == IVX_SEL_MAX_OVERLAP || BY == IVX_SEL_MIN_OVERLAP;
template <int BY> constexpr bool sel_largest = BY == IVX_SEL_MAX_VAL || BY == IVX_SEL_MAX_OVERLAP || BY == IVX_SEL_LAST_ROW;

// c(b, i): v is val[b] (read only by the *_VAL criteria), the coordinates give the overlap's length, unclamped in 64 bits
template <int BY>
__device__ __forceinline__ i64 sel_crit(i64 v, u32 row, i32 qs, i32 qe, i32 bs, i32 be)
{
    if (sel_by_val<BY>) return v;
    if (sel_by_len<BY>) return (i64)(qe < be ? qe : be) - (i64)(qs > bs ? qs : bs) + 1;
    return (i64)row;
}

// A call's criterion, value width and "score wanted" as template arguments: f(tag of BY, tag of VB, tag of SCORE).  The four
// criteria that read no value have one form (VB = 4, never used).
template <class F>
inline void sel_dispatch(int by, u32 val_bytes, bool score, F &&f)
{
    auto with_score = [&](auto b, auto vb) { if (score) f(b, vb, std::true_type{}); else f(b, vb, std::false_type{}); };
    auto with_width = [&](auto b) {
        if (val_bytes == 8) with_score(b, std::integral_constant<int, 8>{}); else with_score(b, std::integral_constant<int, 4>{});
    };
    switch (by) {
    case IVX_SEL_MIN_VAL: with_width(std::integral_constant<int, IVX_SEL_MIN_VAL>{}); break;
    case IVX_SEL_MAX_VAL: with_width(std::integral_constant<int, IVX_SEL_MAX_VAL>{}); break;
    case IVX_SEL_MAX_OVERLAP: with_score(std::integral_constant<int, IVX_SEL_MAX_OVERLAP>{}, std::integral_constant<int, 4>{}); break;
    case IVX_SEL_MIN_OVERLAP: with_score(std::integral_constant<int, IVX_SEL_MIN_OVERLAP>{}, std::integral_constant<int, 4>{}); break;
    case IVX_SEL_FIRST_ROW: with_score(std::integral_constant<int, IVX_SEL_FIRST_ROW>{}, std::integral_constant<int, 4>{}); break;
    default: with_score(std::integral_constant<int, IVX_SEL_LAST_ROW>{}, std::integral_constant<int, 4>{}); break;
    }
}

// One probe row's winner.  "None yet" is kept in the row (IVX_NULL_IDX), never in the value: INT64_MIN under MAX_VAL,
// INT64_MAX under MIN_VAL and row 0 under LAST_ROW are legal winners.  (c, row) compare lexicographically, ties on c go to
// the smaller row: a total order, so the walk's order does not show.  SCORE: the criterion value is stored as well.
template <int BY, bool SCORE>
struct SelAcc {
    u32 row = IVX_NULL_IDX;
    i64 c = 0;                                                          // (0: the score of a row without a match)
    __device__ __forceinline__ void add(i64 v, u32 b)
    {
        const bool better = sel_largest<BY> ? v > c : v < c;
        if (row == IVX_NULL_IDX || better || (v == c && b < row)) { c = v; row = b; }
    }
    __device__ __forceinline__ void store(const SelOut &o, u64 i) const
    {
        o.idx[i] = row;
        if (SCORE) o.score[i] = c;
    }
};

// The result names a build row, so k_lean stages the slice's build ROW IDS when a region is entered, row[j] = the row of slice
// entry j, and for the two *_VAL criteria the values as AggOp does (24 KB of LDS more than the slice alone, 48 or 72 KB with
// values: one 1024-thread workgroup per CU either way).  (winner, score) go to out.idx[at], and out.score[at] when wanted: on
// the region path a record, as the aggregates'.
template <int BY, int VB, bool SCORE>
struct SelOp : RowOpBase {
    using VT = typename std::conditional<VB == 4, i32, i64>::type;
    static constexpr bool VAL = sel_by_val<BY>;
    const void *val; SelOut out;
    struct RowsVals { u32 row[RP_ECAP]; VT val[RP_ECAP]; };
    struct Rows { u32 row[RP_ECAP]; };
    using Lds = typename std::conditional<VAL, RowsVals, Rows>::type;
    // (the slice load's first barrier: nobody reads the old rows and values any more)
    template <class S> __device__ __forceinline__ void enter(const JoinIndexView &ix, const S &sl, u32 r, Lds &l) const
    {
        slice_rows(ix, sl, r, [&](u32 j, u32 row) { l.row[j] = row; if constexpr (VAL) l.val[j] = ((const VT *)val)[row]; });
    }
    struct Row : SelAcc<BY, SCORE> {
        __device__ __forceinline__ void hit(const SelOp &, const Lds &l, u32 j, i32 qs, i32 qe, i32 xs, i32 xe)
        {
            const u32 row = l.row[j];
            i64 v = 0;
            if constexpr (VAL) v = (i64)l.val[j];
            this->add(sel_crit<BY>(v, row, qs, qe, xs, xe), row);
        }
        __device__ __forceinline__ void hit(const SelOp &op, const ivx_ent &x, i32 qs, i32 qe)
        {
            this->add(sel_crit<BY>(VAL ? agg_val<VB>(op.val, x.row) : 0, x.row, qs, qe, x.s, x.e), x.row);
        }
        __device__ __forceinline__ void done(const SelOp &op, const u64 *, u64 at, u32) const { this->store(op.out, at); }
    };
};
