// ivx_select.hpp -- device pieces shared by the overlap-select kernels (ivx_select.hip: the direct walk;
// ivx_regions_probe.hip: k_sel_fast / k_sel_rest): the criterion value of one match, the best match one probe row has seen
// so far, and its store into the output columns (SelOut, ivx_internal.hpp: the caller's columns by row, or the region
// path's records by pool index).
#pragma once
#include <type_traits>
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
