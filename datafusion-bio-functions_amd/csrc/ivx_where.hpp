// ivx_where.hpp -- overlap thresholds (include/ivx_where.h) on the device: the predicate of one matched pair, and WhereOp<Op>,
// which puts it in front of any per-row operator (ivx_rowops.hpp).  Every kernel that runs an operator -- k_probe_rows, k_lean,
// k_lean_rest -- hands hit() each row's OWN two ends: the probe row's from the input columns or as rbase + rel, rel + len of
// its packed word (a row is routed to one region, whole), the build row's from the index entry (ivx_ent, or the two words the
// slice stages of it: a build row that spans regions is an entry of each, with its own ends).  So plen and blen are the rows'
// lengths on every path, and the wrapper is written once.
#pragma once
#include "ivx_select.hpp"
#include "ivx_where.h"

// The threshold as the kernels carry it (where_pred() makes it from a checked ivx_overlap_where).  A fraction that is not
// asked is 0 / 1, which every pair with len >= 1 passes, so pass() has no branch per condition; `either` is set only when
// both fractions are asked.  Products: |len|, |plen|, |blen| <= 2^32 and num <= den <= 2^31 - 1, below 2^63.
struct WherePred {
    i64 min_bases;                  // max(1, min_bases): len >= 1 is part of every asked threshold
    u32 pn, pd, bn, bd;
    u32 either;
    u32 any;                        // 0: nothing asked, every matched pair passes (rows with end < start included)
    __host__ __device__ __forceinline__ bool pass(i32 qs, i32 qe, i32 bs, i32 be) const
    {
        if (!any) return true;
        const i64 len = (i64)(qe < be ? qe : be) - (i64)(qs > bs ? qs : bs) + 1;
        const bool p = len * (i64)pd >= ((i64)qe - (i64)qs + 1) * (i64)pn;
        const bool b = len * (i64)bd >= ((i64)be - (i64)bs + 1) * (i64)bn;
        return (len >= min_bases) & (either ? (p | b) : (p & b));
    }
};

// nullptr: valid.  Else the text of the first rule of ivx_where.h that w breaks
inline const char *where_invalid(const ivx_overlap_where *w)
{
    if (!w) return nullptr;
    if (w->min_bases < 0) return "overlap_where: min_bases is negative";
    if (w->probe_den > 0x7FFFFFFFu || w->build_den > 0x7FFFFFFFu) return "overlap_where: a denominator exceeds 2^31 - 1";
    if ((w->probe_num && !w->probe_den) || (w->build_num && !w->build_den)) return "overlap_where: a fraction's denominator is 0";
    if (w->probe_num > w->probe_den || w->build_num > w->build_den) return "overlap_where: a fraction is above 1 (num > den)";
    if (w->either > 1u) return "overlap_where: either is 0 or 1";
    return nullptr;
}
inline bool where_asks(const ivx_overlap_where *w) { return w && (w->min_bases > 0 || w->probe_num || w->build_num); }
inline WherePred where_pred(const ivx_overlap_where *w)
{
    WherePred p{1, 0u, 1u, 0u, 1u, 0u, 0u};
    if (!where_asks(w)) return p;
    p.any = 1u;
    p.min_bases = w->min_bases > 1 ? w->min_bases : 1;
    if (w->probe_num) { p.pn = w->probe_num; p.pd = w->probe_den; }
    if (w->build_num) { p.bn = w->build_num; p.bd = w->build_den; }
    p.either = (w->probe_num && w->build_num && w->either) ? 1u : 0u;
    return p;
}

// Op behind the threshold: Op's kernel arguments, LDS, begin / enter / leave and its row's done() as they are; a match reaches
// Op::Row::hit only when the pair passes.
template <class Op>
struct WhereOp : Op {
    WherePred w;
    struct Row : Op::Row {
        template <class L>
        __device__ __forceinline__ void hit(const WhereOp &op, L &l, u32 j, i32 qs, i32 qe, i32 xs, i32 xe)
        {
            if (op.w.pass(qs, qe, xs, xe)) Op::Row::hit(op, l, j, qs, qe, xs, xe);
        }
        __device__ __forceinline__ void hit(const WhereOp &op, const ivx_ent &x, i32 qs, i32 qe)
        {
            if (op.w.pass(qs, qe, x.s, x.e)) Op::Row::hit(op, x, qs, qe);
        }
    };
};

// run(op) for the plain call, run(WhereOp<Op>) under a threshold: the choice is the host's, no kernel of the plain call changes
template <class Op, class F>
inline void with_where(const WherePred *w, const Op &op, F &&run)
{
    if (w) run(WhereOp<Op>{op, *w}); else run(op);
}

// the pair filter's decomposition (k_pairs_count / k_pairs_write, ivx_where.hip): workgroup, pairs per lane, pairs per tile
constexpr int PW_T = 256;
constexpr int PW_PI = 4;
constexpr int PW_TILE = PW_T * PW_PI;

// RvOp<RV_MATCHES> leaves its count in the row's packed word, which only the region path has.  On the direct walk the same
// count goes to the call's columns: per_row[i] and / or exists[i] (null: not wanted).
struct MatchOut : RowOpBase {
    u32 *per_row; u8 *exists;
    struct Row {
        u32 v = 0;
        __device__ __forceinline__ void hit(const MatchOut &, const Lds &, u32, i32, i32, i32, i32) { v++; }
        __device__ __forceinline__ void hit(const MatchOut &, const ivx_ent &, i32, i32) { v++; }
        __device__ __forceinline__ void done(const MatchOut &op, const u64 *, u64 at, u32) const
        {
            if (op.per_row) op.per_row[at] = v;
            if (op.exists) op.exists[at] = v != 0u;
        }
    };
};
