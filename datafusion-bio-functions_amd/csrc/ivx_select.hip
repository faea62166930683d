// ivx_select.hip -- overlap select: per probe row, over exactly the build rows ivx_probe_overlap_fill pairs it with, the one
// build row that is best by a criterion -- the smallest or largest value of a build-side column, the longest or shortest
// overlap, the first or last row -- and, if wanted, the criterion's value there (ivx_probe_overlap_select; a left join to
// at most one row, bedtools map -o first / last, SQL's ROW_NUMBER() ... = 1 over the range join).  No pair is ever written.
//
// This file is the direct path: SelOp (ivx_select.hpp) on k_probe_rows (ivx_rowops.hpp).  Any index, any batch size; what
// small batches take, and what every batch takes whose index is not lean.  (Big batches over a lean index: the same operator
// on k_lean / k_lean_rest in ivx_regions_probe.hip.)
//
// A row without a match stores IVX_NULL_IDX and score 0.
#include "ivx_where.hpp"

ivx_status ivx_sel_probe(ivx_ctx *ctx, const JoinIndexView &jv, const u32 *key, const i32 *s, const i32 *e, u64 n,
                         const void *val, u32 val_bytes, int by, const SelOut &out, const WherePred *w)
{
    ivx_status st = IVX_OK;
    sel_dispatch(by, val_bytes, out.score != nullptr, [&](auto b, auto vb, auto sc) {
        with_where(w, SelOp<decltype(b)::value, decltype(vb)::value, decltype(sc)::value>{{}, val, out}, [&](const auto &op) { st = ivx_direct_probe(ctx, jv, key, s, e, n, op); });
    });
    return st;
}
