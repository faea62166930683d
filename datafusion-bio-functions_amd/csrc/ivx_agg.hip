// ivx_agg.hip -- overlap aggregates: per probe row, over exactly the build rows ivx_probe_overlap_fill pairs it with, the
// count, sum, min and max of a build-side value column, the overlapped bases and the bases-weighted sum
// (ivx_probe_overlap_agg; SQL's GROUP BY probe row over the join, bedtools map).  No pair is ever written.
//
// This file is the direct path: AggOp (ivx_agg.hpp) on k_probe_rows (ivx_rowops.hpp), val[row] gathered per match.  Any
// index, any batch size; what small batches take, and what every batch takes whose index is not lean.  (Big batches over a
// lean index: the same operator on k_lean / k_lean_rest in ivx_regions_probe.hip.)
//
// A row without a match stores count 0, sum 0, bases 0, wsum 0 and the identities INT64_MAX / INT64_MIN for min / max.
#include "ivx_where.hpp"

ivx_status ivx_agg_probe(ivx_ctx *ctx, const JoinIndexView &jv, const u32 *key, const i32 *s, const i32 *e, u64 n,
                         const void *val, u32 val_bytes, const AggOut &out, const WherePred *w)
{
    ivx_status st = IVX_OK;
    with_bools([&](auto wide, auto mm, auto wt) {
        with_where(w, AggOp<IVX_B(wide) ? 8 : 4, IVX_B(mm), IVX_B(wt)>{{}, val, out}, [&](const auto &op) { st = ivx_direct_probe(ctx, jv, key, s, e, n, op); });
    }, val_bytes == 8, out.vmin || out.vmax, out.bases || out.wsum);
    return st;
}
