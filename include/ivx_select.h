/*
 * ivx_select.h -- companion header of ivx.h: overlap select, the ONE best build row per probe row.
 *
 * Conventions, types, status codes and the meaning of `mem` are those of ivx.h.  The entry lives in libivx_hip.so like
 * every other; it has a header of its own until it is folded into ivx.h and the entry catalogue ("Overlap
 * select").
 */
#ifndef IVX_SELECT_H
#define IVX_SELECT_H

#include "ivx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a3'''': overlap select -- join on overlap and keep, per probe row, the one build row that is best by a criterion ("assign
 *      each read to the gene it overlaps most", "the highest-scoring feature under each target", bedtools map -o first /
 *      last, SQL's ROW_NUMBER() OVER (PARTITION BY probe ORDER BY ...) = 1 over the range join) without ever writing a pair.
 *      The reference has no counterpart; the contract is stated against the join's own pairs.  Index kind OVERLAP.
 *      M(i) is exactly what ivx_probe_overlap_agg defines: the build rows ivx_probe_overlap_fill pairs with probe row i for
 *      the same (already adjusted) columns.  len(b, i) = min(qe, be) - max(qs, bs) + 1 in int64, not clamped.  The
 *      criterion value c(b, i):
 *        IVX_SEL_MIN_VAL, IVX_SEL_MAX_VAL            val[b], sign-extended from val_bytes = 4 (int32) or 8 (int64); `val` has
 *                                                    ivx_index_rows(ix) elements and lives where `mem` says
 *        IVX_SEL_MAX_OVERLAP, IVX_SEL_MIN_OVERLAP    len(b, i)
 *        IVX_SEL_FIRST_ROW, IVX_SEL_LAST_ROW         b
 *      The winner is the b in M(i) with the smallest (MIN_*, FIRST_ROW) or largest (MAX_*, LAST_ROW) c; ties go to the
 *      smallest build row.  That is a total order: the result does not depend on the path taken or on the order the index
 *      is walked in.  One element per probe row, in input order:
 *        build_idx[i] = the winner, or IVX_NULL_IDX when M(i) is empty      (what ivx_take_* take as a row index)
 *        score[i]     = c(winner, i), or 0 when M(i) is empty               (NULL: not wanted, neither computed nor stored)
 *      IVX_ERR_INVALID: build_idx = NULL; `by` outside 0 .. IVX_SEL_N - 1; for the two *_VAL criteria val_bytes other than
 *      4 or 8, or val = NULL with a non-empty index (for the other four val and val_bytes are ignored and nothing of val is
 *      read).  Another index kind: IVX_ERR_UNSUPPORTED.  A refused call writes nothing.  n = 0 is a no-op.
 *      The call waits for an index whose build tail still runs, drops the state a count call left for its fill call, and
 *      feeds ivx_ctx_metrics like ivx_probe_overlap_agg: one input batch, n input and n output rows. */
enum { IVX_SEL_MIN_VAL = 0, IVX_SEL_MAX_VAL = 1, IVX_SEL_MAX_OVERLAP = 2, IVX_SEL_MIN_OVERLAP = 3,
       IVX_SEL_FIRST_ROW = 4, IVX_SEL_LAST_ROW = 5, IVX_SEL_N = 6 };
ivx_status ivx_probe_overlap_select(ivx_ctx *ctx, const ivx_index *ix, int mem,
                                    const uint32_t *key, const int32_t *start, const int32_t *end, uint64_t n,
                                    const void *val /* nullable */, uint32_t val_bytes, int by,
                                    uint32_t *build_idx, int64_t *score /* nullable */);

#ifdef __cplusplus
}
#endif

#endif /* IVX_SELECT_H */
