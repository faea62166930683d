/*
 * ivx_where.h -- companion header of ivx.h, beside ivx_select.h: overlap thresholds.  A minimum number of shared bases and
 * minimum overlap fractions of the probe row and of the build row (bedtools intersect -f / -F / -r / -e, minoverlap in
 * GenomicRanges, SQL's residual filter beside the range join), on every per-row probe and as a stable filter of the
 * join's pairs.
 *
 * Conventions, types, status codes and the meaning of `mem` are those of ivx.h.  The entries live in libivx_hip.so like
 * every other; they have a header of their own until they are folded into ivx.h and the entry catalogue (DESIGN.md,
 * "Overlap thresholds").
 */
#ifndef IVX_WHERE_H
#define IVX_WHERE_H

#include "ivx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The threshold.  For a pair of build row b = (bs, be) and probe row i = (qs, qe) that the join matches (same key,
 * bs <= qe && be >= qs), on the already adjusted columns, all in int64:
 *     len  = min(qe, be) - max(qs, bs) + 1
 *     plen = qe - qs + 1
 *     blen = be - bs + 1
 * If nothing is asked every matched pair passes.  Otherwise a pair passes iff
 *     len >= 1                                   (a pair that exists only because a row has end < start never passes),
 *     min_bases holds when it is asked, and
 *     the fractions asked hold: both when both are asked and either = 0, one of them when both are asked and either = 1.
 * Comparisons are exact integers: with num <= den <= 2^31 - 1 and |len|, |plen|, |blen| <= 2^32 every product is below
 * 2^63 in magnitude and fits int64.  There are no float fractions at this boundary.
 * IVX_ERR_INVALID, each with its own text: min_bases < 0; num > den; den == 0 with num > 0; den > 2^31 - 1; either not
 * 0 or 1.  (A fraction that is not asked, num == 0, may have any den up to 2^31 - 1, 0 included.) */
typedef struct ivx_overlap_where {
    int64_t  min_bases;              /* asked iff > 0:           len >= min_bases                      */
    uint32_t probe_num, probe_den;   /* asked iff probe_num > 0: len * probe_den >= plen * probe_num   */
    uint32_t build_num, build_den;   /* asked iff build_num > 0: len * build_den >= blen * build_num   */
    uint32_t either;                 /* both fractions asked: 0 = both must hold (-f -F, -r), 1 = one suffices (-e) */
} ivx_overlap_where;

/* M_w(i) is the set of build rows that ivx_probe_overlap_fill pairs with probe row i and that pass w.  Every entry below
 * with w == NULL, or a w that asks nothing, gives its unfiltered counterpart's result bit for bit, rows with end < start
 * included.  Everything not said here is the unfiltered counterpart's: index kind OVERLAP (another: IVX_ERR_UNSUPPORTED),
 * the null-key rule, n = 0 as a no-op, the wait for a build tail, the dropped join plan, the metrics, device-mode stream
 * ordering, and a reservation refused under a memory limit leaving the outputs untouched. */

/* per_row[i] = |M_w(i)|, exists[i] = |M_w(i)| != 0, *total = the sum of per_row in 64 bits (a device reduction).  Each
 * output is nullable; all three NULL: IVX_ERR_INVALID.  Counterparts: ivx_probe_overlap_count / ivx_probe_exists. */
ivx_status ivx_probe_overlap_count_where(ivx_ctx *ctx, const ivx_index *ix, int mem,
                                         const uint32_t *key, const int32_t *start, const int32_t *end, uint64_t n,
                                         const ivx_overlap_where *w /* nullable */,
                                         uint32_t *per_row /* nullable */, uint8_t *exists /* nullable */, uint64_t *total /* nullable */);

/* ivx_probe_mark_build over M_w: bit b of `marks` is ORed when some probe row i has b in M_w(i). */
ivx_status ivx_probe_mark_build_where(ivx_ctx *ctx, const ivx_index *ix, int mem,
                                      const uint32_t *key, const int32_t *start, const int32_t *end, uint64_t n,
                                      const ivx_overlap_where *w /* nullable */, uint32_t *marks);

/* ivx_probe_overlap_agg with M_w(i) in place of M(i). */
ivx_status ivx_probe_overlap_agg_where(ivx_ctx *ctx, const ivx_index *ix, int mem,
                                       const uint32_t *key, const int32_t *start, const int32_t *end, uint64_t n,
                                       const void *val, uint32_t val_bytes, const ivx_overlap_where *w /* nullable */,
                                       uint32_t *count, int64_t *sum, int64_t *vmin, int64_t *vmax, int64_t *bases, int64_t *wsum);

/* ivx_probe_overlap_select over M_w(i). */
ivx_status ivx_probe_overlap_select_where(ivx_ctx *ctx, const ivx_index *ix, int mem,
                                          const uint32_t *key, const int32_t *start, const int32_t *end, uint64_t n,
                                          const void *val /* nullable */, uint32_t val_bytes, int by,
                                          const ivx_overlap_where *w /* nullable */,
                                          uint32_t *build_idx, int64_t *score /* nullable */);

/* A stable filter of pairs: the pairs (build_idx[j], probe_idx[j]) of the input that pass w, in input order, computed from
 * the coordinates alone (bstart / bend: nb build rows; pstart / pend: np probe rows; the columns the join was given).
 * *n_out = the pairs that pass.  cap = 0 with NULL outputs only counts; cap < *n_out: IVX_ERR_CAPACITY with *n_out set to
 * the size needed and nothing written.  An index >= nb or >= np (IVX_NULL_IDX is one): IVX_ERR_INVALID, found on the
 * device before anything is gathered, nothing written.  An output that overlaps an input or the other output:
 * IVX_ERR_INVALID.  w == NULL or a w that asks nothing: every pair passes (the indexes are still checked). */
ivx_status ivx_pairs_where(ivx_ctx *ctx, int mem,
                           const uint32_t *build_idx, const uint32_t *probe_idx, uint64_t n_pairs,
                           const int32_t *bstart, const int32_t *bend, uint64_t nb,
                           const int32_t *pstart, const int32_t *pend, uint64_t np,
                           const ivx_overlap_where *w /* nullable */,
                           uint32_t *out_build, uint32_t *out_probe, uint64_t cap, uint64_t *n_out);

#ifdef __cplusplus
}
#endif

#endif /* IVX_WHERE_H */
