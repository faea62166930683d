/*
 * ivx_nearest.h -- companion header of ivx.h, beside ivx_select.h and ivx_where.h: nearest on one side only and / or within a
 * distance cap.
 *
 * Conventions, types, status codes and the meaning of `mem` are those of ivx.h.  The entry lives in libivx_hip.so like
 * every other; it has a header of its own until it is folded into ivx.h and the entry catalogue ("Directional
 * and distance-capped nearest").
 */
#ifndef IVX_NEAREST_H
#define IVX_NEAREST_H

#include "ivx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a6': ivx_probe_nearest restricted to one side of the probe row and / or to build rows within max_distance ("the gene
 *      upstream of each peak", "the nearest TSS if it is within 10 kb, else nothing", "every feature within D": bedtools
 *      closest -iu / -id, bedtools window, pyranges nearest(how=...), GenomicRanges precede / follow).  Index kind NEAREST.
 *      Everything is stated against the reference's own algorithm (nearest_index.rs:91-235, nearest.rs:330-456), which
 *      ivx_probe_nearest reproduces.  The candidate stream of a probe row is the one nearest_k produces for the
 *      strict-adjusted query [qs, qe]:
 *        first, if include_overlaps, the overlapping rows in (start, end, row) order;
 *        then the two cursors -- left: by_end, going down from partition_point(last < qs); right: by_start, going up from
 *        partition_point(first <= qe) -- their heads merged by cmp_candidate (left before right at equal distance; among
 *        left candidates of equal end the larger start first, then the larger row; right candidates in (start, end, row)
 *        order), candidates at distance 0 skipped when !include_overlaps, rows already taken skipped.
 *      IVX_NEAR_BEFORE is that stream with the right cursor empty from the start, IVX_NEAR_AFTER with the left cursor empty
 *      from the start.  Direction does not touch the overlap stage: include_overlaps alone decides it (precede / follow is
 *      include_overlaps = 0, bedtools -iu / -id is include_overlaps = 1).
 *      max_distance = D >= 0: a cursor whose next candidate's REPORTED distance (candidate_distance on the raw probe
 *      coordinates, nearest.rs:367-374) exceeds D counts as exhausted.  Along one cursor that distance never decreases for a
 *      probe row with start <= end, so this is "drop every candidate farther than D", and a row with a small D does not walk
 *      its whole key.  Overlaps have distance 0 and always pass; under `strict` a touching row has raw distance 0 and passes
 *      D = 0.  max_distance < 0: no cap.
 *      The answer is the first k of that stream; k = 1 follows nearest_one (the first overlap if asked for and present, else
 *      the head of the cursor(s), else NULL); k = 0 gives one NULL row per probe row.
 *      Output shape, `cap`, `rows` and IVX_ERR_CAPACITY are those of ivx_probe_nearest: max(1, found) rows per probe row in
 *      probe order, IVX_NULL_IDX / -1 for a row without an answer.  direction = IVX_NEAR_ANY with max_distance < 0 IS
 *      ivx_probe_nearest, bit for bit, on every path.
 *      IVX_ERR_INVALID: direction outside 0 .. IVX_NEAR_N - 1; a NULL build_idx / probe_idx / rows.  Another index kind:
 *      IVX_ERR_UNSUPPORTED.  A refused call writes nothing.  n = 0 is a no-op.  Metrics and stream behaviour are those of
 *      ivx_probe_nearest. */
enum { IVX_NEAR_ANY = 0, IVX_NEAR_BEFORE = 1, IVX_NEAR_AFTER = 2, IVX_NEAR_N = 3 };
ivx_status ivx_probe_nearest_dir(ivx_ctx *ctx, const ivx_index *ix, int mem,
                                 const uint32_t *key, const int32_t *start, const int32_t *end, uint64_t n,
                                 int strict, uint32_t k, int include_overlaps,
                                 int direction, int64_t max_distance /* < 0: no cap */,
                                 uint32_t *build_idx, uint32_t *probe_idx, int64_t *distance /* nullable */,
                                 uint64_t cap, uint64_t *rows);

#ifdef __cplusplus
}
#endif

#endif /* IVX_NEAREST_H */
