/*
 * bio_ranges_host.h -- host-side mirror of the reference's operator interface over the
 * Arrow C Data Interface (libbio_ranges_hip.so, plain C++; no Arrow library needed).
 *
 * The reference's operators take Arrow RecordBatches and column-name triples
 * (contig, start, end); this layer does what their host code does before and after
 * the hot loop, then calls the HIP kernels through include/ivx.h:
 *   - contig column access: Utf8 / LargeUtf8 / Utf8View   (R/src/array_utils.rs:10-24, :196-229)
 *   - position columns: Int32 / Int64 / UInt32 / UInt64, null check and checked
 *     narrowing with the reference's error text            (array_utils.rs:33-172, :231-295)
 *   - key dictionary: contig (or several key columns) -> dense uint32 ids, assigned in
 *     byte order of the names so merge/subtract emit groups like
 *     StreamCollector::take_groups                          (R/src/grouped_stream.rs:105-113)
 *   - output columns as Arrow arrays (count/coverage Int64; UInt32 index arrays with
 *     validity for nearest; Utf8 + Int64 columns for merge/subtract).
 * Gathering payload columns with the returned index arrays (`compute::take`) stays with
 * the caller, exactly as in the reference (interval_join.rs:1655-1667, nearest.rs:469-482).
 *
 * Every function returns 0 on success; brh_last_error() gives the message
 * (DataFusionError::Execution text).  Input batches are borrowed, outputs are
 * released by the caller through the usual ArrowArray.release callback.
 */
#ifndef BIO_RANGES_HOST_H
#define BIO_RANGES_HOST_H
#include <stdint.h>
#include "ivx.h"   /* ivx_metrics */
#ifdef __cplusplus
extern "C" {
#endif

#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
struct ArrowSchema {
    const char *format; const char *name; const char *metadata; int64_t flags; int64_t n_children;
    struct ArrowSchema **children; struct ArrowSchema *dictionary;
    void (*release)(struct ArrowSchema *); void *private_data;
};
struct ArrowArray {
    int64_t length; int64_t null_count; int64_t offset; int64_t n_buffers; int64_t n_children;
    const void **buffers; struct ArrowArray **children; struct ArrowArray *dictionary;
    void (*release)(struct ArrowArray *); void *private_data;
};
#endif

typedef struct brh_session brh_session;

/* one table = one struct-typed ArrowArray + its ArrowSchema (RecordBatch export) */
typedef struct { const struct ArrowArray *array; const struct ArrowSchema *schema; } brh_batch;

/* column names: keys[0..n_keys) are the equi-key columns (the contig; more for multi-column
 * joins such as contig+strand, R/tests/integration_test.rs:393-397), then start and end */
typedef struct { const char *const *keys; int n_keys; const char *start; const char *end; } brh_columns;

int  brh_session_create(int device_ordinal, brh_session **out);      /* fails without a gfx950 device */
void brh_session_free(brh_session *s);
const char *brh_last_error(const brh_session *s);

/* FilterOp (R/src/filter_op.rs:4-10) */
enum { BRH_WEAK = 0, BRH_STRICT = 1 };
/* JoinType.  The first three are the subset with real semantics in IntervalJoinExec (interval_join.rs:1014-1024); for the
 * types from BRH_JOIN_LEFT_SEMI on the reference emits the Inner rows -- here they mean what SQL (and HashJoinExec, with its
 * visited_left_side bitmap) means by them, over the build side's match marks (ivx.h ivx_probe_mark_build).  `build` is
 * the SQL left side throughout. */
enum { BRH_JOIN_INNER = 0, BRH_JOIN_RIGHT_SEMI = 1, BRH_JOIN_RIGHT_ANTI = 2,
       BRH_JOIN_NEAREST = 3 /* join stream only: Inner with Algorithm::CoitreesNearest (interval_join.rs:864-870) */,
       BRH_JOIN_LEFT_SEMI = 4,  /* the build rows with a match */
       BRH_JOIN_LEFT_ANTI = 5,  /* the build rows without one */
       BRH_JOIN_LEFT = 6,       /* the pairs, then every unmatched build row with a NULL probe_idx */
       BRH_JOIN_RIGHT = 7,      /* the pairs, then every unmatched probe row with a NULL build_idx */
       BRH_JOIN_FULL = 8        /* both */ };
#define BRH_MAX_OUTPUT_ENV UINT64_MAX   /* join stream: take the output budget from BIO_MAX_OUTPUT_BATCH_SIZE (default 100000) */

/* count_overlaps('left','right') / coverage(...): CountOverlapsProvider (R/src/count_overlaps.rs:107-169),
 * get_count_stream / get_stream (interval_tree.rs:155-280).  `left` is indexed, `right` streamed;
 * out = the Int64 column ("count"/"coverage") to append to `right`. */
int brh_count_overlaps(brh_session *s, brh_batch left, brh_columns lcols, brh_batch right, brh_columns rcols,
                       int filter_op, int coverage, struct ArrowArray *out, struct ArrowSchema *out_schema);

/* nearest('left','right',k,overlap,compute_distance): NearestProvider / get_nearest_stream
 * (R/src/nearest.rs:127-166, :266-496).  Outputs: left_idx UInt32 (nullable), right_idx UInt32,
 * distance Int64 (nullable; NULL pointers when compute_distance == 0). */
int brh_nearest(brh_session *s, brh_batch left, brh_columns lcols, brh_batch right, brh_columns rcols,
                int filter_op, uint32_t k, int include_overlaps, int compute_distance,
                struct ArrowArray *left_idx, struct ArrowSchema *left_idx_schema,
                struct ArrowArray *right_idx, struct ArrowSchema *right_idx_schema,
                struct ArrowArray *distance, struct ArrowSchema *distance_schema);

/* nearest on one side only and / or within a distance cap (ivx_nearest.h ivx_probe_nearest_dir): brh_nearest plus
 * direction = BRH_NEAR_ANY | BRH_NEAR_BEFORE (only left rows that end before the right row: "upstream") | BRH_NEAR_AFTER
 * (only left rows that start after it: "downstream") and max_distance (< 0: no cap; else no left row farther than that is
 * an answer, and a right row without one gets the NULL row).  Direction does not touch overlapping rows: include_overlaps
 * alone decides them.  BRH_NEAR_ANY with max_distance < 0 is brh_nearest.  Another direction is refused. */
enum { BRH_NEAR_ANY = 0, BRH_NEAR_BEFORE = 1, BRH_NEAR_AFTER = 2 };
int brh_nearest_dir(brh_session *s, brh_batch left, brh_columns lcols, brh_batch right, brh_columns rcols,
                    int filter_op, uint32_t k, int include_overlaps, int compute_distance, int direction, int64_t max_distance,
                    struct ArrowArray *left_idx, struct ArrowSchema *left_idx_schema,
                    struct ArrowArray *right_idx, struct ArrowSchema *right_idx_schema,
                    struct ArrowArray *distance, struct ArrowSchema *distance_schema);

/* IntervalJoinExec (interval_join.rs:442-550, :1418-1677): `build` is the SQL join's left side.
 * strict_predicate = the planner's `<`/`>` rewrite: both sides' END minus one (intervals.rs:85-115).
 * nearest_algorithm != 0 = Algorithm::CoitreesNearest (one row per probe row, NULL build index when
 * nothing is found).  Inner: (build_idx, probe_idx); RightSemi/RightAnti: probe_idx only
 * (build_idx output left released/empty).
 * LeftSemi/LeftAnti: build_idx only, ascending (probe_idx empty): one ivx_probe_mark_build and one ivx_bits_select, no
 * pairs are made.  Right / Left / Full: the Inner pairs first, then the NULL-extended rows -- Right / Full: the probe rows
 * without a match (from ivx_probe_exists) with a NULL build_idx; Left / Full: the build rows without a match
 * (ivx_bits_mark over the filled build_idx, ivx_bits_select of the clear bits) with a NULL probe_idx.  NULL is the
 * validity buffer of a nullable UInt32 column, as the nearest join produces it (the slot's value is 0).  Pair order
 * stays unspecified; the only promise is that the NULL-extended rows follow the pairs (Full: probe rows, then build rows). */
int brh_interval_join(brh_session *s, brh_batch build, brh_columns bcols, brh_batch probe, brh_columns pcols,
                      int join_type, int strict_predicate, int nearest_algorithm,
                      struct ArrowArray *build_idx, struct ArrowSchema *build_idx_schema,
                      struct ArrowArray *probe_idx, struct ArrowSchema *probe_idx_schema);

/* Overlap aggregates: join `probe` to `build` on overlap (same keys, closed intervals), group by probe row and aggregate the
 * build side's `value_column` -- SELECT p.*, COUNT(*), SUM(b.v), MIN(b.v), MAX(b.v) ... GROUP BY the probe row, bedtools map,
 * the mean of a signal track over targets -- in one ivx_probe_overlap_agg call: no pair is ever made.  The reference has no
 * counterpart.  Tables and strict_predicate as in brh_interval_join (end - 1 on both sides; bases and wsum are computed on
 * the adjusted coordinates).
 * The value column is Int8 .. Int64 or UInt8 .. UInt32, widened to int32 or int64 on the host; UInt64, floats (their sums
 * would not be bit-reproducible) and value columns with nulls are refused, each with its own message.
 * ops: a non-empty set of BRH_AGG_* bits.  out / out_schema: arrays of BRH_AGG_N slots in the order of the bits; the slot of
 * an op that was not asked for stays released (zeroed).  Every output is an Int64 column with one value per probe row, in
 * probe order: count (matches) and bases (sum over the matches of the closed overlap length) are non-null, 0 without a match;
 * sum, min, max and wsum (sum of value * overlap length) are NULL where count is 0, as in SQL over a left join.  Sums wrap
 * in int64. */
enum { BRH_AGG_COUNT = 1, BRH_AGG_SUM = 2, BRH_AGG_MIN = 4, BRH_AGG_MAX = 8, BRH_AGG_BASES = 16, BRH_AGG_WSUM = 32,
       BRH_AGG_ALL = 63, BRH_AGG_N = 6 };
int brh_overlap_aggregate(brh_session *s, brh_batch build, brh_columns bcols, const char *value_column,
                          brh_batch probe, brh_columns pcols, int strict_predicate, uint32_t ops,
                          struct ArrowArray *out, struct ArrowSchema *out_schema);

/* Overlap select: join `probe` to `build` on overlap and keep, per probe row, the ONE build row that is best by `by` -- "assign
 * each read to the gene it overlaps most", the highest-scoring feature under each target, bedtools map -o first / last, SQL's
 * ROW_NUMBER() OVER (PARTITION BY the probe row ORDER BY ...) = 1 -- in one ivx_probe_overlap_select call (ivx_select.h): no
 * pair is ever made.  The reference has no counterpart.  Tables, keys and strict_predicate as in brh_overlap_aggregate (the
 * overlap lengths are those of the adjusted coordinates).  Ties go to the smallest build row.
 * by: a BRH_SEL_* criterion (numbered like IVX_SEL_*).  value_column is named for BRH_SEL_MIN_VAL / BRH_SEL_MAX_VAL and for
 * them only: one that is missing, or given with another criterion, is refused with its own message.  It is Int8 .. Int64 or
 * UInt8 .. UInt32 (as brh_overlap_aggregate), UInt64 (compared with the top bit flipped), or Float32 / Float64 (widened to
 * double and compared in the order of the reals, -0.0 below +0.0; a NaN anywhere is refused by name); nulls are refused.
 * Outputs, one row per probe row in probe order:
 *   build_idx  UInt32, NULL where the probe row overlaps nothing: what a take of the build table wants for a left join to at
 *              most one row
 *   score      Int64, NULL where build_idx is: the criterion at the winner -- its value, the closed overlap length, or the
 *              row.  For a UInt64 or float value column the slot stays released (zeroed): take the value with build_idx. */
enum { BRH_SEL_MIN_VAL = 0, BRH_SEL_MAX_VAL = 1, BRH_SEL_MAX_OVERLAP = 2, BRH_SEL_MIN_OVERLAP = 3,
       BRH_SEL_FIRST_ROW = 4, BRH_SEL_LAST_ROW = 5, BRH_SEL_N = 6 };
int brh_overlap_select(brh_session *s, brh_batch build, brh_columns bcols, const char *value_column /* nullable */,
                       brh_batch probe, brh_columns pcols, int strict_predicate, int by,
                       struct ArrowArray *build_idx, struct ArrowSchema *build_idx_schema,
                       struct ArrowArray *score, struct ArrowSchema *score_schema);

/* Overlap thresholds (ivx_where.h): the integer fields of ivx_overlap_where, with its pass rule and its refusals (a negative
 * min_bases, a fraction above 1, a zero or too large denominator, either not 0 or 1).  On the adjusted coordinates of the two
 * tables (strict_predicate: end - 1 on both sides): len = the closed overlap length, plen / blen = the probe / build row's.
 * A pair passes iff len >= max(1, min_bases), len * probe_den >= plen * probe_num and len * build_den >= blen * build_num
 * (a fraction with num = 0 is not asked; either = 1: one of two asked fractions suffices).  where = NULL, or one that asks
 * nothing, is the function without _where.
 *   brh_interval_join_where      every join type over the same filtered matches: Inner = the pairs that pass (ivx_pairs_where
 *                                behind the fill); RightSemi / RightAnti = the probe rows with / without a passing pair;
 *                                LeftSemi / LeftAnti = the build rows with / without one; Left / Right / Full = the passing
 *                                pairs, then the rows without one.  nearest_algorithm != 0 with a threshold is refused.
 *   brh_overlap_aggregate_where  the aggregates over the passing build rows of each probe row
 *   brh_overlap_select_where     the best of the passing build rows of each probe row */
typedef struct brh_overlap_where {
    int64_t  min_bases;
    uint32_t probe_num, probe_den;
    uint32_t build_num, build_den;
    uint32_t either;
} brh_overlap_where;
int brh_interval_join_where(brh_session *s, brh_batch build, brh_columns bcols, brh_batch probe, brh_columns pcols,
                            int join_type, int strict_predicate, int nearest_algorithm, const brh_overlap_where *where,
                            struct ArrowArray *build_idx, struct ArrowSchema *build_idx_schema,
                            struct ArrowArray *probe_idx, struct ArrowSchema *probe_idx_schema);
int brh_overlap_aggregate_where(brh_session *s, brh_batch build, brh_columns bcols, const char *value_column,
                                brh_batch probe, brh_columns pcols, int strict_predicate, uint32_t ops, const brh_overlap_where *where,
                                struct ArrowArray *out, struct ArrowSchema *out_schema);
int brh_overlap_select_where(brh_session *s, brh_batch build, brh_columns bcols, const char *value_column /* nullable */,
                             brh_batch probe, brh_columns pcols, int strict_predicate, int by, const brh_overlap_where *where,
                             struct ArrowArray *build_idx, struct ArrowSchema *build_idx_schema,
                             struct ArrowArray *score, struct ArrowSchema *score_schema);

/* merge('table'[,min_dist]...): MergeProvider/MergeStream (R/src/merge.rs:84-112, :263-350).
 * Outputs contig Utf8, start Int64, end Int64, n_intervals Int64. */
int brh_merge(brh_session *s, brh_batch table, brh_columns cols, int64_t min_dist, int filter_op,
              struct ArrowArray *contig, struct ArrowSchema *contig_schema,
              struct ArrowArray *start, struct ArrowSchema *start_schema,
              struct ArrowArray *end, struct ArrowSchema *end_schema,
              struct ArrowArray *n_intervals, struct ArrowSchema *n_schema);

/* subtract('left','right'): SubtractStream / SubtractStreamExtra (R/src/subtract.rs:354-462, :529-662).
 * Outputs contig Utf8, start Int64, end Int64 and left_row UInt32 (the row of `left` each fragment
 * came from, for the extra-columns take). */
int brh_subtract(brh_session *s, brh_batch left, brh_columns lcols, brh_batch right, brh_columns rcols,
                 int filter_op,
                 struct ArrowArray *contig, struct ArrowSchema *contig_schema,
                 struct ArrowArray *start, struct ArrowSchema *start_schema,
                 struct ArrowArray *end, struct ArrowSchema *end_schema,
                 struct ArrowArray *left_row, struct ArrowSchema *left_row_schema);

/* intersect('left','right'): the pieces of every left row that the right table's merged intervals cover (ivx_intersect,
 * include/ivx.h; the reference has no such table function).  Schema and behaviour of brh_subtract: contig Utf8, start
 * Int64, end Int64 named after the LEFT table's columns, in (contig in byte order, start, end, left row) order with a
 * row's pieces ascending, and left_row UInt32 (the row of `left` each piece came from, for the extra-columns take).  A row
 * with end < start in either table is an error. */
int brh_intersect(brh_session *s, brh_batch left, brh_columns lcols, brh_batch right, brh_columns rcols,
                  int filter_op,
                  struct ArrowArray *contig, struct ArrowSchema *contig_schema,
                  struct ArrowArray *start, struct ArrowSchema *start_schema,
                  struct ArrowArray *end, struct ArrowSchema *end_schema,
                  struct ArrowArray *left_row, struct ArrowSchema *left_row_schema);

/* cluster('table'[,min_dist]...): ClusterProvider / ClusterStream / ClusterStreamExtra
 * (R/src/cluster.rs:29-82, :517-760, :762-977).  One output row per input row, sorted by
 * (contig, start, end, input row): contig Utf8, start Int64, end Int64, row UInt32 (the input row,
 * for the extra-columns take, cluster.rs:787-806), cluster Int64, cluster_start Int64, cluster_end Int64. */
int brh_cluster(brh_session *s, brh_batch table, brh_columns cols, int64_t min_dist, int filter_op,
                struct ArrowArray *contig, struct ArrowSchema *contig_schema,
                struct ArrowArray *start, struct ArrowSchema *start_schema,
                struct ArrowArray *end, struct ArrowSchema *end_schema,
                struct ArrowArray *row, struct ArrowSchema *row_schema,
                struct ArrowArray *cluster, struct ArrowSchema *cluster_schema,
                struct ArrowArray *cluster_start, struct ArrowSchema *cluster_start_schema,
                struct ArrowArray *cluster_end, struct ArrowSchema *cluster_end_schema);

/* complement('table'[,'view_table']...): ComplementProvider / ComplementStream
 * (R/src/complement.rs:28-75, :236-478).  view.array == NULL means no view table: every contig gets
 * [0, i64::MAX).  Outputs contig Utf8, start Int64, end Int64 named after the INPUT table's columns. */
int brh_complement(brh_session *s, brh_batch table, brh_columns cols, brh_batch view, brh_columns view_cols, int filter_op,
                   struct ArrowArray *contig, struct ArrowSchema *contig_schema,
                   struct ArrowArray *start, struct ArrowSchema *start_schema,
                   struct ArrowArray *end, struct ArrowSchema *end_schema);

/* depth('reads'): the pileup crate's coverage blocks (bio-function-pileup: events.rs process_batch / process_batch_dense,
 * coverage.rs events_to_coverage_blocks / dense_depth_to_coverage_blocks) in one ivx_depth call.
 * reads: a batch with the reference's column names (schema.rs:7-11): chrom Utf8 / LargeUtf8 / Utf8View; start, flags,
 *   mapping_quality UInt32; cigar Binary (packed u32 ops).  Rows with a NULL chrom or start are skipped; the validity of flags
 *   and mapping_quality is not read (events.rs:114-121).  A Utf8 cigar column is the error "depth: string CIGAR columns are
 *   not supported, use the binary CIGAR column" unless the session has brh_session_set_string_cigars on: then cigar may also be
 *   Utf8 or LargeUtf8 ("5M3D5M"), parsed on the device (ivx.h ivx_cigar_parse: its token rules, its two divergences and its
 *   errors); sliced arrays as for Binary, the validity of cigar is not read, and any other type is the error "depth: unsupported
 *   data type <format> for column 'cigar'; expected Binary, Utf8 or LargeUtf8".  brh_depth_per_base_open and brh_depth_push_batch
 *   follow the same rule.
 * prior (array == NULL: none): contig, pos_start, pos_end, coverage -- the output of an earlier call, fed in as weighted
 *   segments: that is how coverage accumulates over batches.
 * lengths (array == NULL: none): name Utf8, length (any integer type; clamped to 2^32-1) -- the reference's dense mode: events
 *   beyond a contig's length are dropped, reads on a contig the table lacks are skipped (events.rs:247-260).
 * Contig ids are assigned in byte order of the names (coverage.rs:75-76, physical_exec.rs:400-402).  Outputs
 * (schema.rs:28-41): contig Utf8, pos_start Int32, pos_end Int32 (the u32 positions `as i32`), coverage Int16 (`as i16`),
 * in the coordinate system `start` came in. */
int brh_depth(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths, uint32_t filter_flag, uint32_t min_mapq,
              struct ArrowArray *contig, struct ArrowSchema *contig_schema,
              struct ArrowArray *pos_start, struct ArrowSchema *pos_start_schema,
              struct ArrowArray *pos_end, struct ArrowSchema *pos_end_schema,
              struct ArrowArray *coverage, struct ArrowSchema *coverage_schema);

/* depth('reads', zero_based, per_base = true): one (contig, pos Int32, coverage Int16) row per position of every contig that
 * has reads (bio-function-pileup coverage.rs:271-365 PerBaseEmitter, physical_exec.rs:404-414, :517-548), as a pull stream.
 * open: the column rules of brh_depth; builds ONE depth profile (ivx_depth_profile_build) that the stream keeps on the device.
 *   lengths is required: without it the error is the reference's "per_base mode requires dense accumulation (BAM header with
 *   contig lengths). Sparse fallback (e.g. MemTable) is not supported for per_base output." (physical_exec.rs:299-303).
 * next: mirrors PerBaseEmitter::next_batch.  Contigs come in byte order of their names, and only those an event touched
 *   (events.rs:198-206) -- also when its events cancel; a contig of the length table without reads is absent.  Positions run
 *   [0, len) when zero_based, else [1, len + 1) without the depth array's slot 0 (coverage.rs:294-301).  A batch holds at most
 *   max_rows rows and never spans two contigs; max_rows = 0 is an error.  *done = 1, with no arrays exported, once everything
 *   has been returned.  contig: Utf8 (the name repeated, filled on the host); pos: Int32; coverage: Int16 (`as i16`).
 * close: frees the profile.  The stream must not outlive its session. */
typedef struct brh_depth_stream brh_depth_stream;
int  brh_depth_per_base_open(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths, int zero_based,
                             uint32_t filter_flag, uint32_t min_mapq, brh_depth_stream **out);
int  brh_depth_per_base_next(brh_depth_stream *ds, uint64_t max_rows, int *done,
                             struct ArrowArray *contig, struct ArrowSchema *contig_schema,
                             struct ArrowArray *pos, struct ArrowSchema *pos_schema,
                             struct ArrowArray *coverage, struct ArrowSchema *coverage_schema);
void brh_depth_per_base_close(brh_depth_stream *ds);

/* Streaming depth(): the shape the reference runs depth() in -- accumulate_partition drains a STREAM of read batches into one
 * accumulator (bio-function-pileup physical_exec.rs:269-329), merge_dense_results / merge_sparse_results add the partitions'
 * accumulators together (:367-463), and only then is anything emitted.  The accumulator here is a depth profile on the device
 * (ivx.h g'): exact int32 coverage, the open block of a clipped contig and key_seen included, none of which the `prior`
 * round trip of brh_depth can carry.
 * open: lengths (array == NULL: the sparse mode) as for brh_depth.  With it the contig dictionary is the table's names in byte
 *   order, fixed for the stream; reads elsewhere are skipped.  Without it the dictionary grows in arrival order: a new name gets
 *   the next id, and a batch's profile is built with as many keys as the dictionary has by then.
 * push: the column rules and errors of brh_depth's reads batch (a batch that fails them changes nothing: the stream goes on).
 *   One ivx_depth_profile_build per batch; the profile goes onto a stack that is merged like a binary counter -- while the new
 *   top has at least half the steps of the profile below it, the two are merged (ivx_depth_profile_merge) and freed -- so about
 *   log2(batches) profiles are alive and the merge work is O(n log n) instead of one merge of everything per batch.  A batch
 *   of 0 rows is a no-op (:282-284).  Coalescing 8192-row batches into large ones before they are pushed remains the caller's
 *   job (CoalesceBatchesExec), as for the join stream: a device call per small batch is all launch latency.
 * finish: merges the stack down to one profile and returns its blocks (ivx_depth_profile_blocks) as brh_depth does: contig
 *   Utf8, pos_start / pos_end Int32, coverage Int16 (`as i16`), contigs in byte order of their names -- in the sparse mode a
 *   per-contig copy on the host.  A stream that never received a row gives four empty arrays.
 * finish_per_base: without lengths the error is the reference's (see brh_depth_per_base_open).  Otherwise the merged profile
 *   MOVES into a brh_depth_stream, which brh_depth_per_base_next / _close then serve as ever.
 * After either finish the push object holds no profile, and push / finish* fail with "depth stream: already finished"; close is
 *   still required and frees whatever is left.  The stream must not outlive its session. */
typedef struct brh_depth_push brh_depth_push;
int  brh_depth_push_open(brh_session *s, brh_batch lengths, uint32_t filter_flag, uint32_t min_mapq, brh_depth_push **out);
int  brh_depth_push_batch(brh_depth_push *dp, brh_batch reads);
int  brh_depth_push_finish(brh_depth_push *dp,
                           struct ArrowArray *contig, struct ArrowSchema *contig_schema,
                           struct ArrowArray *pos_start, struct ArrowSchema *pos_start_schema,
                           struct ArrowArray *pos_end, struct ArrowSchema *pos_end_schema,
                           struct ArrowArray *coverage, struct ArrowSchema *coverage_schema);
int  brh_depth_push_finish_per_base(brh_depth_push *dp, int zero_based, brh_depth_stream **out);
void brh_depth_push_close(brh_depth_push *dp);

/* Depth region summaries: per row of a regions table the number of bases, the sum of the coverage over them and the number of
 * bases at or above each threshold (ivx.h ivx_depth_profile_summarize) -- mean depth per target, bases at 10x / 20x / 30x,
 * coverage in bins (samtools bedcov, mosdepth --by / --thresholds).  The reference has no counterpart: its coverage() counts
 * merged build intervals, not read depth.
 * brh_depth_regions: reads / prior / lengths as for brh_depth; builds ONE depth profile, summarises and frees it.
 * regions: region_cols names one contig column (Utf8 / LargeUtf8 / Utf8View) and the start and end columns (Int32, Int64, UInt32
 *   or UInt64, each on its own); a value outside [0, 2^32-1] is clamped; a NULL coordinate is the error "coordinate column
 *   contains null values; requires non-null coordinates".  Ends are inclusive; end_exclusive = 1 reads BED-style half-open ends
 *   (end <= start: an empty region).  A contig the dictionary lacks has coverage 0 everywhere (and no domain).
 * Domain: with lengths it is the one brh_depth_per_base_next emits -- [0, len - 1] when zero_based, else [1, len] without the
 *   step at position 0 -- so `sum` equals the sum of the per-base rows inside the region whenever those fit Int16; the part of
 *   a region outside it counts nowhere.  Without lengths it is the whole u32 range (zero_based is not read).
 * Outputs: one row per region, in region order, all Int64 and non-null: bases, sum, and n_thr (<= 8) arrays ge[j] named
 *   bases_ge_<thresholds[j]>; ge / ge_schemas point at n_thr structs (NULL when n_thr = 0).  No floating point: the caller divides.
 * brh_depth_push_regions: the same over everything pushed so far.  Merges the stack down to one profile, which stays the
 *   stack's only entry: the stream stays open, can be pushed to and finished as ever; after a finish it fails with "depth stream:
 *   already finished". */
int  brh_depth_regions(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths, brh_batch regions, brh_columns region_cols,
                       int zero_based, int end_exclusive, uint32_t filter_flag, uint32_t min_mapq,
                       const int32_t *thresholds, uint32_t n_thr,
                       struct ArrowArray *bases, struct ArrowSchema *bases_schema,
                       struct ArrowArray *sum, struct ArrowSchema *sum_schema,
                       struct ArrowArray *ge, struct ArrowSchema *ge_schemas);
int  brh_depth_push_regions(brh_depth_push *dp, brh_batch regions, brh_columns region_cols, int zero_based, int end_exclusive,
                            const int32_t *thresholds, uint32_t n_thr,
                            struct ArrowArray *bases, struct ArrowSchema *bases_schema,
                            struct ArrowArray *sum, struct ArrowSchema *sum_schema,
                            struct ArrowArray *ge, struct ArrowSchema *ge_schemas);

/* Depth region order statistics: per row of a regions table the number of bases and the minimum, the maximum and up to 8
 * quantiles of the per-base coverage over them (ivx.h ivx_depth_profile_quantiles) -- minimum and median coverage per target or
 * bin (bedtools map -o min,max, Picard MIN_ / MEDIAN_TARGET_COVERAGE, mosdepth --use-median).
 * brh_depth_region_quantiles / brh_depth_push_region_quantiles take the arguments of brh_depth_regions / brh_depth_push_regions
 * one for one (reads / prior / lengths / regions / region_cols / zero_based / end_exclusive / the read filter; the same domain,
 * the same unknown contigs, the stream stays open), with q_num[n_q] (n_q <= 8) and q_den (1 .. 65536, every q_num <= q_den) in
 * place of the thresholds: quantile j is element floor((bases - 1) * q_num[j] / q_den) of the region's per-base values sorted
 * ascending -- q_num = 1, q_den = 2 is the lower median -- which equals that element of the sorted per-base rows inside the
 * region whenever those fit Int16.
 * Outputs: one row per region, in region order: bases Int64, non-null; min, max and n_q arrays q[j] named q_<q_num[j]>_<q_den>,
 *   all Int32 and NULL exactly where bases = 0; q / q_schemas point at n_q structs (NULL when n_q = 0). */
int  brh_depth_region_quantiles(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths, brh_batch regions, brh_columns region_cols,
                                int zero_based, int end_exclusive, uint32_t filter_flag, uint32_t min_mapq,
                                const uint32_t *q_num, uint32_t n_q, uint32_t q_den,
                                struct ArrowArray *bases, struct ArrowSchema *bases_schema,
                                struct ArrowArray *min, struct ArrowSchema *min_schema,
                                struct ArrowArray *max, struct ArrowSchema *max_schema,
                                struct ArrowArray *q, struct ArrowSchema *q_schemas);
int  brh_depth_push_region_quantiles(brh_depth_push *dp, brh_batch regions, brh_columns region_cols, int zero_based, int end_exclusive,
                                     const uint32_t *q_num, uint32_t n_q, uint32_t q_den,
                                     struct ArrowArray *bases, struct ArrowSchema *bases_schema,
                                     struct ArrowArray *min, struct ArrowSchema *min_schema,
                                     struct ArrowArray *max, struct ArrowSchema *max_schema,
                                     struct ArrowArray *q, struct ArrowSchema *q_schemas);

/* Depth coverage classes: every base classified by its coverage (ivx.h ivx_depth_profile_quantize / ivx_depth_profile_hist).
 * brh_depth_quantize: the maximal intervals whose coverage stays in one bin -- mosdepth --quantize, GATK CallableLoci, "the
 *   intervals at 10x or more".  bin(v) = the number of cuts <= v (cuts[n_cuts], n_cuts <= 31, strictly ascending); a run goes out
 *   iff bit `bin` of emit_mask is set, and the runs of the other bins still separate their neighbours.
 *   Outputs, ordered by (contig, start), all non-null but contig's schema: contig Utf8, start and end Int64 (end inclusive;
 *   end_exclusive = 1 adds 1: mosdepth's BED is zero_based with end_exclusive), bin Int32.  Contigs come in the order brh_depth
 *   emits them.  The result is an interval table: subtract, complement and the joins take it.
 * brh_depth_dist: per contig the number of bases at each coverage value -- bedtools genomecov's default output, mosdepth's dist,
 *   the histogram of Picard CollectWgsMetrics.  Bin b of n_bins (1 .. 65536) counts the bases with coverage v_lo + b.  The two end
 *   bins are clamped: coverage v_lo stands for "v_lo or less" and coverage v_lo + n_bins - 1 for "that or more"; they keep their
 *   edge value in the output.  Outputs: contig Utf8, coverage Int32, bases Int64; one row per contig and bin with bases > 0, in
 *   (contig, coverage) order.  No floating point: cumulative fractions are the caller's division.
 * Both: reads / prior / lengths and the read filter as for brh_depth_regions; ONE depth profile is built, read and freed.  The
 *   domain is that of brh_depth_regions: with lengths [0, len - 1] when zero_based, else [1, len] without the step at position 0;
 *   without lengths the whole u32 range (zero_based is not read).  touched_only = 1: only contigs that kept a read or a prior
 *   block after the filter and the clipping take part (the contigs brh_depth_per_base_next emits); 0: every contig of the
 *   dictionary with a non-empty domain, a contig without coverage as one run / one row of coverage 0.
 * brh_depth_push_quantize / brh_depth_push_dist: the same over everything pushed so far.  They merge the stack down to one
 *   profile, which stays the stack's only entry: the stream stays open, as with brh_depth_push_regions.
 * Not built: distributions or runs restricted to a region set, a minimum run length, labels for the bins. */
int  brh_depth_quantize(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths, int zero_based, int end_exclusive,
                        int touched_only, uint32_t filter_flag, uint32_t min_mapq,
                        const int32_t *cuts, uint32_t n_cuts, uint32_t emit_mask,
                        struct ArrowArray *contig, struct ArrowSchema *contig_schema,
                        struct ArrowArray *start, struct ArrowSchema *start_schema,
                        struct ArrowArray *end, struct ArrowSchema *end_schema,
                        struct ArrowArray *bin, struct ArrowSchema *bin_schema);
int  brh_depth_push_quantize(brh_depth_push *dp, int zero_based, int end_exclusive, int touched_only,
                             const int32_t *cuts, uint32_t n_cuts, uint32_t emit_mask,
                             struct ArrowArray *contig, struct ArrowSchema *contig_schema,
                             struct ArrowArray *start, struct ArrowSchema *start_schema,
                             struct ArrowArray *end, struct ArrowSchema *end_schema,
                             struct ArrowArray *bin, struct ArrowSchema *bin_schema);
int  brh_depth_dist(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths, int zero_based, int touched_only,
                    uint32_t filter_flag, uint32_t min_mapq, int32_t v_lo, uint32_t n_bins,
                    struct ArrowArray *contig, struct ArrowSchema *contig_schema,
                    struct ArrowArray *coverage, struct ArrowSchema *coverage_schema,
                    struct ArrowArray *bases, struct ArrowSchema *bases_schema);
int  brh_depth_push_dist(brh_depth_push *dp, int zero_based, int touched_only, int32_t v_lo, uint32_t n_bins,
                         struct ArrowArray *contig, struct ArrowSchema *contig_schema,
                         struct ArrowArray *coverage, struct ArrowSchema *coverage_schema,
                         struct ArrowArray *bases, struct ArrowSchema *bases_schema);

/* compute::take of ONE payload column with an index array a join / nearest call returned
 * (interval_join.rs:1655-1667, nearest.rs:469-482), on the device.  column: any fixed-width primitive
 * (ints, floats, date/time/timestamp/duration, decimal128/256, fixed-size binary of 1/2/4/8/16/32 bytes),
 * Boolean, Utf8 / LargeUtf8 / Binary / LargeBinary, or Utf8View / BinaryView (the output is compacted
 * into one data buffer), or a dictionary-encoded column over any of the flat value types (the keys are gathered, the
 * output carries its own copy of the dictionary); idx: UInt32, nulls allowed (-> null output slots).
 * Nested columns -- Struct, List / LargeList / FixedSizeList, Map, in any nesting over the types above -- are taken level
 * by level (a struct's row selection on every child, a list's rows as ranges of child elements); their leaves go through
 * the same device gathers, offsets and validity of the nesting levels are host work.  Union and run-end-encoded layouts
 * return an error.  The output has the column's type and is nullable. */
int brh_take(brh_session *s, const struct ArrowArray *column, const struct ArrowSchema *column_schema,
             const struct ArrowArray *idx, const struct ArrowSchema *idx_schema,
             struct ArrowArray *out, struct ArrowSchema *out_schema);

/* IntervalJoinStream as a push interface (interval_join.rs:934-1140, :1418-1677).  open indexes the build side once
 * (collect_left_input, :584-700); push takes one probe RecordBatch (FetchProbeBatch / ProcessProbeBatch).  Probe
 * batches are coalesced into groups of at least `coalesce_rows` rows (0 = 4 Mi) before they go to the GPU -- the job
 * of CoalesceBatchesExec in a DataFusion plan: a device call per 8192-row batch would be all launch latency.
 * join_type:
 *   BRH_JOIN_INNER       (build_idx, probe_idx) pairs (:1614-1653)
 *   BRH_JOIN_RIGHT_SEMI / _ANTI   probe_idx only: the probe rows with / without a match, ascending (:1014-1024, :1433-1463)
 *   BRH_JOIN_NEAREST     Algorithm::CoitreesNearest: one row per probe row, build_idx NULL where the key has no build row
 *                        (:864-870, :1226-1238, :1628-1635)
 *   BRH_JOIN_LEFT_SEMI / _ANTI / BRH_JOIN_LEFT / _RIGHT / _FULL   the stream keeps one match bitmap for its index (host
 *                        words: this layer holds no device memory of its own; the library ORs every call's marks into
 *                        them).  LeftSemi / LeftAnti: a flushed group marks the bitmap (ivx_probe_mark_build) and gives
 *                        NO result.  Left / Full: the group's Inner pairs, and ivx_bits_mark over them.  Right / Full: the
 *                        group's unmatched probe rows follow its pairs, build_idx NULL.  finish queues ONE more result
 *                        behind the last group's: n_batches = 0, batch_offsets = [0], the build-side rows -- the matched
 *                        ones for LeftSemi, the unmatched ones for LeftAnti / Left / Full (none for Right) -- ascending,
 *                        with probe_idx all NULL (LeftSemi / LeftAnti: empty).
 * max_output_rows: 0 = every group gives ONE result (the regular mode).  > 0 = the reference's low-memory stream
 *   (:1153-1299): a result holds whole probe rows and ends after the row at which its running output-row count
 *   reaches the budget (:1199-1216, :1256-1273), so it stays below budget + the matches of its last row;
 *   BRH_MAX_OUTPUT_ENV = the reference's default, BIO_MAX_OUTPUT_BATCH_SIZE or 100000 (:543-548).  With a join type from
 *   BRH_JOIN_LEFT_SEMI on, open fails with "join stream: max_output_rows > 0 (the low-memory mode) is not supported with
 *   LeftSemi / LeftAnti / Left / Right / Full joins".
 * next: probe_idx counts over the group's concatenated rows; batch_offsets Int64 [n_batches + 1] = the first row of
 * each of the group's batches, so the caller can concatenate its buffered batches (or split the pairs) and `take`
 * the payload columns as the reference does (:1655-1667); *group_done = 1 with the group's last result (the
 * caller may drop the group's buffered batches).  *n_ready = results waiting in the queue.  Probe rows whose key
 * the build side does not have never match.  finish flushes the last, partial group. */
typedef struct brh_join_stream brh_join_stream;
int  brh_join_stream_open(brh_session *s, brh_batch build, brh_columns bcols, brh_columns pcols, int strict_predicate,
                          uint64_t coalesce_rows, int join_type, uint64_t max_output_rows, brh_join_stream **out);
int  brh_join_stream_push(brh_join_stream *js, brh_batch probe, int *n_ready);
int  brh_join_stream_finish(brh_join_stream *js, int *n_ready);
int  brh_join_stream_next(brh_join_stream *js, uint64_t *first_batch, uint64_t *n_batches, int *group_done,
                          struct ArrowArray *build_idx, struct ArrowSchema *build_idx_schema,
                          struct ArrowArray *probe_idx, struct ArrowSchema *probe_idx_schema,
                          struct ArrowArray *batch_offsets, struct ArrowSchema *batch_offsets_schema);
void brh_join_stream_close(brh_join_stream *js);

/* the checks alone (no GPU): resolve a position column like PosArray::resolve / resolve_i64 would;
 * 0 = fine, else the error text is set.  Used by the CPU-only tests. */
int brh_check_position_column(brh_session *s_or_null, brh_batch table, const char *column, int as_i64,
                              char *errbuf, int errbuf_len);
/* ... and a contig column like ContigArray (array_utils.rs:10-24, :178-229): Utf8 / LargeUtf8 / Utf8View.  NULL contigs
 * pass unless the session (or, without one, BIO_STRICT_NULL_CONTIGS=1) is strict about them, see below. */
int brh_check_contig_column(brh_session *s_or_null, brh_batch table, const char *column, char *errbuf, int errbuf_len);
/* NULL contigs.  Default (on = 0), as the reference, which never reads a contig column's validity bitmap: the table
 * functions key a NULL slot by the bytes its offsets span (`value(i)`: "" for builder-made arrays), the join treats NULL as a
 * key of its own that matches only NULL (create_hashes; hashes are compared, never values: interval_join.rs:857, :922-928).
 * None of the reference's tests pins this (parity unpinned).  on = 1: a batch with a NULL contig is refused with an error
 * instead (the default of new sessions when BIO_STRICT_NULL_CONTIGS=1 is set). */
int brh_session_set_strict_null_contigs(brh_session *s, int on);
/* Text CIGARs for depth().  Default (on = 0): a Utf8 / LargeUtf8 cigar column is refused, see brh_depth.  on = 1: brh_depth,
 * brh_depth_per_base_open and brh_depth_push_batch accept one and go through ivx_depth_text / ivx_depth_profile_build_text;
 * Binary columns work as before. */
int brh_session_set_string_cigars(brh_session *s, int on);

/* BuildProbeJoinMetrics of the session's context under the reference's names (joins/utils.rs:399-453), and the device
 * memory the session may reserve (MemoryReservation::try_grow, interval_join.rs:614-639): ivx.h ivx_ctx_metrics /
 * ivx_ctx_set_memory_limit. */
int brh_session_metrics(brh_session *s, ivx_metrics *out);
int brh_session_set_memory_limit(brh_session *s, uint64_t bytes);
/* device bytes the session holds reserved right now: scratch plus live indexes and depth profiles (ivx_ctx_reserved_bytes) */
int brh_session_reserved_bytes(brh_session *s, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif
