/*
 * ivx.h -- C ABI of the MI355X-native interval build-and-probe library
 *          (libivx_hip.so, hand-written HIP for gfx950).
 *
 * This is the drop-in boundary for ONE path of
 * biodatageeks/datafusion-bio-functions: the interval index build + probe
 * behind `datafusion-bio-function-ranges` (IntervalJoinExec and the
 * overlap / count_overlaps / coverage / nearest / merge / subtract table
 * functions).  The reference has no FFI of its own (no extern "C" anywhere);
 * each entry point below names the reference Rust function whose inner loop
 * it replaces -- the call a maintainer would swap for an `unsafe extern "C"`
 * call in the stream implementation (see INTEGRATION.md for the Rust stub).
 * R/ = datafusion/bio-function-ranges/ in the reference tree.
 *
 * Conventions
 *  - Plain pointers and sizes only.  No Arrow, torch or C++ types.
 *  - `mem` says where EVERY data pointer of that call lives:
 *      IVX_MEM_HOST   host memory (Arrow buffers); the library copies them to
 *                     device scratch with hipMemcpyAsync on the ctx stream;
 *      IVX_MEM_DEVICE device memory of the ctx's GPU (e.g. buffers the caller
 *                     already keeps in HBM); no copies, kernels run on the
 *                     ctx stream.
 *    Scalar out-parameters (`uint64_t *total`, `*n_out`, ...) are always host
 *    pointers; writing them synchronises the ctx stream.
 *  - An IVX_MEM_DEVICE call is ordered on the ctx stream like a kernel launch
 *    of the caller's own.  Its input columns may be the product of earlier
 *    work on that stream that has not run yet when the call is made; its
 *    output columns may be consumed by work queued on that stream right after
 *    the call returns, with no host synchronisation (the call may return with
 *    kernels in flight); work on any other stream is the caller's to order
 *    against the ctx stream.  Two exceptions, stated with their entries: with
 *    the build overlap on (ivx_ctx_set_build_overlap) the build columns stay
 *    unchanged until the index's first probe call has returned, and the input
 *    columns stay unchanged between a total-only ivx_probe_overlap_count (an
 *    ivx_subtract sizing call) and the fill call its state serves.
 *    (tests/test_gpu_entry_stream_order.py; DESIGN.md, "What a device-mode
 *    call may assume of its stream".)
 *  - Keys never cross the boundary as strings: the host maps the equi-key
 *    column(s) (contig, or contig+strand, ...) to dense ids 0..n_keys-1.  The
 *    reference groups rows by a 64-bit hash of the key columns and never
 *    compares key values (interval_join.rs:857, :922-928); dense ids differ
 *    from that only under a hash collision (documented divergence).
 *    `key == NULL` means "one key" (range-only join: interval_join.rs on
 *    [(lit 1, lit 1)], bio_physical_planner.rs:125-146).
 *  - Join/count/coverage/nearest coordinates are int32, closed [start,end]
 *    (array_utils.rs:66-135 `resolve()`); merge/subtract are int64
 *    (`resolve_i64()`, :137-172).  Range checks and null checks stay in the
 *    host layer, with the reference's wording.
 *  - "build" is the reference's left / collected side, "probe" the streamed
 *    right side.  Row indices are uint32 (interval_join.rs:759-760, :1616).
 *  - `strict` for count/coverage/nearest shrinks the QUERY (qs+1, qe-1) as the
 *    UDTFs do (interval_tree.rs:185-188, :253-256; nearest.rs:341-344).  The
 *    SQL join path instead rewrites `<`/`>` into `end-1` on both sides
 *    (intervals.rs:85-115); callers of ivx_probe_overlap_* pass already
 *    adjusted columns, exactly as IntervalJoinExec evaluates them.
 *  - Every function returns an ivx_status; ivx_last_error(ctx) holds the text
 *    (maps to DataFusionError::Execution).
 *  - An ivx_index is immutable after build and may be probed concurrently
 *    from several host threads, each with its OWN ivx_ctx on the same device
 *    (the reference shares Arc<JoinLeftData> across partitions,
 *    interval_join.rs:466-480).  It is complete when ivx_index_build returns
 *    (the build has waited for its stream), up to the tail of an overlapped
 *    build, behind which every probe call of every ctx orders its own stream:
 *    another ctx on another stream may probe it at once, no
 *    ivx_ctx_synchronize on the building ctx is owed first.
 *  - There is NO CPU fallback: without a usable gfx950 device
 *    ivx_ctx_create fails with IVX_ERR_NO_DEVICE.
 */
#ifndef IVX_H
#define IVX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ivx_ctx ivx_ctx;
typedef struct ivx_index ivx_index;
typedef int32_t ivx_status;

enum {
    IVX_OK = 0,
    IVX_ERR_INVALID = 1,      /* bad argument (null pointer, key id >= n_keys, min_dist < 0 ...) */
    IVX_ERR_NO_DEVICE = 2,    /* no HIP device / not gfx950 */
    IVX_ERR_HIP = 3,          /* a HIP runtime call failed; text in ivx_last_error */
    IVX_ERR_OOM = 4,          /* device or pinned allocation failed (ResourcesExhausted) */
    IVX_ERR_CAPACITY = 5,     /* caller's output buffers too small; the needed size is returned */
    IVX_ERR_UNSUPPORTED = 6   /* e.g. wrong index kind for this probe */
};

enum { IVX_MEM_HOST = 0, IVX_MEM_DEVICE = 1 };

/* which reference structure the index replaces */
enum {
    IVX_KIND_OVERLAP = 0,   /* COITree per key            interval_join.rs:745-763 (a1+a2)        */
    IVX_KIND_COUNT = 1,     /* CountOverlapIndex          interval_tree.rs:20-39, :113-143        */
    IVX_KIND_COVERAGE = 2,  /* merged COITree             interval_tree.rs:52-111 (coverage=true) */
    IVX_KIND_NEAREST = 3,   /* NearestIntervalIndex       nearest_index.rs:44-71                  */
    IVX_KIND_DEPTH_PROFILE = 4  /* the step function of depth(); made by ivx_depth_profile_build only, see there */
};

#define IVX_NULL_IDX 0xFFFFFFFFu   /* NULL build row (interval_join.rs:1233 u32::MAX marker) */

/* ---- context ----------------------------------------------------------- */
ivx_status ivx_ctx_create(int device_ordinal, ivx_ctx **out);
void       ivx_ctx_free(ivx_ctx *ctx);
const char *ivx_last_error(const ivx_ctx *ctx);
/* run on a caller-owned hipStream_t, used verbatim (e.g. torch's current
 * stream; NULL is HIP's default stream, which orders against the caller's
 * other default-stream work).  A fresh ctx runs on its own non-blocking
 * stream; ivx_ctx_use_own_stream switches back to it. */
ivx_status ivx_ctx_set_stream(ivx_ctx *ctx, void *hip_stream);
ivx_status ivx_ctx_use_own_stream(ivx_ctx *ctx);
ivx_status ivx_ctx_synchronize(ivx_ctx *ctx);
/* Build overlap (off by default; IVX_BUILD_OVERLAP=1 turns it on for new contexts).  With it on, ivx_index_build of an
 * IVX_KIND_OVERLAP index from IVX_MEM_DEVICE columns returns as soon as the per-key tables and the region layout are final --
 * all that the routing pass of a big probe batch reads -- and lets the rest of the build (cell count, scan, scatter, region
 * descriptors) run on a second stream of the context.  The next big ivx_probe_overlap_count / _fill call routes its rows
 * beside that tail and only its probe kernel waits for it (the call itself waits on the host for the tail once its routing
 * pass is queued, to learn which probe kernel the finished index takes, and notes that in the index -- the one thing a probe
 * call writes in an index, atomically: other contexts and threads may go on probing it); every other use of the index (any context) and every other call
 * on this context is ordered behind the tail first, so results never change.  What changes is the caller's side of the
 * IVX_MEM_DEVICE contract: the build columns must stay unchanged until the index's first probe call has returned, or
 * ivx_ctx_synchronize (which waits for the tail too) -- as IntervalJoinExec keeps the build batches alive in JoinLeftData
 * for the whole join (interval_join.rs:466-480).  ivx_index_free waits for the tail by itself. */
ivx_status ivx_ctx_set_build_overlap(ivx_ctx *ctx, int on);
/* device time (ms, hipEvent) of the kernels of the last call on this ctx */
double     ivx_ctx_last_kernel_ms(const ivx_ctx *ctx);
const char *ivx_version(void);

/* BuildProbeJoinMetrics (joins/utils.rs:399-453) under the reference's names, accumulated over the calls made on this
 * context since creation / the last reset: build_* by ivx_index_build, the rest by the probe and sweep calls (one
 * call = one input batch and, if it returns rows, one output batch).  Times are host wall time of the calls in ms
 * (what the reference's timers bracket); build_mem_used = device bytes of the indexes built. */
typedef struct ivx_metrics {
    double build_time, join_time;
    uint64_t build_input_batches, build_input_rows, build_mem_used;
    uint64_t input_batches, input_rows, output_batches, output_rows;
} ivx_metrics;
ivx_status ivx_ctx_metrics(const ivx_ctx *ctx, ivx_metrics *out);
void       ivx_ctx_reset_metrics(ivx_ctx *ctx);
/* Device memory this context may hold at once (0 = no limit): its scratch buffers, the index it is building and every
 * index it has built that is still alive -- an index stays reserved against the limit of the context that built it until
 * ivx_index_free, as the reference holds the build side's MemoryReservation until the join stream ends
 * (interval_join.rs:614-639; try_grow fails with ResourcesExhausted).  A call that would go over the limit returns
 * IVX_ERR_OOM and allocates nothing: its out-handle is NULL, its scalar result 0 (or the true count), a host-mode
 * caller's output buffers are untouched, no output batch is counted, and the same call under a higher limit gives the
 * full answer ("What a refused reservation leaves behind").  Not counted: the caller's own buffers, and
 * freed indexes' buffers waiting in the library's recycling pool (ivx_ctx_trim returns those to the device). */
ivx_status ivx_ctx_set_memory_limit(ivx_ctx *ctx, uint64_t bytes);
/* What counts against that limit right now (MemoryReservation::size): scratch + the live indexes this context built. */
uint64_t   ivx_ctx_reserved_bytes(const ivx_ctx *ctx);
/* Give scratch back to the device: waits for the context's stream, then frees scratch buffers, largest first, until
 * at most keep_bytes remain (0 = all), and empties the device's pool of recycled index buffers.  Scratch is grow-only
 * otherwise (a 10^9-row sweep leaves ~100 GB behind); the reference returns its reservation when the stream ends
 * (interval_join.rs:614-639) -- call this where the Rust side drops a stream.  Drops the state a sizing / count call
 * left for its fill call. */
ivx_status ivx_ctx_trim(ivx_ctx *ctx, uint64_t keep_bytes);

/* ---- index build: replaces collect_left_input's update_hashmap +
 *      IntervalJoinAlgorithm::new (interval_join.rs:584-668, :745-847, :903-931),
 *      build_count_index_from_batches / build_coitree_from_batches
 *      (interval_tree.rs:75-143) and build_nearest_indexes (nearest.rs:498-547) */
ivx_status ivx_index_build(ivx_ctx *ctx, int kind, int mem,
                           const uint32_t *key /* nullable */, const int32_t *start, const int32_t *end,
                           uint64_t n, uint32_t n_keys, ivx_index **out);
/* The caller must have synchronised (ivx_ctx_synchronize) every ctx that probed the index with
 * IVX_MEM_DEVICE buffers: those calls may return with kernels still in flight, and the index's
 * device buffers go back to a pool that later builds draw from. */
void       ivx_index_free(ivx_index *ix);
uint64_t   ivx_index_rows(const ivx_index *ix);
uint64_t   ivx_index_device_bytes(const ivx_index *ix);

/* ---- layout readout (tests and diagnostics): the form the build picked on the device for the binned overlap index
 *      behind OVERLAP, COUNT and COVERAGE indexes.  Writes min(n_out, IVX_LAYOUT_WORDS) words, the slots below; a
 *      NEAREST index reports its kind and zeros.  Waits for an index whose build tail still runs (build overlap on),
 *      so IVX_LAYOUT_SLOW is final; reads only, the index is unchanged. */
enum {
    IVX_LAYOUT_KIND = 0,        /* IVX_KIND_* */
    IVX_LAYOUT_SH0 = 1,         /* log2 of the level-0 cell width */
    IVX_LAYOUT_NLEV = 2,        /* length-class levels */
    IVX_LAYOUT_LEVROWS = 3,     /* bit l set: level l holds build rows */
    IVX_LAYOUT_RCELLS = 4,      /* level-0 cells per probe region (0: no regions) */
    IVX_LAYOUT_RCS = 5,         /* log2 of that when it is a power of two, else 0xFFFFFFFF */
    IVX_LAYOUT_NREG = 6,        /* probe regions (0: the region probe is not available) */
    IVX_LAYOUT_PK24 = 7,        /* 1: a region spans at most 2^24 coordinates (routed rows pack into 8 bytes) */
    IVX_LAYOUT_SLOW = 8,        /* 1: a row above level 0, or a region slice too big for LDS: no lean fill */
    IVX_LAYOUT_FG = 9,          /* log2 of the occupancy bitmap's block width, or 0xFFFFFFFF: no bitmap */
    IVX_LAYOUT_FBITS = 10,      /* the bitmap's size in bits */
    IVX_LAYOUT_NROUTE_NREG = 11,/* regions of the routing view of big per-row probes (0: none) */
    IVX_LAYOUT_LBUILD = 12,     /* 1: the build sorted every region's rows in LDS; 0: the global counting sort (IVX_BUILD=global) */
    IVX_LAYOUT_WORDS = 13
};
ivx_status ivx_index_layout(ivx_ctx *ctx, const ivx_index *ix, uint32_t *out, uint32_t n_out);

/* ---- a3: IntervalJoinAlgorithm::get + probe loop
 *      (interval_join.rs:849-900, :1614-1653).  Index kind OVERLAP. ---------
 * count: total pairs and, if per_row != NULL, the reference's rle_right
 *        (matches per probe row, uint32). */
ivx_status ivx_probe_overlap_count(ivx_ctx *ctx, const ivx_index *ix, int mem,
                                   const uint32_t *key, const int32_t *start, const int32_t *end, uint64_t n,
                                   uint32_t *per_row /* nullable */, uint64_t *total);
/* fill: the (build_idx, probe_idx) pairs = the reference's (left_indexes,
 *       index_right) before compute::take.  Pair ORDER is unspecified (the
 *       reference pins only the row multiset).  If more than cap pairs exist
 *       nothing useful is written, *written = pairs needed and the call
 *       returns IVX_ERR_CAPACITY.  cap also serves as the hint for the expected
 *       pairs per row (cap / n): size it from ivx_probe_overlap_count, not with
 *       a blanket maximum, or large batches run with needlessly small rounds.
 *       A total-only count call (per_row = NULL) of a large batch leaves the
 *       probe rows routed to the index regions (and, for IVX_MEM_HOST, copied to
 *       the device) in the context: the fill call for the same index, column
 *       pointers, n and stream that is the next call on that context skips that
 *       work (and takes the counted total, not cap, as the density hint) --
 *       the three columns must not change between the two calls.  The state
 *       serves ONE successful fill call (it survives an IVX_ERR_CAPACITY
 *       retry); any other call drops it and a fill call does everything itself.
 *       An IVX_MEM_HOST fill of a big batch (16 M rows or more) that has no such
 *       state to use runs in chunks: the pairs of one chunk are copied to
 *       build_idx / probe_idx by a helper thread while the next chunk's columns
 *       are uploaded (both directions of the link at once).  On IVX_ERR_CAPACITY
 *       the buffers may then hold the pairs of the first chunks. */
ivx_status ivx_probe_overlap_fill(ivx_ctx *ctx, const ivx_index *ix, int mem,
                                  const uint32_t *key, const int32_t *start, const int32_t *end, uint64_t n,
                                  uint32_t *build_idx, uint32_t *probe_idx, uint64_t cap, uint64_t *written);
/* a3': RightSemi / RightAnti (interval_join.rs:1014-1024, :1433-1447):
 *      exists[i] = 1 iff probe row i has a match. */
ivx_status ivx_probe_exists(ivx_ctx *ctx, const ivx_index *ix, int mem,
                            const uint32_t *key, const int32_t *start, const int32_t *end, uint64_t n,
                            uint8_t *exists);

/* a3'': which BUILD rows matched -- LeftSemi / LeftAnti / LeftMark and the unmatched side of Left / Full.  The reference
 *      has no counterpart (IntervalJoinExec emits Inner rows for these types, interval_join.rs:1014-1024); semantics are
 *      HashJoinExec's visited_left_side.  Index kind OVERLAP.
 *      A mark bitmap is caller-owned: (ivx_index_rows(ix) + 31) / 32 uint32_t words, build row b = bit b & 31 of word
 *      b >> 5 -- byte for byte an Arrow validity / Boolean bitmap, so a LeftMark column is the buffer itself.  It lives
 *      where `mem` says.  The library only ever ORs into it: the caller zeroes it once and passes it to as many calls as it
 *      has probe batches; bits set beforehand survive.
 *      Same already-adjusted columns as the other ivx_probe_overlap_* calls; a key id the build side does not have never
 *      matches (as in ivx_probe_exists); n = 0 is a no-op.  A build row is marked iff at least one probe row of the call
 *      overlaps it: same key, bs <= qe && be >= qs.
 *      IVX_MEM_DEVICE: the kernels use device-scope atomic OR, so several contexts may mark into the same buffer at once,
 *      each on its own stream; the call may return with kernels in flight, like other device-mode calls, and the caller
 *      synchronises all of those contexts before ivx_bits_select.  IVX_MEM_HOST: the library marks a zeroed scratch bitmap
 *      (counted against the memory limit like other scratch), copies it back and ORs it into the caller's words on the host.
 *      The call waits for an index whose build tail still runs, drops the state a count call left for its fill call, and
 *      feeds ivx_ctx_metrics like ivx_probe_exists: one input batch and its rows, no output rows. */
ivx_status ivx_probe_mark_build(ivx_ctx *ctx, const ivx_index *ix, int mem,
                                const uint32_t *key, const int32_t *start, const int32_t *end, uint64_t n,
                                uint32_t *marks);
/*      OR bit idx[i] for i < n (what Left / Full use: the pairs exist anyway).  IVX_NULL_IDX is skipped, any other
 *      idx[i] >= n_bits is IVX_ERR_INVALID (in-range bits of that call may or may not be set then; IVX_MEM_HOST leaves
 *      the caller's words as they were).  n_bits < 2^32. */
ivx_status ivx_bits_mark(ivx_ctx *ctx, int mem, const uint32_t *idx, uint64_t n, uint32_t *bits, uint64_t n_bits);
/*      The positions < n_bits whose bit is set (want_set = 1) or clear (0), ascending.  cap = 0 with out = NULL only
 *      counts; cap < *n_out is IVX_ERR_CAPACITY with *n_out = the size needed and nothing written.  Bits at or past
 *      n_bits in the last word are ignored (they may hold anything).  n_bits < 2^32. */
ivx_status ivx_bits_select(ivx_ctx *ctx, int mem, const uint32_t *bits, uint64_t n_bits, int want_set,
                           uint32_t *out, uint64_t cap, uint64_t *n_out);

/* a3''': overlap aggregates -- join on overlap, group by probe row, aggregate a build-side value (SQL's COUNT / SUM / MIN /
 *      MAX over the join, bedtools map, the mean of a signal track over targets) without ever writing a pair.  The reference
 *      has no counterpart; the contract is stated against the join's own pairs.  Index kind OVERLAP.
 *      `val` is one signed integer per BUILD row, val_bytes = 4 (int32, sign-extended) or 8 (int64), ivx_index_rows(ix)
 *      elements, living where `mem` says.  For probe row i let M(i) be exactly the build rows ivx_probe_overlap_fill pairs
 *      with i for the same (already adjusted) columns: same key, bs <= qe && be >= qs.  Then, one element per probe row in
 *      input order:
 *        count[i] = |M(i)|                       (uint32; what ivx_probe_overlap_count's per_row gives)
 *        sum[i]   = sum of val[b] over M(i)      (int64, two's-complement wrapping)
 *        vmin[i], vmax[i]                        (int64, signed; INT64_MAX / INT64_MIN when M(i) is empty)
 *        bases[i] = sum of len(b, i)             with len = min(qe, be) - max(qs, bs) + 1 in int64, not clamped (the plain
 *                                                closed count: neither coverage's formula nor a union)
 *        wsum[i]  = sum of val[b] * len(b, i)    (int64, wrapping)
 *      A row without a match gets count, sum, bases and wsum 0 and the two identities, on every path.
 *      Every output pointer may be NULL: only the others are computed and stored.  All six NULL, val = NULL with a non-empty
 *      index, or val_bytes other than 4 or 8: IVX_ERR_INVALID.  Another index kind: IVX_ERR_UNSUPPORTED.  n = 0 is a no-op.
 *      The call waits for an index whose build tail still runs, drops the state a count call left for its fill call, and
 *      feeds ivx_ctx_metrics like ivx_probe_count: one input batch, n input and n output rows. */
ivx_status ivx_probe_overlap_agg(ivx_ctx *ctx, const ivx_index *ix, int mem,
                                 const uint32_t *key, const int32_t *start, const int32_t *end, uint64_t n,
                                 const void *val, uint32_t val_bytes,
                                 uint32_t *count, int64_t *sum, int64_t *vmin, int64_t *vmax, int64_t *bases, int64_t *wsum);

/* ---- a4: CountOverlapIndex::query_count in get_count_stream
 *      (interval_tree.rs:41-49, :249-267).  Index kind COUNT. */
ivx_status ivx_probe_count(ivx_ctx *ctx, const ivx_index *ix, int mem,
                           const uint32_t *key, const int32_t *start, const int32_t *end, uint64_t n,
                           int strict, int64_t *out);
/* ---- a5: get_coverage in get_stream (interval_tree.rs:145-152, :181-208).
 *      Index kind COVERAGE. */
ivx_status ivx_probe_coverage(ivx_ctx *ctx, const ivx_index *ix, int mem,
                              const uint32_t *key, const int32_t *start, const int32_t *end, uint64_t n,
                              int strict, int64_t *out);

/* ---- a6: NearestIntervalIndex::nearest_one / nearest_k in get_nearest_stream
 *      (nearest_index.rs:91-235, nearest.rs:330-456) and Algorithm::CoitreesNearest
 *      (interval_join.rs:864-870).  Index kind NEAREST.
 *      Every probe row yields max(1, found) output rows, in probe order:
 *      build_idx (IVX_NULL_IDX = NULL left columns), probe_idx, and if
 *      distance != NULL candidate_distance on the RAW probe coordinates
 *      (-1 = NULL).  cap >= n*max(k,1) always suffices. */
ivx_status ivx_probe_nearest(ivx_ctx *ctx, const ivx_index *ix, int mem,
                             const uint32_t *key, const int32_t *start, const int32_t *end, uint64_t n,
                             int strict, uint32_t k, int include_overlaps,
                             uint32_t *build_idx, uint32_t *probe_idx, int64_t *distance /* nullable */,
                             uint64_t cap, uint64_t *rows);

/* ---- a7+a8: StreamCollector sort + MergeStream sweep
 *      (grouped_stream.rs:50-113, merge.rs:282-350).
 *      Output rows ordered by (key id, start); give key ids in the byte order
 *      of the contig names to reproduce the reference's group order.
 *      cap >= n always suffices. */
ivx_status ivx_merge(ivx_ctx *ctx, int mem,
                     const uint32_t *key /* nullable */, const int64_t *start, const int64_t *end, uint64_t n,
                     uint32_t n_keys, int64_t min_dist, int strict,
                     uint32_t *out_key, int64_t *out_start, int64_t *out_end, int64_t *out_n,
                     uint64_t cap, uint64_t *n_out);

/* ---- a7+a9: SubtractStream / SubtractStreamExtra sweep
 *      (subtract.rs:390-462, :575-655).  out_row (nullable) = the left input row
 *      of each fragment (for the extra-columns `take`).  Passing cap = 0 with
 *      NULL outputs only counts (the sizing call).  The sizing call leaves its
 *      sorted sides and per-row output offsets in the context: a fill call with
 *      the same input pointers, sizes, n_keys, strict and stream that is the next
 *      sort/sweep call on that context runs the output pass only -- the six input
 *      columns must not change between the two calls (the size would be stale
 *      anyway).  The state serves ONE successful fill call (it survives an
 *      IVX_ERR_CAPACITY retry); any other call on the context drops it; a fill call
 *      then (or one made without a sizing call) does all the work itself. */
ivx_status ivx_subtract(ivx_ctx *ctx, int mem,
                        const uint32_t *lkey, const int64_t *lstart, const int64_t *lend, uint64_t nl,
                        const uint32_t *rkey, const int64_t *rstart, const int64_t *rend, uint64_t nr,
                        uint32_t n_keys, int strict,
                        uint32_t *out_key, int64_t *out_start, int64_t *out_end, uint32_t *out_row,
                        uint64_t cap, uint64_t *n_out);

/* ---- INTERSECT: the pieces of every left row that the right side covers (bedtools intersect, pyranges intersect, "my
 *      targets clipped to the callable regions"; the dual of ivx_subtract; the reference has no such table function, so the
 *      contract is stated against ivx_merge and the join's predicate).  Coordinates are int64, key ids < n_keys, strict as
 *      everywhere: 0 weak (closed coordinates), 1 strict (half-open).
 *      Let U = the rows ivx_merge(right, min_dist = 0, strict) returns, (key, ms, me): the right side's merged runs.  The
 *      left rows are taken in (key, start, end, input row) order, the order of ivx_subtract.  A left row (k, ls, le) overlaps
 *      a run of key k iff  ms <= le && me >= ls  (strict: ms < le && me > ls), and for every left row in that order and
 *      every run it overlaps in ascending ms one output row goes out:
 *          (k, max(ls, ms), min(le, me), left input row)
 *      and nothing else.  The output order is thereby fully specified.  A left row whose key has no right row emits
 *      nothing; nr = 0 or nl = 0 gives *n_out = 0 (the rows of the other side are still checked).  start == end is legal
 *      on both sides.  Together with the fragments ivx_subtract gives a left row, its pieces tile [ls, le].
 *      A row with end < start on either side: IVX_ERR_INVALID, "intersect: a row with end < start", nothing written.
 *      Arguments as ivx_subtract: keys nullable on both sides together (one side only, both non-empty: IVX_ERR_INVALID);
 *      fewer than 2^32 - 1 rows per side; a key id >= n_keys is IVX_ERR_INVALID; cap = 0 with NULL outputs only counts;
 *      cap < *n_out is IVX_ERR_CAPACITY with *n_out = the size needed and nothing written; any output may be NULL on its
 *      own.  Drops the state a sizing call of another operation left on the context, and keeps none of its own: the fill
 *      call after a sizing call sorts, merges and counts again.  Work: two sorts, the merge sweep, per left row two
 *      partition points over the runs, one thread per output row. */
ivx_status ivx_intersect(ivx_ctx *ctx, int mem,
                         const uint32_t *lkey, const int64_t *lstart, const int64_t *lend, uint64_t nl,
                         const uint32_t *rkey, const int64_t *rstart, const int64_t *rend, uint64_t nr,
                         uint32_t n_keys, int strict,
                         uint32_t *out_key, int64_t *out_start, int64_t *out_end, uint32_t *out_row,
                         uint64_t cap, uint64_t *n_out);

/* ---- f1: ClusterStream / ClusterStreamExtra (cluster.rs:443-477, :598-661, :813-884) and the
 *      ClusterIdCoordinator offsets (cluster.rs:380-420).  Output has exactly n rows, sorted by
 *      (key, start, end, input row): the sorted row itself (out_key/out_start/out_end, and
 *      out_row = its input row for the extra-columns `take`), the id of its cluster and the
 *      cluster's extent.  Any output may be NULL.  Ids count clusters from 0 in output order
 *      (keys ascending = contig names in byte order); a caller that holds only some of the
 *      contigs (one DataFusion partition, one GPU of a sharded job) passes key_base[n_keys] =
 *      the global id of each key's first cluster, computed from everybody's key_clusters
 *      (out, [n_keys], clusters per key) -- call once with the row outputs NULL to get them.
 *      *n_clusters = clusters in this call. */
ivx_status ivx_cluster(ivx_ctx *ctx, int mem,
                       const uint32_t *key /* nullable */, const int64_t *start, const int64_t *end, uint64_t n,
                       uint32_t n_keys, int64_t min_dist, int strict, const int64_t *key_base /* nullable */,
                       uint32_t *out_key, int64_t *out_start, int64_t *out_end, uint32_t *out_row,
                       int64_t *out_cluster, int64_t *out_cluster_start, int64_t *out_cluster_end,
                       uint64_t *key_clusters /* nullable */, uint64_t *n_clusters);

/* ---- f2: ComplementStream (complement.rs:297-357, :394-465).  Input rows are merged per key
 *      (strict: start < cur_end, else <=), gaps are emitted against the key's view intervals
 *      (vkey/vstart/vend, nv rows; sorted per key, not merged); a key with input rows and no
 *      view row gets the implicit view [0, INT64_MAX).  Output order as the reference: keys
 *      with input rows ascending, then keys that only have view rows (their views, whole).
 *      Passing cap = 0 with NULL outputs only counts. */
ivx_status ivx_complement(ivx_ctx *ctx, int mem,
                          const uint32_t *key /* nullable */, const int64_t *start, const int64_t *end, uint64_t n,
                          const uint32_t *vkey /* nullable */, const int64_t *vstart, const int64_t *vend, uint64_t nv,
                          uint32_t n_keys, int strict,
                          uint32_t *out_key, int64_t *out_start, int64_t *out_end,
                          uint64_t cap, uint64_t *n_out);

/* ---- g: depth(), the pileup crate's coverage blocks (bio-function-pileup: cigar.rs:1-13, :78-132, :177-230;
 *      events.rs:111-137, :181-185; coverage.rs:25-65) from two input groups, either of which may be empty.
 *      READS: read i has rkey[i] (nullable column: one key), rpos[i], rflags[i] / rmapq[i] (nullable columns: every
 *      flag 0 / every mapq passes) and the packed ops cigar_ops[cigar_offsets[i]/4 .. cigar_offsets[i+1]/4), an op being
 *      BAM's u32 (len = w >> 4, code = w & 15).  cigar_offsets[n_reads+1] are the BYTE offsets of an Arrow Binary column
 *      (element 0 need not be 0), cigar_ops that column's data buffer.  A read is skipped when rkey[i] == IVX_NULL_IDX,
 *      it has no ops, (rflags[i] & filter_flag) != 0, or rmapq[i] < min_mapq.  Otherwise, with ref = rpos[i]: codes
 *      0, 7, 8 (M = X) emit (ref, +1), advance ref by len saturating at 2^32-1, and emit (ref, -1); codes 2, 3 (D N)
 *      only advance; every other code does nothing.
 *      WEIGHTED SEGMENTS: segment j emits (sstart[j], +w) and (send[j] + 1 saturating, -w), w = sweight ? sweight[j] : 1
 *      (any int32; send < sstart is not checked; skey[j] == IVX_NULL_IDX skips the segment).  The blocks of an earlier
 *      call, with their coverage as weight, are such segments: that is how coverage accumulates over batches.
 *      key_len (nullable, [n_keys]): the reference's dense mode -- every event with position > key_len[key] is dropped.
 *      BLOCKS, per key ascending: the deltas at equal positions are summed (int32 wrap-around), c_i is the running sum
 *      after the i-th distinct position; every i with c_i != c_(i-1) and c_i != 0 that has a later such change in its
 *      key gives (key, p_i, p_next - 1, c_i) (coverage.rs:38-62).  A key whose coverage never returns to 0 (clipping,
 *      saturation) loses its last open block, as in the reference.  Output is ordered by (key, start).
 *      cap = 0 with NULL outputs only counts; cap < *n_out is IVX_ERR_CAPACITY with *n_out = the size needed; any
 *      output may be NULL on its own.  IVX_ERR_INVALID, found on the device before anything is indexed with the values:
 *      a key id >= n_keys other than IVX_NULL_IDX; offsets that decrease or are not multiples of 4 (the reference's
 *      chunks_exact(4) silently drops a ragged tail instead).  Drops the state a sizing call of another operation left
 *      on the context; nothing is kept between a sizing call and the fill call of this one. */
ivx_status ivx_depth(ivx_ctx *ctx, int mem,
                     const uint32_t *rkey /* nullable */, const uint32_t *rpos,
                     const uint32_t *rflags /* nullable */, const uint32_t *rmapq /* nullable */,
                     const int32_t *cigar_offsets, const uint32_t *cigar_ops, uint64_t n_reads,
                     const uint32_t *skey /* nullable */, const uint32_t *sstart, const uint32_t *send,
                     const int32_t *sweight /* nullable */, uint64_t n_seg,
                     uint32_t n_keys, const uint32_t *key_len /* nullable */, uint32_t filter_flag, uint32_t min_mapq,
                     uint32_t *out_key, uint32_t *out_start, uint32_t *out_end, int32_t *out_cov,
                     uint64_t cap, uint64_t *n_out);

/* ---- g-text: the cigar column as TEXT.  The reference's pileup crate reads `cigar` as Binary (packed ops, above) or as
 *      Utf8 ("5M3D5M": events.rs:42-55, :138-165, :295-321; cigar.rs:78-168); ivx_cigar_parse turns the bytes of an Arrow
 *      Utf8 (large = 0: int32 offsets) or LargeUtf8 (large = 1: int64 offsets) column into the packed form of ivx_depth, on
 *      the device, in one segmented scan over the bytes: no thread walks a read.  text_offsets[n_reads+1] are the column's
 *      offsets (element 0 need not be 0), text its data buffer.
 *      TOKENS, per read and over BYTES (cigar.rs:141-168): every byte that is not '0'..'9' ends a token whose length is the
 *      decimal value of the digits immediately before it, back to the previous non-digit byte or the read's first byte;
 *      no digits give 0, a value >= 2^32 gives 0 (Rust's parse::<u32>() error -> 0), leading zeros are fine.  M I D N S H
 *      P = X emit an op with BAM's codes 0..8; any other non-digit byte ('*', '+', ' ', 'B', a byte >= 0x80) only separates.
 *      Digits after a read's last non-digit byte are dropped (they never reach the next read).  A read without an emitted op
 *      ("*", "", "12") has zero ops, which ivx_depth skips: the reference's output.
 *      OUTPUT: out_offsets[n_reads+1] (nullable) = 4 * (ops emitted by the reads before i), element 0 = 0; out_ops (nullable)
 *      = len << 4 | code in text order; *n_ops = the op count.  The capacity protocol of ivx_depth: cap_ops = 0 with NULL
 *      outputs only counts; cap_ops < *n_ops is IVX_ERR_CAPACITY with *n_ops = the size needed and no op written;
 *      out_offsets is written whenever it is given.
 *      IVX_ERR_INVALID, found on the device before a byte is read through an offset: offsets that are negative or decrease;
 *      2^32 or more bytes between the first and the last offset; more than 2^29-1 ops.  DIVERGENCES from the reference: an
 *      emitted op with 2^28 <= len <= 2^32-1 cannot be packed (nor held by BAM) and is IVX_ERR_INVALID, the text naming the
 *      lowest such read index -- checked on every read, whatever a later filter keeps, and in a counting call too; bytes >=
 *      0x80 are separators, where the reference panics when it slices inside a multi-byte character.
 *      Synchronises (it needs the count); drops the state a sizing call of another operation left on the context; is not
 *      counted in ivx_metrics; n_reads = 0 is a no-op with *n_ops = 0. */
ivx_status ivx_cigar_parse(ivx_ctx *ctx, int mem, int large, const void *text_offsets, const uint8_t *text, uint64_t n_reads,
                           int32_t *out_offsets /* [n_reads+1], nullable */, uint32_t *out_ops /* nullable */,
                           uint64_t cap_ops, uint64_t *n_ops);
/*      ivx_depth with (large, text_offsets, text) in place of (cigar_offsets, cigar_ops): the text is staged (IVX_MEM_HOST:
 *      the bytes between the first and the last host offset), parsed into context scratch, and ivx_depth runs on the result.
 *      Contract, errors, metrics and memory-limit accounting are those of ivx_depth (the scratch of the parse counts against
 *      the limit); the IVX_ERR_INVALID cases of ivx_cigar_parse come on top. */
ivx_status ivx_depth_text(ivx_ctx *ctx, int mem,
                          const uint32_t *rkey /* nullable */, const uint32_t *rpos,
                          const uint32_t *rflags /* nullable */, const uint32_t *rmapq /* nullable */,
                          int large, const void *text_offsets, const uint8_t *text, uint64_t n_reads,
                          const uint32_t *skey /* nullable */, const uint32_t *sstart, const uint32_t *send,
                          const int32_t *sweight /* nullable */, uint64_t n_seg,
                          uint32_t n_keys, const uint32_t *key_len /* nullable */, uint32_t filter_flag, uint32_t min_mapq,
                          uint32_t *out_key, uint32_t *out_start, uint32_t *out_end, int32_t *out_cov,
                          uint64_t cap, uint64_t *n_out);

/* ---- g': per-base depth(), the pileup crate's per_base = true form (bio-function-pileup table_function.rs:97-123,
 *      coverage.rs:271-365 PerBaseEmitter, physical_exec.rs:404-414, :517-548): one (position, coverage Int16) row per base.
 *      It cannot be made from ivx_depth's blocks -- a key whose coverage never returns to 0 loses its last open block, and a
 *      key whose events all cancel has no block at all, yet the reference emits both -- so the step function itself is kept
 *      on the device, as a DEPTH PROFILE, and windows of it are expanded to positions.
 *      A profile is an ivx_index of kind IVX_KIND_DEPTH_PROFILE: immutable after the build, readable and expandable by any
 *      context on the same device, its device bytes reserved against the building context's memory limit until it is freed
 *      (ivx_ctx_reserved_bytes shows them); a build that would go over the limit returns IVX_ERR_OOM.  ivx_index_build does
 *      not make one, the probes refuse one (IVX_ERR_UNSUPPORTED), and the calls below refuse any other index.
 *      build: the 17 input arguments of ivx_depth, with the same checks and the same IVX_ERR_INVALID cases; drops the state a
 *      sizing call of another operation left on the context.  STEPS: with p_i, g_i, c_i as for ivx_depth's blocks, position
 *      i is a step iff g_i != 0 (that is c_i != c_(i-1), c_(-1) = 0); the profile holds (key, p_i, c_i) ordered by (key,
 *      position), the first step of every key, and key_seen[k] = 1 iff key k keeps at least one event after the read filter
 *      and the key_len clipping, whether or not those events cancel (the reference's "touched" contig: events.rs:198-206,
 *      physical_exec.rs:378-382).  A call without any event gives a valid empty profile. */
ivx_status ivx_depth_profile_build(ivx_ctx *ctx, int mem,
                                   const uint32_t *rkey /* nullable */, const uint32_t *rpos,
                                   const uint32_t *rflags /* nullable */, const uint32_t *rmapq /* nullable */,
                                   const int32_t *cigar_offsets, const uint32_t *cigar_ops, uint64_t n_reads,
                                   const uint32_t *skey /* nullable */, const uint32_t *sstart, const uint32_t *send,
                                   const int32_t *sweight /* nullable */, uint64_t n_seg,
                                   uint32_t n_keys, const uint32_t *key_len /* nullable */, uint32_t filter_flag, uint32_t min_mapq,
                                   ivx_index **out);
/*      ivx_depth_profile_build with the cigar column as text: see ivx_depth_text. */
ivx_status ivx_depth_profile_build_text(ivx_ctx *ctx, int mem,
                                        const uint32_t *rkey /* nullable */, const uint32_t *rpos,
                                        const uint32_t *rflags /* nullable */, const uint32_t *rmapq /* nullable */,
                                        int large, const void *text_offsets, const uint8_t *text, uint64_t n_reads,
                                        const uint32_t *skey /* nullable */, const uint32_t *sstart, const uint32_t *send,
                                        const int32_t *sweight /* nullable */, uint64_t n_seg,
                                        uint32_t n_keys, const uint32_t *key_len /* nullable */, uint32_t filter_flag, uint32_t min_mapq,
                                        ivx_index **out);
/*      Same contract as ivx_index_free (synchronise every context that expanded it in device mode first). */
void       ivx_depth_profile_free(ivx_index *profile);
uint64_t   ivx_depth_profile_steps(const ivx_index *profile);
uint64_t   ivx_depth_profile_device_bytes(const ivx_index *profile);
/*      Copy the steps out (tests, diagnostics, accumulation).  cap = 0 with NULL outputs only counts; cap < *n_out is
 *      IVX_ERR_CAPACITY with *n_out = the size needed; any output may be NULL on its own.  key_seen (nullable, [n_keys],
 *      where `mem` says) is written whenever it is given. */
ivx_status ivx_depth_profile_read(ivx_ctx *ctx, const ivx_index *profile, int mem,
                                  uint32_t *out_key, uint32_t *out_pos, int32_t *out_cov,
                                  uint8_t *key_seen /* nullable */, uint64_t cap, uint64_t *n_out);
/*      The window [first_pos, first_pos + n) of `key`, for i < n and p = first_pos + i:
 *        out_pos[i] = (int32_t)p                           (int32_t[n], nullable)
 *        out_cov[i] = (int16_t)(C(p) - c0), int32 wrap     (int16_t[n], nullable)
 *      C(p) = the c of the key's last step at a position <= p, 0 if there is none; c0 = the c of the key's step at
 *      position 0 when skip_pos0 is set and that step exists, else 0 -- the reference's 1-based emitter starts at index 1
 *      and never adds depth[0] (coverage.rs:294-301).  A key without steps gives zeros; n = 0 is a no-op.
 *      IVX_ERR_INVALID: key >= n_keys; first_pos + n > 2^32; in device mode a pointer that is not aligned to its element.
 *      Both columns leave in 16-byte stores whatever the alignment of the two pointers; only the window's first and last
 *      partial 16 bytes are written element by element.  IVX_MEM_DEVICE calls may return with the kernel in flight. */
ivx_status ivx_depth_profile_expand(ivx_ctx *ctx, const ivx_index *profile, int mem,
                                    uint32_t key, uint32_t first_pos, uint64_t n, int skip_pos0,
                                    int32_t *out_pos /* nullable */, void *out_cov /* int16_t[n], nullable */);

/*      STREAMING depth(): the reference drains a stream of read batches into one accumulator per partition and adds the
 *      partitions' accumulators together before anything is emitted (physical_exec.rs:269-329 accumulate_partition,
 *      :367-463 merge_dense_results / merge_sparse_results).  A profile is that accumulator: coverage is additive, so
 *      out = a + b is the profile of the union of the inputs that made a and b, by a merge of the two sorted step lists.
 *      MERGE.  Let w = key << 32 | pos.  The merged positions are the union of both lists' w; for a merged w of key k,
 *      c(w) = CA(w) + CB(w) with int32 wrap-around, CX(w) = the c of X's last step with the same key and a position <= pos
 *      (0 if there is none), and prev(w) = the same sum over the steps at positions < pos; w is a step of the result iff
 *      c(w) != prev(w).  A position present in both lists appears once.  n_keys of the result = the larger of the two (the
 *      profile with fewer keys has no steps for the higher ones), key_seen = a.key_seen | b.key_seen with missing keys
 *      counting as 0, and the first step of every key is found again.  a == b is allowed: the inputs are only read, stay
 *      valid and stay the caller's to free.  The result is a normal profile, reserved against ctx's memory limit until it
 *      is freed; a merge that would go over the limit returns IVX_ERR_OOM, keeps nothing allocated and leaves
 *      ivx_ctx_reserved_bytes as it was.  Errors: a null profile or one on another device is IVX_ERR_INVALID, any other
 *      index IVX_ERR_UNSUPPORTED; steps(a) + steps(b) >= 0xFFFFFF00 is IVX_ERR_INVALID (the merged index space is 32-bit,
 *      like the expand kernel's search).  Drops the state a sizing call left on the context, synchronises before it returns
 *      (it needs the step count anyway) and adds the result's bytes to build_mem_used. */
ivx_status ivx_depth_profile_merge(ivx_ctx *ctx, const ivx_index *a, const ivx_index *b, ivx_index **out);
/*      The coverage blocks of a profile: what ivx_depth returns for the inputs that made it.  Step i gives the block
 *      (key_i, p_i, p_(i+1) - 1, c_i) iff c_i != 0 and step i + 1 exists and has the same key (coverage.rs:38-62 restated on
 *      steps: a key's last step never gives a block).  Output is ordered by (key, start).  The capacity protocol of
 *      ivx_depth: cap = 0 with NULL outputs only counts; cap < *n_out is IVX_ERR_CAPACITY with *n_out = the size needed and
 *      nothing written; any output may be NULL on its own.  IVX_MEM_DEVICE calls may return with kernels in flight. */
ivx_status ivx_depth_profile_blocks(ivx_ctx *ctx, const ivx_index *profile, int mem,
                                    uint32_t *out_key, uint32_t *out_start, uint32_t *out_end, int32_t *out_cov,
                                    uint64_t cap, uint64_t *n_out);

/*      REGION SUMMARIES of a profile: bases, coverage sum and bases at or above each threshold per region -- mean depth per
 *      target, bases at 10x / 20x / 30x, coverage in fixed bins (samtools bedcov, mosdepth --by / --thresholds; the
 *      reference has nothing here beyond coverage(), which counts merged build intervals, not read depth).
 *      With C(p) and c0(k) as for ivx_depth_profile_expand, v(p) = (int32)(C(p) - c0(k)) with int32 wrap-around: expand's
 *      value BEFORE its cast to Int16; the summaries use the exact int32.  The domain of key k is D(k) = [pos_lo,
 *      key_hi ? key_hi[k] : 2^32-1], empty if key_hi[k] < pos_lo.  Region i is the closed interval [qstart[i], qend[i]] on
 *      qkey[i] intersected with D(qkey[i]): R_i, empty when qend[i] < qstart[i], when qkey[i] == IVX_NULL_IDX or when the
 *      domain cuts it away.
 *        out_len[i]       = |R_i|                                     (int64_t[n], nullable)
 *        out_sum[i]       = sum of v(p) over p in R_i                 (int64_t[n], nullable; always fits: 2^32 * 2^31 <= 2^63)
 *        out_ge[j*n + i]  = #{p in R_i : v(p) >= thresholds[j]}       (int64_t[n_thr * n], threshold-major, nullable)
 *      The zero-coverage stretches before a key's first step and on a key without steps count whenever thresholds[j] <= 0.
 *      A key's last step extends to the end of its domain (the open block of a clipped or saturated contig that ivx_depth
 *      drops).  Output order = input order; n = 0 is a no-op; any output may be NULL on its own; a valid empty profile
 *      gives zeros and the lengths.  thresholds is HOST memory in both modes.  key_hi: [n_keys], where `mem` says.
 *      IVX_ERR_INVALID: a key id >= n_keys other than IVX_NULL_IDX (found on the device before it indexes anything, as in
 *      ivx_depth; nothing is written then); n_thr > IVX_DEPTH_MAX_THRESHOLDS; in device mode a pointer that is not aligned
 *      to its element.  IVX_ERR_UNSUPPORTED: any index that is not a profile.  Usable from any context on the profile's
 *      device; IVX_MEM_DEVICE calls may return with kernels in flight; drops the state a sizing call of another operation
 *      left on the context; the scratch (8 * (1 + n_thr) bytes per 1024 steps, and the staged columns in host mode) counts
 *      against the context's memory limit.  Cost per region: two searches in the key's steps and at most two tiles of
 *      steps, whatever the region's length. */
#define IVX_DEPTH_MAX_THRESHOLDS 8
ivx_status ivx_depth_profile_summarize(ivx_ctx *ctx, const ivx_index *profile, int mem,
                                       const uint32_t *qkey /* nullable: every region on key 0 */, const uint32_t *qstart, const uint32_t *qend, uint64_t n,
                                       uint32_t pos_lo, const uint32_t *key_hi /* nullable */, int skip_pos0,
                                       const int32_t *thresholds /* host memory */, uint32_t n_thr,
                                       int64_t *out_len /* nullable */, int64_t *out_sum /* nullable */, int64_t *out_ge /* nullable */);
/*      The same three outputs for n fixed-width windows of one key: window i = [first_pos + i * width, first_pos + i * width
 *      + width - 1] intersected with [first_pos, last_pos] (the domain is the whole position range); no region arrays are
 *      made.  With width = 1 it is ivx_depth_profile_expand in int32.  IVX_ERR_INVALID: width = 0; key >= n_keys;
 *      first_pos + (n - 1) * width > 2^32 - 1; and the cases above. */
ivx_status ivx_depth_profile_windows(ivx_ctx *ctx, const ivx_index *profile, int mem, uint32_t key,
                                     uint32_t first_pos, uint32_t last_pos, uint32_t width, uint64_t n, int skip_pos0,
                                     const int32_t *thresholds /* host memory */, uint32_t n_thr,
                                     int64_t *out_len /* nullable */, int64_t *out_sum /* nullable */, int64_t *out_ge /* nullable */);

/*      REGION ORDER STATISTICS of a profile: the smallest and the largest per-base coverage of a region and up to 8 of its
 *      quantiles -- minimum coverage per target, median depth per target or bin (bedtools map -o min,max, Picard MIN_ /
 *      MEDIAN_TARGET_COVERAGE, mosdepth --use-median).  Exact and bit-reproducible.  v(p), D(k), R_i, the zero stretches,
 *      the last step that extends to the end of its domain, skip_pos0 and the null key are those of REGION SUMMARIES above.
 *      With L = |R_i| > 0:
 *        out_len[i]       = L                                         (int64_t[n], nullable)
 *        out_min[i]       = min of v(p) over p in R_i                 (int32_t[n], nullable)
 *        out_max[i]       = max of v(p) over p in R_i                 (int32_t[n], nullable)
 *        out_q[j*n + i]   = element r of the L values v(p), p in R_i, sorted ascending,
 *                           r = floor((L - 1) * q_num[j] / q_den)     (int32_t[n_q * n], quantile-major, nullable)
 *      in integers (L - 1 < 2^32, q_num <= 2^16): the "lower" quantile, the lower median for q = 1/2 and an even L; q_num = 0
 *      is the minimum and q_num = q_den the maximum.  L = 0 (an empty region, the null key, a domain that cuts the region
 *      away) gives 0 in all three, and out_len tells.  Output order = input order; n = 0 is a no-op; any output may be NULL
 *      on its own.  q_num is HOST memory in both modes.
 *      IVX_ERR_INVALID: n_q > IVX_DEPTH_MAX_QUANTILES; q_den = 0 or q_den > 65536; a q_num[j] > q_den; and every case of
 *      ivx_depth_profile_summarize / _windows (a key id >= n_keys is found on the device before it indexes anything, and
 *      nothing is written then; out_len aligned to 8 bytes, the other pointers to 4 in device mode; width = 0, ...).
 *      IVX_ERR_UNSUPPORTED: any index that is not a profile.  Usable from any context on the profile's device;
 *      IVX_MEM_DEVICE calls may return with kernels in flight; no host round trip between the kernels of a call beyond the
 *      key check's; drops the state a sizing call of another operation left on the context.  Scratch, counted against the
 *      context's memory limit: 8 bytes per 1024 steps and level of a sparse table of (min, max), at most log2(steps / 1024)
 *      levels; 24 bytes per region when quantiles are asked for; the staged columns in host mode.
 *      Cost per region: min and max take two searches in the key's steps, at most two tiles of steps and two table entries,
 *      whatever the region's length; so do the quantiles of a region of at most 64 segments (its steps, plus the zero
 *      stretch ahead of the key's first step), ranked in one wavefront's registers.  A region of more segments is selected
 *      by one workgroup in 1 to 4 passes over its steps (one per 8 bits of max - min; a coverage span below 256 is one pass
 *      for all quantiles): linear in the region's steps, times the passes. */
#define IVX_DEPTH_MAX_QUANTILES 8
ivx_status ivx_depth_profile_quantiles(ivx_ctx *ctx, const ivx_index *profile, int mem,
                                       const uint32_t *qkey /* nullable: every region on key 0 */, const uint32_t *qstart, const uint32_t *qend, uint64_t n,
                                       uint32_t pos_lo, const uint32_t *key_hi /* nullable */, int skip_pos0,
                                       const uint32_t *q_num /* host memory */, uint32_t n_q, uint32_t q_den,
                                       int64_t *out_len /* nullable */, int32_t *out_min /* nullable */, int32_t *out_max /* nullable */,
                                       int32_t *out_q /* nullable */);
/*      The same four outputs for the windows of ivx_depth_profile_windows.  With width = 1, min = max = every quantile =
 *      ivx_depth_profile_expand in int32. */
ivx_status ivx_depth_profile_window_quantiles(ivx_ctx *ctx, const ivx_index *profile, int mem, uint32_t key,
                                              uint32_t first_pos, uint32_t last_pos, uint32_t width, uint64_t n, int skip_pos0,
                                              const uint32_t *q_num /* host memory */, uint32_t n_q, uint32_t q_den,
                                              int64_t *out_len /* nullable */, int32_t *out_min /* nullable */, int32_t *out_max /* nullable */,
                                              int32_t *out_q /* nullable */);

/*      COVERAGE CLASSES of a profile: every base classified by its coverage -- the maximal intervals whose coverage stays in
 *      one class (mosdepth --quantize, GATK CallableLoci, "the intervals at 10x or more"), and per key the number of bases at
 *      each coverage value (bedtools genomecov's default output, mosdepth's dist, the histogram of Picard CollectWgsMetrics;
 *      the reference has neither).  v(p), c0(k), skip_pos0, pos_lo, key_hi, the domain D(k), the zero stretch before a key's
 *      first step, the keys without steps (v = 0 on the whole domain) and the last step that extends to the end of its
 *      domain are those of REGION SUMMARIES above.  seen_only != 0: a key with key_seen[k] == 0 does not take part (the
 *      reference's "touched" contig, as its per-base emitter uses it); seen_only = 0: every key < n_keys with a non-empty
 *      domain takes part.  An empty profile is valid: all its keys are keys without steps.
 *      QUANTIZE.  class(v) = the number of cuts <= v, in 0 .. n_cuts: class 0 is v < cuts[0], class j is cuts[j-1] <= v <
 *      cuts[j], class n_cuts is v >= cuts[n_cuts-1]; with n_cuts = 0 everything is class 0.  For each key that takes part, in
 *      ascending order, the output is the maximal runs of consecutive positions of D(k) with the same class, as closed
 *      intervals [out_start, out_end] with out_class, ordered by (key, start).  A run goes out iff bit `class` of emit_mask
 *      is set; the runs of a class that is not emitted still separate their neighbours.  The result is an interval set:
 *      ivx_subtract, ivx_complement, the overlap join and ivx_probe_overlap_agg take it as input.  cuts is HOST memory in
 *      both modes.  The capacity protocol of ivx_depth_profile_blocks: the count is always made and read back; cap = 0 with
 *      NULL outputs only counts; cap < *n_out is IVX_ERR_CAPACITY with *n_out = the size needed and nothing written; any
 *      output may be NULL on its own.
 *      IVX_ERR_INVALID: n_cuts > IVX_DEPTH_MAX_CUTS; cuts not strictly ascending; a bit of emit_mask above n_cuts; in device
 *      mode a pointer that is not aligned to its element.  IVX_ERR_UNSUPPORTED: any index that is not a profile.
 *      HIST.  out_hist[k * n_bins + b] = #{p in D(k) : clamp((int64)v(p) - v_lo, 0, n_bins - 1) = b} (int64_t[n_keys *
 *      n_bins], key-major): the first bin takes everything at or below v_lo, the last one everything at or above v_lo +
 *      n_bins - 1.  Every element is written: a key that does not take part, or whose domain is empty, gets zeros.
 *      IVX_ERR_INVALID: n_bins = 0 or n_bins > IVX_DEPTH_MAX_BINS; in device mode a pointer that is not aligned to its
 *      element.  IVX_ERR_UNSUPPORTED as above.
 *      Both: usable from any context on the profile's device; drop the state a sizing call of another operation left on the
 *      context; IVX_MEM_DEVICE calls may return with kernels in flight (quantize has read back its count by then); key_hi:
 *      [n_keys], where `mem` says.  Scratch, counted against the context's memory limit: quantize 16 bytes per key and 8
 *      bytes per 1024 steps; hist none; the staged columns in host mode.  Cost: a quantize sizing call reads the step list
 *      once, a fill call three times (its own count, then the scan that writes); hist reads it once.
 *      Not built: distributions or runs restricted to a region set, a minimum run length, labels for the classes, float
 *      output (cumulative fractions are the caller's division). */
#define IVX_DEPTH_MAX_CUTS 31
ivx_status ivx_depth_profile_quantize(ivx_ctx *ctx, const ivx_index *profile, int mem,
                                      uint32_t pos_lo, const uint32_t *key_hi /* nullable */, int skip_pos0, int seen_only,
                                      const int32_t *cuts /* host memory, strictly ascending */, uint32_t n_cuts, uint32_t emit_mask,
                                      uint32_t *out_key, uint32_t *out_start, uint32_t *out_end, uint32_t *out_class,
                                      uint64_t cap, uint64_t *n_out);
#define IVX_DEPTH_MAX_BINS 65536
ivx_status ivx_depth_profile_hist(ivx_ctx *ctx, const ivx_index *profile, int mem,
                                  uint32_t pos_lo, const uint32_t *key_hi /* nullable */, int skip_pos0, int seen_only,
                                  int32_t v_lo, uint32_t n_bins, int64_t *out_hist /* [n_keys * n_bins], key-major */);

/* ---- f3: `compute::take` of payload columns with the index arrays the probes return
 *      (interval_join.rs:1655-1667, nearest.rs:469-482).  idx[i] == IVX_NULL_IDX or a null source
 *      slot (src_valid_bits: Arrow validity bitmap of the source, bit offset 0, nullable) gives
 *      out_valid[i] = 0 (one byte per output row, nullable) and zero bytes / an empty string;
 *      any other idx[i] >= n_src is IVX_ERR_INVALID.
 *      fixed: width = bytes per element, one of 1, 2, 4, 8, 16, 32. */
ivx_status ivx_take_fixed(ivx_ctx *ctx, int mem, const void *src, uint32_t width, uint64_t n_src,
                          const uint8_t *src_valid_bits, const uint32_t *idx, uint64_t n,
                          void *out, uint8_t *out_valid);

/*      The inverse: out[idx[i]] = src[i] for i < n (idx[i] >= n_out is IVX_ERR_INVALID; rows no index names keep their
 *      contents; equal indices: one of the values).  What puts a per-row result column (count_overlaps, coverage,
 *      nearest) computed on a SHARD of the probe rows back in the order of the whole input -- the reference's partitioned
 *      forms return their batches in stream order (count_overlaps.rs:143-153, R/tests/integration_test.rs:3783-3890);
 *      with contigs sharded over GPUs the rows come back as (row, value) lists instead. */
ivx_status ivx_scatter_fixed(ivx_ctx *ctx, int mem, const void *src, uint32_t width, const uint32_t *idx, uint64_t n,
                             void *out, uint64_t n_out);

/*      Boolean columns (bit-packed, LSB first): out_bits gets (n+7)/8 bytes. */
ivx_status ivx_take_bits(ivx_ctx *ctx, int mem, const uint8_t *src_bits, uint64_t n_src, const uint8_t *src_valid_bits,
                         const uint32_t *idx, uint64_t n, uint8_t *out_bits, uint8_t *out_valid);

/*      Utf8 / Binary (large = 0, int32 offsets) and LargeUtf8 / LargeBinary (large = 1, int64).
 *      out_offsets[n+1] is written whenever given; *data_bytes always returns the bytes needed.
 *      out_data = NULL sizes only; data_cap < *data_bytes is IVX_ERR_CAPACITY, which still leaves
 *      out_offsets and out_valid written, in either memory mode.  More than 2^31-1 bytes with
 *      int32 offsets is IVX_ERR_INVALID and writes no offsets. */
ivx_status ivx_take_utf8(ivx_ctx *ctx, int mem, int large, const void *offsets, const uint8_t *data, uint64_t n_src,
                         uint64_t src_data_bytes, const uint8_t *src_valid_bits, const uint32_t *idx, uint64_t n,
                         void *out_offsets, uint8_t *out_data, uint64_t data_cap, uint64_t *data_bytes,
                         uint8_t *out_valid);

/*      Utf8View / BinaryView: views = [n_src] 16-byte views, data_bufs[n_bufs] the variadic data buffers
 *      with their sizes.  The output is self-contained: out_views[n] plus ONE data buffer holding the
 *      gathered strings longer than 12 bytes (views rewritten to buffer 0).  out_data = NULL sizes only
 *      (*data_bytes); more than 2^31-1 gathered bytes is IVX_ERR_UNSUPPORTED. */
ivx_status ivx_take_view(ivx_ctx *ctx, int mem, const void *views, const uint8_t *const *data_bufs, const uint64_t *data_buf_bytes,
                         uint32_t n_bufs, uint64_t n_src, const uint8_t *src_valid_bits, const uint32_t *idx, uint64_t n,
                         void *out_views, uint8_t *out_data, uint64_t data_cap, uint64_t *data_bytes, uint8_t *out_valid);

#ifdef __cplusplus
}
#endif
#endif
