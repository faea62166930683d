// ivx_scalars.hpp -- the context's scalar words: ivx_ctx::d_scalars (SC_DEVICE_WORDS 64-bit device words) and h_scalars, its
// pinned and device-mapped mirror (SC_HOST_WORDS words; hd_scalars is its device pointer).  Flags, totals, ranges and headers
// travel between device and host through them.  Included by ivx_internal.hpp, behind ivx_ctx and the HDR_* words.
//
// The rule.  Every word has ONE owner, named here; the table is laid out by arithmetic, so two owners cannot overlap.
//   call-local   dead when the API call that wrote it returns: whoever uses it clears it first and reads it back before it
//                returns.  Callees have words of their own (the radix sort under the sweeps, depth(), the nearest build and the
//                two-level routing; the CIGAR parse ahead of depth()), so no caller's word changes under it.
//   outlives     read by a later call: nothing else may ever write it.
// A word below SC_DEVICE_WORDS exists on both sides, mirror word w belonging to device word w; "host only" words live in the
// mirror alone (landing places of copies from scratch, pinned sources of host-to-device copies, headers).
// Every range laid over several words has a static_assert on its size or adjacency: below where the type is visible here,
// else (IVX_SC_FITS) next to the type's definition.  A block that ONE memset clears starts on an even word: the runtime clears
// whole 16-byte lines with one fill kernel and a ragged head or tail with one more each (seen in kernel traces).
#pragma once

enum { SC_SORT_FIELDS = 8 };            // most fields of one radix sort (ivx_radix_sort)
enum { SC_LENHIST_N = 34 };             // length-class counters of the join build (k_keystats -> k_join_layout), u32 each

enum {
    // ---- overlap probes (ivx_capi.hip: probe_impl; the probe kernels get the pair as `d_cursor`).  Call-local.  The lean fill's
    // last kernel (k_fill_rest) stores both HOST words itself, through hd_scalars: no sharing, and they stay words 0 and 1.
    SC_PAIRS = 0,                               // 1 word, u64: the pair cursor = the call's total
    SC_FAULT = SC_PAIRS + 1,                    // 1 word, u64: != 0: a probe met an unpublished page of routed rows
    // ---- merge sweeps (ivx_runs.hip).  Call-local.
    SC_RUNS = SC_FAULT + 1,                     // 1 word, u64: the runs found
    // ---- overlap index build (ivx_join.hip: ivx_join_build; its length-class counters are SC_JOIN_LENHIST below).  Call-local:
    // cleared by the key statistics' first kernel, read by k_join_layout (which passes it on as HDR_BADKEY of the header).
    SC_JOIN_BAD = SC_RUNS + 1,                  // 1 word, u32: a build key id >= n_keys
    // ---- routing pass (ivx_regions_route.hip: flat and two-level).  OUTLIVES its call: ivx_routed::unsorted points here, and a
    // count call leaves that in ivx_ctx::join_plan for the fill call that follows.  No other writer, ever.
    SC_UNSORTED = SC_JOIN_BAD + 1,              // 1 word, u32: != 0: the rows were moved (0: they came in region order)
    // ---- region fill (ivx_regions_probe.hip: probe_pairs).  Call-local.
    SC_BSEL = SC_UNSORTED + 1,                  // 1 word, u32: the rows-per-lane variant k_pick_rows chose
    // ---- take and marks (ivx_take.hip, ivx_marks.hip).  Call-local.
    SC_TAKE_BAD = SC_BSEL + 1,                  // 1 word, u32: an index out of range
    SC_MARK_BAD = SC_TAKE_BAD + 1,              // 1 word, u32: bits_mark: an index out of range
    // ---- count / coverage / nearest builds and the rank grids under them (ivx_ops32.hip, ivx_grid.hip).  Call-local.  One
    // family, one flag: the builds clear it, ivx_grid_build's key statistics raise it, the builds read it back.  The four words
    // are adjacent: the count build clears two, the nearest build fetches all four at once.
    SC_BUILD_FLAG = SC_MARK_BAD + 1,            // 1 word, u32[2]: [0] key id >= n_keys, [1] unsorted / a run too long / end < start
    SC_BUILD_INVERTED = SC_BUILD_FLAG + 1,      // 1 word, u32: count build: some row has end < start
    SC_NEAR_HDR = SC_BUILD_INVERTED + 1,        // 2 words, u32[3]: nearest build (k_nlin_layout): position bits, row bits, usable
    // ---- sweeps: merge / subtract / intersect / cluster / complement and sort64 under them (ivx_sweep.hip).  Call-local.  One family, one
    // flag: the operator clears it, sort64 raises it and reads its upper half, the operator reads it back at its end.
    SC_SWEEP_FLAG = SC_NEAR_HDR + 2,            // 1 word, u32[2]: [0] key id >= n_keys, [1] a (key, start) run too long to repair
                                                // (intersect with one side empty, which sorts nothing: [1] a row with end < start)
    SC_SWEEP_IRREGULAR = SC_SWEEP_FLAG + 1,     // 1 word, u32: complement: the merged runs are not disjoint and ascending (cleared with the flag)
    // ---- depth regions (ivx_depth_regions.hip) and the text CIGARs' write pass (ivx_cigar.hip).  Call-local.
    SC_REGIONS_BAD = SC_SWEEP_IRREGULAR + 1,    // 1 word, u64: a region's key id >= n_keys
    SC_CIG_BADREAD = SC_REGIONS_BAD + 1,        // 1 word, u64: the first read with an op length that cannot be packed, or ~0
    // ---- radix sort (ivx_sort.hip), a callee of the sweeps, the builds, depth() and the routing.  Call-local.
    SC_SORT_VAR = SC_CIG_BADREAD + 1,           // SC_SORT_FIELDS words, u64 each: the bits that vary, per field
    // ---- sort64 (ivx_sweep.hip).  Call-local, but for the host copy of SC_RANGE, which subtract and intersect read once more
    // after sort64 returned (inside the same subtract / intersect call, before its next sort64).
    SC_RANGE = SC_SORT_VAR + SC_SORT_FIELDS,    // 6 words, Range64: the value ranges of the rows
    SC_LIN = SC_RANGE + 6,                      // 2 words, u64[2]: {usable, positions} of the linearised sort word; fetched with SC_RANGE
    // ---- depth() (ivx_depth.hip: ivx_depth_events, ivx_depth_device).  Call-local.  Six words cleared and fetched as one.
    SC_DEPTH_BAD = SC_LIN + 2,                  // 1 word, u32: 1 bad offsets, 2 key id >= n_keys
    SC_DEPTH_MAXPOS = SC_DEPTH_BAD + 1,         // 1 word, u32: the largest event position
    SC_DEPTH_TOTAL = SC_DEPTH_MAXPOS + 1,       // 1 word, u64: coverage blocks
    SC_DEPTH_OFF0 = SC_DEPTH_TOTAL + 1,         // 1 word, u64: the first CIGAR offset
    SC_DEPTH_OFFN = SC_DEPTH_OFF0 + 1,          // 1 word, u64: the last one
    SC_DEPTH_SPARE = SC_DEPTH_OFFN + 1,         // 1 word, unused: six words are three whole 16-byte lines, so one fill kernel clears the block
    // ---- depth profiles (ivx_depth_expand.hip, ivx_depth_merge.hip).  Call-local.
    SC_STEPS_TOTAL = SC_DEPTH_SPARE + 1,        // 1 word, u64: steps of a new profile
    SC_BLOCKS_TOTAL = SC_STEPS_TOTAL + 1,       // 1 word, u64: coverage blocks of a profile
    // ---- text CIGARs (ivx_cigar.hip), run ahead of depth(): the check pass.  Call-local.  Cleared and fetched as one.
    SC_CIG_BAD = SC_BLOCKS_TOTAL + 1,           // 1 word, u32: offsets descend or are negative
    SC_CIG_OFF0 = SC_CIG_BAD + 1,               // 1 word, u64: the first text offset
    SC_CIG_OFFN = SC_CIG_OFF0 + 1,              // 1 word, u64: the last one
    // ---- overlap index build, see SC_JOIN_BAD
    SC_JOIN_LENHIST = SC_CIG_OFFN + 1,          // SC_LENHIST_N u32: rows per length class
    // ---- depth region order statistics (ivx_depth_rank.hip).  Call-local: cleared ahead of the query kernel, read by the select
    // kernel on the device only.
    SC_RANK_LONG = SC_JOIN_LENHIST + (SC_LENHIST_N + 1) / 2,        // 1 word, u64: regions of more than 64 segments listed for the select kernel
    SC_DEVICE_WORDS = SC_RANK_LONG + 1,         // ---- length of d_scalars

    // ---- host only
    SC_LANDING = SC_DEVICE_WORDS,               // SC_LANDING_WORDS words, any T: where ivx_ctx::fetch_wait(src, ...) lands a value from scratch; dead when it returns
    SC_LANDING_WORDS = 3,
    SC_COMP_IMPLICIT = SC_LANDING + SC_LANDING_WORDS,   // 1 word, u32: complement: implicit views, fetched ahead of the key flag's wait.  Call-local.
    SC_RANGE_INIT = SC_COMP_IMPLICIT + 1,       // 6 words, Range64: sort64's initialiser, the pinned source of its copy to SC_RANGE.  Call-local.
    SC_TAKE_TOTAL = SC_RANGE_INIT + 6,          // 1 word, u64: take: gathered bytes, fetched ahead of the index flag's wait.  Call-local.
    SC_CIG_IDENT = SC_TAKE_TOTAL + 1,           // 3 words, CigState: the CIGAR scan's identity, the pinned source of a copy to scratch.  Call-local.
    SC_ROUTE_HDR = SC_CIG_IDENT + 3,            // HDR_WORDS u32: a routing view's header (ivx_route_view_build), read by ivx_route_view_ready behind the
                                                // build's next wait.  Dead when the build call returns.
    // The header of the overlap index built last (ivx_join_build; k_join_layout and k_join_regdesc store it through hd_scalars).
    // OUTLIVES the build: the first region probe of an index built with its tail overlapped reads HDR_SLOW here
    // (ivx_ctx::hdr_mirror_serial says whose header it is).  No other writer, ever.
    SC_HDR_MIRROR = SC_ROUTE_HDR + (HDR_WORDS + 1) / 2,     // HDR_WORDS u32
    SC_HOST_WORDS = SC_HDR_MIRROR + (HDR_WORDS + 1) / 2     // ---- length of h_scalars
};

// The words that outlive their call, in ascending order, as {first word, words}: every word above whose comment says OUTLIVES,
// and no other, each with the length the table gives it (tests/test_scalar_words.py compares both).  The test hook ivx_debug_poison (ivx_capi.hip) overwrites every word of both
// arrays but these.
struct ivx_sc_span { int first, words; };
static constexpr ivx_sc_span SC_OUTLIVES[] = {{SC_UNSORTED, 1}, {SC_HDR_MIRROR, (HDR_WORDS + 1) / 2}};
static_assert(SC_OUTLIVES[0].first + SC_OUTLIVES[0].words <= SC_OUTLIVES[1].first && SC_OUTLIVES[1].first + SC_OUTLIVES[1].words <= SC_HOST_WORDS,
              "the outliving words ascend and lie inside the host words");

// the blocks that one memset or one copy covers, in words
enum { SC_BUILD_WORDS = SC_SWEEP_FLAG - SC_BUILD_FLAG, SC_RANGE_LIN_WORDS = SC_DEPTH_BAD - SC_RANGE, SC_DEPTH_WORDS = SC_STEPS_TOTAL - SC_DEPTH_BAD,
       SC_CIG_CHECK_WORDS = SC_JOIN_LENHIST - SC_CIG_BAD };

// T laid over the words from `first` up to (not including) `next`
#define IVX_SC_FITS(T, first, next) static_assert(sizeof(T) <= (size_t)((next) - (first)) * sizeof(u64), #T " must fit the scalar words named for it")

static_assert(SC_PAIRS == 0 && SC_FAULT == 1, "the probe kernels index the cursor pair themselves, and one clear / one copy covers both");
static_assert(SC_BUILD_INVERTED == SC_BUILD_FLAG + 1 && SC_BUILD_FLAG % 2 == 0, "the count build clears its two flags with one memset");
static_assert(SC_NEAR_HDR == SC_BUILD_FLAG + 2 && SC_SWEEP_FLAG == SC_BUILD_FLAG + 4, "the nearest build fetches flags and header as four words");
static_assert(SC_SWEEP_IRREGULAR == SC_SWEEP_FLAG + 1 && SC_SWEEP_FLAG % 2 == 0, "complement clears its two flags with one memset");
static_assert(SC_RANGE - SC_SORT_VAR == SC_SORT_FIELDS && SC_SORT_VAR % 2 == 0, "a word per sort field, cleared with one memset");
static_assert(SC_LIN == SC_RANGE + 6 && SC_DEPTH_BAD == SC_LIN + 2, "sort64 fetches the ranges and the two lin words as eight words");
static_assert(SC_DEPTH_SPARE == SC_DEPTH_BAD + 5 && SC_STEPS_TOTAL == SC_DEPTH_BAD + 6 && SC_DEPTH_BAD % 2 == 0, "depth()'s six words are cleared and fetched as one");
static_assert(SC_CIG_OFF0 == SC_CIG_BAD + 1 && SC_CIG_OFFN == SC_CIG_BAD + 2 && SC_CIG_BAD % 2 == 0, "the CIGAR check's three words are cleared and fetched as one");
static_assert(SC_LENHIST_N * sizeof(u32) <= (size_t)(SC_RANK_LONG - SC_JOIN_LENHIST) * sizeof(u64), "the length-class counters fit their words");
static_assert(HDR_WORDS * sizeof(u32) <= (size_t)(SC_HDR_MIRROR - SC_ROUTE_HDR) * sizeof(u64), "a routing view's header ends at or below the header mirror");
static_assert(SC_HDR_MIRROR * sizeof(u64) + HDR_WORDS * sizeof(u32) <= SC_HOST_WORDS * sizeof(u64), "the header mirror fits the host words");

// ---- ivx_ctx's accessors (declared in the struct)
template <typename T> inline ivx_status ivx_ctx::fetch_wait(int w, hipStream_t st, T *out)
{
    static_assert(sizeof(T) <= sizeof(u64), "one word");
    hipError_t e = fetch(w, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail_hip("scalar word fetch", e);
    *out = *hword<T>(w);
    return IVX_OK;
}
template <typename T> inline ivx_status ivx_ctx::fetch_wait(const T *src, hipStream_t st, T *out)
{
    IVX_SC_FITS(T, SC_LANDING, SC_LANDING + SC_LANDING_WORDS);
    hipError_t e = fetch(SC_LANDING, src, sizeof(T), st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail_hip("scalar fetch", e);
    *out = *hword<T>(SC_LANDING);
    return IVX_OK;
}
inline ivx_status ivx_ctx::check_flag(int w, hipStream_t st, const char *what)
{
    u32 bad;
    const ivx_status s = fetch_wait(w, st, &bad);
    return s != IVX_OK ? s : bad ? fail(IVX_ERR_INVALID, what) : IVX_OK;
}
