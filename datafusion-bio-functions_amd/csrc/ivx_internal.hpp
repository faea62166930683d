// ivx_internal.hpp -- shared host/device definitions of libivx_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <memory>
#include <string>
#include <vector>
#include "../../include/ivx.h"
#include "../../include/ivx_select.h"
#include "../../include/ivx_nearest.h"

typedef uint8_t u8;
typedef uint32_t u32;
typedef int32_t i32;
typedef uint64_t u64;
typedef int64_t i64;

#define IVX_WAVE 64

// ---------------------------------------------------------------- context
struct ivx_buf { void *p = nullptr; size_t cap = 0; };

enum { IVX_NSCRATCH = 56, IVX_NPIN = 4 };

// What a subtract sizing call leaves behind for the fill call that follows it: the sorted sides, the right
// side's running max / gap heads and the scanned per-row output counts all sit in scratch slots (`slots` =
// bit per slot); touching any of them drops the plan.
struct ivx_sub_plan {
    bool valid = false;
    u64 slots = 0;
    int mem = 0;
    const void *in[6] = {};             // the caller's six input columns
    u64 nl = 0, nr = 0, nh = 0, total = 0;
    u32 nkeys = 0;
    int strict = 0;
    int wf = 0;                         // the count pass took the two-search plan (every right row has start <= end)
    hipStream_t stream = nullptr;
    const u32 *lk, *lrow, *rk, *hk, *hj;
    const i64 *lsv, *lev, *rsv, *hrs, *hpm;
    const void *sm;
    const u64 *offs;
    const u32 *plan_hlo; const i64 *plan_tail;      // per left row: its first gap head, where its tail fragment starts
};

// Probe rows routed to the regions of an overlap index or routing view (ivx_regions_route.hip fills one in, the probes of
// ivx_regions_probe.hip and the routed operators of ivx_join.hip / ivx_ops32.hip read it).  It says where the rows are and in
// what form, not who routed them.
struct PageTab { u32 *ptab; u32 pstride, lgpg; };     // [region][page slot] -> pool page + 1 (0 = not there yet); a page holds 2^lgpg rows
// control block of the one-pass partition, one zero-initialised scratch buffer (the counters up to `rfirst` are cleared per call)
struct ivx_route_ctl {
    u32 rcur[1024];                     // rows routed to every region
    u32 pool_next, pad0[3];             // pages taken from the pool
    u32 rest_n[2];                      // the lean probes' rest lists: batches, rows
    u32 fill_done, pad1;                // workgroups of k_fill_rest that have left (the last one publishes the call's totals); zeroed with rest_n
    u32 rfirst[1032];                   // first routed row of every region (k_page_bounds / k_chunk_bounds)
    u32 cfirst[1032];                   // first 8192-row chunk of every region (k_chunk_bounds)
};
struct FpRest;                          // a batch the lean fill kernel leaves to the generic walk (ivx_regions.hpp)
enum {
    IVX_ROWS_FLAT = 0,                  // contiguous runs; rfirst = scanned [digit][nblk] histogram: region r starts at rfirst[r * nblk]
    IVX_ROWS_PAGED,                     // region pages behind a page table (one-pass partition); rfirst[r] = first routed row of region r
    IVX_ROWS_TABLE                      // contiguous regions, rfirst[r] a global table (two-level routing: more than IVX_MAXREG_WIDE regions)
};
struct ivx_routed {
    int form = IVX_ROWS_FLAT;
    const u64 *se = nullptr;            // the row words in routed order: (start,end), or the packed form; PAGED: the page pool
    const u32 *ids = nullptr;           // each row's id, at the row's position (null: packed rows carry their own) ...
    const unsigned short *cidx = nullptr;   // ... or its index inside its workgroup's chunk (per-row-value consumers: k_unpermute)
    const u32 *rfirst = nullptr;
    u32 nblk = 1, chunk = 0, ndig = 0;  // FLAT: workgroups of the partition, rows each took, digits of the histogram (256 / 1024)
    const u32 *unsorted = nullptr;      // FLAT / TABLE: *unsorted == 0: the rows came in region order, nothing was moved (read ds / de in place);
                                        // the context's word SC_UNSORTED (ivx_scalars.hpp), which is the routing pass's alone: a plan may hold this
    PageTab pt{nullptr, 0u, 0u};
    bool packed = false;                // 8-byte routed rows (start in region | length | row), else (start,end) + row id
    u32 rowbits = 32;                   // bits of a packed row's id (the rest of the word's upper half extends the length)
    bool tables_due = false;            // PAGED: rfirst and ctl->cfirst are NOT computed yet (ivx_paged_opts::defer_bounds): whoever reads them queues ivx_route_paged_bounds first
    bool all_routed = false;            // no occupancy bitmap in use: every row was routed (the fill's rows-per-lane rule is then known on the host)
    ivx_route_ctl *ctl = nullptr;
    FpRest *rest = nullptr; u64 *rest_rows = nullptr;   // the lean probes' rest lists (batches: fill only; single rows), or null
    const uint2 *vtab = nullptr;        // PAGED, per-row-value consumers: [tile][region] -> (virtual start, rows) of the tile's run
    const i32 *ds = nullptr, *de = nullptr;   // device start / end columns the rows were routed from (packed escapes and unmoved rows read them)
    u32 adj = 0;                        // 1: the UDTFs' strict mode, rows hold [start+1, end-1]
    u64 slots = 0;                      // scratch slots all of this sits in (bit per slot)
};

// What a region-partitioned overlap COUNT call leaves behind for the fill call that follows it: the routed probe
// rows and whose they are -- the fill call for the same index, columns and stream goes straight to its probe kernel.
// Touching any scratch slot of the rows drops the plan (ivx_ctx::get_scratch).
struct ivx_join_plan {
    bool valid = false;
    int mem = 0;
    const void *in[3] = {};
    u64 n = 0;
    u64 total = 0;                      // the pairs the count call found: the fill call's density hint, whatever its cap
    const void *ix = nullptr; u64 ix_serial = 0;
    hipStream_t stream = nullptr;
    ivx_routed rows;
};

struct ivx_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_ms = 0.0;
    std::string err;
    ivx_buf scratch[IVX_NSCRATCH];      // grow-only device scratch, one slot per use
    ivx_buf pinned[IVX_NPIN];           // grow-only pinned host staging
    // the scalar words: ivx_scalars.hpp names every one of them (SC_*) and says whose it is
    u64 *d_scalars = nullptr;           // SC_DEVICE_WORDS device words for flags / counters / totals
    u64 *h_scalars = nullptr;           // SC_HOST_WORDS words, the pinned mirror: mapped and coherent, so that a kernel can leave a few words in it itself
    u64 *hd_scalars = nullptr;          // ... its device pointer (SC_PAIRS / SC_FAULT: a lean fill's totals; SC_HDR_MIRROR: the header of the overlap
                                        // index built last)
    template <typename T = u64> T *dword(int w) const { return (T *)(d_scalars + w); }     // device word w, and its mirror word
    template <typename T = u64> T *hword(int w) const { return (T *)(h_scalars + w); }
    template <typename T = u64> T *hdword(int w) const { return (T *)(hd_scalars + w); }   // the mirror word, for a kernel
    // queue the copy of device words w .. w + words - 1 into their mirror words; of `bytes` device bytes at src into mirror word w
    hipError_t fetch(int w, hipStream_t st, int words = 1) { return hipMemcpyAsync(h_scalars + w, d_scalars + w, words * sizeof(u64), hipMemcpyDeviceToHost, st); }
    hipError_t fetch(int w, const void *src, size_t bytes, hipStream_t st) { return hipMemcpyAsync(h_scalars + w, src, bytes, hipMemcpyDeviceToHost, st); }
    // ... and wait for it: *out = device word w, as a T; = *src (device memory), landed in SC_LANDING
    template <typename T> ivx_status fetch_wait(int w, hipStream_t st, T *out);
    template <typename T> ivx_status fetch_wait(const T *src, hipStream_t st, T *out);
    ivx_status check_flag(int w, hipStream_t st, const char *what);    // fetch_wait of a u32 flag: IVX_ERR_INVALID with `what` if it is raised
    u64 hdr_mirror_serial = 0;          // the index whose header that is (its HDR_SLOW arrives with the build's tail: ivx_join_probe_regions)
    ivx_sub_plan sub_plan;
    ivx_join_plan join_plan;
    u64 join_fills_planned = 0, sub_fills_planned = 0;     // fill calls a plan served (test hook ivx_debug_ctx_state)
    u32 sweep_form[16] = {};            // IVX_SWEEP_* (below): what the last sweep's sort and packed sweep decided on the host (test hook)
    ivx_metrics metrics{};              // BuildProbeJoinMetrics, see ivx.h
    u64 mem_limit = 0;                  // device bytes of scratch + the index being built (0 = unlimited)
    u64 fill_hint = 0;                  // pairs a fill call should expect instead of its cap (a chunk of a host-resident batch writes into the whole batch's buffers)
    u64 scratch_bytes = 0, building_bytes = 0;
    // Build overlap (ivx_ctx_set_build_overlap): an overlap index build returns once the per-key tables and the region layout
    // are final -- all a probe's routing pass reads -- and leaves the rest (cell count, scan, scatter, region descriptors) running
    // on `aux`; `tail_ev` marks its end.  A probe's routing then runs beside it and only its probe kernel waits for the
    // index's `ready` event; anything else that could touch what the tail still uses waits first (get_scratch, join_tail).
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, tail_ev = nullptr;
    bool overlap = false, tail_pending = false;
    void join_tail();                   // order this context's stream behind a pending build tail
    // device bytes of the indexes this context built that are still alive (shared with those indexes: ivx_index_free
    // gives the bytes back whichever thread calls it, also after the context is gone)
    std::shared_ptr<std::atomic<u64>> live_index_bytes = std::make_shared<std::atomic<u64>>(0);
    u64 reserved() const { return scratch_bytes + building_bytes + live_index_bytes->load(std::memory_order_relaxed); }

    ivx_status fail(ivx_status st, const std::string &msg) { err = msg; return st; }
    ivx_status fail_hip(const char *what, hipError_t e)
    {
        err = std::string(what) + ": " + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? IVX_ERR_OOM : IVX_ERR_HIP;
    }
    // device scratch of at least `bytes` in slot `slot` (contents undefined)
    ivx_status get_scratch(int slot, size_t bytes, void **out);
    ivx_status get_pinned(int slot, size_t bytes, void **out);
};

#define IVX_HIP(ctx, call)                                              \
    do {                                                                \
        hipError_t e__ = (call);                                        \
        if (e__ != hipSuccess) return (ctx)->fail_hip(#call, e__);      \
    } while (0)

#define IVX_TRY(call)                                                   \
    do {                                                                \
        ivx_status s__ = (call);                                        \
        if (s__ != IVX_OK) return s__;                                  \
    } while (0)

// scratch slot ids (one per concurrent use inside a call)
enum {
    WS_IN_KEY = 0, WS_IN_START, WS_IN_END, WS_IN2_KEY, WS_IN2_START, WS_IN2_END,   // staged host inputs
    WS_OUT_A, WS_OUT_B, WS_OUT_C, WS_OUT_D, WS_OUT_E, WS_OUT_F, WS_OUT_G, WS_OUT_H,     // staged host outputs
    WS_SCAN0, WS_SCAN1, WS_SCAN2,                                                   // scan partials
    WS_GRID0, WS_GRID1, WS_GRID2,                                                   // key stats + cell cursors
    WS_SORTHIST,                                                                    // radix-sort histograms
    WS_SA0, WS_SA1, WS_SA2, WS_SB0, WS_SB1, WS_SB2,                                 // sort ping/pong records
    WS_RA0, WS_RA1, WS_RA2, WS_RB0, WS_RB1, WS_RB2,                                 // second record set (subtract's right side)
    WS_T0, WS_T1, WS_T2, WS_T3, WS_T4, WS_T5, WS_T6, WS_T7, WS_T8, WS_T9,           // per-op temporaries
    WS_IN3_KEY, WS_IN3_START, WS_IN3_END, WS_IN3_WEIGHT, WS_IN_KEYLEN,              // staged host inputs of depth(): the weighted segments, the key lengths
    WS_IN_TEXTOFF, WS_IN_TEXT                                                       // staged host inputs of the text-CIGAR calls: the Utf8 offsets and bytes
};
static_assert(WS_IN_TEXT < IVX_NSCRATCH, "scratch slot ids must fit the context's slot array");

// ---------------------------------------------------------------- indexes
#ifndef IVX_LSTEP
#define IVX_LSTEP 2       // bin width grows 4x per level: a level's cell is at most 4x wider than the rows it holds
#endif
#define IVX_MAXL (32 / IVX_LSTEP)   // length-class levels of the binned overlap index
#define IVX_SH_MIN 4

struct ivx_ent { i32 s, e; u32 row; };          // 12-byte AoS entry of the overlap index

// header words written by the layout kernel (device resident, read by probes)
enum { HDR_SH0 = 0, HDR_NLEV = 1, HDR_NBINS = 2, HDR_CS = 3 /* log2(cells per region) or ~0u */, HDR_NREG = 4,
       HDR_RCELLS = 5 /* cells per region */, HDR_RMUL_LO = 6, HDR_RMUL_HI = 7 /* ceil(2^40 / cells per region) */, HDR_LEVCNT = 8 /* .. +IVX_MAXL */,
       HDR_FG = 8 + IVX_MAXL /* log2(block width) of the occupancy bitmap, or ~0u: no bitmap */, HDR_FBITS = 9 + IVX_MAXL /* its size in bits */,
       HDR_PK24 = 10 + IVX_MAXL /* 1: a region spans at most 2^24 coordinates (routed rows pack into 8 bytes) */,
       HDR_SLOW = 11 + IVX_MAXL /* 0: every region is ONE LDS-resident level (all build rows in level 0, every slice fits): the lean fill probe applies */,
       HDR_LBUILD = 12 + IVX_MAXL /* 1: the build's tail sorts every region's rows in LDS (ivx_join.hip: k_lbuild_*); 0: the global counting sort */,
       HDR_BADKEY = 13 + IVX_MAXL /* != 0: a build row's key id is >= n_keys (the key statistics' flag: one copy brings it to the host with the layout) */,
       HDR_WORDS = 14 + IVX_MAXL };
#include "ivx_scalars.hpp"
// Occupancy bitmap of the build side ("can a probe row match anything at all"): per key one bit per 2^g-wide block of
// [origin, origin + span] plus one overflow block behind it; a bit is set when some build row touches the block.  Sized to
// stay resident in an XCD's 4 MiB L2 next to the streamed probe rows.
#define IVX_FBITS_MAX (1u << 24)    // 2 MiB
#define IVX_MAXREG 255   // probe regions routed with ONE partition pass (one radix digit; 255 = rows that cannot match)
#define IVX_MAXREG_WIDE 1023   // ... still one pass, with 1024 digits (overlap join count / fill only)
#define IVX_MAXREG2 65025u   // most regions at all: beyond 255 the probe rows are routed by a two-digit stable sort
#define IVX_REG_CS_MAX 13   // a region spans at most 2^13 level-0 cells, what a workgroup can stage in LDS

// what a probe workgroup needs to stage one region's slice of level 0 (ivx_regions_probe.hip), precomputed at
// build time so that staging starts with ONE load instead of a chain of four dependent ones
#ifndef IVX_RP_ECAP
#define IVX_RP_ECAP 6144          // level-0 entries a region's LDS slice holds (ivx_regions_probe.hip)
#endif
#define IVX_RP_HALO 8u      // slice cells past the region's last cell
struct ivx_regdesc { u32 k; i32 origin; u32 span, lb, slo, shi, e0, ne; i32 rbase; /* coordinate of the region's first cell */ };

struct JoinIndexView {
    const i32 *origin;      // [nkeys] smallest start of the key
    const u32 *span;        // [nkeys] largest start - smallest start
    const u32 *kcnt;        // [nkeys] build rows of the key
    const u32 *lbase;       // [IVX_MAXL*nkeys] first bin of (level,key)
    const u32 *binstart;    // [nbins+1] CSR offsets into ent
    const ivx_ent *ent;     // [n] entries grouped by bin
    const u32 *hdr;         // [HDR_WORDS]
    const u32 *kreg;        // [nkeys+1] first probe region of the key (regions never straddle keys)
    const u32 *rkey;        // [IVX_MAXREG2+1] key of a region
    const ivx_regdesc *rdesc;   // [IVX_MAXREG2+1] slice window of a region
    const u32 *fbits;       // occupancy bitmap words (+2 words of padding), valid when hdr[HDR_FG] != ~0u
    const u32 *fbase;       // [nkeys] first bit of the key (a multiple of 32)
    u32 nkeys;
};

// sorted-rank grid over one int32 column grouped by key (count_overlaps,
// coverage, nearest): rank(x) = cum[bin(x)] + #{v in bin : v <= x}
struct RankGridView {
    const i32 *origin;      // [nkeys] smallest value of the key
    const u32 *span;        // [nkeys]
    const u32 *kcnt;        // [nkeys]
    const u32 *koff;        // [nkeys+1] rows before the key
    const u32 *kbase;       // [nkeys] first bin of the key
    const u32 *binstart;    // [nbins+1]
    const i32 *val;         // [n] values grouped by (key,bin); sorted if `sorted`
    const u32 *hdr;         // [0] = shift
    u32 nkeys;
};

struct CoverageView {
    RankGridView first, last;   // over merged nodes' first / last (both ascending per key)
    const i64 *pw;              // [m+1] prefix sums of max(1, last-first)
    const i32 *nfirst, *nlast;  // [m] merged nodes in order
};

// one build row of the nearest index, 16 bytes so that a candidate is ONE load: in by_start order
// a = start, b = end, pmax = running max of end within the key; in by_end order a = end, b = start
struct ivx_nrec { i32 a, b; u32 row; i32 pmax; };

struct NearestView {
    RankGridView by_start, by_end, pmax;   // rank grids over rs[].a / re[].a / rs[].pmax (value stride 4 words)
    const ivx_nrec *rs;                    // by_start order (start,end,row)
    const ivx_nrec *re;                    // by_end order (end,start,row)
    JoinIndexView ov;                               // overlap index for k>1 include_overlaps
};

// a depth profile (ivx_depth_expand.hip): the step function of depth() -- per key ascending, every position where the
// coverage changes and the coverage from there on
struct DepthProfileView {
    const u32 *key, *pos;   // [steps] ordered by (key, position)
    const i32 *cov;         // [steps] coverage from pos on
    const u32 *koff;        // [nkeys+1] first step of the key
    const u8 *seen;         // [nkeys] 1: the key kept an event after the filter and the clipping
    u64 steps;
};

struct ivx_index {
    u64 serial = 0;             // unique per built index (a freed index's address may come back)
    int kind = 0;
    int device = 0;
    u64 n = 0;
    u32 nkeys = 0;
    size_t bytes = 0;
    std::shared_ptr<std::atomic<u64>> owner_bytes;   // the building context's live_index_bytes (null until the build succeeded)
    std::vector<void *> allocs;
    std::vector<size_t> alloc_caps;
    JoinIndexView jv{};
    u32 jv_nreg = 0;            // >0: the region-partitioned probe is available
    bool jv_filter = false;     // jv carries an occupancy bitmap (hdr[HDR_FG] != ~0u)
    bool jv_pk24 = false;       // hdr[HDR_PK24]
    // May the lean probes run on this index: 0 no (hdr[HDR_SLOW] is set or there are no regions), 1 yes, 2 not known on the
    // host yet -- built with the tail overlapped, hdr[HDR_SLOW] is final only behind `ready` (kernels test it themselves).
    // The one field a probe call writes: the first region fill or count that waits for the tail settles 2 to 0 or 1.  Other
    // contexts and threads may probe the index meanwhile, hence an atomic (relaxed: either value they read is right).
    mutable std::atomic<int> jv_lean{0};
    hipEvent_t ready = nullptr; // set when the build's tail ran on the aux stream: everything but the routing tables is valid behind it
    RankGridView gs{}, ge{};
    CoverageView cv{};
    NearestView nv{};
    JoinIndexView nroute{};     // nearest index: regions that only ROUTE big probe batches (origin/span/kcnt/kreg/rkey/hdr; no cells)
    u32 nroute_nreg = 0;
    // nearest index: the form its build's sorts took (ivx_ops32.hip: nearest_sorted_records; read by ivx_debug_index_forms)
    u32 near_words = 0;         // sort words per row: 0 no rows, 1 linearised (key, coordinate) ‖ row, 2 (start, end) + (key, row)
    u32 near_order = 0;         // IVX_NEAR_ORDER_*: how the (key, start, end) order was reached
    u32 near_fallback = 0;      // IVX_NEAR_FB_* bits: forms the build tried and left
    DepthProfileView dp{};      // IVX_KIND_DEPTH_PROFILE
    int flags = 0;              // IVX_IXF_*
};
enum { IVX_IXF_REGION_ROWVAL = 1 };   // count/coverage index: jv is usable for the region-partitioned per-row probe
enum { IVX_NEAR_ORDER_PRESORTED = 0 /* no sort: the rows came in order */, IVX_NEAR_ORDER_REPAIR = 1 /* sort on the leading fields, runs of equal (key, start) put in end order afterwards */,
       IVX_NEAR_ORDER_FULL = 2 /* one sort on all three fields */ };
enum { IVX_NEAR_FB_NOFIT = 1 /* the one-word form did not fit 64 bits */, IVX_NEAR_FB_LIN_RUN = 2 /* the one-word unpack met a run above NLIN_MAXRUN */,
       IVX_NEAR_FB_SE_RUN = 4 /* the two-word run repair met a run above NFIX_MAXRUN */ };
// words of ivx_debug_index_forms (ivx_capi.hip; tests only, not in include/ivx.h): kind, routing regions, the three near_* fields,
// then (shift, cells) of up to three rank grids -- count: starts, ends; coverage: first, last; nearest: by_start, by_end, pmax
enum { IVX_FORMS_KIND = 0, IVX_FORMS_NROUTE_NREG = 1, IVX_FORMS_NEAR_WORDS = 2, IVX_FORMS_NEAR_ORDER = 3, IVX_FORMS_NEAR_FALLBACK = 4,
       IVX_FORMS_GRID0 = 5, IVX_FORMS_WORDS = 11 };
// words of ivx_debug_sweep_form (ivx_sweep.hip; tests only, not in include/ivx.h): the decisions the last sort64 of a sweep's
// input rows (ivx_sweep.hip) and the packed sweep behind it (ivx_runs.hip runs_packed) took ON THE HOST -- nothing is written by
// a kernel.  merge / cluster / complement / intersect clear them at entry (intersect: they describe its right side's sort and
// sweep); after a subtract they describe its last sort64 call.
enum { IVX_SWEEP_SORT_WORDS = 0 /* words of the radix sort that ran: 0 none, 1, 3 */, IVX_SWEEP_NW = 1 /* words the sort key takes: 1 or 3 */,
       IVX_SWEEP_LIN = 2, IVX_SWEEP_BITS_S = 3, IVX_SWEEP_BITS_E = 4, IVX_SWEEP_BITS_K = 5,
       IVX_SWEEP_SORTED_IN = 6 /* the rows were taken as already in order */, IVX_SWEEP_TWO_STEP = 7 /* sort on (key, start), equal starts repaired: tried */,
       IVX_SWEEP_TOOLONG = 8 /* ... and left for the full sort after a run above FIX_MAXRUN */,
       IVX_SWEEP_NARROW_ROWS = 9 /* the sweep's rows are 32-bit offsets */, IVX_SWEEP_K8 = 10 /* ... with one-byte keys */,
       IVX_SWEEP_PACKED = 11 /* 0 the sweep reads rows, 1 packed words instead of rows, 2 packed words beside rows (cluster) */,
       IVX_SWEEP_NARROW_RUNS = 12 /* k_pk_runs<..., NARROW = true> */, IVX_SWEEP_NTILE = 13 /* tiles of the packed sweep */,
       IVX_SWEEP_LEFT_NW = 14, IVX_SWEEP_LEFT_SORT_WORDS = 15 /* intersect only: NW and SORT_WORDS of its LEFT side's sort */,
       IVX_SWEEP_WORDS = 16 };
static_assert(IVX_SWEEP_WORDS <= sizeof(ivx_ctx::sweep_form) / sizeof(u32), "ivx_ctx::sweep_form holds the IVX_SWEEP_* words");
// words of ivx_debug_ctx_state (ivx_capi.hip; tests only, not in include/ivx.h), u64 each: what a context carries from one call
// to the next.  The slot masks have a bit per scratch slot (WS_*) and are meaningful while their plan is valid.
enum { IVX_STATE_JOIN_VALID = 0, IVX_STATE_JOIN_SLOTS = 1 /* ivx_join_plan::rows.slots */, IVX_STATE_SUB_VALID = 2, IVX_STATE_SUB_SLOTS = 3,
       IVX_STATE_TAIL_PENDING = 4, IVX_STATE_SCRATCH_HELD = 5 /* scratch slots that hold memory */,
       IVX_STATE_POOL_FREE = 6 /* free buffers of the index pool on the context's device */,
       IVX_STATE_JOIN_FILLS_PLANNED = 7, IVX_STATE_SUB_FILLS_PLANNED = 8 /* fill calls so far that a plan served */, IVX_STATE_WORDS = 9 };
// bits of ivx_debug_poison's `what` (ivx_capi.hip; tests only, not in include/ivx.h)
enum { IVX_POISON_SCRATCH = 1 /* every scratch slot that holds memory and that no valid plan names, over its full capacity */,
       IVX_POISON_DROP_PLANS = 2 /* both plans dropped first: IVX_POISON_SCRATCH then covers every slot */,
       IVX_POISON_SCALARS = 4 /* the call-local scalar words, device and mirror: all but SC_OUTLIVES (ivx_scalars.hpp) */,
       IVX_POISON_PINNED = 8 /* the pinned staging buffers */, IVX_POISON_POOL = 16 /* this device's free buffers of the index pool */ };

// ---------------------------------------------------------------- internal API
// scan.hip
ivx_status ivx_scan_exclusive_u32(ivx_ctx *ctx, u32 *data, u64 n, const u32 *skip = nullptr);      // in place, uses WS_SCAN*; skip (nullable): the kernels leave at once when *skip != 0
ivx_status ivx_scan_exclusive_u64(ivx_ctx *ctx, u64 *data, u64 n);

// join.hip
ivx_status ivx_join_build(ivx_ctx *ctx, ivx_index *ix, const u32 *key, const i32 *s, const i32 *e, u64 n, bool overlap = false);
ivx_status ivx_join_probe(ivx_ctx *ctx, const JoinIndexView &jv, int mode,
                          const u32 *key, const i32 *s, const i32 *e, u64 n,
                          u32 *per_row, u8 *exists, u32 *ob, u32 *op, u64 cap, u64 *d_cursor);
enum { JP_COUNT = 0, JP_PER_ROW = 1, JP_EXISTS = 2, JP_FILL = 3 };
// ivx_regions_probe.hip: partition the probe rows by index region (ivx_regions_route.hip), probe each region from LDS
// what a call tells its caller besides its status
struct ivx_probe_note {
    u64 ix_serial = 0;          // in: the index probed (fast == 2: is the context's header mirror this index's?)
    int fast = -1;              // out: 0 / 1 when the call came in with fast == 2 and learnt hdr[HDR_SLOW] on the host, else -1
    bool totals_on_host = false;    // out: the call's last kernel leaves d_cursor[0..1] in the mirror words SC_PAIRS / SC_FAULT itself (no copy needed, only the synchronisation)
};
ivx_status ivx_join_probe_regions(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, int mode,
                                  const u32 *key, const i32 *s, const i32 *e, u64 n,
                                  u32 *ob, u32 *op, u64 cap, u64 *d_cursor, bool planned = false, bool has_filter = false, bool pk24 = false,
                                  int fast = 0 /* 0 no, 1 yes, 2 the kernels test hdr[HDR_SLOW] themselves */, hipEvent_t ready = nullptr,
                                  bool clear_cursor = false /* d_cursor[0..1] are still to be zeroed (with the routing pass's own clears) */,
                                  ivx_probe_note *note = nullptr);

// per-row-output operators through the same partition (count_overlaps: jv over the build rows, no row with
// end < start; coverage: jv over the merged nodes)
enum { IVX_RV_COUNT = 0, IVX_RV_COVERAGE = 1, IVX_RV_PER_ROW = 2, IVX_RV_EXISTS = 3 };
ivx_status ivx_route_view_build(ivx_ctx *ctx, ivx_index *ix, const i32 *origin, const u32 *span, const u32 *kcnt);
void ivx_route_view_ready(ivx_ctx *ctx, ivx_index *ix);
ivx_status ivx_join_rowval_routed(ivx_ctx *ctx, const ivx_index *ix, int mode, const u32 *key, const i32 *s, const i32 *e, u64 n,
                                  u32 *per_row, u8 *exists, u64 *d_total);
ivx_status ivx_unroute_u32(ivx_ctx *ctx, const ivx_routed &r, u64 n, const u32 *vb, u32 *out32, u8 *out8);
ivx_status ivx_route_rows(ivx_ctx *ctx, const JoinIndexView &rv, const u32 *key, const i32 *s, const i32 *e, u64 n, u32 adj, ivx_routed *out);
ivx_status ivx_unroute_pair(ivx_ctx *ctx, const ivx_routed &r, u64 n, const u32 *vb, const i64 *vd, u32 *ob, u32 *op, i64 *od, i64 dflt);
ivx_status ivx_rowval_probe_regions(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, int kind,
                                    const u32 *key, const i32 *s, const i32 *e, u64 n, int strict, void *out, u64 *d_total,
                                    bool has_filter = false, bool pk24 = false, bool fast = false);

// An overlap threshold as the kernels carry it (ivx_where.hpp).  The per-row probes below take one as `w`: null is the plain
// call; else only the pairs that pass reach the operator (WhereOp), on the same launchers and un-permute passes.
struct WherePred;
// build-side match marks (ivx_marks.hip; the lean region form in ivx_regions_probe.hip): one bit per build row, ORed
ivx_status ivx_mark_probe(ivx_ctx *ctx, const JoinIndexView &jv, const u32 *key, const i32 *s, const i32 *e, u64 n, u32 *marks,
                          const WherePred *w = nullptr);
ivx_status ivx_mark_probe_regions(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, const u32 *key, const i32 *s, const i32 *e, u64 n,
                                  u32 *marks, bool has_filter, bool pk24, bool fast, bool *took, const WherePred *w = nullptr);
// overlap aggregates (ivx_agg.hip; the lean region form in ivx_regions_probe.hip): per probe row, over the build rows the
// join pairs it with, aggregates of a build-side value column (val_bytes: 4 or 8, signed).  The call's output columns, one
// element per probe row in input order; null: not wanted, neither computed nor stored
struct AggOut { u32 *count; i64 *sum, *vmin, *vmax, *bases, *wsum; };
ivx_status ivx_agg_probe(ivx_ctx *ctx, const JoinIndexView &jv, const u32 *key, const i32 *s, const i32 *e, u64 n,
                         const void *val, u32 val_bytes, const AggOut &out, const WherePred *w = nullptr);
ivx_status ivx_agg_probe_regions(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, const u32 *key, const i32 *s, const i32 *e, u64 n,
                                 const void *val, u32 val_bytes, const AggOut &out, bool has_filter, bool pk24, bool fast, bool *took,
                                 const WherePred *w = nullptr);
// overlap select (ivx_select.hip; the lean region form in ivx_regions_probe.hip): per probe row the one build row of those the
// join pairs it with that is best by `by` (an IVX_SEL_* criterion; val / val_bytes are read by the *_VAL ones only).  idx is
// always wanted; score may be null: neither computed nor stored
struct SelOut { u32 *idx; i64 *score; };
ivx_status ivx_sel_probe(ivx_ctx *ctx, const JoinIndexView &jv, const u32 *key, const i32 *s, const i32 *e, u64 n,
                         const void *val, u32 val_bytes, int by, const SelOut &out, const WherePred *w = nullptr);
ivx_status ivx_sel_probe_regions(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, const u32 *key, const i32 *s, const i32 *e, u64 n,
                                 const void *val, u32 val_bytes, int by, const SelOut &out, bool has_filter, bool pk24, bool fast, bool *took,
                                 const WherePred *w = nullptr);
// overlap thresholds (ivx_where.hip; the lean region form in ivx_regions_probe.hip).  The match count per probe row under a
// threshold: per_row / exists (either may be null), one element per probe row in input order.  The region form has the
// marks' eligibility and *took, writes ONE of the two columns (per_row if given) and, with per_row, adds the counts to *d_total
// (nullable) in its un-permute.
ivx_status ivx_match_probe_where(ivx_ctx *ctx, const JoinIndexView &jv, const u32 *key, const i32 *s, const i32 *e, u64 n,
                                 u32 *per_row, u8 *exists, const WherePred &w);
ivx_status ivx_match_probe_regions_where(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, const u32 *key, const i32 *s, const i32 *e, u64 n,
                                         u32 *per_row, u8 *exists, u64 *d_total, bool has_filter, bool pk24, bool fast, bool *took, const WherePred &w);
// *d_total += the sum of per_row[0 .. n) (null: not wanted), and exists[i] = per_row[i] != 0 when exists is given
ivx_status ivx_match_totals(ivx_ctx *ctx, const u32 *per_row, u64 n, u8 *exists, u64 *d_total);
// the stable pair filter (ivx_pairs_where of include/ivx_where.h, device pointers); scratch: WS_T5, WS_T6 and the scan's
ivx_status ivx_pairs_where_device(ivx_ctx *ctx, const u32 *bidx, const u32 *pidx, u64 n_pairs, const i32 *bs, const i32 *be, u64 nb,
                                  const i32 *ps, const i32 *pe, u64 np, const WherePred &w, u32 *ob, u32 *op, u64 cap, u64 *n_out);
ivx_status ivx_bits_mark_device(ivx_ctx *ctx, const u32 *idx, u64 n, u32 *bits, u64 n_bits);
ivx_status ivx_bits_select_device(ivx_ctx *ctx, const u32 *bits, u64 n_bits, int want_set, u32 *out, u64 cap, u64 *n_out);

// ivx_depth.hip: coverage blocks from reads with binary CIGARs and from weighted segments (device pointers)
ivx_status ivx_depth_device(ivx_ctx *ctx, const u32 *rkey, const u32 *rpos, const u32 *rflags, const u32 *rmapq,
                            const i32 *cigar_offsets, const u32 *cigar_ops, u64 n_reads,
                            const u32 *skey, const u32 *sstart, const u32 *send, const i32 *sweight, u64 n_seg,
                            u32 nkeys, const u32 *key_len, u32 filter_flag, u32 min_mapq,
                            u32 *ok, u32 *os, u32 *oe, i32 *oc, u64 cap, u64 *n_out);

// its front half: the events sorted by (key, position), and (c, g) = (the key's running sum, the group's sum) at the last
// event of every (key, position) group; all of it in scratch
struct ivx_depth_evs { u64 n; const u64 *ev; const uint2 *cg; };
ivx_status ivx_depth_events(ivx_ctx *ctx, const u32 *rkey, const u32 *rpos, const u32 *rflags, const u32 *rmapq,
                            const i32 *cigar_offsets, const u32 *cigar_ops, u64 n_reads,
                            const u32 *skey, const u32 *sstart, const u32 *send, const i32 *sweight, u64 n_seg,
                            u32 nkeys, const u32 *key_len, u32 filter_flag, u32 min_mapq, u8 *seen, ivx_depth_evs *out);
// ivx_cigar.hip: text CIGARs (an Arrow Utf8 / LargeUtf8 column on the device) to packed ops.  count: the checks and the op
// count (synchronises); write: out_off [n_reads + 1] and out_ops [n_ops], either nullable (synchronises: an op length that
// cannot be packed is an error).  Scratch: WS_SCAN0 / WS_SCAN1, which must stay untouched between the two.
struct ivx_cigar_plan {
    int large; const void *off; const u8 *txt; u64 n_reads, n_bytes, n_ops, nblk; i64 off0; u32 mis; void *tsum;
};
ivx_status ivx_cigar_count(ivx_ctx *ctx, int large, const void *text_offsets, const u8 *text, bool text_at_off0, u64 n_reads,
                           ivx_cigar_plan *plan);
ivx_status ivx_cigar_write(ivx_ctx *ctx, const ivx_cigar_plan &plan, i32 *out_off, u32 *out_ops);
// ivx_depth_expand.hip: the steps of those events as a profile (ix->dp), and windows of a profile expanded to positions
ivx_status ivx_depth_profile_begin(ivx_ctx *ctx, ivx_index *ix, u8 **seen);     // before the front half: key_seen and the per-key table, zeroed
ivx_status ivx_depth_profile_finish(ivx_ctx *ctx, ivx_index *ix, const ivx_depth_evs &evs);
ivx_status ivx_depth_profile_koff(ivx_ctx *ctx, const u32 *skey, u32 steps, u32 nkeys, u32 *koff);    // koff[k] = the first step with key >= k
ivx_status ivx_depth_expand_device(ivx_ctx *ctx, const DepthProfileView &dp, u32 key, u32 first_pos, u64 n, int skip_pos0,
                                   i32 *out_pos, int16_t *out_cov);
// ivx_depth_merge.hip: ix (from ivx_depth_profile_begin, nkeys = the larger of the two) = a + b; the coverage blocks of a profile
ivx_status ivx_depth_profile_merge_device(ivx_ctx *ctx, const DepthProfileView &a, u32 nka, const DepthProfileView &b, u32 nkb, ivx_index *ix);
ivx_status ivx_depth_profile_blocks_device(ivx_ctx *ctx, const DepthProfileView &dp, u32 *ok, u32 *os, u32 *oe, i32 *oc, u64 cap, u64 *n_out);
// The n regions of a region statistic: rows (key, start, end) of a table (device columns; qkey null: key 0; IVX_NULL_IDX: the skip
// mark), clipped to [pos_lo, key_hi[key]] (key_hi nullable), or windows of `width` positions of one key from first_pos on, cut
// at last_pos (key < nkeys, first_pos + (n - 1) * width < 2^32: the caller's checks).  with_region_in makes the kernel's form of it.
struct DepthRegionSrc {
    bool windows; const u32 *qkey, *qstart, *qend; u32 pos_lo; const u32 *key_hi;       // the table
    u32 key, first_pos, last_pos, width; u64 n; int skip_pos0;                          // the windows; both
};
// ivx_depth_regions.hip: bases, coverage sum and bases >= each threshold per region (thresholds: host memory; out_ge threshold-
// major [n_thr * n]; any output may be null).  A table's key id >= nkeys other than the skip mark: IVX_ERR_INVALID (one word
// read back), before anything is indexed with it and even when no output is wanted; nothing is written then.
ivx_status ivx_depth_region_sums_device(ivx_ctx *ctx, const DepthProfileView &dp, u32 nkeys, const DepthRegionSrc &src,
                                        const i32 *thresholds, u32 n_thr, i64 *out_len, i64 *out_sum, i64 *out_ge);
// ivx_depth_rank.hip: bases, min, max and up to 8 lower quantiles of the per-base coverage per region (q_num: host memory,
// rank = floor((bases - 1) * q_num / q_den); out_q quantile-major [n_q * n]; any output may be null).  The key check of the sums.
ivx_status ivx_depth_region_ranks_device(ivx_ctx *ctx, const DepthProfileView &dp, u32 nkeys, const DepthRegionSrc &src,
                                         const u32 *q_num, u32 n_q, u32 q_den, i64 *out_len, i32 *out_min, i32 *out_max, i32 *out_q);
// ivx_depth_classes.hip: the maximal runs of one coverage class per key (cuts: host memory, checked by the caller; any output
// may be null; synchronises for the count), and the per-key histogram of the per-base coverage (out: [nkeys * n_bins])
ivx_status ivx_depth_quantize_device(ivx_ctx *ctx, const DepthProfileView &dp, u32 nkeys, u32 pos_lo, const u32 *key_hi, int skip_pos0, int seen_only,
                                     const i32 *cuts, u32 n_cuts, u32 emit_mask, u32 *ok, u32 *os, u32 *oe, u32 *oc, u64 cap, u64 *n_out);
ivx_status ivx_depth_hist_device(ivx_ctx *ctx, const DepthProfileView &dp, u32 nkeys, u32 pos_lo, const u32 *key_hi, int skip_pos0, int seen_only,
                                 i32 v_lo, u32 n_bins, i64 *out);

// ivx_ops32.hip: the count_overlaps / coverage / nearest indexes and their probes (device pointers)
ivx_status ivx_count_build(ivx_ctx *ctx, ivx_index *ix, const u32 *key, const i32 *s, const i32 *e, u64 n);
ivx_status ivx_coverage_build(ivx_ctx *ctx, ivx_index *ix, const u32 *key, const i32 *s, const i32 *e, u64 n);
ivx_status ivx_nearest_build(ivx_ctx *ctx, ivx_index *ix, const u32 *key, const i32 *s, const i32 *e, u64 n);
ivx_status ivx_count_probe(ivx_ctx *ctx, const ivx_index *ix, const u32 *key, const i32 *s, const i32 *e, u64 n, int strict, i64 *out);
ivx_status ivx_coverage_probe(ivx_ctx *ctx, const ivx_index *ix, const u32 *key, const i32 *s, const i32 *e, u64 n, int strict, i64 *out);
ivx_status ivx_nearest_probe(ivx_ctx *ctx, const ivx_index *ix, const u32 *key, const i32 *s, const i32 *e, u64 n,
                             int strict, u32 k, int include_overlaps, u32 *ob, u32 *op, i64 *od, u64 cap, u64 *rows);
// the same on one side only and / or within a distance cap (include/ivx_nearest.h): direction = IVX_NEAR_*, max_distance < 0 = no
// cap; IVX_NEAR_ANY without a cap IS ivx_nearest_probe.  Scratch as ivx_nearest_probe
ivx_status ivx_nearest_probe_dir(ivx_ctx *ctx, const ivx_index *ix, const u32 *key, const i32 *s, const i32 *e, u64 n,
                                 int strict, u32 k, int include_overlaps, int direction, i64 max_distance,
                                 u32 *ob, u32 *op, i64 *od, u64 cap, u64 *rows);

// ivx_sweep.hip: merge / subtract / cluster / complement over int64 coordinates (device pointers); the fill half of a
// subtract whose sizing call left its plan in the context
ivx_status ivx_merge_device(ivx_ctx *ctx, const u32 *key, const i64 *s, const i64 *e, u64 n, u32 nkeys,
                            i64 min_dist, int strict, u32 *ok, i64 *os, i64 *oe, i64 *on, u64 *m);
ivx_status ivx_subtract_device(ivx_ctx *ctx, const u32 *lkey, const i64 *ls, const i64 *le, u64 nl,
                               const u32 *rkey, const i64 *rs, const i64 *re, u64 nr, u32 nkeys, int strict,
                               u32 *ok, i64 *os, i64 *oe, u32 *orow, u64 cap, u64 *n_out);
ivx_status ivx_subtract_fill_planned(ivx_ctx *ctx, u32 *ok, i64 *os, i64 *oe, u32 *orow, u64 cap, u64 *n_out);
// intersect; dbg (nullable; the test hook ivx_debug_intersect_paths): HOST buffers for what the count pass did -- `wg`: words
// per workgroup (k_frag_count), `row_esc`: one byte per left row at its original index -- capacities in workgroups / rows,
// and where the numbers of both go
struct ivx_isect_debug { u32 *wg; u64 wg_cap; u8 *row_esc; u64 row_cap; u64 *n_wg, *n_rows; };
ivx_status ivx_intersect_device(ivx_ctx *ctx, const u32 *lkey, const i64 *ls, const i64 *le, u64 nl,
                                const u32 *rkey, const i64 *rs, const i64 *re, u64 nr, u32 nkeys, int strict,
                                u32 *ok, i64 *os, i64 *oe, u32 *orow, u64 cap, u64 *n_out, const ivx_isect_debug *dbg = nullptr);
ivx_status ivx_cluster_device(ivx_ctx *ctx, const u32 *key, const i64 *s, const i64 *e, u64 n, u32 nkeys,
                              i64 min_dist, int strict, const i64 *key_base,
                              u32 *ok, i64 *os, i64 *oe, u32 *orow, i64 *oc, i64 *ocs, i64 *oce, u64 *key_clusters, u64 *m);
ivx_status ivx_complement_device(ivx_ctx *ctx, const u32 *key, const i64 *s, const i64 *e, u64 n,
                                 const u32 *vkey, const i64 *vs, const i64 *ve, u64 nv, u32 nkeys, int strict,
                                 u32 *ok, i64 *os, i64 *oe, u64 cap, u64 *n_out);

// ivx_take.hip: compute::take of payload columns by uint32 row, and its inverse (device pointers)
ivx_status ivx_take_fixed_device(ivx_ctx *ctx, const void *src, u32 width, u64 n_src, const u8 *src_valid,
                                 const u32 *idx, u64 n, void *out, u8 *out_valid);
ivx_status ivx_scatter_fixed_device(ivx_ctx *ctx, const void *src, u32 width, const u32 *idx, u64 n, void *out, u64 n_out);
ivx_status ivx_take_bits_device(ivx_ctx *ctx, const u8 *src_bits, u64 n_src, const u8 *src_valid, const u32 *idx, u64 n, u8 *out_bits, u8 *out_valid);
ivx_status ivx_take_utf8_device(ivx_ctx *ctx, int large, const void *offsets, const u8 *data, u64 n_src, const u8 *src_valid,
                                const u32 *idx, u64 n, void *out_offsets, u8 *out_data, u64 data_cap, u64 *data_bytes, u8 *out_valid);
ivx_status ivx_take_view_device(ivx_ctx *ctx, const void *views, const u8 *const *bufs, u64 n_src, const u8 *src_valid,
                                const u32 *idx, u64 n, void *out_views, u8 *out_data, u64 data_cap, u64 *data_bytes, u8 *out_valid);

ivx_status ivx_index_alloc(ivx_ctx *ctx, ivx_index *ix, size_t bytes, void **out);
