// ivx_regions_route.hip -- routing: probe rows grouped by index REGION, so that the probe never gathers from HBM.
//
// Unsorted probe rows gathered straight from the index cost ~1.6 fabric reads of
// 64 B per row (profiles/r1_a_probe_count_v1_pmc.txt): the index (tens of MB) does
// not fit a 4 MB XCD L2.  So the probe side is first radix-partitioned by index
// REGION (a run of 2^cs level-0 cells of one key), and every region is then probed by
// workgroups that stage its slice of the index in LDS (ivx_regions_probe.hip).  Three
// ways to route, each one host function that fills in an ivx_routed (ivx_internal.hpp):
//
//   ivx_route_flat       k_part_hist      region histogram per workgroup (LDS counters, 16-byte row loads)
//                        scan             exclusive prefix over [region][workgroup]
//                        k_part_scatter   (qs,qe,row) records re-ordered through LDS, contiguous runs out
//                        (input already in region order: nothing is moved, the consumers read it in place)
//   ivx_route_paged      k_part_onepass   one read of the rows; a region's rows go to pages taken from a pool on
//                                         demand, optionally as packed 8-byte words and filtered by the build side's
//                                         occupancy bitmap
//                        k_page_bounds / k_chunk_bounds   the regions' first rows (and first 8192-row chunks)
//   ivx_route_two_level  k_part_*<SPLIT> + k_p2_* + k_sorted_bounds   more regions than one digit holds
//
// and the way back for consumers that answer per row: k_unpermute / k_unpermute_paged / k_unpermute_pair /
// k_unpermute_records (ivx_unroute_*).  ivx_route_rows is the flat form for operators with a probe kernel of their own (nearest, the
// rank-grid operators, the join's per-row counts over many regions).
//
// HBM traffic per probe row of the flat form: 8 B (hist) + 12 B + 12 B (scatter), all streaming (measured:
// profiles/r1_d_regions_pipeline_pmc.txt); the paged form reads 12 B and writes 8 B or 12 B.
#include "ivx_regions.hpp"

namespace {

// ------------------------------------------------------------------ partition pass

constexpr int PA_T = 1024;
#ifndef IVX_PA_I
#define IVX_PA_I 12
#endif
constexpr int PA_I = IVX_PA_I;                    // rows per thread and tile (multiple of 4)
constexpr int PA_TILE = PA_T * PA_I;              // 12288 rows: ~63 rows per region and tile = the length of the runs written to HBM
constexpr u32 NO_REGION = 0xFFFFFFFFu;
constexpr u32 KT_MAX = 256;                       // per-key tables cached in LDS up to this many keys

// per-key lookup for "which region does a probe row start in", cached in LDS (up to KT_MAX keys; lastcell = 0xFFFFFFFF: key
// has no build rows).  The LDS tables are passed to region_of as the kernel's own arrays, never through a pointer that may
// also be null / global: such a pointer makes every lookup a flat load with full waits.
struct KeyTab {
    bool lds;
    u32 nkeys, sh0, cs;          // cs = log2(cells per region), or ~0u: divide by multiplying with rmul
    u64 rmul;
};

__device__ __forceinline__ void keytab_load(const JoinIndexView &ix, i32 *s_origin, u32 *s_last, u32 *s_kreg, KeyTab &kt)
{
    kt.nkeys = ix.nkeys; kt.sh0 = ix.hdr[HDR_SH0]; kt.cs = ix.hdr[HDR_CS];
    kt.rmul = (u64)ix.hdr[HDR_RMUL_LO] | ((u64)ix.hdr[HDR_RMUL_HI] << 32);
    kt.lds = ix.nkeys <= KT_MAX;
    if (kt.lds) {
        for (u32 k = threadIdx.x; k < ix.nkeys; k += blockDim.x) {
            s_origin[k] = ix.origin[k];
            s_last[k] = ix.kcnt[k] ? (ix.span[k] >> kt.sh0) : 0xFFFFFFFFu;
            s_kreg[k] = ix.kreg[k];
        }
    }
}

#define KEYTAB_DISPATCH(kt_, body_) do { if ((kt_).lds) body_(std::true_type{}); else body_(std::false_type{}); } while (0)

// region of a probe row = region of the level-0 cell its START falls in (clamped into the key).  KLDS is a template
// parameter, not a run-time choice next to the loads: "LDS table or index column" in one expression compiles to flat loads.
// The kernels run their main loop once per case (KEYTAB_DISPATCH).
template <bool KLDS>
__device__ __forceinline__ u32 region_of(const JoinIndexView &ix, const KeyTab &kt, const i32 *s_origin, const u32 *s_last, const u32 *s_kreg, u32 k, i32 qs)
{
    if (k >= kt.nkeys) return NO_REGION;
    i32 origin; u32 last, kreg;
    if (KLDS) { origin = s_origin[k]; last = s_last[k]; kreg = s_kreg[k]; }
    else { origin = ix.origin[k]; last = ix.kcnt[k] ? (ix.span[k] >> kt.sh0) : 0xFFFFFFFFu; kreg = ix.kreg[k]; }
    if (last == 0xFFFFFFFFu) return NO_REGION;                    // cannot match anything
    const i64 d = (i64)qs - (i64)origin;
    const i64 c64 = d <= 0 ? 0 : (d >> kt.sh0);
    const u32 c = c64 > (i64)last ? last : (u32)c64;
    return kreg + (kt.cs != 0xFFFFFFFFu ? c >> kt.cs : (u32)(((u64)c * kt.rmul) >> 40));   // k_join_layout guarantees exactness
}

// LDS counter bump that returns the old value.  Sorted / clustered probe input sends a whole wavefront to
// the same counter; then one lane adds the wavefront's count and the lanes rank themselves by ballot,
// instead of 64 serialised same-address atomics.
__device__ __forceinline__ u32 lds_count_up(u32 *cnt, u32 d, bool active)
{
    const u64 act = __ballot(active);
    if (act == 0) return 0;
    const u32 first = (u32)__builtin_ctzll(act);
    const u32 d0 = __shfl(d, first, IVX_WAVE);
    const u64 same = __ballot(active && d == d0);
    if (same == act) {                                          // wave-uniform digit
        u32 base = 0;
        if (lane_id() == first) base = atomicAdd(&cnt[d0], (u32)__popcll(act));
        base = __shfl(base, first, IVX_WAVE);
        return base + mask_rank(act);
    }
    return active ? atomicAdd(&cnt[d], 1u) : 0u;
}

// The same for the FOUR consecutive rows a lane loads in one go (lane l of a wavefront holds rows 4l .. 4l + 3 of a 256-row
// stretch of the input): coordinate-sorted input puts the whole stretch into one region, and then one lane bumps the
// counter by 256 and every row's rank follows from its place in the stretch; anything else takes four plain LDS atomics per
// lane.  ONE test and one branch per four rows (lds_count_up spends two ballots, a shuffle and two or three branches on
// every row, and the partition is bound by the instructions it issues).
__device__ __forceinline__ void lds_count_up4(u32 *cnt, const u32 (&d)[4], u32 (&rank)[4])
{
    const u32 d0 = __builtin_amdgcn_readfirstlane(d[0]);
    const bool uni = d[0] == d0 && d[1] == d0 && d[2] == d0 && d[3] == d0 && d0 != NO_REGION;
    if (__builtin_amdgcn_ballot_w64(!uni) == 0) {
        u32 base = 0;
        const u32 ln = lane_id();
        if (ln == 0) base = atomicAdd(&cnt[d0], 4u * IVX_WAVE);
        base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
        for (int k = 0; k < 4; k++) rank[k] = base + ln * 4u + (u32)k;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) rank[k] = d[k] != NO_REGION ? atomicAdd(&cnt[d[k]], 1u) : 0u;
}

// four consecutive probe rows per lane: 16-byte loads when the columns are 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void load4(const u32 *__restrict__ pkey, const i32 *__restrict__ ps, const i32 *__restrict__ pe,
                                      u64 i, u64 hi, u32 (&k)[4], i32 (&s)[4], i32 (&e)[4])
{
    if (VEC && i + 4 <= hi) {
        const uint4 kv = pkey ? *reinterpret_cast<const uint4 *>(pkey + i) : make_uint4(0, 0, 0, 0);
        const int4 sv = *reinterpret_cast<const int4 *>(ps + i);
        k[0] = kv.x; k[1] = kv.y; k[2] = kv.z; k[3] = kv.w;
        s[0] = sv.x; s[1] = sv.y; s[2] = sv.z; s[3] = sv.w;
        if (pe) { const int4 ev = *reinterpret_cast<const int4 *>(pe + i); e[0] = ev.x; e[1] = ev.y; e[2] = ev.z; e[3] = ev.w; }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool ok = i + j < hi;
            k[j] = ok ? (pkey ? pkey[i + j] : 0u) : 0xFFFFFFFFu;       // key id 0xFFFFFFFF never matches
            s[j] = ok ? ps[i + j] : 0;
            e[j] = (ok && pe) ? pe[i + j] : 0;
        }
    }
}

// adj = 1 for the UDTFs' strict mode: the query is shrunk to [start+1, end-1] before anything else
// (interval_tree.rs:185-188, :253-256; i32 wrapping like the reference's release build)
// `unsorted` (device flag, preset 0) is raised when the rows are NOT already grouped by ascending region --
// a row of a smaller region after a larger one, or a row that cannot be routed.  If it stays 0 (probe input
// sorted by contig id and start: the usual state of genomic files) the partitioned order IS the input order
// and the scatter pass is skipped altogether.
// ND = digits of the pass: 256 for up to IVX_MAXREG regions, 1024 for up to IVX_MAXREG_WIDE (build sides of a few
// million rows: four times the table, shorter runs in the scatter, still one pass)
// SPLIT (more than IVX_MAXREG_WIDE regions): the digit is the SUPER-region = region / G (G = split.x, as a
// multiplication by split.y = ceil(2^32 / G), exact for region * G < 2^32); a second pass orders each super-region's
// rows by region % G (k_p2_*).  Sortedness is still judged on the regions themselves.
template <bool VEC, int ND, bool SPLIT = false>
__global__ __launch_bounds__(PA_T) void k_part_hist(JoinIndexView ix, const u32 *__restrict__ pkey, const i32 *__restrict__ ps,
                                                    u64 n, u32 nblk, u32 chunk, u32 *__restrict__ hist, u32 adj, u32 *unsorted,
                                                    uint2 split = make_uint2(1u, 0u))
{
    __shared__ u32 cnt[ND];
    __shared__ i32 s_origin[KT_MAX];
    __shared__ u32 s_last[KT_MAX], s_kreg[KT_MAX];
    __shared__ u32 s_unsorted;
    KeyTab kt;
    keytab_load(ix, s_origin, s_last, s_kreg, kt);
    if (threadIdx.x < ND) cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_unsorted = 0;
    __syncthreads();
    const u64 lo = (u64)blockIdx.x * chunk;
    const u64 hi = lo + chunk < n ? lo + chunk : n;
    auto body = [&](auto klds_tag) {
    constexpr bool KLDS = decltype(klds_tag)::value;
    for (u64 i0 = lo; i0 < hi; i0 += (u64)PA_T * 4) {
        u32 k[4]; i32 q[4], unused[4];
        const u64 i = i0 + (u64)threadIdx.x * 4;
        if (i >= hi) continue;
        load4<VEC>(pkey, ps, nullptr, i, hi, k, q, unused);
        u32 d[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            d[u] = region_of<KLDS>(ix, kt, s_origin, s_last, s_kreg, k[u], (i32)((u32)q[u] + adj));
            lds_count_up(cnt, SPLIT ? (u32)(((u64)d[u] * split.y) >> 32) : d[u], d[u] != NO_REGION);
        }
        if (!s_unsorted) {                                  // (once raised nobody needs to look any further)
            bool bad = false;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (i + u >= hi) break;
                bad |= d[u] == NO_REGION || (u && d[u] < d[u - 1]);
            }
            if (i + 3 < hi && i + 4 < n) {                  // the row after this thread's four: next thread, wavefront, loop step or workgroup
                const u32 dn = region_of<KLDS>(ix, kt, s_origin, s_last, s_kreg, pkey ? pkey[i + 4] : 0u, (i32)((u32)ps[i + 4] + adj));
                bad |= dn < d[3];
            }
            if (bad) s_unsorted = 1;
        }
    }
    };
    KEYTAB_DISPATCH(kt, body);
    __syncthreads();
    if (threadIdx.x < ND) hist[(u64)threadIdx.x * nblk + blockIdx.x] = cnt[threadIdx.x];
    if (threadIdx.x == 0 && s_unsorted) *unsorted = 1;
}

// order inside a region is irrelevant (the reference pins only the pair multiset), so the local
// rank of a row is just the value an LDS counter held when the row arrived
// RowT = u32: the row's index in the probe batch (join: it goes into the pair list);
// RowT = u16: its index inside this workgroup's chunk of at most two tiles (per-row-output operators: k_unpermute
// puts the chunk back in input order through LDS, so the chunk-local index is all that is needed)
template <bool VEC, typename RowT, int ND, bool SPLIT = false>
__global__ __launch_bounds__(PA_T) void k_part_scatter(JoinIndexView ix, const u32 *__restrict__ pkey, const i32 *__restrict__ ps,
                                                       const i32 *__restrict__ pe, u64 n, u32 nblk, const u32 *__restrict__ offs,
                                                       u64 *__restrict__ out_se, RowT *__restrict__ out_row, u32 chunk, u32 adj, const u32 *unsorted,
                                                       uint2 split = make_uint2(1u, 0u), unsigned char *__restrict__ out_sub = nullptr)
{
    __shared__ u64 r_se[PA_TILE];
    __shared__ unsigned short r_slot[PA_TILE];          // the row's slot in the tile (its row id follows from it)
    using DigT = typename std::conditional<(ND > 256), unsigned short, unsigned char>::type;
    __shared__ DigT r_dig[PA_TILE];
    __shared__ u32 dstart[ND], gbase[ND];              // dstart: the tile's counters first, then (in place) their exclusive scan
    __shared__ u32 scan_lds[PA_T / IVX_WAVE + 1];
    __shared__ i32 s_origin[KT_MAX];
    __shared__ u32 s_last[KT_MAX], s_kreg[KT_MAX];

    const u32 tid = threadIdx.x;
    if (*unsorted == 0) return;                             // input already in region order: nothing to move
    KeyTab kt;
    keytab_load(ix, s_origin, s_last, s_kreg, kt);
    if (tid < ND) gbase[tid] = offs[(u64)tid * nblk + blockIdx.x];
    const u64 lo = (u64)blockIdx.x * chunk;
    const u64 hi = lo + chunk < n ? lo + chunk : n;
    auto body = [&](auto klds_tag) {
    constexpr bool KLDS = decltype(klds_tag)::value;
    for (u64 t0 = lo; t0 < hi; t0 += PA_TILE) {
        if (tid < ND) dstart[tid] = 0;
        __syncthreads();
        u64 se[PA_I]; u32 dig[PA_I], lrank[PA_I];
        u32 kk[PA_I]; i32 qs[PA_I], qe[PA_I];
#pragma unroll
        for (int v = 0; v < PA_I / 4; v++) {
            u32 k4[4]; i32 s4[4], e4[4];
            load4<VEC>(pkey, ps, pe, t0 + ((u64)v * PA_T + tid) * 4, hi, k4, s4, e4);
#pragma unroll
            for (int j = 0; j < 4; j++) { kk[v * 4 + j] = k4[j]; qs[v * 4 + j] = s4[j]; qe[v * 4 + j] = e4[j]; }
        }
#pragma unroll
        for (int k = 0; k < PA_I; k++) {
            qs[k] = (i32)((u32)qs[k] + adj); qe[k] = (i32)((u32)qe[k] - adj);
            se[k] = (u64)(u32)qs[k] | ((u64)(u32)qe[k] << 32);
            u32 d = region_of<KLDS>(ix, kt, s_origin, s_last, s_kreg, kk[k], qs[k]);
            if (SPLIT && d != NO_REGION) {                       // digit = super-region; region % G rides along in the bits above it
                const u32 sup = (u32)(((u64)d * split.y) >> 32);
                d = sup | ((d - sup * split.x) << 10);
            }
            dig[k] = d;
            lrank[k] = lds_count_up(dstart, SPLIT ? (d & 1023u) : d, d != NO_REGION);
        }
        __syncthreads();
        u32 tot;
        const u32 mine = tid < ND ? dstart[tid] : 0u;
        const u32 ds = block_excl_scan<u32, PA_T>(mine, scan_lds, &tot);     // (barriers inside: every counter is read before any is overwritten)
        if (tid < ND) dstart[tid] = ds;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PA_I; k++) {
            if (dig[k] != NO_REGION) {
                const u32 pos = dstart[SPLIT ? (dig[k] & 1023u) : dig[k]] + lrank[k];
                r_se[pos] = se[k];
                r_slot[pos] = (unsigned short)(((k / 4) * PA_T + tid) * 4 + (k % 4));
                r_dig[pos] = (DigT)dig[k];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PA_I; k++) {
            const u32 j = k * PA_T + tid;
            if (j < tot) {
                const u32 dd = r_dig[j];
                const u32 d = SPLIT ? (dd & 1023u) : dd;
                const u64 g = (u64)gbase[d] + (j - dstart[d]);
                if (SPLIT) out_sub[g] = (unsigned char)(dd >> 10);
                const RowT row = (RowT)(t0 - (sizeof(RowT) == 2 ? lo : 0) + r_slot[j]);
                out_se[g] = r_se[j]; out_row[g] = row;
            }
        }
        __syncthreads();
        if (tid < ND) gbase[tid] += mine;
    }
    };
    KEYTAB_DISPATCH(kt, body);
}

// ------------------------------------------------------------------ one-pass partition into region pages
// The two-pass partition above reads the probe rows twice (histogram, then scatter) because a region's rows must end
// up contiguous, and where a region starts depends on every other tile.  Here a region's rows go to PAGES instead
// (2^lgpg rows each, taken from one pool on demand), so a tile needs nothing from the others but a position in its
// regions' row streams:
//   - the tile's rows are ranked by region in LDS as before; rows that cannot match anything are dropped first:
//     unknown keys, keys without build rows, rows that end before the key's first start, and rows whose blocks of
//     the build side's occupancy bitmap are all empty (filter_pass; the bitmap sits in L2, the rows stream past it);
//   - the thread that owns region r reserves the tile's run in r's stream with ONE returning atomicAdd on rcur[r]
//     (virtual row numbers v .. v+c-1); virtual page p of region r lives wherever ptab[r][p] says.  The tile whose run
//     holds a page's first row takes a page from the pool (atomicAdd on *pool_next) and publishes it; a tile that finds
//     the entry still empty polls it -- the publisher never waits for anything between its reservation and the
//     publication, so the poll ends (the entries are 4-byte granules written and read at agent scope);
//   - rows leave LDS as contiguous runs as before, into their pages.
// The probe kernels read region r's rows through the same table (PAGED).  Order inside a region is free, as everywhere.
// per-key tables of the one-pass partition.  KLDS (at most KT_MAX keys): cached in LDS; otherwise read from the index.
// The two sets are never mixed in one pointer: a pointer that may be LDS or global becomes flat loads with full waits.
struct KeyTab2 {
    const i32 *s_origin; const u32 *s_span, *s_kreg, *s_fbase;      // LDS; kreg = 0xFFFFFFFF: key has no build rows
    const u32 *fbits;
    u32 nkeys, sh0, cs, fg, rcells;
    u64 rmul;
};

template <bool KLDS>
__device__ __forceinline__ void keytab2_load(const JoinIndexView &ix, i32 *s_origin, u32 *s_span, u32 *s_kreg, u32 *s_fbase, KeyTab2 &kt, bool use_filter)
{
    kt.nkeys = ix.nkeys; kt.sh0 = ix.hdr[HDR_SH0]; kt.cs = ix.hdr[HDR_CS]; kt.fg = use_filter ? ix.hdr[HDR_FG] : 0xFFFFFFFFu;
    kt.rmul = (u64)ix.hdr[HDR_RMUL_LO] | ((u64)ix.hdr[HDR_RMUL_HI] << 32);
    kt.rcells = ix.hdr[HDR_RCELLS];
    kt.fbits = ix.fbits;
    if (KLDS) {
        for (u32 k = threadIdx.x; k < ix.nkeys; k += blockDim.x) {
            s_origin[k] = ix.origin[k]; s_span[k] = ix.span[k];
            s_kreg[k] = ix.kcnt[k] ? ix.kreg[k] : 0xFFFFFFFFu;
            s_fbase[k] = kt.fg != 0xFFFFFFFFu ? ix.fbase[k] : 0u;
        }
    }
    kt.s_origin = s_origin; kt.s_span = s_span; kt.s_kreg = s_kreg; kt.s_fbase = s_fbase;
}

// Which region a row is routed to, in two steps so that a thread can have the bitmap gathers of all its rows in flight
// together (a branch on one row's looked-up word would make the next row's gather wait for it):
//   route_prep   region of the row (NO_REGION: unknown key, key without build rows, row ends before the key's first
//                start) and the position of its window of the occupancy bitmap: first bit | (blocks - 1) << 26
//                (0x3F blocks-1 = more than 32 blocks: not tested)
//   route_test   whether any block of the window is set, given the 8 bytes that start at the 4-byte word holding the
//                window's first bit (up to 32 blocks always fit)
// PK: the row's packed form (ivx_regions.hpp): `packed` = start | length << 24 as a 64-bit value, or PK_ESCAPE.
constexpr u64 PK_ESCAPE = ~0ull;
template <bool KLDS, bool FILT, bool PK>
__device__ __forceinline__ u32 route_prep(const JoinIndexView &ix, const KeyTab2 &kt, u32 k, i32 qs, i32 qe, u32 &fpos, u64 &packed, u32 maxlen)
{
    const bool kok = k < kt.nkeys;
    const u32 kk = kok ? k : 0u;
    const u32 kreg = KLDS ? kt.s_kreg[kk] : (ix.kcnt[kk] ? ix.kreg[kk] : 0xFFFFFFFFu);
    const i32 o = KLDS ? kt.s_origin[kk] : ix.origin[kk];
    const u32 span = KLDS ? kt.s_span[kk] : ix.span[kk];
    // qe - o and qs - o in 32 bits: exact as unsigned numbers whenever they are not negative, which one signed compare tells
    // (the partition is bound by the instructions it issues as much as by its LDS phases; 64-bit differences, shifts and
    // clamps were a sixth of them)
    const bool hi_ok = qe >= o;                                     // else: every build row of the key starts behind qe
    const bool d_ok = qs >= o;
    const u32 hi32 = (u32)qe - (u32)o, d32 = (u32)qs - (u32)o;
    const bool ok = kok & (kreg != 0xFFFFFFFFu) & hi_ok;
    fpos = 0;
    if (FILT) {
        const u32 lastb = (span >> kt.fg) + 1u;                     // the overflow block
        const u32 x0 = d_ok ? d32 >> kt.fg : 0u, x1 = hi_ok ? hi32 >> kt.fg : 0u;
        const u32 c0 = x0 > lastb ? lastb : x0, c1 = x1 > lastb ? lastb : x1;
        const u32 b0 = c0 < c1 ? c0 : c1, b1 = c0 < c1 ? c1 : c0;   // (a row with end < start matches build rows that contain [end, start])
        const u32 nb1 = b1 - b0;                                    // blocks - 1
        const u32 fb = KLDS ? kt.s_fbase[kk] : ix.fbase[kk];
        fpos = ok ? (fb + b0) | ((nb1 > 31u ? 0x3Fu : nb1) << 26) : 0u;
    }
    const u32 last = span >> kt.sh0;
    const u32 cc = d_ok ? d32 >> kt.sh0 : 0u;
    const u32 c = cc > last ? last : cc;
    const u32 rin = kt.cs != 0xFFFFFFFFu ? c >> kt.cs : (u32)(((u64)c * kt.rmul) >> 40);    // region inside the key
    packed = PK_ESCAPE;
    if (PK) {
        // for d >= 0 the region's first coordinate (rin * R << sh0 <= span) is at most d, and for end >= start the length
        // is below 2^32
        const u32 rel = d32 - ((rin * kt.rcells) << kt.sh0);
        const u32 len = (u32)qe - (u32)qs;
        if (d_ok && rel < (1u << 24) && qe >= qs && len < maxlen) packed = (u64)rel | ((u64)len << 24);
    }
    return ok ? kreg + rin : NO_REGION;
}

__device__ __forceinline__ bool route_test(u32 fpos, u64 win)
{
    const u32 nb1 = fpos >> 26;
    const u64 m = (2ull << (nb1 & 31u)) - 1ull;
    return (nb1 == 0x3Fu) | (((win >> (fpos & 31u)) & m) != 0);
}


__device__ __forceinline__ u32 page_wait(u32 *slot)
{
    u32 v;
    while ((v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u) __builtin_amdgcn_s_sleep(2);
    return v - 1u;
}

// four consecutive rows per lane, streamed past the caches' keep-lists (the occupancy bitmap should stay in L2)
template <bool VEC>
__device__ __forceinline__ void load4nt(const u32 *__restrict__ pkey, const i32 *__restrict__ ps, const i32 *__restrict__ pe,
                                        u64 i, u64 hi, u32 (&k)[4], i32 (&s)[4], i32 (&e)[4])
{
    if (VEC && i + 4 <= hi) {
        typedef u32 __attribute__((ext_vector_type(4))) v4u;
        typedef i32 __attribute__((ext_vector_type(4))) v4i;
        const v4u kv = pkey ? __builtin_nontemporal_load(reinterpret_cast<const v4u *>(pkey + i)) : v4u{0u, 0u, 0u, 0u};
        const v4i sv = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(ps + i));
        const v4i ev = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(pe + i));
        k[0] = kv.x; k[1] = kv.y; k[2] = kv.z; k[3] = kv.w;
        s[0] = sv.x; s[1] = sv.y; s[2] = sv.z; s[3] = sv.w;
        e[0] = ev.x; e[1] = ev.y; e[2] = ev.z; e[3] = ev.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool ok = i + j < hi;
            k[j] = ok ? (pkey ? pkey[i + j] : 0u) : 0xFFFFFFFFu;
            s[j] = ok ? ps[i + j] : 0;
            e[j] = ok ? pe[i + j] : 0;
        }
    }
}

// CH rows of a thread (CH / 4 quads; quad q of a tile = rows (q * T + tid) * 4 .. + 3 from t0) into registers.  `whole`
// (wave-uniform): the quads lie inside the workgroup's rows and the columns are 16-byte aligned -- 16-byte loads streamed
// past the caches' keep-lists; otherwise element by element, checked against hi
template <int CH, int T>
__device__ __forceinline__ void part_load_rows(const u32 *__restrict__ pkey, const i32 *__restrict__ ps, const i32 *__restrict__ pe,
                                               u64 t0, int quad0, u64 hi, bool whole, u32 (&kk)[CH], i32 (&qs)[CH], i32 (&qe)[CH])
{
    const u32 tid = threadIdx.x;
    if (whole) {
        typedef u32 __attribute__((ext_vector_type(4))) v4u;
        typedef i32 __attribute__((ext_vector_type(4))) v4i;
        // a wave-uniform 64-bit base and the thread's 32-bit offset: one address register for all of a thread's loads.  The
        // offset is made opaque here, or column + offset is kept as three 64-bit per-thread pointers across the whole tile
        // loop (six registers that the rows loaded ahead need)
        u32 o = tid * 4u;
        asm volatile("" : "+v"(o));
#pragma unroll
        for (int v = 0; v < CH / 4; v++) {
            const u64 q = t0 + (u64)(quad0 + v) * T * 4;
            const v4u kv = pkey ? __builtin_nontemporal_load(reinterpret_cast<const v4u *>(pkey + q + o)) : v4u{0u, 0u, 0u, 0u};
            const v4i sv = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(ps + q + o));
            const v4i ev = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(pe + q + o));
            kk[v * 4] = kv.x; kk[v * 4 + 1] = kv.y; kk[v * 4 + 2] = kv.z; kk[v * 4 + 3] = kv.w;
            qs[v * 4] = sv.x; qs[v * 4 + 1] = sv.y; qs[v * 4 + 2] = sv.z; qs[v * 4 + 3] = sv.w;
            qe[v * 4] = ev.x; qe[v * 4 + 1] = ev.y; qe[v * 4 + 2] = ev.z; qe[v * 4 + 3] = ev.w;
        }
    } else {
#pragma unroll
        for (int v = 0; v < CH / 4; v++) {
            u32 k4[4]; i32 s4[4], e4[4];
            load4nt<false>(pkey, ps, pe, t0 + ((u64)(quad0 + v) * T + tid) * 4, hi, k4, s4, e4);
#pragma unroll
            for (int j = 0; j < 4; j++) { kk[v * 4 + j] = k4[j]; qs[v * 4 + j] = s4[j]; qe[v * 4 + j] = e4[j]; }
        }
    }
}

// Whether an instantiation of k_part_onepass loads its rows one stage AHEAD of their use (see there).  The rows loaded
// ahead occupy a chunk's raw columns (3 * CH registers) through the rest of the tile, and the kernel is held to 128
// registers (two workgroups per CU).  With aligned columns (VEC) that fits without scratch where a chunk is eight rows and the
// bitmap is not in use: the 16-row packed tiles without filter (the join's usual form) and all the 8-row tiles (1024
// digits).  The 12-row tiles (one chunk of twelve) and the filtered 16-row tiles would spill three to four times what they
// spill already: they keep loading each chunk at its top.  (profiles/route_prefetch_ab.txt has the resource table.)
template <bool VEC, int I, bool FILT>
constexpr bool part_loads_ahead() { return !(VEC && (I == 12 || (I == 16 && FILT))); }

// ND digits (256 / 1024), T threads, I rows per thread and tile (tile = T * I rows <= one page).  Packed rows need no
// slot array in LDS: two 512-thread workgroups with 8192-row tiles then share a CU, and one's loads overlap the other's
// LDS phases (the kernel is bound by those phases, not by HBM: 8-byte instead of 12-byte rows alone changed nothing)
// Big batches of the join's packed, unfiltered form take 16384-row tiles in ONE 1024-thread workgroup per CU instead
// (T = 1024, 153 672 B of LDS; ivx_route_paged): the runs written to HBM double and what a tile pays per REGION -- the
// rcur atomic, the page look-up, the wtab entry -- is shared by twice the rows, which at 80 M rows and more outweighs the
// partner workgroup (the rank of a row in its tile still fits the 14 bits beside the digit: 16383)
// PK: a routed row is ONE 8-byte word, (start inside its region | length) and the row id (route_prep), instead of
// (start, end) in one array and the row id in another: a third fewer bytes written here and read by the probe
//
// A workgroup walks chunk / TILE consecutive tiles.  Per tile: load the rows (a chunk of CH per thread at a time), route
// them (route_prep), count them per region in LDS, barrier, reserve the runs (rcur) and scan the counts, barrier, re-order
// the rows in LDS by region while the reservations return, take / look up the pages, barrier, write the runs out,
// barrier.  At four wavefronts per SIMD the latency of the row loads is not covered by other wavefronts, so the loads run
// one stage ahead of their use (AHEAD, part_loads_ahead): a chunk's raw columns are dead once it is routed, and the next
// chunk's -- or the next tile's first chunk's -- are loaded into the same registers right then:
//     tile k:   [load c0]* route c0 | LOAD c1 | count c0 | route c1 | LOAD c0 of tile k + 1 | count c1 | barrier | reserve,
//               scan | re-order | pages | write-out | barrier
//     tile k+1: dstart cleared, barrier | route c0 (no load) | LOAD c1 | ...
// (* only a workgroup's first tile, a partial tile and unaligned columns load here.)  What is in flight when: chunk 1's loads
// during chunk 0's LDS counting; the next tile's during chunk 1's counting, the barrier and the scan -- they have landed
// by the time the reservation's return value is waited for, which is before the write-out.  A tile's stores, the closing
// barrier and the next tile's dstart barrier no longer stand between a tile and its first rows.
// Nothing else differs from the order without it: same barriers, same reservation and publication protocol, no wait on
// another workgroup that was not there before.
template <bool VEC, int ND, int I, bool KLDS, bool FILT, bool PK, int T = PA_T>
__global__ __launch_bounds__(T, 4) void k_part_onepass(JoinIndexView ix, const u32 *__restrict__ pkey, const i32 *__restrict__ ps,
                                                       const i32 *__restrict__ pe, u64 n, u32 chunk, u32 *__restrict__ rcur, PageTab pt,
                                                       u32 *pool_next, u64 *__restrict__ out_se, u32 *__restrict__ out_row, u32 rowbits,
                                                       u32 adj = 0, uint2 *__restrict__ vtab = nullptr)
{
    // adj = 1: the UDTFs' strict mode shrinks the query to [start+1, end-1] before anything else (interval_tree.rs:185-188)
    // vtab (per-row-value operators): [tile][region] -> (virtual start, rows) of the tile's run, for the un-permute
    constexpr int TILE = T * I;
    static_assert(ND <= T, "one thread per region");
    __shared__ u64 r_se[TILE];
    __shared__ unsigned short r_slot[PK ? 1 : TILE];            // (packed rows carry their row id with them)
    using DigT = typename std::conditional<(ND > 256), unsigned short, unsigned char>::type;
    __shared__ DigT r_dig[TILE];
    __shared__ u32 dstart[ND];
    __shared__ uint2 wtab[ND];                                   // per region, for the write-out: {virtual row of the run - its LDS start, first pool page | its page slot << 16}
    __shared__ u32 scan_lds[T / IVX_WAVE + 1];
    __shared__ i32 s_origin[KT_MAX];
    __shared__ u32 s_span[KT_MAX], s_kreg[KT_MAX], s_fbase[KT_MAX];

    const u32 tid = threadIdx.x;
    KeyTab2 kt;
    keytab2_load<KLDS>(ix, s_origin, s_span, s_kreg, s_fbase, kt, FILT);
    const u32 pmask = (1u << pt.lgpg) - 1u;
    const u64 lo = (u64)blockIdx.x * chunk;
    const u64 hi = lo + chunk < n ? lo + chunk : n;
    // the tile's rows in chunks of CH per thread (all of them, or eight at a time when a thread holds sixteen: the raw
    // columns of sixteen rows plus their routed form do not fit the registers)
    constexpr int CH = (I % 8 == 0 && I > 8) ? 8 : I;
    constexpr bool AHEAD = part_loads_ahead<VEC, I, FILT>();
    // the raw columns of ONE chunk: the only registers rows are loaded into.  AHEAD: they are loaded one stage before they
    // are used, at the point where the chunk before has been routed and no longer needs them (see the chunk loop)
    u32 kk[CH]; i32 qs[CH], qe[CH];
    bool ahead = false;                                      // wave-uniform: kk / qs / qe hold (or wait for) this tile's first chunk
    for (u64 t0 = lo; t0 < hi; t0 += TILE) {
        if (tid < ND) dstart[tid] = 0;
        __syncthreads();
        u64 se[PK ? 1 : I]; u32 plo[PK ? I : 1], dig[I];     // PK: low word of the packed row (the length's bits above its low 8 ride in dig)
        const bool whole = VEC && t0 + TILE <= hi;
#pragma unroll
        for (int c0 = 0; c0 < I; c0 += CH) {
            // What is in flight when.  A chunk's rows are loaded, routed (route_prep: straight-line code, no per-row
            // branches), tested against the bitmap (all gathers of the chunk in flight together) and counted in LDS.  Its raw
            // columns are dead once route_prep has turned them into dig / plo / fpos, so AHEAD issues the NEXT stage's row
            // loads right there, into the same registers, and they fly while this chunk gathers and counts:
            //   - not the last chunk: the tile's next chunk;
            //   - the last chunk: the first chunk of the workgroup's next tile, if that tile is whole and the columns are
            //     aligned (`ahead`, wave-uniform; nothing at or beyond hi <= n is touched).  Those loads also fly through
            //     the reservation, the LDS re-order, the write-out, the closing barrier and the next tile's dstart
            //     barrier, and the next iteration starts routing without loading.
            // Only a workgroup's first tile, a partial last tile and unaligned columns load at the top of the tile.
            // !AHEAD (the order before): every chunk loads its own rows at its top.
            if (c0 == 0 ? !ahead : !AHEAD) part_load_rows<CH, T>(pkey, ps, pe, t0, c0 / 4, hi, whole, kk, qs, qe);
            u32 fpos[CH];
#pragma unroll
            for (int k = 0; k < CH; k++) {
                u64 packed;
                const u32 maxlen = pk_maxlen(rowbits);
                const i32 s1 = (i32)((u32)qs[k] + adj), e1 = (i32)((u32)qe[k] - adj);
                dig[c0 + k] = route_prep<KLDS, FILT, PK>(ix, kt, kk[k], s1, e1, fpos[k], packed, maxlen);
                if (PK) {
                    const u32 lenf = packed == PK_ESCAPE ? maxlen : (u32)(packed >> 24);
                    plo[PK ? c0 + k : 0] = (packed == PK_ESCAPE ? 0u : (u32)packed & 0xFFFFFFu) | (lenf << 24);
                    fpos[k] = FILT ? fpos[k] : (lenf >> 8);       // (parked until the row's rank is known; with the bitmap in use lengths keep to 8 bits)
                } else se[PK ? 0 : c0 + k] = (u64)(u32)s1 | ((u64)(u32)e1 << 32);
            }
            if (AHEAD) {
                asm volatile("" ::: "memory");                  // (the loads below stay below the routing above: no second set of raw columns)
                if (c0 + CH < I) part_load_rows<CH, T>(pkey, ps, pe, t0, (c0 + CH) / 4, hi, whole, kk, qs, qe);
                else {
                    ahead = VEC && t0 + TILE < hi && t0 + 2 * (u64)TILE <= hi;
                    if (ahead) part_load_rows<CH, T>(pkey, ps, pe, t0 + TILE, 0, hi, true, kk, qs, qe);
                }
            }
            if (FILT) {
                u64 win[CH];
#pragma unroll
                for (int k = 0; k < CH; k++) __builtin_memcpy(&win[k], kt.fbits + ((fpos[k] & 0x3FFFFFFu) >> 5), sizeof(u64));
#pragma unroll
                for (int k = 0; k < CH; k++) dig[c0 + k] = route_test(fpos[k], win[k]) ? dig[c0 + k] : NO_REGION;
            }
#pragma unroll
            for (int v = 0; v < CH / 4; v++) {                  // region and rank share a register from here on (10 + 14 bits)
                const u32 d4[4] = {dig[c0 + v * 4], dig[c0 + v * 4 + 1], dig[c0 + v * 4 + 2], dig[c0 + v * 4 + 3]};
                u32 lr[4];
                lds_count_up4(dstart, d4, lr);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int k = v * 4 + u;
                    const u32 lhi = (PK && !FILT) ? fpos[k] << 24 : 0u;
                    dig[c0 + k] = dig[c0 + k] == NO_REGION ? NO_REGION : (dig[c0 + k] | (lr[u] << 10) | lhi);
                }
            }
            if (!AHEAD && CH != I) asm volatile("" ::: "memory");   // (keeps the next chunk's loads from being hoisted above this chunk's work)
        }
        __syncthreads();
        // ---- reserve the tile's run in every region's row stream; take / look up the pages it touches
        const u32 mine = tid < ND ? dstart[tid] : 0u;
        // (the thread's slots in rcur, vtab and ptab are addressed from a copy of tid that is opaque per tile: their three
        // 64-bit addresses are computed where they are used, not held in six registers across the tile loop)
        u32 tidt = tid;
        asm volatile("" : "+v"(tidt));
        u32 v = 0;
        if (mine) v = atomicAdd(&rcur[tidt], mine);
        if (vtab && tid < ND) vtab[(u64)(t0 / TILE) * ND + tidt] = make_uint2(v, mine);
        u32 tot;
        const u32 ds = block_excl_scan<u32, T>(mine, scan_lds, &tot);     // (barriers inside: every counter is read before any is overwritten)
        if (tid < ND) dstart[tid] = ds;
        __syncthreads();
        // (the returned v is first needed after the LDS re-order below, which runs while the atomics are in flight)
#pragma unroll
        for (int k = 0; k < I; k++) {
            if (dig[k] != NO_REGION) {
                const u32 d = dig[k] & 1023u;
                const u32 pos = dstart[d] + ((dig[k] >> 10) & 0x3FFFu);
                if (PK) {
                    const u32 row = (u32)(t0 + (u32)(((k / 4) * T + tid) * 4 + (k % 4)));
                    r_se[pos] = (u64)plo[PK ? k : 0] | ((u64)(row | (rowbits < 32 ? (dig[k] >> 24) << rowbits : 0u)) << 32);
                } else {
                    r_se[pos] = se[PK ? 0 : k];
                    r_slot[pos] = (unsigned short)(((k / 4) * T + tid) * 4 + (k % 4));
                }
                r_dig[pos] = (DigT)d;
            }
        }
        if (mine) {
            u32 *row = pt.ptab + (u64)tidt * pt.pstride;
            const u32 p0 = v >> pt.lgpg, p1 = (v + mine - 1u) >> pt.lgpg;       // TILE <= page: at most one page border inside the run
            const bool own0 = (v & pmask) == 0u, own1 = p1 != p0;
            u32 got = 0;
            if (own0 || own1) {
                got = atomicAdd(pool_next, (own0 ? 1u : 0u) + (own1 ? 1u : 0u));
                if (own0) __hip_atomic_store(&row[p0], got + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (own1) __hip_atomic_store(&row[p1], got + (own0 ? 2u : 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            wtab[tid] = make_uint2(v - ds, (own0 ? got : page_wait(&row[p0])) | (p0 << 16));    // (pool pages and page slots number at most ~5000: host)
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < I; k++) {
            const u32 j = k * T + tid;
            if (j < tot) {
                const u32 d = r_dig[j];
                const uint2 w = wtab[d];                                        // (one 8-byte LDS read instead of three lookups)
                const u32 x = w.x + j;                                          // virtual row number in region d
                u32 pg = w.y & 0xFFFFu;
                if ((x >> pt.lgpg) != (w.y >> 16)) pg = page_wait(pt.ptab + (u64)d * pt.pstride + (x >> pt.lgpg));   // the run's second page
                const u64 g = ((u64)pg << pt.lgpg) + (x & pmask);
                out_se[g] = r_se[j];
                if (!PK) out_row[g] = (u32)(t0 + r_slot[j]);
            }
        }
        __syncthreads();
    }
}

// first routed row of every region (exclusive scan of the regions' row counts; nreg <= IVX_MAXREG_WIDE), as the probe
// kernels' region table
__global__ __launch_bounds__(1024) void k_page_bounds(const u32 *__restrict__ rcur, u32 nreg, u32 *__restrict__ rfirst)
{
    __shared__ u32 red[1024 / IVX_WAVE + 1];
    const u32 t = threadIdx.x;
    u32 tot;
    const u32 ex = block_excl_scan<u32, 1024>(t < nreg ? rcur[t] : 0u, red, &tot);
    if (t < nreg) rfirst[t] = ex;
    if (t == 0) rfirst[nreg] = tot;
}

// first routed row (rfirst) and first chunk (cfirst) of every region; nreg <= IVX_MAXREG_WIDE
__global__ __launch_bounds__(1024) void k_chunk_bounds(const u32 *__restrict__ rcur, u32 nreg, u32 *__restrict__ rfirst, u32 *__restrict__ cfirst)
{
    __shared__ u32 red[1024 / IVX_WAVE + 1];
    const u32 t = threadIdx.x;
    const u32 rows = t < nreg ? rcur[t] : 0u;
    u32 tot;
    const u32 ex = block_excl_scan<u32, 1024>(rows, red, &tot);
    if (t < nreg) rfirst[t] = ex;
    if (t == 0) rfirst[nreg] = tot;
    __syncthreads();
    const u32 ec = block_excl_scan<u32, 1024>((rows + FP_CHUNK - 1) / FP_CHUNK, red, &tot);
    if (t < nreg) cfirst[t] = ec;
    if (t == 0) cfirst[nreg] = tot;
}

// what the one-pass partition wants zeroed before it starts, in one launch: its counters, the page table and (nullable) two
// words of the caller's
__global__ __launch_bounds__(256) void k_route_clear(u32 *__restrict__ ctl, u32 nctl, u32 *__restrict__ ptab, u64 nptab, u64 *zero2)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x, step = (u64)gridDim.x * 256;
    if (i < nctl) ctl[i] = 0;                                           // (nctl < 256 * gridDim.x: the host sizes the grid)
    if (i < 2 && zero2) zero2[i] = 0;
    uint4 *p4 = (uint4 *)ptab;                                          // (scratch: 256-byte aligned)
    for (u64 j = i; j < nptab / 4; j += step) p4[j] = make_uint4(0u, 0u, 0u, 0u);
    if (i < (nptab & 3)) ptab[(nptab & ~3ull) + i] = 0;
}

// the one-pass partition's 16384-row tiles (ivx_route_paged): from this many rows on, this many tiles per workgroup.
// Measured (profiles/route_bigtile_ab.txt): at 50 M and 64 M rows the form times like the 8192-row one with four tiles
// per workgroup and is 2-5 % behind it with one or two (one workgroup per CU: nothing covers a workgroup's first tile,
// the only one not loaded ahead); from 80 M rows on it is ahead, by 3 % at 100 M
constexpr u64 PART_BIG_ROWS = 80ull * 1000 * 1000;
constexpr u32 PART_BIG_TILES = 4;

// rows one partition workgroup takes: 1, 2 or 4 tiles, so that mid-size batches still spread over all CUs
static inline u32 part_chunk(u64 n, u32 max_tiles = 4) { const u32 t = n >= (16u << 20) ? 4u : n >= (4u << 20) ? 2u : 1u; return (u32)PA_TILE * (t < max_tiles ? t : max_tiles); }

// ------------------------------------------------------------------ values back into input order
// The scatter wrote, for every (region, workgroup chunk), one contiguous run, and kept each row's index
// inside its chunk (one or two tiles).  So the values of one chunk are ~200 runs of the value stream: read them
// (each wavefront a contiguous 1/16 of the chunk's values, coalesced inside runs), drop them at their
// chunk-local index in LDS, write the chunk out in input order.  Rows that were never routed (unknown key,
// key without build rows) keep the zero LDS was cleared to -- the reference's answer for them.
constexpr u32 UP_CHUNK = 2u * PA_TILE;               // the per-row-output path keeps chunks at two tiles (values of a chunk sit in LDS; u16 chunk-local ids)

// OUT: UP_I64 zero-extended (count), UP_I64S sign-extended (coverage), UP_U32 (rle_right; the workgroup's sum
// goes to *total), UP_U8 (exists = value != 0)
enum { UP_I64 = 0, UP_I64S = 1, UP_U32 = 2, UP_U8 = 3 };
template <int OUT>
__device__ __forceinline__ void up_store(void *out, u64 i, u32 v)
{
    if (OUT == UP_I64) ((i64 *)out)[i] = (i64)v;
    else if (OUT == UP_I64S) ((i64 *)out)[i] = (i64)(i32)v;
    else if (OUT == UP_U32) ((u32 *)out)[i] = v;
    else ((u8 *)out)[i] = v != 0;
}

template <int OUT, int ND>
__global__ __launch_bounds__(PA_T) void k_unpermute(const u32 *__restrict__ val, const unsigned short *__restrict__ cidx,
                                                    const u32 *__restrict__ offs, u32 nblk, u32 chunk, u32 nreg, u64 n, void *__restrict__ out,
                                                    const u32 *unsorted, unsigned long long *total, int sorted_done = 0)
{
    __shared__ u64 s_sum[PA_T / IVX_WAVE];
    u64 mysum = 0;
    if (*unsorted == 0 && sorted_done) return;              // (routed callers: another kernel answered the unmoved rows in place)
    if (*unsorted == 0) {                                   // values already sit in input order
        const u64 lo0 = (u64)blockIdx.x * chunk;
        const u64 hi0 = lo0 + chunk < n ? lo0 + chunk : n;
        for (u64 t = lo0 + threadIdx.x; t < hi0; t += PA_T) { const u32 v = val[t]; up_store<OUT>(out, t, v); mysum += v; }
        if (OUT == UP_U32 && total) { const u64 b = block_sum<u64, PA_T>(mysum, s_sum); if (threadIdx.x == 0 && b) atomicAdd(total, (unsigned long long)b); }
        return;
    }
    __shared__ u32 s_val[UP_CHUNK];
    __shared__ u32 s_pre[ND + 1], s_g[ND];
    __shared__ u32 scan_lds[PA_T / IVX_WAVE + 1];
    const u32 tid = threadIdx.x, blk = blockIdx.x;
    const u64 lo = (u64)blk * chunk;
    const u32 len = (u32)(lo + chunk < n ? chunk : n - lo);
    u32 c = 0, g = 0;
    if (tid < nreg) { g = offs[(u64)tid * nblk + blk]; c = offs[(u64)tid * nblk + blk + 1] - g; }
    u32 tot;
    const u32 ex = block_excl_scan<u32, PA_T>(c, scan_lds, &tot);
    if (tid < ND) { s_pre[tid] = ex; s_g[tid] = g; }
    if (tid == 0) s_pre[ND] = tot;
    for (u32 t = tid; t < chunk; t += PA_T) s_val[t] = 0;
    __syncthreads();
    // wavefront w owns elements [w*per, (w+1)*per) of the chunk's region-major value list
    const u32 wv = tid / IVX_WAVE, ln = lane_id();
    const u32 per = (tot + PA_T / IVX_WAVE - 1) / (PA_T / IVX_WAVE);
    const u32 t_lo = wv * per, t_hi = t_lo + per < tot ? t_lo + per : tot;
    u32 r = 0;
    if (t_lo < t_hi) { u32 a = 0, b = ND; while (a < b) { const u32 m = (a + b + 1) >> 1; if (s_pre[m] <= t_lo + ln && m < ND) a = m; else b = m - 1; } r = a; }
    for (u32 t = t_lo + ln; t < t_hi; t += IVX_WAVE) {
        while (r + 1 < ND && s_pre[r + 1] <= t) r++;
        const u64 at = (u64)s_g[r] + (t - s_pre[r]);
        s_val[cidx[at]] = val[at];
    }
    __syncthreads();
    for (u32 t = tid; t < len; t += PA_T) { const u32 v = s_val[t]; up_store<OUT>(out, lo + t, v); mysum += v; }
    if (OUT == UP_U32 && total) { const u64 b = block_sum<u64, PA_T>(mysum, s_sum); if (tid == 0 && b) atomicAdd(total, (unsigned long long)b); }
}

// The same for rows routed by the one-pass partition (packed rows in region pages): the probe left every row's value in the
// low half of its packed word, the row id above it.  One workgroup per partition tile: vtab[tile][region] says where the
// tile's run of every region went (virtual start, rows); the words are read back run by run (each wavefront a contiguous
// share of the tile's words), dropped at row - tile start in LDS and written out in input order.
template <int OUT, int TILE>
__global__ __launch_bounds__(512) void k_unpermute_paged(const u64 *__restrict__ pool, const uint2 *__restrict__ vtab, PageTab pt, u32 nreg, u32 rowbits,
                                                         u64 n, void *__restrict__ out, unsigned long long *total)
{
    constexpr int T = 512, ND = 256;
    __shared__ u32 s_val[TILE];
    __shared__ u32 s_pre[ND + 1], s_v[ND], s_pg0[ND];
    __shared__ u32 scan_lds[T / IVX_WAVE + 1];
    __shared__ u64 s_sum[T / IVX_WAVE];
    const u32 tid = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * TILE;
    const u32 len = (u32)(t0 + TILE < n ? (u64)TILE : n - t0);
    const u32 rowmask = rowbits >= 32 ? 0xFFFFFFFFu : (1u << rowbits) - 1u;
    const u32 pmask = (1u << pt.lgpg) - 1u;
    u32 v = 0, c = 0;
    if (tid < nreg) { const uint2 vc = vtab[(u64)blockIdx.x * ND + tid]; v = vc.x; c = vc.y; }
    u32 tot;
    const u32 ex = block_excl_scan<u32, T>(c, scan_lds, &tot);
    if (tid < ND) { s_pre[tid] = ex; s_v[tid] = v; s_pg0[tid] = c ? pt.ptab[(u64)tid * pt.pstride + (v >> pt.lgpg)] - 1u : 0u; }
    if (tid == 0) s_pre[ND] = tot;
    for (u32 t = tid; t < TILE; t += T) s_val[t] = 0;           // rows that were never routed keep 0: the reference's answer for them
    __syncthreads();
    const u32 wv = tid / IVX_WAVE, ln = lane_id();
    const u32 per = (tot + T / IVX_WAVE - 1) / (T / IVX_WAVE);
    const u32 j_lo = wv * per, j_hi = j_lo + per < tot ? j_lo + per : tot;
    u32 r = 0;
    if (j_lo < j_hi) { u32 a = 0, b = ND; while (a < b) { const u32 m = (a + b + 1) >> 1; if (m < ND && s_pre[m] <= j_lo + ln) a = m; else b = m - 1; } r = a; }
    for (u32 j = j_lo + ln; j < j_hi; j += IVX_WAVE) {
        while (r + 1 < ND && s_pre[r + 1] <= j) r++;
        const u32 x = s_v[r] + (j - s_pre[r]);                  // virtual row number in region r
        u32 pg = s_pg0[r];
        if ((x >> pt.lgpg) != (s_v[r] >> pt.lgpg)) pg = pt.ptab[(u64)r * pt.pstride + (x >> pt.lgpg)] - 1u;   // the run's second page
        const u64 w = pool[((u64)pg << pt.lgpg) + (x & pmask)];
        const u32 slot = ((u32)(w >> 32) & rowmask) - (u32)t0;
        if (slot < (u32)TILE) s_val[slot] = (u32)w;
    }
    __syncthreads();
    u64 mysum = 0;
    for (u32 t = tid; t < len; t += T) { const u32 val = s_val[t]; up_store<OUT>(out, t0 + t, val); mysum += val; }
    if (OUT == UP_U32 && total) { const u64 b = block_sum<u64, T>(mysum, s_sum); if (tid == 0 && b) atomicAdd(total, (unsigned long long)b); }
}

// The record-wide sibling (the overlap aggregates: a row's result does not fit its word).  rec.* hold one value per word of
// the page pool, at the word's own index; the tile's words are walked as above, once per wanted output: the output's records
// are dropped at row - tile start in LDS, over the empty result's value for the rows that were never routed, and written out
// in input order.  The words' second and later reads hit the cache (64 KB a tile).
// RECS says what the outputs are: io.each(pass) calls pass(an output's records, the caller's column, the value of a row that
// was never routed) once per output.
struct AggRecs {
    AggOut rec, out;
    template <class P> __device__ __forceinline__ void each(P &&pass) const
    {
        pass(rec.count, out.count, 0ull);
        pass(rec.sum, out.sum, 0ull);
        pass(rec.vmin, out.vmin, (u64)INT64_MAX);
        pass(rec.vmax, out.vmax, (u64)INT64_MIN);
        pass(rec.bases, out.bases, 0ull);
        pass(rec.wsum, out.wsum, 0ull);
    }
};
struct SelRecs {
    SelOut rec, out;
    template <class P> __device__ __forceinline__ void each(P &&pass) const
    {
        pass(rec.idx, out.idx, (u64)IVX_NULL_IDX);
        pass(rec.score, out.score, 0ull);
    }
};
template <int TILE, class RECS>
__global__ __launch_bounds__(512) void k_unpermute_records(const u64 *__restrict__ pool, const uint2 *__restrict__ vtab, PageTab pt, u32 nreg, u32 rowbits,
                                                           u64 n, RECS io)
{
    constexpr int T = 512, ND = 256;
    __shared__ u64 s_val[TILE];
    __shared__ u32 s_pre[ND + 1], s_v[ND], s_pg0[ND];
    __shared__ u32 scan_lds[T / IVX_WAVE + 1];
    const u32 tid = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * TILE;
    const u32 len = (u32)(t0 + TILE < n ? (u64)TILE : n - t0);
    const u32 rowmask = rowbits >= 32 ? 0xFFFFFFFFu : (1u << rowbits) - 1u;
    const u32 pmask = (1u << pt.lgpg) - 1u;
    u32 v = 0, c = 0;
    if (tid < nreg) { const uint2 vc = vtab[(u64)blockIdx.x * ND + tid]; v = vc.x; c = vc.y; }
    u32 tot;
    const u32 ex = block_excl_scan<u32, T>(c, scan_lds, &tot);
    if (tid < ND) { s_pre[tid] = ex; s_v[tid] = v; s_pg0[tid] = c ? pt.ptab[(u64)tid * pt.pstride + (v >> pt.lgpg)] - 1u : 0u; }
    if (tid == 0) s_pre[ND] = tot;
    const u32 wv = tid / IVX_WAVE, ln = lane_id();
    const u32 per = (tot + T / IVX_WAVE - 1) / (T / IVX_WAVE);
    const u32 j_lo = wv * per, j_hi = j_lo + per < tot ? j_lo + per : tot;
    // one output: src = its records, dst = the caller's column (null: not wanted; the same for every thread)
    auto pass = [&](auto *src, auto *dst, u64 none) {
        using E = std::remove_pointer_t<decltype(dst)>;
        if (dst == nullptr) return;
        for (u32 t = tid; t < TILE; t += T) s_val[t] = none;
        __syncthreads();                                        // (the first pass: s_pre / s_v / s_pg0 are complete behind it, too)
        u32 r = 0;
        if (j_lo < j_hi) { u32 a = 0, b = ND; while (a < b) { const u32 m = (a + b + 1) >> 1; if (m < ND && s_pre[m] <= j_lo + ln) a = m; else b = m - 1; } r = a; }
        for (u32 j = j_lo + ln; j < j_hi; j += IVX_WAVE) {
            while (r + 1 < ND && s_pre[r + 1] <= j) r++;
            const u32 x = s_v[r] + (j - s_pre[r]);                  // virtual row number in region r
            u32 pg = s_pg0[r];
            if ((x >> pt.lgpg) != (s_v[r] >> pt.lgpg)) pg = pt.ptab[(u64)r * pt.pstride + (x >> pt.lgpg)] - 1u;   // the run's second page
            const u64 at = ((u64)pg << pt.lgpg) + (x & pmask);
            const u32 slot = ((u32)(pool[at] >> 32) & rowmask) - (u32)t0;
            if (slot < (u32)TILE) s_val[slot] = (u64)src[at];
        }
        __syncthreads();
        for (u32 t = tid; t < len; t += T) dst[t0 + t] = (E)s_val[t];
        __syncthreads();
    };
    io.each(pass);
}

// two values per row back into input order: the un-permute above for (u32, i64) pairs with one-tile chunks; rows that
// were never routed get (IVX_NULL_IDX, dflt); op = the row's own index; vb / ob / op may be null (one i64 value per row)
__global__ __launch_bounds__(PA_T) void k_unpermute_pair(const u32 *__restrict__ vb, const i64 *__restrict__ vd, const unsigned short *__restrict__ cidx,
                                                         const u32 *__restrict__ offs, u32 nblk, u64 n, u32 *__restrict__ ob, u32 *__restrict__ op,
                                                         i64 *__restrict__ od, const u32 *unsorted, i64 dflt)
{
    constexpr int ND = 1024;
    __shared__ u32 s_b[PA_TILE];
    __shared__ i64 s_d[PA_TILE];
    __shared__ u32 s_pre[ND + 1], s_g[ND];
    __shared__ u32 scan_lds[PA_T / IVX_WAVE + 1];
    if (*unsorted == 0) return;                             // the probe wrote the outputs in place
    const u32 tid = threadIdx.x, blk = blockIdx.x;
    const u64 lo = (u64)blk * PA_TILE;
    const u32 len = (u32)(lo + PA_TILE < n ? PA_TILE : n - lo);
    const u32 g = offs[(u64)tid * nblk + blk];
    const u32 c = offs[(u64)tid * nblk + blk + 1] - g;
    u32 tot;
    const u32 ex = block_excl_scan<u32, PA_T>(c, scan_lds, &tot);
    s_pre[tid] = ex; s_g[tid] = g;
    if (tid == 0) s_pre[ND] = tot;
    for (u32 t = tid; t < PA_TILE; t += PA_T) { s_b[t] = IVX_NULL_IDX; s_d[t] = dflt; }
    __syncthreads();
    const u32 wv = tid / IVX_WAVE, ln = lane_id();
    const u32 per = (tot + PA_T / IVX_WAVE - 1) / (PA_T / IVX_WAVE);
    const u32 t_lo = wv * per, t_hi = t_lo + per < tot ? t_lo + per : tot;
    u32 r = 0;
    if (t_lo < t_hi) { u32 a = 0, b = ND; while (a < b) { const u32 m = (a + b + 1) >> 1; if (s_pre[m] <= t_lo + ln && m < ND) a = m; else b = m - 1; } r = a; }
    for (u32 t = t_lo + ln; t < t_hi; t += IVX_WAVE) {
        while (r + 1 < ND && s_pre[r + 1] <= t) r++;
        const u64 at = (u64)s_g[r] + (t - s_pre[r]);
        const u32 ci = cidx[at];
        if (vb) s_b[ci] = vb[at];
        if (vd) s_d[ci] = vd[at];
    }
    __syncthreads();
    for (u32 t = tid; t < len; t += PA_T) {
        if (ob) ob[lo + t] = s_b[t];
        if (op) op[lo + t] = (u32)(lo + t);
        if (od) od[lo + t] = vd ? s_d[t] : dflt;
    }
}

constexpr int WR_T = 256;

// ------------------------------------------------------------------ second routing pass (more than IVX_MAXREG_WIDE regions)
// Pass A (k_part_* with SPLIT) grouped the probe rows by super-region = region / G and kept region % G ("sub") per
// row.  Pass B orders the rows of every super-region by sub.  Super-region s is cut into tiles of PA_TILE rows;
// the histogram is laid out as [s][sub][tile of s] -- exactly the output order, so ONE plain exclusive scan over it
// gives every (tile, sub) run its place, and (s, sub, tile 0) is where region s*G + sub starts.
constexpr u32 P2_SUBMAX = 64;                           // G <= 64: up to 1023 * 64 = 65 472 >= IVX_MAXREG2 regions

// tprefix[s] = tiles of the super-regions before s (one workgroup; nsuper <= 1023)
__global__ __launch_bounds__(1024) void k_p2_layout(const u32 *__restrict__ offs1, u32 nblk1, u32 nsuper, u32 *tprefix, const u32 *unsorted)
{
    __shared__ u32 red[1024 / IVX_WAVE + 1];
    if (*unsorted == 0) return;
    const u32 t = threadIdx.x;
    const u32 rows = t < nsuper ? offs1[(u64)(t + 1) * nblk1] - offs1[(u64)t * nblk1] : 0u;
    const u32 tiles = (rows + PA_TILE - 1) / PA_TILE;
    u32 tot;
    const u32 ex = block_excl_scan<u32, 1024>(tiles, red, &tot);
    if (t < nsuper) tprefix[t] = ex;
    if (t == 0) tprefix[nsuper] = tot;
}

struct P2Tile { u32 s, t, nt; u64 lo, hi; bool ok; };
__device__ __forceinline__ P2Tile p2_tile(const u32 *__restrict__ offs1, u32 nblk1, u32 nsuper, const u32 *__restrict__ tprefix, u32 *s_tp)
{
    for (u32 i = threadIdx.x; i <= nsuper; i += blockDim.x) s_tp[i] = tprefix[i];
    __syncthreads();
    P2Tile T; T.ok = blockIdx.x < s_tp[nsuper];
    if (!T.ok) return T;
    u32 a = 0, b = nsuper - 1;                                      // last s with tprefix[s] <= block
    while (a < b) { const u32 m = (a + b + 1) >> 1; if (s_tp[m] <= blockIdx.x) a = m; else b = m - 1; }
    T.s = a; T.t = blockIdx.x - s_tp[a]; T.nt = s_tp[a + 1] - s_tp[a];
    const u64 seg_lo = offs1[(u64)a * nblk1], seg_hi = offs1[(u64)(a + 1) * nblk1];
    T.lo = seg_lo + (u64)T.t * PA_TILE;
    T.hi = T.lo + PA_TILE < seg_hi ? T.lo + PA_TILE : seg_hi;
    return T;
}

__global__ __launch_bounds__(PA_T) void k_p2_hist(const unsigned char *__restrict__ sub1, const u32 *__restrict__ offs1, u32 nblk1, u32 nsuper,
                                                  const u32 *__restrict__ tprefix, u32 G, u32 *__restrict__ hist2, const u32 *unsorted)
{
    __shared__ u32 s_tp[IVX_MAXREG_WIDE + 2];
    __shared__ u32 cnt[P2_SUBMAX];
    if (*unsorted == 0) return;
    if (threadIdx.x < P2_SUBMAX) cnt[threadIdx.x] = 0;
    const P2Tile T = p2_tile(offs1, nblk1, nsuper, tprefix, s_tp);  // (barrier inside)
    if (!T.ok) return;
    for (u64 i0 = T.lo; i0 < T.hi; i0 += PA_T) {
        const u64 i = i0 + threadIdx.x;
        const bool ok = i < T.hi;
        lds_count_up(cnt, ok ? (u32)sub1[i] : 0u, ok);
    }
    __syncthreads();
    if (threadIdx.x < G) hist2[(u64)G * s_tp[T.s] + (u64)threadIdx.x * T.nt + T.t] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(PA_T) void k_p2_scatter(const unsigned char *__restrict__ sub1, const u64 *__restrict__ se1, const u32 *__restrict__ row1,
                                                     const u32 *__restrict__ offs1, u32 nblk1, u32 nsuper, const u32 *__restrict__ tprefix, u32 G,
                                                     const u32 *__restrict__ hist2, u64 *__restrict__ se2, u32 *__restrict__ row2, const u32 *unsorted)
{
    __shared__ u32 s_tp[IVX_MAXREG_WIDE + 2];
    __shared__ u32 cur[P2_SUBMAX];
    if (*unsorted == 0) return;
    const P2Tile T = p2_tile(offs1, nblk1, nsuper, tprefix, s_tp);
    if (!T.ok) return;
    if (threadIdx.x < G) cur[threadIdx.x] = hist2[(u64)G * s_tp[T.s] + (u64)threadIdx.x * T.nt + T.t];   // this tile's run of every sub
    __syncthreads();
    for (u64 i0 = T.lo; i0 < T.hi; i0 += PA_T) {
        const u64 i = i0 + threadIdx.x;
        const bool ok = i < T.hi;
        const u32 d = ok ? (u32)sub1[i] : 0u;
        const u32 pos = lds_count_up(cur, d, ok);                   // order inside a run is arbitrary
        if (ok) { se2[pos] = se1[i]; row2[pos] = row1[i]; }
    }
}

// rfirst[r] = first routed position of region r (r = 0 .. nreg), from the scanned second-pass histogram
__global__ __launch_bounds__(WR_T) void k_p2_bounds(u32 nreg, u32 G, u32 nsuper, const u32 *__restrict__ offs1, u32 nblk1, u64 nh1,
                                                    const u32 *__restrict__ tprefix, const u32 *__restrict__ hist2, u32 *__restrict__ rfirst,
                                                    const u32 *unsorted)
{
    if (*unsorted == 0) return;
    const u32 r = blockIdx.x * WR_T + threadIdx.x;
    if (r > nreg) return;
    if (r == nreg) { rfirst[r] = offs1[nh1 - 1]; return; }          // all routed rows
    const u32 sp = r / G, sub = r - sp * G;
    const u32 nt = tprefix[sp + 1] - tprefix[sp];
    rfirst[r] = nt ? hist2[(u64)G * tprefix[sp] + (u64)sub * nt] : offs1[(u64)sp * nblk1];
}

// the same table when the probe rows came in region order already (nothing was moved): binary searches in the input
__global__ __launch_bounds__(WR_T) void k_sorted_bounds(JoinIndexView ix, const u32 *__restrict__ pkey, const i32 *__restrict__ ps, u64 n,
                                                        u32 nreg, u32 *__restrict__ rfirst, const u32 *unsorted)
{
    __shared__ i32 s_origin[KT_MAX];
    __shared__ u32 s_last[KT_MAX], s_kreg[KT_MAX];
    if (*unsorted != 0) return;
    KeyTab kt;
    keytab_load(ix, s_origin, s_last, s_kreg, kt);
    __syncthreads();
    const u32 r = blockIdx.x * WR_T + threadIdx.x;
    if (r > nreg) return;
    u64 lo = 0, hi = n;                                             // first row whose region is >= r (every row is routable here)
    auto body = [&](auto klds_tag) {
        constexpr bool KLDS = decltype(klds_tag)::value;
        while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (region_of<KLDS>(ix, kt, s_origin, s_last, s_kreg, pkey ? pkey[mid] : 0u, ps[mid]) < r) lo = mid + 1; else hi = mid; }
    };
    KEYTAB_DISPATCH(kt, body);
    rfirst[r] = (u32)lo;
}

}  // namespace

// ------------------------------------------------------------------ the three ways to route
static inline bool cols_aligned16(const u32 *key, const i32 *s, const i32 *e) { return (((uintptr_t)key | (uintptr_t)s | (uintptr_t)e) & 15) == 0; }
static constexpr u64 IN_COLS = (1ull << WS_IN_START) | (1ull << WS_IN_END);   // where staged start / end columns sit: R->ds / de

ivx_status ivx_route_flat(ivx_ctx *ctx, const JoinIndexView &jv, const u32 *key, const i32 *s, const i32 *e, u64 n, u32 adj,
                          u32 ndig, bool ids16, u32 max_tiles, ivx_routed *R)
{
    hipStream_t st = ctx->stream;
    const u32 chunk = part_chunk(n, max_tiles);
    const u32 nblk = (u32)((n + chunk - 1) / chunk);
    const u64 nh = (u64)ndig * nblk + 1;
    u32 *hist; u64 *pse; void *ids;
    IVX_TRY(ctx->get_scratch(WS_SORTHIST, nh * sizeof(u32), (void **)&hist));
    IVX_TRY(ctx->get_scratch(WS_T0, n * sizeof(u64), (void **)&pse));
    IVX_TRY(ctx->get_scratch(WS_T1, n * (ids16 ? sizeof(unsigned short) : sizeof(u32)), &ids));
    u32 *unsorted = ctx->dword<u32>(SC_UNSORTED);                      // stays 0 if the rows already come in region order
    IVX_HIP(ctx, hipMemsetAsync(hist + (nh - 1), 0, sizeof(u32), st));
    IVX_HIP(ctx, hipMemsetAsync(unsorted, 0, sizeof(u32), st));
    ivx_status scan = IVX_OK;
    with_bools([&](auto vec, auto wide, auto i16) {
        constexpr int ND = IVX_B(wide) ? 1024 : 256;
        using RowT = typename std::conditional<IVX_B(i16), unsigned short, u32>::type;
        hipLaunchKernelGGL((k_part_hist<IVX_B(vec), ND>), dim3(nblk), dim3(PA_T), 0, st, jv, key, s, n, nblk, chunk, hist, adj, unsorted);
        if ((scan = ivx_scan_exclusive_u32(ctx, hist, nh)) != IVX_OK) return;
        hipLaunchKernelGGL((k_part_scatter<IVX_B(vec), RowT, ND>), dim3(nblk), dim3(PA_T), 0, st, jv, key, s, e, n, nblk, (const u32 *)hist, pse, (RowT *)ids, chunk, adj, (const u32 *)unsorted);
    }, cols_aligned16(key, s, e), ndig > 256, ids16);
    IVX_TRY(scan);
    IVX_HIP(ctx, hipGetLastError());
    *R = ivx_routed{};
    R->form = IVX_ROWS_FLAT; R->se = pse; R->rfirst = hist; R->nblk = nblk; R->chunk = chunk; R->ndig = ndig; R->unsorted = unsorted;
    if (ids16) R->cidx = (const unsigned short *)ids; else R->ids = (const u32 *)ids;
    R->ds = s; R->de = e; R->adj = adj;
    R->slots = (1ull << WS_SORTHIST) | (1ull << WS_T0) | (1ull << WS_T1) | IN_COLS;
    return IVX_OK;
}

ivx_status ivx_route_paged(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, const u32 *key, const i32 *s, const i32 *e, u64 n,
                           const ivx_paged_opts &o, ivx_routed *R)
{
    hipStream_t st = ctx->stream;
    const bool wide = nreg > IVX_MAXREG;
    const bool half = o.packed && !wide;                                // two 512-thread workgroups per CU, 8192-row tiles
    // 16384-row tiles in one 1024-thread workgroup per CU for the join's packed, unfiltered form (fill, count, marks): runs
    // twice as long, and a tile's cost per region (the rcur atomic, the page look-up) shared by twice the rows.
    // Only the instantiation that loads ahead without scratch (aligned columns, key tables in LDS, no bitmap), and never
    // with a vtab: the un-permute indexes it by 8192-row tiles.  From PART_BIG_ROWS rows on.
    // (tests: IVX_PART_BIG=1 takes it whatever n is and IVX_PART_BIG=0 never, where the other conditions hold)
    const bool big_ok = half && !o.filter && !(o.rowval && !o.no_vtab) && cols_aligned16(key, s, e) && jv.nkeys <= KT_MAX;
    bool big = big_ok && n >= PART_BIG_ROWS;
    if (const char *benv = getenv("IVX_PART_BIG"))
        if ((benv[0] == '0' || benv[0] == '1') && benv[1] == 0) big = big_ok && benv[0] == '1';
    const u32 tile = wide ? PA_T * 8u : big ? PA_T * 16u : half ? 512u * 16u : PA_T * 12u;
    u32 rowbits = 1;
    while (rowbits < 32 && (n - 1) >> rowbits) rowbits++;              // bits of the largest row id (the rest of the word's upper half extends the length)
    if (o.filter) rowbits = 32;                                         // (see pk_maxlen)
    u32 lgpg = 14;                                                      // a page holds at least a tile; at most ~4096 pages per region
    while (lgpg < 31 && (n >> lgpg) > 4096) lgpg++;
    const u64 pstride = (n >> lgpg) + 2;
    const u64 npages = (n >> lgpg) + nreg + 1;
    const u64 ntiles = (n + tile - 1) / tile;
    ivx_route_ctl *ctl; u32 *ptab; u64 *pool; u32 *prow = nullptr; uint2 *vtab = nullptr; void *rest = nullptr;
    *R = ivx_routed{};
    R->slots = (1ull << WS_SORTHIST) | (1ull << WS_T0) | (1ull << WS_T1) | (1ull << WS_T2) | IN_COLS;
    IVX_TRY(ctx->get_scratch(WS_SORTHIST, sizeof(ivx_route_ctl), (void **)&ctl));
    IVX_TRY(ctx->get_scratch(WS_T2, (size_t)nreg * pstride * sizeof(u32), (void **)&ptab));
    IVX_TRY(ctx->get_scratch(WS_T0, (size_t)(npages << lgpg) * sizeof(u64), (void **)&pool));
    // WS_T1: the row ids of unpacked rows, or the un-permute's table, or the lean fill's rest lists (batches, then rows); the
    // lean per-row-value kernel lists single rows only, in WS_T3
    if (o.rowval) { if (!o.no_vtab) IVX_TRY(ctx->get_scratch(WS_T1, (size_t)ntiles * 256 * sizeof(uint2), (void **)&vtab)); }
    else if (!o.packed) IVX_TRY(ctx->get_scratch(WS_T1, (size_t)(npages << lgpg) * sizeof(u32), (void **)&prow));
    else if (o.lean) IVX_TRY(ctx->get_scratch(WS_T1, (size_t)fp_max_batches(n, nreg) * sizeof(FpRest) + (size_t)(n + 64) * sizeof(u64), &rest));
    if (rest) { R->rest = (FpRest *)rest; R->rest_rows = (u64 *)(R->rest + fp_max_batches(n, nreg)); }
    if (o.rowval && o.lean) { IVX_TRY(ctx->get_scratch(WS_T3, (size_t)(n + 64) * sizeof(u64), (void **)&R->rest_rows)); R->slots |= 1ull << WS_T3; }
    {
        const u32 nctl = (u32)(offsetof(ivx_route_ctl, rfirst) / sizeof(u32));
        const u64 nptab = (u64)nreg * pstride;
        u64 cg = (nptab / 4 + 256 * 8 - 1) / (256 * 8);                 // eight 16-byte stores a thread
        cg = cg < (nctl + 255) / 256 ? (nctl + 255) / 256 : (cg > 1024 ? 1024 : cg);
        hipLaunchKernelGGL(k_route_clear, dim3((u32)cg), dim3(256), 0, st, (u32 *)ctl, nctl, ptab, nptab, o.zero2);
    }
    const PageTab pt{ptab, (u32)pstride, lgpg};
    // tiles per workgroup: every tile but a workgroup's first finds its first rows loaded ahead (k_part_onepass)
    // (tests: IVX_PART_TILES=t, t in 1, 2, 4, 8, makes it t tiles whatever n is, so that a small batch walks several tiles per
    //  workgroup)
    u32 tiles = big ? PART_BIG_TILES : n >= (16u << 20) ? 4u : n >= (4u << 20) ? 2u : 1u;
    if (const char *tenv = getenv("IVX_PART_TILES"))
        if ((tenv[0] == '1' || tenv[0] == '2' || tenv[0] == '4' || tenv[0] == '8') && tenv[1] == 0) tiles = (u32)(tenv[0] - '0');
    const u32 chunk1 = tile * tiles;
    const u32 nblk1 = (u32)((n + chunk1 - 1) / chunk1);
    with_bools([&](auto vec, auto klds, auto filt, auto pk) {
        auto part = [&](auto kern, u32 threads) {
            hipLaunchKernelGGL(kern, dim3(nblk1), dim3(threads), 0, st, jv, key, s, e, n, chunk1, ctl->rcur, pt, &ctl->pool_next, pool, prow, rowbits, o.adj, vtab);
        };
        if (big) part(k_part_onepass<true, 256, 16, true, false, true, PA_T>, (u32)PA_T);
        else if (half) part(k_part_onepass<IVX_B(vec), 256, 16, IVX_B(klds), IVX_B(filt), true, 512>, 512u);
        else if (wide) part(k_part_onepass<IVX_B(vec), 1024, 8, IVX_B(klds), IVX_B(filt), IVX_B(pk)>, (u32)PA_T);
        else part(k_part_onepass<IVX_B(vec), 256, 12, IVX_B(klds), IVX_B(filt), IVX_B(pk)>, (u32)PA_T);
    }, cols_aligned16(key, s, e), jv.nkeys <= KT_MAX, o.filter, o.packed);
    // (per-row-value consumers that do not run the lean kernel need no chunk table; defer_bounds: the caller queues
    //  ivx_route_paged_bounds itself if its probe turns out to read the tables)
    if (o.rowval && !o.lean) hipLaunchKernelGGL(k_page_bounds, dim3(1), dim3(1024), 0, st, (const u32 *)ctl->rcur, nreg, ctl->rfirst);
    else if (!o.defer_bounds) hipLaunchKernelGGL(k_chunk_bounds, dim3(1), dim3(1024), 0, st, (const u32 *)ctl->rcur, nreg, ctl->rfirst, ctl->cfirst);
    IVX_HIP(ctx, hipGetLastError());
    R->form = IVX_ROWS_PAGED; R->se = pool; R->ids = prow; R->rfirst = ctl->rfirst; R->pt = pt; R->packed = o.packed; R->rowbits = rowbits;
    R->tables_due = o.defer_bounds && !(o.rowval && !o.lean);
    R->all_routed = !o.filter; R->ctl = ctl; R->vtab = vtab; R->ds = s; R->de = e; R->adj = o.adj;
    return IVX_OK;
}

ivx_status ivx_route_paged_bounds(ivx_ctx *ctx, const ivx_routed &R, u32 nreg)
{
    hipLaunchKernelGGL(k_chunk_bounds, dim3(1), dim3(1024), 0, ctx->stream, (const u32 *)R.ctl->rcur, nreg, R.ctl->rfirst, R.ctl->cfirst);
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}

ivx_status ivx_route_two_level(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, const u32 *key, const i32 *s, const i32 *e, u64 n, ivx_routed *R)
{
    hipStream_t st = ctx->stream;
    u32 *unsorted = ctx->dword<u32>(SC_UNSORTED);
    const u32 G = (nreg + IVX_MAXREG_WIDE - 1) / IVX_MAXREG_WIDE;       // regions per super-region
    if (G > P2_SUBMAX) return ctx->fail(IVX_ERR_INVALID, "overlap index with too many probe regions");
    const u32 nsuper = (nreg + G - 1) / G;
    const uint2 split = make_uint2(G, (u32)(((1ull << 32) + G - 1) / G));
    const u32 chunk = part_chunk(n);
    const u32 nblk1 = (u32)((n + chunk - 1) / chunk);
    const u64 nh1 = (u64)1024 * nblk1 + 1;
    const u32 grid2 = (u32)(n / PA_TILE) + nsuper + 1;                   // tiles of the second pass, at most
    const u64 nh2 = (u64)G * grid2 + 1;
    u32 *hist1, *hist2, *tprefix, *prow1, *rfirst, *prow2; u64 *pse1, *pse2; unsigned char *sub1;
    IVX_TRY(ctx->get_scratch(WS_SORTHIST, nh1 * sizeof(u32), (void **)&hist1));
    IVX_TRY(ctx->get_scratch(WS_T0, n * sizeof(u64), (void **)&pse1));
    IVX_TRY(ctx->get_scratch(WS_T1, n * sizeof(u32), (void **)&prow1));
    IVX_TRY(ctx->get_scratch(WS_T2, n, (void **)&sub1));
    IVX_TRY(ctx->get_scratch(WS_SA0, n * sizeof(u64), (void **)&pse2));
    IVX_TRY(ctx->get_scratch(WS_SA1, n * sizeof(u32), (void **)&prow2));
    IVX_TRY(ctx->get_scratch(WS_T4, ((size_t)nsuper + 1) * sizeof(u32), (void **)&tprefix));
    IVX_TRY(ctx->get_scratch(WS_T5, nh2 * sizeof(u32), (void **)&hist2));
    IVX_TRY(ctx->get_scratch(WS_T6, ((size_t)nreg + 1) * sizeof(u32), (void **)&rfirst));
    IVX_HIP(ctx, hipMemsetAsync(hist1 + (nh1 - 1), 0, sizeof(u32), st));
    IVX_HIP(ctx, hipMemsetAsync(hist2, 0, nh2 * sizeof(u32), st));
    IVX_HIP(ctx, hipMemsetAsync(unsorted, 0, sizeof(u32), st));
    // pass A: by super-region (and the sortedness check on the regions themselves)
    ivx_status scan = IVX_OK;
    with_bools([&](auto vec) {
        hipLaunchKernelGGL((k_part_hist<IVX_B(vec), 1024, true>), dim3(nblk1), dim3(PA_T), 0, st, jv, key, s, n, nblk1, chunk, hist1, 0u, unsorted, split);
        if ((scan = ivx_scan_exclusive_u32(ctx, hist1, nh1)) != IVX_OK) return;
        hipLaunchKernelGGL((k_part_scatter<IVX_B(vec), u32, 1024, true>), dim3(nblk1), dim3(PA_T), 0, st, jv, key, s, e, n, nblk1, (const u32 *)hist1, pse1, prow1, chunk, 0u, (const u32 *)unsorted, split, sub1);
    }, cols_aligned16(key, s, e));
    IVX_TRY(scan);
    // pass B: inside every super-region by region
    hipLaunchKernelGGL(k_p2_layout, dim3(1), dim3(1024), 0, st, (const u32 *)hist1, nblk1, nsuper, tprefix, (const u32 *)unsorted);
    hipLaunchKernelGGL(k_p2_hist, dim3(grid2), dim3(PA_T), 0, st, (const unsigned char *)sub1, (const u32 *)hist1, nblk1, nsuper, (const u32 *)tprefix, G, hist2, (const u32 *)unsorted);
    IVX_TRY(ivx_scan_exclusive_u32(ctx, hist2, nh2));
    hipLaunchKernelGGL(k_p2_scatter, dim3(grid2), dim3(PA_T), 0, st, (const unsigned char *)sub1, (const u64 *)pse1, (const u32 *)prow1, (const u32 *)hist1, nblk1, nsuper,
                       (const u32 *)tprefix, G, (const u32 *)hist2, pse2, prow2, (const u32 *)unsorted);
    const u32 bgrid = (nreg + 1 + WR_T - 1) / WR_T;
    hipLaunchKernelGGL(k_p2_bounds, dim3(bgrid), dim3(WR_T), 0, st, nreg, G, nsuper, (const u32 *)hist1, nblk1, nh1, (const u32 *)tprefix, (const u32 *)hist2, rfirst, (const u32 *)unsorted);
    hipLaunchKernelGGL(k_sorted_bounds, dim3(bgrid), dim3(WR_T), 0, st, jv, key, s, n, nreg, rfirst, (const u32 *)unsorted);
    IVX_HIP(ctx, hipGetLastError());
    *R = ivx_routed{};
    R->form = IVX_ROWS_TABLE; R->se = pse2; R->ids = prow2; R->rfirst = rfirst; R->unsorted = unsorted; R->ds = s; R->de = e;
    R->slots = IN_COLS;
    for (int slot : {WS_SORTHIST, WS_T0, WS_T1, WS_T2, WS_SA0, WS_SA1, WS_T4, WS_T5, WS_T6}) R->slots |= 1ull << slot;
    return IVX_OK;
}

// ------------------------------------------------------------------ values back into input order (host side)
ivx_status ivx_unroute_values(ivx_ctx *ctx, const ivx_routed &R, u32 nreg, int kind, const u32 *val, u64 n, void *out, u64 *d_total, int sorted_done)
{
    hipStream_t st = ctx->stream;
    auto go = [&](auto out_tag) {
        constexpr int O = decltype(out_tag)::value;
        if (R.form == IVX_ROWS_PAGED) {
            constexpr u32 TILE = 512u * 16u;                            // the one-pass partition's tile for packed rows
            hipLaunchKernelGGL((k_unpermute_paged<O, (int)TILE>), dim3((u32)((n + TILE - 1) / TILE)), dim3(512), 0, st, R.se, R.vtab, R.pt, nreg, R.rowbits, n, out, (unsigned long long *)d_total);
        } else with_bools([&](auto wide) {
            constexpr int ND = IVX_B(wide) ? 1024 : 256;
            hipLaunchKernelGGL((k_unpermute<O, ND>), dim3(R.nblk), dim3(PA_T), 0, st, val, R.cidx, R.rfirst, R.nblk, R.chunk, (u32)ND, n, out, R.unsorted, (unsigned long long *)d_total, sorted_done);
        }, R.ndig > 256);
    };
    switch (kind) {
    case IVX_RV_COVERAGE: go(std::integral_constant<int, UP_I64S>{}); break;
    case IVX_RV_COUNT: go(std::integral_constant<int, UP_I64>{}); break;
    case IVX_RV_PER_ROW: go(std::integral_constant<int, UP_U32>{}); break;
    default: go(std::integral_constant<int, UP_U8>{}); break;
    }
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}

// ------------------------------------------------------------------ routing for operators with their own probe (nearest, rank grids)
ivx_status ivx_route_rows(ivx_ctx *ctx, const JoinIndexView &rv, const u32 *key, const i32 *s, const i32 *e, u64 n, u32 adj, ivx_routed *out)
{
    return ivx_route_flat(ctx, rv, key, s, e, n, adj, 1024, true, 1, out);
}

// one u32 value per routed row back into input order, as u32 (out32) or as "value != 0" bytes (out8); rows that were
// never routed get 0.  (Rows that came in region order: another kernel answered them in place.)
ivx_status ivx_unroute_u32(ivx_ctx *ctx, const ivx_routed &r, u64 n, const u32 *vb, u32 *out32, u8 *out8)
{
    if (out32) IVX_TRY(ivx_unroute_values(ctx, r, 1024u, IVX_RV_PER_ROW, vb, n, out32, nullptr, 1));
    if (out8) IVX_TRY(ivx_unroute_values(ctx, r, 1024u, IVX_RV_EXISTS, vb, n, out8, nullptr, 1));
    return IVX_OK;
}

ivx_status ivx_unroute_pair(ivx_ctx *ctx, const ivx_routed &r, u64 n, const u32 *vb, const i64 *vd, u32 *ob, u32 *op, i64 *od, i64 dflt)
{
    hipLaunchKernelGGL(k_unpermute_pair, dim3(r.nblk), dim3(PA_T), 0, ctx->stream, vb, vd, r.cidx, r.rfirst, r.nblk, n, ob, op, od, r.unsorted, dflt);
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}

template <class RECS>
static ivx_status unroute_records(ivx_ctx *ctx, const ivx_routed &R, u32 nreg, u64 n, const RECS &io)
{
    if (R.form != IVX_ROWS_PAGED || R.vtab == nullptr || nreg > IVX_MAXREG) return ctx->fail(IVX_ERR_INVALID, "internal error: records are un-permuted from region pages with a tile table");
    constexpr u32 TILE = 512u * 16u;                                    // the one-pass partition's tile for packed rows
    hipLaunchKernelGGL((k_unpermute_records<(int)TILE, RECS>), dim3((u32)((n + TILE - 1) / TILE)), dim3(512), 0, ctx->stream, R.se, R.vtab, R.pt, nreg, R.rowbits, n, io);
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}

ivx_status ivx_unroute_records(ivx_ctx *ctx, const ivx_routed &R, u32 nreg, u64 n, const AggOut &rec, const AggOut &out)
{
    return unroute_records(ctx, R, nreg, n, AggRecs{rec, out});
}

ivx_status ivx_unroute_sel_records(ivx_ctx *ctx, const ivx_routed &R, u32 nreg, u64 n, const SelOut &rec, const SelOut &out)
{
    return unroute_records(ctx, R, nreg, n, SelRecs{rec, out});
}
