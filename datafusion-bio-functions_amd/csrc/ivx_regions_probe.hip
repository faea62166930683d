// ivx_regions_probe.hip -- the overlap probe without random HBM gathers: routed probe rows (ivx_regions_route.hip, described
// by an ivx_routed) are probed region by region against the region's slice of the index -- cell offsets and (start,end) of
// its entries -- staged in LDS, with coalesced reads of the rows.
//
//   k_probe_regions   every row form (flat runs, region pages, packed rows, input left in place); count, fill and the
//                     per-row values.  Fill: matches are compacted into per-wavefront LDS staging rings and written with
//                     ONE global atomicAdd per workgroup and round (~3000 pairs); no LDS or global atomics per pair.
//                     Rows longer than the slice halo, regions whose slice exceeds LDS and the long-interval levels
//                     fall back to global reads inside the same kernel.
//   k_fill_fast/_rest the lean fill for the case the headline always meets: packed rows in pages, every region one
//                     LDS-resident level
//   k_lean/_rest      the same for the per-row operators (ivx_rowops.hpp): per-row values, build-side match marks, overlap
//                     aggregates, overlap select -- one kernel pair, instantiated per operator
//   k_probe_dense     match-dense fill: count the 64-row pieces, scan, write
//   k_pick_rows       rows per lane of the fill, decided on the device when the routed row count is known only there
//
// Host side: region_knobs (the IVX_* environment settings, read once per call), probe_pairs (count / fill over any
// ivx_routed), and the entry points ivx_join_probe_regions (COUNT / FILL; a COUNT call leaves its routed rows to the
// FILL call that follows: ivx_join_plan), ivx_rowval_probe_regions (one value per probe row, in input order) and
// ivx_mark_probe_regions (one bit per matched BUILD row, ORed into the caller's bitmap; lean form only),
// ivx_agg_probe_regions (per probe row, aggregates of a build-side value column; lean form only) and
// ivx_sel_probe_regions (per probe row, the best matching build row by a criterion; lean form only).
//
// HBM traffic per probe row behind the routing: 12 B or 8 B (probe) + 8 B per pair, all streaming (measured:
// profiles/r1_d_regions_pipeline_pmc.txt).
#include "ivx_regions.hpp"
#include "ivx_agg.hpp"
#include "ivx_select.hpp"
#include "ivx_where.hpp"

namespace {

// ------------------------------------------------------------------ region probe

#ifndef IVX_RP_B
#define IVX_RP_B 8
#endif
#ifndef IVX_RP_RING
#define IVX_RP_RING 512
#endif
constexpr int RP_B = IVX_RP_B;             // probe rows per lane per wavefront batch (fill: 8, 4, 2 or 1 by match density)
constexpr u32 RP_HALO = IVX_RP_HALO;       // slice cells past the region's last cell
constexpr u32 RP_CCAP = 8192 + RP_HALO + 2;
constexpr u32 RP_RING = IVX_RP_RING;       // per-wavefront ring of staged pairs: two consecutive rounds must fit (power of two)
constexpr u32 RP_NSLOT = 4;                // rounds whose reservation state is kept (see round_publish)
constexpr u32 RP_NPG = 64;                 // page ids of one region segment kept in LDS (paged rows)
constexpr u32 RP_STASH = 48;               // lean fill: unfinished list tails a wavefront keeps per batch (what LDS is left over holds 48)
// a stashed tail in 32 bits: next slice slot j (13 bits: RP_ECAP <= 8192) | the row's slot in its wavefront batch, q * 64 + lane
// (9 bits).  Where the list ends is not kept: the tail pass fetches the row's word again and finds its last cell from that.
constexpr u32 FD_SLOT_SHIFT = 13;
#ifndef IVX_FD_HEAD
#define IVX_FD_HEAD 3
#endif
constexpr int FD_HEAD = IVX_FD_HEAD;       // steps a draining group that starts with more active lanes than it may drain takes before the next test
static_assert(RP_ECAP <= (1u << FD_SLOT_SHIFT), "a slice slot must fit a stash entry's j field");
constexpr u32 RP_GRID = 256;                // fill pass: one workgroup per CU (LDS-bound)
#ifndef IVX_RP_VGRID
#define IVX_RP_VGRID 512
#endif
constexpr u32 RP_VGRID = IVX_RP_VGRID;       // row shares ("virtual workgroups"); the count pass runs two per CU

struct Slice {
    const JoinIndexView *ix;
    const unsigned short *s_off; const u64 *s_ent; const u32 *s_row;
    u32 sh0, nlev, k, lb, slo, shi, e0, ncell0; bool inlds, upper, lev0;
    i32 origin; u32 span;
    i32 rbase;                  // coordinate of the region's first cell (packed rows hold their start relative to it)
    // packed rows (start relative to rbase, length) find their cells in 32-bit arithmetic when `fast`: the whole region is
    // one LDS-resident level.  off = cells between the slice's first cell and the region's (0 or 1), cmax = the key's last
    // cell and ncm1 = the slice's last cell, both relative to the slice
    bool fast; u32 off, cmax, ncm1;
};

// every match of one probe row: f(v, is_slot, start, end) -- v is a slot of the staged slice (build row =
// s_row[v]) when is_slot, else the build row itself (general path); start/end are the match's coordinates
template <class F>
__device__ __forceinline__ void probe_row(const Slice &S, i32 qs, i32 qe, F &&f)
{
    const JoinIndexView &ix = *S.ix;
    const i64 hi64 = (i64)qe - (i64)S.origin;
    if (hi64 < 0) return;
    if (S.lev0) {
        const u32 ncell = S.ncell0;
        const i64 lo64 = (i64)qs - ((i64)1 << S.sh0) + 1 - (i64)S.origin;
        const i64 bl = lo64 <= 0 ? 0 : (lo64 >> S.sh0);
        if (bl < (i64)ncell) {
            const u32 blo = (u32)bl;
            const i64 bh = hi64 >> S.sh0;
            const u32 bhi = bh >= (i64)ncell ? ncell - 1u : (u32)bh;
            if (blo <= bhi) {
                if (S.inlds && blo >= S.slo && bhi < S.shi) {
                    const u32 a = S.s_off[blo - S.slo], b = S.s_off[bhi + 1 - S.slo];
                    for (u32 j = a; j < b; j++) {
                        const u64 x = S.s_ent[j];
                        if ((i32)(u32)x <= qe && (i32)(u32)(x >> 32) >= qs) f(j, true, (i32)(u32)x, (i32)(u32)(x >> 32));
                    }
                } else {
                    const u32 a = ix.binstart[S.lb + blo], b = ix.binstart[S.lb + bhi + 1];
                    for (u32 j = a; j < b; j++) {
                        const ivx_ent x = ix.ent[j];
                        if (x.s <= qe && x.e >= qs) f(x.row, false, x.s, x.e);
                    }
                }
            }
        }
    }
    if (S.upper) {                                              // long-interval levels: global reads
        for (u32 l = 1; l < S.nlev; l++) {
            if (ix.hdr[HDR_LEVCNT + l] == 0) continue;
            const u32 sh = S.sh0 + IVX_LSTEP * l;
            u32 blo = 0, bhi = 0;
            if (sh < 32) {
                const u32 ncell = (S.span >> sh) + 1u;
                const i64 lo64 = (i64)qs - ((i64)1 << sh) + 1 - (i64)S.origin;
                const i64 bl = lo64 <= 0 ? 0 : (lo64 >> sh);
                const i64 bh = hi64 >> sh;
                if (bl >= (i64)ncell) continue;
                blo = (u32)bl;
                bhi = bh >= (i64)ncell ? ncell - 1u : (u32)bh;
                if (blo > bhi) continue;
            }
            const u32 base = ix.lbase[(u64)l * ix.nkeys + S.k];
            const u32 a = ix.binstart[base + blo], b = ix.binstart[base + bhi + 1];
            for (u32 j = a; j < b; j++) {
                const ivx_ent x = ix.ent[j];
                if (x.s <= qe && x.e >= qs) f(x.row, false, x.s, x.e);
            }
        }
    }
}

// The same for a packed row (rel = start - S.rbase < 2^24, len = end - start; ok = the row really is in that form): on a
// `fast` slice its cells follow from two shifts -- (start - origin) = (region's first cell) * cell + rel -- instead of
// the 64-bit coordinate arithmetic above (the walk is bound by the instructions it issues, and those were a fifth of them)
template <class F>
__device__ __forceinline__ void probe_row_rel(const Slice &S, u32 rel, u32 len, bool ok, i32 qs, i32 qe, F &&f)
{
    if (S.fast && ok) {
        const u32 t = ((rel + 1u) >> S.sh0) + S.off;                  // first cell a matching build row can start in: one cell back
        const u32 bl = t ? t - 1u : 0u;
        u32 bh = ((rel + len) >> S.sh0) + S.off;
        bh = bh < S.cmax ? bh : S.cmax;
        if (bh < S.ncm1) {
            if (bl <= bh) {
                const u32 a = S.s_off[bl], b = S.s_off[bh + 1u];
                for (u32 j = a; j < b; j++) {
                    const u64 x = S.s_ent[j];
                    if ((i32)(u32)x <= qe && (i32)(u32)(x >> 32) >= qs) f(j, true, (i32)(u32)x, (i32)(u32)(x >> 32));
                }
            }
            return;
        }
    }
    probe_row(S, qs, qe, f);
}

// ------------------------------------------------------------------ shared pieces of the probe kernels

struct ProbeLds {
    unsigned short *s_off; u64 *s_ent; u32 *s_row;
    // fill pass only
    u64 (*s_q)[RP_RING];                          // per-wavefront ring of staged (build row, probe row) pairs
    u32 *s_wpos;                                  // per-wavefront ring write position (running, never reset)
    u32 (*s_wcnt)[RP_W];                          // [RP_NSLOT] pairs each wavefront staged in a round
    unsigned long long *s_base;                   // [RP_NSLOT] output position reserved for the round
    u32 *s_arrive, *s_ready;                      // [RP_NSLOT] wavefronts arrived / round tag once s_base is valid
};

__device__ __forceinline__ void slice_init(const JoinIndexView &ix, Slice &S, const ProbeLds &L)
{
    S.ix = &ix; S.s_off = L.s_off; S.s_ent = L.s_ent; S.s_row = L.s_row;
    S.sh0 = ix.hdr[HDR_SH0]; S.nlev = ix.hdr[HDR_NLEV];
    S.upper = false;
    for (u32 l = 1; l < S.nlev; l++) S.upper |= ix.hdr[HDR_LEVCNT + l] != 0;
    S.lev0 = ix.hdr[HDR_LEVCNT] != 0;
}

// stage region r's slice of the index in LDS (all threads of the workgroup; barriers inside)
__device__ __forceinline__ void slice_load(const JoinIndexView &ix, Slice &S, const ProbeLds &L, u32 r, bool reload)
{
    const u32 tid = threadIdx.x;
    __syncthreads();
    const ivx_regdesc d = ix.rdesc[r];                                  // built by k_join_regdesc
    S.k = d.k; S.origin = d.origin; S.span = d.span; S.lb = d.lb;
    S.ncell0 = (S.span >> S.sh0) + 1u;
    S.slo = d.slo; S.shi = d.shi; S.e0 = d.e0; S.rbase = d.rbase;
    const u32 ne = d.ne;
    const u32 nc = S.shi - S.slo + 1u;
    S.inlds = ne <= RP_ECAP && nc <= RP_CCAP;
    S.fast = S.inlds && S.lev0 && !S.upper;
    S.off = (u32)(((i64)S.rbase - (i64)S.origin) >> S.sh0) - S.slo;
    S.cmax = S.ncell0 - 1u - S.slo; S.ncm1 = S.shi - S.slo;
    if (S.inlds && reload) {
        for (u32 c0 = 0; c0 < nc; c0 += RP_T * 4) {
            u32 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const u32 c = c0 + u * RP_T + tid; v[u] = c < nc ? ix.binstart[S.lb + S.slo + c] : 0u; }
#pragma unroll
            for (int u = 0; u < 4; u++) { const u32 c = c0 + u * RP_T + tid; if (c < nc) L.s_off[c] = (unsigned short)(v[u] - S.e0); }
        }
        for (u32 j0 = 0; j0 < ne; j0 += RP_T * 4) {
            ivx_ent x[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const u32 j = j0 + u * RP_T + tid; if (j < ne) x[u] = ix.ent[S.e0 + j]; }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const u32 j = j0 + u * RP_T + tid;
                if (j < ne) { L.s_ent[j] = (u64)(u32)x[u].s | ((u64)(u32)x[u].e << 32); L.s_row[j] = x[u].row; }
            }
        }
    }
    __syncthreads();
}

// One wave batch: B rows per lane (bit q of okmask says whether the lane holds a row in slot q).
// Count pass: returns the lane's pair count.
// Fill pass: every match takes the next slot of the wavefront's LDS staging buffer with an LDS atomic on
// the wavefront's own running counter (lanes of one instruction are serialised by the LDS unit and get
// distinct slots), so no per-row match stash, prefix sum or second walk is needed.  Returns the batch's
// pair count; direct = true if it did not fit the ring (see batch_write_direct).
// PK: rel / len hold the rows' packed form (valid where relmask has the row's bit)
template <bool FILL, int B, bool PK = false>
__device__ __forceinline__ u32 batch_walk(const Slice &S, const ProbeLds &L, const i32 (&qs)[B], const i32 (&qe)[B],
                                          const u32 (&rowv)[B], u32 okmask, u32 wv, u32 ring_tail, u32 &ring_start, bool &direct,
                                          const u32 (&rel)[B], const u32 (&len)[B], u32 relmask)
{
    auto walk = [&](int q, auto &&f) {
        if (PK) probe_row_rel(S, rel[q], len[q], (relmask >> q) & 1u, qs[q], qe[q], f);
        else probe_row(S, qs[q], qe[q], f);
    };
    if (!FILL) {
        u32 tsum = 0;
#pragma unroll
        for (int q = 0; q < B; q++) {
            if (!((okmask >> q) & 1u)) continue;
            walk(q, [&](u32, bool, i32, i32) { tsum++; });
        }
        return tsum;
    }
    u32 *cp = &L.s_wpos[wv];
    const u32 base = __hip_atomic_load(cp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    ring_start = base;
#pragma unroll
    for (int q = 0; q < B; q++) {
        if (!((okmask >> q) & 1u)) continue;
        walk(q, [&](u32 v, bool sl, i32, i32) {
            const u32 pos = __hip_atomic_fetch_add(cp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (pos - ring_tail < RP_RING)
                L.s_q[wv][pos & (RP_RING - 1)] = (u64)(sl ? S.s_row[v] : v) | ((u64)rowv[q] << 32);
        });
    }
    const u32 wtot = __hip_atomic_load(cp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) - base;
    // this round and the previous one must fit the ring together; if not, nothing of this batch counts as
    // staged (the previous round's pairs were never overwritten) and the caller writes the batch directly
    // once the round's output range is known (batch_write_direct)
    direct = base + wtot - ring_tail > RP_RING;
    if (direct) ring_start = base + wtot;
    return wtot;
}

// second walk of a batch that did not fit the staging ring: pairs go straight to their place in the
// output, [g, g + wtot) of the round's reserved range; slots again by LDS atomic
template <int B>
__device__ __forceinline__ void batch_write_direct(const Slice &S, const ProbeLds &L, const i32 (&qs)[B], const i32 (&qe)[B],
                                                   const u32 (&rowv)[B], u32 okmask, u32 wv, u64 g, bool ok, u32 *ob, u32 *op)
{
    u32 *cp = &L.s_wpos[wv];
    const u32 base = __hip_atomic_load(cp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
    for (int q = 0; q < B; q++) {
        if (!((okmask >> q) & 1u)) continue;
        probe_row(S, qs[q], qe[q], [&](u32 v, bool sl, i32, i32) {
            const u32 pos = __hip_atomic_fetch_add(cp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) - base;
            if (ok) { ob[g + pos] = sl ? S.s_row[v] : v; op[g + pos] = rowv[q]; }
        });
    }
}

// Per-row values (RV_*: ivx_rowops.hpp) on the same slices: the row's value instead of its pairs.
template <int KIND, int B, bool PK = false>
__device__ __forceinline__ void batch_rowval(const Slice &S, const i32 (&qs)[B], const i32 (&qe)[B], u32 okmask, u32 (&val)[B],
                                             const u32 (&rel)[B], const u32 (&len)[B], u32 relmask)
{
    auto walk = [&](int q, auto &&f) {
        if (PK) probe_row_rel(S, rel[q], len[q], (relmask >> q) & 1u, qs[q], qe[q], f);
        else probe_row(S, qs[q], qe[q], f);
    };
#pragma unroll
    for (int q = 0; q < B; q++) {
        u32 v = 0;
        if ((okmask >> q) & 1u) {
            if (KIND == RV_COUNT) {
                if (!(qe[q] < qs[q])) walk(q, [&](u32, bool, i32, i32) { v++; });
            } else if (KIND == RV_MATCHES) {
                walk(q, [&](u32, bool, i32, i32) { v++; });
            } else {
                const i32 a = rv_wadd(qe[q], 1), b = rv_wsub(qs[q], 1);
                walk(q, [&](u32, bool, i32 first, i32 last) {
                    const i32 d = rv_wsub(a < last ? a : last, b > first ? b : first);
                    v = (u32)rv_wadd((i32)v, d > 1 ? d : 1);
                });
            }
        }
        val[q] = v;
    }
}

// Fill pass, output reservation without workgroup barriers.  Wavefronts run the rounds of a workgroup
// independently: after its batch of round r a wavefront publishes its staged count and "arrives"; the
// wavefront that arrives LAST adds the 16 counts, reserves the round's output range with ONE global
// atomicAdd and publishes the base with the round's tag.  Nobody waits for that: a wavefront copies the
// pairs of round r out only after it has walked round r+1 (round_copy_out), when the base has long
// arrived.  Every wavefront waits for round r-1's tag before it starts round r+1, so wavefronts are never
// more than one round apart and RP_NSLOT = 4 reservation slots cannot be overwritten while still read.
__device__ __forceinline__ void round_publish(const ProbeLds &L, u32 mine, u32 round, u32 wv, unsigned long long *cursor)
{
    if (lane_id() != 0) return;
    const u32 sl = round % RP_NSLOT;
    L.s_wcnt[sl][wv] = mine;
    const u32 before = __hip_atomic_fetch_add(&L.s_arrive[sl], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (before != RP_W - 1) return;
    u32 tot = 0;
#pragma unroll
    for (int w = 0; w < RP_W; w++) tot += L.s_wcnt[sl][w];
    L.s_base[sl] = tot ? atomicAdd(cursor, (unsigned long long)tot) : 0ull;
    __hip_atomic_store(&L.s_arrive[sl], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_store(&L.s_ready[sl], round + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// wait for round `round`'s reservation; returns where this wavefront's pairs of that round go and whether
// the whole round fits the caller's buffers
__device__ __forceinline__ u64 round_wait(const ProbeLds &L, u32 round, u32 wv, u64 cap, bool &fits)
{
    const u32 sl = round % RP_NSLOT;
    while (__hip_atomic_load(&L.s_ready[sl], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != round + 1u)
        __builtin_amdgcn_s_sleep(1);
    const u64 base = L.s_base[sl];
    u64 g = base;
    u32 tot = 0;
#pragma unroll
    for (int w = 0; w < RP_W; w++) { const u32 c = L.s_wcnt[sl][w]; if (w < (int)wv) g += c; tot += c; }
    fits = base + tot <= cap;
    return g;
}

// copy this wavefront's `mine` staged pairs of round `round` (ring positions start, start+1, ...) to their
// place in the output with full-width stores
__device__ __forceinline__ void round_copy_out(const ProbeLds &L, u32 mine, u32 start, u32 round, u32 wv,
                                               u32 *ob, u32 *op, u64 cap)
{
    bool fits;
    const u64 g = round_wait(L, round, wv, cap, fits);
    if (!mine || !fits) return;
    for (u32 t = lane_id(); t < mine; t += IVX_WAVE) {
        const u64 x = L.s_q[wv][(start + t) & (RP_RING - 1)];
        ob[g + t] = (u32)x; op[g + t] = (u32)(x >> 32);
    }
}

#define IVX_PROBE_LDS(FILL)                                                                          \
    __shared__ unsigned short s_off[RP_CCAP];                                                        \
    __shared__ u64 s_ent[RP_ECAP];                                                                   \
    __shared__ u32 s_row[RP_ECAP];                                                                   \
    __shared__ u64 s_q[FILL ? RP_W : 1][RP_RING];                                                    \
    __shared__ u32 s_wpos[RP_W];                                                                     \
    __shared__ u32 s_wcnt[RP_NSLOT][RP_W];                                                           \
    __shared__ unsigned long long s_base[RP_NSLOT];                                                  \
    __shared__ u32 s_arrive[RP_NSLOT], s_ready[RP_NSLOT];                                            \
    if (threadIdx.x < RP_W) s_wpos[threadIdx.x] = 0;                                                 \
    if (threadIdx.x < RP_NSLOT) { s_arrive[threadIdx.x] = 0; s_ready[threadIdx.x] = 0; }             \
    ProbeLds L{s_off, s_ent, s_row, s_q, s_wpos, s_wcnt, s_base, s_arrive, s_ready};

// ------------------------------------------------------------------ region-major probe (rows scattered by region)
// Persistent workgroups: the partitioned probe rows are cut into equal row shares ("virtual
// workgroups"), a workgroup walks its share region segment by region segment, and inside a segment
// wavefront w owns batches w, w+16, ... of RP_WB rows.
//   MODE 0 (ivx_probe_overlap_count): wavefronts never synchronise; one atomicAdd of the wavefront's
//           total at the end.
//   MODE 1 (fill): single walk, see batch_walk / round_publish / round_copy_out.
//   MODE RV_COUNT / RV_COVERAGE: one 32-bit value per row, written at the row's partitioned position
//           (`ob`), no synchronisation at all; k_unpermute puts the values back in input order.
// rows per lane and wavefront batch of the fill pass, chosen on the device from the pairs expected per ROUTED row
// (`hint` pairs over the rows the partition kept): the same rule as fill_rows_per_lane below
__global__ void k_pick_rows(const u32 *__restrict__ rfirst, u32 nreg, u64 hint, u32 force, u32 *bsel)
{
    const u32 routed = rfirst[nreg];
    const float per_row = (float)((double)hint / (double)(routed ? routed : 1u));
    *bsel = force ? force : per_row <= 0.40f ? 8u : per_row <= 0.8f ? 4u : per_row <= 1.6f ? 2u : 1u;
}

template <int MODE, int B, bool IDENT, bool PAGED = false, bool PK = false>
__global__ __launch_bounds__(RP_T) void k_probe_regions(JoinIndexView ix, const void *__restrict__ rows_a, const void *__restrict__ rows_b,
                                                        const u32 *__restrict__ offs, u32 nblk, u32 vpb,
                                                        u32 *__restrict__ ob, u32 *__restrict__ op, u64 cap,
                                                        unsigned long long *cursor, u32 prow_stride, u32 adj,
                                                        const u32 *unsorted, PageTab pt = PageTab{nullptr, 0u, 0u},
                                                        const u32 *bsel = nullptr, const i32 *__restrict__ ps_in = nullptr, const i32 *__restrict__ pe_in = nullptr,
                                                        u32 rowbits = 32, const u32 *only_if_set = nullptr)
{
    constexpr bool FILL = MODE == 1;
    if (only_if_set != nullptr && *only_if_set == 0u) return;         // (the lean fill kernel took this index: see probe_pairs)
    const u32 rowmask = rowbits >= 32 ? 0xFFFFFFFFu : (1u << rowbits) - 1u;
    const u32 maxlen = pk_maxlen(rowbits);
    static_assert(!PK || PAGED, "packed rows come from the one-pass partition");
    // PK: rows_a holds 8-byte words (start inside the region | length << 24, row id << 32; PK_ESCAPE: the coordinates are
    // read from the input columns ps_in / pe_in by the row id); rows_b is not used
    if (bsel != nullptr && *bsel != (u32)B) return;                   // (every B is launched; k_pick_rows chose one)
    // IDENT: the input already is in region order (k_part_hist left `unsorted` at 0): the partitioned arrays
    // were never written and row i IS input row i.  Both instantiations are launched; the one whose case
    // does not apply returns at once (the host never waits for the flag).
    if ((unsorted != nullptr && *unsorted == 0) != IDENT) return;
    // rows_a / rows_b: the partitioned (qs,qe) and row-id arrays, or -- IDENT -- the input start and end columns, or --
    // PAGED -- the page pool of the one-pass partition: routed row i of region r (whose first routed row is rf) sits at
    // row_at(i, r, rf) of the pool
    static_assert(!(IDENT && PAGED), "paged rows are never read in place");
    __shared__ u32 s_pg[RP_NPG];                                      // the pages of the region segment being walked
    u32 pg_first = 0;
    // (the page id always comes from LDS: a choice between an LDS and a global pointer becomes a flat load with
    //  vmcnt(0) waits that serialise the row loads)
    auto row_at = [&](u64 i, u32, u64 rf) -> u64 {
        if (!PAGED) return i;
        const u32 x = (u32)(i - rf);
        const u32 pg = s_pg[(x >> pt.lgpg) - pg_first] - 1u;
        return ((u64)pg << pt.lgpg) + (x & ((1u << pt.lgpg) - 1u));
    };
    // (all threads; barriers inside) the page ids of routed rows [lo, c_hi) of region r; c_hi is cut back to what RP_NPG
    // pages hold (the caller then walks the rest of the region as another segment)
    auto pages_load = [&](u64 lo, u64 &c_hi, u32 r, u64 rf) {
        if (!PAGED) return;
        __syncthreads();
        pg_first = (u32)(lo - rf) >> pt.lgpg;
        const u64 lim = (rf + ((u64)(pg_first + RP_NPG) << pt.lgpg)) & ~63ull;   // (a cut falls between two 64-row granules)
        if (c_hi > lim) c_hi = lim;
        const u32 npg = ((u32)(c_hi - 1 - rf) >> pt.lgpg) - pg_first + 1u;
        if (threadIdx.x < npg) {
            u32 v = pt.ptab[(u64)r * pt.pstride + pg_first + threadIdx.x];
            // 0 = the partition never published this page (cannot happen once k_part_onepass has completed; it did in a
            // profiling build whose switch skipped the publication, and the page "0 - 1" then was a wild address: round 2's
            // fault).  Read page 0 instead and tell the host.
            if (v == 0u) { v = 1u; if (cursor != nullptr) atomicOr((unsigned int *)(cursor + 1), 1u); }
            s_pg[threadIdx.x] = v;
        }
        __syncthreads();
    };
    auto row_se = [&](u64 i) -> u64 {
        if (IDENT) return (u64)(u32)((u32)((const i32 *)rows_a)[i] + adj) | ((u64)(u32)((u32)((const i32 *)rows_b)[i] - adj) << 32);
        return ((const u64 *)rows_a)[i];
    };
    auto row_id = [&](u64 i, u64 at) -> u32 { return IDENT ? (u32)i : ((const u32 *)rows_b)[at * prow_stride]; };
    constexpr u32 WB = IVX_WAVE * B;                                  // rows per wavefront batch
    IVX_PROBE_LDS(FILL)
    const u32 wv = threadIdx.x / IVX_WAVE, ln = lane_id();
    const u32 nreg = ix.hdr[HDR_NREG];
    // first partitioned row of every region, once, in LDS (the share boundaries below search it)
    __shared__ u32 s_rfirst[IVX_MAXREG_WIDE + 2];
    const bool rf_lds = nreg <= IVX_MAXREG_WIDE;                           // (the two-digit scheme has up to 65025 regions: global table)
    if (rf_lds) for (u32 t = threadIdx.x; t <= nreg; t += RP_T) s_rfirst[t] = offs[(u64)t * nblk];
    __syncthreads();
    auto rfirst = [&](u32 r) -> u32 { return rf_lds ? s_rfirst[r] : offs[(u64)r * nblk]; };
    const u64 total_rows = rfirst(nreg);
    const u32 nvb = gridDim.x * vpb;
    u32 loaded_r = 0xFFFFFFFFu;                                       // region whose slice currently sits in LDS
    Slice S;
    slice_init(ix, S, L);
    u32 round = 0;                                                    // fill pass: rounds of this workgroup so far
    u32 pend_mine = 0, pend_start = 0;                                // the previous round's staged pairs (ring range)
    for (u32 vb = blockIdx.x * vpb; vb < (blockIdx.x + 1) * vpb; vb++) {
        u64 lo = total_rows * vb / nvb;
        const u64 hi = total_rows * (vb + 1) / nvb;
        u64 wcur = 0;                                                 // count pass: pairs seen by this wavefront
        if (lo < hi) {
            u32 r;
            {   // last region whose first row is <= lo
                u32 a = 0, b = nreg;
                while (a < b) { const u32 m = (a + b + 1) >> 1; if (rfirst(m) <= lo) a = m; else b = m - 1; }
                r = a;
            }
            for (; lo < hi; r++) {
                const u64 rend = rfirst(r + 1);
                u64 c_hi = hi < rend ? hi : rend;
                if (c_hi <= lo) continue;
                // every wavefront streams one batch of WB rows per round; the next round's rows are in
                // flight while the current batch walks the LDS slice (the first batch while the slice loads)
                u64 nx[B]; u32 nxr[B];
                // a round is RP_W * WB consecutive rows; wavefront w takes the 64-row granules w, w+16, ... of it, so
                // that dense and empty stretches of sorted input are shared evenly by the 16 wavefronts
                u64 b0 = lo + (u64)wv * IVX_WAVE;
                const u64 rf = PAGED ? rfirst(r) : 0;
                pages_load(lo, c_hi, r, rf);
                // PAGED: when the lane's B rows of the round lie inside the segment and inside one pool page -- nearly always --
                // the first row's place in the pool gives the others' (they are RP_W * 64 rows apart): one bounds test and one
                // page lookup per lane and round instead of B.  (Doing the same with a scalar base per wavefront was measured
                // and dropped, fill 641 -> 703 us: the scalar page lookup waits where the vector one overlaps.)
                u64 nat0 = 0, cat0 = 0;                               // pool position of the lane's first row: of the round in flight / being walked
                auto prefetch = [&](u64, u64 bl) -> bool {
                    if (PAGED) {
                        const u64 i0 = bl + ln, i7 = i0 + (u64)(B - 1) * (RP_W * IVX_WAVE);
                        const u32 x0 = (u32)(i0 - rf), x7 = (u32)(i7 - rf);
                        const bool one = i7 < c_hi && (x0 >> pt.lgpg) == (x7 >> pt.lgpg);
                        if (__ballot(!one) == 0) {                     // (uniform: every lane of the wavefront)
                            const u64 at0 = row_at(i0, r, rf);
                            nat0 = at0;
#pragma unroll
                            for (int q = 0; q < B; q++) {
                                const u64 at = at0 + (u64)q * (RP_W * IVX_WAVE);
                                nx[q] = row_se(at);
                                nxr[q] = (FILL && !PK) ? row_id(i0 + (u64)q * (RP_W * IVX_WAVE), at) : 0u;
                            }
                            return true;
                        }
                    }
#pragma unroll
                    for (int q = 0; q < B; q++) {
                        const u64 i = bl + (u64)q * (RP_W * IVX_WAVE) + ln;
                        const u64 at = i < c_hi ? row_at(i, r, rf) : 0;
                        nx[q] = i < c_hi ? row_se(at) : 0;
                        nxr[q] = (FILL && !PK && i < c_hi) ? row_id(i, at) : 0u;
                    }
                    return false;
                };
                bool nfull = prefetch(lo, b0);
                slice_load(ix, S, L, r, r != loaded_r);
                loaded_r = r;
                for (u64 r0 = lo; r0 < c_hi; r0 += (u64)RP_W * WB, b0 += (u64)RP_W * WB) {
                    i32 qs[B], qe[B]; u32 rowv[B];
                    u32 prel[PK ? B : 1], plen[PK ? B : 1], relmask = 0;   // the packed form, for the walk's 32-bit cell arithmetic
                    u32 okmask = 0;
#pragma unroll
                    for (int q = 0; q < B; q++) {
                        if (PK) {
                            const PkRow w = pk_unpack(nx[q], rowbits);
                            prel[PK ? q : 0] = w.rel; plen[PK ? q : 0] = w.len;
                            qs[q] = (i32)((u32)S.rbase + w.rel); qe[q] = (i32)((u32)qs[q] + w.len); rowv[q] = w.hi & rowmask;
                            nxr[q] = w.len;                             // (kept for the escape test below; the row id prefetch slot is free here)
                        } else { qs[q] = (i32)(u32)nx[q]; qe[q] = (i32)(u32)(nx[q] >> 32); rowv[q] = nxr[q]; }
                        if (!nfull && b0 + (u64)q * (RP_W * IVX_WAVE) + ln < c_hi) okmask |= 1u << q;
                    }
                    if (nfull) okmask = (1u << B) - 1u;
                    const bool cfull = nfull;
                    cat0 = nat0;
                    if (PK) {                                           // rows that did not fit the packed form (rare)
                        u32 esc = 0;
#pragma unroll
                        for (int q = 0; q < B; q++) if (((okmask >> q) & 1u) && nxr[q] == maxlen) esc |= 1u << q;
                        relmask = okmask & ~esc;
                        if (__any(esc != 0)) {                          // all the gathers first, then their uses: one round trip, not 2 * B
                            i32 ts[B], te[B];
#pragma unroll
                            for (int q = 0; q < B; q++) { const u32 rr = ((esc >> q) & 1u) ? rowv[q] : 0u; ts[q] = ps_in[rr]; te[q] = pe_in[rr]; }
#pragma unroll
                            for (int q = 0; q < B; q++) if ((esc >> q) & 1u) { qs[q] = (i32)((u32)ts[q] + adj); qe[q] = (i32)((u32)te[q] - adj); }
                        }
                    }
                    nfull = prefetch(r0 + (u64)RP_W * WB, b0 + (u64)RP_W * WB);
                    if (MODE >= RV_COUNT) {
                        u32 val[B];
                        if constexpr (PK) batch_rowval<MODE, B, true>(S, qs, qe, okmask, val, (const u32 (&)[B])prel, (const u32 (&)[B])plen, relmask);
                        else batch_rowval<MODE, B, false>(S, qs, qe, okmask, val, (const u32 (&)[B])qs, (const u32 (&)[B])qs, 0u);
#pragma unroll
                        for (int q = 0; q < B; q++) {
                            if (!((okmask >> q) & 1u)) continue;
                            const u64 i = b0 + (u64)q * (RP_W * IVX_WAVE) + ln;
                            if (PAGED) {    // in place: the value takes the low half of the row's packed word, the row id stays above it
                                const u64 at = cfull ? cat0 + (u64)q * (RP_W * IVX_WAVE) : row_at(i, r, rf);
                                ((u64 *)ob)[at] = (u64)val[q] | ((u64)rowv[q] << 32);      // (ob = the page pool itself)
                            } else ob[i] = val[q];
                        }
                        continue;
                    }
                    u32 start = 0;
                    bool direct = false;
                    u32 got;
                    if constexpr (PK) got = batch_walk<FILL, B, true>(S, L, qs, qe, rowv, okmask, wv, pend_start, start, direct, (const u32 (&)[B])prel, (const u32 (&)[B])plen, relmask);
                    else got = batch_walk<FILL, B, false>(S, L, qs, qe, rowv, okmask, wv, pend_start, start, direct, (const u32 (&)[B])qs, (const u32 (&)[B])qs, 0u);
                    if (MODE == 0) { wcur += got; continue; }
                    round_publish(L, got, round, wv, cursor);
                    if (direct) {                              // needs this round's range now: wait for the 16th wavefront
                        bool fits;
                        const u64 g = round_wait(L, round, wv, cap, fits);
                        batch_write_direct<B>(S, L, qs, qe, rowv, okmask, wv, g, fits, ob, op);
                        start += got; got = 0;                 // nothing staged; the second walk moved the ring position too
                    }
                    if (round) round_copy_out(L, pend_mine, pend_start, round - 1, wv, ob, op, cap);
                    pend_mine = got; pend_start = start; round++;
                }
                lo = c_hi;
                if (PAGED && lo < hi && lo < rend) r--;               // the segment was cut at the page window: same region again
            }
        }
        if (MODE == 0) {
            const u64 tot = wave_sum(wcur);
            if (ln == 0 && tot) atomicAdd(cursor, (unsigned long long)tot);
        }
    }
    if (FILL && round) round_copy_out(L, pend_mine, pend_start, round - 1, wv, ob, op, cap);
}

// ------------------------------------------------------------------ lean probes: what the lean kernels share
// k_fill_fast and k_lean serve the case the headline always meets: packed 8-byte rows in region pages (k_part_onepass) and
// an index whose every region is one LDS-resident level (hdr[HDR_FAST]).  They share how a workgroup gets its rows
// (LeanRows), how a row finds its cell range in the staged slice (lean_cells) and what happens to a row the packed form
// cannot carry (lean_list_slow, and rest_row in the *_rest kernels that walk the listed rows afterwards with the generic
// walk over the index in global memory -- the lean kernels hold no generic code, and no scratch).  The fill is a kernel of
// its own (a ring, rounds); every per-row operator is k_lean with its LDS, what it does when the region changes and what it
// does with a row's candidates filled in.

// The rows of a workgroup, batch by batch.  Work is dealt in CHUNKS of 8192 routed rows that never straddle a pool page
// (chunk k of region r = its virtual rows [8192 k, 8192 (k + 1)); wavefront w owns rows [512 w, 512 (w + 1)) of it), so the
// rows of a wavefront batch are 64 * B consecutive words behind ONE wave-uniform pointer: loads are `scalar base + lane
// offset + immediate`, with no per-row bounds test, page lookup or 64-bit address arithmetic (a third of the general
// kernel's instructions).  A workgroup takes an equal share of all chunks.  One batch is always in flight: take() hands
// out the one whose loads were started before and starts the next one's.
template <int B, class W>
struct LeanRows {
    static constexpr u32 WB = IVX_WAVE * B;                           // rows of a wavefront batch
    static constexpr u32 SUB = 8u / B;                                // batches a wavefront makes of its 512 rows of a chunk
    const u32 *s_cfirst, *rcur; PageTab pt; W *pool;
    u32 rowbits, maxlen, wv, ln, nreg, c_lo, nbatch;
    // the batch in flight: its region, first virtual row and row count are wave-uniform, its rows 64 * B consecutive words
    // of one pool page behind src
    u32 r, first, cnt; W *src; u64 nx[B];
    struct Batch { u32 first, cnt; W *src; };

    // The workgroup's share of the chunks (all threads; ONE barrier inside, which also covers whatever LDS the kernel
    // initialised before the call).  s_cf: LDS for cfirst, the first chunk of every region.  False: no chunk falls to this
    // workgroup, which leaves.  (init only tests; the work of a workgroup that stays is start's: with it on one side of the
    // test here the compiler kept a second copy of the test behind the call.)
    __device__ __forceinline__ bool init(const JoinIndexView &ix, u32 *s_cf, const u32 *cfirst, const u32 *rcur_, const PageTab &pt_, W *pool_, u32 rowbits_)
    {
        s_cfirst = s_cf; rcur = rcur_; pt = pt_; pool = pool_; rowbits = rowbits_; maxlen = pk_maxlen(rowbits_);
        wv = __builtin_amdgcn_readfirstlane(threadIdx.x / IVX_WAVE); ln = lane_id();
        nreg = ix.hdr[HDR_NREG];
        for (u32 t = threadIdx.x; t <= nreg; t += RP_T) s_cf[t] = cfirst[t];
        __syncthreads();
        return share();
    }
    // The same without a table: the workgroup scans the regions' chunk counts itself, thread t region t's (every workgroup
    // the same 4 KB of counters out of L2, instead of a one-workgroup kernel in front of this one and the boundary it
    // costs).  red: RP_W + 1 words of LDS that hold nothing yet.
    __device__ __forceinline__ bool init_scan(const JoinIndexView &ix, u32 *s_cf, u32 *red, const u32 *rcur_, const PageTab &pt_, W *pool_, u32 rowbits_)
    {
        static_assert(IVX_MAXREG_WIDE < RP_T, "init_scan: one region per thread, and thread nreg for the total");
        s_cfirst = s_cf; rcur = rcur_; pt = pt_; pool = pool_; rowbits = rowbits_; maxlen = pk_maxlen(rowbits_);
        wv = __builtin_amdgcn_readfirstlane(threadIdx.x / IVX_WAVE); ln = lane_id();
        nreg = ix.hdr[HDR_NREG];
        const u32 t = threadIdx.x;
        u32 tot;
        const u32 ex = block_excl_scan<u32, RP_T>(t < nreg ? (rcur_[t] + FP_CHUNK - 1) / FP_CHUNK : 0u, red, &tot);
        if (t <= nreg) s_cf[t] = ex;                                     // (thread nreg: everything before it, the total)
        __syncthreads();
        return share();
    }
    __device__ __forceinline__ bool share()
    {
        const u32 nchunk = s_cfirst[nreg];
        c_lo = (u32)((u64)nchunk * blockIdx.x / gridDim.x);
        const u32 c_hi = (u32)((u64)nchunk * (blockIdx.x + 1) / gridDim.x);
        nbatch = (c_hi - c_lo) * SUB;
        return c_lo < c_hi;
    }
    // batch 0 in flight.  miss(): see routed_word
    template <class Miss>
    __device__ __forceinline__ void start(Miss &&miss)
    {
        {   // last region whose first chunk is <= c_lo
            u32 a = 0, b = nreg;
            while (a < b) { const u32 m = (a + b + 1) >> 1; if (s_cfirst[m] <= c_lo) a = m; else b = m - 1; }
            r = a;
        }
        src = pool;
        prefetch(0, miss);
    }
    // batch i of this wavefront becomes the one in flight (r only ever moves forward)
    template <class Miss>
    __device__ __forceinline__ void prefetch(u32 i, Miss &&miss)
    {
        const u32 c = c_lo + i / SUB, sb = i % SUB;
        while (c >= s_cfirst[r + 1]) r++;
        first = (c - s_cfirst[r]) * FP_CHUNK + wv * (8u * IVX_WAVE) + sb * WB;
        const u32 rows = rcur[r];
        cnt = rows > first ? (rows - first < WB ? rows - first : WB) : 0u;
        if (cnt) {
            src = routed_word(pt, pool, r, first, miss);
#pragma unroll
            for (int q = 0; q < B; q++) nx[q] = src[q * IVX_WAVE + ln];      // (inside the page whatever cnt is: pages are whole)
        }
    }
    // batch i (the caller has read its region from `r`): where it is, and its rows decoded -- start inside the region, length,
    // the word's upper half; batch i + 1 is in flight afterwards
    template <class Miss>
    __device__ __forceinline__ Batch take(u32 i, u32 (&rel)[B], u32 (&len)[B], u32 (&hi)[B], Miss &&miss)
    {
        const Batch b{first, cnt, src};
#pragma unroll
        for (int q = 0; q < B; q++) { const PkRow w = pk_unpack(nx[q], rowbits); rel[q] = w.rel; len[q] = w.len; hi[q] = w.hi; }
        if (i + 1 < nbatch) prefetch(i + 1, miss);
        return b;
    }
};

// The cell offsets [ca, cb) of a batch's B rows in the staged slice S (`fast`: see probe_row_rel), all fetched before the
// first candidate loop runs: their LDS reads are in flight together.  slow: the lane's rows the packed form cannot carry
// (lean_list_slow takes them); okm: its rows that are walked here.
template <int B, bool FULL>
__device__ __forceinline__ void lean_cells_of(const Slice &S, const u32 (&rel)[B], const u32 (&len)[B], u32 maxlen, u32 cnt, u32 ln,
                                              u32 (&ca)[B], u32 (&cb)[B], u32 &slow, u32 &okm)
{
    const u32 sh0 = S.sh0, off = S.off, cmax = S.cmax, ncm1 = S.ncm1;
#pragma unroll
    for (int q = 0; q < B; q++) {
        const u32 t = ((rel[q] + 1u) >> sh0) + off;                      // first cell a matching build row can start in: one cell back
        const u32 bl0 = (t > 1u ? t : 1u) - 1u;
        const u32 bh0 = ((rel[q] + len[q]) >> sh0) + off;
        const u32 bh = bh0 < cmax ? bh0 : cmax;
        bool bad = len[q] == maxlen || bh >= ncm1;                       // escape, or past the slice's halo: the rest list's
        const bool ok = FULL || (u32)q * IVX_WAVE + ln < cnt;            // (only a region's last batch is short)
        if (ok && bad) slow |= 1u << q;
        if (ok && !bad) okm |= 1u << q;
        bad |= !ok;
        // no row to walk: an empty range (twice the same offset); a row behind the key's last cell gets one by the clamp
        const u32 e1 = bad ? 0u : bh + 1u;
        const u32 bl = bl0 < e1 ? bl0 : e1;
        ca[q] = S.s_off[bl];
        cb[q] = S.s_off[e1];
    }
}
// (two copies of the block, chosen once per batch: a per-row choice between "every lane holds B rows" and "test the lane's
//  row number" was two branches per row)
template <int B>
__device__ __forceinline__ void lean_cells(const Slice &S, const u32 (&rel)[B], const u32 (&len)[B], u32 maxlen, u32 cnt, u32 ln,
                                           u32 (&ca)[B], u32 (&cb)[B], u32 &slow, u32 &okm)
{
    slow = 0; okm = 0;
    if (cnt == IVX_WAVE * B) lean_cells_of<B, true>(S, rel, len, maxlen, cnt, ln, ca, cb, slow, okm);
    else lean_cells_of<B, false>(S, rel, len, maxlen, cnt, ln, ca, cb, slow, okm);
}

// this lane's slow rows of the batch at virtual row `first` of region r, one by one, to the rest list (their cell ranges
// were empty: nothing was walked for them)
template <int B>
__device__ __forceinline__ void lean_list_slow(u32 slow, u32 r, u32 first, u32 ln, u64 *__restrict__ rest_rows, u32 *rest_n)
{
#pragma unroll
    for (int q = 0; q < B; q++)
        if ((slow >> q) & 1u) rest_rows[atomicAdd(rest_n + 1, 1u)] = (u64)(first + (u32)q * IVX_WAVE + ln) | ((u64)r << 32);
}

// One listed row -- routed row v of region r -- as the *_rest kernels want it: its word's place in the pool, its row id, the
// word's upper half and its closed coordinates, from the word or -- an escape -- from the input columns by the row id (adj: the
// strict mode's shrinking, which the routing pass applied to the rows it packed)
template <class W> struct RestRow { W *slot; u32 row, hi; i32 qs, qe; };
template <class W, class Miss>
__device__ __forceinline__ RestRow<W> rest_row(const JoinIndexView &ix, const PageTab &pt, W *pool, u32 r, u32 v, u32 rowbits,
                                               const i32 *ps_in, const i32 *pe_in, u32 adj, Miss &&miss)
{
    W *slot = routed_word(pt, pool, r, v, miss);
    const PkRow w = pk_unpack(*slot, rowbits);
    const u32 row = w.hi & (rowbits >= 32 ? 0xFFFFFFFFu : (1u << rowbits) - 1u);
    i32 qs, qe;
    if (w.len == pk_maxlen(rowbits)) { qs = (i32)((u32)ps_in[row] + adj); qe = (i32)((u32)pe_in[row] - adj); }
    else { qs = (i32)((u32)ix.rdesc[r].rbase + w.rel); qe = (i32)((u32)qs + w.len); }
    return RestRow<W>{slot, row, w.hi, qs, qe};
}

// ------------------------------------------------------------------ lean fill probe
// The headline's fill pass over LeanRows.  Same slices, same staging ring and round-level output reservation as
// k_probe_regions<fill>; what differs is what a wavefront executes per row -- that kernel is bound by the instructions it
// issues, 224 per 64 rows:
//  * no per-row address work (LeanRows);
//  * the walk is the 32-bit packed-row form only, staged as (slot, probe row): the slot -> build row lookup happens once per
//    64 pairs in the copy-out, not per match inside the divergent loop; the cell offsets of all B rows are fetched before
//    the first candidate loop runs;
//  * rows the packed form cannot carry (escapes, rows reaching past the slice's halo) and batches that overflow the ring
//    go to the rest lists: k_fill_rest walks them (cold code, out of this kernel);
//  * the last wavefront to arrive in a round leaves every wavefront's output position, not just the round's base.
template <int B, bool DRAIN>
__global__ __launch_bounds__(RP_T) void k_fill_fast(JoinIndexView ix, const u64 *__restrict__ pool, const u32 *__restrict__ rcur,
                                                    PageTab pt, u32 *__restrict__ ob, u32 *__restrict__ op, u64 cap,
                                                    unsigned long long *cursor, const u32 *bsel, u32 rowbits, FpRest *__restrict__ rest, u64 *__restrict__ rest_rows, u32 *rest_n,
                                                    u32 drain)
{
    if (bsel != nullptr && *bsel != (u32)B) return;                   // (every B is launched; k_pick_rows chose one)
    if (ix.hdr[HDR_SLOW] != 0u) return;                               // not every region is one LDS-resident level: the general kernel's
    IVX_PROBE_LDS(true)
    __shared__ u32 s_cfirst[IVX_MAXREG_WIDE + 2];
    __shared__ u32 s_wat[RP_NSLOT][RP_W];                             // a wavefront's output position inside its round's range
    __shared__ u32 s_stash[DRAIN ? RP_W : 1][RP_STASH];                        // a wavefront's unfinished list tails of the batch at hand (see the walk)
    const u32 wv = __builtin_amdgcn_readfirstlane(threadIdx.x / IVX_WAVE), ln = lane_id();
    auto miss = [&]() { if (ln == 0) atomicOr((unsigned int *)(cursor + 1), 1u); };     // a page never published: the host is told
    LeanRows<B, const u64> rows;
    if (!rows.init_scan(ix, s_cfirst, &s_wat[0][0], rcur, pt, pool, rowbits)) return;     // (s_wat: not in use before the first round)
    Slice S;
    slice_init(ix, S, L);
    rows.start(miss);
    const u32 rowmask = rowbits >= 32 ? 0xFFFFFFFFu : (1u << rowbits) - 1u;
    u32 loaded_r = 0xFFFFFFFFu;
    u32 round = 0;
    u32 pend_mine = 0;                                                // pairs the previous round staged (in its half of the ring)
    // The ring is two halves of RP_RING / 2 pairs; round r stages into half r & 1 from the half's start, so nothing a round
    // does can touch the previous round's pairs (which wait in the other half for their copy-out) and the walk needs no
    // per-pair room test: a round that finds more pairs than a half holds wraps over its own pairs, is recognised by its count
    // and goes to the rest list.  The position inside the half is wave-private state in a scalar register (ranks by ballot: no
    // LDS atomic, no wait per match); the candidate loops are wave-uniform -- every lane stays in until the longest list is
    // done, its steps predicated -- so that the position is one value for the wavefront by construction.
    constexpr u32 HALF = RP_RING / 2;
    // copy this wavefront's staged pairs of round pr out: (slice slot as the LDS address of its entry, packed row word) ->
    // (build row, probe row)
    auto copy_out = [&](u32 pr) {
        const u32 sl = pr % RP_NSLOT;
        while (__hip_atomic_load(&L.s_ready[sl], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != pr + 1u) __builtin_amdgcn_s_sleep(1);
        if (!pend_mine) return;
        const u64 base = L.s_base[sl];
        const u32 tot = s_wat[sl][RP_W - 1] + L.s_wcnt[sl][RP_W - 1];
        if (base + tot > cap) return;                                 // the caller's buffers are too small: nothing of the round is written
        const u64 g = base + s_wat[sl][wv];
        u32 *ob_w = ob + g, *op_w = op + g;
        const uint2 *half = (const uint2 *)L.s_q[wv] + (pr & 1u) * HALF;
        for (u32 t = ln; t < pend_mine; t += IVX_WAVE) {
            const uint2 x = half[t];
            ob_w[t] = L.s_row[x.x]; op_w[t] = x.y & rowmask;
        }
    };
    for (u32 i = 0; i < rows.nbatch; i++) {
        const u32 r = rows.r;
        if (r != loaded_r) {
            // the ring holds slice slots: whatever is still staged leaves before the slice changes
            if (round) { copy_out(round - 1u); pend_mine = 0; }
            slice_load(ix, S, L, r, true);
            loaded_r = r;
        }
        // ---- decode the batch in flight, start the next one
        u32 rel[B], len[B], roww[B];                                     // (roww: the row id is masked out of it in the copy-out, 64 pairs at a time)
        const auto bt = rows.take(i, rel, len, roww, miss);
        const u32 first = bt.first, cnt = bt.cnt;
        // ---- cells: of all B rows first, then the candidate loops
        const i32 rbase = S.rbase;
        u32 ca[B], cb[B], slow, okm;
        lean_cells<B>(S, rel, len, rows.maxlen, cnt, ln, ca, cb, slow, okm);
        u32 wpos = 0;                                                    // pairs of this round so far (scalar)
        uint2 *half = (uint2 *)L.s_q[wv] + (round & 1u) * HALF;
        // one step of the lock-step walk: every lane of actm tests the slice entry at its j and moves on
        // (lane masks straight from the compares -- uicmp / sicmp -- and back into a predicate -- inverse_ballot: the
        //  bool-to-ballot round trip of `ballot(act && ...)` cost two VALU instructions per step, the recomputed loop
        //  test one more: 13 -> 10 per step, and the walk is what the kernel's time goes into)
        auto step = [&](u32 &j, u32 jend, i32 qs, i32 qe, u32 rw, u64 &actm) {
            const u64 x = L.s_ent[j];                                    // (a lane past its list reads on inside LDS; its result is not used)
            const u64 mm = actm & __builtin_amdgcn_sicmp((i32)(u32)x, qe, 41 /* SLE */) & __builtin_amdgcn_sicmp((i32)(u32)(x >> 32), qs, 39 /* SGE */);
            if (__builtin_amdgcn_inverse_ballot_w64(mm)) half[mask_rank_from(mm, wpos) & (HALF - 1)] = make_uint2(j, rw);      // (the counter's addend carries the position)
            wpos += (u32)__popcll(mm);
            j++;
            actm = __builtin_amdgcn_uicmp(j, jend, 36 /* ULT */);       // lanes whose list is not done
        };
        // Drained walk (DRAIN; without it the kernel is the plain walk, instruction for instruction, and holds no stash).  A
        // 64-row group runs as many steps as its longest list, and after two steps most lanes idle (1.4 candidates per row,
        // the longest of 64 lists ~5).  So a group's walk ends as soon as at most `drain` lanes are still active: each of them
        // leaves (next slice slot, the row's slot in the batch) in the wavefront's stash, and ONE 64-lane pass per batch walks
        // all stashed tails side by side (below).  Slots by ballot rank behind a scalar fill count, as in the ring; no atomic,
        // no barrier, no wait on another wavefront.
        u32 sfill = 0;                                                   // tails stashed so far in this batch (scalar)
#pragma unroll
        for (int q = 0; q < B; q++) {
            const i32 qs = (i32)((u32)rbase + rel[q]), qe = (i32)((u32)qs + len[q]);
            u32 j = ca[q];
            const u32 jend = cb[q];
            // (walking two or four rows' lists side by side -- their slice reads in flight together, one wait for all -- was
            //  measured: no change.  The walk is bound by the instructions it issues, not by those waits.)
            // One backward branch per step; the match block sits on the fall-through path (a taken branch empties the
            // wavefront's instruction buffer, and the kernel retired 31 branches per 64 rows).
            u64 actm = __builtin_amdgcn_uicmp(j, jend, 36);
            if constexpr (!DRAIN) {
                if (actm != 0) {
                    do step(j, jend, qs, qe, roww[q], actm); while (actm != 0);
                }
            } else {
                // the group walks on while more lanes are active than may be drained or the stash has room for
                const u32 lim = drain < RP_STASH - sfill ? drain : RP_STASH - sfill;
                if ((u32)__popcll(actm) > lim) {
                    // (a group that starts with that many lists takes its first steps without a test -- no count, no compare,
                    //  no branch: a step past the longest list changes nothing -- a group of few lists is stashed at once)
#pragma unroll
                    for (int h = 0; h < FD_HEAD; h++) step(j, jend, qs, qe, roww[q], actm);
                    while ((u32)__popcll(actm) > lim) step(j, jend, qs, qe, roww[q], actm);
                }
                if (actm != 0) {
                    if (__builtin_amdgcn_inverse_ballot_w64(actm)) s_stash[wv][mask_rank_from(actm, sfill)] = j | (((u32)q * IVX_WAVE + ln) << FD_SLOT_SHIFT);
                    sfill += (u32)__popcll(actm);
                }
            }
        }
        // ---- the stashed tails, one per lane: the row's word again from the batch's 4 KB (just streamed), the end of its list
        // as lean_cells found it (a stashed row is one that was walked: neither slow nor past the batch's rows), the same step
        if (DRAIN && sfill != 0) {
            // the entries were written by other lanes of this wavefront: order the LDS writes above before the reads below
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const bool has = ln < sfill;
            const u32 e = has ? s_stash[wv][ln] : 0u;
            const PkRow w = pk_unpack(bt.src[e >> FD_SLOT_SHIFT], rowbits);     // (a lane without a tail: row 0 of the batch, an empty list)
            const i32 qs = (i32)((u32)rbase + w.rel), qe = (i32)((u32)qs + w.len);
            const u32 bh0 = ((w.rel + w.len) >> S.sh0) + S.off;
            u32 j = e & ((1u << FD_SLOT_SHIFT) - 1u);
            const u32 jend = has ? (u32)S.s_off[(bh0 < S.cmax ? bh0 : S.cmax) + 1u] : 0u;
            u64 actm = __builtin_amdgcn_uicmp(j, jend, 36);
            while (actm != 0) step(j, jend, qs, qe, w.hi, actm);
            // (the stash is empty again: sfill starts from 0 in the next batch, and nothing staged outlives a slice)
        }
        u32 got = wpos;
        // more pairs than the half holds: nothing of this batch counts as staged
        const bool skip = got > HALF;
        if (__builtin_expect(skip, 0)) {
            // (as 64-row pieces: each gets a wavefront of its own in k_fill_rest)
            if (ln < B && ln * IVX_WAVE < cnt) rest[atomicAdd(rest_n, 1u)] = FpRest{r, first + ln * IVX_WAVE, cnt - ln * IVX_WAVE < IVX_WAVE ? cnt - ln * IVX_WAVE : (u32)IVX_WAVE, 0u};
            got = 0;
        } else if (__builtin_expect(slow != 0, 0)) lean_list_slow<B>(slow, r, first, ln, rest_rows, rest_n);
        // ---- publish the round's count; the last wavefront to arrive reserves the round's output range
        if (ln == 0) {
            const u32 sl = round % RP_NSLOT;
            L.s_wcnt[sl][wv] = got;
            const u32 before = __hip_atomic_fetch_add(&L.s_arrive[sl], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (before == RP_W - 1) {
                u32 tot = 0;
#pragma unroll
                for (int w = 0; w < RP_W; w++) { s_wat[sl][w] = tot; tot += L.s_wcnt[sl][w]; }
                L.s_base[sl] = tot ? atomicAdd(cursor, (unsigned long long)tot) : 0ull;
                __hip_atomic_store(&L.s_arrive[sl], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_store(&L.s_ready[sl], round + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        if (round) copy_out(round - 1u);                              // the previous round's pairs: its base has long arrived
        pend_mine = got; round++;
    }
    if (round) copy_out(round - 1u);
}

// What k_fill_fast left: single rows (one lane each) and whole batches (one wavefront each, 64 rows at a time); coordinates
// from the packed word or -- escapes -- the input columns, the generic walk over the index in global memory (count, one
// output reservation per 64 rows, write).
__global__ __launch_bounds__(256) void k_fill_rest(JoinIndexView ix, const u64 *__restrict__ pool, PageTab pt, const FpRest *__restrict__ rest,
                                                   const u64 *__restrict__ rest_rows, const u32 *__restrict__ rest_n, u32 *__restrict__ ob,
                                                   u32 *__restrict__ op, u64 cap, unsigned long long *cursor, const i32 *__restrict__ ps_in,
                                                   const i32 *__restrict__ pe_in, u32 rowbits, u32 *done, u64 *host_totals)
{
    const u32 nbat = rest_n[0], nrow = rest_n[1];
    const u32 wpb = blockDim.x / IVX_WAVE, ln = lane_id();
    const u32 sh0 = ix.hdr[HDR_SH0], nlev = ix.hdr[HDR_NLEV];
    // 64 routed rows, one per lane: (region, virtual row) or nothing
    auto rows64 = [&](bool ok, u32 r, u32 v) {
        i32 qs = 0, qe = -1; u32 row = 0, k = 0;
        if (ok) {
            // (the fault word's atomic returns its value and the lane takes it: performed before the lane goes on, as the
            //  exit below needs it)
            const auto e = rest_row(ix, pt, pool, r, v, rowbits, ps_in, pe_in, 0u, [&]() {
                const u32 was = atomicOr((unsigned int *)(cursor + 1), 1u);
                asm volatile("" ::"v"(was));
            });
            qs = e.qs; qe = e.qe; row = e.row;
            k = ix.rkey[r];
        }
        u32 m = 0;
        if (ok) walk(ix, sh0, 0, nlev, k, qs, qe, [&](u32) { m++; });
        const u32 inc = wave_incl_scan(m);
        const u32 tot = __shfl(inc, IVX_WAVE - 1, IVX_WAVE);
        if (tot == 0) return;
        unsigned long long g = 0;
        if (ln == 0) g = atomicAdd(cursor, (unsigned long long)tot);
        g = __shfl(g, 0, IVX_WAVE);
        if (g + tot > cap) return;                                       // (the count still tells the caller what it needs)
        u64 at = g + inc - m;
        if (m) walk(ix, sh0, 0, nlev, k, qs, qe, [&](u32 brow) { ob[at] = brow; op[at] = row; at++; });
    };
    const u32 wave = blockIdx.x * wpb + threadIdx.x / IVX_WAVE, nwave = gridDim.x * wpb;
    for (u32 i0 = wave * IVX_WAVE; i0 < nrow; i0 += nwave * IVX_WAVE) {
        const bool ok = i0 + ln < nrow;
        const u64 e = ok ? rest_rows[i0 + ln] : 0ull;
        rows64(ok, (u32)(e >> 32), (u32)e);
    }
    for (u32 b = wave; b < nbat; b += nwave) {
        const FpRest w = rest[b];
        for (u32 t0 = 0; t0 < w.cnt; t0 += IVX_WAVE) rows64(t0 + ln < w.cnt, w.r, w.first + t0 + ln);
    }
    // host_totals (nullable; mapped host memory): this kernel is the call's last device work, and its last workgroup to
    // leave hands the pair total and the fault word to the host -- no copy kernel behind it, the host only waits for the
    // stream.  What orders the accesses: both words change by device-scope atomics only, which are performed at the memory's
    // coherent point, not in an XCD's L2, and EVERY one of this kernel's atomics on them returns its value to a lane that
    // uses it (the cursor's addend base; the fault word's old value, taken by an empty asm) -- so the wavefront has waited for
    // it, i.e. it is performed, before the wavefront reaches the barrier below.  Thread 0 counts its workgroup after that
    // barrier with a returning atomic of the same scope, and the workgroup that counts last reads both words with loads of
    // that scope, issued after its count has returned.  No release fence: one per wavefront wrote its XCD's L2 back behind
    // k_fill_fast's output and took the kernel from 15 to 49 us.  No workgroup waits for another.
    if (host_totals == nullptr) return;
    __syncthreads();
    if (threadIdx.x == 0 && __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u) {
        host_store(host_totals, (u64)__hip_atomic_load(cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        host_store(host_totals + 1, (u64)__hip_atomic_load(cursor + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
}

// ------------------------------------------------------------------ lean per-row operators
// A per-row operator Op (ivx_rowops.hpp: RvOp, MarkOp, AggOp, SelOp) over LeanRows and lean_cells, without a ring, rounds or
// any synchronisation between wavefronts: when the region changes, the slice load between Op's leave and enter; per row, the
// candidate loop over the staged entries, Op::Row::hit for a match, Op::Row::done for the row.  Rows the packed form cannot
// carry are listed (region, virtual row) and k_lean_rest walks them.
#ifndef IVX_RV_WPS
#define IVX_RV_WPS 4
#endif
#ifndef IVX_RV_B
#define IVX_RV_B 8
#endif
#ifndef IVX_AGG_B
#define IVX_AGG_B 4
#endif
template <int B, class Op>
__global__ __launch_bounds__(RP_T, IVX_RV_WPS) void k_lean(JoinIndexView ix, typename Op::W *__restrict__ pool, const u32 *__restrict__ rcur, const u32 *__restrict__ cfirst,
                                               PageTab pt, u32 rowbits, u64 *__restrict__ rest_rows, u32 *rest_n, Op op)
{
    __shared__ unsigned short s_off[RP_CCAP];
    __shared__ u64 s_ent[RP_ECAP];
    __shared__ u32 s_cfirst[IVX_MAXREG_WIDE + 2];
    // (the compiler lays a kernel's LDS out by the variables' names: s_own sits behind s_ent and s_off, which keep the low
    //  offsets that a DS instruction's 16-bit immediate reaches)
    __shared__ typename Op::Lds s_own;
    ProbeLds L{s_off, s_ent, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const u32 ln = lane_id();
    op.begin(s_own);                                                      // (the barrier behind it is init's)
    auto miss = []() {};                                                 // (a page never published: stay in bounds, silently)
    LeanRows<B, typename Op::W> rows;
    if (!rows.init(ix, s_cfirst, cfirst, rcur, pt, pool, rowbits)) return;
    Slice S;
    slice_init(ix, S, L);
    rows.start(miss);
    u32 loaded_r = 0xFFFFFFFFu;
    for (u32 i = 0; i < rows.nbatch; i++) {
        const u32 r = rows.r;
        if (r != loaded_r) {
            if (loaded_r != 0xFFFFFFFFu) op.leave(ix, S, s_own);
            slice_load(ix, S, L, r, true);
            op.enter(ix, S, r, s_own);
            loaded_r = r;
        }
        u32 rel[B], len[B], roww[B];                                     // (roww: the word's upper half, for operators that write the word)
        const auto bt = rows.take(i, rel, len, roww, miss);
        const u64 at = (u64)(bt.src - pool) + ln;                        // the lane's first row of the batch: its word's place in the pool
        const i32 rbase = S.rbase;
        u32 ca[B], cb[B], slow, okm;
        lean_cells<B>(S, rel, len, rows.maxlen, bt.cnt, ln, ca, cb, slow, okm);
#pragma unroll
        for (int q = 0; q < B; q++) {
            const i32 qs = (i32)((u32)rbase + rel[q]), qe = (i32)((u32)qs + len[q]);
            typename Op::Row a;
            for (u32 j = ca[q]; j < cb[q]; j++) {
                const u64 x = s_ent[j];
                const i32 xs = (i32)(u32)x, xe = (i32)(u32)(x >> 32);
                if (xs <= qe && xe >= qs) a.hit(op, s_own, j, qs, qe, xs, xe);
            }
            if ((okm >> q) & 1u) a.done(op, bt.src + q * IVX_WAVE + ln, at + (u32)q * IVX_WAVE, roww[q]);
        }
        if (__builtin_expect(slow != 0, 0)) lean_list_slow<B>(slow, r, bt.first, ln, rest_rows, rest_n);
    }
    op.leave(ix, S, s_own);
}

template <class Op>
__global__ __launch_bounds__(256) void k_lean_rest(JoinIndexView ix, typename Op::W *__restrict__ pool, PageTab pt, const u64 *__restrict__ rest_rows,
                                                   const u32 *__restrict__ rest_n, const i32 *__restrict__ ps_in, const i32 *__restrict__ pe_in,
                                                   u32 rowbits, Op op)
{
    const u32 nrow = rest_n[1];
    const u32 sh0 = ix.hdr[HDR_SH0], nlev = ix.hdr[HDR_NLEV];
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < nrow; i += gridDim.x * blockDim.x) {
        const u64 ent = rest_rows[i];
        const u32 r = (u32)(ent >> 32);
        const auto e = rest_row(ix, pt, pool, r, (u32)ent, rowbits, ps_in, pe_in, op.adj, []() {});
        const i32 qs = e.qs, qe = e.qe;
        typename Op::Row a;
        if (!Op::skip_empty || !(qe < qs)) walk_ent(ix, sh0, 0, nlev, ix.rkey[r], qs, qe, [&](const ivx_ent &x) { a.hit(op, x, qs, qe); });
        a.done(op, e.slot, (u64)(e.slot - pool), e.hi);
    }
}

// ------------------------------------------------------------------ match-dense fill: count, scan, write
// With several pairs per probe row the staging ring holds only one 64-row batch per wavefront and the 16
// wavefronts of a workgroup end up in lock step, round after round.  For such joins the pairs are written in two
// passes over the same decomposition instead, with no ring, no atomics and no synchronisation between wavefronts:
//   piece   = the rows of one 64-row granule [64g, 64g+64) of the partitioned order that belong to region r
//             (row shares start at multiples of 64, so a piece has ONE owner); slot(piece) = g + r, which grows
//             strictly along the row order
//   PASS 0  every piece's pair count goes to pcount[slot]; an exclusive scan turns it into output offsets
//   PASS 1  the piece is walked again in lock step (every lane steps through its candidates together); the lanes
//           that match in a step take consecutive positions after the piece's running offset by ballot rank, so
//           the stores of a step are contiguous.  Order inside a piece is arbitrary, like everywhere else.
template <int PASS, bool IDENT, bool PAGED = false, bool PK = false>
__global__ __launch_bounds__(RP_T) void k_probe_dense(JoinIndexView ix, const void *__restrict__ rows_a, const void *__restrict__ rows_b,
                                                      const u32 *__restrict__ offs, u32 nblk, u32 prow_stride, const u32 *unsorted,
                                                      u64 *__restrict__ pcount, u32 *__restrict__ ob, u32 *__restrict__ op, u64 cap,
                                                      PageTab pt = PageTab{nullptr, 0u, 0u}, const i32 *__restrict__ ps_in = nullptr, const i32 *__restrict__ pe_in = nullptr,
                                                      u32 rowbits = 32)
{
    const u32 rowmask = rowbits >= 32 ? 0xFFFFFFFFu : (1u << rowbits) - 1u;
    const u32 maxlen = pk_maxlen(rowbits);
    if ((unsorted != nullptr && *unsorted == 0) != IDENT) return;
    static_assert(!(IDENT && PAGED), "paged rows are never read in place");
    __shared__ u32 s_pg[RP_NPG];
    u32 pg_first = 0;
    // (the page id always comes from LDS: a choice between an LDS and a global pointer becomes a flat load with
    //  vmcnt(0) waits that serialise the row loads)
    auto row_at = [&](u64 i, u32, u64 rf) -> u64 {
        if (!PAGED) return i;
        const u32 x = (u32)(i - rf);
        const u32 pg = s_pg[(x >> pt.lgpg) - pg_first] - 1u;
        return ((u64)pg << pt.lgpg) + (x & ((1u << pt.lgpg) - 1u));
    };
    // (all threads; barriers inside) the page ids of routed rows [lo, c_hi) of region r; c_hi is cut back to what RP_NPG
    // pages hold (the caller then walks the rest of the region as another segment)
    auto pages_load = [&](u64 lo, u64 &c_hi, u32 r, u64 rf) {
        if (!PAGED) return;
        __syncthreads();
        pg_first = (u32)(lo - rf) >> pt.lgpg;
        const u64 lim = (rf + ((u64)(pg_first + RP_NPG) << pt.lgpg)) & ~63ull;   // (a cut falls between two 64-row granules)
        if (c_hi > lim) c_hi = lim;
        const u32 npg = ((u32)(c_hi - 1 - rf) >> pt.lgpg) - pg_first + 1u;
        if (threadIdx.x < npg) {
            u32 v = pt.ptab[(u64)r * pt.pstride + pg_first + threadIdx.x];
            // 0 = the partition never published this page (cannot happen once k_part_onepass has completed; it did in a
            // profiling build whose switch skipped the publication, and the page "0 - 1" then was a wild address: round 2's
            // fault).  Read page 0 instead and tell the host.
            if (v == 0u) v = 1u;                                    // (this kernel has no error word in reach: stay in bounds)
            s_pg[threadIdx.x] = v;
        }
        __syncthreads();
    };
    auto row_se = [&](u64 i) -> u64 {
        if (IDENT) return (u64)(u32)((const i32 *)rows_a)[i] | ((u64)(u32)((const i32 *)rows_b)[i] << 32);
        return ((const u64 *)rows_a)[i];
    };
    auto row_id = [&](u64 i, u64 at) -> u32 { return IDENT ? (u32)i : ((const u32 *)rows_b)[at * prow_stride]; };
    __shared__ unsigned short s_off[RP_CCAP];
    __shared__ u64 s_ent[RP_ECAP];
    __shared__ u32 s_row[RP_ECAP];
    __shared__ u32 s_rfirst[IVX_MAXREG_WIDE + 2];
    ProbeLds L{s_off, s_ent, s_row, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const u32 wv = threadIdx.x / IVX_WAVE, ln = lane_id();
    const u32 nreg = ix.hdr[HDR_NREG];
    const bool rf_lds = nreg <= IVX_MAXREG_WIDE;
    if (rf_lds) for (u32 t = threadIdx.x; t <= nreg; t += RP_T) s_rfirst[t] = offs[(u64)t * nblk];
    __syncthreads();
    auto rfirst = [&](u32 r) -> u32 { return rf_lds ? s_rfirst[r] : offs[(u64)r * nblk]; };
    const u64 total_rows = rfirst(nreg);
    const u32 nvb = gridDim.x, vb = blockIdx.x;
    u64 lo = (total_rows * vb / nvb) & ~63ull;
    const u64 hi = vb + 1 == nvb ? total_rows : ((total_rows * (vb + 1) / nvb) & ~63ull);
    if (lo >= hi) return;
    Slice S;
    slice_init(ix, S, L);
    u32 r;
    { u32 a = 0, b = nreg; while (a < b) { const u32 m = (a + b + 1) >> 1; if (rfirst(m) <= lo) a = m; else b = m - 1; } r = a; }
    for (; lo < hi; r++) {
        const u64 rend = rfirst(r + 1);
        u64 c_hi = hi < rend ? hi : rend;
        if (c_hi <= lo) continue;
        u64 g = (lo >> 6) + wv;
        // the first granule's rows are in flight while the slice loads
        u64 nx = 0; u32 nxr = 0;
        const u64 rf = PAGED ? rfirst(r) : 0;
        pages_load(lo, c_hi, r, rf);
        const u64 g1 = (c_hi + 63) >> 6;
        { const u64 i = g * 64 + ln; const bool ok = g < g1 && i >= lo && i < c_hi; const u64 at = ok ? row_at(i, r, rf) : 0; nx = ok ? row_se(at) : 0; nxr = (PASS == 1 && !PK && ok) ? row_id(i, at) : 0u; }
        slice_load(ix, S, L, r, true);
        for (; g < g1; g += RP_W) {
            const u64 i = g * 64 + ln;
            const bool ok = i >= lo && i < c_hi;
            i32 qs = (i32)(u32)nx, qe = (i32)(u32)(nx >> 32);
            u32 rowv = nxr;
            if (PK) {
                const PkRow w = pk_unpack(nx, rowbits);
                rowv = w.hi & rowmask;
                qs = (i32)((u32)S.rbase + w.rel); qe = (i32)((u32)qs + w.len);
                if (ok && w.len == maxlen) { qs = ps_in[rowv]; qe = pe_in[rowv]; }
            }
            { const u64 g2 = g + RP_W; const u64 i2 = g2 * 64 + ln; const bool ok2 = g2 < g1 && i2 >= lo && i2 < c_hi; const u64 at = ok2 ? row_at(i2, r, rf) : 0; nx = ok2 ? row_se(at) : 0; nxr = (PASS == 1 && !PK && ok2) ? row_id(i2, at) : 0u; }
            const u64 slot = g + r;
            if (PASS == 0) {
                u32 c = 0;
                if (ok) probe_row(S, qs, qe, [&](u32, bool, i32, i32) { c++; });
                const u64 tot = wave_sum((u64)c);
                if (ln == 0) pcount[slot] = tot;
                continue;
            }
            // (scanned) the piece's pairs go to [base, base + its count); everything below is relative to it, in 32 bits
            const u64 base = __builtin_amdgcn_readfirstlane((u32)pcount[slot]) | ((u64)__builtin_amdgcn_readfirstlane((u32)(pcount[slot] >> 32)) << 32);
            u32 *const obp = ob + base, *const opp = op + base;
            const u64 room = cap > base ? cap - base : 0;
            const u32 lim = room > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)room;   // pairs of this piece the caller's buffers still hold
            u32 cnt = 0;                                                // pairs of the piece written so far (wavefront-uniform)
            // lock-step walk of one candidate list per lane: [ja, jb) of the staged slice or of the index in HBM
            // (four candidates per lane are fetched before any of them is tested: the steps are otherwise one LDS round
            // trip each, with nothing else in flight)
            auto walk = [&](u32 ja, u32 jb, bool lds) {
                constexpr int U = 4;
                while (__any(ja < jb)) {
                    i32 cs_[U], ce_[U]; u32 cr_[U]; bool v[U];
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        v[u] = ja + u < jb;
                        cs_[u] = 0; ce_[u] = 0; cr_[u] = 0;
                        if (v[u]) {
                            if (lds) { const u64 x = S.s_ent[ja + u]; cs_[u] = (i32)(u32)x; ce_[u] = (i32)(u32)(x >> 32); cr_[u] = S.s_row[ja + u]; }
                            else { const ivx_ent x = ix.ent[ja + u]; cs_[u] = x.s; ce_[u] = x.e; cr_[u] = x.row; }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const bool hit = v[u] && cs_[u] <= qe && ce_[u] >= qs;
                        const u64 m = __ballot(hit);
                        const u32 pos = cnt + mask_rank(m);
                        if (hit && pos < lim) { obp[pos] = cr_[u]; opp[pos] = rowv; }
                        cnt += (u32)__popcll(m);
                    }
                    ja = jb - ja > U ? ja + U : jb;
                }
            };
            const i64 hi64 = (i64)qe - (i64)S.origin;
            const bool live = ok && hi64 >= 0;
            {   // level 0
                u32 ja = 0, jb = 0; bool lds = false;
                if (live && S.lev0) {
                    const u32 ncell = S.ncell0;
                    const i64 lo64 = (i64)qs - ((i64)1 << S.sh0) + 1 - (i64)S.origin;
                    const i64 bl = lo64 <= 0 ? 0 : (lo64 >> S.sh0);
                    if (bl < (i64)ncell) {
                        const u32 blo = (u32)bl;
                        const i64 bh = hi64 >> S.sh0;
                        const u32 bhi = bh >= (i64)ncell ? ncell - 1u : (u32)bh;
                        if (blo <= bhi) {
                            lds = S.inlds && blo >= S.slo && bhi < S.shi;
                            if (lds) { ja = S.s_off[blo - S.slo]; jb = S.s_off[bhi + 1 - S.slo]; }
                            else { ja = ix.binstart[S.lb + blo]; jb = ix.binstart[S.lb + bhi + 1]; }
                        }
                    }
                }
                // lanes of one wavefront may differ in where their list lives (a row reaching past the slice): two rounds
                const u32 la = lds ? ja : 0u, lb = lds ? jb : 0u, ga = lds ? 0u : ja, gb = lds ? 0u : jb;
                walk(la, lb, true);
                if (__any(ga < gb)) walk(ga, gb, false);
            }
            if (S.upper) {
                for (u32 l = 1; l < S.nlev; l++) {
                    if (ix.hdr[HDR_LEVCNT + l] == 0) continue;
                    const u32 sh = S.sh0 + IVX_LSTEP * l;
                    u32 ja = 0, jb = 0;
                    if (live) {
                        u32 blo = 0, bhi = 0; bool any = true;
                        if (sh < 32) {
                            const u32 ncell = (S.span >> sh) + 1u;
                            const i64 lo64 = (i64)qs - ((i64)1 << sh) + 1 - (i64)S.origin;
                            const i64 bl = lo64 <= 0 ? 0 : (lo64 >> sh);
                            const i64 bh = hi64 >> sh;
                            if (bl >= (i64)ncell) any = false;
                            else { blo = (u32)bl; bhi = bh >= (i64)ncell ? ncell - 1u : (u32)bh; if (blo > bhi) any = false; }
                        }
                        if (any) { const u32 lbase = ix.lbase[(u64)l * ix.nkeys + S.k]; ja = ix.binstart[lbase + blo]; jb = ix.binstart[lbase + bhi + 1]; }
                    }
                    if (__any(ja < jb)) walk(ja, jb, false);
                }
            }
        }
        lo = c_hi;
        if (PAGED && lo < hi && lo < rend) r--;                       // cut at the page window: same region again
    }
}

// ------------------------------------------------------------------ host side
// The IVX_* settings of the region probe (each selects a path that is also the product path for some index; tests and A/B
// runs pin every form with them).  Read once per call, not per process: the tests change the environment between calls.
struct RegionKnobs {
    bool two_pass;          // IVX_PART=two: the flat two-pass partition instead of region pages
    bool pack_off;          // IVX_PACK=0: 12-byte routed rows ((start,end) + row id) instead of packed 8-byte words
    bool lean_off;          // IVX_FILL=old: the general kernel where the lean one would do
    bool filter_off;        // IVX_FILTER=0: route every row, whatever the build side's occupancy bitmap says
    const char *dense;      // IVX_DENSE=0/1: the match-dense fill never / always
    const char *rp_rows;    // IVX_RP_ROWS=1/2/4/8: rows per lane of the fill (experiments)
    const char *fill_drain; // IVX_FILL_DRAIN=n: the lean fill ends a row group's walk at n active lanes, whatever the rows per lane (0: never)
};
RegionKnobs region_knobs()
{
    auto is = [](const char *name, const char *v) { const char *x = getenv(name); return x && !strcmp(x, v); };
    return RegionKnobs{is("IVX_PART", "two"), is("IVX_PACK", "0"), is("IVX_FILL", "old"), is("IVX_FILTER", "0"), getenv("IVX_DENSE"), getenv("IVX_RP_ROWS"), getenv("IVX_FILL_DRAIN")};
}

// fill pass: rows per lane and batch from the expected matches per row (cap / n: callers size the output from the count
// pass): two consecutive rounds of a wavefront must fit its 512-pair staging ring, else the batch takes the slow direct path
int fill_rows_per_lane(const RegionKnobs &K, u64 cap, u64 n)
{
    if (K.rp_rows) return atoi(K.rp_rows);
    const double per_row = (double)cap / (double)n;
    // (a round's pairs must fit half a staging ring: 64 * rows per lane * pairs per row <= ~205 of its 256, four sigma below it)
    return per_row <= 0.40 ? 8 : per_row <= 0.8 ? 4 : per_row <= 1.6 ? 2 : 1;
}

// lean fill: the active lanes at which a 64-row group's walk ends and leaves its tails to the batch's tail pass (k_fill_fast's
// `drain`; 0: the plain walk, the kernel without a stash), by rows per lane.  Measured (profiles/fill_drain_ab.txt): 8 rows per
// lane gain from 4 to 12 alike, 4 rows per lane gain at 16 and not at 8, 2 rows per lane gain nothing beyond their own spread.
u32 fill_drain_of(const RegionKnobs &K, int b)
{
    if (K.fill_drain) { const int t = atoi(K.fill_drain); return t <= 0 ? 0u : (u32)t < RP_STASH ? (u32)t : RP_STASH; }
    return b == 8 ? 12u : b == 4 ? 16u : 0u;
}

bool dense_fill_wanted(const RegionKnobs &K, u64 cap, u64 n)
{
    if (K.dense) return atoi(K.dense) != 0;                                // tests / experiments
    return (double)cap / (double)n > 3.5;                                  // measured crossover (tools/probe_only.py IVX_DENSE=0/1): the ring wins below
}

// may the lean kernels (k_fill_fast, k_lean) run on these routed rows: packed words in region pages that
// hold at least a chunk, and a rest list for the rows the packed form cannot carry (the routing pass made one: its `lean`
// option).  Whether the INDEX qualifies (`fast`) and IVX_FILL=old are each launcher's own to test.
bool lean_rows_ok(const ivx_routed &R)
{
    return R.form == IVX_ROWS_PAGED && R.packed && R.pt.lgpg >= 13 && R.rest_rows != nullptr;
}

// ... and the lean fill pair (k_fill_fast + k_fill_rest), which also wants the batch list
bool lean_fill_ok(const ivx_routed &R, const RegionKnobs &K) { return lean_rows_ok(R) && !K.lean_off && R.rest != nullptr; }

// The shared opening of the launchers that have the lean form only (marks, aggregates, select): may the lean kernels run on
// this index under these settings -- the form ivx_rowval_probe_regions runs k_lean on -- and if so, route the rows.  *ok =
// false: the index, the settings or the routed rows do not qualify, and nothing else was taken or launched.
ivx_status lean_route(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, const u32 *key, const i32 *s, const i32 *e, u64 n,
                      bool has_filter, bool pk24, bool fast, bool no_vtab, ivx_routed *R, bool *ok)
{
    *ok = false;
    const RegionKnobs K = region_knobs();
    if (n == 0 || nreg == 0 || nreg > IVX_MAXREG || !pk24 || !fast || K.two_pass || K.pack_off || K.lean_off) return IVX_OK;
    IVX_TRY(ivx_route_paged(ctx, jv, nreg, key, s, e, n, ivx_paged_opts{has_filter && !K.filter_off, true, true, true, 0u, nullptr, false, no_vtab}, R));
    *ok = lean_rows_ok(*R);
    return IVX_OK;
}

// k_lean values the routed rows, k_lean_rest the few the packed form cannot carry (s, e: the input columns, for the escapes)
template <int B, class Op>
void lean_launch(hipStream_t st, const JoinIndexView &jv, const ivx_routed &R, const i32 *s, const i32 *e, const Op &op)
{
    typename Op::W *pool = const_cast<u64 *>(R.se);
    hipLaunchKernelGGL((k_lean<B, Op>), dim3(RP_GRID * (IVX_RV_WPS / 4)), dim3(RP_T), 0, st, jv, pool, (const u32 *)R.ctl->rcur, (const u32 *)R.ctl->cfirst, R.pt, R.rowbits,
                       R.rest_rows, R.ctl->rest_n, op);
    hipLaunchKernelGGL((k_lean_rest<Op>), dim3(256), dim3(256), 0, st, jv, pool, R.pt, (const u64 *)R.rest_rows, (const u32 *)R.ctl->rest_n, s, e, R.rowbits, op);
}

// The operators' records: arrays with a cell per word of the page pool (ivx_route_paged's own size of it), cell_bytes in all,
// out of one scratch buffer.  take(p, wanted) gives p the next array if the output is wanted; 8-byte arrays first.
struct RecCarve {
    u8 *buf = nullptr; u64 cells = 0;
    ivx_status reserve(ivx_ctx *ctx, const ivx_routed &R, u32 nreg, u64 n, size_t cell_bytes)
    {
        cells = ((n >> R.pt.lgpg) + nreg + 1) << R.pt.lgpg;
        return ctx->get_scratch(WS_T4, (size_t)cells * cell_bytes, (void **)&buf);
    }
    template <class T> void take(T *&p, const void *wanted)
    {
        if (!wanted) return;
        p = reinterpret_cast<T *>(buf);
        buf += cells * sizeof(T);
    }
};

template <int V> using int_tag = std::integral_constant<int, V>;
// rows per lane in {1, 2, 4, 8} as a template argument: f(int_tag<B>)
template <class F> void with_rows_per_lane(int b, F &&f)
{
    switch (b) { case 1: f(int_tag<1>{}); break; case 2: f(int_tag<2>{}); break; case 4: f(int_tag<4>{}); break; default: f(int_tag<8>{}); }
}

// k_probe_regions over any row form.  grid: RP_VGRID (count, per-row values: one row share per workgroup) or RP_GRID (fill).
// FLAT / TABLE: both IDENT instantiations are launched; the one whose case does not apply returns at once (the host never
// waits for the `unsorted` flag).  Per-row values over pages come as packed rows only (the value replaces half of the word).
template <int MODE, int B>
void launch_probe_regions(hipStream_t st, const JoinIndexView &jv, const ivx_routed &R, u32 grid, u32 *ob, u32 *op, u64 cap,
                          unsigned long long *cur, const u32 *bsel = nullptr, const u32 *only_if_set = nullptr)
{
    const u32 vpb = RP_VGRID / grid;
    if (R.form == IVX_ROWS_PAGED) {
        auto go = [&](auto pk) {
            hipLaunchKernelGGL((k_probe_regions<MODE, B, false, true, IVX_B(pk)>), dim3(grid), dim3(RP_T), 0, st, jv, (const void *)R.se, (const void *)R.ids, R.rfirst, 1u, vpb,
                               ob, op, cap, cur, 1u, R.adj, (const u32 *)nullptr, R.pt, bsel, R.ds, R.de, R.rowbits, only_if_set);
        };
        if constexpr (MODE >= RV_COUNT) go(std::true_type{}); else with_bools(go, R.packed);
        return;
    }
    hipLaunchKernelGGL((k_probe_regions<MODE, B, false>), dim3(grid), dim3(RP_T), 0, st, jv, (const void *)R.se, (const void *)R.ids, R.rfirst, R.nblk, vpb, ob, op, cap, cur, 1u, R.adj, R.unsorted);
    hipLaunchKernelGGL((k_probe_regions<MODE, B, true>), dim3(grid), dim3(RP_T), 0, st, jv, (const void *)R.ds, (const void *)R.de, R.rfirst, R.nblk, vpb, ob, op, cap, cur, 1u, R.adj, R.unsorted);
}

// match-dense fill (k_probe_dense): count the pieces, scan, write
ivx_status dense_fill(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, const ivx_routed &R, u64 n, u32 *ob, u32 *op, u64 cap, u64 *d_cursor)
{
    hipStream_t st = ctx->stream;
    const u64 slots = (n >> 6) + nreg + 3;
    u64 *pcount;
    IVX_TRY(ctx->get_scratch(WS_T3, slots * sizeof(u64), (void **)&pcount));
    IVX_HIP(ctx, hipMemsetAsync(pcount, 0, slots * sizeof(u64), st));
    auto pass = [&](auto pass_tag) {
        constexpr int P = decltype(pass_tag)::value;
        if (R.form == IVX_ROWS_PAGED) {
            with_bools([&](auto pk) {
                hipLaunchKernelGGL((k_probe_dense<P, false, true, IVX_B(pk)>), dim3(RP_VGRID), dim3(RP_T), 0, st, jv, (const void *)R.se, (const void *)R.ids, R.rfirst, 1u, 1u,
                                   (const u32 *)nullptr, pcount, ob, op, cap, R.pt, R.ds, R.de, R.rowbits);
            }, R.packed);
            return;
        }
        hipLaunchKernelGGL((k_probe_dense<P, false>), dim3(RP_VGRID), dim3(RP_T), 0, st, jv, (const void *)R.se, (const void *)R.ids, R.rfirst, R.nblk, 1u, R.unsorted, pcount, ob, op, cap);
        hipLaunchKernelGGL((k_probe_dense<P, true>), dim3(RP_VGRID), dim3(RP_T), 0, st, jv, (const void *)R.ds, (const void *)R.de, R.rfirst, R.nblk, 1u, R.unsorted, pcount, ob, op, cap);
    };
    pass(int_tag<0>{});
    IVX_TRY(ivx_scan_exclusive_u64(ctx, pcount, slots));
    IVX_HIP(ctx, hipMemcpyAsync(d_cursor, pcount + (slots - 1), sizeof(u64), hipMemcpyDeviceToDevice, st));   // the pair total
    pass(int_tag<1>{});
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}

// COUNT / FILL over routed rows of any form.  hint: the pairs to expect (how dense the matches are); fast: 0 no, 1 every
// region is one LDS-resident level, 2 the kernels test hdr[HDR_SLOW] themselves; reused: R served an earlier fill already
ivx_status probe_pairs(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, int mode, const ivx_routed &R, u64 n, u32 *ob, u32 *op, u64 cap,
                       u64 *d_cursor, u64 hint, int fast, bool reused, const RegionKnobs &K, ivx_probe_note *note)
{
    hipStream_t st = ctx->stream;
    unsigned long long *cur = (unsigned long long *)d_cursor;
    // R.tables_due: the routing pass left rfirst / cfirst to whoever reads them.  Everything below but the lean pair does:
    // each such way calls tables() before its first launch (k_chunk_bounds reads only rcur, final behind the partition)
    bool due = R.tables_due;
    auto tables = [&]() -> ivx_status { if (due) { due = false; return ivx_route_paged_bounds(ctx, R, nreg); } return IVX_OK; };
    if (mode != JP_FILL) {
        IVX_TRY(tables());
        launch_probe_regions<0, RP_B>(st, jv, R, RP_VGRID, ob, op, cap, cur);
        IVX_HIP(ctx, hipGetLastError());
        return IVX_OK;
    }
    // (the rows the probe walks are the routed ones: the density hint is pairs per INPUT row, as the caller sized it)
    if (dense_fill_wanted(K, hint, n)) { IVX_TRY(tables()); return dense_fill(ctx, jv, nreg, R, n, ob, op, cap, d_cursor); }
    // single walk: pairs staged per wavefront, one output reservation per workgroup and round.  Rows per lane follow from the
    // pairs per ROUTED row: known here when every row was routed; with the occupancy bitmap in use the count sits on the
    // device, k_pick_rows decides there and every variant is launched (three exit)
    const bool paged = R.form == IVX_ROWS_PAGED;
    u32 *bsel = paged && !R.all_routed ? ctx->dword<u32>(SC_BSEL) : nullptr;
    if (bsel) IVX_TRY(tables());
    if (bsel) hipLaunchKernelGGL(k_pick_rows, dim3(1), dim3(1), 0, st, R.rfirst, nreg, hint, K.rp_rows ? (u32)atoi(K.rp_rows) : 0u, bsel);
    auto every_b = [&](auto &&f) {
        if (bsel) { f(int_tag<8>{}); f(int_tag<4>{}); f(int_tag<2>{}); f(int_tag<1>{}); }
        else with_rows_per_lane(fill_rows_per_lane(K, hint, n), f);
    };
    // packed rows over an index whose every region is one LDS-resident level: the lean kernel, then whatever batches it
    // left to the generic walk (IVX_FILL=old: the general kernel, for A/B runs and the tests that pin both)
    const u32 *slow_gate = nullptr;
    if (fast != 0 && lean_fill_ok(R, K)) {
        u32 *rest_n = R.ctl->rest_n;                                    // batches, rows
        static_assert(offsetof(ivx_route_ctl, fill_done) == offsetof(ivx_route_ctl, rest_n) + 2 * sizeof(u32), "one memset clears the rest counts and the done-counter");
        if (reused) IVX_HIP(ctx, hipMemsetAsync(rest_n, 0, 3 * sizeof(u32), st));   // (else: zeroed with the routing pass's counters just now)
        // fast == 1: the lean pair is all this call runs, and k_fill_rest leaves the totals on the host itself
        const bool publish = fast == 1 && note != nullptr && ctx->hd_scalars != nullptr;
        every_b([&](auto b) {
            const u32 drain = fill_drain_of(K, decltype(b)::value);
            with_bools([&](auto dr) {
                hipLaunchKernelGGL((k_fill_fast<decltype(b)::value, IVX_B(dr)>), dim3(RP_GRID), dim3(RP_T), 0, st, jv, R.se, (const u32 *)R.ctl->rcur, R.pt, ob, op, cap, cur,
                                   (const u32 *)bsel, R.rowbits, R.rest, R.rest_rows, rest_n, drain);
            }, drain != 0);
        });
        hipLaunchKernelGGL(k_fill_rest, dim3(512), dim3(256), 0, st, jv, R.se, R.pt, (const FpRest *)R.rest, (const u64 *)R.rest_rows, (const u32 *)rest_n, ob, op, cap, cur, R.ds, R.de, R.rowbits,
                           &R.ctl->fill_done, publish ? ctx->hdword(SC_PAIRS) : (u64 *)nullptr);
        IVX_HIP(ctx, hipGetLastError());
        if (publish) note->totals_on_host = true;
        if (fast == 1) return IVX_OK;
        // fast == 2: whether every region is one LDS-resident level is known on the device only (the index's build
        // tail set hdr[HDR_SLOW] after the host had its copy): k_fill_fast has left at once if not, and the
        // general kernel below leaves at once if so
        slow_gate = jv.hdr + HDR_SLOW;
    }
    IVX_TRY(tables());
    every_b([&](auto b) { launch_probe_regions<1, decltype(b)::value>(st, jv, R, RP_GRID, ob, op, cap, cur, bsel, slow_gate); });
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}

}  // namespace

ivx_status ivx_join_probe_regions(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, int mode,
                                  const u32 *key, const i32 *s, const i32 *e, u64 n,
                                  u32 *ob, u32 *op, u64 cap, u64 *d_cursor, bool planned, bool has_filter, bool pk24, int fast, hipEvent_t ready, bool clear_cursor,
                                  ivx_probe_note *note)
{
    // `ready` (an index whose build tail may still run on another stream): the routing pass reads only what was final
    // before that tail started; the probe kernels come behind the event
    auto wait_ready = [&]() -> ivx_status { if (ready) { IVX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ready, 0)); ready = nullptr; } return IVX_OK; };
    // clear_cursor: d_cursor[0..1] (pair cursor, fault flags) are not zeroed yet -- the one-pass routing clears them with its
    // own counters; every other way through here does it now
    const RegionKnobs K = region_knobs();
    const bool paged_route = !planned && n != 0 && nreg <= IVX_MAXREG_WIDE && !K.two_pass;
    if (clear_cursor && !paged_route) IVX_HIP(ctx, hipMemsetAsync(d_cursor, 0, 2 * sizeof(u64), ctx->stream));
    if (n == 0) return wait_ready();
    ivx_join_plan &pl = ctx->join_plan;
    ivx_routed R;
    if (planned) R = pl.rows;               // routed by the count call that sized this fill call (which left `unsorted` as it is)
    else {
        if (nreg > IVX_MAXREG_WIDE) {
            IVX_TRY(wait_ready());
            IVX_TRY(ivx_route_two_level(ctx, jv, nreg, key, s, e, n, &R));
        } else if (K.two_pass) {            // (A/B measurements and the tests that pin both)
            IVX_TRY(wait_ready());          // (its histogram kernel may leave the rows in place: no overlap with the build tail here)
            IVX_TRY(ivx_route_flat(ctx, jv, key, s, e, n, 0u, nreg > IVX_MAXREG ? 1024u : 256u, false, 4, &R));
        } else {
            // 8-byte routed rows whenever a region's coordinates fit 24 bits
            // a fill whose every row is routed may run the lean pair alone, which reads neither rfirst nor the chunk table
            // (k_fill_fast scans the regions' row counts itself): probe_pairs queues k_chunk_bounds where it turns out otherwise
            const bool bounds_due = mode == JP_FILL && !(has_filter && !K.filter_off);
            IVX_TRY(ivx_route_paged(ctx, jv, nreg, key, s, e, n, ivx_paged_opts{has_filter && !K.filter_off, pk24 && !K.pack_off, false, fast != 0, 0u, clear_cursor ? d_cursor : nullptr, bounds_due}, &R));
            // fast == 2, an index whose build tail may still be running: hdr[HDR_SLOW] is that tail's last word.  The routing
            // pass is queued and keeps the device busy; the host waits for the tail here -- the probe kernels had to wait for
            // the same event -- and reads the word from the header mirror the tail's last kernel wrote it to, if that mirror
            // (this context's, one per context) still is this index's.  The call then launches the lean pair or the general
            // kernel, not both with the device choosing, and the index's later calls know.
            if (fast == 2 && ready != nullptr && note != nullptr && note->ix_serial != 0 && ctx->hdr_mirror_serial == note->ix_serial) {
                IVX_HIP(ctx, hipEventSynchronize(ready));
                fast = ctx->hword<u32>(SC_HDR_MIRROR)[HDR_SLOW] == 0 ? 1 : 0;
                note->fast = fast;
            }
        }
        if (mode == JP_COUNT) { pl.rows = R; pl.valid = true; }     // leave the routed rows for the fill call (ivx_capi.hip fills in whose they are)
    }
    IVX_TRY(wait_ready());
    // how dense the matches are: from the caller's capacity, or -- planned -- from what the count call found
    const u64 hint = ctx->fill_hint ? ctx->fill_hint : (planned && pl.total < cap ? pl.total : cap);
    return probe_pairs(ctx, jv, nreg, mode, R, n, ob, op, cap, d_cursor, hint, fast, planned, K, note);
}

// One value per probe row, in input order, through the region partition.  kind: IVX_RV_COUNT (count_overlaps,
// jv over the build rows, i64 out), IVX_RV_COVERAGE (jv over the merged nodes, i64 out), IVX_RV_PER_ROW (the
// join's rle_right: u32 out, *d_total += all matches), IVX_RV_EXISTS (semi / anti join: u8 out).
ivx_status ivx_rowval_probe_regions(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, int kind,
                                    const u32 *key, const i32 *s, const i32 *e, u64 n, int strict, void *out, u64 *d_total,
                                    bool has_filter, bool pk24, bool fast)
{
    if (n == 0) return IVX_OK;
    if (nreg == 0 || nreg > IVX_MAXREG_WIDE) return ctx->fail(IVX_ERR_INVALID, "per-row region probe: one partition pass only");
    hipStream_t st = ctx->stream;
    const RegionKnobs K = region_knobs();
    const u32 adj = strict ? 1u : 0u;
    // Packed rows in region pages (the join's one-pass partition, two 512-thread workgroups per CU) when the index allows
    // them and one 256-digit pass routes the rows: no histogram pass, the probe leaves each value in the row's own word,
    // the un-permute reads the words back through vtab.  (IVX_PART=two / IVX_PACK=0: the two-pass form.)
    const bool paged = pk24 && nreg <= IVX_MAXREG && !K.two_pass && !K.pack_off;
    ivx_routed R;
    u32 *val = nullptr;                     // flat rows: the values in routed order
    if (paged) IVX_TRY(ivx_route_paged(ctx, jv, nreg, key, s, e, n, ivx_paged_opts{has_filter && !K.filter_off, true, true, fast && !K.lean_off, adj}, &R));
    else {
        IVX_TRY(ivx_route_flat(ctx, jv, key, s, e, n, adj, nreg > IVX_MAXREG ? 1024u : 256u, true, 2, &R));
        IVX_TRY(ctx->get_scratch(WS_T2, n * sizeof(u32), (void **)&val));
    }
    u64 *pool = const_cast<u64 *>(R.se);
    auto probe = [&](auto kind_tag) {
        constexpr int M = decltype(kind_tag)::value;
        // every region one LDS-resident level: the lean pair (IVX_FILL=old: the general kernel)
        if (lean_rows_ok(R)) lean_launch<IVX_RV_B>(st, jv, R, s, e, RvOp<M>{{}, adj});
        else launch_probe_regions<M, RP_B>(st, jv, R, RP_VGRID, paged ? (u32 *)pool : val, nullptr, 0, nullptr);
    };
    if (kind == IVX_RV_COVERAGE) probe(int_tag<RV_COVERAGE>{}); else if (kind == IVX_RV_COUNT) probe(int_tag<RV_COUNT>{}); else probe(int_tag<RV_MATCHES>{});
    IVX_HIP(ctx, hipGetLastError());
    return ivx_unroute_values(ctx, R, nreg, kind, val, n, out, d_total);
}

// The build rows a big batch matched, ORed into `marks` (one bit per build row), through the region partition -- the lean
// form only: packed rows in region pages over an index whose every region is one LDS-resident level (lean_route).  *took =
// false (nothing launched) when the index or the settings do not qualify: the caller then runs the direct kernel
// (ivx_mark_probe) on its columns.  (*took means something on IVX_OK only.)
ivx_status ivx_mark_probe_regions(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, const u32 *key, const i32 *s, const i32 *e, u64 n,
                                  u32 *marks, bool has_filter, bool pk24, bool fast, bool *took, const WherePred *w)
{
    ivx_routed R;
    IVX_TRY(lean_route(ctx, jv, nreg, key, s, e, n, has_filter, pk24, fast, true, &R, took));       // (no un-permute: no vtab)
    if (!*took) return IVX_OK;
    with_where(w, MarkOp{{}, marks}, [&](const auto &op) { lean_launch<IVX_RV_B>(ctx->stream, jv, R, s, e, op); });
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}

// Per-row aggregates of `val` over each probe row's matches, through the region partition -- the lean form only, as
// ivx_mark_probe_regions: *took = false (nothing launched, no scratch taken) when the index or the settings do not qualify,
// and the caller runs the direct kernel (ivx_agg_probe).  The outputs are device columns in input order:
// ivx_unroute_records brings the records there and gives the rows the routing pass dropped the empty result.
ivx_status ivx_agg_probe_regions(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, const u32 *key, const i32 *s, const i32 *e, u64 n,
                                 const void *val, u32 val_bytes, const AggOut &out, bool has_filter, bool pk24, bool fast, bool *took,
                                 const WherePred *w)
{
    ivx_routed R;
    IVX_TRY(lean_route(ctx, jv, nreg, key, s, e, n, has_filter, pk24, fast, false, &R, took));
    if (!*took) return IVX_OK;
    const int n64 = (out.sum != nullptr) + (out.vmin != nullptr) + (out.vmax != nullptr) + (out.bases != nullptr) + (out.wsum != nullptr);
    RecCarve c;
    IVX_TRY(c.reserve(ctx, R, nreg, n, 8u * (size_t)n64 + (out.count ? 4u : 0u)));
    AggOut rec{};
    c.take(rec.sum, out.sum); c.take(rec.vmin, out.vmin); c.take(rec.vmax, out.vmax); c.take(rec.bases, out.bases); c.take(rec.wsum, out.wsum);
    c.take(rec.count, out.count);
    with_bools([&](auto wide, auto mm, auto wt) {
        with_where(w, AggOp<IVX_B(wide) ? 8 : 4, IVX_B(mm), IVX_B(wt)>{{}, val, rec}, [&](const auto &op) { lean_launch<IVX_AGG_B>(ctx->stream, jv, R, s, e, op); });
    }, val_bytes == 8, out.vmin || out.vmax, out.bases || out.wsum);
    IVX_HIP(ctx, hipGetLastError());
    return ivx_unroute_records(ctx, R, nreg, n, rec, out);
}

// Per probe row the best matching build row by `by` (and the criterion's value there), through the region partition -- the
// lean form only, with ivx_agg_probe_regions' eligibility and *took.  The outputs are device columns in input order:
// ivx_unroute_sel_records brings the records there and gives the rows the routing pass dropped (IVX_NULL_IDX, 0).
ivx_status ivx_sel_probe_regions(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, const u32 *key, const i32 *s, const i32 *e, u64 n,
                                 const void *val, u32 val_bytes, int by, const SelOut &out, bool has_filter, bool pk24, bool fast, bool *took,
                                 const WherePred *w)
{
    ivx_routed R;
    IVX_TRY(lean_route(ctx, jv, nreg, key, s, e, n, has_filter, pk24, fast, false, &R, took));
    if (!*took) return IVX_OK;
    RecCarve c;
    IVX_TRY(c.reserve(ctx, R, nreg, n, out.score ? 12u : 4u));
    SelOut rec{};
    c.take(rec.score, out.score); c.take(rec.idx, out.idx);
    sel_dispatch(by, val_bytes, out.score != nullptr, [&](auto b, auto vb, auto sc) {
        with_where(w, SelOp<decltype(b)::value, decltype(vb)::value, decltype(sc)::value>{{}, val, rec}, [&](const auto &op) { lean_launch<IVX_AGG_B>(ctx->stream, jv, R, s, e, op); });
    });
    IVX_HIP(ctx, hipGetLastError());
    return ivx_unroute_sel_records(ctx, R, nreg, n, rec, out);
}

// The match count per probe row under a threshold, through the region partition -- the lean form only, with
// ivx_mark_probe_regions' eligibility and *took.  RvOp<RV_MATCHES> behind the threshold leaves each count in the row's own
// word; the un-permute brings it to per_row -- adding the counts to *d_total on its way, if that is given -- or, per_row null,
// as "count != 0" to exists.
ivx_status ivx_match_probe_regions_where(ivx_ctx *ctx, const JoinIndexView &jv, u32 nreg, const u32 *key, const i32 *s, const i32 *e, u64 n,
                                         u32 *per_row, u8 *exists, u64 *d_total, bool has_filter, bool pk24, bool fast, bool *took, const WherePred &w)
{
    ivx_routed R;
    IVX_TRY(lean_route(ctx, jv, nreg, key, s, e, n, has_filter, pk24, fast, false, &R, took));
    if (!*took) return IVX_OK;
    lean_launch<IVX_RV_B>(ctx->stream, jv, R, s, e, WhereOp<RvOp<RV_MATCHES>>{RvOp<RV_MATCHES>{{}, 0u}, w});
    IVX_HIP(ctx, hipGetLastError());
    return ivx_unroute_values(ctx, R, nreg, per_row ? IVX_RV_PER_ROW : IVX_RV_EXISTS, nullptr, n, per_row ? (void *)per_row : (void *)exists, per_row ? d_total : nullptr);
}
