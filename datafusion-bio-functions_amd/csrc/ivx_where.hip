// ivx_where.hip -- overlap thresholds (include/ivx_where.h): what is not an operator behind WhereOp on an existing launcher
// (ivx_where.hpp; the marks, the aggregates and select take the threshold in their own files).
//
//   ivx_match_probe_where   the per-row match count under a threshold on the direct walk: MatchOut behind WhereOp on
//                           k_probe_rows.  (Big batches over a lean index: RvOp<RV_MATCHES> behind WhereOp on k_lean /
//                           k_lean_rest, ivx_regions_probe.hip.)
//   k_match_totals          the count entry's total: a device reduction of the per-row counts, and the exists bytes from them
//   k_pairs_count / _write  the stable pair filter, two passes over the same tiles:
//       a tile is PW_TILE = 1024 consecutive pairs of one 256-thread workgroup; wavefront v of it owns pairs
//       [256 v, 256 v + 256) as PW_PI = 4 groups of 64 CONSECUTIVE pairs, one per lane, so the loads of the two index
//       columns are coalesced; the four coordinates of a pair are gathers (the index columns are in no order).
//       COUNT  every pair: both indexes in range (else the call's flag is raised and nothing is gathered for the pair), the
//              four gathers, the predicate; a ballot per group, kept (one bit per pair); the tile's passes go to counts[tile].
//              An exclusive scan (ivx_scan_exclusive_u64) turns the counts into the tiles' output offsets and leaves the total
//              behind them.
//       WRITE  reads the ballots back instead of gathering again (the gathers are what the filter costs); a passing pair of
//              group g goes to tile offset + passes of the groups before + its rank in the group's ballot: input order,
//              whatever order the workgroups run in.
//       The host reads total and flag once between the passes: a bad index or a short buffer ends the call with nothing
//       written.
#include "ivx_where.hpp"

namespace {

constexpr int MT_T = 256;

__global__ __launch_bounds__(MT_T) void k_match_totals(const u32 *__restrict__ per_row, u64 n, u8 *__restrict__ exists, unsigned long long *total)
{
    __shared__ unsigned long long lds[MT_T / IVX_WAVE];
    unsigned long long s = 0;
    for (u64 i = (u64)blockIdx.x * MT_T + threadIdx.x; i < n; i += (u64)gridDim.x * MT_T) {
        const u32 c = per_row[i];
        s += c;
        if (exists) exists[i] = c != 0u;
    }
    const unsigned long long t = block_sum<unsigned long long, MT_T>(s, lds);
    if (threadIdx.x == 0 && total && t) atomicAdd(total, t);
}

struct PwTail { u64 total, bad; };      // behind the tile counts: the scan's total, the bad-index flag

// COUNT: the tile's passes to counts[tile], every group's ballot to masks (a word per 64 pairs: group g of wavefront v of tile
// t is word t * PW_TILE / 64 + v * PW_PI + g -- the pair's own 64-pair block), the flag raised for an index out of range
__global__ __launch_bounds__(PW_T) void k_pairs_count(const u32 *__restrict__ bidx, const u32 *__restrict__ pidx, u64 n,
                                                      const i32 *__restrict__ bs, const i32 *__restrict__ be, u64 nb,
                                                      const i32 *__restrict__ ps, const i32 *__restrict__ pe, u64 np, WherePred w,
                                                      u64 *__restrict__ counts, u64 *__restrict__ masks, u64 *bad)
{
    constexpr int NW = PW_T / IVX_WAVE;
    __shared__ u32 s_w[NW];
    const u32 ln = lane_id(), wv = threadIdx.x / IVX_WAVE;
    const u64 ntiles = (n + PW_TILE - 1) / PW_TILE;
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const u64 i0 = tile * PW_TILE + (u64)wv * (IVX_WAVE * PW_PI) + ln;
        u32 b[PW_PI], p[PW_PI];
        bool in[PW_PI];
        bool wild = false;
#pragma unroll
        for (int g = 0; g < PW_PI; g++) {
            const u64 i = i0 + (u64)g * IVX_WAVE;
            const bool ok = i < n;
            b[g] = ok ? bidx[i] : 0u;
            p[g] = ok ? pidx[i] : 0u;
            in[g] = ok && b[g] < nb && p[g] < np;                        // (IVX_NULL_IDX is never below a row count)
            wild |= ok && !in[g];
        }
        i32 xs[PW_PI], xe[PW_PI], qs[PW_PI], qe[PW_PI];                  // all sixteen gathers in flight before the first use
#pragma unroll
        for (int g = 0; g < PW_PI; g++) {
            xs[g] = in[g] ? bs[b[g]] : 0; xe[g] = in[g] ? be[b[g]] : 0;
            qs[g] = in[g] ? ps[p[g]] : 0; qe[g] = in[g] ? pe[p[g]] : 0;
        }
        u32 wtot = 0;
#pragma unroll
        for (int g = 0; g < PW_PI; g++) {
            const u64 m = __ballot(in[g] && w.pass(qs[g], qe[g], xs[g], xe[g]));
            wtot += (u32)__popcll(m);
            if (ln == 0) masks[tile * (PW_TILE / IVX_WAVE) + wv * PW_PI + g] = m;
        }
        if (wild) *bad = 1;
        if (ln == 0) s_w[wv] = wtot;
        __syncthreads();
        if (threadIdx.x == 0) {
            u32 t = 0;
#pragma unroll
            for (int v = 0; v < NW; v++) t += s_w[v];
            counts[tile] = t;
        }
        __syncthreads();                                                 // (s_w is written again in the next tile)
    }
}

// WRITE: nothing is gathered or tested again -- the ballots are read back.  A passing pair of group g goes to the tile's offset
// + the passes of the tile's groups before it (the tile's 16 mask words, which every lane reads) + its rank in its ballot
__global__ __launch_bounds__(PW_T) void k_pairs_write(const u32 *__restrict__ bidx, const u32 *__restrict__ pidx, u64 n,
                                                      const u64 *__restrict__ counts, const u64 *__restrict__ masks,
                                                      u32 *__restrict__ ob, u32 *__restrict__ op, u64 cap)
{
    constexpr u32 GPT = PW_TILE / IVX_WAVE;                              // groups (mask words) per tile
    const u32 ln = lane_id(), wv = threadIdx.x / IVX_WAVE;
    const u64 ntiles = (n + PW_TILE - 1) / PW_TILE;
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const u64 *tm = masks + tile * GPT;
        u64 at = counts[tile];
        for (u32 j = 0; j < wv * PW_PI; j++) at += (u32)__popcll(tm[j]);
        const u64 i0 = tile * PW_TILE + (u64)wv * (IVX_WAVE * PW_PI) + ln;
#pragma unroll
        for (int g = 0; g < PW_PI; g++) {
            const u64 m = tm[wv * PW_PI + g];
            const u64 i = i0 + (u64)g * IVX_WAVE;
            const u64 mine = at + (u32)__popcll(m & ((1ull << ln) - 1ull));
            if (((m >> ln) & 1ull) && i < n && mine < cap) { ob[mine] = bidx[i]; op[mine] = pidx[i]; }
            at += (u32)__popcll(m);
        }
    }
}

}  // namespace

ivx_status ivx_match_probe_where(ivx_ctx *ctx, const JoinIndexView &jv, const u32 *key, const i32 *s, const i32 *e, u64 n,
                                 u32 *per_row, u8 *exists, const WherePred &w)
{
    return ivx_direct_probe(ctx, jv, key, s, e, n, WhereOp<MatchOut>{MatchOut{{}, per_row, exists}, w});
}

ivx_status ivx_match_totals(ivx_ctx *ctx, const u32 *per_row, u64 n, u8 *exists, u64 *d_total)
{
    if (n == 0) return IVX_OK;
    hipLaunchKernelGGL(k_match_totals, dim3(ivx_stream_grid(n, MT_T * 8, 256 * 8)), dim3(MT_T), 0, ctx->stream, per_row, n, exists, (unsigned long long *)d_total);
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}

ivx_status ivx_pairs_where_device(ivx_ctx *ctx, const u32 *bidx, const u32 *pidx, u64 n_pairs, const i32 *bs, const i32 *be, u64 nb,
                                  const i32 *ps, const i32 *pe, u64 np, const WherePred &w, u32 *ob, u32 *op, u64 cap, u64 *n_out)
{
    *n_out = 0;
    if (n_pairs == 0) return IVX_OK;
    hipStream_t st = ctx->stream;
    const u64 ntiles = (n_pairs + PW_TILE - 1) / PW_TILE;
    const u32 grid = ivx_stream_grid(n_pairs, PW_TILE, 256 * 16);
    u64 *counts, *masks;
    IVX_TRY(ctx->get_scratch(WS_T5, (size_t)(ntiles + 2) * sizeof(u64), (void **)&counts));
    IVX_TRY(ctx->get_scratch(WS_T6, (size_t)ntiles * (PW_TILE / IVX_WAVE) * sizeof(u64), (void **)&masks));
    IVX_HIP(ctx, hipMemsetAsync(counts + ntiles, 0, sizeof(PwTail), st));
    hipLaunchKernelGGL(k_pairs_count, dim3(grid), dim3(PW_T), 0, st, bidx, pidx, n_pairs, bs, be, nb, ps, pe, np, w, counts, masks, counts + ntiles + 1);
    IVX_HIP(ctx, hipGetLastError());
    IVX_TRY(ivx_scan_exclusive_u64(ctx, counts, ntiles + 1));          // counts[ntiles] = the total
    PwTail tail;
    IVX_TRY(ctx->fetch_wait((const PwTail *)(counts + ntiles), st, &tail));
    if (tail.bad) return ctx->fail(IVX_ERR_INVALID, "pairs_where: index out of bounds");
    *n_out = tail.total;
    if (ob == nullptr && cap == 0) return IVX_OK;
    if (tail.total > cap) return ctx->fail(IVX_ERR_CAPACITY, "pairs_where: output buffers too small");
    if (tail.total == 0) return IVX_OK;
    hipLaunchKernelGGL(k_pairs_write, dim3(grid), dim3(PW_T), 0, st, bidx, pidx, n_pairs, (const u64 *)counts, (const u64 *)masks, ob, op, cap);
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}
