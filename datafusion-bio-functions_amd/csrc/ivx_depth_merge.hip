// ivx_depth_merge.hip -- streaming depth(): two depth profiles added on the device, and the coverage blocks of a profile
// (the reference's accumulate_partition / merge_dense_results / merge_sparse_results: bio-function-pileup
// physical_exec.rs:269-329, :367-463; the blocks: coverage.rs:38-62 restated on steps).
//
//   merge     Coverage is additive, so the profile of the union of two inputs is the merge of their two sorted step lists:
//             no events, no sort.  With w = key << 32 | pos, the virtual merged sequence holds every step of A and of B, A
//             before B at equal w.  k_merge_partition cuts it into tiles of DEPTH_MERGE_TILE elements (a search along each
//             tile's diagonal); k_merge_tile stages a tile's A and B slices in LDS and every thread merges MI consecutive
//             elements of it serially.  The merge itself gives each element its four ranks (#A < w, #A <= w, #B < w,
//             #B <= w), and the coverage at a rank is one lookup: the step before it, if that step has the element's key.
//             The slices are staged with the step before each and the element just past each, which are the carry-in and
//             the tie partner when a tile boundary splits them: no running state crosses a tile.  A B element with a tied
//             A element is dropped (the A element speaks for both); any other element is a step iff c != prev.
//   passes    count per tile, exclusive scan of the counts, one read-back of the total, then the same kernel again compacts
//             the tile in LDS and stores it in merge order, contiguous per tile.
//   blocks    step i gives (key_i, p_i, p_(i+1) - 1, c_i) iff c_i != 0 and step i + 1 has the same key: a counting scan,
//             run once to size and once to write.
#include "ivx_device.hpp"
#include "ivx_scan.hpp"

namespace {

constexpr int DEPTH_MERGE_TILE = 2048;          // merged elements per workgroup; the LDS image is 24 KiB: 6 workgroups fit a CU's 160 KiB
constexpr int MT = 256;                         // threads
constexpr int MI = DEPTH_MERGE_TILE / MT;       // consecutive merged elements per thread
static_assert(DEPTH_MERGE_TILE % MT == 0 && MT == ivxscan::T_, "whole elements per thread; the scan's workgroup size");

constexpr int KT = 256;

struct CntScan {
    using T = u32;
    __host__ __device__ static T identity() { return 0u; }
    __device__ static T combine(const T &a, const T &b) { return a + b; }
    __device__ static T shfl_up(const T &v, int d) { return __shfl_up(v, d, IVX_WAVE); }
};

__device__ __forceinline__ u64 step_w(const u32 *__restrict__ key, const u32 *__restrict__ pos, u64 i) { return ((u64)key[i] << 32) | pos[i]; }

// part[t] = steps of A among the first min(t * TILE, N) elements of the merged sequence, t <= ntiles
__global__ __launch_bounds__(KT) void k_merge_partition(const u32 *__restrict__ ak, const u32 *__restrict__ ap, u32 sa,
                                                        const u32 *__restrict__ bk, const u32 *__restrict__ bp, u32 sb,
                                                        u32 ntiles, u32 *__restrict__ part)
{
    const u64 t = (u64)blockIdx.x * KT + threadIdx.x;
    if (t > ntiles) return;
    const u64 N = (u64)sa + sb;
    u64 d = t * DEPTH_MERGE_TILE;
    if (d > N) d = N;
    u64 lo = d > sb ? d - sb : 0, hi = d < sa ? d : sa;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);                  // mid < sa, d - 1 - mid < sb
        if (step_w(ak, ap, mid) <= step_w(bk, bp, d - 1 - mid)) lo = mid + 1; else hi = mid;
    }
    part[t] = (u32)lo;
}

// key_seen of the result: the OR, a missing key counting as 0
__global__ __launch_bounds__(KT) void k_seen_or(const u8 *__restrict__ sa, u32 nka, const u8 *__restrict__ sb, u32 nkb, u32 nk, u8 *__restrict__ out)
{
    const u64 k = (u64)blockIdx.x * KT + threadIdx.x;
    if (k >= nk) return;
    u8 v = 0;
    if (k < nka) v |= sa[k];
    if (k < nkb) v |= sb[k];
    out[k] = v;
}

// WRITE = false: cnt[tile] = steps the tile gives (and cnt[ntiles] = 0, the slot the scan turns into the total).
// WRITE = true: cnt holds the scanned counts; the tile's steps go to ok / op / oc from cnt[tile] on.
template <bool WRITE>
__global__ __launch_bounds__(MT) void k_merge_tile(DepthProfileView A, DepthProfileView B, const u32 *__restrict__ part, u32 ntiles,
                                                   u32 *__restrict__ cnt, u32 *__restrict__ ok, u32 *__restrict__ op, i32 *__restrict__ oc)
{
    constexpr int T = DEPTH_MERGE_TILE;
    // A's slice with the step before it and the one past it at [0, na + 2), B's likewise at [na + 2, na + nb + 4)
    __shared__ u64 sw[T + 4];
    __shared__ u32 sc[T + 4];
    __shared__ u32 red[MT / IVX_WAVE + 1];
    const u32 t = threadIdx.x, tile = blockIdx.x;
    const u64 N = A.steps + B.steps;
    const u64 d_lo = (u64)tile * T, d_hi = d_lo + T < N ? d_lo + T : N;
    const u32 a0 = part[tile], a1 = part[tile + 1];
    const u32 b0 = (u32)(d_lo - a0), b1 = (u32)(d_hi - a1);
    const u32 na = a1 - a0, nb = b1 - b0, nt = na + nb;     // nt <= T
    const u32 boff = na + 2;

    for (u32 i = t; i < na + 2; i += MT) {
        const i64 g = (i64)a0 + i - 1;
        const bool in = g >= 0 && (u64)g < A.steps;
        sw[i] = in ? step_w(A.key, A.pos, (u64)g) : ~0ull;          // (no key is 2^32 - 1: never a match)
        sc[i] = in ? (u32)A.cov[g] : 0u;
    }
    for (u32 i = t; i < nb + 2; i += MT) {
        const i64 g = (i64)b0 + i - 1;
        const bool in = g >= 0 && (u64)g < B.steps;
        sw[boff + i] = in ? step_w(B.key, B.pos, (u64)g) : ~0ull;
        sc[boff + i] = in ? (u32)B.cov[g] : 0u;
    }
    __syncthreads();
    // element i of the A slice is sw[1 + i], i in [-1, na]; of the B slice sw[boff + 1 + i], i in [-1, nb]
    const u64 *wa = sw + 1, *wb = sw + boff + 1;
    const u32 *ca = sc + 1, *cb = sc + boff + 1;

    const u32 d0 = t * MI < nt ? t * MI : nt, d1 = d0 + MI < nt ? d0 + MI : nt;
    u32 lo = d0 > nb ? d0 - nb : 0u, hi = d0 < na ? d0 : na;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (wa[mid] <= wb[d0 - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    i32 ai = (i32)lo, bi = (i32)(d0 - lo);

    u64 ow[MI]; u32 ov[MI];
    u32 flags = 0;
#pragma unroll
    for (int e = 0; e < MI; e++) {
        ow[e] = 0; ov[e] = 0;
        if (d0 + e < d1) {
            const bool take_a = ai < (i32)na && (bi >= (i32)nb || wa[ai] <= wb[bi]);
            const u64 w = take_a ? wa[ai] : wb[bi];
            const u32 k = (u32)(w >> 32);
            const u32 cb_lt = (u32)(wb[bi - 1] >> 32) == k ? cb[bi - 1] : 0u;       // B's coverage below w
            u32 c, prev; bool keep;
            if (take_a) {
                const u32 ca_lt = (u32)(wa[ai - 1] >> 32) == k ? ca[ai - 1] : 0u;
                const u32 cb_le = wb[bi] == w ? cb[bi] : cb_lt;                     // (bi == nb: the element past the slice)
                c = ca[ai] + cb_le; prev = ca_lt + cb_lt; keep = true;
                ai++;
            } else {
                const u64 wp = wa[ai - 1];                                          // (ai == 0: the step before the slice)
                const u32 ca_le = (u32)(wp >> 32) == k ? ca[ai - 1] : 0u;
                c = ca_le + cb[bi]; prev = ca_le + cb_lt; keep = wp != w;           // a tied A element has spoken for both
                bi++;
            }
            if (keep && c != prev) { flags |= 1u << e; ow[e] = w; ov[e] = c; }
        }
    }
    const u32 mine = (u32)__popc(flags);
    u32 total;
    u32 at = block_excl_scan<u32, MT>(mine, red, &total);          // (its last barrier: every thread is done with the slices)
    if (!WRITE) {
        if (t == 0) { cnt[tile] = total; if (tile == 0) cnt[ntiles] = 0u; }
        return;
    }
    // compact in LDS, in merge order, then store the tile's steps side by side
#pragma unroll
    for (int e = 0; e < MI; e++)
        if ((flags >> e) & 1u) { sw[at] = ow[e]; sc[at] = ov[e]; at++; }
    __syncthreads();
    const u64 base = cnt[tile];
    for (u32 i = t; i < total; i += MT) {
        const u64 w = sw[i];
        ok[base + i] = (u32)(w >> 32); op[base + i] = (u32)w; oc[base + i] = (i32)sc[i];
    }
}

// ------------------------------------------------------------------------------------------------ steps -> blocks
struct BlockIn {
    const u32 *key; const i32 *cov; u64 n;
    __device__ u32 operator()(u64 i) const { return (cov[i] != 0 && i + 1 < n && key[i + 1] == key[i]) ? 1u : 0u; }
};
struct BlockOut {
    BlockIn in; const u32 *pos; u32 *ok, *os, *oe; i32 *oc; bool write; u64 *total;
    __device__ void operator()(u64 i, const u32 &t) const
    {
        if (write && in(i)) {
            if (ok) ok[t - 1] = in.key[i];
            if (os) os[t - 1] = pos[i];
            if (oe) oe[t - 1] = pos[i + 1] - 1u;
            if (oc) oc[t - 1] = in.cov[i];
        }
        if (i + 1 == in.n) *total = t;
    }
};

}  // namespace

// Scratch: WS_T0 (tile partition), WS_T1 (tile counts), WS_SCAN* (their scan).  `ix` comes from ivx_depth_profile_begin
// with nkeys = max of the two; a and b are only read (they may be the same profile).
ivx_status ivx_depth_profile_merge_device(ivx_ctx *ctx, const DepthProfileView &a, u32 nka, const DepthProfileView &b, u32 nkb, ivx_index *ix)
{
    hipStream_t st = ctx->stream;
    const u32 nk = ix->nkeys;
    if (nk) {
        hipLaunchKernelGGL(k_seen_or, dim3((u32)(((u64)nk + KT - 1) / KT)), dim3(KT), 0, st, a.seen, nka, b.seen, nkb, nk, const_cast<u8 *>(ix->dp.seen));
        IVX_HIP(ctx, hipGetLastError());
    }
    const u64 N = a.steps + b.steps;
    if (N == 0) return IVX_OK;
    if (N >= 0xFFFFFF00ull) return ctx->fail(IVX_ERR_INVALID, "depth profile merge: more than 2^32-257 steps in the two profiles");
    const u32 ntiles = (u32)((N + DEPTH_MERGE_TILE - 1) / DEPTH_MERGE_TILE);
    u32 *part, *cnt;
    IVX_TRY(ctx->get_scratch(WS_T0, ((size_t)ntiles + 1) * sizeof(u32), (void **)&part));
    IVX_TRY(ctx->get_scratch(WS_T1, ((size_t)ntiles + 1) * sizeof(u32), (void **)&cnt));
    hipLaunchKernelGGL(k_merge_partition, dim3((ntiles + 1 + KT - 1) / KT), dim3(KT), 0, st, a.key, a.pos, (u32)a.steps, b.key, b.pos, (u32)b.steps, ntiles, part);
    hipLaunchKernelGGL((k_merge_tile<false>), dim3(ntiles), dim3(MT), 0, st, a, b, (const u32 *)part, ntiles, cnt, (u32 *)nullptr, (u32 *)nullptr, (i32 *)nullptr);
    IVX_HIP(ctx, hipGetLastError());
    IVX_TRY(ivx_scan_exclusive_u32(ctx, cnt, (u64)ntiles + 1));
    IVX_HIP(ctx, hipGetLastError());
    u32 S32;
    IVX_TRY(ctx->fetch_wait((const u32 *)cnt + ntiles, st, &S32));
    const u64 S = S32;
    if (S == 0) return IVX_OK;
    u32 *sk, *sp; i32 *sv;
    IVX_TRY(ivx_index_alloc(ctx, ix, S * sizeof(u32), (void **)&sk));
    IVX_TRY(ivx_index_alloc(ctx, ix, S * sizeof(u32), (void **)&sp));
    IVX_TRY(ivx_index_alloc(ctx, ix, S * sizeof(i32), (void **)&sv));
    hipLaunchKernelGGL((k_merge_tile<true>), dim3(ntiles), dim3(MT), 0, st, a, b, (const u32 *)part, ntiles, cnt, sk, sp, sv);
    IVX_HIP(ctx, hipGetLastError());
    IVX_TRY(ivx_depth_profile_koff(ctx, sk, (u32)S, nk, const_cast<u32 *>(ix->dp.koff)));
    ix->dp.key = sk; ix->dp.pos = sp; ix->dp.cov = sv; ix->dp.steps = S;
    return IVX_OK;
}

// Scratch: WS_SCAN0 / WS_SCAN1 (tile sums of the counting scan).  The count is always made and read back; the write pass
// runs only when the buffers hold it.
ivx_status ivx_depth_profile_blocks_device(ivx_ctx *ctx, const DepthProfileView &dp, u32 *ok, u32 *os, u32 *oe, i32 *oc, u64 cap, u64 *n_out)
{
    using namespace ivxscan;
    *n_out = 0;
    if (dp.steps < 2) return IVX_OK;                        // (a key's last step never gives a block)
    hipStream_t st = ctx->stream;
    u64 *d_total = ctx->dword(SC_BLOCKS_TOTAL);
    const BlockIn in{dp.key, dp.cov, dp.steps};
    IVX_TRY((inclusive_f<CntScan>(ctx, in, BlockOut{in, dp.pos, nullptr, nullptr, nullptr, nullptr, false, d_total}, dp.steps)));
    IVX_HIP(ctx, hipGetLastError());
    IVX_TRY(ctx->fetch_wait(SC_BLOCKS_TOTAL, st, n_out));
    if (cap == 0 && !ok && !os && !oe && !oc) return IVX_OK;            // count only
    if (*n_out > cap) return ctx->fail(IVX_ERR_CAPACITY, "depth profile blocks: output buffers too small");
    if (*n_out == 0 || (!ok && !os && !oe && !oc)) return IVX_OK;
    IVX_TRY((inclusive_f<CntScan>(ctx, in, BlockOut{in, dp.pos, ok, os, oe, oc, true, d_total}, dp.steps)));
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}
