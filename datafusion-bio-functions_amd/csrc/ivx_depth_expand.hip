// ivx_depth_expand.hip -- per-base depth(): the step function of the coverage kept on the device (a depth profile), and
// windows of it expanded to one (position, coverage Int16) row per base (the reference's per_base = true:
// bio-function-pileup coverage.rs:271-365 PerBaseEmitter, physical_exec.rs:404-414, :517-548).
//
//   profile   from the front half of depth() (ivx_depth.hip: the sorted events and, per (key, position) group, the key's
//             running sum c and the group's sum g): a group with g != 0 is a step (key, position, c).  One counting scan
//             sizes the three columns, the same scan again writes them; a search per key gives the key's first step.
//   expand    one workgroup makes one tile of DEPTH_EXPAND_TILE consecutive outputs.  The wavefront-wide 64-ary search inside
//             the key's slice (ivx_depth_regions.hpp, which the region statistics share, with the key's c0) finds the
//             tile's first step (4 dependent loads for 16 M steps, not 24); the step before it,
//             if the key has one, is the carry-in.  A tile without a step -- most of a genome -- is a constant fill and
//             touches no LDS.  Otherwise the tile's steps (at most one per slot: positions are distinct) are scattered to an
//             LDS image with a bit per set slot, every thread takes the last set slot of its 8 slots, a scan over the
//             threads ("the later set slot wins") spreads them, and the thread fills its 8 slots from there.
//   stores    2-byte stores cost ~12.5x a 16-byte store per byte on this chip, so the tile grid is laid over the OUTPUT
//             ADDRESSES, not over the positions: tile b covers the elements whose 16-byte line is b * TILE/8 ... of the
//             coverage column (and, independently, b * TILE/4 ... of the position column: positions are arithmetic and
//             need no step).  Every thread then owns whole aligned lines and stores each with one 16-byte store; only the
//             window's first and last line, when the caller's pointer or length cuts them, leave as scalar stores.
#include "ivx_depth_regions.hpp"
#include "ivx_scan.hpp"

namespace {

constexpr int DEPTH_EXPAND_TILE = 4096;         // outputs per workgroup; the LDS image is 16.5 KiB: 9 workgroups fit a CU's 160 KiB
constexpr int XT = DEPTH_EXPAND_TILE / 8;       // threads: 8 slots = one 16-byte line of coverages each
constexpr int XW = XT / IVX_WAVE;
static_assert(XT % IVX_WAVE == 0 && XT <= 1024, "one 16-byte coverage line per thread");

constexpr int PT = 256;

// ------------------------------------------------------------------------------------------------ events -> steps
struct CntScan {
    using T = u32;
    __host__ __device__ static T identity() { return 0u; }
    __device__ static T combine(const T &a, const T &b) { return a + b; }
    __device__ static T shfl_up(const T &v, int d) { return __shfl_up(v, d, IVX_WAVE); }
};
// event i is a step: the last event of its (key, position) group, and the group's deltas do not cancel
struct StepIn {
    const u64 *ev; const uint2 *cg; u64 n;
    __device__ u32 operator()(u64 i) const { return ((i + 1 == n || ev[i + 1] != ev[i]) && cg[i].y != 0) ? 1u : 0u; }
};
struct StepOut {
    StepIn in; u32 *ok, *op; i32 *oc; u64 *total;       // ok == null: count only
    __device__ void operator()(u64 i, const u32 &t) const
    {
        if (ok && in(i)) {
            const u64 w = in.ev[i];
            ok[t - 1] = (u32)(w >> 32); op[t - 1] = (u32)w; oc[t - 1] = (i32)in.cg[i].x;
        }
        if (i + 1 == in.n) *total = t;
    }
};

// koff[k] = the first step with key >= k, k <= nkeys
__global__ __launch_bounds__(PT) void k_profile_koff(const u32 *__restrict__ skey, u32 steps, u32 nkeys, u32 *__restrict__ koff)
{
    const u64 k = (u64)blockIdx.x * PT + threadIdx.x;
    if (k > nkeys) return;
    u32 lo = 0, hi = steps;
    while (lo < hi) { const u32 mid = lo + ((hi - lo) >> 1); if ((u64)skey[mid] < k) lo = mid + 1; else hi = mid; }
    koff[k] = lo;
}

// ------------------------------------------------------------------------------------------------ steps -> positions
// Frames: the coverage column's frame starts `sc` elements before out_cov, at the 16-byte line out_cov points into; element v
// of it is output i = v - sc, position first_pos + v - sc.  The position column's frame (shift `sp`) likewise.  Tile b is
// elements [b * TILE, (b + 1) * TILE) of BOTH frames.
__global__ __launch_bounds__(XT) void k_depth_expand(DepthProfileView dp, u32 key, u64 first_pos, u64 n, u32 sc, u32 sp, int skip_pos0,
                                                     i32 *__restrict__ out_pos, int16_t *__restrict__ out_cov)
{
    constexpr int T = DEPTH_EXPAND_TILE;
    __shared__ i32 img[T];
    __shared__ u32 setw[T / 32];
    __shared__ i32 wval[XW];
    __shared__ u32 whas[XW];
    const u32 t = threadIdx.x, l = lane_id(), w = t / IVX_WAVE;
    const u64 tile0 = (u64)blockIdx.x * T;

    if (out_pos) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const u64 u0 = tile0 + 4ull * (t + (u32)XT * j);
            if (u0 >= sp && u0 + 4 <= sp + n) {
                const u64 i = u0 - sp;
                const u32 p = (u32)(first_pos + i);
                *(int4 *)(out_pos + i) = make_int4((i32)p, (i32)(p + 1u), (i32)(p + 2u), (i32)(p + 3u));
            } else {
#pragma unroll
                for (u32 e = 0; e < 4; e++) {
                    const u64 u = u0 + e;
                    if (u >= sp && u < sp + n) out_pos[u - sp] = (i32)(u32)(first_pos + (u - sp));
                }
            }
        }
    }
    if (!out_cov || tile0 >= sc + n) return;            // (the same for the whole workgroup)

    const u32 klo = dp.koff[key], khi = dp.koff[key + 1];
    const i64 P0 = (i64)first_pos + (i64)tile0 - (i64)sc;   // position of the tile's slot 0 (below 0 only in the window's first line)
    const u64 lo_pos = P0 < 0 ? 0ull : (u64)P0;
    const u64 hi_pos = (u64)(P0 + T);                       // (> first_pos: the tile holds an element of the window)

    const u32 a = wave_first_at_or_after(dp.pos, klo, khi - klo, lo_pos, l);    // the first step of the key at or after lo_pos
    const u32 cin = a > klo ? (u32)dp.cov[a - 1] : 0u;      // the step before it belongs to the same key, or there is no carry
    const u32 c0 = klo < khi ? key_c0(dp, klo, skip_pos0) : 0u;     // (a key without steps has no first step to read)
    const bool busy = a < khi && (u64)dp.pos[a] < hi_pos;

    u32 o[8];
    if (!busy) {
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = (cin - c0) & 0xFFFFu;
    } else {
        if (t < T / 32) setw[t] = 0u;
        __syncthreads();
        for (u64 idx = (u64)a + t; idx < khi; idx += XT) {
            const u64 p = dp.pos[idx];
            if (p >= hi_pos) break;
            const u32 slot = (u32)((i64)p - P0);
            img[slot] = dp.cov[idx];
            atomicOr(&setw[slot >> 5], 1u << (slot & 31u));
        }
        __syncthreads();
        const u32 bits = (setw[t >> 2] >> (8u * (t & 3u))) & 0xFFu;
        u32 has = bits != 0u ? 1u : 0u;
        u32 val = has ? (u32)img[8u * t + (31u - (u32)__clz((int)bits))] : 0u;
        // inclusive scan over the lanes: the later set slot wins
#pragma unroll
        for (int d = 1; d < IVX_WAVE; d <<= 1) {
            const u32 oh = __shfl_up(has, d, IVX_WAVE), ov = __shfl_up(val, d, IVX_WAVE);
            if (l >= (u32)d && !has) { has = oh; val = ov; }
        }
        if (l == IVX_WAVE - 1) { whas[w] = has; wval[w] = (i32)val; }
        __syncthreads();
        u32 ph = __shfl_up(has, 1, IVX_WAVE), pv = __shfl_up(val, 1, IVX_WAVE);
        if (l == 0) ph = 0u;
        for (int j = (int)w - 1; j >= 0 && !ph; j--) { ph = whas[j]; pv = (u32)wval[j]; }
        u32 cur = ph ? pv : cin;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            if ((bits >> e) & 1u) cur = (u32)img[8u * t + e];
            o[e] = (cur - c0) & 0xFFFFu;
        }
    }
    const u64 v0 = tile0 + 8ull * t;
    if (v0 >= sc && v0 + 8 <= sc + n) {
        *(int4 *)(out_cov + (v0 - sc)) = make_int4((i32)(o[0] | (o[1] << 16)), (i32)(o[2] | (o[3] << 16)),
                                                   (i32)(o[4] | (o[5] << 16)), (i32)(o[6] | (o[7] << 16)));
    } else {
#pragma unroll
        for (u32 e = 0; e < 8; e++) {
            const u64 v = v0 + e;
            if (v >= sc && v < sc + n) out_cov[v - sc] = (int16_t)o[e];
        }
    }
}

}  // namespace

// key_seen and the per-key table, zeroed: what an empty profile consists of.  Before the front half runs, which marks key_seen.
ivx_status ivx_depth_profile_begin(ivx_ctx *ctx, ivx_index *ix, u8 **seen)
{
    u32 *koff; u8 *sn;
    const size_t nk = ix->nkeys;
    IVX_TRY(ivx_index_alloc(ctx, ix, (nk + 1) * sizeof(u32), (void **)&koff));
    IVX_TRY(ivx_index_alloc(ctx, ix, nk ? nk : 1, (void **)&sn));
    IVX_HIP(ctx, hipMemsetAsync(koff, 0, (nk + 1) * sizeof(u32), ctx->stream));
    IVX_HIP(ctx, hipMemsetAsync(sn, 0, nk ? nk : 1, ctx->stream));
    ix->dp = DepthProfileView{nullptr, nullptr, nullptr, koff, sn, 0};
    *seen = sn;
    return IVX_OK;
}

// the per-key table of a profile's key column (also what a merge rebuilds: ivx_depth_merge.hip)
ivx_status ivx_depth_profile_koff(ivx_ctx *ctx, const u32 *skey, u32 steps, u32 nkeys, u32 *koff)
{
    hipLaunchKernelGGL(k_profile_koff, dim3((u32)(((u64)nkeys + 1 + PT - 1) / PT)), dim3(PT), 0, ctx->stream, skey, steps, nkeys, koff);
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}

// Scratch: WS_SCAN0 / WS_SCAN1 (tile sums of the counting scan); reads the front half's WS_SA0 / WS_SB0 and WS_T0.
ivx_status ivx_depth_profile_finish(ivx_ctx *ctx, ivx_index *ix, const ivx_depth_evs &evs)
{
    using namespace ivxscan;
    if (evs.n == 0) return IVX_OK;
    hipStream_t st = ctx->stream;
    u64 *d_total = ctx->dword(SC_STEPS_TOTAL);
    const StepIn in{evs.ev, evs.cg, evs.n};
    IVX_TRY((inclusive_f<CntScan>(ctx, in, StepOut{in, nullptr, nullptr, nullptr, d_total}, evs.n)));
    IVX_HIP(ctx, hipGetLastError());
    u64 S;
    IVX_TRY(ctx->fetch_wait(SC_STEPS_TOTAL, st, &S));
    if (S == 0) return IVX_OK;
    if (S >= 0xFFFFFF00ull) return ctx->fail(IVX_ERR_INVALID, "depth profile: more than 2^32-257 steps");     // (the expand kernel's search is 32-bit)
    u32 *sk, *sp; i32 *sv;
    IVX_TRY(ivx_index_alloc(ctx, ix, S * sizeof(u32), (void **)&sk));
    IVX_TRY(ivx_index_alloc(ctx, ix, S * sizeof(u32), (void **)&sp));
    IVX_TRY(ivx_index_alloc(ctx, ix, S * sizeof(i32), (void **)&sv));
    IVX_TRY((inclusive_f<CntScan>(ctx, in, StepOut{in, sk, sp, sv, d_total}, evs.n)));
    u32 *koff = const_cast<u32 *>(ix->dp.koff);
    IVX_TRY(ivx_depth_profile_koff(ctx, sk, (u32)S, ix->nkeys, koff));
    ix->dp.key = sk; ix->dp.pos = sp; ix->dp.cov = sv; ix->dp.steps = S;
    return IVX_OK;
}

ivx_status ivx_depth_expand_device(ivx_ctx *ctx, const DepthProfileView &dp, u32 key, u32 first_pos, u64 n, int skip_pos0,
                                   i32 *out_pos, int16_t *out_cov)
{
    if (n == 0 || (!out_pos && !out_cov)) return IVX_OK;
    const u32 sc = out_cov ? (u32)(((uintptr_t)out_cov & 15u) / sizeof(int16_t)) : 0u;
    const u32 sp = out_pos ? (u32)(((uintptr_t)out_pos & 15u) / sizeof(i32)) : 0u;
    u64 span = 0;
    if (out_cov) span = sc + n;
    if (out_pos && sp + n > span) span = sp + n;
    const u64 ntiles = (span + DEPTH_EXPAND_TILE - 1) / DEPTH_EXPAND_TILE;
    hipLaunchKernelGGL(k_depth_expand, dim3((u32)ntiles), dim3(XT), 0, ctx->stream, dp, key, (u64)first_pos, n, sc, sp, skip_pos0, out_pos, out_cov);
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}
