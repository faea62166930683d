// ivx_agg.hip -- overlap aggregates: per probe row, over exactly the build rows ivx_probe_overlap_fill pairs it with, the
// count, sum, min and max of a build-side value column, the overlapped bases and the bases-weighted sum
// (ivx_probe_overlap_agg; SQL's GROUP BY probe row over the join, bedtools map).  No pair is ever written.
//
//   k_probe_agg   the direct path: k_probe_overlap's row loop, walk_ent (the coordinates give the overlap's length) and
//                 val[row] gathered per match.  Any index, any batch size; what small batches take, and what every batch
//                 takes whose index is not lean.  (Big batches over a lean index: k_agg_fast / k_agg_rest in
//                 ivx_regions_probe.hip.)
//
// A row without a match stores count 0, sum 0, bases 0, wsum 0 and the identities INT64_MAX / INT64_MIN for min / max: every
// row is walked here, so every wanted output element is written.
#include <type_traits>
#include "ivx_agg.hpp"

namespace {

constexpr int AT = 256;     // workgroup
constexpr int AI = 4;       // probe rows per thread per tile of a big batch (as k_probe_overlap's PI)

// AI_: probe rows per thread per tile; VB: bytes of a value; MM / WT: see AggAcc
template <int AI_, int VB, bool MM, bool WT>
__global__ __launch_bounds__(AT) void k_probe_agg(JoinIndexView ix, const u32 *__restrict__ pkey, const i32 *__restrict__ ps,
                                                  const i32 *__restrict__ pe, u64 n, const void *__restrict__ val, AggOut out)
{
    const u32 sh0 = ix.hdr[HDR_SH0], nlev = ix.hdr[HDR_NLEV];
    constexpr int TILE_ = AT * AI_;
    const u64 ntiles = (n + TILE_ - 1) / TILE_;
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
        for (int it = 0; it < AI_; it++) {
            const u64 i = tile * TILE_ + (u64)it * AT + threadIdx.x;
            if (i >= n) continue;
            const u32 k = pkey ? pkey[i] : 0u;                      // (a key id the build side does not have: walk_ent leaves at once)
            const i32 qs = ps[i], qe = pe[i];
            AggAcc<MM, WT> a;
            walk_ent(ix, sh0, 0, nlev, k, qs, qe, [&](const ivx_ent &x) { a.add(agg_val<VB>(val, x.row), qs, qe, x.s, x.e); });
            a.store(out, i);
        }
    }
}

}  // namespace

ivx_status ivx_agg_probe(ivx_ctx *ctx, const JoinIndexView &jv, const u32 *key, const i32 *s, const i32 *e, u64 n,
                         const void *val, u32 val_bytes, const AggOut &out)
{
    if (n == 0) return IVX_OK;
    const bool small = n <= (1u << 18);                                // one row per thread, as ivx_join_probe
    const u32 grid = small ? (u32)((n + AT - 1) / AT) : ivx_stream_grid(n, AT * AI, 256 * 8);
    const bool mm = out.vmin || out.vmax, wt = out.bases || out.wsum;
    auto launch = [&](auto ai, auto vb, auto m, auto w) {
        hipLaunchKernelGGL((k_probe_agg<decltype(ai)::value, decltype(vb)::value, decltype(m)::value, decltype(w)::value>), dim3(grid), dim3(AT), 0,
                           ctx->stream, jv, key, s, e, n, val, out);
    };
    auto by_flags = [&](auto ai, auto vb) {
        if (mm && wt) launch(ai, vb, std::true_type{}, std::true_type{});
        else if (mm) launch(ai, vb, std::true_type{}, std::false_type{});
        else if (wt) launch(ai, vb, std::false_type{}, std::true_type{});
        else launch(ai, vb, std::false_type{}, std::false_type{});
    };
    auto by_width = [&](auto ai) {
        if (val_bytes == 4) by_flags(ai, std::integral_constant<int, 4>{}); else by_flags(ai, std::integral_constant<int, 8>{});
    };
    if (small) by_width(std::integral_constant<int, 1>{}); else by_width(std::integral_constant<int, AI>{});
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}
