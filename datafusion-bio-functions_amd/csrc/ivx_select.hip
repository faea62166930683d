// ivx_select.hip -- overlap select: per probe row, over exactly the build rows ivx_probe_overlap_fill pairs it with, the one
// build row that is best by a criterion -- the smallest or largest value of a build-side column, the longest or shortest
// overlap, the first or last row -- and, if wanted, the criterion's value there (ivx_probe_overlap_select; a left join to
// at most one row, bedtools map -o first / last, SQL's ROW_NUMBER() ... = 1 over the range join).  No pair is ever written.
//
//   k_probe_select  the direct path: k_probe_agg's row loop and walk_ent, with SelAcc (ivx_select.hpp) in place of the sums.
//                   Any index, any batch size; what small batches take, and what every batch takes whose index is not lean.
//                   (Big batches over a lean index: k_sel_fast / k_sel_rest in ivx_regions_probe.hip.)
//
// A row without a match stores IVX_NULL_IDX and score 0: every row is walked here, so every wanted output element is written.
#include <type_traits>
#include "ivx_select.hpp"

namespace {

constexpr int ST = 256;     // workgroup
constexpr int SI = 4;       // probe rows per thread per tile of a big batch (as k_probe_agg's AI)

// AI_: probe rows per thread per tile; BY: the criterion; VB: bytes of a value (read by the *_VAL criteria only); SCORE: see SelAcc
template <int AI_, int BY, int VB, bool SCORE>
__global__ __launch_bounds__(ST) void k_probe_select(JoinIndexView ix, const u32 *__restrict__ pkey, const i32 *__restrict__ ps,
                                                     const i32 *__restrict__ pe, u64 n, const void *__restrict__ val, SelOut out)
{
    const u32 sh0 = ix.hdr[HDR_SH0], nlev = ix.hdr[HDR_NLEV];
    constexpr int TILE_ = ST * AI_;
    const u64 ntiles = (n + TILE_ - 1) / TILE_;
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
        for (int it = 0; it < AI_; it++) {
            const u64 i = tile * TILE_ + (u64)it * ST + threadIdx.x;
            if (i >= n) continue;
            const u32 k = pkey ? pkey[i] : 0u;                      // (a key id the build side does not have: walk_ent leaves at once)
            const i32 qs = ps[i], qe = pe[i];
            SelAcc<BY, SCORE> a;
            walk_ent(ix, sh0, 0, nlev, k, qs, qe, [&](const ivx_ent &x) {
                const i64 v = sel_by_val<BY> ? agg_val<VB>(val, x.row) : 0;
                a.add(sel_crit<BY>(v, x.row, qs, qe, x.s, x.e), x.row);
            });
            a.store(out, i);
        }
    }
}

}  // namespace

ivx_status ivx_sel_probe(ivx_ctx *ctx, const JoinIndexView &jv, const u32 *key, const i32 *s, const i32 *e, u64 n,
                         const void *val, u32 val_bytes, int by, const SelOut &out)
{
    if (n == 0) return IVX_OK;
    const bool small = n <= (1u << 18);                                // one row per thread, as ivx_agg_probe
    const u32 grid = small ? (u32)((n + ST - 1) / ST) : ivx_stream_grid(n, ST * SI, 256 * 8);
    auto launch = [&](auto ai) {
        sel_dispatch(by, val_bytes, out.score != nullptr, [&](auto b, auto vb, auto sc) {
            hipLaunchKernelGGL((k_probe_select<decltype(ai)::value, decltype(b)::value, decltype(vb)::value, decltype(sc)::value>), dim3(grid), dim3(ST), 0,
                               ctx->stream, jv, key, s, e, n, val, out);
        });
    };
    if (small) launch(std::integral_constant<int, 1>{}); else launch(std::integral_constant<int, SI>{});
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}
