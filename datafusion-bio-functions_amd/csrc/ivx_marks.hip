// ivx_marks.hip -- build-side match marks: which BUILD rows a probe batch matched (HashJoinExec's visited_left_side; the
// reference's IntervalJoinExec has no counterpart, it emits Inner rows for LeftSemi / LeftAnti / Left / Full).
//
// A mark bitmap is one bit per build row, bit b & 31 of word b >> 5 (an Arrow Boolean / validity buffer).  Kernels only
// ever OR into it, with device-scope atomics behind a plain test of the word (mark_bit, ivx_join.hpp), so several
// streams and contexts may mark into one buffer at once.
//
//   ivx_mark_probe the direct path: MarkOp on k_probe_rows (ivx_rowops.hpp), the match sets the build row's bit.  Any index,
//                  any batch size; what small batches take.  (Big batches over a lean index: the same operator on k_lean /
//                  k_lean_rest in ivx_regions_probe.hip.)
//   k_bits_mark    OR bit idx[i] for a list of row numbers (Left / Full joins: the pairs exist anyway)
//   k_bits_count / k_bits_write   ivx_bits_select: positions of the set (or clear) bits, ascending -- popcount per 256-word
//                  block, exclusive scan of the block counts, then every lane expands its word at block base + prefix.
#include "ivx_where.hpp"

namespace {

constexpr int MT = 256;     // workgroup of every kernel here

__global__ __launch_bounds__(MT) void k_bits_mark(const u32 *__restrict__ idx, u64 n, u32 *bits, u64 n_bits, u32 *bad)
{
    for (u64 i = (u64)blockIdx.x * MT + threadIdx.x; i < n; i += (u64)gridDim.x * MT) {
        const u32 j = idx[i];
        if (j == IVX_NULL_IDX) continue;
        if (j >= n_bits) { *bad = 1; continue; }
        mark_bit(bits, j);
    }
}

// word w of the selection: the bits wanted (flip = ~0u selects the clear ones), nothing at or past n_bits
__device__ __forceinline__ u32 select_word(const u32 *__restrict__ bits, u64 w, u64 nw, u64 n_bits, u32 flip)
{
    if (w >= nw) return 0u;
    u32 v = bits[w] ^ flip;
    if (w == nw - 1 && (n_bits & 31u)) v &= (1u << (n_bits & 31u)) - 1u;
    return v;
}

__global__ __launch_bounds__(MT) void k_bits_count(const u32 *__restrict__ bits, u64 nw, u64 n_bits, u32 flip, u32 *__restrict__ counts)
{
    __shared__ u32 lds[MT / IVX_WAVE];
    const u32 c = (u32)__popc(select_word(bits, (u64)blockIdx.x * MT + threadIdx.x, nw, n_bits, flip));
    const u32 tot = block_sum<u32, MT>(c, lds);
    if (threadIdx.x == 0) counts[blockIdx.x] = tot;
}

__global__ __launch_bounds__(MT) void k_bits_write(const u32 *__restrict__ bits, u64 nw, u64 n_bits, u32 flip, const u32 *__restrict__ base,
                                                   u32 *__restrict__ out)
{
    __shared__ u32 lds[MT / IVX_WAVE + 1];
    const u64 w = (u64)blockIdx.x * MT + threadIdx.x;
    u32 v = select_word(bits, w, nw, n_bits, flip);
    u32 total;
    const u32 ex = block_excl_scan<u32, MT>((u32)__popc(v), lds, &total);
    u64 at = (u64)base[blockIdx.x] + ex;
    while (v) {
        out[at++] = (u32)(w << 5) + (u32)__builtin_ctz(v);
        v &= v - 1u;
    }
}

}  // namespace

ivx_status ivx_mark_probe(ivx_ctx *ctx, const JoinIndexView &jv, const u32 *key, const i32 *s, const i32 *e, u64 n, u32 *marks,
                          const WherePred *w)
{
    ivx_status st = IVX_OK;
    with_where(w, MarkOp{{}, marks}, [&](const auto &op) { st = ivx_direct_probe(ctx, jv, key, s, e, n, op); });
    return st;
}

ivx_status ivx_bits_mark_device(ivx_ctx *ctx, const u32 *idx, u64 n, u32 *bits, u64 n_bits)
{
    if (n == 0) return IVX_OK;
    hipStream_t st = ctx->stream;
    u32 *bad = ctx->dword<u32>(SC_MARK_BAD);                           // the out-of-range flag, as the take kernels'
    IVX_HIP(ctx, hipMemsetAsync(bad, 0, sizeof(u64), st));
    hipLaunchKernelGGL(k_bits_mark, dim3(ivx_stream_grid(n, MT * 4, 256 * 16)), dim3(MT), 0, st, idx, n, bits, n_bits, bad);
    IVX_HIP(ctx, hipGetLastError());
    return ctx->check_flag(SC_MARK_BAD, st, "bits_mark: index out of bounds");
}

// out == nullptr: count only.  *n_out = the positions there are; more than cap: IVX_ERR_CAPACITY, nothing written
ivx_status ivx_bits_select_device(ivx_ctx *ctx, const u32 *bits, u64 n_bits, int want_set, u32 *out, u64 cap, u64 *n_out)
{
    *n_out = 0;
    if (n_bits == 0) return IVX_OK;
    hipStream_t st = ctx->stream;
    const u64 nw = (n_bits + 31) / 32;
    const u64 nblk = (nw + MT - 1) / MT;
    const u32 flip = want_set ? 0u : 0xFFFFFFFFu;
    u32 *counts;
    IVX_TRY(ctx->get_scratch(WS_T0, (nblk + 1) * sizeof(u32), (void **)&counts));
    IVX_HIP(ctx, hipMemsetAsync(counts + nblk, 0, sizeof(u32), st));
    hipLaunchKernelGGL(k_bits_count, dim3((u32)nblk), dim3(MT), 0, st, bits, nw, n_bits, flip, counts);
    IVX_TRY(ivx_scan_exclusive_u32(ctx, counts, nblk + 1));            // counts[nblk] = the total
    IVX_HIP(ctx, hipGetLastError());
    u32 total32;
    IVX_TRY(ctx->fetch_wait((const u32 *)counts + nblk, st, &total32));
    const u64 total = total32;
    *n_out = total;
    if (out == nullptr && cap == 0) return IVX_OK;
    if (total > cap) return ctx->fail(IVX_ERR_CAPACITY, "bits_select: output buffer too small");
    if (total == 0) return IVX_OK;
    hipLaunchKernelGGL(k_bits_write, dim3((u32)nblk), dim3(MT), 0, st, bits, nw, n_bits, flip, (const u32 *)counts, out);
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}
