// ivx_rowops.hpp -- per-row operators over the overlap index: what ONE probe row does with its matches, written once per
// operator and run by three kernels -- k_probe_rows (here: the direct walk over the index in global memory, any index, any
// batch size) and k_lean / k_lean_rest (ivx_regions_probe.hip: big batches over a lean index, the candidates out of LDS).
//
// An operator is a small struct that carries its kernel arguments and defines
//   W                      the page pool's word type: u64 for values written in place, const u64 otherwise
//   Lds                    the LDS it keeps beside the staged slice (k_lean only)
//   skip_empty             a row with end < start is not walked (k_lean_rest; the lean kernel never sees one: it is an escape)
//   adj                    the strict mode's shrinking of an escape's coordinates (k_lean_rest: see rest_row); 0 but for RvOp
//   begin(Lds&)            all threads, before LeanRows::init, whose barrier covers it
//   enter(ix, S, r, Lds&)  all threads, after region r's slice S is staged; an operator that stages here ends in a barrier
//   leave(ix, S, Lds&)     all threads, before the slice is replaced and at the kernel's end
//   Row                    one probe row's state:
//     hit(op, lds, j, qs, qe, xs, xe)   a match with slice slot j (k_lean)
//     hit(op, x, qs, qe)                a match with index entry x (k_lean_rest, k_probe_rows)
//     done(op, word, at, hi)            the row is finished.  Region path: word = the row's own word in the pool, at = its pool
//                                       index (the operators' records are indexed like the pool), hi = the word's upper half.
//                                       Direct path: word = nullptr, at = the input row.
// RowOpBase holds what most operators leave empty.  RvOp and MarkOp are here; AggOp: ivx_agg.hpp; SelOp: ivx_select.hpp.
#pragma once
#include <type_traits>
#include "ivx_join.hpp"

// run-time bools as template arguments: f(std::true_type / std::false_type ...), one per bool, in order
template <class F> inline void with_bools(F &&f) { f(); }
template <class F, class... B> inline void with_bools(F &&f, bool b, B... rest)
{
    if (b) with_bools([&](auto... t) { f(std::true_type{}, t...); }, rest...);
    else with_bools([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}
#define IVX_B(tag) (decltype(tag)::value)

#ifndef IVX_RP_ECAP
#define IVX_RP_ECAP 6144
#endif
constexpr u32 RP_ECAP = IVX_RP_ECAP;       // index entries staged per slice: what an operator's per-entry LDS is sized by
constexpr int RP_T = 1024;                 // region probe kernels: one workgroup per CU (LDS-bound), 16 wavefronts

struct RowOpBase {
    using W = const u64;
    struct Lds {};
    static constexpr bool skip_empty = false;
    static constexpr u32 adj = 0u;
    template <class L> __device__ __forceinline__ void begin(L &) const {}
    template <class S, class L> __device__ __forceinline__ void enter(const JoinIndexView &, const S &, u32, L &) const {}
    template <class S, class L> __device__ __forceinline__ void leave(const JoinIndexView &, const S &, L &) const {}
};

// all threads: f(j, build row of slice entry j) for every entry of the staged slice S, then a barrier (the slice stages no
// row ids: ix.ent again)
template <class S, class F>
__device__ __forceinline__ void slice_rows(const JoinIndexView &ix, const S &sl, u32 r, F &&f)
{
    const u32 ne = ix.rdesc[r].ne;
    if (sl.inlds) for (u32 j = threadIdx.x; j < ne; j += RP_T) f(j, ix.ent[sl.e0 + j].row);   // (inlds: ne <= RP_ECAP)
    __syncthreads();
}

// ------------------------------------------------------------------ one 32-bit value per probe row
//   RV_COUNT     count_overlaps: 0 if qe < qs (interval_tree.rs:42-44), else the number of build rows the
//                literal predicate matches -- equal to #{starts <= qe} - #{ends < qs} (:45-48) whenever no
//                build row has end < start, which is when the host takes this path
//   RV_COVERAGE  get_coverage over the merged nodes: sum of max(1, min(qe+1, last) - max(qs-1, first)) in
//                wrapping i32 arithmetic (:145-152)
enum { RV_COUNT = 2, RV_COVERAGE = 3, RV_MATCHES = 4 };   // RV_MATCHES: the join's rle_right / exists (plain match count)

__device__ __forceinline__ i32 rv_wadd(i32 a, i32 b) { return (i32)((u32)a + (u32)b); }
__device__ __forceinline__ i32 rv_wsub(i32 a, i32 b) { return (i32)((u32)a - (u32)b); }

// The value replaces the low half of the row's packed word in place; the un-permute masks the row id out of the upper half.
template <int KIND>
struct RvOp : RowOpBase {
    using W = u64;
    static constexpr bool skip_empty = KIND == RV_COUNT;
    u32 adj;
    struct Row {
        u32 v = 0;
        __device__ __forceinline__ void hit(const RvOp &, const Lds &, u32, i32 qs, i32 qe, i32 xs, i32 xe)
        {
            if (KIND == RV_COVERAGE) {                                   // the closed query grown by one on either side
                const i32 a = rv_wadd(qe, 1), b = rv_wsub(qs, 1);
                const i32 d = rv_wsub(a < xe ? a : xe, b > xs ? b : xs);
                v = (u32)rv_wadd((i32)v, d > 1 ? d : 1);
            } else v++;
        }
        __device__ __forceinline__ void hit(const RvOp &op, const ivx_ent &x, i32 qs, i32 qe) { hit(op, Lds{}, 0u, qs, qe, x.s, x.e); }
        __device__ __forceinline__ void done(const RvOp &, u64 *word, u64, u32 hi) const { *word = (u64)v | ((u64)hi << 32); }
    };
};

// ------------------------------------------------------------------ build-side match marks
// Which BUILD rows the batch matched: nothing is stored per probe row.  k_lean: one bit per slice entry in LDS, a match ORs
// bit j with one LDS atomic; when the workgroup leaves a region, and at the end of its share, it sweeps the words -- every
// set bit is a matched entry, whose build row gets its bit in the caller's bitmap by test-then-OR (mark_bit), and the LDS
// word is cleared.  Global atomics are then per distinct matched build row and workgroup visit, not per match (the headline:
// ~37 matches per build row).  The other two kernels mark straight into the caller's bitmap.
struct MarkOp : RowOpBase {
    u32 *marks;
    static constexpr u32 NBW = RP_ECAP / 32u;
    static_assert(RP_ECAP % 32u == 0, "one LDS bit per slice entry, whole words");
    struct Lds { u32 bits[NBW]; };
    __device__ __forceinline__ void begin(Lds &l) const { for (u32 t = threadIdx.x; t < NBW; t += RP_T) l.bits[t] = 0u; }
    // (the slice load or the kernel's end that follows brings the barrier behind the sweep)
    template <class S> __device__ __forceinline__ void leave(const JoinIndexView &ix, const S &sl, Lds &l) const
    {
        __syncthreads();
        for (u32 w = threadIdx.x; w < NBW; w += RP_T) {
            u32 m = l.bits[w];
            if (m == 0u) continue;
            l.bits[w] = 0u;
            do {
                const u32 j = (w << 5) + (u32)__builtin_ctz(m);
                m &= m - 1u;
                mark_bit(marks, ix.ent[sl.e0 + j].row);
            } while (m);
        }
    }
    struct Row {
        __device__ __forceinline__ void hit(const MarkOp &, Lds &l, u32 j, i32, i32, i32, i32)
        {
            __hip_atomic_fetch_or(&l.bits[j >> 5], 1u << (j & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __device__ __forceinline__ void hit(const MarkOp &op, const ivx_ent &x, i32, i32) { mark_bit(op.marks, x.row); }
        __device__ __forceinline__ void done(const MarkOp &, const u64 *, u64, u32) const {}
    };
};

// ------------------------------------------------------------------ the direct walk
// AI: probe rows per thread per tile; a DataFusion-sized batch takes ONE row per thread (see k_probe_overlap)
constexpr int ROWS_T = 256;    // workgroup
constexpr int ROWS_AI = 4;     // probe rows per thread per tile of a big batch (as k_probe_overlap's PI)

template <int AI, class Op>
__global__ __launch_bounds__(ROWS_T) void k_probe_rows(JoinIndexView ix, const u32 *__restrict__ pkey, const i32 *__restrict__ ps,
                                                       const i32 *__restrict__ pe, u64 n, Op op)
{
    const u32 sh0 = ix.hdr[HDR_SH0], nlev = ix.hdr[HDR_NLEV];
    constexpr int TILE_ = ROWS_T * AI;
    const u64 ntiles = (n + TILE_ - 1) / TILE_;
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
        for (int it = 0; it < AI; it++) {
            const u64 i = tile * TILE_ + (u64)it * ROWS_T + threadIdx.x;
            if (i >= n) continue;
            const u32 k = pkey ? pkey[i] : 0u;                      // (a key id the build side does not have: walk_ent leaves at once)
            const i32 qs = ps[i], qe = pe[i];
            typename Op::Row a;
            walk_ent(ix, sh0, 0, nlev, k, qs, qe, [&](const ivx_ent &x) { a.hit(op, x, qs, qe); });
            a.done(op, nullptr, i, 0u);                             // every row is walked, so every wanted output element is written
        }
    }
}

template <class Op>
inline ivx_status ivx_direct_probe(ivx_ctx *ctx, const JoinIndexView &jv, const u32 *key, const i32 *s, const i32 *e, u64 n, const Op &op)
{
    if (n == 0) return IVX_OK;
    const bool small = n <= (1u << 18);                                // one row per thread, as ivx_join_probe
    const u32 grid = small ? (u32)((n + ROWS_T - 1) / ROWS_T) : ivx_stream_grid(n, ROWS_T * ROWS_AI, 256 * 8);
    if (small) hipLaunchKernelGGL((k_probe_rows<1, Op>), dim3(grid), dim3(ROWS_T), 0, ctx->stream, jv, key, s, e, n, op);
    else hipLaunchKernelGGL((k_probe_rows<ROWS_AI, Op>), dim3(grid), dim3(ROWS_T), 0, ctx->stream, jv, key, s, e, n, op);
    IVX_HIP(ctx, hipGetLastError());
    return IVX_OK;
}
