// ivx_cigar.hip -- text CIGARs ("5M3D5M") to the packed ops depth() takes: the bytes of an Arrow Utf8 / LargeUtf8
// column in, cigar_offsets[n_reads + 1] (int32 BYTE offsets, element 0 = 0) and cigar_ops (u32, len << 4 | code) out.
// The reference tokenises every read in a serial byte loop (bio-function-pileup cigar.rs:141-168); here no thread walks a
// read: the tokeniser is ONE segmented scan over the BYTES of the column, in the reduce / scan of the tile sums / apply
// form of the scan over ops (ivx_depth.hip), so a 5 000-digit run or a 100 000-op read is spread over tiles like any
// other text.
//
// Per read, over bytes: every byte that is not '0'..'9' ends a token whose length is the decimal value of the digits
// immediately before it (back to the previous non-digit byte or the read's first byte); no digits give 0, a value
// >= 2^32 gives 0 (Rust's parse::<u32>() error); M I D N S H P = X emit an op with BAM's codes 0..8, every other
// non-digit byte (also one >= 0x80) only separates; digits after a read's last non-digit byte are dropped.
//
// The scan state of a byte range is (reset, v, p, ops): reset = the range holds a non-digit byte or a read's first byte;
// v = the value of the digits after the last such point (of the whole range without one), cut at 2^32; p = 10^(their
// number), cut at 2^32; ops = emitted ops.  combine(a, b) = b (ops added) when b.reset, else
// (a.reset, min(a.v * b.p + b.v, 2^32), min(a.p * b.p, 2^32), a.ops + b.ops): with the cuts it stays associative and
// min(true value, 2^32) exact (tests/test_cigar_text_cpu.py pins it against the byte loop).  The token at a non-digit
// byte is v of the EXCLUSIVE prefix, 0 if the byte is its read's first or v = 2^32.
//
//   k_cigar_check   offsets are non-negative and ascend; the first and the last come back to the host
//   k_cigar_reduce  the state of every tile of CIGAR_TILE bytes
//   (scan of the tile states; the total op count comes back to the host)
//   k_cigar_apply   every emitted op to its slot, out_offsets[r] of every read that has a byte; an op whose length does
//                   not fit 28 bits raises the lowest such read index
//   k_cigar_fill    out_offsets of the reads without bytes and of element n_reads: the value of the next read with
//                   bytes, or the total (an upper-bound search on the input offsets)
//
// A thread owns CIGAR_B = 16 consecutive bytes of the 16-byte ALIGNED grid under the text, read with one 16-byte load;
// the partial 16 bytes at the head and the tail of the text are read byte by byte, so nothing outside the text is read
// whatever the alignment of its first byte.
#include "ivx_device.hpp"
#include "ivx_scan.hpp"

namespace {

constexpr int CIGAR_B = 16;                                  // bytes per thread
constexpr int CIGAR_TILE = ivxscan::T_ * CIGAR_B;            // bytes per workgroup (4096)
constexpr u64 CCAP = 1ull << 32;
constexpr int CT = 256;

template <class OT>
__global__ __launch_bounds__(CT) void k_cigar_check(const OT *__restrict__ off, u64 n_reads, u64 *sc)
{
    const u64 i = (u64)blockIdx.x * CT + threadIdx.x;
    if (i > n_reads) return;
    const i64 o = (i64)off[i];
    if (o < 0 || (i > 0 && o < (i64)off[i - 1])) atomicOr((u32 *)(sc + SC_CIG_BAD), 1u);
    if (i == 0) sc[SC_CIG_OFF0] = (u64)o;
    if (i == n_reads) sc[SC_CIG_OFFN] = (u64)o;
}

struct CigState { u64 v, p; u32 ops, reset; };
IVX_SC_FITS(CigState, SC_CIG_IDENT, SC_ROUTE_HDR);
IVX_SC_FITS(CigState, SC_LANDING, SC_LANDING + SC_LANDING_WORDS);
struct CigScan {
    using T = CigState;
    __host__ __device__ static T identity() { T t; t.v = 0; t.p = 1; t.ops = 0; t.reset = 0; return t; }
    __device__ static T combine(const T &a, const T &b)
    {
        T r;
        r.ops = a.ops + b.ops;
        if (b.reset) { r.v = b.v; r.p = b.p; r.reset = 1; return r; }
        r.reset = a.reset;
        // min(a.v * b.p + b.v, 2^32) and min(a.p * b.p, 2^32) without leaving 64 bits: a factor at the cut decides alone
        if (a.v == 0) r.v = b.v;
        else if (a.v >= CCAP || b.p >= CCAP) r.v = CCAP;
        else { const u64 x = a.v * b.p + b.v; r.v = x > CCAP ? CCAP : x; }
        if (a.p >= CCAP || b.p >= CCAP) r.p = CCAP;
        else { const u64 x = a.p * b.p; r.p = x > CCAP ? CCAP : x; }
        return r;
    }
    __device__ static T shfl_up(const T &v, int d)
    {
        T r; r.v = __shfl_up(v.v, d, IVX_WAVE); r.p = __shfl_up(v.p, d, IVX_WAVE);
        r.ops = __shfl_up(v.ops, d, IVX_WAVE); r.reset = __shfl_up(v.reset, d, IVX_WAVE); return r;
    }
};

// combine(s, element of one byte), written out: a digit multiplies by 10, anything else starts over
__device__ __forceinline__ void push_digit(CigState &s, u32 d, bool first)
{
    if (first) { s.v = d; s.p = 10; s.reset = 1; return; }
    const u64 x = s.v * 10 + d; s.v = x > CCAP ? CCAP : x;   // (s.v <= 2^32: no overflow)
    const u64 y = s.p * 10; s.p = y > CCAP ? CCAP : y;
}
__device__ __forceinline__ void push_sep(CigState &s, bool emits) { s.v = 0; s.p = 1; s.reset = 1; s.ops += emits ? 1u : 0u; }

// M I D N S H P = X -> 0..8 (cigar.rs:155-165 and BAM's order); letters as bits / nibbles of 'A' + index
__device__ __forceinline__ bool op_code(u32 c, u32 *code)
{
    if (c == (u32)'=') { *code = 7; return true; }
    const u32 ix = c - (u32)'A';
    if (ix >= 24u || !((0x84B188u >> ix) & 1u)) return false;                  // D H I M N P S X
    const u64 lo = (2ull << 12) | (5ull << 28) | (1ull << 32) | (0ull << 48) | (3ull << 52) | (6ull << 60);    // D H I M N P
    const u64 hi = (4ull << 8) | (8ull << 28);                                                                   // S X
    *code = (u32)(((ix < 16u ? lo : hi) >> (4u * (ix & 15u))) & 15ull);
    return true;
}

template <class OT>
struct CigarText {
    const OT *off;              // [n_reads + 1]
    const u8 *txt;              // the byte at offset off[0]
    u64 n_reads, n_bytes;       // n_bytes = off[n_reads] - off[0], > 0
    i64 off0;
    u32 mis;                    // txt & 15: the thread grid starts at txt - mis
};

// the read that holds byte offset b: the last j >= lo with off[j] <= b (off[lo] <= b < off[n_reads])
template <class OT>
__device__ __forceinline__ u64 cig_read_of(const CigarText<OT> &X, i64 b, u64 lo)
{
    u64 a = lo, c = X.n_reads;
    while (c - a > 1) { const u64 mid = a + ((c - a) >> 1); if ((i64)X.off[mid] <= b) a = mid; else c = mid; }
    return a;
}

// a thread's 16 bytes: c[k] and bit k of the returned mask = byte k is inside the text
template <class OT>
__device__ __forceinline__ u32 cig_load(const CigarText<OT> &X, u64 g0, u32 (&w)[4])
{
    const u64 lo = X.mis, hi = (u64)X.mis + X.n_bytes;       // the text on the thread grid: [lo, hi)
    w[0] = w[1] = w[2] = w[3] = 0;
    if (g0 >= hi || g0 + CIGAR_B <= lo) return 0;
    if (g0 >= lo && g0 + CIGAR_B <= hi) {
        const uint4 q = *reinterpret_cast<const uint4 *>(X.txt - X.mis + g0);   // 16-byte aligned by construction
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        return 0xFFFFu;
    }
    u32 m = 0;
#pragma unroll
    for (int k = 0; k < CIGAR_B; k++) {
        const u64 g = g0 + k;
        if (g >= lo && g < hi) { w[k >> 2] |= (u32)X.txt[g - lo] << (8 * (k & 3)); m |= 1u << k; }
    }
    return m;
}

// which read a thread's bytes belong to: ONE search for the first byte, a step (or a search past a run of reads without
// bytes) for the later ones
template <class OT>
struct ReadCursor {
    u64 r; i64 cur, nxt; bool have;
    __device__ __forceinline__ void init() { r = 0; cur = 0; nxt = 0; have = false; }
    // -> is b the first byte of its read
    __device__ __forceinline__ bool at(const CigarText<OT> &X, i64 b)
    {
        if (!have) { r = cig_read_of(X, b, 0); have = true; cur = (i64)X.off[r]; nxt = (i64)X.off[r + 1]; }
        else if (b >= nxt) {
            r++; cur = nxt; nxt = (i64)X.off[r + 1];
            if (b >= nxt) { r = cig_read_of(X, b, r + 1); cur = (i64)X.off[r]; nxt = (i64)X.off[r + 1]; }
        }
        return b == cur;
    }
};

template <class OT>
__global__ __launch_bounds__(ivxscan::T_) void k_cigar_reduce(CigarText<OT> X, CigState *__restrict__ sums)
{
    using namespace ivxscan;
    __shared__ CigState lds[T_ / IVX_WAVE + 1];
    const u64 g0 = (u64)blockIdx.x * CIGAR_TILE + (u64)threadIdx.x * CIGAR_B;
    u32 w[4];
    const u32 m = cig_load(X, g0, w);
    CigState s = CigScan::identity();
    ReadCursor<OT> rc; rc.init();
#pragma unroll
    for (int k = 0; k < CIGAR_B; k++) {
        if (!((m >> k) & 1u)) continue;
        const bool first = rc.at(X, X.off0 + (i64)(g0 + k - X.mis));
        const u32 c = (w[k >> 2] >> (8 * (k & 3))) & 255u;
        const u32 d = c - (u32)'0';
        if (d < 10u) push_digit(s, d, first);
        else { u32 code; push_sep(s, op_code(c, &code)); }
    }
    CigState tot;
    block_incl<CigScan>(s, lds, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// offs[tile] = the scan over every earlier tile.  out_off / out_ops may be null on their own.
template <class OT>
__global__ __launch_bounds__(ivxscan::T_) void k_cigar_apply(CigarText<OT> X, const CigState *__restrict__ offs,
                                                             i32 *__restrict__ out_off, u32 *__restrict__ out_ops, u64 *badread)
{
    using namespace ivxscan;
    __shared__ CigState lds[T_ / IVX_WAVE + 1];
    __shared__ CigState edge[T_ / IVX_WAVE];
    const u64 g0 = (u64)blockIdx.x * CIGAR_TILE + (u64)threadIdx.x * CIGAR_B;
    u32 w[4];
    const u32 m = cig_load(X, g0, w);
    // pass 1 over the thread's bytes: its state
    CigState s = CigScan::identity();
    ReadCursor<OT> rc, rc0; rc.init(); rc0.init();          // rc0: the cursor at the thread's first byte, where pass 2 starts again
#pragma unroll
    for (int k = 0; k < CIGAR_B; k++) {
        if (!((m >> k) & 1u)) continue;
        const bool first = rc.at(X, X.off0 + (i64)(g0 + k - X.mis));
        if (!rc0.have) rc0 = rc;
        const u32 c = (w[k >> 2] >> (8 * (k & 3))) & 255u;
        const u32 d = c - (u32)'0';
        if (d < 10u) push_digit(s, d, first);
        else { u32 code; push_sep(s, op_code(c, &code)); }
    }
    CigState tot;
    CigState inc = block_incl<CigScan>(s, lds, &tot);
    CigState run = offs[blockIdx.x];
    CigState prev = CigScan::shfl_up(inc, 1);
    if (lane_id() == IVX_WAVE - 1) edge[threadIdx.x / IVX_WAVE] = inc;
    __syncthreads();
    if (threadIdx.x == 0) prev = CigScan::identity();
    else if (lane_id() == 0) prev = edge[threadIdx.x / IVX_WAVE - 1];
    run = CigScan::combine(run, prev);
    // pass 2: `run` is the exclusive prefix of byte k (no second search: the cursor is back at the first byte's read)
    rc = rc0;
    u64 bad = ~0ull;
#pragma unroll
    for (int k = 0; k < CIGAR_B; k++) {
        if (!((m >> k) & 1u)) continue;
        const bool first = rc.at(X, X.off0 + (i64)(g0 + k - X.mis));
        const u32 c = (w[k >> 2] >> (8 * (k & 3))) & 255u;
        const u32 d = c - (u32)'0';
        if (first && out_off) out_off[rc.r] = (i32)(4u * run.ops);
        if (d < 10u) { push_digit(run, d, first); continue; }
        u32 code;
        const bool emits = op_code(c, &code);
        if (emits) {
            const u64 len = first || run.v >= CCAP ? 0ull : run.v;
            if (len >= (1ull << 28)) bad = rc.r < bad ? rc.r : bad;
            else if (out_ops) out_ops[run.ops] = ((u32)len << 4) | code;
        }
        push_sep(run, emits);
    }
    if (bad != ~0ull) atomicMin((unsigned long long *)badread, (unsigned long long)bad);
}

// reads without bytes, and element n_reads: the offset of the next read with bytes, or the total
template <class OT>
__global__ __launch_bounds__(CT) void k_cigar_fill(const OT *__restrict__ off, u64 n_reads, i32 *__restrict__ out_off, u32 total_ops)
{
    const u64 i = (u64)blockIdx.x * CT + threadIdx.x;
    if (i > n_reads) return;
    const i64 o = (i64)off[i];
    if (i < n_reads && (i64)off[i + 1] > o) return;          // has bytes: k_cigar_apply wrote it
    u64 a = i, c = n_reads + 1;                              // off[a] <= o < off[c] (c = n_reads + 1: none)
    while (c - a > 1) { const u64 mid = a + ((c - a) >> 1); if ((i64)off[mid] <= o) a = mid; else c = mid; }
    // a < n_reads: off[a] == o < off[a + 1], read a has bytes and i < a
    out_off[i] = c > n_reads ? (i32)(4u * total_ops) : out_off[a];
}

template <class OT>
ivx_status cigar_count_t(ivx_ctx *ctx, const OT *off, ivx_cigar_plan *P)
{
    using namespace ivxscan;
    hipStream_t st = ctx->stream;
    const u64 nblk = (P->mis + P->n_bytes + CIGAR_TILE - 1) / CIGAR_TILE;
    CigState *tsum;                                         // [0] = identity, [1 + t] = the scan up to and including tile t
    IVX_TRY(ctx->get_scratch(WS_SCAN0, (nblk + 1) * sizeof(CigState), (void **)&tsum));
    const CigState id = CigScan::identity();
    CigState *hid = ctx->hword<CigState>(SC_CIG_IDENT);     // pinned: the async copy may read it later
    *hid = id;
    IVX_HIP(ctx, hipMemcpyAsync(tsum, hid, sizeof(CigState), hipMemcpyHostToDevice, st));
    CigarText<OT> X{off, P->txt, P->n_reads, P->n_bytes, P->off0, P->mis};
    hipLaunchKernelGGL((k_cigar_reduce<OT>), dim3((u32)nblk), dim3(T_), 0, st, X, tsum + 1);
    IVX_TRY((scan_rec<CigScan, true>(ctx, tsum + 1, nblk, 1, WS_SCAN0)));
    IVX_HIP(ctx, hipGetLastError());
    CigState tot;
    IVX_TRY(ctx->fetch_wait((const CigState *)tsum + nblk, st, &tot));
    P->n_ops = tot.ops;
    P->tsum = tsum; P->nblk = nblk;
    return IVX_OK;
}

template <class OT>
ivx_status cigar_write_t(ivx_ctx *ctx, const OT *off, const ivx_cigar_plan &P, i32 *out_off, u32 *out_ops)
{
    using namespace ivxscan;
    hipStream_t st = ctx->stream;
    u64 *badread = ctx->dword(SC_CIG_BADREAD);
    IVX_HIP(ctx, hipMemsetAsync(badread, 0xFF, sizeof(u64), st));
    CigarText<OT> X{off, P.txt, P.n_reads, P.n_bytes, P.off0, P.mis};
    hipLaunchKernelGGL((k_cigar_apply<OT>), dim3((u32)P.nblk), dim3(T_), 0, st, X, (const CigState *)P.tsum, out_off, out_ops, badread);
    if (out_off)
        hipLaunchKernelGGL((k_cigar_fill<OT>), dim3((u32)((P.n_reads + CT) / CT)), dim3(CT), 0, st, off, P.n_reads, out_off, (u32)P.n_ops);
    IVX_HIP(ctx, hipGetLastError());
    u64 read;
    IVX_TRY(ctx->fetch_wait(SC_CIG_BADREAD, st, &read));
    if (read != ~0ull)
        return ctx->fail(IVX_ERR_INVALID, "cigar: an op length of 2^28 or more cannot be packed (read " + std::to_string(read) + ")");
    return IVX_OK;
}

}  // namespace

// Passes (a) to (c): the checks and the op count.  `text` is the column's data buffer (the byte at offset 0) unless
// text_at_off0, when it is the byte at offset text_offsets[0] (a staged copy of the extent the offsets name).
ivx_status ivx_cigar_count(ivx_ctx *ctx, int large, const void *text_offsets, const u8 *text, bool text_at_off0, u64 n_reads,
                           ivx_cigar_plan *P)
{
    P->large = large; P->off = text_offsets; P->n_reads = n_reads; P->n_bytes = 0; P->n_ops = 0; P->nblk = 0; P->tsum = nullptr;
    P->txt = nullptr; P->off0 = 0; P->mis = 0;
    if (n_reads == 0) return IVX_OK;
    hipStream_t st = ctx->stream;
    IVX_HIP(ctx, hipMemsetAsync(ctx->dword(SC_CIG_BAD), 0, SC_CIG_CHECK_WORDS * sizeof(u64), st));
    const u32 grid = (u32)((n_reads + CT) / CT);
    if (large) hipLaunchKernelGGL((k_cigar_check<i64>), dim3(grid), dim3(CT), 0, st, (const i64 *)text_offsets, n_reads, ctx->d_scalars);
    else hipLaunchKernelGGL((k_cigar_check<i32>), dim3(grid), dim3(CT), 0, st, (const i32 *)text_offsets, n_reads, ctx->d_scalars);
    IVX_HIP(ctx, hipGetLastError());
    IVX_HIP(ctx, ctx->fetch(SC_CIG_BAD, st, SC_CIG_CHECK_WORDS));
    IVX_HIP(ctx, hipStreamSynchronize(st));
    const u64 off0 = *ctx->hword(SC_CIG_OFF0), offn = *ctx->hword(SC_CIG_OFFN);
    if (*ctx->hword<u32>(SC_CIG_BAD)) return ctx->fail(IVX_ERR_INVALID, "cigar: text offsets must ascend and be non-negative");
    const u64 nb = offn - off0;
    if (nb >= CCAP) return ctx->fail(IVX_ERR_INVALID, "cigar: 2^32 or more bytes of CIGAR text in one call");
    if (nb == 0) return IVX_OK;
    if (!text) return ctx->fail(IVX_ERR_INVALID, "cigar: null text buffer");
    P->n_bytes = nb; P->off0 = (i64)off0;
    P->txt = text_at_off0 ? text : text + off0;
    P->mis = (u32)((uintptr_t)P->txt & 15u);
    IVX_TRY(large ? cigar_count_t<i64>(ctx, (const i64 *)text_offsets, P) : cigar_count_t<i32>(ctx, (const i32 *)text_offsets, P));
    if (P->n_ops > 0x1FFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "cigar: more than 2^29-1 ops in one call");
    return IVX_OK;
}

// Passes (d) and (e): out_off [n_reads + 1] and out_ops [P.n_ops], either may be null
ivx_status ivx_cigar_write(ivx_ctx *ctx, const ivx_cigar_plan &P, i32 *out_off, u32 *out_ops)
{
    if (P.n_reads == 0) return IVX_OK;
    if (P.n_bytes == 0) {                                   // every read is empty
        if (out_off) IVX_HIP(ctx, hipMemsetAsync(out_off, 0, (P.n_reads + 1) * sizeof(i32), ctx->stream));
        return IVX_OK;
    }
    return P.large ? cigar_write_t<i64>(ctx, (const i64 *)P.off, P, out_off, out_ops)
                   : cigar_write_t<i32>(ctx, (const i32 *)P.off, P, out_off, out_ops);
}
