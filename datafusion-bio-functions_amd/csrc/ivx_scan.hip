// ivx_scan.hip -- sum scans used by the counting sorts (instances of ivx_scan.hpp).
#include "ivx_scan.hpp"

namespace {
template <typename V>
struct SumOp {
    using T = V;
    __host__ __device__ static T identity() { return 0; }
    __device__ static T combine(const T &a, const T &b) { return a + b; }
    __device__ static T shfl_up(const T &v, int d) { return __shfl_up(v, d, IVX_WAVE); }
};
}  // namespace

ivx_status ivx_scan_exclusive_u32(ivx_ctx *ctx, u32 *data, u64 n, const u32 *skip) { return ivxscan::exclusive<SumOp<u32>>(ctx, data, n, skip); }
ivx_status ivx_scan_exclusive_u64(ivx_ctx *ctx, u64 *data, u64 n) { return ivxscan::exclusive<SumOp<unsigned long long>>(ctx, (unsigned long long *)data, n); }

namespace {
// test-only operator that does not commute: affine maps x -> a * x + b modulo 2^32, an element holding (a, b) as a << 32 | b.
// combine(earlier, later) is "earlier, then later": (l.a * e.a, l.a * e.b + l.b).  Swapped operands anywhere in the scan
// kernels give another map.
struct AffineOp {
    using T = unsigned long long;
    __host__ __device__ static T identity() { return 1ull << 32; }
    __device__ static T combine(const T &e, const T &l)
    {
        const u32 ea = (u32)(e >> 32), eb = (u32)e, la = (u32)(l >> 32), lb = (u32)l;
        return ((T)(u32)(la * ea) << 32) | (u32)(la * eb + lb);
    }
    __device__ static T shfl_up(const T &v, int d) { return __shfl_up(v, d, IVX_WAVE); }
};
}  // namespace

// test hook (not part of include/ivx.h): scan n host elements in place on the device.  kind 0: exclusive u32 sum, 1: exclusive
// u64 sum, 2 / 3: inclusive / exclusive scan of AffineOp (u64 elements).  skip_value >= 0: that value is written to a device
// word whose address goes in as `skip`; negative: a null pointer.  Kinds 0 and 3 take `skip` (the entry points of the others
// have no such parameter).
extern "C" ivx_status ivx_debug_scan(ivx_ctx *ctx, int kind, void *data, u64 n, int skip_value)
{
    if (!ctx || kind < 0 || kind > 3 || (n && !data)) return IVX_ERR_INVALID;
    if (skip_value >= 0 && kind != 0 && kind != 3) return ctx->fail(IVX_ERR_INVALID, "debug scan: this kind takes no skip word");
    if (n == 0) return IVX_OK;
    IVX_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = n * (kind == 0 ? sizeof(u32) : sizeof(u64));
    void *d; u32 *skip = nullptr;
    IVX_TRY(ctx->get_scratch(WS_SA0, bytes, &d));
    IVX_HIP(ctx, hipMemcpyAsync(d, data, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (skip_value >= 0) {
        IVX_TRY(ctx->get_scratch(WS_T0, sizeof(u32), (void **)&skip));
        IVX_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)skip, skip_value, 1, ctx->stream));
    }
    switch (kind) {
    case 0: IVX_TRY(ivx_scan_exclusive_u32(ctx, (u32 *)d, n, skip)); break;
    case 1: IVX_TRY(ivx_scan_exclusive_u64(ctx, (u64 *)d, n)); break;
    case 2: IVX_TRY(ivxscan::inclusive<AffineOp>(ctx, (AffineOp::T *)d, n)); break;
    default: IVX_TRY(ivxscan::exclusive<AffineOp>(ctx, (AffineOp::T *)d, n, skip)); break;
    }
    IVX_HIP(ctx, hipGetLastError());
    IVX_HIP(ctx, hipMemcpyAsync(data, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    IVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return IVX_OK;
}
