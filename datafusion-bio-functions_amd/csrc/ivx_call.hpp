// ivx_call.hpp -- the protocol of one public call, for ivx_capi.hip alone (hence the anonymous namespace): the shared head
// of the argument checks, staging of host columns into the context's scratch, the timing bracket around the device call,
// the copy-back and the host-mode synchronise.  An entry point says what its columns are; which slot, how many bytes
// and what goes back where follow from that.
#pragma once
#include "ivx_internal.hpp"
#include <chrono>
#include <new>

namespace {

// stage one input column: host -> device scratch, or pass the device pointer through
template <typename T>
ivx_status stage_in(ivx_ctx *ctx, int mem, int slot, const T *src, u64 n, const T **dev)
{
    if (src == nullptr) { *dev = nullptr; return IVX_OK; }
    if (mem == IVX_MEM_DEVICE) { *dev = src; return IVX_OK; }
    T *d;
    IVX_TRY(ctx->get_scratch(slot, (size_t)n * sizeof(T), (void **)&d));
    if (n) IVX_HIP(ctx, hipMemcpyAsync(d, src, (size_t)n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    *dev = d;
    return IVX_OK;
}

// output column: device scratch (host mode) or the caller's device pointer
template <typename T>
ivx_status stage_out(ivx_ctx *ctx, int mem, int slot, T *dst, u64 n, T **dev)
{
    if (dst == nullptr) { *dev = nullptr; return IVX_OK; }
    if (mem == IVX_MEM_DEVICE) { *dev = dst; return IVX_OK; }
    T *d;
    IVX_TRY(ctx->get_scratch(slot, (size_t)n * sizeof(T), (void **)&d));
    *dev = d;
    return IVX_OK;
}

template <typename T>
ivx_status copy_out(ivx_ctx *ctx, int mem, T *dst, const T *dev, u64 n)
{
    if (mem == IVX_MEM_DEVICE || dst == nullptr || n == 0) return IVX_OK;
    IVX_HIP(ctx, hipMemcpyAsync(dst, dev, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return IVX_OK;
}

// the context's two timing events around a device call (ivx_ctx_last_kernel_ms)
struct KernelTimer {
    ivx_ctx *c;
    explicit KernelTimer(ivx_ctx *ctx) : c(ctx) { (void)hipEventRecord(c->ev0, c->stream); c->last_ms = -1.0; }
    ~KernelTimer() { (void)hipEventRecord(c->ev1, c->stream); }
};

// One public call, built from (ctx, mem).  Staging errors are sticky: after the first one in() / out() return null and do
// nothing, run() does not start the device call, back() copies nothing and finish() returns the error -- an entry point
// stages its columns in one run of lines and checks once.  No heap, no virtual call: a frame sits inside the join's step.
//
// What a frame does NOT decide is whether the call drops the plans a sizing call left in the context (ivx_sub_plan,
// ivx_join_plan): an entry point that does says so with drop_plans() / drop_join_plan(); one that does not drops a plan
// only by taking a scratch slot the plan lives in (ivx_ctx::get_scratch).
struct Frame {
    ivx_ctx *const ctx;
    const int mem;
    ivx_status st = IVX_OK;

    Frame(ivx_ctx *c, int m) : ctx(c), mem(m) {}
    Frame(const Frame &) = delete;
    ~Frame()
    {
        if (!metered) return;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        (build ? ctx->metrics.build_time : ctx->metrics.join_time) += ms;
    }

    // ---- the head of the argument checks, in the order every entry point has them: the context; the call's scalar result
    // (null: `what` is the error; else zeroed); then the entry's own checks up to check_mem()
    ivx_status begin() { return ctx ? IVX_OK : IVX_ERR_INVALID; }
    template <typename S> ivx_status begin(S *scalar, const char *what)
    {
        if (!ctx) return IVX_ERR_INVALID;
        if (!scalar) return ctx->fail(IVX_ERR_INVALID, what);
        *scalar = S{};
        return IVX_OK;
    }
    ivx_status check_mem() { return mem == IVX_MEM_HOST || mem == IVX_MEM_DEVICE ? IVX_OK : ctx->fail(IVX_ERR_INVALID, "bad mem"); }
    ivx_status enter() { IVX_TRY(begin()); return check_mem(); }
    template <typename S> ivx_status enter(S *scalar, const char *what) { IVX_TRY(begin(scalar, what)); return check_mem(); }

    // the context's device made current, once per frame: the first staged column or run() does it, an entry point that
    // touches the stream before either calls it itself
    ivx_status device()
    {
        if (st == IVX_OK && !on_device) {
            const hipError_t e = hipSetDevice(ctx->device);
            if (e != hipSuccess) st = ctx->fail_hip("hipSetDevice(ctx->device)", e);
            on_device = true;
        }
        return st;
    }

    void drop_plans() { ctx->sub_plan.valid = false; ctx->join_plan.valid = false; }
    void drop_join_plan() { ctx->join_plan.valid = false; }

    // ---- BuildProbeJoinMetrics bookkeeping of the call (host wall time up to the frame's end, as the reference's timers)
    void meter(bool is_build, u64 rows)
    {
        metered = true; build = is_build; t0 = std::chrono::steady_clock::now();
        if (build) { ctx->metrics.build_input_batches++; ctx->metrics.build_input_rows += rows; }
        else { ctx->metrics.input_batches++; ctx->metrics.input_rows += rows; }
    }
    void rows_out(u64 rows) { if (rows) { ctx->metrics.output_batches++; ctx->metrics.output_rows += rows; } }

    // ---- input columns: the caller's own pointer (device mode) or staged scratch (host mode); null in, null out.  Slots
    // go in the fixed order IN_ORDER; a column that sits elsewhere names its slot with in_at().  No slot twice in a frame.
    template <typename T> const T *in(const T *src, u64 n) { return in_at(n_in < N_IN ? IN_ORDER[n_in++] : -1, src, n); }
    template <typename T> const T *in_at(int slot, const T *src, u64 n)
    {
        const T *d = nullptr;
        if (device() == IVX_OK && take(slot)) st = stage_in(ctx, mem, slot, src, n, &d);
        return d;
    }
    // device scratch that is no column of the caller's (host mode: an area several small buffers are packed into)
    ivx_status scratch_at(int slot, size_t bytes, void **out)
    {
        if (device() == IVX_OK && take(slot)) st = ctx->get_scratch(slot, bytes, out);
        return st;
    }

    // ---- output columns, WS_OUT_A .. WS_OUT_H in order: as in(), and the frame remembers what to copy back where
    template <typename T> T *out(T *dst, u64 cap)
    {
        T *d = nullptr;
        const int slot = WS_OUT_A + n_out++;
        if (device() == IVX_OK && take(slot <= WS_OUT_H ? slot : -1)) st = stage_out(ctx, mem, slot, dst, cap, &d);
        if (st == IVX_OK && mem == IVX_MEM_HOST && dst && cap) outs[n_staged++] = Staged{dst, d, (u32)sizeof(T), cap, false};
        return d;
    }
    // a bitmap the device ORs into: the caller's own words (device mode), or a ZEROED scratch bitmap that or_back() copies
    // to the host and ORs into the caller's words (the caller's set bits survive)
    u32 *out_or(u32 *bits, u64 nw)
    {
        if (device() != IVX_OK) return nullptr;
        if (mem == IVX_MEM_DEVICE) return bits;
        u32 *d = nullptr;
        if (scratch_at(WS_OUT_A + n_out++, (size_t)nw * sizeof(u32), (void **)&d) != IVX_OK) return nullptr;
        if (nw && hip(hipMemsetAsync(d, 0, (size_t)nw * sizeof(u32), ctx->stream), "hipMemsetAsync(marks)") == IVX_OK)
            outs[n_staged++] = Staged{bits, d, (u32)sizeof(u32), nw, false};
        return d;
    }

    // ---- the one device call, between the context's two timing events; not started after a staging error.  Its status
    // is the caller's to read (a short buffer still sets the call's scalars): it is not sticky.
    template <typename F> ivx_status run(F &&device_call)
    {
        if (device() != IVX_OK) return st;
        KernelTimer t(ctx);
        return device_call();
    }

    // ---- copy-back (host mode; nothing in device mode): `count` elements of a staged output, by default all it was staged
    // with.  The element type is the one of out(): another one is an error, as is an output that finish() finds forgotten.
    template <typename T> void back(T *dst, u64 count)
    {
        Staged *o = find(dst);
        if (o && (o->elem != sizeof(T) || count > o->cap)) { misuse("copy-back does not match the staged output"); return; }
        if (o) copy(*o, count);
    }
    template <typename T> void back(T *dst) { if (Staged *o = find(dst)) copy(*o, o->cap); }
    void back_all() { for (int i = 0; i < n_staged; i++) copy(outs[i], outs[i].cap); }
    void back_all(u64 count) { for (int i = 0; i < n_staged; i++) copy(outs[i], count < outs[i].cap ? count : outs[i].cap); }
    void or_back(u32 *bits)
    {
        Staged *o = find(bits);
        if (!o || st != IVX_OK) return;
        std::vector<u32> got;
        try { got.resize((size_t)o->cap); } catch (const std::bad_alloc &) { st = ctx->fail(IVX_ERR_OOM, "host allocation failed"); return; }
        if (hip(hipMemcpyAsync(got.data(), o->dev, (size_t)o->cap * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(marks)") != IVX_OK) return;
        if (hip(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize(ctx->stream)") != IVX_OK) return;
        for (u64 w = 0; w < o->cap; w++) bits[w] |= got[w];
        o->done = true;
    }
    // an output the call keeps from the caller on purpose
    template <typename T> void withhold(T *dst) { if (Staged *o = find(dst)) o->done = true; }

    // ---- the end of a call that got this far: host mode returns with the caller's buffers filled
    ivx_status finish()
    {
        for (int i = 0; i < n_staged && st == IVX_OK; i++)
            if (!outs[i].done) misuse("a staged output was not copied back");
        if (st == IVX_OK && mem == IVX_MEM_HOST) hip(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize(ctx->stream)");
        return st;
    }

private:
    static constexpr int N_IN = 11, N_OUT = 8;
    static constexpr int IN_ORDER[N_IN] = {WS_IN_KEY, WS_IN_START, WS_IN_END, WS_IN2_KEY, WS_IN2_START, WS_IN2_END,
                                           WS_IN3_KEY, WS_IN3_START, WS_IN3_END, WS_IN3_WEIGHT, WS_IN_KEYLEN};
    struct Staged { void *host; const void *dev; u32 elem; u64 cap; bool done; };
    Staged outs[N_OUT];
    int n_in = 0, n_out = 0, n_staged = 0;
    u64 taken = 0;                      // scratch slots this frame has handed out (bit per slot)
    bool on_device = false, metered = false, build = false;
    std::chrono::steady_clock::time_point t0;

    void misuse(const char *what) { st = ctx->fail(IVX_ERR_INVALID, std::string("internal error: ") + what); }
    ivx_status hip(hipError_t e, const char *what) { if (e != hipSuccess && st == IVX_OK) st = ctx->fail_hip(what, e); return st; }
    bool take(int slot)
    {
        if (slot < 0 || ((taken >> slot) & 1)) { misuse("a scratch slot taken twice, or more columns than slots"); return false; }
        taken |= 1ull << slot;
        return true;
    }
    Staged *find(const void *host)
    {
        for (int i = 0; i < n_staged; i++) if (outs[i].host == host) return &outs[i];
        return nullptr;
    }
    void copy(Staged &o, u64 count)
    {
        if (st != IVX_OK) return;
        st = copy_out(ctx, mem, (u8 *)o.host, (const u8 *)o.dev, count * o.elem);
        o.done = true;
    }
};

}  // namespace
