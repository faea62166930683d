// ivx_capi.hip -- extern "C" entry points of libivx_hip.so (see include/ivx.h).
// Host-side plumbing only: argument checks, staging of host buffers, stream and
// scratch management.  All arithmetic happens in the HIP kernels.
#include "ivx_internal.hpp"
#include "ivx_call.hpp"
#include "ivx_where.hpp"
#include <cstdlib>
#include <atomic>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <condition_variable>
#include <deque>

// ------------------------------------------------------------- ctx helpers

void ivx_ctx::join_tail()
{
    if (!tail_pending) return;
    (void)hipStreamWaitEvent(stream, tail_ev, 0);
    tail_pending = false;
}

ivx_status ivx_ctx::get_scratch(int slot, size_t bytes, void **out)
{
    // a build tail still running on the aux stream uses the build's scratch (cell ids, ranks, scan partials): whoever asks
    // for scratch is ordered behind it first -- except for the slots a probe's routing pass takes, which the tail never
    // touches: that pass is what runs beside the tail
    if (tail_pending && slot != WS_SORTHIST && slot != WS_T0 && slot != WS_T1 && slot != WS_T2) join_tail();
    ivx_buf &b = scratch[slot];
    if (sub_plan.valid && ((sub_plan.slots >> slot) & 1)) sub_plan.valid = false;
    if (join_plan.valid && ((join_plan.rows.slots >> slot) & 1)) join_plan.valid = false;
    if (bytes < 256) bytes = 256;
    if (b.cap < bytes) {
        size_t want = bytes + bytes / 8;
        if (mem_limit) {
            const u64 others = reserved() - b.cap;
            if (others + bytes > mem_limit)
                return fail(IVX_ERR_OOM, "Resources exhausted: failed to reserve " + std::to_string(bytes) + " bytes of device scratch (" +
                                         std::to_string(others) + " bytes reserved, limit " + std::to_string(mem_limit) + ")");
            if (others + want > mem_limit) want = bytes;
        }
        if (b.p) { (void)hipStreamSynchronize(stream); if (aux) (void)hipStreamSynchronize(aux); (void)hipFree(b.p); b.p = nullptr; scratch_bytes -= b.cap; b.cap = 0; }
        hipError_t e = hipMalloc(&b.p, want);
        if (e != hipSuccess) { want = bytes; e = hipMalloc(&b.p, want); }
        if (e != hipSuccess) { b.p = nullptr; return fail_hip("hipMalloc(scratch)", e); }
        b.cap = want; scratch_bytes += want;
    }
    *out = b.p;
    return IVX_OK;
}

ivx_status ivx_ctx::get_pinned(int slot, size_t bytes, void **out)
{
    ivx_buf &b = pinned[slot];
    if (bytes < 256) bytes = 256;
    if (b.cap < bytes) {
        if (b.p) { (void)hipStreamSynchronize(stream); (void)hipHostFree(b.p); b.p = nullptr; b.cap = 0; }
        hipError_t e = hipHostMalloc(&b.p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) { b.p = nullptr; return fail_hip("hipHostMalloc", e); }
        b.cap = bytes;
    }
    *out = b.p;
    return IVX_OK;
}

// Index buffers are recycled through a small per-process pool: IntervalJoinExec builds one
// index per query/partition and drops it, and hipMalloc/hipFree cost more than the build kernels.
namespace {
struct PoolBuf { void *p; size_t cap; int device; };
std::mutex g_pool_mu;
std::vector<PoolBuf> g_pool;
constexpr size_t POOL_MAX_BUFS = 96;

void *pool_take(int device, size_t bytes, size_t *cap)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    size_t best = g_pool.size();
    for (size_t i = 0; i < g_pool.size(); i++) {
        const PoolBuf &b = g_pool[i];
        if (b.device != device || b.cap < bytes || b.cap > 2 * bytes + 4096) continue;
        if (best == g_pool.size() || b.cap < g_pool[best].cap) best = i;
    }
    if (best == g_pool.size()) return nullptr;
    void *p = g_pool[best].p;
    *cap = g_pool[best].cap;
    g_pool.erase(g_pool.begin() + best);
    return p;
}

void pool_give(int device, void *p, size_t cap)
{
    void *drop = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        g_pool.push_back({p, cap, device});
        if (g_pool.size() > POOL_MAX_BUFS) { drop = g_pool.front().p; g_pool.erase(g_pool.begin()); }
    }
    if (drop) (void)hipFree(drop);
}

void pool_drop(int device)
{
    std::vector<void *> drop;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (size_t i = 0; i < g_pool.size();)
            if (g_pool[i].device == device) { drop.push_back(g_pool[i].p); g_pool.erase(g_pool.begin() + i); }
            else i++;
    }
    for (void *p : drop) (void)hipFree(p);
}
}  // namespace

ivx_status ivx_index_alloc(ivx_ctx *ctx, ivx_index *ix, size_t bytes, void **out)
{
    if (bytes < 256) bytes = 256;
    if (ctx->mem_limit && ctx->reserved() + bytes > ctx->mem_limit)
        return ctx->fail(IVX_ERR_OOM, "Resources exhausted: failed to reserve " + std::to_string(bytes) + " bytes for the index (" +
                                      std::to_string(ctx->reserved()) + " bytes reserved, limit " + std::to_string(ctx->mem_limit) + ")");
    ctx->building_bytes += bytes;
    size_t cap = bytes;
    void *p = pool_take(ctx->device, bytes, &cap);
    if (!p) {
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return ctx->fail_hip("hipMalloc(index)", e);
    }
    ix->allocs.push_back(p);
    ix->alloc_caps.push_back(cap);
    ix->bytes += bytes;
    *out = p;
    return IVX_OK;
}

namespace {

// the head of every probe call (the frame's begin() and check_mem() around the index checks), then the device
ivx_status check_probe_args(Frame &f, const ivx_index *ix, int kind, const void *s, const void *e, u64 n, bool defer_ready = false)
{
    IVX_TRY(f.begin());
    ivx_ctx *ctx = f.ctx;
    if (!ix) return ctx->fail(IVX_ERR_INVALID, "null index");
    if (ix->kind != kind) return ctx->fail(IVX_ERR_UNSUPPORTED, "index kind does not match this probe");
    if (ix->device != ctx->device) return ctx->fail(IVX_ERR_INVALID, "index lives on another device");
    IVX_TRY(f.check_mem());
    if (n && (!s || !e)) return ctx->fail(IVX_ERR_INVALID, "null coordinate column");
    if (n > 0xFFFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "probe batch exceeds UInt32 index capacity");
    IVX_TRY(f.device());
    // an index whose build tail ran beside other work is complete behind its `ready` event: this context's stream is
    // ordered behind it here, unless the caller takes care of that itself (the region path: after its routing pass)
    if (ix->ready != nullptr && !defer_ready) IVX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ix->ready, 0));
    return IVX_OK;
}

// the threshold of a *_where entry (include/ivx_where.h), behind the entry's own head: refused by its rule's text, else *asked
// says whether it filters at all (a call that asks nothing is the plain call) and *p is what the kernels take
ivx_status check_where(ivx_ctx *ctx, const ivx_overlap_where *w, WherePred *p, bool *asked)
{
    if (const char *bad = where_invalid(w)) return ctx->fail(IVX_ERR_INVALID, bad);
    *p = where_pred(w);
    *asked = where_asks(w);
    return IVX_OK;
}

// An index object in the making (an index, a depth profile): what its device buffers take is counted in
// ctx->building_bytes until index_commit
ivx_status index_new(ivx_ctx *ctx, int kind, u64 n, u32 nkeys, ivx_index **out)
{
    ivx_index *ix = new (std::nothrow) ivx_index();
    if (!ix) return ctx->fail(IVX_ERR_OOM, "host allocation failed");
    static std::atomic<u64> next_serial{1};
    ix->serial = next_serial.fetch_add(1);
    ix->kind = kind; ix->device = ctx->device; ix->n = n; ix->nkeys = nkeys;
    ctx->building_bytes = 0;
    *out = ix;
    return IVX_OK;
}

// ... built (st = what the build said): wait for the device, `what` being the error if that fails; then the object is the
// caller's, or freed
ivx_status index_commit(ivx_ctx *ctx, ivx_index *ix, ivx_status st, const char *what, ivx_index **out)
{
    if (st == IVX_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) st = ctx->fail(IVX_ERR_HIP, what);
    ctx->building_bytes = 0;
    if (st != IVX_OK) {
        // a build that was refused half-way has queued kernels that write the buffers it did get, and ivx_index_free hands
        // those to the pool every context of the process draws from: another context's build could take them on its own
        // stream while they are still being written.  Wait for this context's streams first -- on this path only
        (void)hipStreamSynchronize(ctx->stream);
        if (ctx->aux) (void)hipStreamSynchronize(ctx->aux);
        ivx_index_free(ix);
        return st;
    }
    if (ix->kind == IVX_KIND_DEPTH_PROFILE) ix->n = ix->dp.steps;
    // the finished index stays reserved against the context's limit until ivx_index_free (the reference holds the
    // build side's MemoryReservation until the join stream ends, interval_join.rs:614-639)
    ix->owner_bytes = ctx->live_index_bytes;
    ix->owner_bytes->fetch_add(ix->bytes, std::memory_order_relaxed);
    ctx->metrics.build_mem_used += ix->bytes;
    *out = ix;
    return IVX_OK;
}

}  // namespace

// ------------------------------------------------------------------ ctx

extern "C" const char *ivx_version(void) { return "ivx-hip 0.1 (gfx950)"; }

// the build tail's stream: highest priority, so that its short kernels take the workgroup slots a long routing kernel frees
// first and are done long before that kernel is
static bool create_aux_stream(hipStream_t *out)
{
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hipStreamCreateWithPriority(out, hipStreamNonBlocking, hi) == hipSuccess) return true;
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking) == hipSuccess;
}

extern "C" ivx_status ivx_ctx_create(int device_ordinal, ivx_ctx **out)
{
    if (!out) return IVX_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return IVX_ERR_NO_DEVICE;   // no CPU fallback
    if (device_ordinal < 0 || device_ordinal >= ndev) return IVX_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) return IVX_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return IVX_ERR_NO_DEVICE;       // code objects are gfx950 only
    ivx_ctx *c = new (std::nothrow) ivx_ctx();
    if (!c) return IVX_ERR_OOM;
    c->device = device_ordinal;
    bool ok = hipSetDevice(device_ordinal) == hipSuccess &&
              hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) == hipSuccess &&
              create_aux_stream(&c->aux) &&
              hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&c->tail_ev, hipEventDisableTiming) == hipSuccess &&
              hipEventCreate(&c->ev0) == hipSuccess && hipEventCreate(&c->ev1) == hipSuccess &&
              hipMalloc((void **)&c->d_scalars, SC_DEVICE_WORDS * sizeof(u64)) == hipSuccess &&
              // mapped and coherent: a kernel's stores through hd_scalars are in h_scalars once the kernel has completed
              hipHostMalloc((void **)&c->h_scalars, SC_HOST_WORDS * sizeof(u64), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
              hipHostGetDevicePointer((void **)&c->hd_scalars, c->h_scalars, 0) == hipSuccess;
    if (!ok) { ivx_ctx_free(c); return IVX_ERR_HIP; }
    memset(c->h_scalars, 0, SC_HOST_WORDS * sizeof(u64));
    c->stream = c->own_stream;
    if (const char *e = getenv("IVX_BUILD_OVERLAP")) c->overlap = e[0] == '1';
    *out = c;
    return IVX_OK;
}

extern "C" void ivx_ctx_free(ivx_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->aux) (void)hipStreamSynchronize(c->aux);
    for (auto &b : c->scratch) if (b.p) (void)hipFree(b.p);
    for (auto &b : c->pinned) if (b.p) (void)hipHostFree(b.p);
    if (c->d_scalars) (void)hipFree(c->d_scalars);
    if (c->h_scalars) (void)hipHostFree(c->h_scalars);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->aux) (void)hipStreamDestroy(c->aux);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->tail_ev) (void)hipEventDestroy(c->tail_ev);
    delete c;
}

extern "C" const char *ivx_last_error(const ivx_ctx *c) { return c ? c->err.c_str() : "null ctx"; }

extern "C" ivx_status ivx_ctx_set_stream(ivx_ctx *c, void *hip_stream)
{
    if (!c) return IVX_ERR_INVALID;
    if (c->tail_pending) { (void)hipStreamSynchronize(c->aux); c->tail_pending = false; }
    c->stream = (hipStream_t)hip_stream;
    return IVX_OK;
}

extern "C" ivx_status ivx_ctx_use_own_stream(ivx_ctx *c)
{
    if (!c) return IVX_ERR_INVALID;
    if (c->tail_pending) { (void)hipStreamSynchronize(c->aux); c->tail_pending = false; }
    c->stream = c->own_stream;
    return IVX_OK;
}

extern "C" ivx_status ivx_ctx_set_build_overlap(ivx_ctx *c, int on)
{
    if (!c) return IVX_ERR_INVALID;
    c->overlap = on != 0;
    return IVX_OK;
}

extern "C" ivx_status ivx_ctx_synchronize(ivx_ctx *c)
{
    if (!c) return IVX_ERR_INVALID;
    if (c->tail_pending) { IVX_HIP(c, hipStreamSynchronize(c->aux)); c->tail_pending = false; }
    IVX_HIP(c, hipStreamSynchronize(c->stream));
    return IVX_OK;
}

extern "C" ivx_status ivx_ctx_metrics(const ivx_ctx *c, ivx_metrics *out)
{
    if (!c || !out) return IVX_ERR_INVALID;
    *out = c->metrics;
    return IVX_OK;
}

extern "C" void ivx_ctx_reset_metrics(ivx_ctx *c) { if (c) c->metrics = ivx_metrics{}; }

extern "C" ivx_status ivx_ctx_set_memory_limit(ivx_ctx *c, uint64_t bytes)
{
    if (!c) return IVX_ERR_INVALID;
    c->mem_limit = bytes;
    return IVX_OK;
}

extern "C" uint64_t ivx_ctx_reserved_bytes(const ivx_ctx *c) { return c ? c->reserved() : 0; }

// Scratch back to the device: the reference's build-side reservation is returned when the stream ends
// (interval_join.rs:614-639); a context that served a 10^9-row call would otherwise keep ~100 GB for good.
extern "C" ivx_status ivx_ctx_trim(ivx_ctx *c, uint64_t keep_bytes)
{
    if (!c) return IVX_ERR_INVALID;
    IVX_HIP(c, hipSetDevice(c->device));
    IVX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->aux) { IVX_HIP(c, hipStreamSynchronize(c->aux)); c->tail_pending = false; }
    c->sub_plan.valid = false; c->join_plan.valid = false;      // both live in scratch slots
    while (c->scratch_bytes > keep_bytes) {
        int big = -1;
        for (int i = 0; i < IVX_NSCRATCH; i++)
            if (c->scratch[i].p && (big < 0 || c->scratch[i].cap > c->scratch[big].cap)) big = i;
        if (big < 0) break;
        IVX_HIP(c, hipFree(c->scratch[big].p));
        c->scratch_bytes -= c->scratch[big].cap;
        c->scratch[big] = ivx_buf{};
    }
    pool_drop(c->device);                                       // recycled index buffers of freed indexes on this device, too
    return IVX_OK;
}

extern "C" double ivx_ctx_last_kernel_ms(const ivx_ctx *cc)
{
    ivx_ctx *c = const_cast<ivx_ctx *>(cc);
    if (!c) return -1.0;
    if (c->last_ms < 0.0) {
        float ms = 0.f;
        if (hipEventSynchronize(c->ev1) == hipSuccess && hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) c->last_ms = ms;
    }
    return c->last_ms;
}

// ---------------------------------------------------------------- index

extern "C" ivx_status ivx_index_build(ivx_ctx *ctx, int kind, int mem, const uint32_t *key, const int32_t *start,
                                      const int32_t *end, uint64_t n, uint32_t n_keys, ivx_index **out)
{
    Frame f(ctx, mem);
    IVX_TRY(f.begin(out, "null out"));
    if (kind < IVX_KIND_OVERLAP || kind > IVX_KIND_NEAREST) return ctx->fail(IVX_ERR_INVALID, "bad index kind");
    IVX_TRY(f.check_mem());
    if (n && (!start || !end)) return ctx->fail(IVX_ERR_INVALID, "null coordinate column");
    if (n > 0xFFFFFFFEull) return ctx->fail(IVX_ERR_INVALID, "build side exceeds UInt32 index capacity");   // interval_join.rs:759
    if (n_keys == 0) n_keys = 1;
    if (!key) n_keys = 1;
    if (kind == IVX_KIND_NEAREST && n >= 0x80000000ull) return ctx->fail(IVX_ERR_INVALID, "nearest index: more than 2^31-1 rows");
    IVX_TRY(f.device());
    ivx_index *ix;
    IVX_TRY(index_new(ctx, kind, n, n_keys, &ix));
    f.meter(true, n);
    const u32 *dk = f.in(key, n);
    const i32 *ds = f.in(start, n), *de = f.in(end, n);
    const ivx_status st = f.run([&]() -> ivx_status {
        switch (kind) {
        // (overlapped tail: device-resident columns only -- staged host columns live in scratch the next call reuses)
        case IVX_KIND_OVERLAP: return ivx_join_build(ctx, ix, dk, ds, de, n, mem == IVX_MEM_DEVICE);
        case IVX_KIND_COUNT: return ivx_count_build(ctx, ix, dk, ds, de, n);
        case IVX_KIND_COVERAGE: return ivx_coverage_build(ctx, ix, dk, ds, de, n);
        default: return ivx_nearest_build(ctx, ix, dk, ds, de, n);
        }
    });
    return index_commit(ctx, ix, st, "index build failed on device", out);
}

extern "C" void ivx_index_free(ivx_index *ix)
{
    if (!ix) return;
    // the caller guarantees no probe on this index is still running (same contract as dropping
    // Arc<JoinLeftData>); buffers go back to the pool, to be reused only by later builds
    if (ix->ready) { (void)hipEventSynchronize(ix->ready); (void)hipEventDestroy(ix->ready); }   // (its build tail may still be writing)
    for (size_t i = 0; i < ix->allocs.size(); i++) pool_give(ix->device, ix->allocs[i], ix->alloc_caps[i]);
    if (ix->owner_bytes) ix->owner_bytes->fetch_sub(ix->bytes, std::memory_order_relaxed);
    delete ix;
}

extern "C" uint64_t ivx_index_rows(const ivx_index *ix) { return ix ? ix->n : 0; }
extern "C" uint64_t ivx_index_device_bytes(const ivx_index *ix) { return ix ? ix->bytes : 0; }

// the binned overlap index's header, as the build left it (ivx_join.hip: k_join_layout, k_join_count, k_join_regdesc)
extern "C" ivx_status ivx_index_layout(ivx_ctx *ctx, const ivx_index *ix, uint32_t *out, uint32_t n_out)
{
    if (!ctx) return IVX_ERR_INVALID;
    if (!ix) return ctx->fail(IVX_ERR_INVALID, "null index");
    if (n_out && !out) return ctx->fail(IVX_ERR_INVALID, "null out");
    if (ix->device != ctx->device) return ctx->fail(IVX_ERR_INVALID, "index lives on another device");
    u32 w[IVX_LAYOUT_WORDS] = {};
    w[IVX_LAYOUT_KIND] = (u32)ix->kind;
    if (ix->kind != IVX_KIND_NEAREST && ix->jv.hdr != nullptr) {
        IVX_HIP(ctx, hipSetDevice(ctx->device));
        // hdr[HDR_SLOW] and the level flags are written by the build's tail: with the build overlap on, behind `ready`
        if (ix->ready != nullptr) IVX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ix->ready, 0));
        u32 h[HDR_WORDS];
        IVX_HIP(ctx, hipMemcpyAsync(h, ix->jv.hdr, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        IVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const u32 nlev = h[HDR_NLEV] < IVX_MAXL ? h[HDR_NLEV] : IVX_MAXL;
        u32 levrows = 0;
        for (u32 l = 0; l < nlev; l++) if (h[HDR_LEVCNT + l]) levrows |= 1u << l;
        w[IVX_LAYOUT_SH0] = h[HDR_SH0];
        w[IVX_LAYOUT_NLEV] = h[HDR_NLEV];
        w[IVX_LAYOUT_LEVROWS] = levrows;
        w[IVX_LAYOUT_RCELLS] = h[HDR_NREG] ? h[HDR_RCELLS] : 0u;
        w[IVX_LAYOUT_RCS] = h[HDR_NREG] ? h[HDR_CS] : 0xFFFFFFFFu;
        w[IVX_LAYOUT_NREG] = h[HDR_NREG];
        w[IVX_LAYOUT_PK24] = h[HDR_PK24];
        w[IVX_LAYOUT_SLOW] = h[HDR_SLOW];
        w[IVX_LAYOUT_FG] = h[HDR_FG];
        w[IVX_LAYOUT_FBITS] = h[HDR_FG] != 0xFFFFFFFFu ? h[HDR_FBITS] : 0u;
        w[IVX_LAYOUT_NROUTE_NREG] = ix->nroute_nreg;
        w[IVX_LAYOUT_LBUILD] = h[HDR_LBUILD];
    }
    for (u32 i = 0; i < n_out && i < (u32)IVX_LAYOUT_WORDS; i++) out[i] = w[i];
    return IVX_OK;
}

// TEST HOOK (exported, not in include/ivx.h; tests/test_gpu_rank_edges.py): the forms a count / coverage / nearest index
// took -- the routing view's region count, what the nearest build's sorts did (host fields of the index) and every rank
// grid's header {shift, cells} (read back here: builds and probes never pay for it).  Reads only; words: IVX_FORMS_*
extern "C" ivx_status ivx_debug_index_forms(ivx_ctx *ctx, const ivx_index *ix, uint32_t *out, uint32_t n_out)
{
    if (!ctx) return IVX_ERR_INVALID;
    if (!ix) return ctx->fail(IVX_ERR_INVALID, "null index");
    if (n_out && !out) return ctx->fail(IVX_ERR_INVALID, "null out");
    if (ix->device != ctx->device) return ctx->fail(IVX_ERR_INVALID, "index lives on another device");
    u32 w[IVX_FORMS_WORDS] = {};
    w[IVX_FORMS_KIND] = (u32)ix->kind;
    w[IVX_FORMS_NROUTE_NREG] = ix->nroute_nreg;
    const RankGridView *g[3] = {nullptr, nullptr, nullptr};
    if (ix->kind == IVX_KIND_COUNT) { g[0] = &ix->gs; g[1] = &ix->ge; }
    else if (ix->kind == IVX_KIND_COVERAGE) { g[0] = &ix->cv.first; g[1] = &ix->cv.last; }
    else if (ix->kind == IVX_KIND_NEAREST) {
        g[0] = &ix->nv.by_start; g[1] = &ix->nv.by_end; g[2] = &ix->nv.pmax;
        w[IVX_FORMS_NEAR_WORDS] = ix->near_words; w[IVX_FORMS_NEAR_ORDER] = ix->near_order; w[IVX_FORMS_NEAR_FALLBACK] = ix->near_fallback;
    }
    IVX_HIP(ctx, hipSetDevice(ctx->device));
    for (int i = 0; i < 3; i++)
        if (g[i] && g[i]->hdr) IVX_HIP(ctx, hipMemcpyAsync(&w[IVX_FORMS_GRID0 + 2 * i], g[i]->hdr, 2 * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
    IVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (u32 i = 0; i < n_out && i < (u32)IVX_FORMS_WORDS; i++) out[i] = w[i];
    return IVX_OK;
}

// TEST HOOK (exported, not in include/ivx.h; tests/test_gpu_entry_state.py): what the context carries from one call to the next
// -- both plans and their slot masks, the pending build tail, the scratch slots that hold memory, the free buffers of the index
// pool, the fill calls that a plan served.  Reads host fields only:
// nothing is launched, no scratch is taken.  Words: IVX_STATE_*
extern "C" ivx_status ivx_debug_ctx_state(ivx_ctx *ctx, uint64_t *out, uint32_t n_out)
{
    if (!ctx) return IVX_ERR_INVALID;
    if (n_out && !out) return ctx->fail(IVX_ERR_INVALID, "null out");
    u64 w[IVX_STATE_WORDS] = {};
    w[IVX_STATE_JOIN_VALID] = ctx->join_plan.valid ? 1 : 0;
    w[IVX_STATE_JOIN_SLOTS] = ctx->join_plan.rows.slots;
    w[IVX_STATE_SUB_VALID] = ctx->sub_plan.valid ? 1 : 0;
    w[IVX_STATE_SUB_SLOTS] = ctx->sub_plan.slots;
    w[IVX_STATE_TAIL_PENDING] = ctx->tail_pending ? 1 : 0;
    w[IVX_STATE_JOIN_FILLS_PLANNED] = ctx->join_fills_planned;
    w[IVX_STATE_SUB_FILLS_PLANNED] = ctx->sub_fills_planned;
    for (int i = 0; i < IVX_NSCRATCH; i++) if (ctx->scratch[i].p) w[IVX_STATE_SCRATCH_HELD] |= 1ull << i;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (const PoolBuf &b : g_pool) if (b.device == ctx->device) w[IVX_STATE_POOL_FREE]++;
    }
    for (u32 i = 0; i < n_out && i < (u32)IVX_STATE_WORDS; i++) out[i] = w[i];
    return IVX_OK;
}

// TEST HOOK (exported, not in include/ivx.h; tests/test_gpu_entry_state.py): `word` (0 or 1) into every 32-bit word of the
// state `what` selects (IVX_POISON_* bits), so that a kernel that reads what an earlier call left -- a scratch slot, a
// call-local scalar word, a recycled index buffer -- gives a wrong answer instead of a right one by luck.  Left alone: the
// slots a valid plan names (unless IVX_POISON_DROP_PLANS), the scalar words of SC_OUTLIVES, the memory of live indexes; and a
// running build tail is refused, not waited for (the caller synchronises first).  Takes no scratch, allocates nothing and,
// without IVX_POISON_DROP_PLANS, leaves both plans as they are.  slots_written (nullable): the scratch slots written.
extern "C" ivx_status ivx_debug_poison(ivx_ctx *ctx, uint32_t word, int what, uint64_t *slots_written)
{
    if (!ctx) return IVX_ERR_INVALID;
    if (slots_written) *slots_written = 0;
    if (word > 1u) return ctx->fail(IVX_ERR_INVALID, "debug_poison: the word is 0 or 1");
    if (ctx->tail_pending) return ctx->fail(IVX_ERR_INVALID, "debug_poison: a build tail is pending");
    IVX_HIP(ctx, hipSetDevice(ctx->device));
    IVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    hipStream_t st = ctx->stream;
    const auto fill_host = [word](void *p, size_t bytes) { u32 *q = (u32 *)p; for (size_t i = 0; i < bytes / sizeof(u32); i++) q[i] = word; };
    if (what & IVX_POISON_DROP_PLANS) { ctx->sub_plan.valid = false; ctx->join_plan.valid = false; }
    if (what & IVX_POISON_SCRATCH) {
        const u64 keep = (ctx->sub_plan.valid ? ctx->sub_plan.slots : 0) | (ctx->join_plan.valid ? ctx->join_plan.rows.slots : 0);
        u64 wrote = 0;
        for (int i = 0; i < IVX_NSCRATCH; i++) {
            const ivx_buf &b = ctx->scratch[i];
            if (!b.p || ((keep >> i) & 1)) continue;
            IVX_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)b.p, (int)word, b.cap / sizeof(u32), st));
            wrote |= 1ull << i;
        }
        if (slots_written) *slots_written = wrote;
    }
    if (what & IVX_POISON_SCALARS) {
        // every run of words between two entries of SC_OUTLIVES (ascending): the device words, then their mirror and the host-only words
        int w = 0;
        for (size_t k = 0; k <= sizeof(SC_OUTLIVES) / sizeof(SC_OUTLIVES[0]); k++) {
            const bool last = k == sizeof(SC_OUTLIVES) / sizeof(SC_OUTLIVES[0]);
            const int stop = last ? (int)SC_HOST_WORDS : SC_OUTLIVES[k].first;
            if (w < stop) {
                const int dstop = stop < (int)SC_DEVICE_WORDS ? stop : (int)SC_DEVICE_WORDS;
                if (w < dstop) IVX_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)ctx->dword(w), (int)word, (size_t)(dstop - w) * 2, st));
                fill_host(ctx->hword(w), (size_t)(stop - w) * sizeof(u64));
            }
            if (!last) w = SC_OUTLIVES[k].first + SC_OUTLIVES[k].words;
        }
    }
    if (what & IVX_POISON_PINNED)
        for (const ivx_buf &b : ctx->pinned) if (b.p) fill_host(b.p, b.cap);
    if (what & IVX_POISON_POOL) {
        // (under the pool's lock up to the wait: no build of another thread takes a buffer while it is being written)
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (const PoolBuf &b : g_pool)
            if (b.device == ctx->device) IVX_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)b.p, (int)word, b.cap / sizeof(u32), st));
        IVX_HIP(ctx, hipStreamSynchronize(st));
    }
    IVX_HIP(ctx, hipStreamSynchronize(st));
    return IVX_OK;
}

// ---------------------------------------------------------------- a3 probes

static bool rowval_routed_ok(u64 n)
{
    if (const char *f = getenv("IVX_JOIN_PATH")) return !strcmp(f, "routed");      // tests: "direct" | "regions" | "routed"
    return n >= (1u << 21);
}

// Big batches of a per-row operator take the region path (nreg: one partition pass must do) from min_rows rows on;
// IVX_JOIN_PATH overrides the size rule (tests: "direct" | "regions")
static bool region_path_wanted(const ivx_index *ix, u64 n, u64 min_rows)
{
    const bool can = ix->jv_nreg > 0 && ix->jv_nreg <= IVX_MAXREG_WIDE;
    if (const char *p = getenv("IVX_JOIN_PATH")) {
        if (!strcmp(p, "direct")) return false;
        if (!strcmp(p, "regions")) return can;
    }
    return can && n >= min_rows;
}

static ivx_status overlap_common(ivx_ctx *ctx, const ivx_index *ix, int mem, int mode,
                                 const u32 *key, const i32 *start, const i32 *end, u64 n,
                                 u32 *per_row, u8 *exists, u32 *bidx, u32 *pidx, u64 cap, u64 *total)
{
    Frame f(ctx, mem);
    IVX_TRY(check_probe_args(f, ix, IVX_KIND_OVERLAP, start, end, n, true));
    if (total) *total = 0;                                  // (as Frame::begin(scalar): a refused call leaves 0, not the caller's word)
    f.meter(false, n);
    // large COUNT/FILL batches: partition the probe rows by index region and probe from LDS;
    // small batches and the per-row modes gather straight from the index
    bool regions = ix->jv_nreg > 0 && (mode == JP_COUNT || mode == JP_FILL) && n >= (1u << 21);   // measured crossover (tools/crossover.py)
    // the per-row modes (rle_right, semi / anti) of big batches: same partition, one value per row, un-permuted
    const bool rowval = (mode == JP_PER_ROW || mode == JP_EXISTS) && region_path_wanted(ix, n, 1u << 21);
    if (const char *p = getenv("IVX_JOIN_PATH")) {
        if (!strcmp(p, "direct")) regions = false;
        else if (!strcmp(p, "regions")) regions = ix->jv_nreg > 0 && (mode == JP_COUNT || mode == JP_FILL);
    }
    // a fill call right after the count call that sized it: the routed probe rows are still in the context
    const void *in[3] = {key, start, end};
    ivx_join_plan &pl = ctx->join_plan;
    const bool planned = regions && mode == JP_FILL && pl.valid && !getenv("IVX_NO_PLAN") && pl.mem == mem && memcmp(pl.in, in, sizeof(in)) == 0 && pl.n == n &&
                         pl.ix == (const void *)ix && pl.ix_serial == ix->serial && pl.stream == ctx->stream;
    // (the region path orders itself behind the index's build tail after its routing pass; everything else here)
    if (ix->ready != nullptr && !(regions && !planned)) IVX_HIP(ctx, hipStreamWaitEvent(ctx->stream, ix->ready, 0));
    const u32 *dk = nullptr; const i32 *ds = nullptr, *de = nullptr;
    if (!planned) { dk = f.in(key, n); ds = f.in(start, n); de = f.in(end, n); }
    u32 *d_row = f.out(per_row, n); u8 *d_ex = f.out(exists, n);
    u32 *d_b = f.out(bidx, cap), *d_p = f.out(pidx, cap);
    IVX_TRY(f.st);
    // pair cursor | probe fault flags: zeroed here, or -- a region probe that routes its rows -- by the routing pass's clearing kernel
    const bool defer_clear = regions && !planned;
    if (!defer_clear) IVX_HIP(ctx, hipMemsetAsync(ctx->dword(SC_PAIRS), 0, 2 * sizeof(u64), ctx->stream));
    ivx_probe_note note;
    note.ix_serial = ix->serial;
    IVX_TRY(f.run([&]() -> ivx_status {
        if (regions) {
            if (!planned) pl.valid = false;                 // whatever an earlier count call left is gone now
            const ivx_status st = ivx_join_probe_regions(ctx, ix->jv, ix->jv_nreg, mode, dk, ds, de, n, d_b, d_p, cap, ctx->dword(SC_PAIRS), planned, ix->jv_filter, ix->jv_pk24,
                                                         ix->jv_lean.load(std::memory_order_relaxed), planned ? nullptr : ix->ready, defer_clear, &note);
            // the call waited for the index's build tail and read hdr[HDR_SLOW] from the header mirror: known from here on
            if (note.fast >= 0) ix->jv_lean.store(note.fast, std::memory_order_relaxed);
            if (st != IVX_OK) { pl.valid = false; return st; }
            if (mode == JP_COUNT && pl.valid) { memcpy(pl.in, in, sizeof(in)); pl.mem = mem; pl.n = n; pl.ix = ix; pl.ix_serial = ix->serial; pl.stream = ctx->stream; }
            return IVX_OK;
        }
        if (rowval) return ivx_rowval_probe_regions(ctx, ix->jv, ix->jv_nreg, mode == JP_PER_ROW ? IVX_RV_PER_ROW : IVX_RV_EXISTS, dk, ds, de, n, 0,
                                                    mode == JP_PER_ROW ? (void *)d_row : (void *)d_ex, ctx->dword(SC_PAIRS), ix->jv_filter, ix->jv_pk24, ix->jv_lean.load(std::memory_order_relaxed) == 1);
        if (n && (mode == JP_PER_ROW || mode == JP_EXISTS) && ix->nroute_nreg > 0 && rowval_routed_ok(n))
            return ivx_join_rowval_routed(ctx, ix, mode, dk, ds, de, n, d_row, d_ex, ctx->dword(SC_PAIRS));   // too many regions for the LDS slices: route, gather, put back
        return ivx_join_probe(ctx, ix->jv, mode, dk, ds, de, n, d_row, d_ex, d_b, d_p, cap, ctx->dword(SC_PAIRS));
    }));
    u64 tot = 0;
    if (mode != JP_EXISTS) {
        // (a lean fill's last kernel has left both words in the mapped mirror itself: k_fill_rest)
        if (!note.totals_on_host) IVX_HIP(ctx, ctx->fetch(SC_PAIRS, ctx->stream, 2));
        IVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        tot = *ctx->hword(SC_PAIRS);
        // a probe kernel met a routed-row page that the partition never published (it substituted a valid page, so nothing
        // was read out of bounds): an internal error, reported instead of returning wrong pairs
        if (*ctx->hword(SC_FAULT)) { ctx->join_plan.valid = false; return ctx->fail(IVX_ERR_HIP, "internal error: the probe met an unpublished page of routed rows"); }
    }
    if (mode == JP_COUNT && regions && pl.valid) pl.total = tot;
    if (total) *total = tot;
    if (mode == JP_FILL && tot > cap) return ctx->fail(IVX_ERR_CAPACITY, "pair buffers too small");   // (a plan survives this: the retry with bigger buffers reuses it)
    f.rows_out(mode == JP_FILL ? tot : (mode == JP_COUNT ? 0 : n));
    if (planned) ctx->join_fills_planned++;
    if (planned) pl.valid = false;                          // a plan serves ONE successful fill: a caller that refills the same buffers with its next batch must not get this batch's rows
    f.back(per_row); f.back(exists);                        // (one value per probe row, in whichever mode asked for them)
    if (mode == JP_FILL) { f.back(bidx, tot); f.back(pidx, tot); }
    return f.finish();
}

extern "C" ivx_status ivx_probe_overlap_count(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key,
                                              const int32_t *start, const int32_t *end, uint64_t n,
                                              uint32_t *per_row, uint64_t *total)
{
    return overlap_common(ctx, ix, mem, per_row ? JP_PER_ROW : JP_COUNT, key, start, end, n, per_row, nullptr, nullptr, nullptr, 0, total);
}

// ---- host-resident columns of a big batch: chunks, so that the link runs in both directions at once
// The columns of 100 M probe rows cross the link in ~21 ms, the pairs come back in ~5 ms, the kernels take 1.3 ms: done one
// after the other that is what the call costs.  Cut into chunks, the results of chunk c go back to the host (a helper thread
// on a stream of its own: a copy from or to pageable memory occupies the thread that issues it) while the columns of chunk
// c + 1 come in.  Every chunk is a device-resident call of its own.

// device -> host copies on a thread and stream of their own, each after an event of the compute stream
struct HostCopier {
    struct Job { void *dst; const void *src; size_t bytes; hipEvent_t ev; };
    std::mutex mu; std::condition_variable cv, cv_done; std::deque<Job> jobs; bool closed = false; hipError_t herr = hipSuccess;
    u64 done = 0;                                           // copies finished so far (in the order they were pushed)
    hipStream_t cs = nullptr; std::thread th; std::vector<hipEvent_t> evs; bool started = false;
    hipError_t start(int device)
    {
        const hipError_t e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
        if (e != hipSuccess) return e;
        try {
        th = std::thread([this, device]() {
            (void)hipSetDevice(device);
            for (;;) {
                Job j;
                { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return closed || !jobs.empty(); }); if (jobs.empty()) return; j = jobs.front(); jobs.pop_front(); }
                hipError_t e2 = j.ev ? hipStreamWaitEvent(cs, j.ev, 0) : hipSuccess;
                if (e2 == hipSuccess && j.bytes) e2 = hipMemcpyAsync(j.dst, j.src, j.bytes, hipMemcpyDeviceToHost, cs);
                if (e2 == hipSuccess) e2 = hipStreamSynchronize(cs);
                { std::lock_guard<std::mutex> lk(mu); if (e2 != hipSuccess) herr = e2; done++; }
                cv_done.notify_all();
            }
        });
        } catch (...) { (void)hipStreamDestroy(cs); cs = nullptr; return hipErrorOutOfMemory; }     // (no thread to be had: the caller reports it)
        started = true;
        return hipSuccess;
    }
    // an event recorded on `st` now; the copies pushed with it run after everything enqueued on `st` so far
    hipError_t mark(hipStream_t st, hipEvent_t *ev)
    {
        hipError_t e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
        if (e != hipSuccess) return e;
        evs.push_back(*ev);
        return hipEventRecord(*ev, st);
    }
    void push(void *dst, const void *src, size_t bytes, hipEvent_t ev)
    {
        { std::lock_guard<std::mutex> lk(mu); jobs.push_back(Job{dst, src, bytes, ev}); }
        cv.notify_all();
    }
    void wait_until(u64 k) { std::unique_lock<std::mutex> lk(mu); cv_done.wait(lk, [&] { return done >= k; }); }   // the first k copies are done
    hipError_t finish()                                     // waits for every copy
    {
        if (!started) return hipSuccess;
        { std::lock_guard<std::mutex> lk(mu); closed = true; }
        cv.notify_all();
        th.join();
        for (hipEvent_t e : evs) (void)hipEventDestroy(e);
        (void)hipStreamDestroy(cs);
        started = false;
        return herr;
    }
    ~HostCopier() { (void)finish(); }
};

// IVX_HOST_CHUNKS = number of chunks, 1 switches chunking off; default 4 from 16 M rows; a chunk is a multiple of 65 536 rows
static u32 host_chunks(u64 n)
{
    const char *ce = getenv("IVX_HOST_CHUNKS");
    const u32 nchunk = ce ? (u32)atoi(ce) : (n >= (16ull << 20) ? 4u : 1u);
    return nchunk > 1 && n >= (u64)nchunk * 65536 ? nchunk : 1u;
}

// one chunk, as its device call sees it: rows [c0, c0 + n) of the batch, their columns on the device, and what the call
// wants copied back to the host once everything it has enqueued is done
struct HostChunk {
    u32 c; int set; u64 c0, n;
    const u32 *key; const i32 *start, *end;
    struct Copy { void *dst; const void *src; size_t bytes; } back[2];
    int n_back = 0;
    void push(void *dst, const void *src, size_t bytes) { back[n_back++] = Copy{dst, src, bytes}; }
};

// The pipeline: two sets of staged columns (WS_IN* / WS_IN2*: chunk c + 1 arrives while the kernels of chunk c may still
// read theirs), per_chunk(HostChunk &) for the device call of every chunk, the copies it pushes handed to the helper thread.
// out_sets: the per_chunk calls write their results into two alternating buffers of their own (chunk c into set c & 1), so
// the device call of chunk c waits for the copies of chunk c - 2; false: nothing a chunk writes is written again.
// copy_what names the copies in an error.  Errors: the first of per_chunk's, the stream's, the copies'.
template <typename PerChunk>
static ivx_status host_chunked(ivx_ctx *ctx, const u32 *key, const i32 *start, const i32 *end, u64 n, u32 nchunk, bool out_sets,
                               const char *copy_what, PerChunk &&per_chunk)
{
    hipStream_t st = ctx->stream;
    const u64 rows = ((n + nchunk - 1) / nchunk + 65535) & ~65535ull;           // rows per chunk
    u32 *dk[2] = {nullptr, nullptr}; i32 *ds[2], *de[2];
    for (int b = 0; b < 2; b++) {
        if (key) IVX_TRY(ctx->get_scratch(b ? WS_IN2_KEY : WS_IN_KEY, rows * sizeof(u32), (void **)&dk[b]));
        IVX_TRY(ctx->get_scratch(b ? WS_IN2_START : WS_IN_START, rows * sizeof(i32), (void **)&ds[b]));
        IVX_TRY(ctx->get_scratch(b ? WS_IN2_END : WS_IN_END, rows * sizeof(i32), (void **)&de[b]));
    }
    HostCopier hc;
    IVX_HIP(ctx, hc.start(ctx->device));
    u64 pushed = 0, pushed_by[2] = {0, 0};                                      // copies pushed so far; ... up to the last chunk of either set
    ivx_status rc = IVX_OK;
    for (u32 c = 0; c < nchunk && rc == IVX_OK; c++) {
        HostChunk ch;
        ch.c = c; ch.set = (int)(c & 1u); ch.c0 = (u64)c * rows;
        const u64 c1 = ch.c0 + rows < n ? ch.c0 + rows : n;
        if (ch.c0 >= c1) break;
        ch.n = c1 - ch.c0;
        const int b = ch.set;
        // (input set b was last read by the kernels of chunk c - 2, earlier on this stream; an output set b by the COPY of
        //  chunk c - 2, on the helper's stream: that one is awaited before this chunk's kernels are enqueued)
        hipError_t e = hipSuccess;
        if (key) e = hipMemcpyAsync(dk[b], key + ch.c0, ch.n * sizeof(u32), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(ds[b], start + ch.c0, ch.n * sizeof(i32), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(de[b], end + ch.c0, ch.n * sizeof(i32), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) { rc = ctx->fail_hip("hipMemcpyAsync(chunk)", e); break; }
        if (out_sets && c >= 2) hc.wait_until(pushed_by[b]);
        ch.key = dk[b]; ch.start = ds[b]; ch.end = de[b];
        rc = per_chunk(ch);
        if (rc != IVX_OK || ch.n_back == 0) continue;
        hipEvent_t ev;
        e = hc.mark(st, &ev);
        if (e != hipSuccess) { rc = ctx->fail_hip("hipEventRecord(chunk)", e); break; }
        for (int i = 0; i < ch.n_back; i++) hc.push(ch.back[i].dst, ch.back[i].src, ch.back[i].bytes, ev);
        pushed += (u64)ch.n_back;
        pushed_by[b] = pushed;
    }
    // (the staged columns of the last chunks must not be reused before their kernels are done: the stream is idle here)
    const hipError_t es = hipStreamSynchronize(st);
    const hipError_t herr = hc.finish();
    if (rc != IVX_OK) return rc;
    if (es != hipSuccess) return ctx->fail_hip("hipStreamSynchronize", es);
    if (herr != hipSuccess) return ctx->fail_hip(copy_what, herr);
    return IVX_OK;
}

// the overlap fill, chunked: every chunk appends to the same pair buffers; probe row ids are shifted by the chunk's first
// row afterwards.  Order of the pairs is free, as everywhere.
__global__ void k_add_base(u32 *__restrict__ p, u64 n, u32 base)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) p[i] += base;
}

static ivx_status overlap_fill_host_chunked(ivx_ctx *ctx, const ivx_index *ix, const u32 *key, const i32 *start, const i32 *end, u64 n,
                                            u32 *bidx, u32 *pidx, u64 cap, u64 *written, u32 nchunk)
{
    Frame f(ctx, IVX_MEM_HOST);
    IVX_TRY(check_probe_args(f, ix, IVX_KIND_OVERLAP, start, end, n));
    if (written) *written = 0;
    u32 *d_b, *d_p;
    IVX_TRY(ctx->get_scratch(WS_OUT_C, (size_t)(cap ? cap : 1) * sizeof(u32), (void **)&d_b));
    IVX_TRY(ctx->get_scratch(WS_OUT_D, (size_t)(cap ? cap : 1) * sizeof(u32), (void **)&d_p));
    const ivx_metrics m0 = ctx->metrics;                                        // (the chunks are one batch to the caller)
    u64 cum = 0, need = 0;
    bool over = false;                                                          // the pair buffers ran out: only count from here on
    const ivx_status rc = host_chunked(ctx, key, start, end, n, nchunk, false, "hipMemcpyAsync(pairs)", [&](HostChunk &ch) -> ivx_status {
        u64 tot = 0;
        if (over) {
            const ivx_status st = overlap_common(ctx, ix, IVX_MEM_DEVICE, JP_COUNT, ch.key, ch.start, ch.end, ch.n, nullptr, nullptr, nullptr, nullptr, 0, &tot);
            need += tot;
            return st;
        }
        ctx->fill_hint = (u64)((double)cap * (double)ch.n / (double)n) + 1;     // (the chunk's share of the pairs the caller expects: cap - cum would read as a dense join)
        const ivx_status st = overlap_common(ctx, ix, IVX_MEM_DEVICE, JP_FILL, ch.key, ch.start, ch.end, ch.n, nullptr, nullptr, d_b + cum, d_p + cum, cap - cum, &tot);
        ctx->fill_hint = 0;
        if (st == IVX_ERR_CAPACITY) { over = true; need = cum + tot; return IVX_OK; }
        if (st != IVX_OK) return st;
        if (tot && ch.c0) hipLaunchKernelGGL(k_add_base, dim3(1024), dim3(256), 0, ctx->stream, d_p + cum, tot, (u32)ch.c0);
        ch.push(bidx + cum, d_b + cum, tot * sizeof(u32));
        ch.push(pidx + cum, d_p + cum, tot * sizeof(u32));
        cum += tot;
        return IVX_OK;
    });
    ctx->join_plan.valid = false;                                               // (the count calls above may have left one: it refers to a chunk)
    ctx->metrics.input_batches = m0.input_batches + 1;
    ctx->metrics.output_batches = m0.output_batches + ((rc == IVX_OK && !over && cum) ? 1 : 0);
    if (over) ctx->metrics.output_rows = m0.output_rows;
    if (rc != IVX_OK) return rc;
    if (written) *written = over ? need : cum;
    if (over) return ctx->fail(IVX_ERR_CAPACITY, "pair buffers too small");
    return IVX_OK;
}

extern "C" ivx_status ivx_probe_overlap_fill(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key,
                                             const int32_t *start, const int32_t *end, uint64_t n,
                                             uint32_t *build_idx, uint32_t *probe_idx, uint64_t cap, uint64_t *written)
{
    if (ctx && cap && (!build_idx || !probe_idx)) return ctx->fail(IVX_ERR_INVALID, "null pair buffers");
    // host-resident columns of a big batch, and no count call left its routed rows (and device copies) behind: chunked
    if (ctx && ix && mem == IVX_MEM_HOST && cap && start && end) {
        const u32 nchunk = host_chunks(n);
        const void *in[3] = {key, start, end};
        const ivx_join_plan &pl = ctx->join_plan;
        const bool planned = pl.valid && pl.mem == mem && memcmp(pl.in, in, sizeof(in)) == 0 && pl.n == n && pl.ix == (const void *)ix && pl.ix_serial == ix->serial;
        if (nchunk > 1 && !planned && ix->kind == IVX_KIND_OVERLAP)
            return overlap_fill_host_chunked(ctx, ix, key, start, end, n, build_idx, probe_idx, cap, written, nchunk);
    }
    return overlap_common(ctx, ix, mem, JP_FILL, key, start, end, n, nullptr, nullptr, build_idx, probe_idx, cap, written);
}

extern "C" ivx_status ivx_probe_exists(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key,
                                       const int32_t *start, const int32_t *end, uint64_t n, uint8_t *exists)
{
    if (ctx && n && !exists) return ctx->fail(IVX_ERR_INVALID, "null exists buffer");
    return overlap_common(ctx, ix, mem, JP_EXISTS, key, start, end, n, nullptr, exists, nullptr, nullptr, 0, nullptr);
}

// ---------------------------------------------------------------- a3'': build-side match marks

// Beside overlap_common: the same two ways through the index, the match recorded by BUILD row.  Big batches over a lean
// index (the form ivx_rowval_probe_regions runs k_lean on) take the region kernels; everything else the direct one.
static ivx_status mark_build_impl(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key,
                                  const int32_t *start, const int32_t *end, uint64_t n, const ivx_overlap_where *where, uint32_t *marks)
{
    Frame f(ctx, mem);
    IVX_TRY(check_probe_args(f, ix, IVX_KIND_OVERLAP, start, end, n));             // (orders the stream behind a build tail, too)
    WherePred wp; bool filtered;
    IVX_TRY(check_where(ctx, where, &wp, &filtered));
    const WherePred *w = filtered ? &wp : nullptr;
    if (n && ix->n && !marks) return ctx->fail(IVX_ERR_INVALID, "null mark bitmap");
    f.meter(false, n);
    f.drop_join_plan();                                     // as any other call between a count call and its fill
    const u64 nw = (ix->n + 31) / 32;
    if (n == 0 || nw == 0) return IVX_OK;
    const bool regions = region_path_wanted(ix, n, 1u << 21);             // the threshold of overlap_common's per-row branch
    const u32 *dk = f.in(key, n);
    const i32 *ds = f.in(start, n), *de = f.in(end, n);
    u32 *dm = f.out_or(marks, nw);
    IVX_TRY(f.run([&]() -> ivx_status {
        bool took = false;
        if (regions) IVX_TRY(ivx_mark_probe_regions(ctx, ix->jv, ix->jv_nreg, dk, ds, de, n, dm, ix->jv_filter, ix->jv_pk24, ix->jv_lean.load(std::memory_order_relaxed) == 1, &took, w));
        return took ? IVX_OK : ivx_mark_probe(ctx, ix->jv, dk, ds, de, n, dm, w);
    }));
    f.or_back(marks);                                       // (synchronises: nothing is left for finish())
    return f.st;
}
extern "C" ivx_status ivx_probe_mark_build(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key,
                                           const int32_t *start, const int32_t *end, uint64_t n, uint32_t *marks)
{
    return mark_build_impl(ctx, ix, mem, key, start, end, n, nullptr, marks);
}
extern "C" ivx_status ivx_probe_mark_build_where(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key,
                                                 const int32_t *start, const int32_t *end, uint64_t n, const ivx_overlap_where *w, uint32_t *marks)
{
    return mark_build_impl(ctx, ix, mem, key, start, end, n, w, marks);
}

// ---------------------------------------------------------------- a3''': overlap aggregates

// Beside ivx_probe_mark_build, and with its path choice: big batches over a lean index take the region kernels
// (ivx_agg_probe_regions), everything else the direct one.  One value per probe row and wanted output, in input order.
// The switch between the two, measured (tools/overlap_agg_timing.py, profiles/overlap_agg_timing.txt): the region path's
// un-permute makes one pass per output, so what it saves on the walk it loses again with every 8-byte output wanted.  By
// the number of those: the batch size from which the region path won by more than the repeats' spread, or never.
static u64 agg_regions_rows(int n64)
{
    return n64 <= 1 ? 1ull << 23 : n64 <= 3 ? 1ull << 24 : ~0ull;
}
static ivx_status overlap_agg_impl(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key,
                                   const int32_t *start, const int32_t *end, uint64_t n, const void *val, uint32_t val_bytes,
                                   const ivx_overlap_where *where,
                                   uint32_t *count, int64_t *sum, int64_t *vmin, int64_t *vmax, int64_t *bases, int64_t *wsum)
{
    Frame f(ctx, mem);
    IVX_TRY(check_probe_args(f, ix, IVX_KIND_OVERLAP, start, end, n));             // (orders the stream behind a build tail, too)
    WherePred wp; bool filtered;
    IVX_TRY(check_where(ctx, where, &wp, &filtered));
    const WherePred *w = filtered ? &wp : nullptr;
    if (!count && !sum && !vmin && !vmax && !bases && !wsum) return ctx->fail(IVX_ERR_INVALID, "overlap_agg: no output wanted");
    if (val_bytes != 4 && val_bytes != 8) return ctx->fail(IVX_ERR_INVALID, "overlap_agg: val_bytes is 4 or 8");
    if (ix->n && !val) return ctx->fail(IVX_ERR_INVALID, "overlap_agg: null value column");
    f.meter(false, n);
    f.drop_join_plan();                                     // as any other call between a count call and its fill
    if (n == 0) return IVX_OK;
    const int n64 = (sum != nullptr) + (vmin != nullptr) + (vmax != nullptr) + (bases != nullptr) + (wsum != nullptr);
    const bool regions = region_path_wanted(ix, n, agg_regions_rows(n64));
    const u32 *dk = f.in(key, n);
    const i32 *ds = f.in(start, n), *de = f.in(end, n);
    const void *dv = f.in((const u8 *)val, (u64)ix->n * val_bytes);
    AggOut o;
    o.count = f.out(count, n); o.sum = f.out(sum, n); o.vmin = f.out(vmin, n); o.vmax = f.out(vmax, n);
    o.bases = f.out(bases, n); o.wsum = f.out(wsum, n);
    IVX_TRY(f.st);
    IVX_TRY(f.run([&]() -> ivx_status {
        bool took = false;
        if (regions) IVX_TRY(ivx_agg_probe_regions(ctx, ix->jv, ix->jv_nreg, dk, ds, de, n, dv, val_bytes, o, ix->jv_filter, ix->jv_pk24, ix->jv_lean.load(std::memory_order_relaxed) == 1, &took, w));
        return took ? IVX_OK : ivx_agg_probe(ctx, ix->jv, dk, ds, de, n, dv, val_bytes, o, w);
    }));
    f.rows_out(n);                                          // (as ivx_probe_count: not on a refused call)
    f.back_all();
    return f.finish();
}
extern "C" ivx_status ivx_probe_overlap_agg(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key,
                                            const int32_t *start, const int32_t *end, uint64_t n, const void *val, uint32_t val_bytes,
                                            uint32_t *count, int64_t *sum, int64_t *vmin, int64_t *vmax, int64_t *bases, int64_t *wsum)
{
    return overlap_agg_impl(ctx, ix, mem, key, start, end, n, val, val_bytes, nullptr, count, sum, vmin, vmax, bases, wsum);
}
extern "C" ivx_status ivx_probe_overlap_agg_where(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key,
                                                  const int32_t *start, const int32_t *end, uint64_t n, const void *val, uint32_t val_bytes,
                                                  const ivx_overlap_where *w,
                                                  uint32_t *count, int64_t *sum, int64_t *vmin, int64_t *vmax, int64_t *bases, int64_t *wsum)
{
    return overlap_agg_impl(ctx, ix, mem, key, start, end, n, val, val_bytes, w, count, sum, vmin, vmax, bases, wsum);
}

// ---------------------------------------------------------------- a3'''': overlap select (include/ivx_select.h)

// Beside ivx_probe_overlap_agg, and with its path choice: big batches over a lean index take the region kernels
// (ivx_sel_probe_regions), everything else the direct one.  One winner per probe row, in input order.
// The switch between the two, measured (tools/overlap_select_timing.py, profiles/overlap_select_timing.txt; max_val on int32
// and max_overlap, with and without the score): from 2^23 rows the region path's slowest repeat beat the direct kernel's
// fastest in all four variants (0.26 against 0.35 ms with value and score; 2.51 against 3.49 ms at 10^8 rows); at 2^22 rows
// it did in three of them and lost with max_overlap and score; at 2^21 it lost in all.
static u64 sel_regions_rows()
{
    return 1ull << 23;
}
static ivx_status overlap_select_impl(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key,
                                      const int32_t *start, const int32_t *end, uint64_t n, const void *val, uint32_t val_bytes,
                                      int by, const ivx_overlap_where *where, uint32_t *build_idx, int64_t *score)
{
    Frame f(ctx, mem);
    IVX_TRY(check_probe_args(f, ix, IVX_KIND_OVERLAP, start, end, n));             // (orders the stream behind a build tail, too)
    WherePred wp; bool filtered;
    IVX_TRY(check_where(ctx, where, &wp, &filtered));
    const WherePred *w = filtered ? &wp : nullptr;
    if (!build_idx) return ctx->fail(IVX_ERR_INVALID, "overlap_select: null build_idx");
    if (by < 0 || by >= IVX_SEL_N) return ctx->fail(IVX_ERR_INVALID, "overlap_select: unknown criterion");
    const bool by_val = by == IVX_SEL_MIN_VAL || by == IVX_SEL_MAX_VAL;
    if (by_val && val_bytes != 4 && val_bytes != 8) return ctx->fail(IVX_ERR_INVALID, "overlap_select: val_bytes is 4 or 8");
    if (by_val && ix->n && !val) return ctx->fail(IVX_ERR_INVALID, "overlap_select: null value column");
    f.meter(false, n);
    f.drop_join_plan();                                     // as any other call between a count call and its fill
    if (n == 0) return IVX_OK;
    const bool regions = region_path_wanted(ix, n, sel_regions_rows());
    const u32 *dk = f.in(key, n);
    const i32 *ds = f.in(start, n), *de = f.in(end, n);
    const void *dv = by_val ? f.in((const u8 *)val, (u64)ix->n * val_bytes) : nullptr;      // (the other criteria stage nothing of val)
    SelOut o;
    o.idx = f.out(build_idx, n); o.score = f.out(score, n);
    IVX_TRY(f.st);
    IVX_TRY(f.run([&]() -> ivx_status {
        bool took = false;
        if (regions) IVX_TRY(ivx_sel_probe_regions(ctx, ix->jv, ix->jv_nreg, dk, ds, de, n, dv, val_bytes, by, o, ix->jv_filter, ix->jv_pk24, ix->jv_lean.load(std::memory_order_relaxed) == 1, &took, w));
        return took ? IVX_OK : ivx_sel_probe(ctx, ix->jv, dk, ds, de, n, dv, val_bytes, by, o, w);
    }));
    f.rows_out(n);                                          // (as ivx_probe_count: not on a refused call)
    f.back_all();
    return f.finish();
}
extern "C" ivx_status ivx_probe_overlap_select(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key,
                                               const int32_t *start, const int32_t *end, uint64_t n, const void *val, uint32_t val_bytes,
                                               int by, uint32_t *build_idx, int64_t *score)
{
    return overlap_select_impl(ctx, ix, mem, key, start, end, n, val, val_bytes, by, nullptr, build_idx, score);
}
extern "C" ivx_status ivx_probe_overlap_select_where(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key,
                                                     const int32_t *start, const int32_t *end, uint64_t n, const void *val, uint32_t val_bytes,
                                                     int by, const ivx_overlap_where *w, uint32_t *build_idx, int64_t *score)
{
    return overlap_select_impl(ctx, ix, mem, key, start, end, n, val, val_bytes, by, w, build_idx, score);
}

// ---------------------------------------------------------------- a3''''': overlap thresholds (include/ivx_where.h)

// The per-row match count under a threshold: per_row, exists and the total, each wanted or not.  Beside ivx_probe_mark_build,
// with its path choice (region_path_wanted from 2^21 rows: the threshold of overlap_common's per-row branch); where the plain
// per-row modes take the routed per-row path (an index of too many regions) this one takes the direct kernel.  One walk:
// the counts go to per_row -- the caller's, or scratch when only the total is wanted.  The total is a device reduction of them:
// the region path's un-permute adds them up on its way (as for the plain per-row mode), the direct path runs k_match_totals,
// which also derives the exists bytes where the region path wrote per_row alone; exists alone is written by the walk itself.
extern "C" ivx_status ivx_probe_overlap_count_where(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key,
                                                    const int32_t *start, const int32_t *end, uint64_t n, const ivx_overlap_where *where,
                                                    uint32_t *per_row, uint8_t *exists, uint64_t *total)
{
    Frame f(ctx, mem);
    IVX_TRY(check_probe_args(f, ix, IVX_KIND_OVERLAP, start, end, n));             // (orders the stream behind a build tail, too)
    WherePred wp; bool filtered;
    IVX_TRY(check_where(ctx, where, &wp, &filtered));
    if (!per_row && !exists && !total) return ctx->fail(IVX_ERR_INVALID, "overlap_count_where: no output wanted");
    if (total) *total = 0;
    f.meter(false, n);
    f.drop_join_plan();                                     // as any other call between a count call and its fill
    if (n == 0) return IVX_OK;
    const bool regions = region_path_wanted(ix, n, 1u << 21);
    const u32 *dk = f.in(key, n);
    const i32 *ds = f.in(start, n), *de = f.in(end, n);
    u32 *d_row = f.out(per_row, n);
    u8 *d_ex = f.out(exists, n);
    if (!d_row && total) IVX_TRY(f.scratch_at(WS_T6, (size_t)n * sizeof(u32), (void **)&d_row));   // (the reduction's input)
    IVX_TRY(f.st);
    u64 *d_total = ctx->dword(SC_PAIRS);                    // this call is an overlap probe: the pair's first word is its total
    if (total) IVX_HIP(ctx, hipMemsetAsync(d_total, 0, 2 * sizeof(u64), ctx->stream));
    IVX_TRY(f.run([&]() -> ivx_status {
        bool took = false;
        if (regions) IVX_TRY(ivx_match_probe_regions_where(ctx, ix->jv, ix->jv_nreg, dk, ds, de, n, d_row, d_ex, total ? d_total : nullptr, ix->jv_filter, ix->jv_pk24,
                                                           ix->jv_lean.load(std::memory_order_relaxed) == 1, &took, wp));
        // the region form has summed the counts in its un-permute and wrote per_row alone when both columns were wanted: the
        // exists bytes are still to derive; the direct walk wrote both columns and has no total yet
        if (took) return d_row && d_ex ? ivx_match_totals(ctx, d_row, n, d_ex, nullptr) : IVX_OK;
        IVX_TRY(ivx_match_probe_where(ctx, ix->jv, dk, ds, de, n, d_row, d_ex, wp));
        return total ? ivx_match_totals(ctx, d_row, n, nullptr, d_total) : IVX_OK;
    }));
    if (total) IVX_TRY(ctx->fetch_wait(SC_PAIRS, ctx->stream, total));
    f.rows_out(n);
    f.back_all();
    return f.finish();
}

// The stable pair filter.  Its columns are the join's own: the pairs a fill call wrote, the coordinate columns it was given.
extern "C" ivx_status ivx_pairs_where(ivx_ctx *ctx, int mem, const uint32_t *build_idx, const uint32_t *probe_idx, uint64_t n_pairs,
                                      const int32_t *bstart, const int32_t *bend, uint64_t nb,
                                      const int32_t *pstart, const int32_t *pend, uint64_t np, const ivx_overlap_where *where,
                                      uint32_t *out_build, uint32_t *out_probe, uint64_t cap, uint64_t *n_out)
{
    Frame f(ctx, mem);
    IVX_TRY(f.enter(n_out, "pairs_where: null n_out"));
    WherePred wp; bool filtered;
    IVX_TRY(check_where(ctx, where, &wp, &filtered));
    if (n_pairs && (!build_idx || !probe_idx)) return ctx->fail(IVX_ERR_INVALID, "pairs_where: null pair columns");
    if ((nb && (!bstart || !bend)) || (np && (!pstart || !pend))) return ctx->fail(IVX_ERR_INVALID, "pairs_where: null coordinate column");
    if (nb > 0xFFFFFFFFull || np > 0xFFFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "pairs_where: row count exceeds UInt32 index capacity");
    if (cap && (!out_build || !out_probe)) return ctx->fail(IVX_ERR_INVALID, "pairs_where: null output columns");
    if (!cap && (out_build || out_probe)) return ctx->fail(IVX_ERR_INVALID, "pairs_where: output columns without capacity");
    // an output is written while other workgroups still read the inputs: no overlap with any of them, nor with the other output
    {
        struct Span { const void *p; u64 bytes; };
        const Span ins[] = {{build_idx, n_pairs * 4}, {probe_idx, n_pairs * 4}, {bstart, nb * 4}, {bend, nb * 4}, {pstart, np * 4}, {pend, np * 4},
                            {out_probe, cap * 4}};
        const Span outs[] = {{out_build, cap * 4}, {out_probe, cap * 4}};
        for (int o = 0; o < 2; o++)
            for (int i = 0; i < 7 - o; i++) {
                const uintptr_t a = (uintptr_t)outs[o].p, b = (uintptr_t)ins[i].p;
                if (outs[o].bytes && ins[i].bytes && a < b + ins[i].bytes && b < a + outs[o].bytes)
                    return ctx->fail(IVX_ERR_INVALID, "pairs_where: an output overlaps an input or the other output");
            }
    }
    f.meter(false, n_pairs);
    f.drop_join_plan();
    if (n_pairs == 0) return IVX_OK;
    const u32 *db = f.in(build_idx, n_pairs), *dp = f.in(probe_idx, n_pairs);
    const i32 *dbs = f.in(bstart, nb), *dbe = f.in(bend, nb), *dps = f.in(pstart, np), *dpe = f.in(pend, np);
    u32 *dob = f.out(out_build, cap), *dop = f.out(out_probe, cap);
    IVX_TRY(f.st);
    u64 m = 0;
    const ivx_status st = f.run([&] { return ivx_pairs_where_device(ctx, db, dp, n_pairs, dbs, dbe, nb, dps, dpe, np, wp, dob, dop, cap, &m); });
    *n_out = m;
    if (st != IVX_OK) return st;
    f.rows_out(m);
    f.back(out_build, m); f.back(out_probe, m);
    return f.finish();
}

extern "C" ivx_status ivx_bits_mark(ivx_ctx *ctx, int mem, const uint32_t *idx, uint64_t n, uint32_t *bits, uint64_t n_bits)
{
    Frame f(ctx, mem);
    IVX_TRY(f.enter());
    if (n && !idx) return ctx->fail(IVX_ERR_INVALID, "bits_mark: null idx");
    if (n_bits && !bits) return ctx->fail(IVX_ERR_INVALID, "bits_mark: null bitmap");
    if (n_bits > 0xFFFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "bits_mark: bitmap exceeds UInt32 index capacity");
    if (n == 0) return IVX_OK;
    const u32 *didx = f.in(idx, n);
    u32 *dbits = f.out_or(bits, (n_bits + 31) / 32);
    IVX_TRY(f.run([&] { return ivx_bits_mark_device(ctx, didx, n, dbits, n_bits); }));
    f.or_back(bits);
    return f.st;
}

extern "C" ivx_status ivx_bits_select(ivx_ctx *ctx, int mem, const uint32_t *bits, uint64_t n_bits, int want_set,
                                      uint32_t *out, uint64_t cap, uint64_t *n_out)
{
    Frame f(ctx, mem);
    IVX_TRY(f.enter(n_out, "null n_out"));
    if (n_bits && !bits) return ctx->fail(IVX_ERR_INVALID, "bits_select: null bitmap");
    if (cap && !out) return ctx->fail(IVX_ERR_INVALID, "bits_select: null out");
    if (n_bits > 0xFFFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "bits_select: bitmap exceeds UInt32 index capacity");
    const u32 *dbits = f.in(bits, (n_bits + 31) / 32);
    u32 *dout = f.out(out, cap);
    u64 m = 0;
    const ivx_status st = f.run([&] { return ivx_bits_select_device(ctx, dbits, n_bits, want_set, dout, cap, &m); });
    *n_out = m;
    if (st != IVX_OK) return st;
    f.back(out, m);
    return f.finish();
}

// ---------------------------------------------------------------- a4 / a5 / a6 probes

static ivx_status per_row_i64(ivx_ctx *ctx, const ivx_index *ix, int kind, int mem, const u32 *key, const i32 *start,
                              const i32 *end, u64 n, int strict, i64 *out)
{
    Frame f(ctx, mem);
    IVX_TRY(check_probe_args(f, ix, kind, start, end, n));
    if (n && !out) return ctx->fail(IVX_ERR_INVALID, "null output column");
    f.meter(false, n);
    const auto probe = [&](const u32 *dk, const i32 *ds, const i32 *de, u64 rows, i64 *dout) {
        return kind == IVX_KIND_COUNT ? ivx_count_probe(ctx, ix, dk, ds, de, rows, strict, dout) : ivx_coverage_probe(ctx, ix, dk, ds, de, rows, strict, dout);
    };
    // host-resident columns of a big batch: in chunks, the values of chunk c go back while the columns of chunk c + 1 come in
    const u32 nchunk = mem == IVX_MEM_HOST ? host_chunks(n) : 1u;
    if (nchunk > 1) {
        const u64 rows = ((n + nchunk - 1) / nchunk + 65535) & ~65535ull;
        i64 *doo[2];
        IVX_TRY(ctx->get_scratch(WS_OUT_A, rows * sizeof(i64), (void **)&doo[0]));
        IVX_TRY(ctx->get_scratch(WS_OUT_B, rows * sizeof(i64), (void **)&doo[1]));
        IVX_TRY(host_chunked(ctx, key, start, end, n, nchunk, true, "hipMemcpyAsync(values)", [&](HostChunk &ch) -> ivx_status {
            KernelTimer t(ctx);
            IVX_TRY(probe(ch.key, ch.start, ch.end, ch.n, doo[ch.set]));
            ch.push(out + ch.c0, doo[ch.set], ch.n * sizeof(i64));
            return IVX_OK;
        }));
        f.rows_out(n);
        return IVX_OK;
    }
    const u32 *dk = f.in(key, n);
    const i32 *ds = f.in(start, n), *de = f.in(end, n);
    i64 *dout = f.out(out, n);
    IVX_TRY(f.run([&] { return probe(dk, ds, de, n, dout); }));
    f.rows_out(n);                                          // (an output batch only once it exists: a refused call has none)
    f.back_all();
    return f.finish();
}

extern "C" ivx_status ivx_probe_count(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key, const int32_t *start,
                                      const int32_t *end, uint64_t n, int strict, int64_t *out)
{
    return per_row_i64(ctx, ix, IVX_KIND_COUNT, mem, key, start, end, n, strict, out);
}

extern "C" ivx_status ivx_probe_coverage(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key, const int32_t *start,
                                         const int32_t *end, uint64_t n, int strict, int64_t *out)
{
    return per_row_i64(ctx, ix, IVX_KIND_COVERAGE, mem, key, start, end, n, strict, out);
}

extern "C" ivx_status ivx_probe_nearest(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key, const int32_t *start,
                                        const int32_t *end, uint64_t n, int strict, uint32_t k, int include_overlaps,
                                        uint32_t *build_idx, uint32_t *probe_idx, int64_t *distance, uint64_t cap, uint64_t *rows)
{
    Frame f(ctx, mem);
    IVX_TRY(check_probe_args(f, ix, IVX_KIND_NEAREST, start, end, n));
    if (!rows) return ctx->fail(IVX_ERR_INVALID, "null rows");
    *rows = 0;                                              // (a refused call leaves 0, not the caller's word)
    if (n && (!build_idx || !probe_idx)) return ctx->fail(IVX_ERR_INVALID, "null output column");
    if ((u64)k * n > 0xFFFFFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "nearest: k * rows too large");
    f.meter(false, n);
    const u32 *dk = f.in(key, n);
    const i32 *ds = f.in(start, n), *de = f.in(end, n);
    u32 *db = f.out(build_idx, cap), *dp = f.out(probe_idx, cap);
    i64 *dd = f.out(distance, cap);
    IVX_TRY(f.st);
    u64 r = 0;
    const ivx_status st = f.run([&] { return ivx_nearest_probe(ctx, ix, dk, ds, de, n, strict, k, include_overlaps, db, dp, dd, cap, &r); });
    *rows = r;
    if (st != IVX_OK) return st;
    f.rows_out(r);
    f.back_all(r);
    return f.finish();
}

// a6' (include/ivx_nearest.h): one side only and / or within a distance cap.  Without either it IS ivx_probe_nearest
extern "C" ivx_status ivx_probe_nearest_dir(ivx_ctx *ctx, const ivx_index *ix, int mem, const uint32_t *key, const int32_t *start,
                                            const int32_t *end, uint64_t n, int strict, uint32_t k, int include_overlaps,
                                            int direction, int64_t max_distance,
                                            uint32_t *build_idx, uint32_t *probe_idx, int64_t *distance, uint64_t cap, uint64_t *rows)
{
    if (direction == IVX_NEAR_ANY && max_distance < 0)
        return ivx_probe_nearest(ctx, ix, mem, key, start, end, n, strict, k, include_overlaps, build_idx, probe_idx, distance, cap, rows);
    Frame f(ctx, mem);
    IVX_TRY(check_probe_args(f, ix, IVX_KIND_NEAREST, start, end, n));
    if (!rows) return ctx->fail(IVX_ERR_INVALID, "null rows");
    *rows = 0;
    if (direction < 0 || direction >= IVX_NEAR_N) return ctx->fail(IVX_ERR_INVALID, "nearest: direction must be IVX_NEAR_ANY, IVX_NEAR_BEFORE or IVX_NEAR_AFTER");
    if (n && (!build_idx || !probe_idx)) return ctx->fail(IVX_ERR_INVALID, "null output column");
    if ((u64)k * n > 0xFFFFFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "nearest: k * rows too large");
    f.meter(false, n);
    const u32 *dk = f.in(key, n);
    const i32 *ds = f.in(start, n), *de = f.in(end, n);
    u32 *db = f.out(build_idx, cap), *dp = f.out(probe_idx, cap);
    i64 *dd = f.out(distance, cap);
    IVX_TRY(f.st);
    u64 r = 0;
    const ivx_status st = f.run([&] { return ivx_nearest_probe_dir(ctx, ix, dk, ds, de, n, strict, k, include_overlaps, direction, max_distance, db, dp, dd, cap, &r); });
    *rows = r;
    if (st != IVX_OK) return st;
    f.rows_out(r);
    f.back_all(r);
    return f.finish();
}

// ---------------------------------------------------------------- a7..a9

extern "C" ivx_status ivx_merge(ivx_ctx *ctx, int mem, const uint32_t *key, const int64_t *start, const int64_t *end, uint64_t n,
                                uint32_t n_keys, int64_t min_dist, int strict,
                                uint32_t *out_key, int64_t *out_start, int64_t *out_end, int64_t *out_n,
                                uint64_t cap, uint64_t *n_out)
{
    Frame f(ctx, mem);
    IVX_TRY(f.enter(n_out, "null n_out"));
    if (n && (!start || !end)) return ctx->fail(IVX_ERR_INVALID, "null coordinate column");
    if (min_dist < 0) return ctx->fail(IVX_ERR_INVALID, "merge() min_dist must be >= 0, got " + std::to_string(min_dist));   // table_function.rs:237
    if (cap < n) return ctx->fail(IVX_ERR_CAPACITY, "merge: output buffers need capacity n");
    if (n >= 0xFFFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "merge: more than 2^32-1 rows in one call");
    if (!key || n_keys == 0) n_keys = 1;
    const u32 *dk = f.in(key, n);
    const i64 *ds = f.in(start, n), *de = f.in(end, n);
    u32 *ok = f.out(out_key, n);
    i64 *os = f.out(out_start, n), *oe = f.out(out_end, n), *on = f.out(out_n, n);
    u64 m = 0;
    IVX_TRY(f.run([&] { return ivx_merge_device(ctx, dk, ds, de, n, n_keys, min_dist, strict, ok, os, oe, on, &m); }));
    *n_out = m;
    f.back_all(m);
    return f.finish();
}

extern "C" ivx_status ivx_subtract(ivx_ctx *ctx, int mem,
                                   const uint32_t *lkey, const int64_t *lstart, const int64_t *lend, uint64_t nl,
                                   const uint32_t *rkey, const int64_t *rstart, const int64_t *rend, uint64_t nr,
                                   uint32_t n_keys, int strict,
                                   uint32_t *out_key, int64_t *out_start, int64_t *out_end, uint32_t *out_row,
                                   uint64_t cap, uint64_t *n_out)
{
    Frame f(ctx, mem);
    IVX_TRY(f.enter(n_out, "null n_out"));
    if ((nl && (!lstart || !lend)) || (nr && (!rstart || !rend))) return ctx->fail(IVX_ERR_INVALID, "null coordinate column");
    if (nl >= 0xFFFFFFFFull || nr >= 0xFFFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "subtract: more than 2^32-1 rows in one call");
    if ((lkey == nullptr) != (rkey == nullptr) && nl && nr) return ctx->fail(IVX_ERR_INVALID, "subtract: key given for one side only");
    if (n_keys == 0 || (!lkey && !rkey)) n_keys = 1;
    IVX_TRY(f.device());
    // a fill call right after the sizing call for the same arguments: the sorted sides, gap heads and output
    // offsets are still in the context (nothing else ran in between), only the output pass is left
    const void *in[6] = {lkey, lstart, lend, rkey, rstart, rend};
    ivx_sub_plan &pl = ctx->sub_plan;
    const bool sizing = cap == 0 && !out_key && !out_start && !out_end && !out_row;
    const bool planned = !sizing && nl && pl.valid && !getenv("IVX_NO_PLAN") && pl.mem == mem && memcmp(pl.in, in, sizeof(in)) == 0 && pl.nl == nl && pl.nr == nr &&
                         pl.nkeys == n_keys && pl.strict == strict && pl.stream == ctx->stream;
    const u32 *dlk = nullptr, *drk = nullptr; const i64 *dls = nullptr, *dle = nullptr, *drs = nullptr, *dre = nullptr;
    if (!planned) {
        dlk = f.in(lkey, nl); dls = f.in(lstart, nl); dle = f.in(lend, nl);
        drk = f.in(rkey, nr); drs = f.in(rstart, nr); dre = f.in(rend, nr);
    }
    u32 *ok = f.out(out_key, cap);
    i64 *os = f.out(out_start, cap), *oe = f.out(out_end, cap);
    u32 *orow = f.out(out_row, cap);
    IVX_TRY(f.st);
    u64 m = 0;
    const ivx_status st = f.run([&]() -> ivx_status {
        if (!planned) pl.valid = false;                     // whatever an earlier sizing call left is gone now
        return planned ? ivx_subtract_fill_planned(ctx, ok, os, oe, orow, cap, &m)
                       : ivx_subtract_device(ctx, dlk, dls, dle, nl, drk, drs, dre, nr, n_keys, strict, ok, os, oe, orow, cap, &m);
    });
    *n_out = m;
    if (st != IVX_OK) { if (st != IVX_ERR_CAPACITY) pl.valid = false; return st; }
    if (planned) ctx->sub_fills_planned++;
    if (planned) pl.valid = false;                          // consumed: the next fill call sorts and counts again (its input columns may have been refilled in place)
    if (sizing && pl.valid) { memcpy(pl.in, in, sizeof(in)); pl.mem = mem; }
    if (cap) f.back_all(m);
    return f.finish();
}

// ivx_intersect, and the same call with the count pass's report (the test hook below)
static ivx_status intersect_impl(ivx_ctx *ctx, int mem,
                                 const uint32_t *lkey, const int64_t *lstart, const int64_t *lend, uint64_t nl,
                                 const uint32_t *rkey, const int64_t *rstart, const int64_t *rend, uint64_t nr,
                                 uint32_t n_keys, int strict,
                                 uint32_t *out_key, int64_t *out_start, int64_t *out_end, uint32_t *out_row,
                                 uint64_t cap, uint64_t *n_out, const ivx_isect_debug *dbg)
{
    Frame f(ctx, mem);
    IVX_TRY(f.enter(n_out, "null n_out"));
    if ((nl && (!lstart || !lend)) || (nr && (!rstart || !rend))) return ctx->fail(IVX_ERR_INVALID, "null coordinate column");
    if (nl >= 0xFFFFFFFFull || nr >= 0xFFFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "intersect: more than 2^32-1 rows in one call");
    if ((lkey == nullptr) != (rkey == nullptr) && nl && nr) return ctx->fail(IVX_ERR_INVALID, "intersect: key given for one side only");
    if (n_keys == 0 || (!lkey && !rkey)) n_keys = 1;
    f.drop_plans();                                         // as any other call between a sizing call and its fill
    const u32 *dlk = f.in(lkey, nl);
    const i64 *dls = f.in(lstart, nl), *dle = f.in(lend, nl);
    const u32 *drk = f.in(rkey, nr);
    const i64 *drs = f.in(rstart, nr), *dre = f.in(rend, nr);
    u32 *ok = f.out(out_key, cap);
    i64 *os = f.out(out_start, cap), *oe = f.out(out_end, cap);
    u32 *orow = f.out(out_row, cap);
    IVX_TRY(f.st);
    u64 m = 0;
    const ivx_status st = f.run([&] { return ivx_intersect_device(ctx, dlk, dls, dle, nl, drk, drs, dre, nr, n_keys, strict, ok, os, oe, orow, cap, &m, dbg); });
    *n_out = m;
    if (st != IVX_OK) return st;
    if (cap) f.back_all(m);
    return f.finish();
}

extern "C" ivx_status ivx_intersect(ivx_ctx *ctx, int mem,
                                    const uint32_t *lkey, const int64_t *lstart, const int64_t *lend, uint64_t nl,
                                    const uint32_t *rkey, const int64_t *rstart, const int64_t *rend, uint64_t nr,
                                    uint32_t n_keys, int strict,
                                    uint32_t *out_key, int64_t *out_start, int64_t *out_end, uint32_t *out_row,
                                    uint64_t cap, uint64_t *n_out)
{
    return intersect_impl(ctx, mem, lkey, lstart, lend, nl, rkey, rstart, rend, nr, n_keys, strict, out_key, out_start, out_end, out_row, cap, n_out, nullptr);
}

// Test hook (not in include/ivx.h; tests/test_gpu_intersect_edges.py): an intersect SIZING call for these inputs that also says
// what its count pass did.  wg: frag_dbg_words<IsectOp> words per workgroup (k_frag_count, ivx_sweep.hip; ivx_debug_intersect_geometry
// gives the constants), row_esc: one byte per left row at its original index; both HOST buffers in either mode, capacities in
// workgroups / rows.  *n_wg and *n_rows are set before the capacities are checked (IVX_ERR_CAPACITY); both are 0, and nothing is
// written, when a side is empty.
extern "C" ivx_status ivx_debug_intersect_paths(ivx_ctx *ctx, int mem,
                                                const uint32_t *lkey, const int64_t *lstart, const int64_t *lend, uint64_t nl,
                                                const uint32_t *rkey, const int64_t *rstart, const int64_t *rend, uint64_t nr,
                                                uint32_t n_keys, int strict, uint32_t *wg, uint64_t wg_cap, uint8_t *row_esc, uint64_t row_cap,
                                                uint64_t *n_wg, uint64_t *n_rows, uint64_t *n_out)
{
    if (!ctx) return IVX_ERR_INVALID;
    if (!n_wg || !n_rows) return ctx->fail(IVX_ERR_INVALID, "debug_intersect_paths: null n_wg / n_rows");
    *n_wg = 0; *n_rows = 0;
    const ivx_isect_debug dbg{wg, wg_cap, row_esc, row_cap, n_wg, n_rows};
    const ivx_status st = intersect_impl(ctx, mem, lkey, lstart, lend, nl, rkey, rstart, rend, nr, n_keys, strict, nullptr, nullptr, nullptr, nullptr, 0, n_out, &dbg);
    if (st != IVX_OK) return st;
    IVX_HIP(ctx, hipStreamSynchronize(ctx->stream));        // (the two report copies; the count's read-back has waited for them already)
    return IVX_OK;
}

extern "C" ivx_status ivx_cluster(ivx_ctx *ctx, int mem, const uint32_t *key, const int64_t *start, const int64_t *end, uint64_t n,
                                  uint32_t n_keys, int64_t min_dist, int strict, const int64_t *key_base,
                                  uint32_t *out_key, int64_t *out_start, int64_t *out_end, uint32_t *out_row,
                                  int64_t *out_cluster, int64_t *out_cluster_start, int64_t *out_cluster_end,
                                  uint64_t *key_clusters, uint64_t *n_clusters)
{
    Frame f(ctx, mem);
    IVX_TRY(f.enter(n_clusters, "null n_clusters"));
    if (n && (!start || !end)) return ctx->fail(IVX_ERR_INVALID, "null coordinate column");
    if (min_dist < 0) return ctx->fail(IVX_ERR_INVALID, "cluster() min_dist must be >= 0, got " + std::to_string(min_dist));   // table_function.rs:237
    if (n >= 0xFFFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "cluster: more than 2^32-1 rows in one call");
    if (!key || n_keys == 0) n_keys = 1;
    const u32 *dk = f.in(key, n);
    const i64 *ds = f.in(start, n), *de = f.in(end, n), *dbase = f.in(key_base, (u64)n_keys);
    u32 *ok = f.out(out_key, n);
    i64 *os = f.out(out_start, n), *oe = f.out(out_end, n);
    u32 *orow = f.out(out_row, n);
    i64 *oc = f.out(out_cluster, n), *ocs = f.out(out_cluster_start, n), *oce = f.out(out_cluster_end, n);
    u64 *okc = f.out(key_clusters, (u64)n_keys);
    u64 m = 0;
    IVX_TRY(f.run([&] { return ivx_cluster_device(ctx, dk, ds, de, n, n_keys, min_dist, strict, dbase, ok, os, oe, orow, oc, ocs, oce, okc, &m); }));
    *n_clusters = m;
    f.back_all();                                           // (every row column in full: n rows; key_clusters: n_keys)
    return f.finish();
}

extern "C" ivx_status ivx_complement(ivx_ctx *ctx, int mem, const uint32_t *key, const int64_t *start, const int64_t *end, uint64_t n,
                                     const uint32_t *vkey, const int64_t *vstart, const int64_t *vend, uint64_t nv,
                                     uint32_t n_keys, int strict, uint32_t *out_key, int64_t *out_start, int64_t *out_end,
                                     uint64_t cap, uint64_t *n_out)
{
    Frame f(ctx, mem);
    IVX_TRY(f.enter(n_out, "null n_out"));
    if ((n && (!start || !end)) || (nv && (!vstart || !vend))) return ctx->fail(IVX_ERR_INVALID, "null coordinate column");
    if (n >= 0xFFFFFFFFull || nv >= 0xFFFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "complement: more than 2^32-1 rows in one call");
    if ((key == nullptr) != (vkey == nullptr) && n && nv) return ctx->fail(IVX_ERR_INVALID, "complement: key given for one side only");
    if (n_keys == 0 || (!key && !vkey)) n_keys = 1;
    const u32 *dk = f.in(key, n);
    const i64 *ds = f.in(start, n), *de = f.in(end, n);
    const u32 *dvk = f.in(vkey, nv);
    const i64 *dvs = f.in(vstart, nv), *dve = f.in(vend, nv);
    u32 *ok = f.out(out_key, cap);
    i64 *os = f.out(out_start, cap), *oe = f.out(out_end, cap);
    u64 m = 0;
    const ivx_status st = f.run([&] { return ivx_complement_device(ctx, dk, ds, de, n, dvk, dvs, dve, nv, n_keys, strict, ok, os, oe, cap, &m); });
    *n_out = m;
    if (st != IVX_OK) return st;
    if (cap) f.back_all(m);
    return f.finish();
}

// ---------------------------------------------------------------- g: depth()

namespace {

// the cigar column of the text calls: an Arrow Utf8 (large = 0) / LargeUtf8 (1) column
struct TextIn { int large; const void *off; const uint8_t *text; };

// the caller's columns of a depth() call: the reads with their cigar column as packed ops (cigar_offsets / cigar_ops) or as
// text (text, the other two null), the weighted segments, the key table and the read filters
struct DepthArgs {
    const u32 *rkey, *rpos, *rflags, *rmapq; const i32 *cigar_offsets; const u32 *cigar_ops; const TextIn *text; u64 n_reads;
    const u32 *skey, *sstart, *send; const i32 *sweight; u64 n_seg;
    u32 n_keys; const u32 *key_len; u32 filter_flag, min_mapq;
};

// ... and the same columns on the device
struct DepthIn {
    const u32 *rkey, *rpos, *rflags, *rmapq, *ops, *skey, *ss, *se, *key_len; const i32 *off, *sw;
};

// the checks made on the host, from check_mem() on
ivx_status depth_check_args(Frame &f, DepthArgs *a)
{
    ivx_ctx *ctx = f.ctx;
    const void *offsets = a->cigar_offsets;
    if (a->text) {
        if (a->text->large != 0 && a->text->large != 1) return ctx->fail(IVX_ERR_INVALID, "cigar: large must be 0 (Utf8) or 1 (LargeUtf8)");
        offsets = a->text->off;                                 // (for the null check only)
    }
    IVX_TRY(f.check_mem());
    if (a->n_reads && (!a->rpos || !offsets)) return ctx->fail(IVX_ERR_INVALID, "depth: null read position or CIGAR offset column");
    if (a->n_seg && (!a->sstart || !a->send)) return ctx->fail(IVX_ERR_INVALID, "depth: null segment coordinate column");
    if (a->n_reads >= 0xFFFFFFFFull || a->n_seg >= 0x7FFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "depth: too many rows in one call");
    if (a->n_keys == 0 && !a->rkey && !a->skey) a->n_keys = 1;
    return IVX_OK;
}

ivx_status depth_stage_in(Frame &f, const DepthArgs &a, DepthIn *d)
{
    IVX_TRY(f.device());
    // IVX_MEM_HOST: the ops column is staged up to the last offset (the device checks the offsets before it reads an op)
    u64 n_ops_host = 0;
    if (f.mem == IVX_MEM_HOST && a.n_reads && a.cigar_offsets && a.cigar_offsets[a.n_reads] > 0) n_ops_host = (u64)a.cigar_offsets[a.n_reads] / 4;   // (null: the text calls)
    if (n_ops_host && !a.cigar_ops) return f.ctx->fail(IVX_ERR_INVALID, "depth: null CIGAR data buffer");
    d->rkey = f.in(a.rkey, a.n_reads); d->rpos = f.in(a.rpos, a.n_reads); d->rflags = f.in(a.rflags, a.n_reads); d->rmapq = f.in(a.rmapq, a.n_reads);
    d->off = f.in(a.n_reads ? a.cigar_offsets : nullptr, a.n_reads + 1);
    d->ops = f.in(a.cigar_ops, n_ops_host);
    d->skey = f.in(a.skey, a.n_seg); d->ss = f.in(a.sstart, a.n_seg); d->se = f.in(a.send, a.n_seg); d->sw = f.in(a.sweight, a.n_seg);
    d->key_len = f.in(a.key_len, (u64)a.n_keys);
    return f.st;
}

// the text column on the device.  IVX_MEM_HOST: the offsets, and the bytes between the first and the last offset (the extent
// is read from the host offsets, as depth_stage_in does for ops; the device checks the offsets before it reads a byte
// through one, and offsets that pass name bytes inside the extent) -- *at_off0: *dtext is the byte at offset off[0]
ivx_status cigar_stage_text(Frame &f, const TextIn &t, u64 n_reads, const void **doff, const u8 **dtext, bool *at_off0)
{
    ivx_ctx *ctx = f.ctx;
    *at_off0 = false;
    if (f.mem == IVX_MEM_DEVICE) { *doff = t.off; *dtext = t.text; return IVX_OK; }
    const i64 o0 = t.large ? ((const i64 *)t.off)[0] : (i64)((const i32 *)t.off)[0];
    const i64 oN = t.large ? ((const i64 *)t.off)[n_reads] : (i64)((const i32 *)t.off)[n_reads];
    u64 extent = 0;
    if (o0 >= 0 && oN > o0) {
        extent = (u64)(oN - o0);
        if (extent >= (1ull << 32)) return ctx->fail(IVX_ERR_INVALID, "cigar: 2^32 or more bytes of CIGAR text in one call");
        if (!t.text) return ctx->fail(IVX_ERR_INVALID, "cigar: null text buffer");
    }
    *doff = f.in_at(WS_IN_TEXTOFF, (const u8 *)t.off, (n_reads + 1) * (t.large ? 8 : 4));
    *dtext = nullptr;
    if (extent) { *dtext = f.in_at(WS_IN_TEXT, t.text + o0, extent); *at_off0 = true; }
    return f.st;
}

// the text column parsed into context scratch (the slots of the binary cigar column, which a text call leaves empty):
// d->off / d->ops as the binary calls take them
ivx_status depth_parse_text(Frame &f, const TextIn &t, u64 n_reads, DepthIn *d)
{
    ivx_ctx *ctx = f.ctx;
    d->off = nullptr; d->ops = nullptr;
    if (n_reads == 0) return IVX_OK;
    const void *doff; const u8 *dtext; bool at0;
    IVX_TRY(cigar_stage_text(f, t, n_reads, &doff, &dtext, &at0));
    ivx_cigar_plan P;
    IVX_TRY(ivx_cigar_count(ctx, t.large, doff, dtext, at0, n_reads, &P));
    i32 *off; u32 *ops;
    IVX_TRY(ctx->get_scratch(WS_IN2_START, (size_t)(n_reads + 1) * sizeof(i32), (void **)&off));
    IVX_TRY(ctx->get_scratch(WS_IN2_END, (size_t)P.n_ops * sizeof(u32), (void **)&ops));
    IVX_TRY(ivx_cigar_write(ctx, P, off, ops));
    d->off = off; d->ops = ops;
    return IVX_OK;
}

// ivx_depth (a.text = null) and ivx_depth_text (the cigar column as text, parsed into context scratch first)
ivx_status depth_call(ivx_ctx *ctx, int mem, DepthArgs a,
                      uint32_t *out_key, uint32_t *out_start, uint32_t *out_end, int32_t *out_cov, uint64_t cap, uint64_t *n_out)
{
    Frame f(ctx, mem);
    IVX_TRY(f.begin(n_out, "null n_out"));
    IVX_TRY(depth_check_args(f, &a));
    f.drop_plans();                                         // as any other call between a sizing call and its fill
    f.meter(false, a.n_reads + a.n_seg);
    if (a.n_reads == 0 && a.n_seg == 0) return IVX_OK;
    DepthIn d;
    IVX_TRY(depth_stage_in(f, a, &d));
    u32 *ok = f.out(out_key, cap), *os = f.out(out_start, cap), *oe = f.out(out_end, cap);
    i32 *oc = f.out(out_cov, cap);
    const bool sizing = cap == 0 && !out_key && !out_start && !out_end && !out_cov;
    u64 m = 0;
    const ivx_status st = f.run([&]() -> ivx_status {
        if (a.text) IVX_TRY(depth_parse_text(f, *a.text, a.n_reads, &d));
        return ivx_depth_device(ctx, d.rkey, d.rpos, d.rflags, d.rmapq, d.off, d.ops, a.n_reads, d.skey, d.ss, d.se, d.sw, a.n_seg,
                                a.n_keys, d.key_len, a.filter_flag, a.min_mapq, ok, os, oe, oc, cap, &m);
    });
    *n_out = m;
    if (st != IVX_OK) return st;
    if (!sizing) { f.rows_out(m); f.back_all(m); }
    return f.finish();
}

// ivx_depth_profile_build and its text form: the same inputs, kept as a depth profile on the device
ivx_status depth_profile_call(ivx_ctx *ctx, int mem, DepthArgs a, ivx_index **out)
{
    Frame f(ctx, mem);
    IVX_TRY(f.begin(out, "null out"));
    IVX_TRY(depth_check_args(f, &a));
    f.drop_plans();                                         // as any other call between a sizing call and its fill
    f.meter(true, a.n_reads + a.n_seg);
    DepthIn d{};
    if (a.n_reads || a.n_seg) IVX_TRY(depth_stage_in(f, a, &d));
    else IVX_TRY(f.device());
    ivx_index *ix;
    IVX_TRY(index_new(ctx, IVX_KIND_DEPTH_PROFILE, 0, a.n_keys, &ix));
    u8 *seen = nullptr;
    ivx_depth_evs evs{0, nullptr, nullptr};
    ivx_status st = ivx_depth_profile_begin(ctx, ix, &seen);
    if (st == IVX_OK) st = f.run([&]() -> ivx_status {
        if (a.text) IVX_TRY(depth_parse_text(f, *a.text, a.n_reads, &d));
        IVX_TRY(ivx_depth_events(ctx, d.rkey, d.rpos, d.rflags, d.rmapq, d.off, d.ops, a.n_reads, d.skey, d.ss, d.se, d.sw, a.n_seg,
                                 a.n_keys, d.key_len, a.filter_flag, a.min_mapq, seen, &evs));
        return ivx_depth_profile_finish(ctx, ix, evs);
    });
    return index_commit(ctx, ix, st, "depth profile build failed on device", out);
}

}  // namespace

extern "C" ivx_status ivx_depth(ivx_ctx *ctx, int mem,
                                const uint32_t *rkey, const uint32_t *rpos, const uint32_t *rflags, const uint32_t *rmapq,
                                const int32_t *cigar_offsets, const uint32_t *cigar_ops, uint64_t n_reads,
                                const uint32_t *skey, const uint32_t *sstart, const uint32_t *send, const int32_t *sweight, uint64_t n_seg,
                                uint32_t n_keys, const uint32_t *key_len, uint32_t filter_flag, uint32_t min_mapq,
                                uint32_t *out_key, uint32_t *out_start, uint32_t *out_end, int32_t *out_cov,
                                uint64_t cap, uint64_t *n_out)
{
    const DepthArgs a{rkey, rpos, rflags, rmapq, cigar_offsets, cigar_ops, nullptr, n_reads, skey, sstart, send, sweight, n_seg, n_keys, key_len, filter_flag, min_mapq};
    return depth_call(ctx, mem, a, out_key, out_start, out_end, out_cov, cap, n_out);
}

extern "C" ivx_status ivx_depth_text(ivx_ctx *ctx, int mem,
                                     const uint32_t *rkey, const uint32_t *rpos, const uint32_t *rflags, const uint32_t *rmapq,
                                     int large, const void *text_offsets, const uint8_t *text, uint64_t n_reads,
                                     const uint32_t *skey, const uint32_t *sstart, const uint32_t *send, const int32_t *sweight, uint64_t n_seg,
                                     uint32_t n_keys, const uint32_t *key_len, uint32_t filter_flag, uint32_t min_mapq,
                                     uint32_t *out_key, uint32_t *out_start, uint32_t *out_end, int32_t *out_cov,
                                     uint64_t cap, uint64_t *n_out)
{
    const TextIn t{large, text_offsets, text};
    const DepthArgs a{rkey, rpos, rflags, rmapq, nullptr, nullptr, &t, n_reads, skey, sstart, send, sweight, n_seg, n_keys, key_len, filter_flag, min_mapq};
    return depth_call(ctx, mem, a, out_key, out_start, out_end, out_cov, cap, n_out);
}

extern "C" ivx_status ivx_cigar_parse(ivx_ctx *ctx, int mem, int large, const void *text_offsets, const uint8_t *text, uint64_t n_reads,
                                      int32_t *out_offsets, uint32_t *out_ops, uint64_t cap_ops, uint64_t *n_ops)
{
    Frame f(ctx, mem);
    IVX_TRY(f.enter(n_ops, "null n_ops"));
    if (large != 0 && large != 1) return ctx->fail(IVX_ERR_INVALID, "cigar: large must be 0 (Utf8) or 1 (LargeUtf8)");
    if (n_reads >= 0xFFFFFFFFull) return ctx->fail(IVX_ERR_INVALID, "cigar: too many rows in one call");
    f.drop_plans();                                         // as any other call between a sizing call and its fill
    if (n_reads == 0) return IVX_OK;
    if (!text_offsets) return ctx->fail(IVX_ERR_INVALID, "cigar: null text offset column");
    IVX_TRY(f.device());
    const TextIn t{large, text_offsets, text};
    const void *doff; const u8 *dtext; bool at0;
    IVX_TRY(cigar_stage_text(f, t, n_reads, &doff, &dtext, &at0));
    ivx_cigar_plan P;
    IVX_TRY(ivx_cigar_count(ctx, large, doff, dtext, at0, n_reads, &P));
    *n_ops = P.n_ops;
    // the op lengths are checked in every call, a counting call included; ops are written only into a buffer that holds all
    const bool fits = out_ops && cap_ops >= P.n_ops;
    i32 *ooff = f.out(out_offsets, n_reads + 1);
    u32 *oops = fits ? f.out(out_ops, P.n_ops) : nullptr;
    IVX_TRY(f.st);
    IVX_TRY(ivx_cigar_write(ctx, P, ooff, oops));
    f.back_all();
    IVX_TRY(f.st);
    IVX_HIP(ctx, hipStreamSynchronize(ctx->stream));        // (in both modes)
    if (out_ops && !fits) return ctx->fail(IVX_ERR_CAPACITY, "cigar: op buffer too small");
    if (!out_ops && cap_ops && cap_ops < P.n_ops) return ctx->fail(IVX_ERR_CAPACITY, "cigar: op buffer too small");
    return IVX_OK;
}

// ---------------------------------------------------------------- g': depth profiles (per-base depth())

extern "C" ivx_status ivx_depth_profile_build(ivx_ctx *ctx, int mem,
                                              const uint32_t *rkey, const uint32_t *rpos, const uint32_t *rflags, const uint32_t *rmapq,
                                              const int32_t *cigar_offsets, const uint32_t *cigar_ops, uint64_t n_reads,
                                              const uint32_t *skey, const uint32_t *sstart, const uint32_t *send, const int32_t *sweight, uint64_t n_seg,
                                              uint32_t n_keys, const uint32_t *key_len, uint32_t filter_flag, uint32_t min_mapq,
                                              ivx_index **out)
{
    const DepthArgs a{rkey, rpos, rflags, rmapq, cigar_offsets, cigar_ops, nullptr, n_reads, skey, sstart, send, sweight, n_seg, n_keys, key_len, filter_flag, min_mapq};
    return depth_profile_call(ctx, mem, a, out);
}

extern "C" ivx_status ivx_depth_profile_build_text(ivx_ctx *ctx, int mem,
                                                   const uint32_t *rkey, const uint32_t *rpos, const uint32_t *rflags, const uint32_t *rmapq,
                                                   int large, const void *text_offsets, const uint8_t *text, uint64_t n_reads,
                                                   const uint32_t *skey, const uint32_t *sstart, const uint32_t *send, const int32_t *sweight, uint64_t n_seg,
                                                   uint32_t n_keys, const uint32_t *key_len, uint32_t filter_flag, uint32_t min_mapq,
                                                   ivx_index **out)
{
    const TextIn t{large, text_offsets, text};
    const DepthArgs a{rkey, rpos, rflags, rmapq, nullptr, nullptr, &t, n_reads, skey, sstart, send, sweight, n_seg, n_keys, key_len, filter_flag, min_mapq};
    return depth_profile_call(ctx, mem, a, out);
}

extern "C" void ivx_depth_profile_free(ivx_index *p) { if (p && p->kind == IVX_KIND_DEPTH_PROFILE) ivx_index_free(p); }
extern "C" uint64_t ivx_depth_profile_steps(const ivx_index *p) { return p && p->kind == IVX_KIND_DEPTH_PROFILE ? p->dp.steps : 0; }
extern "C" uint64_t ivx_depth_profile_device_bytes(const ivx_index *p) { return p && p->kind == IVX_KIND_DEPTH_PROFILE ? p->bytes : 0; }

// the head of every call on a profile, after the frame's begin(): the profile, check_mem(), the device
static ivx_status check_profile_args(Frame &f, const ivx_index *p)
{
    ivx_ctx *ctx = f.ctx;
    if (!p) return ctx->fail(IVX_ERR_INVALID, "null depth profile");
    if (p->kind != IVX_KIND_DEPTH_PROFILE) return ctx->fail(IVX_ERR_UNSUPPORTED, "not a depth profile");
    if (p->device != ctx->device) return ctx->fail(IVX_ERR_INVALID, "depth profile lives on another device");
    IVX_TRY(f.check_mem());
    return f.device();
}

extern "C" ivx_status ivx_depth_profile_read(ivx_ctx *ctx, const ivx_index *p, int mem,
                                             uint32_t *out_key, uint32_t *out_pos, int32_t *out_cov, uint8_t *key_seen,
                                             uint64_t cap, uint64_t *n_out)
{
    Frame f(ctx, mem);
    IVX_TRY(f.begin(n_out, "null n_out"));
    IVX_TRY(check_profile_args(f, p));
    const DepthProfileView &dp = p->dp;
    const hipMemcpyKind kind = mem == IVX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    *n_out = dp.steps;
    if (key_seen && p->nkeys) IVX_HIP(ctx, hipMemcpyAsync(key_seen, dp.seen, p->nkeys, kind, ctx->stream));
    const bool sizing = cap == 0 && !out_key && !out_pos && !out_cov;
    ivx_status st = IVX_OK;
    if (!sizing && dp.steps > cap) st = ctx->fail(IVX_ERR_CAPACITY, "depth profile: output buffers too small");
    else if (!sizing && dp.steps) {
        if (out_key) IVX_HIP(ctx, hipMemcpyAsync(out_key, dp.key, dp.steps * sizeof(u32), kind, ctx->stream));
        if (out_pos) IVX_HIP(ctx, hipMemcpyAsync(out_pos, dp.pos, dp.steps * sizeof(u32), kind, ctx->stream));
        if (out_cov) IVX_HIP(ctx, hipMemcpyAsync(out_cov, dp.cov, dp.steps * sizeof(i32), kind, ctx->stream));
    }
    IVX_TRY(f.finish());                                    // (key_seen has gone out whatever st says)
    return st;
}

extern "C" ivx_status ivx_depth_profile_expand(ivx_ctx *ctx, const ivx_index *p, int mem,
                                               uint32_t key, uint32_t first_pos, uint64_t n, int skip_pos0,
                                               int32_t *out_pos, void *out_cov)
{
    Frame f(ctx, mem);
    IVX_TRY(f.begin());
    IVX_TRY(check_profile_args(f, p));
    if (key >= p->nkeys) return ctx->fail(IVX_ERR_INVALID, "depth profile: key id >= n_keys");
    if (n > 0x100000000ull || (u64)first_pos + n > 0x100000000ull) return ctx->fail(IVX_ERR_INVALID, "depth profile: window ends beyond position 2^32 - 1");
    if (mem == IVX_MEM_DEVICE && ((((uintptr_t)out_pos) & 3u) || (((uintptr_t)out_cov) & 1u)))
        return ctx->fail(IVX_ERR_INVALID, "depth profile: output pointer not aligned to its element size");
    f.drop_plans();
    if (n == 0) return IVX_OK;
    i32 *dpos = f.out(out_pos, n);
    int16_t *dcov = f.out((int16_t *)out_cov, n);
    IVX_TRY(f.run([&] { return ivx_depth_expand_device(ctx, p->dp, key, first_pos, n, skip_pos0 != 0, dpos, dcov); }));
    f.back_all();
    return f.finish();
}

extern "C" ivx_status ivx_depth_profile_merge(ivx_ctx *ctx, const ivx_index *a, const ivx_index *b, ivx_index **out)
{
    Frame f(ctx, IVX_MEM_DEVICE);
    IVX_TRY(f.begin(out, "null out"));
    IVX_TRY(check_profile_args(f, a));
    IVX_TRY(check_profile_args(f, b));
    f.drop_plans();                                         // as any other call between a sizing call and its fill
    if (a->dp.steps + b->dp.steps >= 0xFFFFFF00ull)
        return ctx->fail(IVX_ERR_INVALID, "depth profile merge: more than 2^32-257 steps in the two profiles");
    f.meter(true, a->dp.steps + b->dp.steps);
    ivx_index *ix;
    IVX_TRY(index_new(ctx, IVX_KIND_DEPTH_PROFILE, 0, a->nkeys > b->nkeys ? a->nkeys : b->nkeys, &ix));
    u8 *seen = nullptr;
    ivx_status st = ivx_depth_profile_begin(ctx, ix, &seen);
    if (st == IVX_OK) st = f.run([&] { return ivx_depth_profile_merge_device(ctx, a->dp, a->nkeys, b->dp, b->nkeys, ix); });
    return index_commit(ctx, ix, st, "depth profile merge failed on device", out);
}

extern "C" ivx_status ivx_depth_profile_blocks(ivx_ctx *ctx, const ivx_index *p, int mem,
                                               uint32_t *out_key, uint32_t *out_start, uint32_t *out_end, int32_t *out_cov,
                                               uint64_t cap, uint64_t *n_out)
{
    Frame f(ctx, mem);
    IVX_TRY(f.begin(n_out, "null n_out"));
    IVX_TRY(check_profile_args(f, p));
    f.drop_plans();
    f.meter(false, p->dp.steps);
    u32 *ok = f.out(out_key, cap), *os = f.out(out_start, cap), *oe = f.out(out_end, cap);
    i32 *oc = f.out(out_cov, cap);
    const bool sizing = cap == 0 && !out_key && !out_start && !out_end && !out_cov;
    u64 m = 0;
    const ivx_status st = f.run([&] { return ivx_depth_profile_blocks_device(ctx, p->dp, ok, os, oe, oc, cap, &m); });
    *n_out = m;
    if (st != IVX_OK) return st;
    if (!sizing) { f.rows_out(m); f.back_all(m); }
    return f.finish();
}

// ---- region statistics of a profile.  Where the regions come from: a table of (key, start, end) rows, clipped to the key's
// domain [pos_lo, key_hi[key]], or n windows of `width` positions of one key from first_pos on, cut at last_pos
namespace {

using RegionSrc = DepthRegionSrc;         // (the table's columns as the caller gave them, until regions_stage)
RegionSrc region_table(const u32 *qkey, const u32 *qstart, const u32 *qend, u64 n, u32 pos_lo, const u32 *key_hi, int skip_pos0)
{
    return RegionSrc{false, qkey, qstart, qend, pos_lo, key_hi, 0, 0, 0, 0, n, skip_pos0 != 0};
}
RegionSrc region_windows(u32 key, u32 first_pos, u32 last_pos, u32 width, u64 n, int skip_pos0)
{
    return RegionSrc{true, nullptr, nullptr, nullptr, 0, nullptr, key, first_pos, last_pos, width, n, skip_pos0 != 0};
}

// the checks of the source, after the statistic's own; then the call counts as made (the caller returns if it has no region)
ivx_status regions_begin(Frame &f, const ivx_index *p, const RegionSrc &r)
{
    ivx_ctx *ctx = f.ctx;
    f.drop_plans();
    if (r.windows) {
        if (r.width == 0) return ctx->fail(IVX_ERR_INVALID, "depth profile: window width 0");
        if (r.key >= p->nkeys) return ctx->fail(IVX_ERR_INVALID, "depth profile: key id >= n_keys");
        if (r.n && (r.n - 1) > (0xFFFFFFFFull - r.first_pos) / r.width)
            return ctx->fail(IVX_ERR_INVALID, "depth profile: a window starts beyond position 2^32 - 1");
    } else {
        if (r.n && (!r.qstart || !r.qend)) return ctx->fail(IVX_ERR_INVALID, "null coordinate column");
        if (f.mem == IVX_MEM_DEVICE && ((((uintptr_t)r.qkey) | ((uintptr_t)r.qstart) | ((uintptr_t)r.qend) | ((uintptr_t)r.key_hi)) & 3u))
            return ctx->fail(IVX_ERR_INVALID, "depth profile: input pointer not aligned to its element size");
    }
    f.meter(false, r.n);
    return IVX_OK;
}

// the source as the device entries take it: the table's columns on the device
RegionSrc regions_stage(Frame &f, const ivx_index *p, RegionSrc r)
{
    if (r.windows) return r;
    r.qkey = f.in(r.qkey, r.n); r.qstart = f.in(r.qstart, r.n); r.qend = f.in(r.qend, r.n);
    r.key_hi = f.in_at(WS_IN_KEYLEN, r.key_hi, p->nkeys);
    return r;
}

// bases, coverage sum and bases at or above each threshold, per region
ivx_status depth_summary(ivx_ctx *ctx, const ivx_index *p, int mem, const RegionSrc &r, const int32_t *thresholds, uint32_t n_thr,
                         int64_t *out_len, int64_t *out_sum, int64_t *out_ge)
{
    Frame f(ctx, mem);
    IVX_TRY(f.begin());
    IVX_TRY(check_profile_args(f, p));
    if (n_thr > IVX_DEPTH_MAX_THRESHOLDS) return ctx->fail(IVX_ERR_INVALID, "depth profile: more than 8 thresholds");
    if (n_thr && !thresholds) return ctx->fail(IVX_ERR_INVALID, "depth profile: null thresholds");
    if (mem == IVX_MEM_DEVICE && ((((uintptr_t)out_len) | ((uintptr_t)out_sum) | ((uintptr_t)out_ge)) & 7u))
        return ctx->fail(IVX_ERR_INVALID, "depth profile: output pointer not aligned to its element size");
    IVX_TRY(regions_begin(f, p, r));
    if (r.n == 0) return IVX_OK;
    const RegionSrc d = regions_stage(f, p, r);
    i64 *ol = f.out(out_len, r.n), *os = f.out(out_sum, r.n), *og = f.out(out_ge, (u64)n_thr * r.n);
    IVX_TRY(f.run([&] { return ivx_depth_region_sums_device(ctx, p->dp, p->nkeys, d, thresholds, n_thr, ol, os, og); }));
    f.rows_out(r.n);
    f.back_all();
    return f.finish();
}

// bases, min, max and the quantiles q_num[j] / q_den of the per-base coverage, per region
ivx_status depth_ranks(ivx_ctx *ctx, const ivx_index *p, int mem, const RegionSrc &r, const uint32_t *q_num, uint32_t n_q, uint32_t q_den,
                       int64_t *out_len, int32_t *out_min, int32_t *out_max, int32_t *out_q)
{
    Frame f(ctx, mem);
    IVX_TRY(f.begin());
    IVX_TRY(check_profile_args(f, p));
    if (n_q > IVX_DEPTH_MAX_QUANTILES) return ctx->fail(IVX_ERR_INVALID, "depth profile: more than 8 quantiles");
    if (n_q && !q_num) return ctx->fail(IVX_ERR_INVALID, "depth profile: null q_num");
    if (q_den == 0 || q_den > 65536u) return ctx->fail(IVX_ERR_INVALID, "depth profile: q_den outside 1 .. 65536");
    for (uint32_t j = 0; j < n_q; j++)
        if (q_num[j] > q_den) return ctx->fail(IVX_ERR_INVALID, "depth profile: a q_num above q_den");
    if (mem == IVX_MEM_DEVICE && ((((uintptr_t)out_len) & 7u) || ((((uintptr_t)out_min) | ((uintptr_t)out_max) | ((uintptr_t)out_q)) & 3u)))
        return ctx->fail(IVX_ERR_INVALID, "depth profile: output pointer not aligned to its element size");
    IVX_TRY(regions_begin(f, p, r));
    if (r.n == 0) return IVX_OK;
    const RegionSrc d = regions_stage(f, p, r);
    i64 *ol = f.out(out_len, r.n);
    i32 *omn = f.out(out_min, r.n), *omx = f.out(out_max, r.n), *oq = f.out(out_q, (u64)n_q * r.n);
    IVX_TRY(f.run([&] { return ivx_depth_region_ranks_device(ctx, p->dp, p->nkeys, d, q_num, n_q, q_den, ol, omn, omx, oq); }));
    f.rows_out(r.n);
    f.back_all();
    return f.finish();
}

}  // namespace

extern "C" ivx_status ivx_depth_profile_summarize(ivx_ctx *ctx, const ivx_index *p, int mem,
                                                  const uint32_t *qkey, const uint32_t *qstart, const uint32_t *qend, uint64_t n,
                                                  uint32_t pos_lo, const uint32_t *key_hi, int skip_pos0,
                                                  const int32_t *thresholds, uint32_t n_thr,
                                                  int64_t *out_len, int64_t *out_sum, int64_t *out_ge)
{
    return depth_summary(ctx, p, mem, region_table(qkey, qstart, qend, n, pos_lo, key_hi, skip_pos0), thresholds, n_thr, out_len, out_sum, out_ge);
}

extern "C" ivx_status ivx_depth_profile_windows(ivx_ctx *ctx, const ivx_index *p, int mem, uint32_t key,
                                                uint32_t first_pos, uint32_t last_pos, uint32_t width, uint64_t n, int skip_pos0,
                                                const int32_t *thresholds, uint32_t n_thr,
                                                int64_t *out_len, int64_t *out_sum, int64_t *out_ge)
{
    return depth_summary(ctx, p, mem, region_windows(key, first_pos, last_pos, width, n, skip_pos0), thresholds, n_thr, out_len, out_sum, out_ge);
}

extern "C" ivx_status ivx_depth_profile_quantiles(ivx_ctx *ctx, const ivx_index *p, int mem,
                                                  const uint32_t *qkey, const uint32_t *qstart, const uint32_t *qend, uint64_t n,
                                                  uint32_t pos_lo, const uint32_t *key_hi, int skip_pos0,
                                                  const uint32_t *q_num, uint32_t n_q, uint32_t q_den,
                                                  int64_t *out_len, int32_t *out_min, int32_t *out_max, int32_t *out_q)
{
    return depth_ranks(ctx, p, mem, region_table(qkey, qstart, qend, n, pos_lo, key_hi, skip_pos0), q_num, n_q, q_den, out_len, out_min, out_max, out_q);
}

extern "C" ivx_status ivx_depth_profile_window_quantiles(ivx_ctx *ctx, const ivx_index *p, int mem, uint32_t key,
                                                         uint32_t first_pos, uint32_t last_pos, uint32_t width, uint64_t n, int skip_pos0,
                                                         const uint32_t *q_num, uint32_t n_q, uint32_t q_den,
                                                         int64_t *out_len, int32_t *out_min, int32_t *out_max, int32_t *out_q)
{
    return depth_ranks(ctx, p, mem, region_windows(key, first_pos, last_pos, width, n, skip_pos0), q_num, n_q, q_den, out_len, out_min, out_max, out_q);
}

// ---- coverage classes of a profile: maximal runs of one class per key, and the per-key histogram of the per-base coverage
extern "C" ivx_status ivx_depth_profile_quantize(ivx_ctx *ctx, const ivx_index *p, int mem,
                                                 uint32_t pos_lo, const uint32_t *key_hi, int skip_pos0, int seen_only,
                                                 const int32_t *cuts, uint32_t n_cuts, uint32_t emit_mask,
                                                 uint32_t *out_key, uint32_t *out_start, uint32_t *out_end, uint32_t *out_class,
                                                 uint64_t cap, uint64_t *n_out)
{
    Frame f(ctx, mem);
    IVX_TRY(f.begin(n_out, "null n_out"));
    IVX_TRY(check_profile_args(f, p));
    if (n_cuts > IVX_DEPTH_MAX_CUTS) return ctx->fail(IVX_ERR_INVALID, "depth profile: more than 31 cuts");
    if (n_cuts && !cuts) return ctx->fail(IVX_ERR_INVALID, "depth profile: null cuts");
    for (uint32_t j = 1; j < n_cuts; j++)
        if (cuts[j] <= cuts[j - 1]) return ctx->fail(IVX_ERR_INVALID, "depth profile: cuts not strictly ascending");
    if (n_cuts < 31 && (emit_mask >> (n_cuts + 1))) return ctx->fail(IVX_ERR_INVALID, "depth profile: emit_mask names a class above n_cuts");
    if (mem == IVX_MEM_DEVICE && ((((uintptr_t)key_hi) | ((uintptr_t)out_key) | ((uintptr_t)out_start) | ((uintptr_t)out_end) | ((uintptr_t)out_class)) & 3u))
        return ctx->fail(IVX_ERR_INVALID, "depth profile: pointer not aligned to its element size");
    f.drop_plans();
    f.meter(false, p->dp.steps);
    const u32 *hi = f.in_at(WS_IN_KEYLEN, key_hi, p->nkeys);
    u32 *ok = f.out(out_key, cap), *os = f.out(out_start, cap), *oe = f.out(out_end, cap), *oc = f.out(out_class, cap);
    const bool sizing = cap == 0 && !out_key && !out_start && !out_end && !out_class;
    u64 m = 0;
    const ivx_status st = f.run([&] {
        return ivx_depth_quantize_device(ctx, p->dp, p->nkeys, pos_lo, hi, skip_pos0, seen_only, cuts, n_cuts, emit_mask, ok, os, oe, oc, cap, &m);
    });
    *n_out = m;
    if (st != IVX_OK) return st;
    if (!sizing) { f.rows_out(m); f.back_all(m); }
    return f.finish();
}

extern "C" ivx_status ivx_depth_profile_hist(ivx_ctx *ctx, const ivx_index *p, int mem,
                                             uint32_t pos_lo, const uint32_t *key_hi, int skip_pos0, int seen_only,
                                             int32_t v_lo, uint32_t n_bins, int64_t *out_hist)
{
    Frame f(ctx, mem);
    IVX_TRY(f.begin());
    IVX_TRY(check_profile_args(f, p));
    if (n_bins == 0 || n_bins > IVX_DEPTH_MAX_BINS) return ctx->fail(IVX_ERR_INVALID, "depth profile: n_bins outside 1 .. 65536");
    if (p->nkeys && !out_hist) return ctx->fail(IVX_ERR_INVALID, "depth profile: null out_hist");
    if (mem == IVX_MEM_DEVICE && ((((uintptr_t)key_hi) & 3u) || (((uintptr_t)out_hist) & 7u)))
        return ctx->fail(IVX_ERR_INVALID, "depth profile: pointer not aligned to its element size");
    f.drop_plans();
    f.meter(false, p->dp.steps);
    if (p->nkeys == 0) return IVX_OK;
    const u64 words = (u64)p->nkeys * n_bins;
    const u32 *hi = f.in_at(WS_IN_KEYLEN, key_hi, p->nkeys);
    i64 *oh = f.out(out_hist, words);
    IVX_TRY(f.run([&] { return ivx_depth_hist_device(ctx, p->dp, p->nkeys, pos_lo, hi, skip_pos0, seen_only, v_lo, n_bins, oh); }));
    f.rows_out(words);
    f.back_all();
    return f.finish();
}

// ---------------------------------------------------------------- f3: take / scatter of payload columns

extern "C" ivx_status ivx_take_fixed(ivx_ctx *ctx, int mem, const void *src, uint32_t width, uint64_t n_src,
                                     const uint8_t *src_valid_bits, const uint32_t *idx, uint64_t n, void *out, uint8_t *out_valid)
{
    Frame f(ctx, mem);
    IVX_TRY(f.enter());
    if (n && (!idx || !out)) return ctx->fail(IVX_ERR_INVALID, "take: null idx or out");
    if (n_src && !src) return ctx->fail(IVX_ERR_INVALID, "take: null source column");
    if (width == 0 || width > 32 || (width & (width - 1))) return ctx->fail(IVX_ERR_UNSUPPORTED, "take: fixed width must be 1, 2, 4, 8, 16 or 32 bytes");
    const u8 *dsrc = f.in((const u8 *)src, n_src * width), *dvalid = f.in(src_valid_bits, (n_src + 7) / 8);
    const u32 *didx = f.in(idx, n);
    u8 *dout = f.out((u8 *)out, n * width), *dov = f.out(out_valid, n);
    IVX_TRY(f.run([&] { return ivx_take_fixed_device(ctx, dsrc, width, n_src, dvalid, didx, n, dout, dov); }));
    f.back_all();
    return f.finish();
}

extern "C" ivx_status ivx_scatter_fixed(ivx_ctx *ctx, int mem, const void *src, uint32_t width, const uint32_t *idx, uint64_t n,
                                        void *out, uint64_t n_out)
{
    Frame f(ctx, mem);
    IVX_TRY(f.enter());
    if (n && (!idx || !src || !out)) return ctx->fail(IVX_ERR_INVALID, "scatter: null src, idx or out");
    if (width == 0 || width > 32 || (width & (width - 1))) return ctx->fail(IVX_ERR_UNSUPPORTED, "scatter: fixed width must be 1, 2, 4, 8, 16 or 32 bytes");
    const u8 *dsrc = f.in((const u8 *)src, n * width);
    const u32 *didx = f.in_at(WS_IN_END, idx, n);
    u8 *dout = f.out((u8 *)out, n_out * width);
    IVX_TRY(f.st);
    // host mode: rows that no index names keep what the caller's buffer holds
    if (mem == IVX_MEM_HOST && n_out) IVX_HIP(ctx, hipMemcpyAsync(dout, out, (size_t)n_out * width, hipMemcpyHostToDevice, ctx->stream));
    IVX_TRY(f.run([&] { return ivx_scatter_fixed_device(ctx, dsrc, width, didx, n, dout, n_out); }));
    f.back_all();
    return f.finish();
}

extern "C" ivx_status ivx_take_utf8(ivx_ctx *ctx, int mem, int large, const void *offsets, const uint8_t *data, uint64_t n_src,
                                    uint64_t src_data_bytes, const uint8_t *src_valid_bits, const uint32_t *idx, uint64_t n,
                                    void *out_offsets, uint8_t *out_data, uint64_t data_cap, uint64_t *data_bytes, uint8_t *out_valid)
{
    Frame f(ctx, mem);
    IVX_TRY(f.enter(data_bytes, "null data_bytes"));
    if (n && !idx) return ctx->fail(IVX_ERR_INVALID, "take: null idx");
    if (!offsets || (src_data_bytes && !data)) return ctx->fail(IVX_ERR_INVALID, "take: null source column");
    const size_t ow = large ? 8 : 4;
    const u8 *doff = f.in((const u8 *)offsets, (n_src + 1) * ow), *ddata = f.in(data, src_data_bytes), *dvalid = f.in(src_valid_bits, (n_src + 7) / 8);
    const u32 *didx = f.in(idx, n);
    u8 *dooff = f.out((u8 *)out_offsets, (n + 1) * ow), *dodata = f.out(out_data, data_cap), *dov = f.out(out_valid, n);
    u64 total = 0;
    const ivx_status st = f.run([&] { return ivx_take_utf8_device(ctx, large, doff, ddata, n_src, dvalid, didx, n, dooff, dodata, data_cap, &total, dov); });
    *data_bytes = total;
    // a short data buffer leaves the offsets and out_valid final (the device has written them): they go out as in device mode
    if (st != IVX_OK && st != IVX_ERR_CAPACITY) return st;
    f.back((u8 *)out_offsets);
    if (st == IVX_ERR_CAPACITY) f.withhold(out_data);
    else f.back(out_data, total);
    f.back(out_valid);
    const ivx_status fin = f.finish();
    return fin != IVX_OK ? fin : st;
}

extern "C" ivx_status ivx_take_bits(ivx_ctx *ctx, int mem, const uint8_t *src_bits, uint64_t n_src, const uint8_t *src_valid_bits,
                                    const uint32_t *idx, uint64_t n, uint8_t *out_bits, uint8_t *out_valid)
{
    Frame f(ctx, mem);
    IVX_TRY(f.enter());
    if (n && (!idx || !out_bits)) return ctx->fail(IVX_ERR_INVALID, "take: null idx or out");
    if (n_src && !src_bits) return ctx->fail(IVX_ERR_INVALID, "take: null source column");
    const u8 *dsrc = f.in(src_bits, (n_src + 7) / 8), *dvalid = f.in(src_valid_bits, (n_src + 7) / 8);
    const u32 *didx = f.in(idx, n);
    u8 *dout = f.out(out_bits, (n + 7) / 8), *dov = f.out(out_valid, n);
    IVX_TRY(f.run([&] { return ivx_take_bits_device(ctx, dsrc, n_src, dvalid, didx, n, dout, dov); }));
    f.back_all();
    return f.finish();
}

extern "C" ivx_status ivx_take_view(ivx_ctx *ctx, int mem, const void *views, const uint8_t *const *data_bufs, const uint64_t *data_buf_bytes,
                                    uint32_t n_bufs, uint64_t n_src, const uint8_t *src_valid_bits, const uint32_t *idx, uint64_t n,
                                    void *out_views, uint8_t *out_data, uint64_t data_cap, uint64_t *data_bytes, uint8_t *out_valid)
{
    Frame f(ctx, mem);
    IVX_TRY(f.enter(data_bytes, "null data_bytes"));
    if (n && !idx) return ctx->fail(IVX_ERR_INVALID, "take: null idx");
    if ((n_src && !views) || (n_bufs && (!data_bufs || !data_buf_bytes))) return ctx->fail(IVX_ERR_INVALID, "take: null source column");
    if (n_bufs > 4096) return ctx->fail(IVX_ERR_UNSUPPORTED, "take: more than 4096 view data buffers");
    const u8 *dviews = f.in((const u8 *)views, n_src * 16), *dvalid = f.in(src_valid_bits, (n_src + 7) / 8);
    const u32 *didx = f.in(idx, n);
    IVX_TRY(f.st);
    // the variadic data buffers: device pointers in one small device table (host mode: one staging area for all)
    std::vector<const u8 *> ptrs(n_bufs ? n_bufs : 1, nullptr);
    if (mem == IVX_MEM_HOST) {
        u64 tot = 0;
        for (u32 b = 0; b < n_bufs; b++) tot += (data_buf_bytes[b] + 15) & ~15ull;
        u8 *area;
        IVX_TRY(f.scratch_at(WS_IN2_START, tot ? tot : 16, (void **)&area));
        u64 at = 0;
        for (u32 b = 0; b < n_bufs; b++) {
            if (data_buf_bytes[b]) IVX_HIP(ctx, hipMemcpyAsync(area + at, data_bufs[b], data_buf_bytes[b], hipMemcpyHostToDevice, ctx->stream));
            ptrs[b] = area + at;
            at += (data_buf_bytes[b] + 15) & ~15ull;
        }
    } else {
        for (u32 b = 0; b < n_bufs; b++) ptrs[b] = data_bufs[b];
    }
    const u8 **dtable;
    IVX_TRY(f.scratch_at(WS_IN2_KEY, ptrs.size() * sizeof(u8 *), (void **)&dtable));
    IVX_HIP(ctx, hipMemcpyAsync(dtable, ptrs.data(), ptrs.size() * sizeof(u8 *), hipMemcpyHostToDevice, ctx->stream));
    IVX_HIP(ctx, hipStreamSynchronize(ctx->stream));                            // `ptrs` is pageable host memory
    u8 *doviews = f.out((u8 *)out_views, n * 16), *dodata = f.out(out_data, data_cap), *dov = f.out(out_valid, n);
    u64 total = 0;
    const ivx_status st = f.run([&] { return ivx_take_view_device(ctx, dviews, dtable, n_src, dvalid, didx, n, doviews, dodata, data_cap, &total, dov); });
    *data_bytes = total;
    if (st != IVX_OK) return st;
    // a sizing call that was given out_views: the views go out only with the data they point into
    if (out_data || total == 0) f.back((u8 *)out_views);
    else f.withhold((u8 *)out_views);
    f.back(out_data, total);
    f.back(out_valid);
    return f.finish();
}
