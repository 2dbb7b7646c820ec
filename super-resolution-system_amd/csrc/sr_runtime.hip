// sr_runtime.hip -- the library runtime every device source and sr_comm.cpp link against: the context's table uploads,
// stream sync, scratch and profiling events (declared in sr_ctx.h), the registry of live contexts, and the context, device
// memory and profiling part of the C ABI in include/sr_hip.h.  No kernel is defined here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "sr_ctx.h"

// ---------------------------------------------------------------------------------------------
// context (struct, Guard, ProfScope: sr_ctx.h)
// ---------------------------------------------------------------------------------------------
hipError_t upload_small(sr_ctx *c, void *d_dst, const void *h_src, size_t bytes)
{
    // bound what a caller that never synchronises can pile up: drain the stream once 32 MB of table copies are parked
    c->pending_bytes += bytes;
    if (c->pending_bytes > ((size_t)32 << 20)) {
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return e;
        c->pending_host.clear();
        c->pending_bytes = bytes;
    }
    c->pending_host.emplace_back((const char *)h_src, (const char *)h_src + bytes);
    return hipMemcpyAsync(d_dst, c->pending_host.back().data(), bytes, hipMemcpyHostToDevice, c->stream);
}

hipError_t upload_if_changed(sr_ctx *c, void *d_dst, const void *h_src, size_t bytes, std::vector<char> &shadow)
{
    if (shadow.size() == bytes && bytes > 0 && memcmp(shadow.data(), h_src, bytes) == 0) return hipSuccess;
    shadow.assign((const char *)h_src, (const char *)h_src + bytes);
    return upload_small(c, d_dst, h_src, bytes);
}

int upload_cached(sr_ctx *c, CachedTable &t, const void *h_src, size_t bytes)
{
    bool regrown = false;
    SRCHK(t.buf.reserve(c, "upload_cached", bytes, 0, 4096, &regrown));
    if (regrown) t.shadow.clear();
    HIPCHK(upload_if_changed(c, t.buf.d, h_src, bytes, t.shadow));
    return SR_OK;
}

int dev_alloc_error(const char *who, const char *what, size_t bytes, hipError_t e)
{
    return sr_set_error(e == hipErrorOutOfMemory ? SR_ERR_OOM : SR_ERR_HIP, "%s: %s of %zu bytes: %s", who, what, bytes,
                        hipGetErrorString(e));
}

int DevBuf::reserve(sr_ctx *c, const char *who, size_t bytes, size_t floor, size_t page, bool *regrown)
{
    if (bytes <= cap) return SR_OK;
    if (d) {
        HIPCHK(stream_sync(c));
        release();
    }
    const size_t nb = (std::max(bytes, floor) + page - 1) / page * page;
    const hipError_t e = hipMalloc(&d, nb);
    if (e != hipSuccess) {
        d = nullptr;
        return dev_alloc_error(who, "device buffer", nb, e);
    }
    cap = nb;
    if (regrown) *regrown = true;
    return SR_OK;
}

void DevBuf::release()
{
    if (d) (void)hipFree(d);
    d = nullptr;
    cap = 0;
}

DevTemp::~DevTemp()
{
    if (!d) return;
    (void)stream_sync(c);
    (void)hipFree(d);
}

int DevTemp::alloc(const char *who, size_t bytes)
{
    const hipError_t e = hipMalloc(&d, bytes);
    if (e == hipSuccess) return SR_OK;
    d = nullptr;
    return dev_alloc_error(who, "temporary", bytes, e);
}

hipError_t stream_sync(sr_ctx *c)
{
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) {
        c->pending_host.clear();
        c->pending_bytes = 0;
    }
    return e;
}

// Live-handle registry: destroying a context destroys its plans; destroying (or using) a handle that is
// no longer live is a harmless no-op / SR_ERR_INVALID_ARG instead of a use-after-free (host languages with
// garbage collectors finalise objects in arbitrary order at shutdown).
static std::mutex g_reg_mu;
static std::set<const void *> g_live_ctx;
bool ctx_is_live(const sr_ctx *c)
{
    std::lock_guard<std::mutex> lk(g_reg_mu);
    return c && g_live_ctx.count(c) != 0;
}

int ctx_scratch(sr_ctx *c, size_t bytes, void **out)
{
    SRCHK(c->scratch.reserve(c, "ctx_scratch", bytes, (size_t)1 << 20));
    *out = c->scratch.d;
    return SR_OK;
}

hipEvent_t prof_event(sr_ctx *c)
{
    if (!c->ev_pool.empty()) {
        hipEvent_t e = c->ev_pool.back();
        c->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return sr_set_error(SR_ERR_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
    return SR_OK;
}

extern "C" {

int sr_device_count(int *count)
{
    if (!count) return sr_set_error(SR_ERR_INVALID_ARG, "sr_device_count: null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return sr_set_error(SR_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return SR_OK;
}

static int ctx_create_impl(int device_id, void *stream, bool adopt, sr_ctx **out)
{
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_ctx_create: null out");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return sr_set_error(SR_ERR_HIP, "sr_ctx_create: no HIP device available (%s)",
                            e == hipSuccess ? "count is 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_ctx_create: device %d out of range (0..%d)", device_id, n - 1);
    int prev = 0;
    HIPCHK(hipGetDevice(&prev));
    HIPCHK(hipSetDevice(device_id));
    sr_ctx *c = new sr_ctx();
    c->device = device_id;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) c->num_cu = cus;
    }
    if (adopt) {
        c->stream = (hipStream_t)stream;
        c->own_stream = false;
    } else {
        hipError_t e2 = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e2 != hipSuccess) {
            delete c;
            (void)hipSetDevice(prev);
            return sr_set_error(SR_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e2));
        }
        c->own_stream = true;
    }
    (void)hipSetDevice(prev);
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        g_live_ctx.insert(c);
    }
    *out = c;
    return SR_OK;
}

int sr_ctx_create(int device_id, sr_ctx **out) { return ctx_create_impl(device_id, nullptr, false, out); }

int sr_ctx_create_on_stream(int device_id, void *hip_stream, sr_ctx **out)
{
    return ctx_create_impl(device_id, hip_stream, true, out);
}

int sr_ctx_destroy(sr_ctx *ctx)
{
    if (!ctx_is_live(ctx)) return SR_OK;
    destroy_plans_of(ctx);
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        g_live_ctx.erase(ctx);
    }
    {
        Guard g(ctx);
        (void)hipStreamSynchronize(ctx->stream);
        for (auto &p : ctx->prof_pairs) {
            (void)hipEventDestroy(p.a);
            (void)hipEventDestroy(p.b);
        }
        for (auto e : ctx->ev_pool) (void)hipEventDestroy(e);
        ctx->release_device();
        if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    }
    delete ctx;
    return SR_OK;
}

int sr_ctx_sync(sr_ctx *ctx)
{
    CTX_ENTER(ctx);
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_ctx_num_cu(sr_ctx *ctx, int *num_cu)
{
    CTX_ENTER(ctx);
    if (!num_cu) return sr_set_error(SR_ERR_INVALID_ARG, "sr_ctx_num_cu: null out");
    *num_cu = ctx->num_cu;
    return SR_OK;
}

int sr_dev_alloc(sr_ctx *ctx, size_t bytes, void **d_ptr)
{
    CTX_ENTER(ctx);
    if (!d_ptr) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dev_alloc: null out");
    *d_ptr = nullptr;
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(d_ptr, bytes);
    if (e != hipSuccess) return dev_alloc_error("sr_dev_alloc", "device memory", bytes, e);
    return SR_OK;
}

int sr_dev_free(sr_ctx *ctx, void *d_ptr)
{
    CTX_ENTER(ctx);
    if (!d_ptr) return SR_OK;
    HIPCHK(stream_sync(ctx));
    HIPCHK(hipFree(d_ptr));
    return SR_OK;
}

int sr_memcpy_h2d(sr_ctx *ctx, void *d_dst, const void *h_src, size_t bytes)
{
    CTX_ENTER(ctx);
    if (bytes == 0) return SR_OK;
    HIPCHK(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_memcpy_d2h(sr_ctx *ctx, void *h_dst, const void *d_src, size_t bytes)
{
    CTX_ENTER(ctx);
    if (bytes == 0) return SR_OK;
    HIPCHK(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_memcpy_d2d(sr_ctx *ctx, void *d_dst, const void *d_src, size_t bytes)
{
    CTX_ENTER(ctx);
    if (bytes == 0) return SR_OK;
    HIPCHK(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return SR_OK;
}

int sr_memset_d(sr_ctx *ctx, void *d_dst, int value, size_t bytes)
{
    CTX_ENTER(ctx);
    if (bytes == 0) return SR_OK;
    HIPCHK(hipMemsetAsync(d_dst, value, bytes, ctx->stream));
    return SR_OK;
}

int sr_prof_enable(sr_ctx *ctx, int on)
{
    CTX_ENTER(ctx);
    ctx->prof = on != 0;
    return SR_OK;
}

int sr_prof_select(sr_ctx *ctx, const char *name)
{
    CTX_ENTER(ctx);
    ctx->prof_only = name ? name : "";
    return SR_OK;
}

int sr_prof_reset(sr_ctx *ctx)
{
    CTX_ENTER(ctx);
    HIPCHK(stream_sync(ctx));
    for (auto &p : ctx->prof_pairs) {
        ctx->ev_pool.push_back(p.a);
        ctx->ev_pool.push_back(p.b);
    }
    ctx->prof_pairs.clear();
    return SR_OK;
}

int sr_prof_get(sr_ctx *ctx, sr_prof_record *h_records, int cap, int *n)
{
    CTX_ENTER(ctx);
    if (!n) return sr_set_error(SR_ERR_INVALID_ARG, "sr_prof_get: null n");
    HIPCHK(stream_sync(ctx));
    std::vector<double> ms(ctx->prof_names.size(), 0.0);
    std::vector<int64_t> cnt(ctx->prof_names.size(), 0);
    for (auto &p : ctx->prof_pairs) {
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, p.a, p.b));
        ms[p.name_id] += t;
        cnt[p.name_id] += 1;
    }
    int k = 0;
    for (size_t i = 0; i < ctx->prof_names.size(); ++i) {
        if (cnt[i] == 0) continue;
        if (h_records && k < cap) {
            memset(&h_records[k], 0, sizeof(sr_prof_record));
            strncpy(h_records[k].name, ctx->prof_names[i].c_str(), sizeof(h_records[k].name) - 1);
            h_records[k].ms = ms[i];
            h_records[k].launches = cnt[i];
        }
        ++k;
    }
    *n = k;
    return SR_OK;
}

}  // extern "C"
