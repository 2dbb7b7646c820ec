// sr_ctx.h -- the device context shared by the .hip translation units of libsrhip.so (sr_runtime.hip owns the
// definitions, except plan_describe and destroy_plans_of: sr_engine.hip, and reduce_partials: sr_assess.hip; every
// other .hip file and sr_comm.cpp use them, the convolution networks through sr_conv_mfma.h, the SSIM column march through
// sr_ssim11.h).  Device memory is owned here: DevBuf (grow-only, released by its owner) and DevTemp (one call).
// Internal: nothing here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "sr_internal.h"

#define SRCHK(expr)                                                                                \
    do {                                                                                           \
        const int rc_ = (expr);                                                                    \
        if (rc_ != SR_OK) return rc_;                                                              \
    } while (0)

#define HIPCHK(expr)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return sr_set_error(SR_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                                __LINE__);                                                         \
    } while (0)

struct sr_ctx;

// The error of a failed device allocation: SR_ERR_OOM when the device is out of memory, SR_ERR_HIP otherwise.
int dev_alloc_error(const char *who, const char *what, size_t bytes, hipError_t e);

// An owned device buffer that only grows.  It has no destructor: its owner calls release() with the stream drained and the
// buffer's device current (sr_ctx_destroy and the model destroys do, under their Guard).
struct DevBuf {
    void *d = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : d(o.d), cap(o.cap) { o.d = nullptr; o.cap = 0; }
    // bytes <= cap: nothing.  Otherwise the stream is drained, the old buffer freed (its contents are lost) and
    // max(bytes, floor) rounded up to a multiple of page allocated; *regrown tells.  On failure d == nullptr, cap == 0.
    int reserve(sr_ctx *c, const char *who, size_t bytes, size_t floor = 0, size_t page = 1, bool *regrown = nullptr);
    void release();
    template <class T>
    T *as(size_t byte_off = 0) const { return (T *)((char *)d + byte_off); }
};

// A device temporary of one call.  Declared after CTX_ENTER, so it goes before the Guard does: every return path drains the
// context's stream and frees it, with the context's device current.
struct DevTemp {
    sr_ctx *c;
    void *d = nullptr;
    explicit DevTemp(sr_ctx *ctx) : c(ctx) {}
    DevTemp(const DevTemp &) = delete;
    DevTemp &operator=(const DevTemp &) = delete;
    DevTemp(DevTemp &&o) noexcept : c(o.c), d(o.d) { o.d = nullptr; }
    ~DevTemp();
    int alloc(const char *who, size_t bytes);
    template <class T>
    T *as(size_t byte_off = 0) const { return (T *)((char *)d + byte_off); }
};

struct ProfPair {
    int name_id;
    hipEvent_t a, b;
};

// A small device table with a host shadow of what was last uploaded into it: per-step descriptor tables (tile
// pointers, strides, rectangles) rarely change between calls, and a host->device copy between two kernels costs a
// stream bubble of several microseconds -- identical content is not uploaded again.
struct CachedTable {
    DevBuf buf;
    std::vector<char> shadow;
};

struct sr_ctx {
    int device = 0;
    int num_cu = 256;               // compute units of the device (launch-shape heuristics)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::recursive_mutex mu;
    bool prof = false;
    std::string prof_only;          // when not empty: the one kernel family that is timed
    std::vector<std::string> prof_names;
    std::vector<ProfPair> prof_pairs;
    std::vector<hipEvent_t> ev_pool;
    // small reusable device scratch (resize tables, reduction partials, result words)
    DevBuf scratch;
    // host copies of small tables handed to hipMemcpyAsync; released at the next stream sync
    std::vector<std::vector<char>> pending_host;
    size_t pending_bytes = 0;
    CachedTable extract_tab;                            // tile-extract descriptors
    CachedTable resize_tab;                             // cubic tables of the resized assessment
    CachedTable cubic_tab;                              // cubic tables of sr_resize_cubic_u8
    DevBuf gray_planes;                                 // resized gray planes + SSE partials of the resized assessment
    DevBuf cm_ws;                                       // commercial / no-reference metrics: planes, FFT buffers, partials
    DevBuf msssim_ws;                                   // MS-SSIM: level planes (x | y << 16 sums), partials, per-level results
    int msssim_h = 0, msssim_w = 0, msssim_levels = 0;  // what the planes hold (levels == 0: nothing valid)
    DevBuf bench_ws;                                    // SR-benchmark PSNR / SSIM: per-block partials
    DevBuf niqe_ws;                                     // NIQE: the int32 half plane, then the block records
    int niqe_H = 0, niqe_W = 0;                         // the kept plane whose half plane the scratch holds (0: nothing valid)
    DevBuf brisque_ws;                                  // BRISQUE: the int32 half plane, then the per-tile partials
    int brisque_H2 = 0, brisque_W2 = 0;                 // the half plane the scratch holds (0: nothing valid)
    DevBuf vif_ws;                                      // VIF: the float64 planes of scales 2 .. 4, then the per-block partials
    DevBuf gmsd_ws;                                     // GMSD: per-block partials
    DevBuf fsim_ws;                                     // FSIM: pooled sums, filters, twiddles, transform planes, partials
    int fsim_rows = 0, fsim_cols = 0;                   // the pooled size whose filters and twiddles the scratch holds (0: none)
    double fsim_consts[12] = {0};                       // ... and EM_n, S2, Sij of its four orientations
    DevBuf vsi_ws;                                      // VSI: pooled sums, LG / SD / twiddles, the axis tables, the SDSP planes, partials
    int vsi_h = 0, vsi_w = 0;                           // the image size whose tables the scratch holds (0: none)
    DevBuf deltae_ws;                                   // colour difference: the linearisation table, histogram, partials, cell slabs
    bool deltae_table = false;                          // the table is in place (false again whenever the buffer is regrown)
    DevBuf haarpsi_ws;                                  // HaarPSI: per-block partials; the per-cell form adds the sample map, edges, records
    DevBuf mser_ws;                                     // MSER: gray plane, sorted pixels, union-find, node table (sr_mser.h)
    std::vector<sr_mser_region> mser_last;              // the sorted records of the last sr_mser_u8 (sr_mser_last_regions)
    DevBuf cascade_ws;                                  // cascade: gray plane, scaled planes, summed-area tables, model, lists (sr_cascade.h)
    std::vector<sr_tile_rect> cascade_last;             // the candidates of the last sr_cascade_u8 (sr_cascade_last_candidates)
    CachedTable imresize_tab;                           // imresize: both axes' weights, indices and starts of the last geometry
    // Frees every device buffer above; sr_ctx_destroy calls it with the stream drained and the device current.
    void release_device()
    {
        for (DevBuf *b : {&scratch, &extract_tab.buf, &resize_tab.buf, &cubic_tab.buf, &gray_planes, &cm_ws, &msssim_ws, &bench_ws, &niqe_ws, &brisque_ws, &vif_ws, &gmsd_ws, &fsim_ws, &vsi_ws, &deltae_ws, &haarpsi_ws, &mser_ws, &cascade_ws, &imresize_tab.buf})
            b->release();
    }
};

// Enqueue a small host->device table upload whose source stays alive until the next sync.
hipError_t upload_small(sr_ctx *c, void *d_dst, const void *h_src, size_t bytes);
hipError_t stream_sync(sr_ctx *c);
// Upload into a fixed destination unless `shadow` shows the same bytes are already there.
hipError_t upload_if_changed(sr_ctx *c, void *d_dst, const void *h_src, size_t bytes, std::vector<char> &shadow);
// Same with a table that owns (and grows, in 4 KiB pages) its device buffer; an SR_* code.
int upload_cached(sr_ctx *c, CachedTable &t, const void *h_src, size_t bytes);
bool ctx_is_live(const sr_ctx *c);
// What a blend plan was made for (sr_comm.cpp cross-checks the arguments of the sharded blend); false when the plan is
// null or destroyed.
struct sr_blend_plan;
bool plan_describe(const sr_blend_plan *p, sr_ctx **ctx, int *n, int *cn);
// Destroys every live plan of the context (sr_engine.hip, which alone knows a plan's context; for sr_ctx_destroy).
void destroy_plans_of(sr_ctx *ctx);
int ctx_scratch(sr_ctx *c, size_t bytes, void **out);
hipEvent_t prof_event(sr_ctx *c);
int check_launch(const char *what);
// Deterministic tree sum of part[n][ncomp] -> pointer (inside the two ping-pong buffers) to the ncomp results
// (sr_assess.hip, beside k_reduce_partials).
const double *reduce_partials(sr_ctx *ctx, const double *part, long long n, int ncomp, double *buf0, double *buf1);

struct Guard {
    sr_ctx *c;
    int prev = -1;
    bool ok = true;
    explicit Guard(sr_ctx *ctx) : c(ctx)
    {
        c->mu.lock();
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != c->device && hipSetDevice(c->device) != hipSuccess) ok = false;
    }
    ~Guard()
    {
        if (prev >= 0 && prev != c->device) (void)hipSetDevice(prev);
        c->mu.unlock();
    }
};

// fn: the name the two messages carry (a frame shared by several entry points passes its caller's).
#define CTX_ENTER_AS(ctx, fn)                                                        \
    if (!ctx_is_live(ctx)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed context", fn); \
    Guard guard_(ctx);                                                               \
    if (!guard_.ok) return sr_set_error(SR_ERR_HIP, "%s: hipSetDevice(%d) failed", fn, (ctx)->device)
#define CTX_ENTER(ctx) CTX_ENTER_AS(ctx, __func__)

struct ProfScope {
    sr_ctx *c;
    ProfPair p{};
    bool on;
    ProfScope(sr_ctx *ctx, const char *name) : c(ctx), on(ctx->prof)
    {
        if (on && !c->prof_only.empty() && c->prof_only != name) on = false;
        if (!on) return;
        int id = -1;
        for (size_t i = 0; i < c->prof_names.size(); ++i)
            if (c->prof_names[i] == name) id = (int)i;
        if (id < 0) {
            c->prof_names.push_back(name);
            id = (int)c->prof_names.size() - 1;
        }
        p.name_id = id;
        p.a = prof_event(c);
        p.b = prof_event(c);
        (void)hipEventRecord(p.a, c->stream);
    }
    ~ProfScope()
    {
        if (!on) return;
        (void)hipEventRecord(p.b, c->stream);
        c->prof_pairs.push_back(p);
    }
};
