// sr_cascade.hip -- Viola-Jones cascade detection (ContentAnalyzer.detect_faces; cv2.CascadeClassifier.detectMultiScale) on
// gfx950; the definition is in include/sr_hip.h ("Cascade"), the evaluation of one window in sr_cascade.h (the text the host
// restatement compiles too).  Everything the kernels produce is an integer: equal inputs give equal candidates whatever
// order the hardware takes; the one unordered thing, the append position of a detection, is removed by the host's sort.
//
// The pyramid is ONE flattened index space per kernel, not a launch per scale: a per-scale table (CcScale, at most 128
// entries, copied into LDS by every block) holds the prefix offsets of the planes' pixels, the tables' rows and columns and
// the window positions; a thread finds its scale by binary search.  Six launches whatever the number of scales:
//   k_cc_gray     the gray plane (the content section's rule)
//   k_cc_planes   every scaled plane, one thread per output sample (exact-integer bilinear, int64)
//   k_cc_rows     per plane row the running sums into row y + 1 of its (sw + 1) x (sh + 1) table (and of the squares for
//                 HAAR): one wave per row, 64 samples per step scanned by shuffles; column 0 of the table is written 0
//   k_cc_cols     per table column the running sum down the rows, one thread per column (adjacent threads, adjacent
//                 words); row 0 is written 0.  Tables are unsigned 32-bit and wrap: a box sum is taken by unsigned
//                 differences and every box sum (and sum of squares: sides <= 255) fits, so the wrap cancels
//   k_cc_dense    one thread per window position: the model's leading stages (at most 64 stumps, held in LDS) on every
//                 window; the survivors' position indices are compacted into a list (one atomic add per wave: ballot,
//                 popcount, lane rank).  A model that ends inside the dense stages appends its detections directly
//   k_cc_tail     the remaining stages over the compacted list, stumps from global memory (every active lane of a wave is
//                 at the same stump: uniform loads); detections are appended to the candidate list the same way
//   (host)        the two counters and the candidate list come down; position indices sort into canonical order (scale, y,
//                 x) as plain integers; sr_cascade_host.cpp turns them into rectangles
// k_cc_map (inspection) evaluates every stage on every position of the scale-0 plane and stores the count passed.
//
// Visibility rests on kernel boundaries alone: every kernel reads what an earlier kernel finished writing; the counters are
// changed by device-scope atomics and read by the next kernel or the host.
#include <algorithm>
#include <vector>

#include "sr_cascade.h"
#include "sr_ctx.h"

namespace {

#define CC_THREADS 256

template <int CcScale::*OFF>
__device__ __forceinline__ int cc_find(const CcScale *sc, int ns, int idx)
{
    int lo = 0, hi = ns - 1;                 // the last scale whose offset is <= idx
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sc[mid].*OFF <= idx) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void cc_load_scales(CcScale *sc, const CcScale *__restrict__ g_sc, int ns)
{
    const int *src = (const int *)g_sc;
    int *dst = (int *)sc;
    for (int i = threadIdx.x; i < ns * (int)(sizeof(CcScale) / 4); i += CC_THREADS) dst[i] = src[i];
    __syncthreads();
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_gray(const unsigned char *__restrict__ img, long long stride, int cn, int H, int W,
                                                        unsigned char *__restrict__ g)
{
    const int p = blockIdx.x * CC_THREADS + threadIdx.x;
    if (p >= H * W) return;
    const int y = p / W, x = p - y * W;
    const unsigned char *px = img + (long long)y * stride + (long long)x * cn;
    g[p] = (unsigned char)(cn == 1 ? px[0] : (px[0] * 3735 + px[1] * 19235 + px[2] * 9798 + (1 << 14)) >> 15);
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_planes(const unsigned char *__restrict__ g, int H, int W,
                                                          const CcScale *__restrict__ g_sc, int ns, int total,
                                                          unsigned char *__restrict__ planes)
{
    __shared__ CcScale sc[SR_CASCADE_MAX_SCALES];
    cc_load_scales(sc, g_sc, ns);
    const int idx = blockIdx.x * CC_THREADS + threadIdx.x;
    if (idx >= total) return;
    const CcScale s = sc[cc_find<&CcScale::pix_off>(sc, ns, idx)];
    const int q = idx - s.pix_off, y = q / s.sw, x = q - y * s.sw;
    planes[idx] = (unsigned char)cc_resample(g, W, H, s.sw, s.sh, x, y);
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_rows(const unsigned char *__restrict__ planes, const CcScale *__restrict__ g_sc,
                                                        int ns, int rows, int squares, unsigned *__restrict__ T,
                                                        unsigned *__restrict__ S)
{
    __shared__ CcScale sc[SR_CASCADE_MAX_SCALES];
    cc_load_scales(sc, g_sc, ns);
    const int lane = threadIdx.x & 63, r = blockIdx.x * (CC_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;                   // a whole wave leaves together
    const CcScale s = sc[cc_find<&CcScale::row_off>(sc, ns, r)];
    const int y = r - s.row_off, pitch = s.sw + 1;
    const unsigned char *row = planes + s.pix_off + y * s.sw;
    unsigned *t = T + s.tab_off + (y + 1) * pitch, *sq = S + s.tab_off + (y + 1) * pitch;
    if (lane == 0) {
        t[0] = 0u;
        if (squares) sq[0] = 0u;
    }
    unsigned carry = 0u, carry2 = 0u;
    for (int base = 0; base < s.sw; base += 64) {
        const int x = base + lane;
        const unsigned v = x < s.sw ? row[x] : 0u;
        unsigned a = v, b = v * v;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned ua = __shfl_up(a, o), ub = __shfl_up(b, o);
            if (lane >= o) {
                a += ua;
                b += ub;
            }
        }
        if (x < s.sw) {
            t[x + 1] = carry + a;
            if (squares) sq[x + 1] = carry2 + b;
        }
        carry += __shfl(a, 63);
        carry2 += __shfl(b, 63);
    }
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_cols(const CcScale *__restrict__ g_sc, int ns, int cols, int squares,
                                                        unsigned *__restrict__ T, unsigned *__restrict__ S)
{
    __shared__ CcScale sc[SR_CASCADE_MAX_SCALES];
    cc_load_scales(sc, g_sc, ns);
    const int c = blockIdx.x * CC_THREADS + threadIdx.x;
    if (c >= cols) return;
    const CcScale s = sc[cc_find<&CcScale::col_off>(sc, ns, c)];
    const int x = c - s.col_off, pitch = s.sw + 1;
    unsigned *t = T + s.tab_off + x;
    unsigned acc = 0u;
    t[0] = 0u;
    for (int y = 1; y <= s.sh; ++y) {
        acc += t[y * pitch];
        t[y * pitch] = acc;
    }
    if (squares) {
        unsigned *q = S + s.tab_off + x;
        acc = 0u;
        q[0] = 0u;
        for (int y = 1; y <= s.sh; ++y) {
            acc += q[y * pitch];
            q[y * pitch] = acc;
        }
    }
}

// Every lane of the wave calls this; the keepers take consecutive slots behind one atomic add.
__device__ __forceinline__ void cc_append(bool keep, unsigned v, unsigned *ctr, unsigned *__restrict__ list, unsigned cap)
{
    const unsigned long long m = __ballot(keep);
    if (!m) return;
    const int lane = threadIdx.x & 63, lead = __ffsll((long long)m) - 1;
    unsigned slot = 0u;
    if (lane == lead) slot = atomicAdd(ctr, (unsigned)__popcll(m));
    slot = __shfl(slot, lead) + (unsigned)__popcll(m & ((1ULL << lane) - 1ULL));
    if (keep && slot < cap) list[slot] = v;
}

struct CcModelArgs {
    const CcStage *stages;
    const unsigned *stumps;
    int type, W0, H0, n_stages, dense_stages, dense_stumps;
};

__global__ __launch_bounds__(CC_THREADS) void k_cc_dense(CcModelArgs md, const CcScale *__restrict__ g_sc, int ns, int positions,
                                                         const unsigned *__restrict__ T, const unsigned *__restrict__ S,
                                                         unsigned *ctr, unsigned *__restrict__ surv, unsigned *__restrict__ cand)
{
    __shared__ CcScale sc[SR_CASCADE_MAX_SCALES];
    __shared__ CcStage sg[CC_DENSE_STAGES];
    __shared__ unsigned sst[CC_DENSE_STUMPS * CC_STUMP_WORDS];
    for (int i = threadIdx.x; i < md.dense_stages * 4; i += CC_THREADS) ((int *)sg)[i] = ((const int *)md.stages)[i];
    for (int i = threadIdx.x; i < md.dense_stumps * CC_STUMP_WORDS; i += CC_THREADS) sst[i] = md.stumps[i];
    cc_load_scales(sc, g_sc, ns);
    const int idx = blockIdx.x * CC_THREADS + threadIdx.x;
    bool keep = false;
    if (idx < positions) {
        const CcScale s = sc[cc_find<&CcScale::pos_off>(sc, ns, idx)];
        const int q = idx - s.pos_off, iy = q / s.nx, ix = q - iy * s.nx;
        keep = cc_run(sg, sst, 0, 0, md.dense_stages, md.type, T + s.tab_off, S + s.tab_off, s.sw + 1, ix * s.step, iy * s.step,
                      md.W0, md.H0) == md.dense_stages;
    }
    const bool done = md.dense_stages == md.n_stages;
    cc_append(keep, (unsigned)idx, done ? ctr + 1 : ctr, done ? cand : surv, (unsigned)positions);
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_tail(CcModelArgs md, const CcScale *__restrict__ g_sc, int ns, int positions,
                                                        const unsigned *__restrict__ T, const unsigned *__restrict__ S,
                                                        unsigned *ctr, const unsigned *__restrict__ surv,
                                                        unsigned *__restrict__ cand)
{
    __shared__ CcScale sc[SR_CASCADE_MAX_SCALES];
    cc_load_scales(sc, g_sc, ns);
    const int n = (int)min(ctr[0], (unsigned)positions);
    for (int base = blockIdx.x * CC_THREADS; base < n; base += gridDim.x * CC_THREADS) {
        const int i = base + threadIdx.x;
        bool keep = false;
        unsigned idx = 0u;
        if (i < n) {
            idx = surv[i];
            if (idx < (unsigned)positions) {
                const CcScale s = sc[cc_find<&CcScale::pos_off>(sc, ns, (int)idx)];
                const int q = (int)idx - s.pos_off, iy = q / s.nx, ix = q - iy * s.nx;
                keep = cc_run(md.stages, md.stumps, 0, md.dense_stages, md.n_stages, md.type, T + s.tab_off, S + s.tab_off, s.sw + 1,
                              ix * s.step, iy * s.step, md.W0, md.H0) == md.n_stages - md.dense_stages;
            }
        }
        cc_append(keep, idx, ctr + 1, cand, (unsigned)positions);
    }
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_map(CcModelArgs md, CcScale s, const unsigned *__restrict__ T,
                                                      const unsigned *__restrict__ S, int *__restrict__ map)
{
    const int q = blockIdx.x * CC_THREADS + threadIdx.x;
    if (q >= s.nx * s.ny) return;
    const int iy = q / s.nx, ix = q - iy * s.nx;
    map[q] = cc_run(md.stages, md.stumps, 0, 0, md.n_stages, md.type, T + s.tab_off, S + s.tab_off, s.sw + 1, ix * s.step, iy * s.step,
                    md.W0, md.H0);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
unsigned cc_grid(long long n) { return (unsigned)std::max(1LL, (n + CC_THREADS - 1) / CC_THREADS); }

bool bad_image(const void *d_img, int64_t stride, int h, int w, int cn)
{
    return !d_img || h < 1 || w < 1 || (cn != 1 && cn != 3 && cn != 4) || stride < (int64_t)w * cn;
}

struct CcView {
    unsigned char *g, *planes;
    unsigned *T, *S, *ctr, *surv, *cand;
    CcScale *scales;
    CcModelArgs md;
};

// Gray plane, scaled planes and tables of a plan with at least one scale into the workspace; the model and the scale table
// go up with them and the counters are cleared.
int build_pyramid(sr_ctx *ctx, const char *who, const sr_cascade *m, const uint8_t *d_img, int64_t stride, int h, int w, int cn,
                  const CcPlan &pl, CcView *view)
{
    SRCHK(ctx->cascade_ws.reserve(ctx, who, pl.total));
    char *ws = ctx->cascade_ws.as<char>();
    CcView v;
    v.g = (unsigned char *)(ws + pl.off_gray);
    v.planes = (unsigned char *)(ws + pl.off_planes);
    v.T = (unsigned *)(ws + pl.off_tab);
    const bool haar = m->info.feature_type == SR_CASCADE_HAAR;
    v.S = haar ? (unsigned *)(ws + pl.off_sq) : v.T;       // LBP never reads it
    v.ctr = (unsigned *)(ws + pl.off_ctr);
    v.surv = (unsigned *)(ws + pl.off_surv);
    v.cand = (unsigned *)(ws + pl.off_cand);
    v.scales = (CcScale *)(ws + pl.off_scales);
    v.md = {(const CcStage *)(ws + pl.off_stages), (const unsigned *)(ws + pl.off_stumps), m->info.feature_type, m->info.win_w,
            m->info.win_h, m->info.n_stages, m->dense_stages, m->dense_stumps};
    *view = v;
    const int ns = (int)pl.dev.size();
    const dim3 block(CC_THREADS);
    // one profiling scope per launch: the launches of a call are counted, not read off this text (tools/cascade_timing.py)
    {
        ProfScope ps(ctx, "cc_gray");                      // with the counters' memset and the three small uploads
        HIPCHK(hipMemsetAsync(v.ctr, 0, 256, ctx->stream));
        if (!m->stumps.empty()) HIPCHK(upload_small(ctx, ws + pl.off_stumps, m->stumps.data(), m->stumps.size() * 4));
        HIPCHK(upload_small(ctx, ws + pl.off_stages, m->stages.data(), m->stages.size() * sizeof(CcStage)));
        HIPCHK(upload_small(ctx, v.scales, pl.dev.data(), (size_t)ns * sizeof(CcScale)));
        hipLaunchKernelGGL(k_cc_gray, dim3(cc_grid(pl.npx)), block, 0, ctx->stream, d_img, (long long)stride, cn, h, w, v.g);
    }
    {
        ProfScope ps(ctx, "cc_planes");
        hipLaunchKernelGGL(k_cc_planes, dim3(cc_grid(pl.plane_px)), block, 0, ctx->stream, (const unsigned char *)v.g, h, w,
                           (const CcScale *)v.scales, ns, (int)pl.plane_px, v.planes);
    }
    {
        ProfScope ps(ctx, "cc_rows");
        hipLaunchKernelGGL(k_cc_rows, dim3((unsigned)((pl.rows + CC_THREADS / 64 - 1) / (CC_THREADS / 64))), block, 0, ctx->stream,
                           (const unsigned char *)v.planes, (const CcScale *)v.scales, ns, (int)pl.rows, haar ? 1 : 0, v.T, v.S);
    }
    {
        ProfScope ps(ctx, "cc_cols");
        hipLaunchKernelGGL(k_cc_cols, dim3(cc_grid(pl.cols)), block, 0, ctx->stream, (const CcScale *)v.scales, ns, (int)pl.cols,
                           haar ? 1 : 0, v.T, v.S);
    }
    return check_launch(who);
}

}  // namespace

int sr_cascade_u8(sr_ctx *ctx, const sr_cascade *model, const uint8_t *d_img, int64_t stride, int h, int w, int cn,
                  const sr_cascade_params *params, sr_tile_rect *h_cands, int64_t cap, int64_t *count)
{
    CTX_ENTER(ctx);
    ctx->cascade_last.clear();
    if (bad_image(d_img, stride, h, w, cn) || !count || cap < 0 || (cap > 0 && !h_cands))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_u8: bad arguments");
    CcPlan pl;
    SRCHK(cascade_plan("sr_cascade_u8", model, h, w, params, &pl));
    *count = 0;
    if (pl.scales.empty()) return SR_OK;                   // the image is smaller than the window: nothing is launched
    CcView v;
    SRCHK(build_pyramid(ctx, "sr_cascade_u8", model, d_img, stride, h, w, cn, pl, &v));
    const int ns = (int)pl.dev.size(), positions = (int)pl.positions;
    {
        ProfScope ps(ctx, "cc_dense");
        hipLaunchKernelGGL(k_cc_dense, dim3(cc_grid(positions)), dim3(CC_THREADS), 0, ctx->stream, v.md, (const CcScale *)v.scales, ns,
                           positions, (const unsigned *)v.T, (const unsigned *)v.S, v.ctr, v.surv, v.cand);
    }
    if (model->dense_stages < model->info.n_stages) {
        ProfScope ps(ctx, "cc_tail");
        const unsigned grid = std::min(cc_grid(positions), (unsigned)std::max(ctx->num_cu, 1) * 8u);
        hipLaunchKernelGGL(k_cc_tail, dim3(grid), dim3(CC_THREADS), 0, ctx->stream, v.md, (const CcScale *)v.scales, ns, positions,
                           (const unsigned *)v.T, (const unsigned *)v.S, v.ctr, (const unsigned *)v.surv, v.cand);
    }
    SRCHK(check_launch("sr_cascade_u8"));
    unsigned ctr[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(ctr, v.ctr, sizeof(ctr), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    if (ctr[0] > (unsigned)positions || ctr[1] > (unsigned)positions)
        return sr_set_error(SR_ERR_HIP, "sr_cascade_u8: list overflow (%u survivors, %u detections, %d positions)", ctr[0], ctr[1], positions);
    std::vector<uint32_t> pos(ctr[1]);
    if (ctr[1]) {
        HIPCHK(hipMemcpyAsync(pos.data(), v.cand, (size_t)ctr[1] * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(stream_sync(ctx));
    }
    std::sort(pos.begin(), pos.end());
    for (uint32_t p : pos)
        if (p >= (uint32_t)positions) return sr_set_error(SR_ERR_HIP, "sr_cascade_u8: a detection lies outside the position list");
    std::vector<sr_tile_rect> all(pos.size());
    cascade_candidates(pl, pos.data(), pos.size(), all.data());
    *count = (int64_t)all.size();
    const size_t n = std::min<size_t>(all.size(), (size_t)cap);
    if (n) std::copy(all.begin(), all.begin() + n, h_cands);
    ctx->cascade_last.swap(all);
    return SR_OK;
}

int sr_cascade_last_candidates(sr_ctx *ctx, sr_tile_rect *h_cands, int64_t cap, int64_t *count)
{
    CTX_ENTER(ctx);
    if (!count || cap < 0 || (cap > 0 && !h_cands)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_last_candidates: bad arguments");
    *count = (int64_t)ctx->cascade_last.size();
    const size_t n = std::min<size_t>(ctx->cascade_last.size(), (size_t)cap);
    if (n) std::copy(ctx->cascade_last.begin(), ctx->cascade_last.begin() + n, h_cands);
    return SR_OK;
}

int sr_cascade_workspace(sr_ctx *ctx, void **d_ptr, size_t *bytes)
{
    CTX_ENTER(ctx);
    if (!d_ptr || !bytes) return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_workspace: null output");
    *d_ptr = ctx->cascade_ws.d;
    *bytes = ctx->cascade_ws.cap;
    return SR_OK;
}

int sr_cascade_plane_u8(sr_ctx *ctx, const sr_cascade *model, const uint8_t *d_img, int64_t stride, int h, int w, int cn,
                        const sr_cascade_params *params, int k, uint8_t *h_plane)
{
    CTX_ENTER(ctx);
    if (bad_image(d_img, stride, h, w, cn) || !h_plane) return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_plane_u8: bad arguments");
    CcPlan pl;
    SRCHK(cascade_plan("sr_cascade_plane_u8", model, h, w, params, &pl));
    if (k < 0 || k >= (int)pl.scales.size())
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_plane_u8: scale %d of %d", k, (int)pl.scales.size());
    CcView v;
    SRCHK(build_pyramid(ctx, "sr_cascade_plane_u8", model, d_img, stride, h, w, cn, pl, &v));
    HIPCHK(hipMemcpyAsync(h_plane, v.planes + pl.dev[k].pix_off, (size_t)pl.scales[k].sw * pl.scales[k].sh, hipMemcpyDeviceToHost,
                          ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_cascade_stage_map_u8(sr_ctx *ctx, const sr_cascade *model, const uint8_t *d_img, int64_t stride, int h, int w, int cn, int step,
                            int32_t *h_map, int64_t cap, int64_t *count)
{
    CTX_ENTER(ctx);
    if (bad_image(d_img, stride, h, w, cn) || !count || cap < 0 || (cap > 0 && !h_map))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_stage_map_u8: bad arguments");
    CcPlan pl;
    SRCHK(cascade_plan_map("sr_cascade_stage_map_u8", model, h, w, step, &pl));
    *count = pl.positions;
    if (pl.positions > cap || pl.scales.empty()) return SR_OK;
    CcView v;
    SRCHK(build_pyramid(ctx, "sr_cascade_stage_map_u8", model, d_img, stride, h, w, cn, pl, &v));
    int *d_map = (int *)v.surv;                            // the survivor list is not in use here: one int per position
    hipLaunchKernelGGL(k_cc_map, dim3(cc_grid(pl.positions)), dim3(CC_THREADS), 0, ctx->stream, v.md, pl.dev[0], (const unsigned *)v.T,
                       (const unsigned *)v.S, d_map);
    SRCHK(check_launch("sr_cascade_stage_map_u8"));
    HIPCHK(hipMemcpyAsync(h_map, d_map, (size_t)pl.positions * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}
