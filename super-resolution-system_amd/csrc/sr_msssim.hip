// sr_msssim.hip -- multi-scale SSIM of two u8 images (sr_ms_ssim_plan, sr_ms_ssim_u8, sr_ms_ssim_value, sr_ms_ssim_planes).
//
// The definition is in include/sr_hip.h: L <= 5 levels, level j + 1 is the exact 2 x 2 mean of level j (a last odd row or column
// is dropped), per level the Gaussian-11 (sigma 1.5) SSIM over the valid region with the population covariance, split into
// l and cs; S_j = mean(l cs), CS_j = mean(cs); the value is the weighted product, finished on the host.
//
// One kernel, one launch per level, on the column march of sr_ssim11.h (window, vertical pass, LDS rows, horizontal pass,
// quotient, block tree are there).  What is this file's own:
//   k_msssim_level<SRC>  SRC = 1 / 3: the two u8 images (level 0; 3: RGB -> gray once per pixel), SRC = 0: a level plane.
//     A block owns S11_OUT map columns and one chunk of map rows, valid region only (no border rule): 10 halo rows per chunk,
//     10 halo columns per block, each input row is read once per block.  l cs and cs come from one reciprocal and are added
//     per column in row order.
//     Pooling in the same pass: on every second row the thread of an even column adds its column's last two rows to its
//     right neighbour's (one wave shuffle) and stores the 2 x 2 SUM as one dword x | y << 16 of the next level's plane: a
//     level-j value is the integer sum of 4^j u8 values (<= 255 * 256 = 65280 at j = 4), never divided, so nothing rounds.
//     Chunks start on even rows, S11_OUT is even, the last chunk / column block takes the rest: every pooled pixel is
//     written exactly once.
//     SSIM does not change when x and y are scaled by 4^j and C1, C2 by 16^j, so level j works on the integer sums as they are.
//     Level 0 uses the packed u8 window; from level 1 on x y still fits 32 bits unsigned (65280^2 < 2^32) but x^2 + y^2 does
//     not: it is formed and kept in fp64, exact below 2^53 (the 16-bit-sums window).
//   The per-block partials go through reduce_partials.
// The level planes and the partials are context scratch (sr_ctx::msssim_ws), grown on demand: 4 bytes per level-1 pixel and a
// third more for the coarser levels, about h w / 3 * 4 bytes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "sr_ctx.h"
#include "sr_device.h"
#include "sr_ssim11.h"

namespace {

constexpr int MS_MAX_LEVELS = 5;

struct MsParams {
    int h, w;                   // this level's size
    int step;                   // map rows per chunk (even)
    int shift;                  // gray_shift (SRC == 3)
    int emit;                   // write the next level's plane
    int ow;                     // its width, w / 2
    double c1, c2;              // C1, C2 scaled by 16^level
    double k[6];                // k[0] centre tap, k[j] the +-j taps
};

struct MsPlan {
    int lh[MS_MAX_LEVELS], lw[MS_MAX_LEVELS];
    uint64_t count[MS_MAX_LEVELS];
    size_t off_plane[MS_MAX_LEVELS];        // [0] unused
    PartialsLayout red;
    size_t off_res, total;
    int step[MS_MAX_LEVELS], gx[MS_MAX_LEVELS], gy[MS_MAX_LEVELS];
};

template <int SRC>
__device__ __forceinline__ void ms_load(const unsigned char *__restrict__ pa, const unsigned char *__restrict__ pb, int shift,
                                        unsigned &x, unsigned &y)
{
    if constexpr (SRC == 0) {
        const unsigned v = *(const unsigned *)pa;
        x = v & 0xFFFFu;
        y = v >> 16;
    } else if constexpr (SRC == 1) {
        x = pa[0];
        y = pb[0];
    } else {
        x = (unsigned)gray_rgb(pa[0], pa[1], pa[2], shift);
        y = (unsigned)gray_rgb(pb[0], pb[1], pb[2], shift);
    }
}

template <int SRC>
__global__ __launch_bounds__(S11_TX) void k_msssim_level(const unsigned char *__restrict__ a, long long sa,
                                                         const unsigned char *__restrict__ b, long long sb, MsParams P,
                                                         unsigned *__restrict__ next, double *__restrict__ part)
{
    constexpr bool WIDE = SRC == 0;
    constexpr int PX = SRC == 0 ? 4 : SRC;                               // bytes per pixel of a source row
    __shared__ double F[2][4][S11_TX];
    const int t = threadIdx.x;
    const int mh = P.h - 2 * S11_R;                                      // map rows
    const int y0 = (int)blockIdx.x * P.step, y1 = min(y0 + P.step, mh);  // this chunk's map rows = its first input rows
    const bool last_chunk = blockIdx.x == gridDim.x - 1, last_cols = blockIdx.y == gridDim.y - 1;
    const int c = (int)blockIdx.y * S11_OUT + t;                         // the input column this thread filters vertically
    const bool in = c < P.w;
    const bool own = t < S11_OUT && c <= P.w - S11_SIDE;                 // ... and the map column it produces
    // pooling: input rows [y0, pool_end) and the block's own columns (the last block of either axis takes the rest)
    const int pool_end = last_chunk ? P.h : y1;
    const bool pool_col = !(t & 1) && (t < S11_OUT || last_cols) && c + 1 < P.w;
    const unsigned char *ca = a + (size_t)(in ? c : 0) * PX, *cb = WIDE ? ca : b + (size_t)(in ? c : 0) * PX;
    if constexpr (WIDE) sb = sa;
    // level 0: wx holds x | y << 14 and wy is not used; from level 1 on x^2 + y^2 is fp64
    Window11<unsigned> wx, wy, wq;
    Window11<std::conditional_t<WIDE, double, unsigned>> wp;
    double sum_s = 0.0, sum_cs = 0.0;
    const double kk[6] = {P.k[0], P.k[1], P.k[2], P.k[3], P.k[4], P.k[5]};
    const int nrows = (y1 - y0) + 2 * S11_R;                             // input rows y0 .. y1 + 9 (< h)
    unsigned nx = 0u, ny = 0u;
    if (in) ms_load<SRC>(ca + (size_t)y0 * (size_t)sa, cb + (size_t)y0 * (size_t)sb, P.shift, nx, ny);
#pragma unroll 1
    for (int lr = 0; lr < nrows; ++lr) {
        wq.push(nx * ny);                                                // <= 65280^2 < 2^32
        if constexpr (WIDE) {
            wx.push(nx);
            wy.push(ny);
            wp.push(fma((double)nx, (double)nx, (double)ny * (double)ny));    // exact: < 2^34
        } else {
            wx.push(nx | (ny << 14));
            wp.push(nx * nx + ny * ny);
        }
        if (in) {   // the next row is requested before this one is worked on (the last iteration reads its own row again)
            const size_t sy = (size_t)(y0 + min(lr + 1, nrows - 1));
            ms_load<SRC>(ca + sy * (size_t)sa, cb + sy * (size_t)sb, P.shift, nx, ny);
        }
        const int r = y0 + lr;                                           // the input row just pushed
        if (P.emit && (lr & 1) && r < pool_end) {                        // block-uniform; y0 is even, so r is odd
            unsigned px, py;
            if constexpr (WIDE) {
                const unsigned vx = wx[9] + wx[10], vy = wy[9] + wy[10];
                px = vx + (unsigned)__shfl_down((int)vx, 1);
                py = vy + (unsigned)__shfl_down((int)vy, 1);
            } else {
                const unsigned v = wx[9] + wx[10];
                const unsigned s4 = v + (unsigned)__shfl_down((int)v, 1);    // fields <= 1020 < 2^14
                px = s4 & 0x3FFFu;
                py = s4 >> 14;
            }
            if (pool_col) next[(size_t)(r >> 1) * (size_t)P.ow + (size_t)(c >> 1)] = px | (py << 16);
        }
        if (lr < 2 * S11_R) continue;                                    // block-uniform
        const int pb = lr & 1;
        {
            double hv[4];
            if constexpr (WIDE) s11_col_pass<true>(wx, wy, wp, wq, kk, hv);    // the integer pair sum of two x y can pass 2^32
            else s11_col_pass_packed(wx, wp, wq, kk, hv);
            s11_store_col(F[pb], t, hv);
        }
        __syncthreads();
        if (!own) continue;
        double u[4];
        s11_row_pass(F[pb], t + S11_R, kk, u);
        const SsimTerms q = ssim_terms(u[0], u[1], u[2], u[3], P.c1, P.c2);
        const double rb = ssim_recip(q.b1 * q.b2);
        sum_cs += (q.a2 * q.b1) * rb;
        sum_s += (q.a1 * q.a2) * rb;
    }
    // columns that produce nothing add 0
    s11_block_sum2(&F[0][0][0], &F[0][1][0], t, own ? sum_s : 0.0, own ? sum_cs : 0.0,
                   part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2);
}

// sizes, counts, launch shapes and the scratch layout; the refusals of sr_ms_ssim_plan
int ms_plan(const char *scope, int h, int w, int levels, MsPlan *p)
{
    if (levels < 1 || levels > MS_MAX_LEVELS)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: levels must be 1 .. %d (got %d)", scope, MS_MAX_LEVELS, levels);
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need h, w >= 1", scope);
    const int min_side = S11_SIDE << (levels - 1);
    if (h < min_side || w < min_side)
        return sr_set_error(SR_ERR_SHAPE, "%s: image %dx%d is too small for %d levels: both sides must be at least %d (11 at the "
                            "coarsest level)", scope, w, h, levels, min_side);
    memset(p, 0, sizeof(*p));
    size_t off = 0, nblk_max = 0;
    for (int j = 0; j < levels; ++j) {
        p->lh[j] = h >> j;
        p->lw[j] = w >> j;
        const int mh = p->lh[j] - 2 * S11_R, mw = p->lw[j] - 2 * S11_R;
        p->count[j] = (uint64_t)mh * (uint64_t)mw;
        p->gy[j] = (mw + S11_OUT - 1) / S11_OUT;
        const ChunkCut cut = s11_chunk_cut(mh, p->gy[j], true);         // even: a pooled row pair never straddles two chunks
        p->step[j] = cut.step;
        p->gx[j] = cut.count;
        nblk_max = std::max(nblk_max, (size_t)p->gx[j] * (size_t)p->gy[j]);
        if (j >= 1) {
            p->off_plane[j] = off;
            off += up256((size_t)p->lh[j] * (size_t)p->lw[j] * 4);
        }
    }
    p->red = s11_partials_layout(off, nblk_max);
    p->off_res = p->red.end;
    p->total = p->off_res + up256(MS_MAX_LEVELS * 2 * sizeof(double));
    return SR_OK;
}

const double MS_WEIGHTS[MS_MAX_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};    // Wang, Simoncelli, Bovik 2003

}  // namespace

extern "C" {

int sr_ms_ssim_plan(int h, int w, int levels, int *level_h, int *level_w, uint64_t *counts, size_t *scratch_bytes)
{
    MsPlan p;
    const int rc = ms_plan("sr_ms_ssim_plan", h, w, levels, &p);
    if (rc) return rc;
    for (int j = 0; j < levels; ++j) {
        if (level_h) level_h[j] = p.lh[j];
        if (level_w) level_w[j] = p.lw[j];
        if (counts) counts[j] = p.count[j];
    }
    if (scratch_bytes) *scratch_bytes = p.total;
    return SR_OK;
}

int sr_ms_ssim_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w, int cn,
                  int gray_shift, double data_range, int levels, sr_ms_ssim_level *h_out)
{
    // every argument check comes before the context (and so the device) is touched
    if (!d_a || !d_b || !h_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_ms_ssim_u8: null argument");
    if (cn != 1 && cn != 3) return sr_set_error(SR_ERR_INVALID_ARG, "sr_ms_ssim_u8: need 1 or 3 channels");
    if (gray_shift != 14 && gray_shift != 15) return sr_set_error(SR_ERR_INVALID_ARG, "sr_ms_ssim_u8: gray_shift must be 14 or 15");
    if (!std::isfinite(data_range) || !(data_range > 0.0))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_ms_ssim_u8: data_range must be finite and positive");
    MsPlan p;
    int rc = ms_plan("sr_ms_ssim_u8", h, w, levels, &p);
    if (rc) return rc;
    const int64_t min_stride = (int64_t)w * cn;
    if (stride_a < min_stride || stride_b < min_stride) return sr_set_error(SR_ERR_SHAPE, "sr_ms_ssim_u8: stride smaller than a row");
    CTX_ENTER(ctx);
    ctx->msssim_levels = 0;                                              // the planes are about to be overwritten
    SRCHK(ctx->msssim_ws.reserve(ctx, "sr_ms_ssim_u8", p.total));
    char *ws = ctx->msssim_ws.as<char>();
    double *part = (double *)(ws + p.red.off_part), *buf0 = (double *)(ws + p.red.off_buf0), *buf1 = (double *)(ws + p.red.off_buf1),
           *res = (double *)(ws + p.off_res);
    static const char *const names[MS_MAX_LEVELS] = {"msssim_l0", "msssim_l1", "msssim_l2", "msssim_l3", "msssim_l4"};
    double scale = 1.0;                                                  // 16^level
    for (int j = 0; j < levels; ++j, scale *= 16.0) {
        MsParams P;
        memset(&P, 0, sizeof(P));
        P.h = p.lh[j]; P.w = p.lw[j]; P.step = p.step[j]; P.shift = gray_shift;
        P.emit = j + 1 < levels ? 1 : 0;
        P.ow = P.w / 2;
        P.c1 = (0.01 * data_range) * (0.01 * data_range) * scale;
        P.c2 = (0.03 * data_range) * (0.03 * data_range) * scale;
        gauss_taps(P.k);
        unsigned *next = P.emit ? (unsigned *)(ws + p.off_plane[j + 1]) : nullptr;
        const dim3 grid((unsigned)p.gx[j], (unsigned)p.gy[j]), block(S11_TX);
        {
            ProfScope ps(ctx, names[j]);
            if (j > 0) {
                const unsigned char *src = (const unsigned char *)(ws + p.off_plane[j]);
                hipLaunchKernelGGL(k_msssim_level<0>, grid, block, 0, ctx->stream, src, (long long)P.w * 4, src, (long long)P.w * 4, P,
                                   next, part);
            } else if (cn == 3) {
                hipLaunchKernelGGL(k_msssim_level<3>, grid, block, 0, ctx->stream, d_a, (long long)stride_a, d_b, (long long)stride_b, P,
                                   next, part);
            } else {
                hipLaunchKernelGGL(k_msssim_level<1>, grid, block, 0, ctx->stream, d_a, (long long)stride_a, d_b, (long long)stride_b, P,
                                   next, part);
            }
            const double *sums = reduce_partials(ctx, part, (long long)p.gx[j] * p.gy[j], 2, buf0, buf1);
            rc = check_launch(names[j]);
            if (rc) return rc;
            HIPCHK(hipMemcpyAsync(res + 2 * j, sums, 2 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        }
    }
    double h_res[MS_MAX_LEVELS * 2];
    HIPCHK(hipMemcpyAsync(h_res, res, (size_t)levels * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    for (int j = 0; j < levels; ++j) {
        h_out[j].sum_lcs = h_res[2 * j];
        h_out[j].sum_cs = h_res[2 * j + 1];
        h_out[j].count = p.count[j];
    }
    ctx->msssim_h = h;
    ctx->msssim_w = w;
    ctx->msssim_levels = levels;
    return SR_OK;
}

double sr_ms_ssim_value(const sr_ms_ssim_level *out, int levels, const double *weights)
{
    const double nan = std::nan("");
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_ms_ssim_value: null argument"), nan;
    if (levels < 1 || levels > MS_MAX_LEVELS)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_ms_ssim_value: levels must be 1 .. %d (got %d)", MS_MAX_LEVELS, levels), nan;
    const double *wt = weights ? weights : MS_WEIGHTS;
    double v = 1.0;
    for (int j = 0; j < levels; ++j) {
        if (out[j].count == 0) return sr_set_error(SR_ERR_INVALID_ARG, "sr_ms_ssim_value: level %d has no samples", j), nan;
        const double mean = (j == levels - 1 ? out[j].sum_lcs : out[j].sum_cs) / (double)out[j].count;
        v *= std::pow(std::max(mean, 0.0), wt[j]);
    }
    return v;
}

int sr_ms_ssim_planes(sr_ctx *ctx, int level, uint16_t *h_x, uint16_t *h_y)
{
    if (!h_x || !h_y) return sr_set_error(SR_ERR_INVALID_ARG, "sr_ms_ssim_planes: null argument");
    CTX_ENTER(ctx);
    if (ctx->msssim_levels < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_ms_ssim_planes: no sr_ms_ssim_u8 call has completed on this context");
    if (level < 1 || level >= ctx->msssim_levels)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_ms_ssim_planes: the last call stored levels 1 .. %d (asked for %d)",
                            ctx->msssim_levels - 1, level);
    MsPlan p;
    const int rc = ms_plan("sr_ms_ssim_planes", ctx->msssim_h, ctx->msssim_w, ctx->msssim_levels, &p);
    if (rc) return rc;
    const size_t n = (size_t)p.lh[level] * (size_t)p.lw[level];
    std::vector<unsigned> host(n);
    HIPCHK(hipMemcpyAsync(host.data(), ctx->msssim_ws.as<char>(p.off_plane[level]), n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    for (size_t i = 0; i < n; ++i) {
        h_x[i] = (uint16_t)(host[i] & 0xFFFFu);
        h_y[i] = (uint16_t)(host[i] >> 16);
    }
    return SR_OK;
}

}  // extern "C"
