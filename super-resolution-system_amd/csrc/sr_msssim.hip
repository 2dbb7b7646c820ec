// sr_msssim.hip -- multi-scale SSIM of two u8 images (sr_ms_ssim_plan, sr_ms_ssim_u8, sr_ms_ssim_value, sr_ms_ssim_planes).
//
// The definition is in include/sr_hip.h: L <= 5 levels, level j + 1 is the exact 2 x 2 mean of level j (a last odd row or column
// is dropped), per level the Gaussian-11 (sigma 1.5) SSIM over the valid region with the population covariance, split into
// l and cs; S_j = mean(l cs), CS_j = mean(cs); the value is the weighted product, finished on the host.
//
// One kernel, one launch per level:
//   k_msssim_level<SRC>  SRC = 1 / 3: the two u8 images (level 0; 3: RGB -> gray once per pixel), SRC = 0: a level plane.
//     A block owns MS_OUT map columns and one chunk of map rows.  Each thread owns an input column and walks down the chunk:
//     the vertical pass of its column comes from an 11-row register window of exact integers (x, y, x y, x^2 + y^2), the
//     horizontal pass reads the neighbours' vertical results through LDS; l cs and cs are added per column in row order.
//     Each input row is read once per block (10 halo rows per chunk, 10 halo columns per block).  On every second row the
//     thread of an even column adds its column's last two rows to its right neighbour's (one wave shuffle) and stores the
//     2 x 2 SUM as one dword x | y << 16 of the next level's plane: a level-j value is the integer sum of 4^j u8 values
//     (<= 255 * 256 = 65280 at j = 4), never divided, so nothing rounds.  Chunks start on even rows, MS_OUT is even, the
//     last chunk / column block takes the rest: every pooled pixel is written exactly once.
//     SSIM does not change when x and y are scaled by 4^j and C1, C2 by 16^j, so level j works on the integer sums as they are.
//     Level 0 keeps x | y << 14 packed and its products in 32 bits (as sr_qmap.hip does); from level 1 on x y still fits 32
//     bits unsigned (65280^2 < 2^32) but x^2 + y^2 does not: it is formed and kept in fp64, exact below 2^53.
//   The block's 256 column sums go through a fixed tree, the per-block partials through reduce_partials: no floating-point
//   atomics, equal inputs give equal bits.
// The level planes and the partials are context scratch (sr_ctx::msssim_ws), grown on demand: 4 bytes per level-1 pixel and a
// third more for the coarser levels, about h w / 3 * 4 bytes.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "sr_ctx.h"
#include "sr_device.h"

namespace {

constexpr int MS_TX = 256;                 // threads = input columns of a block
constexpr int MS_R = 5;                    // radius of the Gaussian
constexpr int MS_OUT = MS_TX - 2 * MS_R;   // map columns a block produces (even: a pooled pair never straddles two blocks)
constexpr int MS_ROWS = 128;               // longest chunk of map rows (10 halo rows on top: 8 %)
constexpr int MS_ROWS_MIN = 16;            // shortest chunk a small level is cut into ...
constexpr int MS_BLOCKS = 1024;            // ... to reach this many blocks
constexpr int MS_MAX_LEVELS = 5;
constexpr int MS_MIN_SIDE = 2 * MS_R + 1;

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
    size_t off_part, off_buf0, off_buf1, off_res, total;
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

// 1 / d: hardware estimate + one Newton step (relative error ~1e-15), d a product of positive SSIM terms
__device__ __forceinline__ double ms_recip(double d)
{
    const double r = __builtin_amdgcn_rcp(d);
    return fma(fma(-d, r, 1.0), r, r);
}

template <int SRC>
__global__ __launch_bounds__(MS_TX) void k_msssim_level(const unsigned char *__restrict__ a, long long sa,
                                                        const unsigned char *__restrict__ b, long long sb, MsParams P,
                                                        unsigned *__restrict__ next, double *__restrict__ part)
{
    constexpr bool WIDE = SRC == 0;
    constexpr int PX = SRC == 0 ? 4 : SRC;                               // bytes per pixel of a source row
    // vertical results of one row, double-buffered by row parity: one barrier per row
    __shared__ double F[2][4][MS_TX];
    const int t = threadIdx.x;
    const int mh = P.h - 2 * MS_R;                                       // map rows
    const int y0 = (int)blockIdx.x * P.step, y1 = min(y0 + P.step, mh);  // this chunk's map rows = its first input rows
    const bool last_chunk = blockIdx.x == gridDim.x - 1, last_cols = blockIdx.y == gridDim.y - 1;
    const int c = (int)blockIdx.y * MS_OUT + t;                          // the input column this thread filters vertically
    const bool in = c < P.w;
    const bool own = t < MS_OUT && c <= P.w - MS_MIN_SIDE;               // ... and the map column it produces
    // pooling: input rows [y0, pool_end) and the block's own columns (the last block of either axis takes the rest)
    const int pool_end = last_chunk ? P.h : y1;
    const bool pool_col = !(t & 1) && (t < MS_OUT || last_cols) && c + 1 < P.w;
    const unsigned char *ca = a + (size_t)(in ? c : 0) * PX, *cb = WIDE ? ca : b + (size_t)(in ? c : 0) * PX;
    if constexpr (WIDE) sb = sa;
    // rows lr - 10 .. lr of this column.  Level 0: x | y << 14 packed (pair sums <= 510 stay in their fields)
    unsigned wx[11], wy[WIDE ? 11 : 1], wq[11], wp[WIDE ? 1 : 11];
    double wpd[WIDE ? 11 : 1];
#pragma unroll
    for (int i = 0; i < 11; ++i) {
        wx[i] = wq[i] = 0u;
        if constexpr (WIDE) { wy[i] = 0u; wpd[i] = 0.0; }
        else wp[i] = 0u;
    }
    double sum_s = 0.0, sum_cs = 0.0;
    const double kk[6] = {P.k[0], P.k[1], P.k[2], P.k[3], P.k[4], P.k[5]};
    const int nrows = (y1 - y0) + 2 * MS_R;                              // input rows y0 .. y1 + 9 (< h)
    unsigned nx = 0u, ny = 0u;
    if (in) ms_load<SRC>(ca + (size_t)y0 * (size_t)sa, cb + (size_t)y0 * (size_t)sb, P.shift, nx, ny);
#pragma unroll 1
    for (int lr = 0; lr < nrows; ++lr) {
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            wx[i] = wx[i + 1];
            wq[i] = wq[i + 1];
            if constexpr (WIDE) { wy[i] = wy[i + 1]; wpd[i] = wpd[i + 1]; }
            else wp[i] = wp[i + 1];
        }
        wq[10] = nx * ny;                                                // <= 65280^2 < 2^32
        if constexpr (WIDE) {
            wx[10] = nx;
            wy[10] = ny;
            wpd[10] = fma((double)nx, (double)nx, (double)ny * (double)ny);   // exact: < 2^34
        } else {
            wx[10] = nx | (ny << 14);
            wp[10] = nx * nx + ny * ny;
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
        if (lr < 2 * MS_R) continue;                                     // block-uniform
        const int pb = lr & 1;
        {
            double hx, hy, hp, hq;
            if constexpr (WIDE) {
                hx = (double)wx[5] * kk[0];
                hy = (double)wy[5] * kk[0];
                hp = wpd[5] * kk[0];
                hq = (double)wq[5] * kk[0];
#pragma unroll
                for (int j = 1; j <= MS_R; ++j) {
                    hx = fma((double)(wx[5 - j] + wx[5 + j]), kk[j], hx);
                    hy = fma((double)(wy[5 - j] + wy[5 + j]), kk[j], hy);
                    hp = fma(wpd[5 - j] + wpd[5 + j], kk[j], hp);
                    hq = fma((double)wq[5 - j] + (double)wq[5 + j], kk[j], hq);   // the integer pair sum can pass 2^32
                }
            } else {
                hx = (double)(wx[5] & 0x3FFFu) * kk[0];
                hy = (double)(wx[5] >> 14) * kk[0];
                hp = (double)wp[5] * kk[0];
                hq = (double)wq[5] * kk[0];
#pragma unroll
                for (int j = 1; j <= MS_R; ++j) {
                    const unsigned sxy = wx[5 - j] + wx[5 + j];          // both images in one add
                    hx = fma((double)(sxy & 0x3FFFu), kk[j], hx);
                    hy = fma((double)(sxy >> 14), kk[j], hy);
                    hp = fma((double)(wp[5 - j] + wp[5 + j]), kk[j], hp);
                    hq = fma((double)(wq[5 - j] + wq[5 + j]), kk[j], hq);
                }
            }
            F[pb][0][t] = hx; F[pb][1][t] = hy; F[pb][2][t] = hp; F[pb][3][t] = hq;
        }
        __syncthreads();
        if (!own) continue;
        double u[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            double acc = F[pb][m][t + MS_R] * kk[0];
#pragma unroll
            for (int j = 1; j <= MS_R; ++j) acc = fma(F[pb][m][t + MS_R - j] + F[pb][m][t + MS_R + j], kk[j], acc);
            u[m] = acc;
        }
        // u[2] = E[x^2 + y^2], u[3] = E[x y]
        const double uxuy = u[0] * u[1], uu = fma(u[0], u[0], u[1] * u[1]);
        const double a1 = fma(2.0, uxuy, P.c1), a2 = fma(2.0, u[3] - uxuy, P.c2);
        const double b1 = uu + P.c1, b2 = (u[2] - uu) + P.c2;
        const double rb = ms_recip(b1 * b2);
        sum_cs += (a2 * b1) * rb;
        sum_s += (a1 * a2) * rb;
    }
    // the block's column sums in a fixed tree (columns that produce nothing add 0)
    __syncthreads();
    double *sd0 = &F[0][0][0], *sd1 = &F[0][1][0];
    sd0[t] = own ? sum_s : 0.0;
    sd1[t] = own ? sum_cs : 0.0;
    __syncthreads();
    for (int s = MS_TX / 2; s > 0; s >>= 1) {
        if (t < s) {
            sd0[t] += sd0[t + s];
            sd1[t] += sd1[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        part[blk * 2 + 0] = sd0[0];
        part[blk * 2 + 1] = sd1[0];
    }
}

void ms_gauss_taps(double *k6)
{
    double k[11], sum = 0.0;
    for (int i = 0; i < 11; ++i) {
        const double x = i - 5;
        k[i] = std::exp(-0.5 / (1.5 * 1.5) * x * x);     // scipy.ndimage._gaussian_kernel1d(sigma=1.5, radius=5)
        sum += k[i];
    }
    for (int j = 0; j <= 5; ++j) k6[j] = k[5 + j] / sum;
}

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// sizes, counts, launch shapes and the scratch layout; the refusals of sr_ms_ssim_plan
int ms_plan(const char *scope, int h, int w, int levels, MsPlan *p)
{
    if (levels < 1 || levels > MS_MAX_LEVELS)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: levels must be 1 .. %d (got %d)", scope, MS_MAX_LEVELS, levels);
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need h, w >= 1", scope);
    const int min_side = MS_MIN_SIDE << (levels - 1);
    if (h < min_side || w < min_side)
        return sr_set_error(SR_ERR_SHAPE, "%s: image %dx%d is too small for %d levels: both sides must be at least %d (11 at the "
                            "coarsest level)", scope, w, h, levels, min_side);
    memset(p, 0, sizeof(*p));
    size_t off = 0, nblk_max = 0;
    for (int j = 0; j < levels; ++j) {
        p->lh[j] = h >> j;
        p->lw[j] = w >> j;
        const int mh = p->lh[j] - 2 * MS_R, mw = p->lw[j] - 2 * MS_R;
        p->count[j] = (uint64_t)mh * (uint64_t)mw;
        // Chunks of at most MS_ROWS map rows; a small level takes shorter ones (down to MS_ROWS_MIN) until it has MS_BLOCKS
        // blocks: a block walks its rows one after the other, so a coarse level cut into a few long chunks would take as long
        // as a chunk takes on an empty chip.  The cut depends on the size alone, never on the device: equal bits everywhere.
        p->gy[j] = (mw + MS_OUT - 1) / MS_OUT;
        int rows = MS_ROWS;
        while (rows > MS_ROWS_MIN && (long long)((mh + rows - 1) / rows) * p->gy[j] < MS_BLOCKS) rows /= 2;
        const int n = (mh + rows - 1) / rows;
        p->step[j] = ((mh + n - 1) / n + 1) & ~1;                       // even: a pooled row pair never straddles two chunks
        p->gx[j] = (mh + p->step[j] - 1) / p->step[j];
        nblk_max = std::max(nblk_max, (size_t)p->gx[j] * (size_t)p->gy[j]);
        if (j >= 1) {
            p->off_plane[j] = off;
            off += up256((size_t)p->lh[j] * (size_t)p->lw[j] * 4);
        }
    }
    p->off_part = off;
    off += up256(nblk_max * 2 * sizeof(double));
    p->off_buf0 = off;
    off += up256((nblk_max / 1024 + 2) * 2 * sizeof(double));
    p->off_buf1 = off;
    off += up256((nblk_max / 1024 + 2) * 2 * sizeof(double));
    p->off_res = off;
    off += up256(MS_MAX_LEVELS * 2 * sizeof(double));
    p->total = off;
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
    if (p.total > ctx->msssim_ws_bytes) {
        if (ctx->msssim_ws) {
            HIPCHK(stream_sync(ctx));
            HIPCHK(hipFree(ctx->msssim_ws));
            ctx->msssim_ws = nullptr;
            ctx->msssim_ws_bytes = 0;
        }
        hipError_t e = hipMalloc(&ctx->msssim_ws, p.total);
        if (e != hipSuccess) {
            ctx->msssim_ws = nullptr;
            return sr_set_error(e == hipErrorOutOfMemory ? SR_ERR_OOM : SR_ERR_HIP, "sr_ms_ssim_u8: scratch of %zu bytes: %s", p.total,
                                hipGetErrorString(e));
        }
        ctx->msssim_ws_bytes = p.total;
    }
    char *ws = (char *)ctx->msssim_ws;
    double *part = (double *)(ws + p.off_part), *buf0 = (double *)(ws + p.off_buf0), *buf1 = (double *)(ws + p.off_buf1),
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
        ms_gauss_taps(P.k);
        unsigned *next = P.emit ? (unsigned *)(ws + p.off_plane[j + 1]) : nullptr;
        const dim3 grid((unsigned)p.gx[j], (unsigned)p.gy[j]), block(MS_TX);
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
    HIPCHK(hipMemcpyAsync(host.data(), (char *)ctx->msssim_ws + p.off_plane[level], n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    for (size_t i = 0; i < n; ++i) {
        h_x[i] = (uint16_t)(host[i] & 0xFFFFu);
        h_y[i] = (uint16_t)(host[i] >> 16);
    }
    return SR_OK;
}

}  // extern "C"
