// sr_srbench.hip -- the SR-benchmark PSNR / SSIM of two u8 images (sr_bench_plan, sr_bench_u8): border crop, then the
// channels as they are, the BT.601 luma Y carried exactly, or MATLAB's rounded u8 luma.
//
// The definition is in include/sr_hip.h.  One kernel, one launch, one pass over both images for the squared differences AND
// the Gaussian-11 SSIM, on the column march of sr_ssim11.h (window, vertical pass, LDS rows, horizontal pass, quotient, block
// tree are there).  What is this file's own:
//   k_srbench<MODE, PX>  A block owns S11_OUT map columns and one chunk of map rows of one plane (blockIdx.z: the channel in
//     SR_BENCH_CHANNELS with 3 channels), valid region only.  The SSIM terms are added per column in row order.  The squared
//     difference of a pixel is added by the block that owns it: input rows [y0, y1) of the chunk and the block's own S11_OUT
//     columns, the last block of either axis taking the rest (the 10 halo rows / columns), so every cropped pixel is counted
//     exactly once.  Per thread that sum stays an integer and becomes fp64 once.
//   The window, by mode:
//     u8 planes (CHANNELS, Y_ROUND)  the packed u8 window.
//     Y                              X = 65481 R + 128553 G + 24966 B + 4080000 (= 255000 Y, < 2^26) and X' as 32-bit
//                                    integers, X X' and X^2 + X'^2 as fp64, exact below 2^53 and formed once per pixel (the
//                                    26-bit-luma window).  SSIM is homogeneous of degree 0 in (planes, C1, C2): C1, C2 come in
//                                    multiplied by 255000^2 and the integers are filtered as they are.
//   Pixels are read byte by byte: the crop is pointer arithmetic on the host and crop_border * cn has any residue mod 4.
//   The per-block partials go through reduce_partials.
// The partials are context scratch (sr_ctx::bench_ws), grown on demand: 16 bytes per block.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "sr_ctx.h"
#include "sr_device.h"
#include "sr_ssim11.h"

namespace {

constexpr int SB_YSCALE = 255000;          // X = SB_YSCALE * Y

enum { SB_PLANE = 0, SB_YROUND = 1, SB_Y = 2 };       // what a kernel instantiation filters

struct SbParams {
    int h, w;                   // the cropped size
    int step;                   // map rows per chunk
    double c1, c2;              // C1, C2 (SB_Y: times 255000^2)
    double k[6];                // k[0] centre tap, k[j] the +-j taps
};

struct SbPlan {
    int ch, cw, planes;
    uint64_t n_elems, n_map;
    int step, gx, gy;
    PartialsLayout red;
    size_t total;
};

__device__ __forceinline__ unsigned sb_x(const unsigned char *p)
{
    return 65481u * p[0] + 128553u * p[1] + 24966u * p[2] + 4080000u;    // <= 59 925 000
}

template <int MODE>
__device__ __forceinline__ void sb_load(const unsigned char *__restrict__ pa, const unsigned char *__restrict__ pb, unsigned &x,
                                        unsigned &y)
{
    if constexpr (MODE == SB_PLANE) {
        x = pa[0];
        y = pb[0];
    } else if constexpr (MODE == SB_YROUND) {
        x = (2u * sb_x(pa) + 255000u) / 510000u;                         // MATLAB's uint8 rgb2ycbcr: half up, 16 .. 235
        y = (2u * sb_x(pb) + 255000u) / 510000u;
    } else {
        x = sb_x(pa);
        y = sb_x(pb);
    }
}

template <int MODE, int PX>
__global__ __launch_bounds__(S11_TX) void k_srbench(const unsigned char *__restrict__ a, long long sa,
                                                    const unsigned char *__restrict__ b, long long sb, SbParams P,
                                                    double *__restrict__ part)
{
    constexpr bool WIDE = MODE == SB_Y;
    __shared__ double F[2][4][S11_TX];
    const int t = threadIdx.x;
    const int mh = P.h - 2 * S11_R;                                      // map rows
    const int y0 = (int)blockIdx.x * P.step, y1 = min(y0 + P.step, mh);  // this chunk's map rows = its first input rows
    const bool last_chunk = blockIdx.x == gridDim.x - 1, last_cols = blockIdx.y == gridDim.y - 1;
    const int c = (int)blockIdx.y * S11_OUT + t;                         // the input column this thread filters vertically
    const bool in = c < P.w;
    const bool own = t < S11_OUT && c <= P.w - S11_SIDE;                 // ... and the map column it produces
    // squared differences: input rows [y0, sse_end) of the block's own columns (the last block of either axis takes the rest)
    const int sse_rows = (last_chunk ? P.h : y1) - y0;
    const bool sse_col = in && (t < S11_OUT || last_cols);
    const size_t coff = (size_t)(in ? c : 0) * PX + (MODE == SB_PLANE ? blockIdx.z : 0);
    const unsigned char *ca = a + coff, *cb = b + coff;
    // u8 planes: wx holds x | y << 14 and wy is not used
    using prod_t = std::conditional_t<WIDE, double, unsigned>;
    Window11<unsigned> wx, wy;
    Window11<prod_t> wq, wp;
    double sum_s = 0.0;
    unsigned long long sse = 0ull;                                       // one chunk column of (X - X')^2 < 2^52 fits
    const double kk[6] = {P.k[0], P.k[1], P.k[2], P.k[3], P.k[4], P.k[5]};
    const int nrows = (y1 - y0) + 2 * S11_R;                             // input rows y0 .. y1 + 9 (< h)
    unsigned nx = 0u, ny = 0u;
    if (in) sb_load<MODE>(ca + (size_t)y0 * (size_t)sa, cb + (size_t)y0 * (size_t)sb, nx, ny);
#pragma unroll 1
    for (int lr = 0; lr < nrows; ++lr) {
        if constexpr (WIDE) {
            const double dx = (double)nx, dy = (double)ny;               // < 2^26: every product below is exact
            wx.push(nx);
            wy.push(ny);
            wq.push(dx * dy);
            wp.push(fma(dx, dx, dy * dy));                               // < 2^53
        } else {
            wx.push(nx | (ny << 14));
            wq.push(nx * ny);
            wp.push(nx * nx + ny * ny);
        }
        if (lr < sse_rows && sse_col) {
            const long long d = (long long)nx - (long long)ny;
            sse += (unsigned long long)(d * d);
        }
        if (in) {   // the next row is requested before this one is worked on (the last iteration reads its own row again)
            const size_t sy = (size_t)(y0 + min(lr + 1, nrows - 1));
            sb_load<MODE>(ca + sy * (size_t)sa, cb + sy * (size_t)sb, nx, ny);
        }
        if (lr < 2 * S11_R) continue;                                    // block-uniform
        const int pb = lr & 1;
        {
            double hv[4];
            if constexpr (WIDE) s11_col_pass<false>(wx, wy, wp, wq, kk, hv);   // pair sums < 2^27
            else s11_col_pass_packed(wx, wp, wq, kk, hv);
            s11_store_col(F[pb], t, hv);
        }
        __syncthreads();
        if (!own) continue;
        double u[4];
        s11_row_pass(F[pb], t + S11_R, kk, u);
        sum_s += ssim_quot(u[0], u[1], u[2], u[3], P.c1, P.c2);
    }
    // columns that produce nothing add 0
    s11_block_sum2(&F[0][0][0], &F[0][1][0], t, own ? sum_s : 0.0, (double)sse,
                   part + (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2);
}

// the cropped size, counts, launch shape and scratch layout; every shape refusal of sr_bench_plan
int sb_plan(const char *scope, int h, int w, int cn, int crop_border, int mode, SbPlan *p)
{
    if (cn != 1 && cn != 3) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need 1 or 3 channels (got %d)", scope, cn);
    if (mode != SR_BENCH_CHANNELS && mode != SR_BENCH_Y && mode != SR_BENCH_Y_ROUND)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: unknown mode %d", scope, mode);
    if (mode != SR_BENCH_CHANNELS && cn != 3)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: the Y modes need 3 channels (RGB), got %d", scope, cn);
    if (crop_border < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: crop_border must be >= 0 (got %d)", scope, crop_border);
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need h, w >= 1", scope);
    const long long ch = (long long)h - 2LL * crop_border, cw = (long long)w - 2LL * crop_border;
    if (ch < S11_SIDE || cw < S11_SIDE)
        return sr_set_error(SR_ERR_SHAPE, "%s: image %dx%d with crop_border %d leaves %lldx%lld: both sides must be at least %d "
                            "after the crop", scope, w, h, crop_border, std::max(cw, 0LL), std::max(ch, 0LL), S11_SIDE);
    memset(p, 0, sizeof(*p));
    p->ch = (int)ch;
    p->cw = (int)cw;
    p->planes = mode == SR_BENCH_CHANNELS ? cn : 1;
    const int mh = p->ch - 2 * S11_R, mw = p->cw - 2 * S11_R;
    p->n_elems = (uint64_t)p->ch * (uint64_t)p->cw * (uint64_t)p->planes;
    p->n_map = (uint64_t)mh * (uint64_t)mw * (uint64_t)p->planes;
    p->gy = (mw + S11_OUT - 1) / S11_OUT;
    const ChunkCut cut = s11_chunk_cut(mh, (long long)p->gy * p->planes, false);
    p->step = cut.step;
    p->gx = cut.count;
    p->red = s11_partials_layout(0, (size_t)p->gx * (size_t)p->gy * (size_t)p->planes);
    p->total = p->red.end;
    return SR_OK;
}

}  // namespace

extern "C" {

int sr_bench_plan(int h, int w, int cn, int crop_border, int mode, int *ch, int *cw, uint64_t *n_elems, uint64_t *n_map,
                  size_t *scratch_bytes)
{
    SbPlan p;
    const int rc = sb_plan("sr_bench_plan", h, w, cn, crop_border, mode, &p);
    if (rc) return rc;
    if (ch) *ch = p.ch;
    if (cw) *cw = p.cw;
    if (n_elems) *n_elems = p.n_elems;
    if (n_map) *n_map = p.n_map;
    if (scratch_bytes) *scratch_bytes = p.total;
    return SR_OK;
}

int sr_bench_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w, int cn,
                int crop_border, int mode, double data_range, sr_bench_sums *h_out)
{
    // every argument check comes before the context (and so the device) is touched
    if (!d_a || !d_b || !h_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_bench_u8: null argument");
    if (!std::isfinite(data_range) || !(data_range > 0.0))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_bench_u8: data_range must be finite and positive");
    SbPlan p;
    int rc = sb_plan("sr_bench_u8", h, w, cn, crop_border, mode, &p);
    if (rc) return rc;
    const int64_t min_stride = (int64_t)w * cn;
    if (stride_a < min_stride || stride_b < min_stride) return sr_set_error(SR_ERR_SHAPE, "sr_bench_u8: stride smaller than a row");
    CTX_ENTER(ctx);
    SRCHK(ctx->bench_ws.reserve(ctx, "sr_bench_u8", p.total));
    char *ws = ctx->bench_ws.as<char>();
    double *part = (double *)(ws + p.red.off_part), *buf0 = (double *)(ws + p.red.off_buf0), *buf1 = (double *)(ws + p.red.off_buf1);
    SbParams P;
    memset(&P, 0, sizeof(P));
    P.h = p.ch; P.w = p.cw; P.step = p.step;
    const double scale = mode == SR_BENCH_Y ? (double)SB_YSCALE * (double)SB_YSCALE : 1.0;
    P.c1 = (0.01 * data_range) * (0.01 * data_range) * scale;
    P.c2 = (0.03 * data_range) * (0.03 * data_range) * scale;
    gauss_taps(P.k);
    // the crop: rows [cb, h - cb), columns [cb, w - cb) of both images
    const unsigned char *a = d_a + (size_t)crop_border * (size_t)stride_a + (size_t)crop_border * (size_t)cn;
    const unsigned char *b = d_b + (size_t)crop_border * (size_t)stride_b + (size_t)crop_border * (size_t)cn;
    const dim3 grid((unsigned)p.gx, (unsigned)p.gy, (unsigned)p.planes), block(S11_TX);
    double h_res[2];
    {
        ProfScope ps(ctx, "srbench");
        if (mode == SR_BENCH_Y)
            hipLaunchKernelGGL((k_srbench<SB_Y, 3>), grid, block, 0, ctx->stream, a, (long long)stride_a, b, (long long)stride_b, P, part);
        else if (mode == SR_BENCH_Y_ROUND)
            hipLaunchKernelGGL((k_srbench<SB_YROUND, 3>), grid, block, 0, ctx->stream, a, (long long)stride_a, b, (long long)stride_b, P,
                               part);
        else if (cn == 3)
            hipLaunchKernelGGL((k_srbench<SB_PLANE, 3>), grid, block, 0, ctx->stream, a, (long long)stride_a, b, (long long)stride_b, P,
                               part);
        else
            hipLaunchKernelGGL((k_srbench<SB_PLANE, 1>), grid, block, 0, ctx->stream, a, (long long)stride_a, b, (long long)stride_b, P,
                               part);
        const double *sums = reduce_partials(ctx, part, (long long)p.gx * p.gy * p.planes, 2, buf0, buf1);
        rc = check_launch("srbench");
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(h_res, sums, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(stream_sync(ctx));
    h_out->ssim_sum = h_res[0];
    h_out->sse = mode == SR_BENCH_Y ? h_res[1] / ((double)SB_YSCALE * (double)SB_YSCALE) : h_res[1];
    h_out->n_elems = p.n_elems;
    h_out->n_map = p.n_map;
    return SR_OK;
}

}  // extern "C"
