// sr_brisque.hip -- the device side of BRISQUE (sr_brisque_u8, sr_brisque_half_plane): the exact half-resolution plane of any
// H x W >= 16 and, per scale, the moments of the MSCN coefficients and their four rolled products over the whole plane.  The
// definition is in include/sr_hip.h; the plan, the features and the score are host code (sr_brisque_host.cpp).
// The MSCN core is sr_mscn.h's, shared with NIQE (sr_niqe.hip): the half-plane kernel, the two passes of the window, the
// register-window march, the 25 quantities of a position and the block sum.  This unit holds what is BRISQUE's own.
//   k_mscn_half<PX, true>  The exact half plane of a plane of any size: partial blocks, guarded stores, pitch W2.
//   k_brisque_moments<SCALE, PX>  A workgroup of 256 threads owns a 64 x 64 tile of m (the single-pass form: m is never
//     stored to memory).  The tile plus its 3-pixel halo goes into LDS as integers (u8 at scale 1 with the luma on the fly,
//     int32 at scale 2); a pixel outside the plane is 0 there, which is the filter's zero padding.  Thread (c, seg) owns column
//     c and 16 rows and marches down them (mscn_march); m goes to a 65 x 66 float64 LDS tile that also holds what the four
//     shifts read beyond the tile: the row above and a column on each side.  Those m lie on the far side of the plane when the
//     tile touches its top, left or right edge (the roll wraps over the whole plane), and their windows are not contiguous
//     with the tile's, so each of the at most 194 halo values is computed by one thread directly from memory (bq_m_at), its
//     own 7 x 7 window zero-padded at its own position, through the same mscn_hpass and mscn_vpass as the march: equal bits.
//     The roll wraps; the filter pads.  Each thread adds its 25 quantities in row order; mscn_block_sum gives the tile's
//     partial, and reduce_partials sums the tiles.
// The half plane and the partials are context scratch (sr_ctx::brisque_ws), grown on demand.
#include <type_traits>

#include "sr_ctx.h"
#include "sr_device.h"
#include "sr_mscn.h"

namespace {

constexpr int BM_SEG = 4;                   // row segments of one tile of k_brisque_moments
constexpr int BM_T = BQ_TILE * BM_SEG;      // its threads

// the plane's integer at (y, x), 0 outside it (the filter's zero padding)
template <int SCALE, int PX>
__device__ __forceinline__ int bq_pixel(const void *__restrict__ src, long long stride, int Hs, int Ws, int y, int x)
{
    if (y < 0 || y >= Hs || x < 0 || x >= Ws) return 0;
    if constexpr (SCALE == 1)
        return (int)nq_luma<PX>((const unsigned char *)src + (size_t)y * (size_t)stride + (size_t)x * PX);
    else
        return ((const int *)src)[(size_t)y * (size_t)Ws + (size_t)x];
}

// m at one position of the plane, from memory: the march's own passes over a window zero-padded at this position
template <int SCALE, int PX>
__device__ double bq_m_at(const void *__restrict__ src, long long stride, int Hs, int Ws, int y, int x, const double *k)
{
    double wm[7], wq[7];
#pragma unroll PX == 3 ? 1 : 7     // with the luma on the fly the rolled loop is the faster one (profiles/mscn_share_timing.json)
    for (int j = 0; j < 7; ++j)
        mscn_hpass<SCALE>(k, [&](int i) { return bq_pixel<SCALE, PX>(src, stride, Hs, Ws, y - NQ_R + j, x - NQ_R + i); }, wm[j], wq[j]);
    double sigma;
    return mscn_vpass<SCALE>(k, wm, wq, bq_pixel<SCALE, PX>(src, stride, Hs, Ws, y, x), sigma);
}

// src: the image (SCALE 1, u8, stride in bytes) or the half plane (SCALE 2, int32, dense, Ws wide); Hs x Ws is the scale's
// plane, ntx its tiles per row; part: BQ_Q doubles per tile
template <int SCALE, int PX>
__global__ __launch_bounds__(BM_T) void k_brisque_moments(const void *__restrict__ src, long long stride, int Hs, int Ws, int ntx,
                                                          MscnWindow Kw, double *__restrict__ part)
{
    constexpr int B = BQ_TILE, T = B + 2 * NQ_R, RS = B / BM_SEG, NWAVE = BM_T / 64;
    static_assert(BM_T % 64 == 0 && B % BM_SEG == 0, "whole waves, whole segments");
    static_assert(3 * B + 2 <= BM_T, "one thread per halo value");
    using tile_t = std::conditional_t<SCALE == 1, unsigned char, int>;
    constexpr int TP = SCALE == 1 ? (T + 3) / 4 * 4 : T;                // a u8 row starts on a dword
    __shared__ __align__(8) tile_t I[T][TP];
    __shared__ double M[B + 1][B + 2];                                  // M[1 + r][1 + c] = m of tile position (r, c)
    // the waves' sums reuse the integer tile, dead after the march: with it three scale-2 workgroups fit a CU's 160 KB, not two
    static_assert(sizeof(double) * NWAVE * BQ_Q <= sizeof(tile_t) * T * TP, "the reduction fits the integer tile");
    double (*red)[BQ_Q] = reinterpret_cast<double (*)[BQ_Q]>(&I[0][0]);
    const int t = threadIdx.x;
    const int ty = (int)blockIdx.x / ntx, tx = (int)blockIdx.x - ty * ntx;
    const int r0p = ty * B, c0p = tx * B;                               // the tile's origin in the plane
    const int th = min(B, Hs - r0p), tw = min(B, Ws - c0p);             // its part inside the plane
    for (int e = t; e < T * T; e += BM_T) {
        const int r = e / T, c = e - r * T;
        I[r][c] = (tile_t)bq_pixel<SCALE, PX>(src, stride, Hs, Ws, r0p - NQ_R + r, c0p - NQ_R + c);
    }
    double k[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) k[i] = Kw.k[i];
    {   // the halo of m: the row above (tile columns -1 .. tw), the column to the left and the column to the right, wrapped
        const int yu = r0p == 0 ? Hs - 1 : r0p - 1, xl = c0p == 0 ? Ws - 1 : c0p - 1, xr = c0p + tw == Ws ? 0 : c0p + tw;
        int y = -1, x = -1, mr = 0, mc = 0;
        if (t < tw + 2) {
            const int j = t - 1;
            y = yu;
            x = j < 0 ? xl : (j == tw ? xr : c0p + j);
            mr = 0;
            mc = t;
        } else if (t < tw + 2 + th) {
            const int r = t - (tw + 2);
            y = r0p + r;
            x = xl;
            mr = 1 + r;
            mc = 0;
        } else if (t < tw + 2 + 2 * th) {
            const int r = t - (tw + 2 + th);
            y = r0p + r;
            x = xr;
            mr = 1 + r;
            mc = 1 + tw;
        }
        if (y >= 0) M[mr][mc] = bq_m_at<SCALE, PX>(src, stride, Hs, Ws, y, x, k);
    }
    __syncthreads();
    const int c = t % B, seg = t / B, r0 = seg * RS;
    mscn_march<SCALE, RS>(I, c, r0, k, [&](int r, double m, double) {
        if (r < th && c < tw) M[1 + r][1 + c] = m;                      // column 1 + tw is the halo's when tw < B
    });
    __syncthreads();
    // the five X of this thread's rows; roll(m, (dy, dx))[i, j] = m[(i - dy) mod Hs, (j - dx) mod Ws]
    double acc[BQ_Q];
#pragma unroll
    for (int i = 0; i < BQ_Q; ++i) acc[i] = 0.0;
    if (c < tw) {
        const int r1 = min(r0 + RS, th);
        for (int r = r0; r < r1; ++r) mscn_accumulate(acc, M[1 + r][1 + c], M[1 + r][c], M[r][1 + c], M[r][c], M[r][2 + c]);
    }
    const double v = mscn_block_sum<NWAVE, BQ_Q>(acc, red, t);
    if (t < BQ_Q) part[(size_t)blockIdx.x * BQ_Q + (size_t)t] = v;
}

}  // namespace

extern "C" {

int sr_brisque_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, int crop_border, sr_brisque_record *h_out)
{
    // every argument check comes before the context (and so the device) is touched
    if (!d_img || !h_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_brisque_u8: null argument");
    BqPlan p;
    int rc = bq_plan("sr_brisque_u8", h, w, cn, crop_border, &p);
    if (rc) return rc;
    if (stride < (int64_t)w * cn) return sr_set_error(SR_ERR_SHAPE, "sr_brisque_u8: stride smaller than a row");
    const long long hgy = ((long long)p.H2 + MH_H - 1) / MH_H;
    if (p.nt[0] > 0x7fffffffLL || hgy > 65535 || p.W > (1 << 30))       // the kernels form 2 W - 1 - x in 32 bits
        return sr_set_error(SR_ERR_SHAPE, "sr_brisque_u8: too many tiles for one launch (%d x %d)", p.W, p.H);
    CTX_ENTER(ctx);
    ctx->brisque_H2 = ctx->brisque_W2 = 0;                              // the scratch holds nothing valid until this call completes
    SRCHK(ctx->brisque_ws.reserve(ctx, "sr_brisque_u8", p.total));
    char *ws = ctx->brisque_ws.as<char>();
    int *half = (int *)(ws + p.off_half);
    double *part[2] = {(double *)(ws + p.off_part[0]), (double *)(ws + p.off_part[1])};
    MscnWindow Kw;
    nq_window(Kw.k);
    // the crop: rows [cb, cb + H), columns [cb, cb + W)
    const unsigned char *img = d_img + (size_t)crop_border * (size_t)stride + (size_t)crop_border * (size_t)cn;
    {
        ProfScope ps(ctx, "brisque_half");
        const dim3 grid((unsigned)((p.W2 + MH_W - 1) / MH_W), (unsigned)hgy);
        if (cn == 3) hipLaunchKernelGGL((k_mscn_half<3, true>), grid, dim3(MH_T), 0, ctx->stream, img, (long long)stride, p.H, p.W, p.H2, p.W2, half);
        else hipLaunchKernelGGL((k_mscn_half<1, true>), grid, dim3(MH_T), 0, ctx->stream, img, (long long)stride, p.H, p.W, p.H2, p.W2, half);
    }
    rc = check_launch("brisque_half");
    if (rc) return rc;
    const int ntx1 = (int)(((long long)p.W + BQ_TILE - 1) / BQ_TILE), ntx2 = (p.W2 + BQ_TILE - 1) / BQ_TILE;
    {
        ProfScope ps(ctx, "brisque_moments_1");
        const dim3 grid((unsigned)p.nt[0]);
        if (cn == 3)
            hipLaunchKernelGGL((k_brisque_moments<1, 3>), grid, dim3(BM_T), 0, ctx->stream, (const void *)img, (long long)stride, p.H, p.W,
                               ntx1, Kw, part[0]);
        else
            hipLaunchKernelGGL((k_brisque_moments<1, 1>), grid, dim3(BM_T), 0, ctx->stream, (const void *)img, (long long)stride, p.H, p.W,
                               ntx1, Kw, part[0]);
    }
    {
        ProfScope ps(ctx, "brisque_moments_2");
        hipLaunchKernelGGL((k_brisque_moments<2, 1>), dim3((unsigned)p.nt[1]), dim3(BM_T), 0, ctx->stream, (const void *)half, 0LL, p.H2,
                           p.W2, ntx2, Kw, part[1]);
    }
    rc = check_launch("brisque_moments");
    if (rc) return rc;
    double sums[2][BQ_Q];
    for (int s = 0; s < 2; ++s) {                                       // stream order keeps the second reduction behind the first copy
        ProfScope ps(ctx, "brisque_reduce");
        const double *res = reduce_partials(ctx, part[s], p.nt[s], BQ_Q, (double *)(ws + p.off_buf0), (double *)(ws + p.off_buf1));
        rc = check_launch("brisque_reduce");
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(sums[s], res, sizeof(sums[s]), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(stream_sync(ctx));
    for (int s = 0; s < 2; ++s) {
        h_out[s].n = s == 0 ? (uint64_t)p.H * (uint64_t)p.W : (uint64_t)p.H2 * (uint64_t)p.W2;
        for (int i = 0; i < 5; ++i) {
            const double *q = sums[s] + 5 * i;
            h_out[s].x[i] = {(uint64_t)q[0], (uint64_t)q[1], q[2], q[3], q[4]};
        }
    }
    ctx->brisque_H2 = p.H2;
    ctx->brisque_W2 = p.W2;
    return SR_OK;
}

int sr_brisque_half_plane(sr_ctx *ctx, int32_t *h_out)
{
    if (!h_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_brisque_half_plane: null argument");
    CTX_ENTER(ctx);
    return mscn_half_plane(ctx, "sr_brisque", ctx->brisque_ws.d, ctx->brisque_H2, ctx->brisque_W2, h_out);
}

}  // extern "C"
