// sr_brisque.hip -- the device side of BRISQUE (sr_brisque_u8, sr_brisque_half_plane): the exact half-resolution plane of any
// H x W >= 16 and, per scale, the moments of the MSCN coefficients and their four rolled products over the whole plane.  The
// definition is in include/sr_hip.h; the plan, the features and the score are host code (sr_brisque_host.cpp).
//   k_brisque_half<PX>  k_niqe_half's arithmetic (same taps, same integer passes) for a plane of any size: the grid covers
//     ceil(H / 2) x ceil(W / 2) outputs with partial blocks, every store is bounds-guarded and the pitch is W2.  Inputs of
//     outputs that do not exist are clamped into the plane after the reflection (they are read, never used).
//   k_brisque_moments<SCALE, PX>  A workgroup of 256 threads owns a 64 x 64 tile of m (the single-pass form: m is never
//     stored to memory).  The tile plus its 3-pixel halo goes into LDS as integers (u8 at scale 1 with the luma on the fly,
//     int32 at scale 2); a pixel outside the plane is 0 there, which is the filter's zero padding.  Thread (c, seg) owns column
//     c and 16 rows and marches down them with k_niqe_blocks' 7-row register window; m goes to a 65 x 66 float64 LDS tile
//     that also holds what the four shifts read beyond the tile: the row above and a column on each side.  Those m lie on the
//     far side of the plane when the tile touches its top, left or right edge (the roll wraps over the whole plane), and
//     their windows are not contiguous with the tile's, so each of the at most 194 halo values is computed by one thread
//     directly from memory, its own 7 x 7 window zero-padded at its own position, in the march's order of operations (equal
//     bits).  The roll wraps; the filter pads.  Each thread adds its 25 quantities in row order; a fixed tree (wave shuffles,
//     then the waves in ascending order) gives the tile's partial, and reduce_partials sums the tiles.
// The half plane and the partials are context scratch (sr_ctx::brisque_ws), grown on demand.
#include <type_traits>

#include "sr_ctx.h"
#include "sr_device.h"
#include "sr_niqe.h"

namespace {

constexpr int BH_H = 24, BH_W = 48;         // outputs of one k_brisque_half block
constexpr int BH_T = 256;
constexpr int BM_SEG = 4;                   // row segments of one tile of k_brisque_moments
constexpr int BM_T = BQ_TILE * BM_SEG;      // its threads

struct BqWindow {
    double k[2 * NQ_R + 1];
};

template <int PX>
__global__ __launch_bounds__(BH_T) void k_brisque_half(const unsigned char *__restrict__ img, long long stride, int H, int W,
                                                       int H2, int W2, int *__restrict__ out)
{
    constexpr int IH = 2 * BH_H + 6, IW = 2 * BH_W + 6;
    __shared__ unsigned short I[IH][IW];
    __shared__ int R[IH][BH_W];
    const int t = threadIdx.x;
    const int oy0 = (int)blockIdx.y * BH_H, ox0 = (int)blockIdx.x * BH_W;
    for (int e = t; e < IH * IW; e += BH_T) {
        const int r = e / IW, c = e - r * IW;
        int y = 2 * oy0 - 3 + r, x = 2 * ox0 - 3 + c;
        y = y < 0 ? -y - 1 : (y >= H ? 2 * H - 1 - y : y);
        x = x < 0 ? -x - 1 : (x >= W ? 2 * W - 1 - x : x);
        y = min(max(y, 0), H - 1);          // only inputs of outputs beyond H2 x W2 need it
        x = min(max(x, 0), W - 1);
        I[r][c] = (unsigned short)nq_luma<PX>(img + (size_t)y * (size_t)stride + (size_t)x * PX);
    }
    __syncthreads();
    for (int e = t; e < IH * BH_W; e += BH_T) {
        const int r = e / BH_W, c = e - r * BH_W;
        const unsigned short *p = &I[r][2 * c];
        R[r][c] = 111 * ((int)p[3] + (int)p[4]) + 29 * ((int)p[2] + (int)p[5]) - 9 * ((int)p[1] + (int)p[6]) - 3 * ((int)p[0] + (int)p[7]);
    }
    __syncthreads();
    for (int e = t; e < BH_H * BH_W; e += BH_T) {
        const int r = e / BH_W, c = e - r * BH_W;
        if (oy0 + r >= H2 || ox0 + c >= W2) continue;
        const int v = 111 * (R[2 * r + 3][c] + R[2 * r + 4][c]) + 29 * (R[2 * r + 2][c] + R[2 * r + 5][c]) -
                      9 * (R[2 * r + 1][c] + R[2 * r + 6][c]) - 3 * (R[2 * r][c] + R[2 * r + 7][c]);
        out[(size_t)(oy0 + r) * (size_t)W2 + (size_t)(ox0 + c)] = v;
    }
}

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

// m at one position of the plane, from memory: the march's operations in the march's order
template <int SCALE, int PX>
__device__ double bq_m_at(const void *__restrict__ src, long long stride, int Hs, int Ws, int y, int x, const double *k)
{
    constexpr double UNIT = SCALE == 1 ? 1.0 : 1.0 / 65536.0;
    double wm[7], wq[7];
    for (int j = 0; j < 7; ++j) {
        double v = (double)bq_pixel<SCALE, PX>(src, stride, Hs, Ws, y - NQ_R + j, x - NQ_R) * UNIT;
        double hm = k[0] * v, hq = k[0] * (v * v);
#pragma unroll
        for (int i = 1; i < 7; ++i) {
            v = (double)bq_pixel<SCALE, PX>(src, stride, Hs, Ws, y - NQ_R + j, x - NQ_R + i) * UNIT;
            hm += k[i] * v;
            hq += k[i] * (v * v);
        }
        wm[j] = hm;
        wq[j] = hq;
    }
    double mu = k[0] * wm[0], q = k[0] * wq[0];
    for (int j = 1; j < 7; ++j) {
        mu += k[j] * wm[j];
        q += k[j] * wq[j];
    }
    const double sigma = sqrt(fabs(q - mu * mu));
    const double v = (double)bq_pixel<SCALE, PX>(src, stride, Hs, Ws, y, x) * UNIT;
    return (v - mu) / (sigma + 1.0);
}

// one quantity summed over the wave in a fixed order
__device__ __forceinline__ double bq_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// src: the image (SCALE 1, u8, stride in bytes) or the half plane (SCALE 2, int32, dense, Ws wide); Hs x Ws is the scale's
// plane, ntx its tiles per row; part: BQ_Q doubles per tile
template <int SCALE, int PX>
__global__ __launch_bounds__(BM_T) void k_brisque_moments(const void *__restrict__ src, long long stride, int Hs, int Ws, int ntx,
                                                          BqWindow Kw, double *__restrict__ part)
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
    constexpr double UNIT = SCALE == 1 ? 1.0 : 1.0 / 65536.0;          // gray levels per integer of the tile
    double wm[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, wq[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int it = 0; it < RS + 2 * NQ_R; ++it) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            wm[j] = wm[j + 1];
            wq[j] = wq[j + 1];
        }
        {   // the horizontal pass of tile row r0 + it at this column: taps in ascending order
            const tile_t *p = &I[r0 + it][c];
            double v = (double)p[0] * UNIT;                             // exact, and so is v * v (|integer| < 2^25)
            double hm = k[0] * v, hq = k[0] * (v * v);
#pragma unroll
            for (int i = 1; i < 7; ++i) {
                v = (double)p[i] * UNIT;
                hm += k[i] * v;
                hq += k[i] * (v * v);
            }
            wm[6] = hm;
            wq[6] = hq;
        }
        if (it < 2 * NQ_R) continue;
        double mu = k[0] * wm[0], q = k[0] * wq[0];
#pragma unroll
        for (int j = 1; j < 7; ++j) {
            mu += k[j] * wm[j];
            q += k[j] * wq[j];
        }
        const double sigma = sqrt(fabs(q - mu * mu));
        const int r = r0 + it - 2 * NQ_R;                               // the tile row: I row r + 3
        const double v = (double)I[r + NQ_R][c + NQ_R] * UNIT;
        if (r < th && c < tw) M[1 + r][1 + c] = (v - mu) / (sigma + 1.0);   // column 1 + tw is the halo's when tw < B
    }
    __syncthreads();
    // the five X of this thread's rows; roll(m, (dy, dx))[i, j] = m[(i - dy) mod Hs, (j - dx) mod Ws]
    double acc[BQ_Q];
#pragma unroll
    for (int i = 0; i < BQ_Q; ++i) acc[i] = 0.0;
    if (c < tw) {
        const int r1 = min(r0 + RS, th);
        for (int r = r0; r < r1; ++r) {
            const double a = M[1 + r][1 + c];
            const double X[5] = {a, a * M[1 + r][c], a * M[r][1 + c], a * M[r][c], a * M[r][2 + c]};
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                const double x = X[s], xx = x * x;
                acc[5 * s + 0] += x < 0.0 ? 1.0 : 0.0;                  // counts stay exact integers in fp64
                acc[5 * s + 1] += x > 0.0 ? 1.0 : 0.0;
                acc[5 * s + 2] += x < 0.0 ? xx : 0.0;
                acc[5 * s + 3] += x > 0.0 ? xx : 0.0;
                acc[5 * s + 4] += fabs(x);
            }
        }
    }
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int i = 0; i < BQ_Q; ++i) {
        const double v = bq_wave_sum(acc[i]);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (t < BQ_Q) {
        double v = red[0][t];
        for (int w = 1; w < NWAVE; ++w) v += red[w][t];
        part[(size_t)blockIdx.x * BQ_Q + (size_t)t] = v;
    }
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
    const long long hgy = ((long long)p.H2 + BH_H - 1) / BH_H;
    if (p.nt[0] > 0x7fffffffLL || hgy > 65535 || p.W > (1 << 30))       // the kernels form 2 W - 1 - x in 32 bits
        return sr_set_error(SR_ERR_SHAPE, "sr_brisque_u8: too many tiles for one launch (%d x %d)", p.W, p.H);
    CTX_ENTER(ctx);
    ctx->brisque_H2 = ctx->brisque_W2 = 0;                              // the scratch holds nothing valid until this call completes
    SRCHK(ctx->brisque_ws.reserve(ctx, "sr_brisque_u8", p.total));
    char *ws = ctx->brisque_ws.as<char>();
    int *half = (int *)(ws + p.off_half);
    double *part[2] = {(double *)(ws + p.off_part[0]), (double *)(ws + p.off_part[1])};
    BqWindow Kw;
    nq_window(Kw.k);
    // the crop: rows [cb, cb + H), columns [cb, cb + W)
    const unsigned char *img = d_img + (size_t)crop_border * (size_t)stride + (size_t)crop_border * (size_t)cn;
    {
        ProfScope ps(ctx, "brisque_half");
        const dim3 grid((unsigned)((p.W2 + BH_W - 1) / BH_W), (unsigned)hgy);
        if (cn == 3) hipLaunchKernelGGL((k_brisque_half<3>), grid, dim3(BH_T), 0, ctx->stream, img, (long long)stride, p.H, p.W, p.H2, p.W2, half);
        else hipLaunchKernelGGL((k_brisque_half<1>), grid, dim3(BH_T), 0, ctx->stream, img, (long long)stride, p.H, p.W, p.H2, p.W2, half);
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
    if (ctx->brisque_H2 < 1)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_brisque_half_plane: no sr_brisque_u8 call has completed on this context");
    const size_t n = (size_t)ctx->brisque_H2 * (size_t)ctx->brisque_W2;
    HIPCHK(hipMemcpyAsync(h_out, ctx->brisque_ws.d, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // extern "C"
