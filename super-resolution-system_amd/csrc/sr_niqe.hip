// sr_niqe.hip -- the device side of NIQE (sr_niqe_u8, sr_niqe_half_plane): the exact half-resolution plane and the per-block
// moment records of the MSCN coefficients at both scales.  The definition is in include/sr_hip.h; the plan, the features, the
// fit and the score are host code (sr_niqe_host.cpp).
//   k_niqe_half<PX>  A block owns NH_H x NH_W outputs.  It reads its (2 NH_H + 6) x (2 NH_W + 6) inputs once (luma on the fly
//     for PX = 3, indices reflected at the plane's edge) into LDS, runs the 8-tap pass along the rows into a second LDS tile
//     and along the columns out of it, and writes int32 = 65536 x the result.  Integer arithmetic only: taps {-3, -9, 29, 111,
//     111, 29, -9, -3}, |row pass| <= 255 * 304, |result| <= 255 * 304^2 < 2^25.
//   k_niqe_blocks<SCALE, PX>  One workgroup per block at both scales, B = 96 / SCALE on a side, 8 B threads: thread (c, seg)
//     owns column c and the B / 8 rows of segment seg.  The block plus its 3-pixel halo goes into LDS as integers (u8 at scale
//     1, read from the image with the luma on the fly; int32 at scale 2; the halo replicates at the plane's edge and is the
//     neighbouring blocks' pixels inside).  Each thread marches down its rows: the horizontal pass of one tile row (I and I^2,
//     taps added in ascending order) enters a 7-row register window, the vertical pass over the window gives mu and sigma, and
//     m goes to a B x B float64 LDS tile (72 KB at scale 1).  A segment recomputes the 6 window rows above it, so no
//     horizontal-pass row is ever stored.  After one barrier each thread forms its rows' four rolled products from the m
//     tile (the roll wraps inside the block) and adds the 26 quantities in row order; a fixed tree (wave shuffles, then the
//     waves in ascending order) gives the record.  No atomics, no second pass over the image.
// The half plane and the records are context scratch (sr_ctx::niqe_ws), grown on demand.
#include <cstring>
#include <type_traits>

#include "sr_ctx.h"
#include "sr_device.h"
#include "sr_niqe.h"
#include "sr_ssim11.h"

namespace {

constexpr int NH_H = 24, NH_W = 48;         // outputs of one k_niqe_half block: both divide 48
constexpr int NH_T = 256;
constexpr int NB_SEG = 8;                   // row segments of one block of k_niqe_blocks
constexpr int NB_Q = 26;                    // quantities of a record

static_assert(sizeof(sr_niqe_block) == NB_Q * 8, "a record is 26 eight-byte slots");

struct NqWindow {
    double k[2 * NQ_R + 1];
};

template <int PX>
__global__ __launch_bounds__(NH_T) void k_niqe_half(const unsigned char *__restrict__ img, long long stride, int H, int W,
                                                    int *__restrict__ out)
{
    constexpr int IH = 2 * NH_H + 6, IW = 2 * NH_W + 6;
    __shared__ unsigned short I[IH][IW];
    __shared__ int R[IH][NH_W];
    const int t = threadIdx.x;
    const int oy0 = (int)blockIdx.y * NH_H, ox0 = (int)blockIdx.x * NH_W;
    for (int e = t; e < IH * IW; e += NH_T) {
        const int r = e / IW, c = e - r * IW;
        int y = 2 * oy0 - 3 + r, x = 2 * ox0 - 3 + c;
        y = y < 0 ? -y - 1 : (y >= H ? 2 * H - 1 - y : y);
        x = x < 0 ? -x - 1 : (x >= W ? 2 * W - 1 - x : x);
        I[r][c] = (unsigned short)nq_luma<PX>(img + (size_t)y * (size_t)stride + (size_t)x * PX);
    }
    __syncthreads();
    for (int e = t; e < IH * NH_W; e += NH_T) {
        const int r = e / NH_W, c = e - r * NH_W;
        const unsigned short *p = &I[r][2 * c];
        R[r][c] = 111 * ((int)p[3] + (int)p[4]) + 29 * ((int)p[2] + (int)p[5]) - 9 * ((int)p[1] + (int)p[6]) - 3 * ((int)p[0] + (int)p[7]);
    }
    __syncthreads();
    const size_t ow = (size_t)(W / 2);
    for (int e = t; e < NH_H * NH_W; e += NH_T) {
        const int r = e / NH_W, c = e - r * NH_W;
        const int v = 111 * (R[2 * r + 3][c] + R[2 * r + 4][c]) + 29 * (R[2 * r + 2][c] + R[2 * r + 5][c]) -
                      9 * (R[2 * r + 1][c] + R[2 * r + 6][c]) - 3 * (R[2 * r][c] + R[2 * r + 7][c]);
        out[(size_t)(oy0 + r) * ow + (size_t)(ox0 + c)] = v;
    }
}

// one quantity summed over the block in a fixed order: down the wave, then the waves in ascending order
__device__ __forceinline__ double nq_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// src: the image (SCALE 1, u8, stride in bytes) or the half plane (SCALE 2, int32, dense, Ws wide); Hs x Ws is the scale's plane
template <int SCALE, int PX>
__global__ __launch_bounds__(NQ_BLOCK / SCALE * NB_SEG) void k_niqe_blocks(const void *__restrict__ src, long long stride, int Hs,
                                                                            int Ws, int nbx, NqWindow Kw,
                                                                            sr_niqe_block *__restrict__ rec)
{
    constexpr int B = NQ_BLOCK / SCALE, T = B + 2 * NQ_R, RS = B / NB_SEG, NT = B * NB_SEG, NWAVE = NT / 64;
    static_assert(NT % 64 == 0 && B % NB_SEG == 0, "whole waves, whole segments");
    using tile_t = std::conditional_t<SCALE == 1, unsigned char, int>;
    constexpr int TP = SCALE == 1 ? (T + 3) / 4 * 4 : T;                // a u8 row starts on a dword
    __shared__ tile_t I[T][TP];
    __shared__ double M[B][B];
    __shared__ double red[NWAVE][NB_Q];
    const int t = threadIdx.x;
    const int by = (int)blockIdx.x / nbx, bx = (int)blockIdx.x - by * nbx;
    const int y0 = by * B - NQ_R, x0 = bx * B - NQ_R;
    for (int e = t; e < T * T; e += NT) {
        const int r = e / T, c = e - r * T;
        const int y = min(max(y0 + r, 0), Hs - 1), x = min(max(x0 + c, 0), Ws - 1);
        if constexpr (SCALE == 1)
            I[r][c] = (unsigned char)nq_luma<PX>((const unsigned char *)src + (size_t)y * (size_t)stride + (size_t)x * PX);
        else
            I[r][c] = ((const int *)src)[(size_t)y * (size_t)Ws + (size_t)x];
    }
    __syncthreads();
    const int c = t % B, seg = t / B, r0 = seg * RS;
    constexpr double UNIT = SCALE == 1 ? 1.0 : 1.0 / 65536.0;          // gray levels per integer of the tile
    double k[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) k[i] = Kw.k[i];
    double wm[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, wq[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double sum_sigma = 0.0;
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
        const int r = r0 + it - 2 * NQ_R;                               // the block row: tile row r + 3
        const double v = (double)I[r + NQ_R][c + NQ_R] * UNIT;
        M[r][c] = (v - mu) / (sigma + 1.0);
        sum_sigma += sigma;
    }
    __syncthreads();
    // the five X of this thread's rows; roll(m, (dy, dx))[i, j] = m[(i - dy) mod B, (j - dx) mod B]
    double acc[NB_Q];
#pragma unroll
    for (int i = 0; i < NB_Q; ++i) acc[i] = 0.0;
    acc[NB_Q - 1] = sum_sigma;
    const int cl = c == 0 ? B - 1 : c - 1, cr = c == B - 1 ? 0 : c + 1;
#pragma unroll 2
    for (int r = r0; r < r0 + RS; ++r) {
        const int rp = r == 0 ? B - 1 : r - 1;
        const double a = M[r][c];
        const double X[5] = {a, a * M[r][cl], a * M[rp][c], a * M[rp][cl], a * M[rp][cr]};
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const double x = X[s], xx = x * x;
            acc[5 * s + 0] += x < 0.0 ? 1.0 : 0.0;                      // counts stay exact integers in fp64
            acc[5 * s + 1] += x > 0.0 ? 1.0 : 0.0;
            acc[5 * s + 2] += x < 0.0 ? xx : 0.0;
            acc[5 * s + 3] += x > 0.0 ? xx : 0.0;
            acc[5 * s + 4] += fabs(x);
        }
    }
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int i = 0; i < NB_Q; ++i) {
        const double v = nq_wave_sum(acc[i]);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (t < NB_Q) {
        double v = red[0][t];
        for (int w = 1; w < NWAVE; ++w) v += red[w][t];
        void *slot = (char *)(rec + blockIdx.x) + (size_t)t * 8;
        const int field = t % 5;
        if (t < NB_Q - 1 && field < 2) *(unsigned long long *)slot = (unsigned long long)v;
        else *(double *)slot = v;
    }
}

}  // namespace

extern "C" {

int sr_niqe_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, int crop_border, sr_niqe_block *h_out)
{
    // every argument check comes before the context (and so the device) is touched
    if (!d_img || !h_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_niqe_u8: null argument");
    NqPlan p;
    int rc = nq_plan("sr_niqe_u8", h, w, cn, crop_border, &p);
    if (rc) return rc;
    if (stride < (int64_t)w * cn) return sr_set_error(SR_ERR_SHAPE, "sr_niqe_u8: stride smaller than a row");
    CTX_ENTER(ctx);
    ctx->niqe_H = ctx->niqe_W = 0;                                      // the scratch holds nothing valid until this call completes
    SRCHK(ctx->niqe_ws.reserve(ctx, "sr_niqe_u8", p.total));
    char *ws = ctx->niqe_ws.as<char>();
    int *half = (int *)(ws + p.off_half);
    sr_niqe_block *rec = (sr_niqe_block *)(ws + p.off_rec);
    NqWindow Kw;
    nq_window(Kw.k);
    // the crop: rows [cb, cb + H), columns [cb, cb + W)
    const unsigned char *img = d_img + (size_t)crop_border * (size_t)stride + (size_t)crop_border * (size_t)cn;
    const long long nblocks = (long long)p.nby * p.nbx;
    if (nblocks > 0x7fffffffLL || 2 * p.nby > 65535) return sr_set_error(SR_ERR_SHAPE, "sr_niqe_u8: too many blocks (%d x %d)", p.nby, p.nbx);
    {
        ProfScope ps(ctx, "niqe_half");
        const dim3 grid((unsigned)p.nbx, (unsigned)(2 * p.nby));        // (W / 2) / NH_W by (H / 2) / NH_H
        if (cn == 3) hipLaunchKernelGGL((k_niqe_half<3>), grid, dim3(NH_T), 0, ctx->stream, img, (long long)stride, p.H, p.W, half);
        else hipLaunchKernelGGL((k_niqe_half<1>), grid, dim3(NH_T), 0, ctx->stream, img, (long long)stride, p.H, p.W, half);
    }
    rc = check_launch("niqe_half");
    if (rc) return rc;
    {
        ProfScope ps(ctx, "niqe_blocks");
        const dim3 grid((unsigned)nblocks);
        if (cn == 3)
            hipLaunchKernelGGL((k_niqe_blocks<1, 3>), grid, dim3(NQ_BLOCK * NB_SEG), 0, ctx->stream, (const void *)img, (long long)stride,
                               p.H, p.W, p.nbx, Kw, rec);
        else
            hipLaunchKernelGGL((k_niqe_blocks<1, 1>), grid, dim3(NQ_BLOCK * NB_SEG), 0, ctx->stream, (const void *)img, (long long)stride,
                               p.H, p.W, p.nbx, Kw, rec);
        hipLaunchKernelGGL((k_niqe_blocks<2, 1>), grid, dim3(NQ_BLOCK / 2 * NB_SEG), 0, ctx->stream, (const void *)half, 0LL, p.H / 2,
                           p.W / 2, p.nbx, Kw, rec + nblocks);
    }
    rc = check_launch("niqe_blocks");
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h_out, rec, (size_t)(2 * nblocks) * sizeof(sr_niqe_block), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    ctx->niqe_H = p.H;
    ctx->niqe_W = p.W;
    return SR_OK;
}

int sr_niqe_half_plane(sr_ctx *ctx, int32_t *h_out)
{
    if (!h_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_niqe_half_plane: null argument");
    CTX_ENTER(ctx);
    if (ctx->niqe_H < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_niqe_half_plane: no sr_niqe_u8 call has completed on this context");
    const size_t n = (size_t)(ctx->niqe_H / 2) * (size_t)(ctx->niqe_W / 2);
    HIPCHK(hipMemcpyAsync(h_out, ctx->niqe_ws.d, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // extern "C"
