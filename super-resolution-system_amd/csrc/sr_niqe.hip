// sr_niqe.hip -- the device side of NIQE (sr_niqe_u8, sr_niqe_half_plane): the exact half-resolution plane and the per-block
// moment records of the MSCN coefficients at both scales.  The definition is in include/sr_hip.h; the plan, the features, the
// fit and the score are host code (sr_niqe_host.cpp).
// The MSCN core is sr_mscn.h's, shared with BRISQUE (sr_brisque.hip): the half-plane kernel, the two passes of the window, the
// register-window march, the 25 quantities of a position and the block sum.  This unit holds what is NIQE's own.
//   k_mscn_half<PX, false>  The exact half plane of the kept plane (sides multiples of 96: whole blocks, no guard).
//   k_niqe_blocks<SCALE, PX>  One workgroup per block at both scales, B = 96 / SCALE on a side, 8 B threads: thread (c, seg)
//     owns column c and the B / 8 rows of segment seg.  The block plus its 3-pixel halo goes into LDS as integers (u8 at scale
//     1, read from the image with the luma on the fly; int32 at scale 2; the halo replicates at the plane's edge and is the
//     neighbouring blocks' pixels inside).  Each thread marches down its rows (mscn_march); m goes to a B x B float64 LDS
//     tile (72 KB at scale 1) and sigma into the thread's sum.  After one barrier each thread forms its rows' four rolled
//     products from the m tile (the roll wraps inside the block) and adds the 26 quantities in row order; mscn_block_sum
//     gives the record, stored in its typed slots.  No atomics, no second pass over the image.
// The half plane and the records are context scratch (sr_ctx::niqe_ws), grown on demand.
#include <cstring>
#include <type_traits>

#include "sr_ctx.h"
#include "sr_device.h"
#include "sr_mscn.h"
#include "sr_ssim11.h"

namespace {

constexpr int NB_SEG = 8;                   // row segments of one block of k_niqe_blocks
constexpr int NB_Q = 26;                    // quantities of a record

static_assert(sizeof(sr_niqe_block) == NB_Q * 8, "a record is 26 eight-byte slots");

// src: the image (SCALE 1, u8, stride in bytes) or the half plane (SCALE 2, int32, dense, Ws wide); Hs x Ws is the scale's plane
template <int SCALE, int PX>
__global__ __launch_bounds__(NQ_BLOCK / SCALE * NB_SEG) void k_niqe_blocks(const void *__restrict__ src, long long stride, int Hs,
                                                                            int Ws, int nbx, MscnWindow Kw,
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
    double k[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) k[i] = Kw.k[i];
    double sum_sigma = 0.0;
    mscn_march<SCALE, RS>(I, c, r0, k, [&](int r, double m, double sigma) {
        M[r][c] = m;
        sum_sigma += sigma;
    });
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
        mscn_accumulate(acc, M[r][c], M[r][cl], M[rp][c], M[rp][cl], M[rp][cr]);
    }
    const double v = mscn_block_sum<NWAVE, NB_Q>(acc, red, t);
    if (t < NB_Q) {
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
    MscnWindow Kw;
    nq_window(Kw.k);
    // the crop: rows [cb, cb + H), columns [cb, cb + W)
    const unsigned char *img = d_img + (size_t)crop_border * (size_t)stride + (size_t)crop_border * (size_t)cn;
    const long long nblocks = (long long)p.nby * p.nbx;
    if (nblocks > 0x7fffffffLL || 2 * p.nby > 65535) return sr_set_error(SR_ERR_SHAPE, "sr_niqe_u8: too many blocks (%d x %d)", p.nby, p.nbx);
    {
        ProfScope ps(ctx, "niqe_half");
        const dim3 grid((unsigned)p.nbx, (unsigned)(2 * p.nby));        // (W / 2) / MH_W by (H / 2) / MH_H
        if (cn == 3) hipLaunchKernelGGL((k_mscn_half<3, false>), grid, dim3(MH_T), 0, ctx->stream, img, (long long)stride, p.H, p.W, p.H / 2, p.W / 2, half);
        else hipLaunchKernelGGL((k_mscn_half<1, false>), grid, dim3(MH_T), 0, ctx->stream, img, (long long)stride, p.H, p.W, p.H / 2, p.W / 2, half);
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
    return mscn_half_plane(ctx, "sr_niqe", ctx->niqe_ws.d, ctx->niqe_H / 2, ctx->niqe_W / 2, h_out);
}

}  // extern "C"
