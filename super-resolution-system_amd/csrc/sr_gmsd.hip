// sr_gmsd.hip -- the gradient magnitude similarity deviation of two u8 images (sr_gmsd_u8), the authors' GMSD.m.  The
// definition is in include/sr_hip.h; sizes, the launch, the scratch layout and every shape refusal are sr_vif_host.cpp's
// (gmsd_plan).
//
// One kernel, one launch, one pass over both images.  Everything up to the gradient magnitude is an exact integer:
//   the plane      the gray value, MATLAB's rounded luma, or X = 65481 R + 128553 G + 24966 B + 4080000 (= 255000 Y, < 2^26)
//   S              the 2 x 2 sum of the plane at (2i, 2j), zero beyond the last row and column (4 avg; < 2^28)
//   Sx, Sy         the Prewitt sums of S with a zero border (12 Ix, 12 Iy; < 2^30 in magnitude)
//   Sx^2 + Sy^2    < 2^61, a 64-bit integer: m^2 = (Sx^2 + Sy^2) / (144 scale^2) rounds in the conversion (Y mode only: the
//                  integer can pass 2^53) and in the division.
// k_gmsd<MODE, PX>  a block owns GMSD_TH x GMSD_TW samples of the half-size map: it forms S of both images for its samples and
//   a border of one into LDS (pixels are read byte by byte: the crop is pointer arithmetic and has any residue), then each
//   thread takes 4 samples, d = (m1 - m2)^2 / (m1^2 + m2^2 + 170), and the block adds d and d^2 through a fixed tree.
// The per-block partials go through reduce_partials: no floating-point atomics, equal inputs give equal bits.
#include <cmath>
#include <cstring>

#include "sr_ctx.h"
#include "sr_device.h"
#include "sr_vif.h"

namespace {

constexpr int GM_SW = GMSD_TW + 2, GM_SH = GMSD_TH + 2;
constexpr double GM_C = 170.0;
enum { GM_PLANE = 0, GM_YROUND = 1, GM_Y = 2 };

template <int MODE>
__device__ __forceinline__ int gm_load(const unsigned char *__restrict__ p)
{
    if constexpr (MODE == GM_PLANE) return p[0];
    const unsigned x = 65481u * p[0] + 128553u * p[1] + 24966u * p[2] + 4080000u;    // <= 59 925 000
    if constexpr (MODE == GM_YROUND) return (int)((2u * x + 255000u) / 510000u);
    return (int)x;
}

// Sx^2 + Sy^2 of the sample whose border-of-one neighbourhood starts at S[li][lj]
__device__ __forceinline__ double gm_mag2(const int (*S)[GM_SW], int li, int lj)
{
    const long long sx = (long long)(S[li][lj] - S[li][lj + 2]) + (long long)(S[li + 1][lj] - S[li + 1][lj + 2]) +
                         (long long)(S[li + 2][lj] - S[li + 2][lj + 2]);
    const long long sy = (long long)(S[li][lj] - S[li + 2][lj]) + (long long)(S[li][lj + 1] - S[li + 2][lj + 1]) +
                         (long long)(S[li][lj + 2] - S[li + 2][lj + 2]);
    return (double)(unsigned long long)(sx * sx + sy * sy);
}

template <int MODE, int PX>
__global__ __launch_bounds__(GMSD_THREADS) void k_gmsd(const unsigned char *__restrict__ a, long long sa,
                                                       const unsigned char *__restrict__ b, long long sb, int h, int w, int h2,
                                                       int w2, int tiles_x, double unit2, double *__restrict__ part)
{
    __shared__ int S[2][GM_SH][GM_SW];
    __shared__ double R[2][GMSD_THREADS];
    const int t = threadIdx.x;
    const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x);
    const int i0 = ty * GMSD_TH, j0 = tx * GMSD_TW;
    for (int idx = t; idx < GM_SH * GM_SW; idx += GMSD_THREADS) {
        const int li = idx / GM_SW, lj = idx - li * GM_SW;
        const int i = i0 - 1 + li, j = j0 - 1 + lj;
        int s1 = 0, s2 = 0;
        if (i >= 0 && i < h2 && j >= 0 && j < w2) {
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const int r = 2 * i + dy;
                if (r >= h) continue;
                const unsigned char *ra = a + (size_t)r * (size_t)sa, *rb = b + (size_t)r * (size_t)sb;
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int c = 2 * j + dx;
                    if (c >= w) continue;
                    s1 += gm_load<MODE>(ra + (size_t)c * PX);
                    s2 += gm_load<MODE>(rb + (size_t)c * PX);
                }
            }
        }
        S[0][li][lj] = s1;
        S[1][li][lj] = s2;
    }
    __syncthreads();
    double sd = 0.0, sd2 = 0.0;
    const int lj = t % GMSD_TW;
#pragma unroll
    for (int k = 0; k < GMSD_TH * GMSD_TW / GMSD_THREADS; ++k) {
        const int li = t / GMSD_TW + k * (GMSD_THREADS / GMSD_TW);
        if (i0 + li >= h2 || j0 + lj >= w2) continue;
        const double q1 = gm_mag2(S[0], li, lj) / unit2, q2 = gm_mag2(S[1], li, lj) / unit2;     // m1^2, m2^2
        const double dm = sqrt(q1) - sqrt(q2);
        const double d = (dm * dm) / ((q1 + q2) + GM_C);
        sd += d;
        sd2 += d * d;
    }
    R[0][t] = sd;
    R[1][t] = sd2;
    __syncthreads();
    for (int s = GMSD_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            R[0][t] += R[0][t + s];
            R[1][t] += R[1][t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        part[(size_t)blockIdx.x * 2] = R[0][0];
        part[(size_t)blockIdx.x * 2 + 1] = R[1][0];
    }
}

}  // namespace

extern "C" int sr_gmsd_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                          int cn, int crop_border, int mode, sr_gmsd_sums *h_out)
{
    // every argument check comes before the context (and so the device) is touched
    if (!d_a || !d_b || !h_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_gmsd_u8: null argument");
    GmsdPlan p;
    int rc = gmsd_plan("sr_gmsd_u8", h, w, cn, crop_border, mode, &p);
    if (rc) return rc;
    const int64_t min_stride = (int64_t)w * cn;
    if (stride_a < min_stride || stride_b < min_stride) return sr_set_error(SR_ERR_SHAPE, "sr_gmsd_u8: stride smaller than a row");
    CTX_ENTER(ctx);
    SRCHK(ctx->gmsd_ws.reserve(ctx, "sr_gmsd_u8", p.total));
    char *ws = ctx->gmsd_ws.as<char>();
    double *part = (double *)(ws + p.off_part), *buf0 = (double *)(ws + p.off_buf0), *buf1 = (double *)(ws + p.off_buf1);
    const unsigned char *a = d_a + (size_t)crop_border * (size_t)stride_a + (size_t)crop_border * (size_t)cn;
    const unsigned char *b = d_b + (size_t)crop_border * (size_t)stride_b + (size_t)crop_border * (size_t)cn;
    const long long tiles = (long long)p.tiles_x * p.tiles_y;
    const dim3 grid((unsigned)tiles), block(GMSD_THREADS);
    // m^2 = (Sx^2 + Sy^2) / unit2: 12^2 for the two means, and the luma's scale squared (exact: < 2^53)
    const double unit2 = mode == SR_BENCH_Y ? 144.0 * 255000.0 * 255000.0 : 144.0;
    double h_res[2];
    {
        ProfScope ps(ctx, "gmsd");
        if (mode == SR_BENCH_Y)
            hipLaunchKernelGGL((k_gmsd<GM_Y, 3>), grid, block, 0, ctx->stream, a, (long long)stride_a, b, (long long)stride_b, p.ch, p.cw,
                               p.h2, p.w2, p.tiles_x, unit2, part);
        else if (mode == SR_BENCH_Y_ROUND)
            hipLaunchKernelGGL((k_gmsd<GM_YROUND, 3>), grid, block, 0, ctx->stream, a, (long long)stride_a, b, (long long)stride_b, p.ch,
                               p.cw, p.h2, p.w2, p.tiles_x, unit2, part);
        else
            hipLaunchKernelGGL((k_gmsd<GM_PLANE, 1>), grid, block, 0, ctx->stream, a, (long long)stride_a, b, (long long)stride_b, p.ch,
                               p.cw, p.h2, p.w2, p.tiles_x, unit2, part);
        const double *sums = reduce_partials(ctx, part, tiles, 2, buf0, buf1);
        rc = check_launch("gmsd");
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(h_res, sums, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(stream_sync(ctx));
    h_out->sum_d = h_res[0];
    h_out->sum_d2 = h_res[1];
    h_out->count = p.count;
    return SR_OK;
}
