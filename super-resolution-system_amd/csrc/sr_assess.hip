// sr_assess.hip -- the quality-assessment stage on gfx950: squared error (PSNR), the SSIM variants, RGB -> gray and
// cv2.resize(INTER_CUBIC) with the resized assessment built on it.
//
// Restates quality_assessment_module.py:277-417 (PSNR / SSIM through skimage and cv2) and :226-253,518-555 (the
// bicubic down-sample comparison).  Holds
//   * k_sse_flat / k_sse_rows / k_sse_f32                    sr_sse_u8[_async], sr_sse_f32
//   * k_rgb2gray                                             sr_rgb2gray_u8
//   * k_assess_march, k_assess_finish / k_assess_store       sr_assess_u8[_async], sr_ssim_u8[_async], sr_ssim_count
//   * k_ssimf_gray / k_ssimf_rows / k_ssimf_cols             sr_ssim_float
//   * k_resize_cubic / _rgb4 / _up_rgb, cubic_table          sr_resize_cubic_u8, sr_resize_cubic_window_u8
//   * k_resize_gray_pair / _lds / _march, k_store_sse        sr_assess_resized_u8[_async]
//   * k_reduce_partials and reduce_partials (declared in sr_ctx.h: the quality maps and the metric files call it).
// It uses the context (sr_ctx.h) and the device helpers of sr_device.h; nothing of the blend plan or its arena.
//
// Numerics contract: integer sums are exact, and every fp32 expression is evaluated in the order written in
// oracle/sr_oracle.c (build with -ffp-contract=off).  Between sr_engine.hip and this file fp64 is used only here, in the
// SSIM kernels and the partial sums, where the reference computes in float64 (in sr_tiles.hip the seam scan finishes a
// window's score, and the feather merge forms its ramp weights, in fp64).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <vector>

#include "sr_ctx.h"
#include "sr_device.h"
#include "sr_ssim11.h"

// ---------------------------------------------------------------------------------------------
// metrics
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// contiguous fast path: both buffers dense and 16-byte aligned
__global__ __launch_bounds__(256) void k_sse_flat(const uint4 *__restrict__ a, const uint4 *__restrict__ b,
                                                  size_t nvec, const unsigned char *__restrict__ ta,
                                                  const unsigned char *__restrict__ tb, int ntail,
                                                  unsigned long long *__restrict__ out)
{
    unsigned long long s = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        const uint4 va = a[i], vb = b[i];
        const unsigned int wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
        unsigned int p = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = (int)((wa[k] >> (8 * j)) & 0xFF) - (int)((wb[k] >> (8 * j)) & 0xFF);
                p += (unsigned int)(d * d);
            }
        s += p;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < ntail) {
        const int d = (int)ta[threadIdx.x] - (int)tb[threadIdx.x];
        s += (unsigned int)(d * d);
    }
    s = wave_sum_u64(s);
    __shared__ unsigned long long ws[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) ws[wid] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, ws[0] + ws[1] + ws[2] + ws[3]);
}

// strided path (cropped / non-dense images): one block row-chunk, byte loads
__global__ __launch_bounds__(256) void k_sse_rows(const unsigned char *__restrict__ a, long long sa,
                                                  const unsigned char *__restrict__ b, long long sb, int h,
                                                  long long rowlen, unsigned long long *__restrict__ out)
{
    unsigned long long s = 0;
    for (int y = blockIdx.y; y < h; y += gridDim.y) {
        const unsigned char *pa = a + (size_t)y * sa, *pb = b + (size_t)y * sb;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < rowlen;
             i += (long long)gridDim.x * blockDim.x) {
            const int d = (int)pa[i] - (int)pb[i];
            s += (unsigned int)(d * d);
        }
    }
    s = wave_sum_u64(s);
    __shared__ unsigned long long ws[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) ws[wid] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, ws[0] + ws[1] + ws[2] + ws[3]);
}

// squared differences of two fp32 images (skimage's PSNR on float input: fp32 difference and square, fp64 mean)
__global__ __launch_bounds__(256) void k_sse_f32(const float *__restrict__ a, long long sa, const float *__restrict__ b,
                                                 long long sb, int h, long long rowlen, double *__restrict__ part)
{
    double s = 0.0;
    for (int y = blockIdx.y; y < h; y += gridDim.y) {
        const float *pa = (const float *)((const char *)a + (size_t)y * sa);
        const float *pb = (const float *)((const char *)b + (size_t)y * sb);
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < rowlen; i += (long long)gridDim.x * blockDim.x) {
            const float d = pa[i] - pb[i];
            s += (double)(d * d);
        }
    }
    s = wave_sum_f64(s);
    __shared__ double ws[4];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

__device__ __forceinline__ int gray_of(const unsigned char *__restrict__ p, int cn, int shift)
{
    if (cn == 1) return p[0];
    const int r = p[0], g = p[1], b = p[2];
    return shift == 15 ? (r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15
                       : (r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14;
}

__global__ __launch_bounds__(256) void k_rgb2gray(const unsigned char *__restrict__ rgb, long long stride, int h,
                                                  int w, int shift, unsigned char *__restrict__ gray,
                                                  long long gstride)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    gray[(size_t)y * gstride + x] = (unsigned char)gray_of(rgb + (size_t)y * stride + (size_t)x * 3, 3, shift);
}

// ---------------------------------------------------------------------------------------------
// Fused assessment (k_assess_march below): one pass over both u8 images (6 B / pixel) for
//   * the sum of squared differences (PSNR),
//   * the Gaussian-11 SSIM map summed over the cropped (valid) region -> "gauss"  (branch A) and over the full
//     frame with REFLECT_101 borders -> "simple" (branch B): scipy's gaussian_filter(sigma 1.5, truncate 3.5) and
//     cv2.GaussianBlur((11,11), 1.5) are the same normalised kernel, the variants differ only in border and crop,
//   * the uniform 7x7 SSIM map, entirely in integers (window sums are exact), fp64 only for the final formula.
// fp64 throughout where the reference is (float64); the row pass works on exact integers: gray values, x^2 + y^2
// and x*y are ints, symmetric taps are pair-summed as ints and only 6 products per map are formed.  4 filtered maps
// (x, y, x^2 + y^2, x*y) replace the reference's 5: SSIM needs uxx and uyy only as their sum.
// ---------------------------------------------------------------------------------------------
// cv2.resize INTER_CUBIC, u8: per destination index the first source tap and four 11-bit fixed-point coefficients
struct CubicTab {
    int ofs;
    short c[4];
};

enum { ASSESS_SSE = 1, ASSESS_UNIFORM = 2, ASSESS_GAUSS = 4, ASSESS_SIMPLE = 8, ASSESS_ALL_BITS = 15 };

struct AssessParams {
    int h, w, shift, ry0, ry1, flags, same_c;
    int nch, ty;       // chunks of 11 rows a block marches, and the rows it produces (11 nch - 10)
    double c1a, c2a;   // constants for data_range (uniform / gauss)
    double c1b, c2b;   // constants for 255 (simple)
    double k1u, k2u;   // 49^2 c1a and 48*49 c2a: the uniform-7 variant in integer-scaled form
    double k[6];       // k[0] centre tap, k[j] the +-j taps
};

template <int CN>
__device__ __forceinline__ void load_gray_pair(const unsigned char *__restrict__ a, long long sa,
                                               const unsigned char *__restrict__ b, long long sb, int sy, int sx,
                                               int shift, int &ga, int &gb, unsigned &sq)
{
    const unsigned char *pa = a + (size_t)sy * sa + (size_t)sx * CN;
    const unsigned char *pb = b + (size_t)sy * sb + (size_t)sx * CN;
    gray_pair<CN>(pa, pb, shift, ga, gb, sq);
}


// 1 / d to full double precision without the IEEE division sequence (d is a product of positive SSIM terms)
__device__ __forceinline__ double fast_recip(double d)
{
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    r = fma(fma(-d, r, 1.0), r, r);
    return r;
}

__device__ __forceinline__ double ssim_value(double ux, double uy, double spq, double dpq, double c1, double c2)
{
    // spq = uxx + uyy,  dpq = uxy
    const double uxuy = ux * uy, uu = ux * ux + uy * uy;
    const double a1 = 2.0 * uxuy + c1, a2 = 2.0 * (dpq - uxuy) + c2;
    const double b1 = uu + c1, b2 = (spq - uu) + c2;
    return (a1 * a2) * fast_recip(b1 * b2);
}

// ---------------------------------------------------------------------------------------------
// k_assess_march: all four metrics in ONE pass, column-marching.  A block is 256 columns wide (768 B of RGB per
// row: whole cache lines, ~4 % column halo) and walks down P.ty + 10 rows in chunks of 11.  Per chunk the block
// converts 11 rows of both images to gray once per pixel and leaves, per pixel, three dwords in LDS: x | y << 16,
// x*y and x^2 + y^2 (so no thread ever recomputes a neighbour's products, and one packed add pair-sums x and y
// together).  Then each thread owns one column: the row pass of its column (integer pair sums, 6 fp64 products per
// map) goes into an 11-deep register FIFO, the column pass reads the FIFO with static indices (the chunk loop body
// is the 11 unrolled rows), so the filtered maps never touch LDS.  The FIFO and the 7x7 window sums carry over
// from chunk to chunk: the only recomputed halo is the 10 rows at the top of a block (8 %).  The uniform-7 variant
// rides along: its per-row 7-tap integer sums go through a 7-slot per-column ring in LDS.
// ---------------------------------------------------------------------------------------------
#ifndef AM_TX
#define AM_TX 256                        /* columns (= threads) per block */
#endif
#define AM_R 5
#define AM_GP (AM_TX + 16)              /* row pitch in pixels: 10 halo columns, rounded up to groups of 4 */
#define AM_CH 11                        /* rows per chunk == FIFO depth */
#define AM_NCH_MAX 12                   /* chunks per block: P.nch <= 12, chosen per launch (rows / tail effect) */
/* a block marches 11 * nch rows and produces P.ty = 11 * nch - 10 of them; LDS 36 KB + 14 KB ring + 2 KB -> 3 blocks per CU */


// cv2.resize(INTER_CUBIC) sample of one destination pixel (all channels) -- the arithmetic of k_resize_cubic
template <int CN>
__device__ __forceinline__ void cubic_sample(const unsigned char *__restrict__ src, long long sstride, int sh, int sw,
                                             const CubicTab X, const CubicTab Y, int (&out)[CN])
{
    // 32-bit accumulators suffice: the cubic's taps (a = -0.75) have sum |c| <= 1.375, i.e. <= 2817 in 1/2048 units per
    // axis, so |acc| <= 255 * 2817^2 = 2.02e9 < 2^31 -- also after the rounding constant
    int acc[CN];
#pragma unroll
    for (int c = 0; c < CN; ++c) acc[c] = 0;
    const bool inner = X.ofs - 1 >= 0 && X.ofs + 2 <= sw - 1;
    const short yc[4] = {Y.c[0], Y.c[1], Y.c[2], Y.c[3]};
#pragma unroll 2
    for (int ky = 0; ky < 4; ++ky) {
        const unsigned char *r = src + (size_t)min(max(Y.ofs + ky - 1, 0), sh - 1) * sstride;
        int v[4][CN];
        if (inner && CN == 3) {
            const u3_t q = ld_u3_a1(r + (size_t)(X.ofs - 1) * 3);
            const unsigned wd[3] = {q.x, q.y, q.z};
#pragma unroll
            for (int b = 0; b < 12; ++b) v[b / 3][b % 3] = (int)((wd[b >> 2] >> (8 * (b & 3))) & 0xFFu);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int sx = min(max(X.ofs + k - 1, 0), sw - 1) * CN;
#pragma unroll
                for (int c = 0; c < CN; ++c) v[k][c] = (int)r[sx + c];
            }
        }
#pragma unroll
        for (int c = 0; c < CN; ++c) {
            const int hs = v[0][c] * X.c[0] + v[1][c] * X.c[1] + v[2][c] * X.c[2] + v[3][c] * X.c[3];
            acc[c] += hs * (int)yc[ky];
        }
    }
#pragma unroll
    for (int c = 0; c < CN; ++c) {
        const int t = (acc[c] + (1 << 21)) >> 22;
        out[c] = t < 0 ? 0 : (t > 255 ? 255 : t);
    }
}

// gray conversion + per-pixel products of 4-pixel groups of chunk `ch` into LDS; returns this thread's share of the
// squared differences of the block's own pixels
template <int CN>
__device__ __forceinline__ unsigned assess_load_chunk(const unsigned char *__restrict__ a, long long sa,
                                                      const unsigned char *__restrict__ b, long long sb,
                                                      const AssessParams &P, int bx0, int by0, int ch,
                                                      int rows_needed, unsigned (*XY)[AM_GP],
                                                      unsigned (*QQ)[AM_GP], unsigned (*PP)[AM_GP])
{
    // a thread squares at most 12 chunks x 3 groups x 4 pixels x 3 channels = 432 differences per block (< 2.9e7): 32 bits
    unsigned sse = 0;
    const bool want_sse = (P.flags & ASSESS_SSE) != 0;
    for (int i = threadIdx.x; i < AM_CH * (AM_GP / 4); i += AM_TX) {
        const int ly = i / (AM_GP / 4), lx = (i - ly * (AM_GP / 4)) * 4;
        const int lr = ch * AM_CH + ly;
        if (lr >= rows_needed) break;                       // rows grow with i
        const int gy = by0 - AM_R + lr, gx = bx0 - AM_R + lx;
        const int sy = reflect101(gy, P.h);
        int ga[4], gb[4];
        unsigned sq[4];
        if (gx >= 0 && gx + 3 < P.w) {
            const unsigned char *pa = a + (size_t)sy * sa + (size_t)gx * CN;
            const unsigned char *pb = b + (size_t)sy * sb + (size_t)gx * CN;
            if (CN == 3) {
                const u3_t qa = ld_u3_a1(pa), qb = ld_u3_a1(pb);
                const unsigned wa[3] = {qa.x, qa.y, qa.z}, wb[3] = {qb.x, qb.y, qb.z};
                int ca[12], cb[12];
#pragma unroll
                for (int t = 0; t < 12; ++t) {
                    ca[t] = (int)((wa[t >> 2] >> (8 * (t & 3))) & 0xFFu);
                    cb[t] = (int)((wb[t >> 2] >> (8 * (t & 3))) & 0xFFu);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    ga[k] = gray_rgb(ca[3 * k], ca[3 * k + 1], ca[3 * k + 2], P.shift);
                    gb[k] = gray_rgb(cb[3 * k], cb[3 * k + 1], cb[3 * k + 2], P.shift);
                    const int dr = ca[3 * k] - cb[3 * k], dg = ca[3 * k + 1] - cb[3 * k + 1], db = ca[3 * k + 2] - cb[3 * k + 2];
                    sq[k] = (unsigned)(dr * dr + dg * dg + db * db);
                }
            } else {
                const unsigned qa = *(const u1_a1_t *)pa, qb = *(const u1_a1_t *)pb;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    ga[k] = (int)((qa >> (8 * k)) & 0xFFu);
                    gb[k] = (int)((qb >> (8 * k)) & 0xFFu);
                    const int d = ga[k] - gb[k];
                    sq[k] = (unsigned)(d * d);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) load_gray_pair<CN>(a, sa, b, sb, sy, reflect101(gx + k, P.w), P.shift, ga[k], gb[k], sq[k]);
        }
        u4_t vxy, vq, vp;
        unsigned txy[4], tq[4], tp[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            txy[k] = (unsigned)ga[k] | ((unsigned)gb[k] << 14);
            tq[k] = (unsigned)__mul24(ga[k], gb[k]);
            tp[k] = (unsigned)(__mul24(ga[k], ga[k]) + __mul24(gb[k], gb[k]));
        }
        vxy.x = txy[0]; vxy.y = txy[1]; vxy.z = txy[2]; vxy.w = txy[3];
        vq.x = tq[0]; vq.y = tq[1]; vq.z = tq[2]; vq.w = tq[3];
        vp.x = tp[0]; vp.y = tp[1]; vp.z = tp[2]; vp.w = tp[3];
        *(u4_t *)&XY[ly][lx] = vxy;
        *(u4_t *)&QQ[ly][lx] = vq;
        *(u4_t *)&PP[ly][lx] = vp;
        if (want_sse && lr >= AM_R && lr < AM_R + P.ty && gy < P.ry1 && gy < P.h) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (lx + k >= AM_R && lx + k < AM_R + AM_TX && gx + k < P.w) sse += sq[k];
        }
    }
    return sse;
}

// An address the compiler cannot fold into its users: the eleven taps of a row are then read with ds_read2_b32 off ONE
// base register per array and row (the 8-bit dword offsets of ds_read2 do not reach across rows, and left alone the
// compiler materialises five bases per array and row with VALU adds).
typedef __attribute__((address_space(3))) const unsigned lds_cu32;
__device__ __forceinline__ lds_cu32 *lds_row_base(lds_cu32 *row0, int bytes)
{
    // one explicit VALU add per array and row off the thread's row-0 address: no per-row base registers kept alive
    lds_cu32 *q;
    asm volatile("v_add_u32 %0, %2, %1" : "=v"(q) : "v"(row0), "n"(bytes));     // literal goes in src0
    return q;
}

// Compile-time variants: GAUSS (the two Gaussian-11 sums and their 88-register FIFO), UNIF (the uniform-7 sum and its LDS
// ring), SAMEC (data_range == 255: the cropped and the full-frame Gaussian variants share one SSIM value per pixel).
// What the march does per row, in instruction terms: 33 LDS dwords, 15 integer pair sums, 24 conversions + 24 fp64
// multiply-adds (row pass), 20 fp64 adds + 24 multiply-adds (column pass), ~20 fp64 operations per SSIM value; validity of
// a ROW is block-uniform (scalar branches), validity of a COLUMN is applied once, to the thread's sums, after the march
// (out-of-image columns hold reflected data, so their values are finite and simply dropped).
// In LDS x and y travel packed as x | y << 14: pair sums (<= 510), 7-tap sums (<= 1785) and 49-sample window sums
// (<= 12495 < 2^14) all stay inside their fields, so one integer add serves both images at every stage.
template <int CN, bool GAUSS, bool UNIF, bool SAMEC>
__global__ __launch_bounds__(AM_TX, 3) void k_assess_march(const unsigned char *__restrict__ a, long long sa,
                                                      const unsigned char *__restrict__ b, long long sb,
                                                      AssessParams P, double *__restrict__ part)
{
    // one array, so the march addresses all three maps off ONE per-thread base register
    __shared__ __attribute__((aligned(16))) unsigned L3[3][AM_CH][AM_GP];
    unsigned (*XY)[AM_GP] = L3[0];                                       // x | y << 14
    unsigned (*QQ)[AM_GP] = L3[1];                                       // x * y
    unsigned (*PP)[AM_GP] = L3[2];                                       // x^2 + y^2
    // per-row 7-tap sums of the last seven rows, two dwords per column: {sx:14 | sy:11 @14 | sq lo:7 @25}, {sp:20 | sq hi:12 @20}
    __shared__ unsigned U[UNIF ? 7 : 1][2][AM_TX];
    __shared__ double red[AM_TX / 64][4];
    const int c = threadIdx.x;
    const int bx0 = blockIdx.x * AM_TX, by0 = P.ry0 + blockIdx.y * P.ty;
    const int rows_needed = min(P.ty, P.ry1 - by0) + 2 * AM_R;          // block-uniform
    const int mx = bx0 + c;
    double f[GAUSS ? 4 : 1][11];
    if (GAUSS) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int i = 0; i < 11; ++i) f[m][i] = 0.0;
    }
    unsigned t_xy = 0, t_p = 0, t_q = 0;                                // 49-sample window sums (uniform-7)
    double sum_int = 0.0, sum_all = 0.0, sum_u = 0.0;
    unsigned sse = 0;                                                   // this thread's squared differences (fits: see the loader)
    int slot = 0;                                                       // row index mod 7
    const double k0 = P.k[0], k1 = P.k[1], k2 = P.k[2], k3 = P.k[3], k4 = P.k[4], k5 = P.k[5];
    lds_cu32 *xy0 = (lds_cu32 *)&L3[0][0][c];
    constexpr int MAPB = AM_CH * AM_GP * 4;                             // bytes between the maps
    // full-frame samples of the 5 top / bottom image rows: touched only by the first and last block rows, so the running
    // sum lives in LDS (2 KB) instead of two registers of every thread of every block
    __shared__ double EDGE[(GAUSS && SAMEC) ? AM_TX : 1];
    if (GAUSS && SAMEC) EDGE[c] = 0.0;                                  // own slot only: no barrier needed
#pragma unroll 1
    for (int ch = 0; ch < P.nch; ++ch) {
        if (ch * AM_CH >= rows_needed) break;
        __syncthreads();                                                // the previous chunk has been read
        sse += assess_load_chunk<CN>(a, sa, b, sb, P, bx0, by0, ch, rows_needed, XY, QQ, PP);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < AM_CH; ++s) {
            const int r = ch * AM_CH + s;
            if (r >= rows_needed) continue;                             // block-uniform (no break: the loop must unroll)
            lds_cu32 *rxy = lds_row_base(xy0, s * AM_GP * 4), *rq = lds_row_base(xy0, MAPB + s * AM_GP * 4),
                     *rp = lds_row_base(xy0, 2 * MAPB + s * AM_GP * 4);
            unsigned xy[11], qv[11], pv[11];
#pragma unroll
            for (int j = 0; j < 11; ++j) {
                xy[j] = rxy[j];
                qv[j] = rq[j];
                pv[j] = rp[j];
            }
            // symmetric pair sums, shared by the Gaussian row pass (all five) and the 7-tap box sums (the first three)
            unsigned sxy[6], sp[6], sq[6];
            sxy[0] = xy[5]; sp[0] = pv[5]; sq[0] = qv[5];
#pragma unroll
            for (int j = 1; j <= (GAUSS ? AM_R : 3); ++j) {
                sxy[j] = xy[5 - j] + xy[5 + j];                         // both images in one add
                sp[j] = pv[5 - j] + pv[5 + j];
                sq[j] = qv[5 - j] + qv[5 + j];
            }
            if (GAUSS) {
                const double kk[6] = {k0, k1, k2, k3, k4, k5};
                double hx = (double)(sxy[0] & 0x3FFFu) * kk[0], hy = (double)(sxy[0] >> 14) * kk[0];
                double hp = (double)sp[0] * kk[0], hq = (double)sq[0] * kk[0];
#pragma unroll
                for (int j = 1; j <= AM_R; ++j) {
                    hx = fma((double)(sxy[j] & 0x3FFFu), kk[j], hx);
                    hy = fma((double)(sxy[j] >> 14), kk[j], hy);
                    hp = fma((double)sp[j], kk[j], hp);
                    hq = fma((double)sq[j], kk[j], hq);
                }
                f[0][s] = hx; f[1][s] = hy; f[2][s] = hp; f[3][s] = hq;
            }
            if (UNIF) {
                const unsigned uxy = ((sxy[0] + sxy[1]) + sxy[2]) + sxy[3];
                const unsigned up = ((sp[0] + sp[1]) + sp[2]) + sp[3];
                const unsigned uq = ((sq[0] + sq[1]) + sq[2]) + sq[3];
                if (r >= 7) {                                           // block-uniform: the slot holds row r - 7
                    const unsigned o0 = U[slot][0][c], o1 = U[slot][1][c];
                    t_xy -= o0 & 0x1FFFFFFu;
                    t_p -= o1 & 0xFFFFFu;
                    t_q -= (o0 >> 25) | ((o1 >> 20) << 7);
                }
                t_xy += uxy; t_p += up; t_q += uq;
                U[slot][0][c] = uxy | (uq << 25);
                U[slot][1][c] = up | ((uq >> 7) << 20);
                slot = slot == 6 ? 0 : slot + 1;
                const int orow = r - 8, my = by0 + orow;                // window rows r-6 .. r, centre r-3
                if (orow >= 0 && orow < P.ty && my < P.ry1 && my >= 3 && my < P.h - 3) {        // block-uniform
                    // SSIM of the 49-sample window with both fractions scaled to integers: with S. the window sums,
                    //   (2 ux uy + C1) / (ux^2 + uy^2 + C1) = (2 Sx Sy + 49^2 C1) / (Sx^2 + Sy^2 + 49^2 C1)
                    //   (2 cov + C2) / (var_x + var_y + C2) = (2 (49 Sxy - Sx Sy) + 48*49 C2)
                    //                                         / (49 (Sxx + Syy) - (Sx^2 + Sy^2) + 48*49 C2)
                    // (sample covariance, N - 1 = 48).  Everything left of the constants is exact 32-bit integer
                    // arithmetic (|values| < 3.2e8, every factor below 2^24); fp64 enters with the constants.
                    const int sx = (int)(t_xy & 0x3FFFu), sy = (int)(t_xy >> 14);
                    const int sxsy = __mul24(sx, sy), ss = __mul24(sx, sx) + __mul24(sy, sy);
                    const int ncov = __mul24(49, (int)t_q) - sxsy, nvar = __mul24(49, (int)t_p) - ss;
                    const double a1 = fma(2.0, (double)sxsy, P.k1u), a2 = fma(2.0, (double)ncov, P.k2u);
                    const double b1 = (double)ss + P.k1u, b2 = (double)nvar + P.k2u;
                    sum_u += (a1 * a2) * ssim_recip(b1 * b2);
                }
            }
            if (GAUSS && r >= 2 * AM_R) {
                const int orow = r - 2 * AM_R, my = by0 + orow;         // rows r-10 .. r are in the FIFO, centre r-5
                if (orow < P.ty && my < P.ry1 && my < P.h) {            // block-uniform
                    const double kk[6] = {k0, k1, k2, k3, k4, k5};
                    double u[4];
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        double acc = f[m][(s + 6) % 11] * kk[0];
#pragma unroll
                        for (int j = 1; j <= AM_R; ++j)
                            acc = fma(f[m][(s + 6 + 11 - j) % 11] + f[m][(s + 6 + j) % 11], kk[j], acc);
                        u[m] = acc;
                    }
                    const bool inner_row = my >= AM_R && my < P.h - AM_R;       // block-uniform
                    if (SAMEC) {
                        // one SSIM value serves both variants: the cropped sum is the full-frame sum minus the (at most
                        // ten) image rows outside the crop, which only the blocks at the top / bottom ever see
                        const double sv = ssim_quot(u[0], u[1], u[2], u[3], P.c1a, P.c2a);
                        sum_all += sv;
                        if (!inner_row) EDGE[c] += sv;
                    } else {
                        if (P.flags & ASSESS_SIMPLE) sum_all += ssim_quot(u[0], u[1], u[2], u[3], P.c1b, P.c2b);
                        if (inner_row && (P.flags & ASSESS_GAUSS)) sum_int += ssim_quot(u[0], u[1], u[2], u[3], P.c1a, P.c2a);
                    }
                }
            }
        }
    }
    // column validity, once: the full-frame variant counts every image column, the cropped ones lose 5 / 3 per side
    if (GAUSS && SAMEC) sum_int = sum_all - EDGE[c];
    if (!(mx < P.w)) sum_all = 0.0;
    if (!(mx >= AM_R && mx < P.w - AM_R)) sum_int = 0.0;
    if (!(mx >= 3 && mx < P.w - 3)) sum_u = 0.0;
    sum_int = wave_sum_f64(sum_int);
    sum_all = wave_sum_f64(sum_all);
    sum_u = wave_sum_f64(sum_u);
    const double dsse = wave_sum_f64((double)sse);
    if ((c & 63) == 0) {
        red[c >> 6][0] = sum_int;
        red[c >> 6][1] = sum_all;
        red[c >> 6][2] = dsse;
        red[c >> 6][3] = sum_u;
    }
    __syncthreads();
    if (c < 4) {
        const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        double t = red[0][c];
#pragma unroll
        for (int wv = 1; wv < AM_TX / 64; ++wv) t += red[wv][c];
        part[blk * 4 + c] = t;
    }
}

// Deterministic two-level sum of per-block partials laid out as part[i * ncomp + comp]:
// level 1: block j sums entries [j*1024, (j+1)*1024) in a fixed tree -> tmp[j * ncomp + comp];
// level 2 (one block): sums the level-1 results -> out[comp].
__global__ __launch_bounds__(256) void k_reduce_partials(const double *__restrict__ part, long long n, int ncomp,
                                                         double *__restrict__ out)
{
    __shared__ double sh[256];
    const long long base = (long long)blockIdx.x * 1024;
    for (int comp = 0; comp < ncomp; ++comp) {
        double s = 0.0;
        for (int k = 0; k < 4; ++k) {
            const long long i = base + k * 256 + threadIdx.x;
            if (i < n) s += part[i * ncomp + comp];
        }
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[(size_t)blockIdx.x * ncomp + comp] = sh[0];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// cv2.resize INTER_CUBIC, u8
// ---------------------------------------------------------------------------------------------

// RGB form: one thread = 4 consecutive destination pixels of a row (one row-table entry, 12 bytes stored as 3 dwords)
__global__ __launch_bounds__(256) void k_resize_cubic_rgb4(const unsigned char *__restrict__ src, long long sstride, int h,
                                                           int w, const CubicTab *__restrict__ xt,
                                                           const CubicTab *__restrict__ yt, int x0, int y0, int ww,
                                                           int wh, unsigned char *__restrict__ dst, long long dstride)
{
    const int x = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= ww || y >= wh) return;
    const CubicTab Y = yt[y0 + y];
    const int nx = min(4, ww - x);
    unsigned ob[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int v[3] = {0, 0, 0};
        if (k < nx) cubic_sample<3>(src, sstride, h, w, xt[x0 + x + k], Y, v);
        ob[3 * k] = (unsigned)v[0]; ob[3 * k + 1] = (unsigned)v[1]; ob[3 * k + 2] = (unsigned)v[2];
    }
    unsigned char *o = dst + (size_t)y * dstride + (size_t)x * 3;
    if (nx == 4 && ((((size_t)o) & 3) == 0)) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
            ((unsigned *)o)[q] = ob[4 * q] | (ob[4 * q + 1] << 8) | (ob[4 * q + 2] << 16) | (ob[4 * q + 3] << 24);
    } else {
        for (int k = 0; k < nx; ++k) {
            o[3 * k] = (unsigned char)ob[3 * k]; o[3 * k + 1] = (unsigned char)ob[3 * k + 1]; o[3 * k + 2] = (unsigned char)ob[3 * k + 2];
        }
    }
}

// Upscaling form (destination rows >= source rows): consecutive destination rows read the same four source rows, so the
// horizontal pass is not repeated per destination row.  One thread owns 4 destination columns and marches down a segment of
// destination rows; it keeps the horizontal results of the four source rows of the current row window (4 x 4 x 3 ints) and
// computes ONE new source row when the window moves on (every dst_h / src_h rows); per destination row only the vertical
// pass remains (48 multiply-adds instead of 192 + 48 and sixteen 12-byte loads).  Same integers as cubic_sample:
// hs = sum v * xc, acc = sum hs * yc, (acc + 2^21) >> 22, clamped.
#define RUP_SEG 64
__device__ __forceinline__ void rup_row_pass(const unsigned char *__restrict__ src, long long sstride, int sh, int sw, int row,
                                             const CubicTab (&X)[4], int (&H)[4][3])
{
    const unsigned char *r = src + (size_t)min(max(row, 0), sh - 1) * sstride;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int v[4][3];
        if (X[k].ofs - 1 >= 0 && X[k].ofs + 2 <= sw - 1) {
            const u3_t q = ld_u3_a1(r + (size_t)(X[k].ofs - 1) * 3);
            const unsigned wd[3] = {q.x, q.y, q.z};
#pragma unroll
            for (int b = 0; b < 12; ++b) v[b / 3][b % 3] = (int)((wd[b >> 2] >> (8 * (b & 3))) & 0xFFu);
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int sx = min(max(X[k].ofs + t - 1, 0), sw - 1) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[t][c] = (int)r[sx + c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) H[k][c] = v[0][c] * X[k].c[0] + v[1][c] * X[k].c[1] + v[2][c] * X[k].c[2] + v[3][c] * X[k].c[3];
    }
}

__global__ __launch_bounds__(256, 2) void k_resize_cubic_up_rgb(const unsigned char *__restrict__ src, long long sstride, int sh,
                                                             int sw, const CubicTab *__restrict__ xt,
                                                             const CubicTab *__restrict__ yt, int x0, int y0, int ww, int wh,
                                                             unsigned char *__restrict__ dst, long long dstride)
{
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int ya = blockIdx.y * RUP_SEG, yb = min(ya + RUP_SEG, wh);
    if (x >= ww || ya >= yb) return;
    const int nx = min(4, ww - x);
    CubicTab X[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) X[k] = xt[x0 + min(x + k, ww - 1)];        // columns past the window repeat the last one, not stored
    // Source row r of the window lives in slot r & 3 (no copying when the window moves: the new row overwrites the slot of
    // the row that left); the vertical taps are matched to the slots instead -- the row window is the same for the whole
    // block, so that is scalar work.
    int H[4][4][3];                                                       // [slot][pixel][channel]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) H[j][k][c] = 0;
    int cur = yt[y0 + ya].ofs - 4;                                        // the window is filled by the step that advances it
#pragma unroll 1
    for (int y = ya; y < yb; ++y) {
        const CubicTab Y = yt[y0 + y];
#pragma unroll 1
        while (cur < Y.ofs) {                                             // the row window moves down by one source row
            ++cur;
            const int row = cur + 2;                                      // rows cur - 1 .. cur + 2 are held
            switch (row & 3) {
            case 0: rup_row_pass(src, sstride, sh, sw, row, X, H[0]); break;
            case 1: rup_row_pass(src, sstride, sh, sw, row, X, H[1]); break;
            case 2: rup_row_pass(src, sstride, sh, sw, row, X, H[2]); break;
            default: rup_row_pass(src, sstride, sh, sw, row, X, H[3]); break;
            }
        }
        // tap t belongs to row cur - 1 + t, which sits in slot (cur - 1 + t) & 3: rotate the taps onto the slots
        const int c0 = Y.c[0], c1 = Y.c[1], c2 = Y.c[2], c3 = Y.c[3];
        int yc[4];
        switch ((cur - 1) & 3) {
        case 0: yc[0] = c0; yc[1] = c1; yc[2] = c2; yc[3] = c3; break;
        case 1: yc[0] = c3; yc[1] = c0; yc[2] = c1; yc[3] = c2; break;
        case 2: yc[0] = c2; yc[1] = c3; yc[2] = c0; yc[3] = c1; break;
        default: yc[0] = c1; yc[1] = c2; yc[2] = c3; yc[3] = c0; break;
        }
        unsigned ob[12];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // the reference adds the four products in tap order; integer addition is exact, so the slot order gives the same sum
                const int acc = (H[0][k][c] * yc[0] + H[1][k][c] * yc[1]) + (H[2][k][c] * yc[2] + H[3][k][c] * yc[3]);
                const int t = (acc + (1 << 21)) >> 22;
                ob[3 * k + c] = (unsigned)(t < 0 ? 0 : (t > 255 ? 255 : t));
            }
        unsigned char *o = dst + (size_t)y * dstride + (size_t)x * 3;
        if (nx == 4 && ((((size_t)o) & 3) == 0)) {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                ((unsigned *)o)[q] = ob[4 * q] | (ob[4 * q + 1] << 8) | (ob[4 * q + 2] << 16) | (ob[4 * q + 3] << 24);
        } else {
            for (int k = 0; k < nx; ++k) {
                o[3 * k] = (unsigned char)ob[3 * k]; o[3 * k + 1] = (unsigned char)ob[3 * k + 1]; o[3 * k + 2] = (unsigned char)ob[3 * k + 2];
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_resize_cubic(const unsigned char *__restrict__ src, long long sstride,
                                                      int h, int w, int cn, const CubicTab *__restrict__ xt,
                                                      const CubicTab *__restrict__ yt, int x0, int y0, int ww,
                                                      int wh, unsigned char *__restrict__ dst, long long dstride)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= ww || y >= wh) return;
    const CubicTab X = xt[x0 + x], Y = yt[y0 + y];
    if (cn == 3 || cn == 1) {                    // one 12-byte load per tap row instead of 12 byte loads (cubic_sample)
        unsigned char *o = dst + (size_t)y * dstride + (size_t)x * cn;
        if (cn == 3) {
            int v[3];
            cubic_sample<3>(src, sstride, h, w, X, Y, v);
            o[0] = (unsigned char)v[0]; o[1] = (unsigned char)v[1]; o[2] = (unsigned char)v[2];
        } else {
            int v[1];
            cubic_sample<1>(src, sstride, h, w, X, Y, v);
            o[0] = (unsigned char)v[0];
        }
        return;
    }
    int sx[4], sy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sx[k] = min(max(X.ofs + k - 1, 0), w - 1) * cn;
        sy[k] = min(max(Y.ofs + k - 1, 0), h - 1);
    }
    for (int c = 0; c < cn; ++c) {
        long long acc = 0;
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
            const unsigned char *r = src + (size_t)sy[ky] * sstride + c;
            const int hs = (int)r[sx[0]] * X.c[0] + (int)r[sx[1]] * X.c[1] + (int)r[sx[2]] * X.c[2] +
                           (int)r[sx[3]] * X.c[3];
            acc += (long long)hs * Y.c[ky];
        }
        const long long v = (acc + (1 << 21)) >> 22;
        dst[(size_t)y * dstride + (size_t)x * cn + c] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}

static void cubic_table(int n_src, int n_dst, std::vector<CubicTab> &tab)
{
    tab.resize(n_dst);
    const double scale = 1.0 / ((double)n_dst / (double)n_src);
    for (int d = 0; d < n_dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        const int s = (int)floorf(f);
        f -= (float)s;
        const float A = -0.75f;
        float c[4];
        c[0] = ((A * (f + 1.0f) - 5.0f * A) * (f + 1.0f) + 8.0f * A) * (f + 1.0f) - 4.0f * A;
        c[1] = ((A + 2.0f) * f - (A + 3.0f)) * f * f + 1.0f;
        const float f2 = 1.0f - f;
        c[2] = ((A + 2.0f) * f2 - (A + 3.0f)) * f2 * f2 + 1.0f;
        c[3] = 1.0f - c[0] - c[1] - c[2];
        tab[d].ofs = s;
        for (int k = 0; k < 4; ++k) {
            const float v = rintf(c[k] * 2048.0f);
            tab[d].c[k] = (short)(v < -32768.f ? -32768.f : (v > 32767.f ? 32767.f : v));
        }
    }
}

// ---- fused assessment ---------------------------------------------------------------------------------------

// Stage 1 of the resized assessment: one thread = 4 consecutive pixels of the RESIZED images; cv2.resize(INTER_CUBIC) sample of
// both images (cubic_sample: the arithmetic of k_resize_cubic), gray of each, the squared channel differences.  Writes the
// two gray planes and one SSE partial per block (exact: integers, < 2^53).
template <int CN>
__global__ __launch_bounds__(256) void k_resize_gray_pair(const unsigned char *__restrict__ a, long long sa,
                                                          const unsigned char *__restrict__ b, long long sb, int sh, int sw,
                                                          const CubicTab *__restrict__ xt, const CubicTab *__restrict__ yt, int dh,
                                                          int dw, int shift, unsigned char *__restrict__ ga,
                                                          unsigned char *__restrict__ gb, long long pitch, double *__restrict__ part)
{
    __shared__ double ws[4];
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
    unsigned sse = 0, pa = 0, pb = 0;
    if (y < dh && x0 < dw) {
        const CubicTab Y = yt[y];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = min(x0 + k, dw - 1);              // columns past the end repeat the last one and are not counted
            int va[CN], vb[CN];
            cubic_sample<CN>(a, sa, sh, sw, xt[x], Y, va);
            cubic_sample<CN>(b, sb, sh, sw, xt[x], Y, vb);
            const int g0 = CN == 3 ? gray_rgb(va[0], va[1], va[2], shift) : va[0];
            const int g1 = CN == 3 ? gray_rgb(vb[0], vb[1], vb[2], shift) : vb[0];
            pa |= (unsigned)g0 << (8 * k);
            pb |= (unsigned)g1 << (8 * k);
            if (x0 + k < dw) {
#pragma unroll
                for (int c = 0; c < CN; ++c) sse += (unsigned)((va[c] - vb[c]) * (va[c] - vb[c]));
            }
        }
        *(unsigned *)(ga + (size_t)y * pitch + x0) = pa;    // pitch is a multiple of 64: the row padding takes the tail
        *(unsigned *)(gb + (size_t)y * pitch + x0) = pb;
    }
    const double s = wave_sum_f64((double)sse);
    const int tid = threadIdx.y * 64 + threadIdx.x;
    if ((tid & 63) == 0) ws[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// Down-sampling form of stage 1 (RGB, destination smaller than the source): the 4 x 4 taps of neighbouring destination pixels
// lie 1 / scale pixels apart, so the gather above issues 12-byte loads that share no cache line between lanes (TA-bound:
// 1.59 ms for the three scales of a 200 MP pair against 0.45 ms of HBM traffic).  Here a block of 64 x 4 destination pixels
// first copies the source window it needs -- the 4 source rows of each of its 4 destination rows, from the first to the last
// tap column, both images -- into LDS with coalesced 16-byte loads, and the taps are read from LDS.  Same integers as
// cubic_sample.  Launched when the window fits 64 KB of LDS (scales down to about 0.1).
__device__ __forceinline__ void lds_tap12(const unsigned char *__restrict__ row, int byte_off, unsigned (&wd)[3])
{
    // 12 bytes at any byte offset of an LDS row: four aligned dwords and a funnel shift
    const unsigned *p = (const unsigned *)(row + (byte_off & ~3));
    const unsigned d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3], m = (unsigned)(byte_off & 3);
    wd[0] = __builtin_amdgcn_alignbyte(d1, d0, m);
    wd[1] = __builtin_amdgcn_alignbyte(d2, d1, m);
    wd[2] = __builtin_amdgcn_alignbyte(d3, d2, m);
}

__global__ __launch_bounds__(256) void k_resize_gray_pair_lds(const unsigned char *__restrict__ a, long long sa,
                                                              const unsigned char *__restrict__ b, long long sb, int sh, int sw,
                                                              const CubicTab *__restrict__ xt, const CubicTab *__restrict__ yt,
                                                              int dh, int dw, int shift, unsigned char *__restrict__ ga,
                                                              unsigned char *__restrict__ gb, long long pitch, int lds_pitch,
                                                              double *__restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char win[];      // [image 2][slot 16][lds_pitch]
    __shared__ double ws[4];
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * 64 + tx;
    const int bx0 = blockIdx.x * 64, by0 = blockIdx.y * 4;
    // window columns: first tap of the first pixel .. last tap of the last pixel, clamped to the image; in bytes, rounded
    // down to 16 at the start
    const int xl = bx0, xr = min(bx0 + 63, dw - 1);
    const int c_lo = max(xt[xl].ofs - 1, 0), c_hi = min(xt[xr].ofs + 2, sw - 1);
    const int byte0 = (c_lo * 3) & ~15, nbytes = (c_hi + 1) * 3 - byte0;       // nbytes <= lds_pitch - 16 (host sizes it)
    const int nchunk = (nbytes + 15) >> 4, rowbytes = sw * 3;
    for (int e = tid; e < 32 * nchunk; e += 256) {
        const int slot = e / nchunk, ck = e - slot * nchunk;                    // slot = image * 16 + dst row * 4 + tap
        const int img = slot >> 4, j = (slot >> 2) & 3, t = slot & 3;
        const int y = min(by0 + j, dh - 1);
        const int srow = min(max(yt[y].ofs - 1 + t, 0), sh - 1);
        const unsigned char *src = (img ? b + (size_t)srow * sb : a + (size_t)srow * sa);
        const int off = byte0 + 16 * ck;
        u4_t v;
        if (off + 16 <= rowbytes) {
            v = *(const __attribute__((address_space(1))) u4_a1_t *)(src + off);
        } else {                                                                // the row's last bytes: never read past it
            unsigned w4[4] = {0u, 0u, 0u, 0u};
            for (int i = 0; i < 16 && off + i < rowbytes; ++i) w4[i >> 2] |= (unsigned)src[off + i] << (8 * (i & 3));
            v.x = w4[0]; v.y = w4[1]; v.z = w4[2]; v.w = w4[3];
        }
        *(u4_t *)(win + (size_t)slot * lds_pitch + 16 * ck) = v;
    }
    __syncthreads();
    const int x = bx0 + tx, y = by0 + ty;
    unsigned sse = 0;
    if (x < dw && y < dh) {
        const CubicTab X = xt[x], Y = yt[y];
        const bool inner = X.ofs - 1 >= 0 && X.ofs + 2 <= sw - 1;
        int va[3], vb[3];
#pragma unroll
        for (int img = 0; img < 2; ++img) {
            int acc[3] = {0, 0, 0};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const unsigned char *row = win + (size_t)(img * 16 + ty * 4 + t) * lds_pitch;
                int v[4][3];
                if (inner) {
                    unsigned wd[3];
                    lds_tap12(row, (X.ofs - 1) * 3 - byte0, wd);
#pragma unroll
                    for (int q = 0; q < 12; ++q) v[q / 3][q % 3] = (int)((wd[q >> 2] >> (8 * (q & 3))) & 0xFFu);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int sx = min(max(X.ofs + k - 1, 0), sw - 1) * 3 - byte0;
#pragma unroll
                        for (int c = 0; c < 3; ++c) v[k][c] = (int)row[sx + c];
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int hs = v[0][c] * X.c[0] + v[1][c] * X.c[1] + v[2][c] * X.c[2] + v[3][c] * X.c[3];
                    acc[c] += hs * (int)Y.c[t];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int r = (acc[c] + (1 << 21)) >> 22;
                (img ? vb : va)[c] = r < 0 ? 0 : (r > 255 ? 255 : r);
            }
        }
        ga[(size_t)y * pitch + x] = (unsigned char)gray_rgb(va[0], va[1], va[2], shift);
        gb[(size_t)y * pitch + x] = (unsigned char)gray_rgb(vb[0], vb[1], vb[2], shift);
#pragma unroll
        for (int c = 0; c < 3; ++c) sse += (unsigned)((va[c] - vb[c]) * (va[c] - vb[c]));
    }
    const double sred = wave_sum_f64((double)sse);
    if ((tid & 63) == 0) ws[tid >> 6] = sred;
    __syncthreads();
    if (tid == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// Round 3: the sampler for gentle down-sampling as a COLUMN MARCH.  cv2's INTER_CUBIC on u8 is exact integer arithmetic and
// separable -- sum_t cy[t] * (sum_k cx[k] * s[t][k]) -- so a lane that owns one destination column walks down the source
// rows, forms the horizontal 4-tap sums of each row ONCE (both images, three channels; a row feeds the 1.6 destination rows
// whose windows contain it), keeps the last four rows' sums in registers and finishes a destination pixel whenever the row
// just pushed is a window's last.  The byte pairs are formed with v_perm_b32 and multiplied with v_dot2_i32_i16 (two taps
// per instruction: the coefficients are 16-bit): ~150 VALU instructions per destination pixel instead of ~270.
// A wave owns RGM_SEG destination rows of 64 columns and is autonomous -- no block barrier.  The source rows reach the lanes
// through a WAVE-PRIVATE LDS window: the wave copies the contiguous span of each row it needs with aligned 16-byte loads
// (five or six cache-line accesses per row) and every lane then picks its 12 bytes from LDS.  Letting each lane load its own
// unaligned 12 bytes from global memory was measured first: 49 L1 accesses per wave instruction (TCP_TOTAL_CACHE_ACCESSES /
// TA_FLAT_READ_WAVEFRONTS), the L1 tag pipeline 75 % busy, 0.49 ms at x0.4.  The next group's rows are requested before the
// current group is processed.  Same integers as cubic_sample.
#ifndef RGM_SEG
#define RGM_SEG 16
#endif
typedef short rg_s2_t __attribute__((ext_vector_type(2)));

// horizontal 4-tap sums of one row's 12 bytes (4 pixels x RGB): hs[c] = sum_k px[k][c] * cx[k]
__device__ __forceinline__ void rgm_hrow(unsigned q0, unsigned q1, unsigned q2, rg_s2_t c01, rg_s2_t c23, int (&hs)[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        // bytes c and 3 + c of (q0, q1); bytes 6 + c and 9 + c of (q1, q2), each zero-extended to 16 bits
        const unsigned pa = __builtin_amdgcn_perm(q1, q0, 0x0c000c00u | (unsigned)c | ((unsigned)(3 + c) << 16));
        const unsigned pb = __builtin_amdgcn_perm(q2, q1, 0x0c000c00u | (unsigned)(2 + c) | ((unsigned)(5 + c) << 16));
        hs[c] = __builtin_amdgcn_sdot2(__builtin_bit_cast(rg_s2_t, pa), c01,
                                       __builtin_amdgcn_sdot2(__builtin_bit_cast(rg_s2_t, pb), c23, 0, false), false);
    }
}

// one 16-byte chunk of a source row's window.  A chunk that crosses the end of its row reads on into the next row (bytes
// no tap uses); only on the image's LAST row would that leave the buffer, and there the bytes are fetched one by one.
__device__ __forceinline__ u4_t rgm_load_chunk(const unsigned char *__restrict__ row, int off, int rowbytes, bool last_row)
{
    if (!last_row || off + 16 <= rowbytes) return *(const __attribute__((address_space(1))) u4_a1_t *)(row + off);
    unsigned w4[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
    for (int i = 0; i < 16 && off + i < rowbytes; ++i) w4[i >> 2] |= (unsigned)row[off + i] << (8 * (i & 3));
    u4_t v;
    v.x = w4[0]; v.y = w4[1]; v.z = w4[2]; v.w = w4[3];
    return v;
}

#ifndef RGM_MINB
#define RGM_MINB 5
#endif
__global__ __launch_bounds__(256, RGM_MINB) void k_resize_gray_pair_march(const unsigned char *__restrict__ a, long long sa,
                                                                const unsigned char *__restrict__ b, long long sb, int sh, int sw,
                                                                const CubicTab *__restrict__ xt, const CubicTab *__restrict__ yt,
                                                                int dh, int dw, int shift, unsigned char *__restrict__ ga,
                                                                unsigned char *__restrict__ gb, long long pitch, int lds_pitch,
                                                                int cols, double *__restrict__ part)
{
    // cols = destination columns per wave: 64, or 32 for scales below 0.19 whose 64-column window would exceed the 64
    // chunks a wave loads per row (all 64 lanes still load; the upper 32 sample a repeated column and store nothing -- at
    // those scales the kernel is bound by its loads, there are 25 x fewer destination than source pixels)
    extern __shared__ __attribute__((aligned(16))) unsigned char win[];      // [wave 4][image 2][row 4][lds_pitch]
    __shared__ double ws[4];
    const int tx = threadIdx.x, tid = threadIdx.y * 64 + tx;
    const int bx0 = blockIdx.x * cols, x = tx < cols ? bx0 + tx : dw;
    const int ys = __builtin_amdgcn_readfirstlane((blockIdx.y * 4 + threadIdx.y) * RGM_SEG), ye = min(ys + RGM_SEG, dh);
    unsigned sse = 0;
    if (ys < dh) {                                                  // wave-uniform
        unsigned char *mine = win + (size_t)threadIdx.y * 8 * lds_pitch;
        const int c_lo = max(xt[bx0].ofs - 1, 0), c_hi = min(xt[min(bx0 + cols - 1, dw - 1)].ofs + 2, sw - 1);
        const int byte0 = (c_lo * 3) & ~15, nchunk = ((c_hi + 1) * 3 - byte0 + 15) >> 4, rowbytes = sw * 3;   // nchunk <= 64 (host)
        const CubicTab X = xt[min(x, min(bx0 + cols, dw) - 1)];     // lanes past the end repeat the wave's last column, store nothing
        const bool inner = X.ofs - 1 >= 0 && X.ofs + 2 <= sw - 1;
        const int loff = max(X.ofs - 1, 0) * 3 - byte0;             // this lane's 12 bytes inside the window
        rg_s2_t c01, c23;
        c01.x = X.c[0]; c01.y = X.c[1]; c23.x = X.c[2]; c23.y = X.c[3];
        int y = ys, yofs = yt[ys].ofs;
        const int r_end = yt[ye - 1].ofs + 2;
        int ha[4][3], hb[4][3];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int c = 0; c < 3; ++c) ha[p][c] = hb[p][c] = 0;
        u4_t va4[4], vb4[4];                                        // the rows in flight (lane = chunk)
        auto request = [&](int r) {                                 // unclamped row numbers: rows beyond the image repeat the edge
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int sr = min(max(r + p, 0), sh - 1);
                if (tx < nchunk) {
                    va4[p] = rgm_load_chunk(a + (size_t)sr * sa, byte0 + 16 * tx, rowbytes, sr == sh - 1);
                    vb4[p] = rgm_load_chunk(b + (size_t)sr * sb, byte0 + 16 * tx, rowbytes, sr == sh - 1);
                }
            }
        };
        request(yofs - 1);
        for (int r = yofs - 1, r_next; r <= r_end; r = r_next) {
            // where the next group of four rows starts: right below this one, or -- when the windows lie further apart than
            // four rows (scales below 0.25) -- at the first row of the next window still to be finished (scalar bookkeeping)
            {
                int yn = y, yo = yofs;
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if (yn < ye && yo + 2 == r + p) {
                        ++yn;
                        yo = yn < ye ? yt[yn].ofs : 0x3fffffff;
                    }
                r_next = yn < ye ? max(r + 4, yo - 1) : r_end + 1;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the previous group's LDS reads are done
            __builtin_amdgcn_wave_barrier();
            if (tx < nchunk) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    *(u4_t *)(mine + (size_t)p * lds_pitch + 16 * tx) = va4[p];
                    *(u4_t *)(mine + (size_t)(4 + p) * lds_pitch + 16 * tx) = vb4[p];
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (r_next <= r_end) request(r_next);                   // flies under this group's arithmetic
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (r + p <= r_end) {                               // wave-uniform
                    const unsigned char *ra = mine + (size_t)p * lds_pitch, *rb = mine + (size_t)(4 + p) * lds_pitch;
                    unsigned wa[3], wb[3];
                    if (inner) {
                        lds_tap12(ra, loff, wa);
                        lds_tap12(rb, loff, wb);
                    } else {                                        // image border columns: taps clamped one by one
                        wa[0] = wa[1] = wa[2] = wb[0] = wb[1] = wb[2] = 0u;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int sx = min(max(X.ofs + k - 1, 0), sw - 1) * 3 - byte0;
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                const int i = 3 * k + c;
                                wa[i >> 2] |= (unsigned)ra[sx + c] << (8 * (i & 3));
                                wb[i >> 2] |= (unsigned)rb[sx + c] << (8 * (i & 3));
                            }
                        }
                    }
                    rgm_hrow(wa[0], wa[1], wa[2], c01, c23, ha[p]);
                    rgm_hrow(wb[0], wb[1], wb[2], c01, c23, hb[p]);
                    if (y < ye && yofs + 2 == r + p) {              // this row completes the window of destination row y
                        const CubicTab Y = yt[y];
                        int va[3], vb[3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            int s0 = 1 << 21, s1 = 1 << 21;
#pragma unroll
                            for (int t = 0; t < 4; ++t) {           // tap t = row r + p - 3 + t = ring slot (p + 1 + t) & 3
                                s0 += ha[(p + 1 + t) & 3][c] * (int)Y.c[t];
                                s1 += hb[(p + 1 + t) & 3][c] * (int)Y.c[t];
                            }
                            va[c] = min(max(s0 >> 22, 0), 255);
                            vb[c] = min(max(s1 >> 22, 0), 255);
                        }
                        if (x < dw) {
                            ga[(size_t)y * pitch + x] = (unsigned char)gray_rgb(va[0], va[1], va[2], shift);
                            gb[(size_t)y * pitch + x] = (unsigned char)gray_rgb(vb[0], vb[1], vb[2], shift);
#pragma unroll
                            for (int c = 0; c < 3; ++c) sse += (unsigned)((va[c] - vb[c]) * (va[c] - vb[c]));
                        }
                        ++y;
                        yofs = y < ye ? yt[y].ofs : 0x3fffffff;
                    }
                }
            }
        }
    }
    const double sred = wave_sum_f64((double)sse);
    if ((tid & 63) == 0) ws[tid >> 6] = sred;
    __syncthreads();
    if (tid == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

__global__ void k_store_sse(const double *__restrict__ src, sr_assess_sums *__restrict__ out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) out->sse = src[0];
}

// Final reduction of the assessment: ONE block sums the per-block partials part[i * 4 + comp] (fixed order: a
// strided serial sum per thread, then a fixed tree -- deterministic) and writes the four sums.
__global__ __launch_bounds__(256) void k_assess_finish(const double *__restrict__ part, long long n, int flags,
                                                       sr_assess_sums *__restrict__ out)
{
    __shared__ double sh[4][256];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long i = threadIdx.x; i < n; i += 256) {
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] += part[i * 4 + c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) sh[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int c = 0; c < 4; ++c) sh[c][threadIdx.x] += sh[c][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out->ssim_gauss = (flags & ASSESS_GAUSS) ? sh[0][0] : 0.0;
        out->ssim_simple = (flags & ASSESS_SIMPLE) ? sh[1][0] : 0.0;
        out->sse = (flags & ASSESS_SSE) ? sh[2][0] : 0.0;
        out->ssim_uniform = (flags & ASSESS_UNIFORM) ? sh[3][0] : 0.0;
    }
}

__global__ void k_assess_store(const double *__restrict__ g, const double *__restrict__ u, int flags,
                               sr_assess_sums *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out->ssim_gauss = (g && (flags & ASSESS_GAUSS)) ? g[0] : 0.0;
    out->ssim_simple = (g && (flags & ASSESS_SIMPLE)) ? g[1] : 0.0;
    out->sse = (g && (flags & ASSESS_SSE)) ? g[2] : 0.0;
    out->ssim_uniform = (u && (flags & ASSESS_UNIFORM)) ? u[0] : 0.0;
}

// reduce part[n][ncomp] -> returns pointer (inside the two ping-pong buffers) holding ncomp results
// ---------------------------------------------------------------------------------------------
// SSIM on FLOAT images.  The reference hands skimage / cv2 whatever _preprocess_image returns: float arrays whose
// maximum exceeds 1 stay float (quality_assessment_module.py:169-195,351-417).  A plain separable float64 form of
// oracle_np.ssim, not a tuned kernel (API convenience path; the u8 march above is the hot one):
//   k_ssimf_gray : gray planes in float64 (float32 RGB: cv2's float cvtColor, ((R*0.299f) + G*0.587f) + B*0.114f in fp32)
//   k_ssimf_rows : horizontal window sums of x, y, x*x, y*y, x*y (five float64 planes)
//   k_ssimf_cols : vertical window sums, the SSIM value of the mode, validity, per-block partial sums
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_ssimf_gray(const T *__restrict__ img, long long stride_bytes, int h, int w, int cn,
                                                    double *__restrict__ out)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const T *row = (const T *)((const char *)img + (size_t)y * stride_bytes);
    double g;
    if (cn == 1) g = (double)row[x];
    else {
        const float r = (float)row[3 * x], gg = (float)row[3 * x + 1], b = (float)row[3 * x + 2];
        g = (double)(((r * 0.299f) + gg * 0.587f) + b * 0.114f);
    }
    out[(size_t)y * w + x] = g;
}

struct SsimFParams {
    int h, w, mode, radius, bmode, crop, row_begin, row_end;
    double c1, c2, cov_norm;
    double k[11];
};

__global__ __launch_bounds__(256) void k_ssimf_rows(const double *__restrict__ ga, const double *__restrict__ gb, SsimFParams P,
                                                    double *__restrict__ tmp)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= P.w || y >= P.h) return;
    const size_t plane = (size_t)P.h * P.w;
    const double *ra = ga + (size_t)y * P.w, *rb = gb + (size_t)y * P.w;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int j = 0; j < 2 * P.radius + 1; ++j) {
        const int xi = border_index(x + j - P.radius, P.w, P.bmode);
        const double a = ra[xi], b = rb[xi], kj = P.k[j];
        sx += a * kj;
        sy += b * kj;
        sxx += (a * a) * kj;
        syy += (b * b) * kj;
        sxy += (a * b) * kj;
    }
    const size_t o = (size_t)y * P.w + x;
    tmp[o] = sx; tmp[plane + o] = sy; tmp[2 * plane + o] = sxx; tmp[3 * plane + o] = syy; tmp[4 * plane + o] = sxy;
}

__global__ __launch_bounds__(256) void k_ssimf_cols(const double *__restrict__ tmp, SsimFParams P, double *__restrict__ part)
{
    __shared__ double ws[4];
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    double v = 0.0;
    if (x < P.w && y < P.h && y >= max(P.crop, P.row_begin) && y < min(P.h - P.crop, P.row_end) && x >= P.crop && x < P.w - P.crop) {
        const size_t plane = (size_t)P.h * P.w;
        double u[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < 2 * P.radius + 1; ++j) {
            const size_t o = (size_t)border_index(y + j - P.radius, P.h, P.bmode) * P.w + x;
            const double kj = P.k[j];
#pragma unroll
            for (int m = 0; m < 5; ++m) u[m] += tmp[m * plane + o] * kj;
        }
        const double ux = u[0], uy = u[1], uxx = u[2], uyy = u[3], uxy = u[4];
        if (P.mode == SR_SSIM_SIMPLE) {
            const double m1 = ux * ux, m2 = uy * uy, m12 = ux * uy;
            const double s1 = uxx - m1, s2 = uyy - m2, s12 = uxy - m12;
            v = ((2.0 * m12 + P.c1) * (2.0 * s12 + P.c2)) / ((m1 + m2 + P.c1) * (s1 + s2 + P.c2));
        } else {
            const double vx = P.cov_norm * (uxx - ux * ux), vy = P.cov_norm * (uyy - uy * uy), vxy = P.cov_norm * (uxy - ux * uy);
            const double a1 = 2.0 * ux * uy + P.c1, a2 = 2.0 * vxy + P.c2;
            const double b1 = ux * ux + uy * uy + P.c1, b2 = vx + vy + P.c2;
            v = (a1 * a2) / (b1 * b2);
        }
    }
    const int tid = threadIdx.y * 64 + threadIdx.x;
    const double sred = wave_sum_f64(v);
    if ((tid & 63) == 0) ws[tid >> 6] = sred;
    __syncthreads();
    if (tid == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

const double *reduce_partials(sr_ctx *ctx, const double *part, long long n, int ncomp, double *buf0, double *buf1)
{
    const double *src = part;
    double *dst = buf0;
    while (true) {
        const long long nb = (n + 1023) / 1024;
        hipLaunchKernelGGL(k_reduce_partials, dim3((unsigned)nb), dim3(256), 0, ctx->stream, src, n, ncomp, dst);
        if (nb == 1) return dst;
        src = dst;
        dst = (dst == buf0) ? buf1 : buf0;
        n = nb;
    }
}

// The blocking form of an assessment: run(d_res) enqueues it into a one-call result word, which is then copied to *h_out.
// The caller holds the context's Guard.
template <typename Run>
static int assess_to_host(sr_ctx *ctx, const char *who, sr_assess_sums *h_out, Run &&run)
{
    DevTemp res(ctx);
    SRCHK(res.alloc(who, sizeof(sr_assess_sums)));
    SRCHK(run(res.as<sr_assess_sums>()));
    HIPCHK(hipMemcpyAsync(h_out, res.d, sizeof(sr_assess_sums), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

extern "C" {

// ---- metrics ------------------------------------------------------------------------------------------
int sr_sse_u8_async(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h,
                    int64_t rowlen, uint64_t *d_sse)
{
    CTX_ENTER(ctx);
    if (!d_a || !d_b || !d_sse || h < 0 || rowlen < 0) return sr_set_error(SR_ERR_INVALID_ARG, "sr_sse_u8: bad arguments");
    HIPCHK(hipMemsetAsync(d_sse, 0, sizeof(uint64_t), ctx->stream));
    if (h == 0 || rowlen == 0) return SR_OK;
    const bool dense = stride_a == rowlen && stride_b == rowlen && ((uintptr_t)d_a % 16 == 0) && ((uintptr_t)d_b % 16 == 0);
    {
        ProfScope ps(ctx, "psnr_sse");
        if (dense) {
            const size_t total = (size_t)h * (size_t)rowlen;
            const size_t nvec = total / 16;
            const int ntail = (int)(total - nvec * 16);
            const int blocks = (int)std::min<size_t>((nvec + 255) / 256 + 1, 256 * 16);
            hipLaunchKernelGGL(k_sse_flat, dim3(blocks), dim3(256), 0, ctx->stream, (const uint4 *)d_a, (const uint4 *)d_b, nvec,
                               d_a + nvec * 16, d_b + nvec * 16, ntail, (unsigned long long *)d_sse);
        } else {
            const int gx = (int)std::min<int64_t>((rowlen + 255) / 256, 64);
            const int gy = std::min(h, 1024);
            hipLaunchKernelGGL(k_sse_rows, dim3(gx, gy), dim3(256), 0, ctx->stream, d_a, (long long)stride_a, d_b,
                               (long long)stride_b, h, (long long)rowlen, (unsigned long long *)d_sse);
        }
    }
    return check_launch("psnr_sse");
}

int sr_sse_f32(sr_ctx *ctx, const float *d_a, int64_t stride_a, const float *d_b, int64_t stride_b, int h,
               int64_t rowlen, double *h_sse)
{
    CTX_ENTER(ctx);
    if (!d_a || !d_b || !h_sse || h < 0 || rowlen < 0) return sr_set_error(SR_ERR_INVALID_ARG, "sr_sse_f32: bad arguments");
    *h_sse = 0.0;
    if (h == 0 || rowlen == 0) return SR_OK;
    const int gx = (int)std::min<int64_t>((rowlen + 255) / 256, 64), gy = std::min(h, 1024);
    void *scr = nullptr;
    int rc = ctx_scratch(ctx, (size_t)8 << 20, &scr);
    if (rc) return rc;
    double *part = (double *)scr, *r0 = part + (size_t)gx * gy + 32, *r1 = r0 + 4096;
    {
        ProfScope ps(ctx, "psnr_sse_f32");
        hipLaunchKernelGGL(k_sse_f32, dim3(gx, gy), dim3(256), 0, ctx->stream, d_a, (long long)stride_a, d_b, (long long)stride_b,
                           h, (long long)rowlen, part);
    }
    const double *res = reduce_partials(ctx, part, (long long)gx * gy, 1, r0, r1);
    rc = check_launch("psnr_sse_f32");
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h_sse, res, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_sse_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h,
              int64_t rowlen, uint64_t *h_sse)
{
    CTX_ENTER(ctx);
    if (!h_sse) return sr_set_error(SR_ERR_INVALID_ARG, "sr_sse_u8: null result");
    void *scr = nullptr;
    int rc = ctx_scratch(ctx, 64, &scr);
    if (rc) return rc;
    rc = sr_sse_u8_async(ctx, d_a, stride_a, d_b, stride_b, h, rowlen, (uint64_t *)scr);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h_sse, scr, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_ssim_count(int h, int w, int mode, int row_begin, int row_end, uint64_t *count)
{
    if (!count || h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_ssim_count: bad arguments");
    int pad;
    if (mode == SR_SSIM_UNIFORM7) pad = 3;
    else if (mode == SR_SSIM_GAUSS11) pad = 5;
    else if (mode == SR_SSIM_SIMPLE) pad = 0;
    else return sr_set_error(SR_ERR_INVALID_ARG, "sr_ssim_count: unknown mode %d", mode);
    const long long y0 = std::max(pad, row_begin), y1 = std::min(h - pad, row_end), nx = (long long)w - 2 * pad;
    *count = (y1 > y0 && nx > 0) ? (uint64_t)((y1 - y0) * nx) : 0;
    return SR_OK;
}

// Shared body of sr_assess_u8_async / sr_assess_resized_u8_async (which hands it the resized gray planes).
static int assess_impl(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h,
                       int w, int cn, int gray_shift, double data_range, int row_begin, int row_end, int flags,
                       sr_assess_sums *d_out, const char *scope)
{
    if (!d_a || !d_b || !d_out) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", scope);
    if (h < 1 || w < 1 || (cn != 1 && cn != 3)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need h,w >= 1 and 1 or 3 channels", scope);
    if (gray_shift != 14 && gray_shift != 15) return sr_set_error(SR_ERR_INVALID_ARG, "%s: gray_shift must be 14 or 15", scope);
    const int64_t min_stride = (int64_t)w * cn;
    if (stride_a < min_stride || stride_b < min_stride) return sr_set_error(SR_ERR_SHAPE, "%s: stride smaller than a row", scope);
    row_begin = std::max(row_begin, 0);
    row_end = std::min(row_end, h);
    AssessParams P;
    memset(&P, 0, sizeof(P));
    P.h = h; P.w = w; P.shift = gray_shift; P.ry0 = row_begin; P.ry1 = row_end; P.flags = flags;
    P.c1a = (0.01 * data_range) * (0.01 * data_range);
    P.c2a = (0.03 * data_range) * (0.03 * data_range);
    P.c1b = (0.01 * 255.0) * (0.01 * 255.0);
    P.c2b = (0.03 * 255.0) * (0.03 * 255.0);
    P.same_c = (P.c1a == P.c1b && P.c2a == P.c2b) ? 1 : 0;
    P.k1u = 2401.0 * P.c1a;
    P.k2u = 2352.0 * P.c2a;
    gauss_taps(P.k);
    const int rows = row_end - row_begin;
    if (rows > 0 && (flags & ASSESS_ALL_BITS)) {
        // Blocks are equal work, 3 resident per CU: pick the chunk count that minimises (rounds of blocks) x (rows a
        // block marches) -- long blocks amortise the 10-row halo, short ones avoid a mostly empty last round on strips.
        const long long gbx = (w + AM_TX - 1) / AM_TX;
        const long long slots = (long long)std::max(ctx->num_cu, 1) * 3;
        // Measured (profiles/r02_assess_nch.json): longer blocks do NOT pay although they amortise the 10-row halo and
        // can fill the chip in exact rounds -- 25 / 33 / 49 chunks run 1.60 / 1.64 / 1.70 ms against 1.55 ms for 12: blocks
        // that start together stay in lockstep, so every wave of a CU sits in its load phase (or its fp64 march) at
        // the same time; many short blocks drift apart and overlap the two.
        long long best_cost = -1;
        for (int n = 2; n <= AM_NCH_MAX; ++n) {
            const int ty = AM_CH * n - 2 * AM_R;
            const long long blocks = gbx * ((rows + ty - 1) / ty);
            const long long cost = ((blocks + slots - 1) / slots) * (AM_CH * n);
            if (best_cost < 0 || cost <= best_cost) { best_cost = cost; P.nch = n; P.ty = ty; }
        }
        // SR_ASSESS_NCH=n, an integer in [2, AM_NCH_MAX]: that chunk count instead of the cost rule's choice (anything else
        // is ignored).  The sums do not depend on it beyond the order of the additions; the suite uses it to run every
        // block length at small shapes.  Read per call.
        if (const char *e = std::getenv("SR_ASSESS_NCH")) {
            char *end = nullptr;
            const long n = std::strtol(e, &end, 10);
            if (end != e && *end == '\0' && n >= 2 && n <= AM_NCH_MAX) { P.nch = (int)n; P.ty = AM_CH * (int)n - 2 * AM_R; }
        }
        const long long gby = (rows + P.ty - 1) / P.ty;
        const size_t nblk = (size_t)(gbx * gby);
        void *scr = nullptr;
        int rc = ctx_scratch(ctx, std::max<size_t>(nblk * 4 * 8 + 512, (size_t)8 << 20), &scr);
        if (rc) return rc;
        double *part = (double *)scr;
        {
            ProfScope ps(ctx, scope);
            const dim3 grid((unsigned)gbx, (unsigned)gby), block(AM_TX);
#define LAUNCH_ASSESS(CNV, GS, US, SC)                                                                               \
    hipLaunchKernelGGL((k_assess_march<CNV, GS, US, SC>), grid, block, 0, ctx->stream, d_a, (long long)stride_a, d_b,   \
                       (long long)stride_b, P, part)
#define LAUNCH_ASSESS_V(CNV)                                                                                            \
    do {                                                                                                                \
        if (gauss && unif) { if (P.same_c) LAUNCH_ASSESS(CNV, true, true, true); else LAUNCH_ASSESS(CNV, true, true, false); } \
        else if (gauss) { if (P.same_c) LAUNCH_ASSESS(CNV, true, false, true); else LAUNCH_ASSESS(CNV, true, false, false); } \
        else if (unif) LAUNCH_ASSESS(CNV, false, true, true);                                                           \
        else LAUNCH_ASSESS(CNV, false, false, true);                                                                    \
    } while (0)
            const bool gauss = (flags & (ASSESS_GAUSS | ASSESS_SIMPLE)) != 0, unif = (flags & ASSESS_UNIFORM) != 0;
            if (cn == 3) LAUNCH_ASSESS_V(3);
            else LAUNCH_ASSESS_V(1);
#undef LAUNCH_ASSESS_V
#undef LAUNCH_ASSESS
            hipLaunchKernelGGL(k_assess_finish, dim3(1), dim3(256), 0, ctx->stream, part, (long long)nblk, flags, d_out);
        }
        return check_launch("assess");
    }
    hipLaunchKernelGGL(k_assess_store, dim3(1), dim3(64), 0, ctx->stream, (const double *)nullptr, (const double *)nullptr, flags, d_out);
    return check_launch("assess");
}

int sr_assess_u8_async(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h,
                       int w, int cn, int gray_shift, double data_range, int row_begin, int row_end, int flags,
                       sr_assess_sums *d_out)
{
    CTX_ENTER(ctx);
    return assess_impl(ctx, d_a, stride_a, d_b, stride_b, h, w, cn, gray_shift, data_range, row_begin, row_end, flags,
                       d_out, "assess_all");
}

int sr_assess_resized_u8_async(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b,
                               int h, int w, int cn, int dst_h, int dst_w, int gray_shift, double data_range, int flags,
                               sr_assess_sums *d_out)
{
    CTX_ENTER(ctx);
    if (h < 1 || w < 1 || dst_h < 1 || dst_w < 1)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_assess_resized_u8: need positive source and destination sizes");
    if (!d_a || !d_b || !d_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_assess_resized_u8: null argument");
    if (cn != 1 && cn != 3) return sr_set_error(SR_ERR_INVALID_ARG, "sr_assess_resized_u8: need 1 or 3 channels");
    if (gray_shift != 14 && gray_shift != 15) return sr_set_error(SR_ERR_INVALID_ARG, "sr_assess_resized_u8: gray_shift must be 14 or 15");
    if (stride_a < (int64_t)w * cn || stride_b < (int64_t)w * cn) return sr_set_error(SR_ERR_SHAPE, "sr_assess_resized_u8: stride smaller than a row");
    // Stage 1: every resized pixel of both images is sampled ONCE by a plain map kernel (8 independent 12-byte loads per
    // pixel, full occupancy), its channel differences squared and summed, and only its two gray values kept: two u8 planes of
    // the resized size (the RGB intermediates of cv2.resize are never materialised).  Stage 2: the ordinary one-channel
    // assessment march over those planes.  (Sampling inside the march's loader -- round 1 -- kept the 88-register filter
    // FIFO alive across a rolled, latency-bound loop: 1.98 ms for the three scales of a 200 MP pair.)
    std::vector<CubicTab> xt, yt;
    cubic_table(w, dst_w, xt);
    cubic_table(h, dst_h, yt);
    xt.insert(xt.end(), yt.begin(), yt.end());
    SRCHK(upload_cached(ctx, ctx->resize_tab, xt.data(), sizeof(CubicTab) * xt.size()));
    const CubicTab *d_xt = ctx->resize_tab.buf.as<const CubicTab>(), *d_yt = d_xt + dst_w;
    const int64_t pitch = ((int64_t)dst_w + 63) / 64 * 64;
    // down-sampling RGB: the LDS-staged kernel when its source window (64 destination columns wide) fits
    int lds_pitch = 0, march_cols = 0, march_pitch = 0;
    if (cn == 3 && dst_w < w && dst_h < h) {
        auto window_pitch = [&](int cols) {
            int span = 0;
            for (int x0b = 0; x0b < dst_w; x0b += cols) {
                const int lo = std::max(xt[(size_t)x0b].ofs - 1, 0), hi = std::min(xt[(size_t)std::min(x0b + cols - 1, dst_w - 1)].ofs + 2, w - 1);
                span = std::max(span, (hi + 1) * 3 - ((lo * 3) & ~15));
            }
            return (span + 15) / 16 * 16 + 16;                                     // + one chunk: lds_tap12 reads 16 aligned bytes
        };
        const int lp = window_pitch(64);
        if (32 * lp <= 64 * 1024) lds_pitch = lp;
        for (int cols = 64; cols >= 32 && !march_cols; cols >>= 1) {
            const int mp = cols == 64 ? lp : window_pitch(cols);
            if (mp <= 64 * 16 + 16) { march_cols = cols; march_pitch = mp; }
        }
    }
    // since round 3 the wave-autonomous column march (k_resize_gray_pair_march) takes every down-sampling whose source window
    // (64 destination columns wide, or 32) is at most 64 chunks of 16 bytes, i.e. scales down to about 0.095
    // (SR_RESIZE_MARCH=0: the block-staged kernel)
    const bool march = march_cols > 0 && !(std::getenv("SR_RESIZE_MARCH") && std::getenv("SR_RESIZE_MARCH")[0] == '0');
    const dim3 block(64, 4), grid(march ? (unsigned)((dst_w + march_cols - 1) / march_cols)
                                 : lds_pitch ? (unsigned)((dst_w + 63) / 64) : (unsigned)((dst_w + 255) / 256),
                                 march ? (unsigned)((dst_h + 4 * RGM_SEG - 1) / (4 * RGM_SEG)) : (unsigned)((dst_h + 3) / 4));
    const size_t nblk = (size_t)grid.x * grid.y, plane = (size_t)pitch * dst_h;
    const size_t off_part = (2 * plane + 255) / 256 * 256, need = off_part + (nblk + 2 * (nblk / 1024 + 2)) * sizeof(double);
    SRCHK(ctx->gray_planes.reserve(ctx, "sr_assess_resized_u8", need));
    uint8_t *ga = ctx->gray_planes.as<uint8_t>(), *gb = ga + plane;
    double *part = ctx->gray_planes.as<double>(off_part), *buf0 = part + nblk, *buf1 = buf0 + nblk / 1024 + 2;
    const bool want_sse = (flags & ASSESS_SSE) != 0;
    const double *sse_ptr = nullptr;
    {
        ProfScope ps(ctx, "resize_gray");
        if (march) {
            hipLaunchKernelGGL(k_resize_gray_pair_march, grid, block, (size_t)32 * march_pitch, ctx->stream, d_a, (long long)stride_a, d_b,
                               (long long)stride_b, h, w, d_xt, d_yt, dst_h, dst_w, gray_shift, ga, gb, (long long)pitch, march_pitch,
                               march_cols, part);
        } else if (lds_pitch) {
            {   // once per device (the attribute belongs to the function ON a device), under a lock: contexts of several
                // devices / threads reach this concurrently
                static std::mutex mu;
                static std::set<int> done;
                std::lock_guard<std::mutex> lk(mu);
                if (!done.count(ctx->device)) {
                    HIPCHK(hipFuncSetAttribute((const void *)k_resize_gray_pair_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
                    done.insert(ctx->device);
                }
            }
            hipLaunchKernelGGL(k_resize_gray_pair_lds, grid, block, (size_t)32 * lds_pitch, ctx->stream, d_a, (long long)stride_a, d_b,
                               (long long)stride_b, h, w, d_xt, d_yt, dst_h, dst_w, gray_shift, ga, gb, (long long)pitch, lds_pitch, part);
        } else if (cn == 3) hipLaunchKernelGGL(k_resize_gray_pair<3>, grid, block, 0, ctx->stream, d_a, (long long)stride_a, d_b, (long long)stride_b, h, w, d_xt, d_yt, dst_h, dst_w, gray_shift, ga, gb, (long long)pitch, part);
        else hipLaunchKernelGGL(k_resize_gray_pair<1>, grid, block, 0, ctx->stream, d_a, (long long)stride_a, d_b, (long long)stride_b, h, w, d_xt, d_yt, dst_h, dst_w, gray_shift, ga, gb, (long long)pitch, part);
        if (want_sse) sse_ptr = reduce_partials(ctx, part, (long long)nblk, 1, buf0, buf1);
    }
    int rc = check_launch("resize_gray");
    if (rc) return rc;
    rc = assess_impl(ctx, ga, pitch, gb, pitch, dst_h, dst_w, 1, gray_shift, data_range, 0, dst_h, flags & ~ASSESS_SSE, d_out, "assess_resized");
    if (rc) return rc;
    if (want_sse) {
        hipLaunchKernelGGL(k_store_sse, dim3(1), dim3(64), 0, ctx->stream, sse_ptr, d_out);
        return check_launch("assess_resized sse");
    }
    return SR_OK;
}

int sr_assess_resized_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h,
                         int w, int cn, int dst_h, int dst_w, int gray_shift, double data_range, int flags,
                         sr_assess_sums *h_out)
{
    CTX_ENTER(ctx);
    if (!h_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_assess_resized_u8: null result");
    return assess_to_host(ctx, "sr_assess_resized_u8", h_out, [&](sr_assess_sums *d_res) {
        return sr_assess_resized_u8_async(ctx, d_a, stride_a, d_b, stride_b, h, w, cn, dst_h, dst_w, gray_shift, data_range, flags, d_res);
    });
}

int sr_assess_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                 int cn, int gray_shift, double data_range, int row_begin, int row_end, int flags, sr_assess_sums *h_out)
{
    CTX_ENTER(ctx);
    if (!h_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_assess_u8: null result");
    return assess_to_host(ctx, "sr_assess_u8", h_out, [&](sr_assess_sums *d_res) {
        return sr_assess_u8_async(ctx, d_a, stride_a, d_b, stride_b, h, w, cn, gray_shift, data_range, row_begin, row_end, flags, d_res);
    });
}

static int ssim_mode_check(int h, int w, int mode, int *flag, size_t *field_off)
{
    int pad;
    if (mode == SR_SSIM_UNIFORM7) { pad = 3; *flag = ASSESS_UNIFORM; *field_off = offsetof(sr_assess_sums, ssim_uniform); }
    else if (mode == SR_SSIM_GAUSS11) { pad = 5; *flag = ASSESS_GAUSS; *field_off = offsetof(sr_assess_sums, ssim_gauss); }
    else if (mode == SR_SSIM_SIMPLE) { pad = 0; *flag = ASSESS_SIMPLE; *field_off = offsetof(sr_assess_sums, ssim_simple); }
    else return sr_set_error(SR_ERR_INVALID_ARG, "sr_ssim_u8: unknown mode %d", mode);
    if (h <= 2 * pad || w <= 2 * pad)
        return sr_set_error(SR_ERR_SHAPE, "sr_ssim_u8: image %dx%d smaller than the %d-tap window", w, h, 2 * pad + 1);
    return SR_OK;
}

int sr_ssim_u8_async(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h,
                     int w, int cn, int mode, int gray_shift, double data_range, int row_begin, int row_end,
                     double *d_sum, uint64_t *h_count)
{
    CTX_ENTER(ctx);
    if (!d_a || !d_b || !d_sum || !h_count) return sr_set_error(SR_ERR_INVALID_ARG, "sr_ssim_u8: null argument");
    int flag = 0;
    size_t off = 0;
    int rc = ssim_mode_check(h, w, mode, &flag, &off);
    if (rc) return rc;
    rc = sr_ssim_count(h, w, mode, row_begin, row_end, h_count);
    if (rc) return rc;
    void *scr = nullptr;
    rc = ctx_scratch(ctx, (size_t)8 << 20, &scr);
    if (rc) return rc;
    // the result record lives in the last 256 bytes of the (>= 8 MiB) scratch, clear of the partial buffers
    sr_assess_sums *rec = ctx->scratch.as<sr_assess_sums>(ctx->scratch.cap - 256);
    rc = sr_assess_u8_async(ctx, d_a, stride_a, d_b, stride_b, h, w, cn, gray_shift, data_range, row_begin, row_end, flag, rec);
    if (rc) return rc;
    rec = ctx->scratch.as<sr_assess_sums>(ctx->scratch.cap - 256);    // scratch may have grown
    HIPCHK(hipMemcpyAsync(d_sum, (const char *)rec + off, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return SR_OK;
}

int sr_ssim_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
               int cn, int mode, int gray_shift, double data_range, int row_begin, int row_end, double *h_sum,
               uint64_t *h_count)
{
    CTX_ENTER(ctx);
    if (!h_sum || !h_count) return sr_set_error(SR_ERR_INVALID_ARG, "sr_ssim_u8: null result");
    int flag = 0;
    size_t off = 0;
    int rc = ssim_mode_check(h, w, mode, &flag, &off);
    if (rc) return rc;
    rc = sr_ssim_count(h, w, mode, row_begin, row_end, h_count);
    if (rc) return rc;
    sr_assess_sums sums;
    rc = sr_assess_u8(ctx, d_a, stride_a, d_b, stride_b, h, w, cn, gray_shift, data_range, row_begin, row_end, flag, &sums);
    if (rc) return rc;
    *h_sum = *(const double *)((const char *)&sums + off);
    return SR_OK;
}

int sr_ssim_float(sr_ctx *ctx, int dtype, const void *d_a, int64_t stride_a, const void *d_b, int64_t stride_b, int h, int w,
                  int cn, int mode, double data_range, int row_begin, int row_end, double *h_sum, uint64_t *h_count)
{
    CTX_ENTER(ctx);
    if (!d_a || !d_b || !h_sum || !h_count) return sr_set_error(SR_ERR_INVALID_ARG, "sr_ssim_float: null argument");
    if (dtype != SR_F32 && dtype != SR_F64) return sr_set_error(SR_ERR_INVALID_ARG, "sr_ssim_float: dtype must be SR_F32 or SR_F64");
    if (cn != 1 && !(cn == 3 && dtype == SR_F32))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_ssim_float: 1 channel, or 3 channels of float32 (cv2.cvtColor rejects float64 RGB)");
    int flag = 0;
    size_t off = 0;
    int rc = ssim_mode_check(h, w, mode, &flag, &off);
    if (rc) return rc;
    const int es = dtype == SR_F32 ? 4 : 8;
    if (stride_a < (int64_t)w * cn * es || stride_b < (int64_t)w * cn * es) return sr_set_error(SR_ERR_SHAPE, "sr_ssim_float: stride smaller than a row");
    row_begin = std::max(row_begin, 0);
    row_end = std::min(row_end, h);
    rc = sr_ssim_count(h, w, mode, row_begin, row_end, h_count);
    if (rc) return rc;
    SsimFParams P;
    memset(&P, 0, sizeof(P));
    P.h = h; P.w = w; P.mode = mode; P.row_begin = row_begin; P.row_end = row_end;
    P.c1 = (0.01 * data_range) * (0.01 * data_range);
    P.c2 = (0.03 * data_range) * (0.03 * data_range);
    P.cov_norm = 1.0;
    if (mode == SR_SSIM_UNIFORM7) {
        P.radius = 3; P.bmode = PAD_REFLECT; P.crop = 3; P.cov_norm = 49.0 / 48.0;
        for (int j = 0; j < 7; ++j) P.k[j] = 1.0 / 7.0;
    } else {
        double k6[6];
        gauss_taps(k6);                                  // scipy's and cv2's normalised 11-tap kernels coincide
        P.radius = 5;
        for (int j = 0; j <= 5; ++j) P.k[5 + j] = P.k[5 - j] = k6[j];
        if (mode == SR_SSIM_GAUSS11) { P.bmode = PAD_REFLECT; P.crop = 5; }
        else { P.bmode = PAD_MIRROR; P.crop = 0; P.c1 = (0.01 * 255.0) * (0.01 * 255.0); P.c2 = (0.03 * 255.0) * (0.03 * 255.0); }
    }
    const size_t plane = (size_t)h * w;
    const dim3 block(64, 4), grid((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4));
    const size_t nblk = (size_t)grid.x * grid.y;
    DevTemp tmp_planes(ctx);
    SRCHK(tmp_planes.alloc("sr_ssim_float", (7 * plane + nblk + 2 * (nblk / 1024 + 2)) * sizeof(double)));
    double *buf = tmp_planes.as<double>();
    double *ga = buf, *gb = buf + plane, *tmp = buf + 2 * plane, *part = buf + 7 * plane, *b0 = part + nblk, *b1 = b0 + nblk / 1024 + 2;
    {
        ProfScope ps(ctx, "ssim_float");
        if (dtype == SR_F32) {
            hipLaunchKernelGGL(k_ssimf_gray<float>, grid, block, 0, ctx->stream, (const float *)d_a, (long long)stride_a, h, w, cn, ga);
            hipLaunchKernelGGL(k_ssimf_gray<float>, grid, block, 0, ctx->stream, (const float *)d_b, (long long)stride_b, h, w, cn, gb);
        } else {
            hipLaunchKernelGGL(k_ssimf_gray<double>, grid, block, 0, ctx->stream, (const double *)d_a, (long long)stride_a, h, w, cn, ga);
            hipLaunchKernelGGL(k_ssimf_gray<double>, grid, block, 0, ctx->stream, (const double *)d_b, (long long)stride_b, h, w, cn, gb);
        }
        hipLaunchKernelGGL(k_ssimf_rows, grid, block, 0, ctx->stream, (const double *)ga, (const double *)gb, P, tmp);
        hipLaunchKernelGGL(k_ssimf_cols, grid, block, 0, ctx->stream, (const double *)tmp, P, part);
    }
    const double *res = reduce_partials(ctx, part, (long long)nblk, 1, b0, b1);
    SRCHK(check_launch("ssim_float"));
    HIPCHK(hipMemcpyAsync(h_sum, res, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_rgb2gray_u8(sr_ctx *ctx, const uint8_t *d_rgb, int64_t stride, int h, int w, int gray_shift, uint8_t *d_gray,
                   int64_t gray_stride)
{
    CTX_ENTER(ctx);
    if (!d_rgb || !d_gray || h < 1 || w < 1 || (gray_shift != 14 && gray_shift != 15))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_rgb2gray_u8: bad arguments");
    {
        ProfScope ps(ctx, "rgb2gray");
        dim3 grid((w + 63) / 64, (h + 3) / 4), block(64, 4);
        hipLaunchKernelGGL(k_rgb2gray, grid, block, 0, ctx->stream, d_rgb, (long long)stride, h, w, gray_shift, d_gray,
                           (long long)gray_stride);
    }
    return check_launch("rgb2gray");
}

int sr_resize_cubic_window_u8(sr_ctx *ctx, const uint8_t *d_src, int64_t src_stride, int h, int w, int cn, int dh,
                              int dw, int x0, int y0, int ww, int wh, uint8_t *d_dst, int64_t dst_stride)
{
    CTX_ENTER(ctx);
    if (!d_src || !d_dst || h < 1 || w < 1 || dh < 1 || dw < 1 || cn < 1 || cn > 4)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_resize_cubic_u8: bad arguments");
    if (x0 < 0 || y0 < 0 || ww < 1 || wh < 1 || x0 + ww > dw || y0 + wh > dh)
        return sr_set_error(SR_ERR_SHAPE, "sr_resize_cubic_u8: window outside the %dx%d result", dw, dh);
    std::vector<CubicTab> xt, yt;
    cubic_table(w, dw, xt);
    cubic_table(h, dh, yt);
    xt.insert(xt.end(), yt.begin(), yt.end());          // both axes in one cached device table (re-used per geometry)
    SRCHK(upload_cached(ctx, ctx->cubic_tab, xt.data(), sizeof(CubicTab) * xt.size()));
    CubicTab *dx = ctx->cubic_tab.buf.as<CubicTab>(), *dy = dx + dw;
    {
        ProfScope ps(ctx, "resize_cubic");
        dim3 grid((ww + 63) / 64, (wh + 3) / 4), block(64, 4);
        if (cn == 3 && dh >= h) {                        // rows are reused: the marching kernel
            dim3 gridu((ww + 1023) / 1024, (wh + RUP_SEG - 1) / RUP_SEG);
            hipLaunchKernelGGL(k_resize_cubic_up_rgb, gridu, dim3(256), 0, ctx->stream, d_src, (long long)src_stride, h, w,
                               (const CubicTab *)dx, (const CubicTab *)dy, x0, y0, ww, wh, d_dst, (long long)dst_stride);
        } else if (cn == 3) {
            dim3 grid4((ww + 255) / 256, (wh + 3) / 4);
            hipLaunchKernelGGL(k_resize_cubic_rgb4, grid4, block, 0, ctx->stream, d_src, (long long)src_stride, h, w,
                               (const CubicTab *)dx, (const CubicTab *)dy, x0, y0, ww, wh, d_dst, (long long)dst_stride);
        } else
        hipLaunchKernelGGL(k_resize_cubic, grid, block, 0, ctx->stream, d_src, (long long)src_stride, h, w, cn,
                           (const CubicTab *)dx, (const CubicTab *)dy, x0, y0, ww, wh, d_dst, (long long)dst_stride);
    }
    return check_launch("resize_cubic");
}

int sr_resize_cubic_u8(sr_ctx *ctx, const uint8_t *d_src, int64_t src_stride, int h, int w, int cn, uint8_t *d_dst,
                       int64_t dst_stride, int dh, int dw)
{
    return sr_resize_cubic_window_u8(ctx, d_src, src_stride, h, w, cn, dh, dw, 0, 0, dw, dh, d_dst, dst_stride);
}

}  // extern "C"
