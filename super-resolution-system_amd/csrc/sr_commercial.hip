// sr_commercial.hip -- QualityAssessmentModule.evaluate_commercial / evaluate_no_reference (quality_assessment_module.py
// of the reference, the NumPy / OpenCV metrics of :611-1193) on gfx950.
//
// Every metric is a stencil, a reduction or a 2-D DFT of the gray plane (or of the RGB data for Lab / YCrCb):
//   k_cm_color    one pass over the u8 image: the RGB2GRAY plane of the whole image (cn >= 3; cn 1 IS the gray plane) and,
//                 per rectangle, exact sums of the 8-bit Lab L, a, b and their squares, the YCrCb skin count and the RGB
//                 sums (brand mean colour).
//   k_cm_stencil  per rectangle over the gray plane with reflect-101 at the RECTANGLE's border (cv2 sees an ROI as an image
//                 of its own): Laplacian and gray sums, the 3x3 Gaussian noise residual (x16, an exact integer), Sobel
//                 |grad|^2 (exact) and |grad| (fp64), the 5x5 box local variance (fp32 per pixel) and the 7x7 Gaussian MSCN
//                 coefficients (fp32 per pixel, one fixed operation order, fp-contract off).
//   k_cm_blocks   8x8 block variances of _detect_artifacts as exact integers 64 sum(x^2) - sum(x)^2.
//   k_cm_regions  the 4x4 region sums of _calculate_brightness_uniformity.
//   k_canny_*     cv2.Canny(gray, 50, 150): L1 magnitude, non-maximum suppression to a state map, hysteresis as LDS-local
//                 flood fills in 32x32 tiles repeated over the image until a sweep changes nothing, then the edge count.
//   k_fft_* / k_hf_reduce  the high-frequency ratio: a hand-written fp32 mixed-radix Stockham FFT (one launch per radix
//                 pass, any radix up to CM_MAX_RADIX as a direct DFT out of LDS), Bluestein for a line length with a larger
//                 prime factor; rows two at a time as one complex line, split into half spectra and transposed, columns,
//                 then sum |F| (fp32 magnitude, fp64 sums) inside and outside the radius.
// Integer sums are taken with 64-bit integer atomics (exact, so order-free); every fp64 sum is per-block partials added
// in block order on the host: repeated calls return identical bits.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_ctx.h"
#include "sr_fft.h"

namespace {

#define CM_THREADS 256
#define CM_NBLK 1024          // blocks per rectangle of the stats kernels (the fp64 partial order depends on it)
#define CM_MAX_RADIX 1024     // largest prime factor transformed by a direct DFT pass; larger ones go through Bluestein
#define CM_MAX_LEN 32768      // longest supported FFT line (image side)
#define CN_TS 32              // Canny hysteresis tile (interior)
#define CN_BATCH 8            // hysteresis sweeps enqueued between two flag readbacks

struct CmRect {
    int x, y, w, h, flags;
};

struct LabCoef {
    int c[9];
};

struct Gauss7 {
    float w[7];
};

__device__ __forceinline__ int refl101(int p, int n)
{
    // cv2.borderInterpolate(BORDER_REFLECT_101), repeated reflection for kernels wider than the image
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

__device__ __forceinline__ int clampi(int p, int n) { return p < 0 ? 0 : (p >= n ? n - 1 : p); }

__device__ __forceinline__ int gray_of(int r, int g, int b, int shift)
{
    return shift == 15 ? (r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15
                       : (r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14;
}

__device__ __forceinline__ int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// K exact sums of the block -> K integer atomics at dst (two's complement: signed sums come out right)
template <int K>
__device__ __forceinline__ void block_add_u64(const unsigned long long (&v)[K], unsigned long long *dst,
                                              unsigned long long (*red)[CM_THREADS / 64])
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        unsigned long long s = v[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (lane == 0) red[k][wv] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        unsigned long long s = 0;
        for (int w = 0; w < CM_THREADS / 64; ++w) s += red[threadIdx.x][w];
        if (s) atomicAdd(dst + threadIdx.x, s);
    }
}

// K fp64 sums of the block in a fixed tree order -> dst[0..K)
template <int K>
__device__ __forceinline__ void block_sum_f64(const double (&v)[K], double *dst, double (*red)[CM_THREADS / 64])
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = v[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (lane == 0) red[k][wv] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double s = 0.0;
        for (int w = 0; w < CM_THREADS / 64; ++w) s += red[threadIdx.x][w];
        dst[threadIdx.x] = s;
    }
}

// ---- 8-bit RGB2Lab tables (OpenCV 4.x color_lab.cpp, restated in tests/_commercial_ref.py lab_tables_b) -------------
__global__ void k_lab_tables(int *__restrict__ gamma_tab, int *__restrict__ cbrt_tab)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 256) {
        const double x = i / 255.0;
        const double v = x <= 0.04045 ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4);
        gamma_tab[i] = (int)rint(255.0 * 8.0 * v);
    }
    if (i < 3072) {
        const double x = i / (255.0 * 8.0);
        const double v = x < 216.0 / 24389.0 ? x * (841.0 / 108.0) + 16.0 / 116.0 : cbrt(x);
        cbrt_tab[i] = (int)rint(32768.0 * v);
    }
}

__device__ __forceinline__ void lab8(int r, int g, int b, const int *gt, const int *ct, const LabCoef &C, int &L, int &A,
                                     int &B)
{
    const int R = gt[r], G = gt[g], Bv = gt[b];
    const int fX = ct[(R * C.c[0] + G * C.c[1] + Bv * C.c[2] + (1 << 11)) >> 12];
    const int fY = ct[(R * C.c[3] + G * C.c[4] + Bv * C.c[5] + (1 << 11)) >> 12];
    const int fZ = ct[(R * C.c[6] + G * C.c[7] + Bv * C.c[8] + (1 << 11)) >> 12];
    const int Lshift = -((16 * 255 * (1 << 15) + 50) / 100);
    L = sat8((296 * fY + Lshift + (1 << 14)) >> 15);
    A = sat8((500 * (fX - fY) + 128 * (1 << 15) + (1 << 14)) >> 15);
    B = sat8((200 * (fY - fZ) + 128 * (1 << 15) + (1 << 14)) >> 15);
}

enum {
    CMF_LAPG = 1, CMF_NOISE = 2, CMF_SOBEL = 4, CMF_MSCN = 8, CMF_TEX = 16, CMF_LAB = 32, CMF_SKIN = 64, CMF_RGB = 128,
    CMF_BLOCKS = 256, CMF_REGIONS = 512, CMF_CANNY = 1024, CMF_HF = 2048
};
enum { NI = 40, NF = 8 };          // integer / fp64 result slots per rectangle (include/sr_hip.h)

// ---- colour pass ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CM_THREADS) void k_cm_color(const unsigned char *__restrict__ img, long long stride, int cn,
                                                         int gray_shift, const CmRect *__restrict__ rects,
                                                         unsigned char *__restrict__ gray, const int *__restrict__ gt,
                                                         const int *__restrict__ ct, LabCoef lc,
                                                         unsigned long long *__restrict__ ints)
{
    __shared__ unsigned long long red[10][CM_THREADS / 64];
    const CmRect R = rects[blockIdx.y];
    const bool wgray = blockIdx.y == 0 && gray != nullptr;
    const bool lab = R.flags & (CMF_LAB | CMF_SKIN), skin = R.flags & CMF_SKIN, rgb = R.flags & CMF_RGB;
    if (!wgray && !lab && !rgb) return;
    unsigned long long v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const long long n = (long long)R.w * R.h;
    for (long long p = (long long)blockIdx.x * CM_THREADS + threadIdx.x; p < n; p += (long long)gridDim.x * CM_THREADS) {
        const int y = (int)(p / R.w), x = (int)(p - (long long)y * R.w);
        const unsigned char *px = img + (long long)(R.y + y) * stride + (long long)(R.x + x) * cn;
        const int r = px[0], g = px[1], b = px[2];
        if (wgray) gray[p] = (unsigned char)gray_of(r, g, b, gray_shift);
        if (lab) {
            int L, A, B;
            lab8(r, g, b, gt, ct, lc, L, A, B);
            v[0] += L; v[1] += L * L; v[2] += A; v[3] += A * A; v[4] += B; v[5] += B * B;
        }
        if (skin) {
            const int Y = (r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14;
            const int Cr = sat8(((r - Y) * 11682 + (128 << 14) + (1 << 13)) >> 14);
            const int Cb = sat8(((b - Y) * 9241 + (128 << 14) + (1 << 13)) >> 14);
            v[6] += (Cr >= 133 && Cr <= 173 && Cb >= 77 && Cb <= 127) ? 1 : 0;
        }
        if (rgb) { v[7] += r; v[8] += g; v[9] += b; }
    }
    block_add_u64<10>(v, ints + (size_t)blockIdx.y * NI + 7, red);
}

// ---- stencil pass over the gray plane ---------------------------------------------------------------------------------
__global__ __launch_bounds__(CM_THREADS) void k_cm_stencil(const unsigned char *__restrict__ gp, long long gs,
                                                           const CmRect *__restrict__ rects, Gauss7 gk,
                                                           unsigned long long *__restrict__ ints, double *__restrict__ part)
{
    __shared__ unsigned long long redi[7][CM_THREADS / 64];
    __shared__ double redf[5][CM_THREADS / 64];
    const CmRect R = rects[blockIdx.y];
    const int F = R.flags;
    if (!(F & (CMF_LAPG | CMF_NOISE | CMF_SOBEL | CMF_MSCN | CMF_TEX))) return;
    const unsigned char *g0 = gp + (long long)R.y * gs + R.x;
    auto G = [&](int yy, int xx) -> int { return g0[(long long)refl101(yy, R.h) * gs + refl101(xx, R.w)]; };
    unsigned long long vi[7] = {0, 0, 0, 0, 0, 0, 0};
    double vf[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const long long n = (long long)R.w * R.h;
    for (long long p = (long long)blockIdx.x * CM_THREADS + threadIdx.x; p < n; p += (long long)gridDim.x * CM_THREADS) {
        const int y = (int)(p / R.w), x = (int)(p - (long long)y * R.w);
        const int c = G(y, x);
        if (F & CMF_LAPG) {
            const long long l = (long long)G(y - 1, x) + G(y + 1, x) + G(y, x - 1) + G(y, x + 1) - 4 * c;
            vi[0] += (unsigned long long)l;
            vi[1] += (unsigned long long)(l * l);
            vi[2] += c;
            vi[3] += (unsigned long long)(c * c);
        }
        if (F & (CMF_NOISE | CMF_SOBEL)) {
            int a[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) a[i][j] = G(y + i - 1, x + j - 1);
            if (F & CMF_NOISE) {
                const int b16 = (a[0][0] + 2 * a[0][1] + a[0][2]) + 2 * (a[1][0] + 2 * a[1][1] + a[1][2]) +
                                (a[2][0] + 2 * a[2][1] + a[2][2]);
                const long long nz = 16 * c - b16;
                vi[4] += (unsigned long long)nz;
                vi[5] += (unsigned long long)(nz * nz);
            }
            if (F & CMF_SOBEL) {
                const int gx = (a[0][2] - a[0][0]) + 2 * (a[1][2] - a[1][0]) + (a[2][2] - a[2][0]);
                const int gy = (a[2][0] - a[0][0]) + 2 * (a[2][1] - a[0][1]) + (a[2][2] - a[0][2]);
                const long long s2 = (long long)gx * gx + (long long)gy * gy;
                vi[6] += (unsigned long long)s2;
                vf[3] += sqrt((double)s2);
            }
        }
        if (F & CMF_TEX) {
            // cv2.blur(g, (5, 5)) and cv2.blur(g^2, (5, 5)) on float32: exact integer box sums scaled by 1/25 in double,
            // rounded to float; the local variance in float32 (no contraction)
            long long s = 0, s2 = 0;
            for (int i = -2; i <= 2; ++i)
                for (int j = -2; j <= 2; ++j) {
                    const int t = G(y + i, x + j);
                    s += t;
                    s2 += t * t;
                }
            const float bm = (float)((double)s * (1.0 / 25.0));
            const float bq = (float)((double)s2 * (1.0 / 25.0));
            const float lv = __fsub_rn(bq, __fmul_rn(bm, bm));
            vf[4] += (double)lv;
        }
        if (F & CMF_MSCN) {
            // GaussianBlur(., (7, 7), 7/6) of g and g^2 in float32: row pass (taps left to right, acc = acc + w * v)
            // then the same column pass over the row results; mscn = (g - mu) / (sqrt(max(E - mu^2, 0)) + 1)
            float mu = 0.0f, e2 = 0.0f;
            for (int i = 0; i < 7; ++i) {
                const long long roff = (long long)refl101(y + i - 3, R.h) * gs;
                float ra = 0.0f, rb = 0.0f;
                for (int j = 0; j < 7; ++j) {
                    const float t = (float)g0[roff + refl101(x + j - 3, R.w)];
                    ra = __fadd_rn(ra, __fmul_rn(gk.w[j], t));
                    rb = __fadd_rn(rb, __fmul_rn(gk.w[j], __fmul_rn(t, t)));
                }
                mu = __fadd_rn(mu, __fmul_rn(gk.w[i], ra));
                e2 = __fadd_rn(e2, __fmul_rn(gk.w[i], rb));
            }
            // sqrt and division through fp64: the fp32 result is the correctly rounded one whatever the fp32 lowering
            const float sg = (float)sqrt((double)fmaxf(__fsub_rn(e2, __fmul_rn(mu, mu)), 0.0f));
            const float m = (float)((double)__fsub_rn((float)c, mu) / (double)__fadd_rn(sg, 1.0f));
            vf[0] += (double)m;
            vf[1] += (double)m * (double)m;
            vf[2] += fabs((double)m);
        }
    }
    block_add_u64<7>(vi, ints + (size_t)blockIdx.y * NI, redi);
    block_sum_f64<5>(vf, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NF, redf);
}

// ---- _detect_artifacts: 8x8 blocks at range(0, h - 8, 8) x range(0, w - 8, 8) -----------------------------------------
__global__ __launch_bounds__(CM_THREADS) void k_cm_blocks(const unsigned char *__restrict__ gp, long long gs, int nby, int nbx,
                                                          unsigned long long *__restrict__ ints)
{
    __shared__ unsigned long long red[3][CM_THREADS / 64];
    unsigned long long v[3] = {0, 0, 0};
    const long long nb = (long long)nby * nbx;
    for (long long i = (long long)blockIdx.x * CM_THREADS + threadIdx.x; i < nb; i += (long long)gridDim.x * CM_THREADS) {
        const int by = (int)(i / nbx), bx = (int)(i - (long long)by * nbx);
        long long s = 0, s2 = 0;
        for (int r = 0; r < 8; ++r) {
            const unsigned char *row = gp + (long long)(by * 8 + r) * gs + bx * 8;
            for (int c = 0; c < 8; ++c) {
                const int t = row[c];
                s += t;
                s2 += t * t;
            }
        }
        const unsigned long long nv = (unsigned long long)(64 * s2 - s * s);   // 4096 * variance, < 2^27
        const unsigned long long sq = nv * nv;                                  // < 2^54
        v[0] += nv;
        v[1] += sq & 0xffffffffull;
        v[2] += sq >> 32;
    }
    block_add_u64<3>(v, ints + 17, red);
}

// ---- _calculate_brightness_uniformity: the 16 region sums (h // 4 x w // 4 regions, remainders excluded) -------------
__global__ __launch_bounds__(CM_THREADS) void k_cm_regions(const unsigned char *__restrict__ gp, long long gs, int rh, int rw,
                                                           unsigned long long *__restrict__ ints)
{
    __shared__ unsigned long long red[1][CM_THREADS / 64];
    const int reg = blockIdx.y, ri = reg >> 2, rj = reg & 3;
    unsigned long long v[1] = {0};
    for (int r = blockIdx.x; r < rh; r += gridDim.x) {
        const unsigned char *row = gp + (long long)(ri * rh + r) * gs + rj * rw;
        for (int c = threadIdx.x; c < rw; c += CM_THREADS) v[0] += row[c];
    }
    block_add_u64<1>(v, ints + 20 + reg, red);
}

// ---- Canny ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sobel_rep(const unsigned char *gp, long long gs, int H, int W, int y, int x, int &dx, int &dy)
{
    int a[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const long long ro = (long long)clampi(y + i - 1, H) * gs;
#pragma unroll
        for (int j = 0; j < 3; ++j) a[i][j] = gp[ro + clampi(x + j - 1, W)];
    }
    dx = (a[0][2] - a[0][0]) + 2 * (a[1][2] - a[1][0]) + (a[2][2] - a[2][0]);
    dy = (a[2][0] - a[0][0]) + 2 * (a[2][1] - a[0][1]) + (a[2][2] - a[0][2]);
}

__global__ __launch_bounds__(CM_THREADS) void k_canny_mag(const unsigned char *__restrict__ gp, long long gs, int H, int W,
                                                          short *__restrict__ mag)
{
    const long long n = (long long)H * W;
    for (long long p = (long long)blockIdx.x * CM_THREADS + threadIdx.x; p < n; p += (long long)gridDim.x * CM_THREADS) {
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        int dx, dy;
        sobel_rep(gp, gs, H, W, y, x, dx, dy);
        mag[p] = (short)(abs(dx) + abs(dy));
    }
}

// state: 0 no edge, 1 candidate (survives NMS, m > low), 2 edge (candidate with m > high, or connected to one)
__global__ __launch_bounds__(CM_THREADS) void k_canny_nms(const unsigned char *__restrict__ gp, long long gs, int H, int W,
                                                          const short *__restrict__ mag, int low, int high,
                                                          unsigned char *__restrict__ st)
{
    const long long n = (long long)H * W;
    auto M = [&](int yy, int xx) -> int {
        return (yy < 0 || yy >= H || xx < 0 || xx >= W) ? 0 : mag[(long long)yy * W + xx];
    };
    for (long long p = (long long)blockIdx.x * CM_THREADS + threadIdx.x; p < n; p += (long long)gridDim.x * CM_THREADS) {
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        const int m = mag[p];
        unsigned char s = 0;
        if (m > low) {
            int xs, ys;
            sobel_rep(gp, gs, H, W, y, x, xs, ys);
            const long long ax = abs(xs), ay = (long long)abs(ys) << 15;
            const long long tg22x = ax * 13573;                 // TG22 = round(0.4142135623730950488 * 2^15)
            bool keep;
            if (ay < tg22x) {
                keep = m > M(y, x - 1) && m >= M(y, x + 1);
            } else {
                const long long tg67x = tg22x + (ax << 16);
                if (ay > tg67x) {
                    keep = m > M(y - 1, x) && m >= M(y + 1, x);
                } else {
                    const int sg = (xs ^ ys) < 0 ? -1 : 1;
                    keep = m > M(y - 1, x - sg) && m > M(y + 1, x + sg);
                }
            }
            if (keep) s = m > high ? 2 : 1;
        }
        st[p] = s;
    }
}

// One hysteresis sweep: every 32x32 tile floods edge state through its candidates inside LDS until it settles (the
// one-pixel halo is read from the neighbours as they are); flags[sweep] is set when any pixel changed.  A sweep whose
// predecessor changed nothing returns at once, so a batch of sweeps can be enqueued ahead of the flag readback.
__global__ __launch_bounds__(CM_THREADS) void k_canny_sweep(unsigned char *__restrict__ st, int H, int W,
                                                            int *__restrict__ flags, int sweep)
{
    if (sweep > 0 && flags[sweep - 1] == 0) return;
    __shared__ unsigned char t[CN_TS + 2][CN_TS + 2];
    __shared__ int ch;
    const int x0 = blockIdx.x * CN_TS, y0 = blockIdx.y * CN_TS;
    for (int e = threadIdx.x; e < (CN_TS + 2) * (CN_TS + 2); e += CM_THREADS) {
        const int ly = e / (CN_TS + 2), lx = e - ly * (CN_TS + 2);
        const int y = y0 + ly - 1, x = x0 + lx - 1;
        t[ly][lx] = (y < 0 || y >= H || x < 0 || x >= W) ? 0 : st[(long long)y * W + x];
    }
    bool any = false;
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) ch = 0;
        __syncthreads();
        bool mine = false;
        for (int e = threadIdx.x; e < CN_TS * CN_TS; e += CM_THREADS) {
            const int ly = e / CN_TS + 1, lx = e % CN_TS + 1;
            if (t[ly][lx] != 1) continue;
            if (t[ly - 1][lx - 1] == 2 || t[ly - 1][lx] == 2 || t[ly - 1][lx + 1] == 2 || t[ly][lx - 1] == 2 ||
                t[ly][lx + 1] == 2 || t[ly + 1][lx - 1] == 2 || t[ly + 1][lx] == 2 || t[ly + 1][lx + 1] == 2) {
                t[ly][lx] = 2;
                mine = true;
            }
        }
        if (mine) ch = 1;
        __syncthreads();
        if (!ch) break;
        any = true;
    }
    if (!any) return;                        // uniform across the block: every thread saw the same ch sequence
    for (int e = threadIdx.x; e < CN_TS * CN_TS; e += CM_THREADS) {
        const int ly = e / CN_TS, lx = e % CN_TS;
        const int y = y0 + ly, x = x0 + lx;
        if (y < H && x < W && t[ly + 1][lx + 1] == 2) {
            unsigned char *q = st + (long long)y * W + x;
            if (*q != 2) *q = 2;
        }
    }
    if (threadIdx.x == 0) flags[sweep] = 1;
}

__global__ __launch_bounds__(CM_THREADS) void k_canny_count(const unsigned char *__restrict__ st, long long n,
                                                            unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long red[1][CM_THREADS / 64];
    unsigned long long v[1] = {0};
    for (long long p = (long long)blockIdx.x * CM_THREADS + threadIdx.x; p < n; p += (long long)gridDim.x * CM_THREADS)
        v[0] += st[p] == 2;
    block_add_u64<1>(v, out, red);
}

// ---- FFT ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float2 cmul(float2 a, float2 b)
{
    return make_float2(__fsub_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fadd_rn(__fmul_rn(a.x, b.y), __fmul_rn(a.y, b.x)));
}

__global__ void k_twiddle(float2 *__restrict__ tw, int n)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < n) {
        double s, c;
        sincospi(-2.0 * (double)m / (double)n, &s, &c);
        tw[m] = make_float2((float)c, (float)s);
    }
}

// One Stockham autosort pass of radix R over `lines` lines of length N (Ns: product of the radices already applied):
// butterfly j (k = j mod Ns) reads in[j + r N/R], twiddles by W_{Ns R}^{r k}, takes the R-point DFT and writes
// out[(j / Ns) Ns R + k + q Ns].  A block holds nb = max(1, 256 / R) butterflies in LDS; W_R comes from LDS too.
// COMP: the R-term sums carry a Kahan compensation term (the saliency map's long direct-DFT passes; the metrics keep the
// plain sums their recorded values were taken with).
template <bool COMP>
__global__ __launch_bounds__(CM_THREADS) void k_fft_pass(const float2 *__restrict__ in, float2 *__restrict__ out,
                                                         long long lines, int N, int R, int Ns, const float2 *__restrict__ tw)
{
    __shared__ float2 v[CM_MAX_RADIX > CM_THREADS ? CM_MAX_RADIX : CM_THREADS];
    __shared__ float2 wr[CM_MAX_RADIX];
    const int nb = R >= CM_THREADS ? 1 : CM_THREADS / R;
    const int NR = N / R;
    const long long total = lines * NR;
    const long long g0 = (long long)blockIdx.x * nb;
    for (int i = threadIdx.x; i < R; i += CM_THREADS) wr[i] = tw[(long long)i * NR];
    const int span = N / (Ns * R);
    for (int e = threadIdx.x; e < nb * R; e += CM_THREADS) {
        const int r = e / nb, b = e - r * nb;
        const long long g = g0 + b;
        float2 val = make_float2(0.0f, 0.0f);
        if (g < total) {
            const long long line = g / NR;
            const int j = (int)(g - line * NR), k = j % Ns;
            val = in[line * N + j + (long long)r * NR];
            if (r && k) val = cmul(val, tw[(long long)r * k * span]);
        }
        v[e] = val;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nb * R; e += CM_THREADS) {
        const int q = e / nb, b = e - q * nb;
        const long long g = g0 + b;
        if (g >= total) continue;
        float2 acc = make_float2(0.0f, 0.0f), lost = make_float2(0.0f, 0.0f);
        int idx = 0;
        for (int r = 0; r < R; ++r) {
            const float2 p = cmul(v[r * nb + b], wr[idx]);
            if (COMP) {
                const float yx = __fsub_rn(p.x, lost.x), yy = __fsub_rn(p.y, lost.y);
                const float tx = __fadd_rn(acc.x, yx), ty = __fadd_rn(acc.y, yy);
                lost.x = __fsub_rn(__fsub_rn(tx, acc.x), yx);
                lost.y = __fsub_rn(__fsub_rn(ty, acc.y), yy);
                acc.x = tx;
                acc.y = ty;
            } else {
                acc.x = __fadd_rn(acc.x, p.x);
                acc.y = __fadd_rn(acc.y, p.y);
            }
            idx += q;
            if (idx >= R) idx -= R;
        }
        const long long line = g / NR;
        const int j = (int)(g - line * NR), k = j % Ns;
        out[line * N + (long long)(j / Ns) * Ns * R + k + (long long)q * Ns] = acc;
    }
}

// Bluestein: chirp w[n] = exp(-i pi (n^2 mod 2N) / N)
__global__ void k_chirp(float2 *__restrict__ w, int N)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < N) {
        const long long nn = ((long long)n * n) % (2LL * N);
        double s, c;
        sincospi(-(double)nn / (double)N, &s, &c);
        w[n] = make_float2((float)c, (float)s);
    }
}

__global__ void k_blu_b(float2 *__restrict__ b, const float2 *__restrict__ w, int N, int M)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float2 v = make_float2(0.0f, 0.0f);
    if (m < N) v = make_float2(w[m].x, -w[m].y);
    else if (m > M - N) v = make_float2(w[M - m].x, -w[M - m].y);
    b[m] = v;
}

__global__ void k_blu_pre(const float2 *__restrict__ x, int N, float2 *__restrict__ a, int M, long long lines,
                          const float2 *__restrict__ w)
{
    const long long total = lines * M;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long l = e / M;
        const int m = (int)(e - l * M);
        a[e] = m < N ? cmul(x[l * N + m], w[m]) : make_float2(0.0f, 0.0f);
    }
}

__global__ void k_blu_mul(float2 *__restrict__ a, const float2 *__restrict__ bf, int M, long long lines)
{
    const long long total = lines * M;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const float2 p = cmul(a[e], bf[e % M]);
        a[e] = make_float2(p.x, -p.y);
    }
}

__global__ void k_blu_post(const float2 *__restrict__ a, int M, float2 *__restrict__ X, int N, long long lines,
                           const float2 *__restrict__ w)
{
    const long long total = lines * N;
    const float inv = 1.0f / (float)M;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long l = e / N;
        const int k = (int)(e - l * N);
        const float2 c = a[l * M + k];
        const float2 p = cmul(w[k], make_float2(__fmul_rn(c.x, inv), __fmul_rn(-c.y, inv)));
        X[e] = p;
    }
}

// rows 2i and 2i + 1 of the gray plane as the real and imaginary part of complex line i
__global__ void k_pack_rows(const unsigned char *__restrict__ gp, long long gs, int H, int W, float2 *__restrict__ out)
{
    const long long lines = (H + 1) / 2, total = lines * W;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long i = e / W;
        const int x = (int)(e - i * W);
        const float re = gp[(2 * i) * gs + x];
        const float im = 2 * i + 1 < H ? (float)gp[(2 * i + 1) * gs + x] : 0.0f;
        out[e] = make_float2(re, im);
    }
}

// Z (lines x W, line i = FFT(row 2i + i row 2i+1)) -> T (Wh x H): T[k][2i] = A_k, T[k][2i+1] = B_k with
// A_k = (Z_k + conj Z_{W-k}) / 2, B_k = (Z_k - conj Z_{W-k}) / 2i; 32 lines x 32 columns per block through LDS.
__global__ __launch_bounds__(256) void k_split_transpose(const float2 *__restrict__ Z, int W, int lines, int H, int Wh,
                                                         float2 *__restrict__ T)
{
    __shared__ float2 s[32][65];
    const int i0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int il = ty; il < 32; il += 8) {
        const int i = i0 + il, k = k0 + tx;
        if (i < lines && k < Wh) {
            const float2 z = Z[(long long)i * W + k];
            const float2 zc = Z[(long long)i * W + (k == 0 ? 0 : W - k)];
            const float2 A = make_float2(__fmul_rn(__fadd_rn(z.x, zc.x), 0.5f), __fmul_rn(__fsub_rn(z.y, zc.y), 0.5f));
            // Z - conj(Zc) = (z.x - zc.x) + i (z.y + zc.y); divided by 2i
            const float2 B = make_float2(__fmul_rn(__fadd_rn(z.y, zc.y), 0.5f), __fmul_rn(__fsub_rn(zc.x, z.x), 0.5f));
            s[tx][2 * il] = A;
            s[tx][2 * il + 1] = B;
        }
    }
    __syncthreads();
    for (int kl = ty; kl < 32; kl += 8) {
        const int k = k0 + kl;
        if (k >= Wh) continue;
        for (int e = tx; e < 64; e += 32) {
            const int row = 2 * i0 + e;
            if (row < H && i0 + e / 2 < lines) T[(long long)k * H + row] = s[kl][e];
        }
    }
}

// sum |F| over the half spectrum (Hermitian weight 2 except the self-conjugate columns), total and outside the radius
__global__ __launch_bounds__(CM_THREADS) void k_hf_reduce(const float2 *__restrict__ F, int Wh, int H, int W, long long r2,
                                                          double *__restrict__ part)
{
    __shared__ double red[2][CM_THREADS / 64];
    double v[2] = {0.0, 0.0};
    const long long total = (long long)Wh * H;
    for (long long e = (long long)blockIdx.x * CM_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * CM_THREADS) {
        const int k = (int)(e / H), u = (int)(e - (long long)k * H);
        const float2 f = F[e];
        const double m = (double)(float)sqrt((double)__fadd_rn(__fmul_rn(f.x, f.x), __fmul_rn(f.y, f.y)));
        const double wt = (k == 0 || 2 * k == W) ? 1.0 : 2.0;
        const long long dy = (long long)((u + H / 2) % H) - H / 2, dx = (long long)((k + W / 2) % W) - W / 2;
        v[0] += wt * m;
        if (dx * dx + dy * dy > r2) v[1] += wt * m;
    }
    block_sum_f64<2>(v, part + (size_t)blockIdx.x * 2, red);
}

// ---- host side --------------------------------------------------------------------------------------------------------
std::vector<int> factor(int n)
{
    std::vector<int> f;
    for (int p = 2; (long long)p * p <= n; ++p)
        while (n % p == 0) {
            f.push_back(p);
            n /= p;
        }
    if (n > 1) f.push_back(n);
    return f;
}

// prime factors in ascending order, neighbours merged while the product stays <= 32
std::vector<int> radices(int n)
{
    std::vector<int> out;
    int cur = 1;
    for (int p : factor(n)) {
        if (cur * p <= 32) {
            cur *= p;
        } else {
            if (cur > 1) out.push_back(cur);
            cur = p;
        }
    }
    if (cur > 1) out.push_back(cur);
    return out;
}

bool needs_bluestein(int n)
{
    const std::vector<int> f = factor(n);
    return !f.empty() && f.back() > CM_MAX_RADIX;
}

int blu_len(int n)
{
    int m = 1;
    while (m < 2 * n - 1) m <<= 1;
    return m;
}

unsigned grid1(long long n, int per = 256, long long cap = 1 << 16)
{
    return (unsigned)std::max(1LL, std::min((n + per - 1) / per, cap));
}

// Stockham passes over `lines` lines of length n: ping-pong a <-> b, returns the buffer holding the result
float2 *run_passes(sr_ctx *ctx, float2 *a, float2 *b, long long lines, int n, const float2 *tw, bool comp = false)
{
    int Ns = 1;
    for (int R : radices(n)) {
        const int nb = R >= CM_THREADS ? 1 : CM_THREADS / R;
        const long long total = lines * (n / R);
        // compensated sums where the sum is long (a merged radix of up to 32 terms gains nothing from them)
        auto pass = comp && R > 32 ? k_fft_pass<true> : k_fft_pass<false>;
        hipLaunchKernelGGL(pass, dim3((unsigned)((total + nb - 1) / nb)), dim3(CM_THREADS), 0, ctx->stream,
                           (const float2 *)a, b, lines, n, R, Ns, tw);
        std::swap(a, b);
        Ns *= R;
    }
    return a;
}

// Table space fft_lines needs for length n (float2 elements)
size_t fft_tab_elems(int n)
{
    if (!needs_bluestein(n)) return (size_t)n;
    const int M = blu_len(n);
    return (size_t)n + (size_t)M + (size_t)n + 2 * (size_t)M;
}

// Line length of the work buffers for length n
size_t fft_work_len(int n) { return needs_bluestein(n) ? (size_t)blu_len(n) : (size_t)n; }

// Forward DFT of `lines` lines of length n held in X; P, Q are work buffers of lines * fft_work_len(n) elements, tab of
// fft_tab_elems(n).  Returns the buffer with the result (X or P).
float2 *fft_lines(sr_ctx *ctx, float2 *X, float2 *P, float2 *Q, float2 *tab, long long lines, int n, bool comp = false)
{
    if (n == 1) return X;
    if (!needs_bluestein(n)) {
        hipLaunchKernelGGL(k_twiddle, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, tab, n);
        return run_passes(ctx, X, P, lines, n, tab, comp);
    }
    const int M = blu_len(n);
    float2 *twM = tab, *w = twM + M, *bA = w + n, *bB = bA + M;
    hipLaunchKernelGGL(k_twiddle, dim3((M + 255) / 256), dim3(256), 0, ctx->stream, twM, M);
    hipLaunchKernelGGL(k_chirp, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, w, n);
    hipLaunchKernelGGL(k_blu_b, dim3((M + 255) / 256), dim3(256), 0, ctx->stream, bA, (const float2 *)w, n, M);
    const float2 *bf = run_passes(ctx, bA, bB, 1, M, twM);
    hipLaunchKernelGGL(k_blu_pre, dim3(grid1(lines * M)), dim3(256), 0, ctx->stream, (const float2 *)X, n, P, M, lines,
                       (const float2 *)w);
    float2 *r = run_passes(ctx, P, Q, lines, M, twM);
    hipLaunchKernelGGL(k_blu_mul, dim3(grid1(lines * M)), dim3(256), 0, ctx->stream, r, bf, M, lines);
    r = run_passes(ctx, r, r == P ? Q : P, lines, M, twM);
    hipLaunchKernelGGL(k_blu_post, dim3(grid1(lines * n)), dim3(256), 0, ctx->stream, (const float2 *)r, M, X, n, lines,
                       (const float2 *)w);
    return X;
}

LabCoef lab_coeffs()
{
    // cvRound(2^12 * sRGB2XYZ_D65[i][j] / D65[i]), RGB order
    static const double m[9] = {0.412453, 0.357580, 0.180423, 0.212671, 0.715160, 0.072169, 0.019334, 0.119193, 0.950227};
    static const double wp[3] = {0.950456, 1.0, 1.088754};
    LabCoef c;
    for (int i = 0; i < 9; ++i) c.c[i] = (int)std::nearbyint(4096.0 * m[i] / wp[i / 3]);
    return c;
}

Gauss7 gauss7()
{
    // cv2.getGaussianKernel(7, 7/6): exp(-(i - 3)^2 / (2 sigma^2)) normalised in fp64, rounded to float -- spelled out so
    // no compiler's constant folding of exp can move a bit (tests/test_commercial_host.py checks them against the rule)
    static const float k[7] = {0x1.9b929ap-7f, 0x1.42e11cp-4f, 0x1.e5fb7cp-3f, 0x1.5edaccp-2f, 0x1.e5fb7cp-3f,
                               0x1.42e11cp-4f, 0x1.9b929ap-7f};
    Gauss7 g;
    for (int i = 0; i < 7; ++i) g.w[i] = k[i];
    return g;
}

int cm_workspace(sr_ctx *ctx, size_t bytes, char **out)
{
    SRCHK(ctx->cm_ws.reserve(ctx, "commercial / FFT workspace", bytes));
    *out = ctx->cm_ws.as<char>();
    return SR_OK;
}

}  // namespace

// the line engine for the other translation units (sr_fft.h)
size_t sr_fft_tab_elems(int n) { return fft_tab_elems(n); }
size_t sr_fft_work_len(int n) { return fft_work_len(n); }
float2 *sr_fft_lines(sr_ctx *ctx, float2 *X, float2 *P, float2 *Q, float2 *tab, long long lines, int n, bool comp)
{
    return fft_lines(ctx, X, P, Q, tab, lines, n, comp);
}
int sr_fft_workspace(sr_ctx *ctx, size_t bytes, char **out) { return cm_workspace(ctx, bytes, out); }

int sr_fft_max_len(void) { return CM_MAX_LEN; }

int sr_fft_c2c(sr_ctx *ctx, const void *d_in, void *d_out, int64_t lines, int n)
{
    CTX_ENTER(ctx);
    if (!d_in || !d_out || lines < 1 || n < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_fft_c2c: bad arguments");
    if (n > CM_MAX_LEN) return sr_set_error(SR_ERR_UNSUPPORTED, "sr_fft_c2c: length %d above %d", n, CM_MAX_LEN);
    const size_t xb = up256((size_t)lines * n * 8), wb = up256((size_t)lines * fft_work_len(n) * 8),
                 tb = up256(fft_tab_elems(n) * 8);
    char *ws = nullptr;
    SRCHK(cm_workspace(ctx, xb + 2 * wb + tb, &ws));
    float2 *X = (float2 *)ws, *P = (float2 *)(ws + xb), *Q = (float2 *)(ws + xb + wb), *T = (float2 *)(ws + xb + 2 * wb);
    HIPCHK(hipMemcpyAsync(X, d_in, (size_t)lines * n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    float2 *r;
    {
        ProfScope ps(ctx, "cm_fft");
        r = fft_lines(ctx, X, P, Q, T, lines, n);
    }
    SRCHK(check_launch("fft_c2c"));
    HIPCHK(hipMemcpyAsync(d_out, r, (size_t)lines * n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_commercial_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, int gray_shift, int flags,
                     const sr_tile_rect *h_rois, const int *h_roi_flags, int n_roi, int64_t *h_ints, double *h_flts)
{
    CTX_ENTER(ctx);
    if (!d_img || !h_ints || !h_flts || h < 1 || w < 1 || (cn != 1 && cn != 3 && cn != 4) || n_roi < 0 ||
        (n_roi > 0 && (!h_rois || !h_roi_flags)) || (gray_shift != 14 && gray_shift != 15) || (flags & ~4095))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_commercial_u8: bad arguments");
    if (stride < (int64_t)w * cn) return sr_set_error(SR_ERR_SHAPE, "sr_commercial_u8: stride smaller than a row");
    if ((flags & CMF_HF) && (h > CM_MAX_LEN || w > CM_MAX_LEN))
        return sr_set_error(SR_ERR_UNSUPPORTED, "sr_commercial_u8: DFT side above %d", CM_MAX_LEN);
    if ((long long)h * w > (1LL << 31)) return sr_set_error(SR_ERR_SHAPE, "sr_commercial_u8: image above 2^31 pixels");
    const int nr = 1 + n_roi;
    std::vector<CmRect> rects(nr);
    const int colour_flags = CMF_LAB | CMF_SKIN | CMF_RGB;
    rects[0] = {0, 0, w, h, flags & (CMF_LAPG | CMF_NOISE | CMF_SOBEL | CMF_MSCN | CMF_TEX | colour_flags)};
    for (int i = 0; i < n_roi; ++i) {
        const sr_tile_rect &r = h_rois[i];
        if (r.w < 1 || r.h < 1 || r.x < 0 || r.y < 0 || r.x + (long long)r.w > w || r.y + (long long)r.h > h ||
            (h_roi_flags[i] & ~(CMF_LAPG | CMF_TEX | colour_flags)))
            return sr_set_error(SR_ERR_INVALID_ARG, "sr_commercial_u8: ROI %d is not a non-empty rectangle inside the image "
                                "or asks for a whole-image metric", i);
        rects[1 + i] = {r.x, r.y, r.w, r.h, h_roi_flags[i]};
    }
    if (cn == 1)
        for (auto &r : rects) r.flags &= ~colour_flags;    // 2-D images: the host reports the reference's constants
    bool colour = cn >= 3;                                 // the gray plane has to be made
    bool lab = false;
    for (auto &r : rects) lab = lab || (r.flags & (CMF_LAB | CMF_SKIN));

    // workspace layout
    const long long npx = (long long)h * w;
    const int lines_r = (h + 1) / 2, Wh = w / 2 + 1;
    size_t fft_buf = 0, fft_tab = 0;
    if (flags & CMF_HF) {
        fft_buf = std::max((size_t)lines_r * fft_work_len(w), (size_t)Wh * fft_work_len(h));
        fft_tab = std::max(fft_tab_elems(w), fft_tab_elems(h));
    }
    const size_t b_ints = up256((size_t)nr * NI * 8), b_part = up256((size_t)nr * CM_NBLK * NF * 8),
                 b_rect = up256(sizeof(CmRect) * nr), b_lab = up256((256 + 3072) * 4), b_hf = up256((size_t)CM_NBLK * 2 * 8),
                 b_flag = 256, b_gray = colour ? up256((size_t)npx) : 0,
                 b_mag = (flags & CMF_CANNY) ? up256((size_t)npx * 2) : 0, b_st = (flags & CMF_CANNY) ? up256((size_t)npx) : 0,
                 b_fft = up256(fft_buf * 8), b_tab = up256(fft_tab * 8);
    char *ws = nullptr;
    int rc = cm_workspace(ctx, b_ints + b_part + b_rect + b_lab + b_hf + b_flag + b_gray + b_mag + b_st + 3 * b_fft + b_tab, &ws);
    if (rc) return rc;
    char *p = ws;
    auto take = [&](size_t b) { char *q = p; p += b; return q; };
    unsigned long long *d_ints = (unsigned long long *)take(b_ints);
    double *d_part = (double *)take(b_part);
    CmRect *d_rect = (CmRect *)take(b_rect);
    int *d_gt = (int *)take(b_lab), *d_ct = d_gt + 256;
    double *d_hf = (double *)take(b_hf);
    int *d_flag = (int *)take(b_flag);
    unsigned char *d_gray = (unsigned char *)take(b_gray);
    short *d_mag = (short *)take(b_mag);
    unsigned char *d_st = (unsigned char *)take(b_st);
    float2 *F0 = (float2 *)take(b_fft), *F1 = (float2 *)take(b_fft), *F2 = (float2 *)take(b_fft), *d_tab = (float2 *)take(b_tab);

    HIPCHK(hipMemsetAsync(d_ints, 0, (size_t)nr * NI * 8, ctx->stream));
    HIPCHK(hipMemsetAsync(d_part, 0, (size_t)nr * CM_NBLK * NF * 8, ctx->stream));
    HIPCHK(upload_small(ctx, d_rect, rects.data(), sizeof(CmRect) * nr));
    const unsigned char *gp = colour ? d_gray : d_img;
    const long long gs = colour ? w : stride;

    if (colour) {
        ProfScope ps(ctx, "cm_color");
        if (lab) hipLaunchKernelGGL(k_lab_tables, dim3(12), dim3(256), 0, ctx->stream, d_gt, d_ct);
        hipLaunchKernelGGL(k_cm_color, dim3(CM_NBLK, nr), dim3(CM_THREADS), 0, ctx->stream, d_img, (long long)stride, cn,
                           gray_shift, (const CmRect *)d_rect, d_gray, (const int *)d_gt, (const int *)d_ct, lab_coeffs(),
                           d_ints);
    }
    {
        ProfScope ps(ctx, "cm_stencil");
        hipLaunchKernelGGL(k_cm_stencil, dim3(CM_NBLK, nr), dim3(CM_THREADS), 0, ctx->stream, gp, gs, (const CmRect *)d_rect,
                           gauss7(), d_ints, d_part);
    }
    if (flags & CMF_BLOCKS) {
        const int nby = h > 8 ? (h - 8 + 7) / 8 : 0, nbx = w > 8 ? (w - 8 + 7) / 8 : 0;
        h_ints[38] = (int64_t)nby * nbx;
        if (nby > 0 && nbx > 0) {
            ProfScope ps(ctx, "cm_blocks");
            hipLaunchKernelGGL(k_cm_blocks, dim3(grid1((long long)nby * nbx, CM_THREADS, 2048)), dim3(CM_THREADS), 0,
                               ctx->stream, gp, gs, nby, nbx, d_ints);
        }
    }
    if ((flags & CMF_REGIONS) && h >= 4 && w >= 4) {
        ProfScope ps(ctx, "cm_regions");
        hipLaunchKernelGGL(k_cm_regions, dim3(std::min(h / 4, 64), 16), dim3(CM_THREADS), 0, ctx->stream, gp, gs, h / 4, w / 4,
                           d_ints);
    }
    int sweeps = 0;
    if (flags & CMF_CANNY) {
        {
            ProfScope ps(ctx, "cm_canny_nms");
            hipLaunchKernelGGL(k_canny_mag, dim3(grid1(npx, CM_THREADS, 8192)), dim3(CM_THREADS), 0, ctx->stream, gp, gs, h, w,
                               d_mag);
            hipLaunchKernelGGL(k_canny_nms, dim3(grid1(npx, CM_THREADS, 8192)), dim3(CM_THREADS), 0, ctx->stream, gp, gs, h, w,
                               (const short *)d_mag, 50, 150, d_st);
        }
        const dim3 tg((w + CN_TS - 1) / CN_TS, (h + CN_TS - 1) / CN_TS);
        for (;;) {
            ProfScope ps(ctx, "cm_canny_sweep");
            HIPCHK(hipMemsetAsync(d_flag, 0, CN_BATCH * sizeof(int), ctx->stream));
            for (int s = 0; s < CN_BATCH; ++s)
                hipLaunchKernelGGL(k_canny_sweep, tg, dim3(CM_THREADS), 0, ctx->stream, d_st, h, w, d_flag, s);
            rc = check_launch("canny_sweep");
            if (rc) return rc;
            int fl[CN_BATCH];
            HIPCHK(hipMemcpyAsync(fl, d_flag, sizeof(fl), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(stream_sync(ctx));
            int done = 0;
            while (done < CN_BATCH && fl[done]) ++done;
            sweeps += done + (done < CN_BATCH ? 1 : 0);
            if (!fl[CN_BATCH - 1]) break;
            if (sweeps > (1 << 22)) return sr_set_error(SR_ERR_HIP, "sr_commercial_u8: Canny hysteresis did not settle");
        }
        ProfScope ps(ctx, "cm_canny_count");
        hipLaunchKernelGGL(k_canny_count, dim3(grid1(npx, CM_THREADS, 4096)), dim3(CM_THREADS), 0, ctx->stream,
                           (const unsigned char *)d_st, npx, d_ints + 36);
    }
    if (flags & CMF_HF) {
        ProfScope ps(ctx, "cm_hf");
        hipLaunchKernelGGL(k_pack_rows, dim3(grid1((long long)lines_r * w)), dim3(256), 0, ctx->stream, gp, gs, h, w, F0);
        float2 *r = fft_lines(ctx, F0, F1, F2, d_tab, lines_r, w);
        float2 *T = r == F0 ? F1 : F0, *o1 = r == F0 ? F0 : F1;
        hipLaunchKernelGGL(k_split_transpose, dim3((Wh + 31) / 32, (lines_r + 31) / 32), dim3(256), 0, ctx->stream,
                           (const float2 *)r, w, lines_r, h, Wh, T);
        float2 *c = fft_lines(ctx, T, o1, F2, d_tab, Wh, h);
        const long long rad = std::min(h, w) / 4;
        hipLaunchKernelGGL(k_hf_reduce, dim3(CM_NBLK), dim3(CM_THREADS), 0, ctx->stream, (const float2 *)c, Wh, h, w, rad * rad,
                           d_hf);
    }
    rc = check_launch("commercial");
    if (rc) return rc;
    std::vector<unsigned long long> ints((size_t)nr * NI);
    std::vector<double> part((size_t)nr * CM_NBLK * NF), hf(flags & CMF_HF ? CM_NBLK * 2 : 0);
    HIPCHK(hipMemcpyAsync(ints.data(), d_ints, ints.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(part.data(), d_part, part.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (!hf.empty()) HIPCHK(hipMemcpyAsync(hf.data(), d_hf, hf.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    const int64_t nblocks = h_ints[38];
    for (size_t i = 0; i < ints.size(); ++i) h_ints[i] = (int64_t)ints[i];
    h_ints[37] = sweeps;
    h_ints[38] = (flags & CMF_BLOCKS) ? nblocks : 0;
    for (int r = 0; r < nr; ++r)
        for (int k = 0; k < NF; ++k) {
            double s = 0.0;
            for (int b = 0; b < CM_NBLK; ++b) s += part[((size_t)r * CM_NBLK + b) * NF + k];
            h_flts[(size_t)r * NF + k] = s;
        }
    if (!hf.empty()) {
        double t = 0.0, o = 0.0;
        for (int b = 0; b < CM_NBLK; ++b) {
            t += hf[2 * b];
            o += hf[2 * b + 1];
        }
        h_flts[6] = t;
        h_flts[5] = o;
    }
    return SR_OK;
}
