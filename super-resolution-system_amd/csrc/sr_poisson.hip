// sr_poisson.hip -- BlendingModule.poisson_fusion / repair_seams (blending_module.py:563-659, 1148-1240 of the reference) on
// gfx950: the Poisson solve behind cv2.seamlessClone on one rectangle, and the three small helpers seam repair needs.
//
// PARITY UNPINNED: cv2 is not available to this repository's tests.  What follows restates OpenCV's Cloning::normalClone
// (photo/src/seamless_cloning_impl.cpp), cv2.GaussianBlur's 8-bit fixed-point path and cv2.resize from memory; the tests
// hold the kernels against this repository's own NumPy / SciPy restatement of the same text (tests/_poisson_ref.py).
//
//   k_ps_mask     eroded mask plane: (mask != 0) under a 7 x 7 minimum (three 3 x 3 erosions); outside the ROI nothing erodes
//   k_ps_lambda   the DST-I eigenvalues 2 cos(pi (k + 1) / (n + 1)) - 2 = -4 sin^2(pi (k + 1) / (2 (n + 1))) in fp64
//   k_ps_rhs      per interior pixel the divergence of the mixed gradient field minus the boundary term -- every term is a
//                 small integer, exact in fp32; the field at (x, y), (x - 1, y), (x, y - 1) is formed in registers from the
//                 three u8 inputs, no gradient plane exists.  Channels 0 and 1 travel as the real and imaginary part of one
//                 complex plane, channel 2 as the real part of a second: the DST is real and linear, so two complex planes
//                 carry the three channels through all four transforms.  Written as odd-extended lines of length 2 (n + 1).
//   sr_fft_lines  rows: the forward DFT of the odd extension is -2i DST-I, so DST-I = (i / 2) F
//   k_ps_xpose    takes (i / 2) F[1..n], transposes through a 32 x 32 LDS tile and writes the odd extension along the other axis
//   sr_fft_lines  columns
//   k_ps_eig      (i / 2) F, divided by (lambda_x + lambda_y) (w - 1) (h - 1) / 4 (the scale of the two inverse DST-I folded
//                 into the divisor), odd-extended again in place of the column lines
//   sr_fft_lines  columns, k_ps_xpose back, sr_fft_lines rows
//   k_ps_final    (i / 2) F -> saturate(round-half-even) into the interior; the 1-pixel frame is the destination's
// Every sum has a fixed order (the FFT passes, no atomics): equal inputs give equal bytes.
//
//   k_blur_rows / k_blur_cols   cv2.GaussianBlur(roi, (15, 15), 0) on u8: the 8.8 fixed-point taps below (sigma 2.6, side taps
//                 rounded, the centre takes what is left of 256), the row pass exact in 16 bits, the column pass rounded
//                 once ((s + 2^15) >> 16), REFLECT_101 at the rectangle's own border
//   k_region_sums exact sums a, b, a^2, b^2, a b of two gray rectangles (BGR2GRAY applied to RGB data, as _compute_ssim)
//   k_resize_lin  cv2.resize(INTER_LINEAR) on u8: the sampling of sr_linear.h, as k_feather_merge's resize branch
#include <algorithm>
#include <cmath>
#include <vector>

#include "sr_ctx.h"
#include "sr_fft.h"
#include "sr_linear.h"

namespace {

#define PS_THREADS 256


__device__ __forceinline__ int ps_refl101(int p, int n)
{
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

__global__ __launch_bounds__(PS_THREADS) void k_ps_mask(const unsigned char *__restrict__ mask, long long stride, int h, int w,
                                                        unsigned char *__restrict__ out)
{
    const int x = blockIdx.x * PS_THREADS + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const int y0 = max(y - 3, 0), y1 = min(y + 3, h - 1), x0 = max(x - 3, 0), x1 = min(x + 3, w - 1);
    int m = 1;
    for (int yy = y0; yy <= y1; ++yy) {
        const unsigned char *r = mask + (long long)yy * stride;
        for (int xx = x0; xx <= x1; ++xx) m &= r[xx] != 0;
    }
    out[(long long)y * w + x] = (unsigned char)m;
}

// lam[0 .. wi) for the x axis, lam[wi .. wi + hi) for the y axis
__global__ void k_ps_lambda(double *__restrict__ lam, int wi, int hi)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= wi + hi) return;
    const int k = i < wi ? i : i - wi, n = i < wi ? wi : hi;
    const double s = sinpi((double)(k + 1) / (2.0 * (double)(n + 1)));
    lam[i] = -4.0 * s * s;
}

struct PsImg {
    const unsigned char *p;
    long long stride;
    int gray;   // mode 3: every channel reads the RGB2GRAY value
    __device__ __forceinline__ int at(int x, int y, int c) const
    {
        const unsigned char *q = p + (long long)y * stride + x * 3;
        return gray ? (q[0] * 9798 + q[1] * 19235 + q[2] * 3735 + (1 << 14)) >> 15 : q[c];
    }
};

// the mixed field (fx, fy) of channel c at (x, y); x <= w - 2 and y <= h - 2 wherever this is called
__device__ __forceinline__ void ps_field(const PsImg &D, const PsImg &P, const unsigned char *__restrict__ em, int w, int mode,
                                         int x, int y, int c, int &fx, int &fy)
{
    const int d0 = D.at(x, y, c);
    fx = D.at(x + 1, y, c) - d0;
    fy = D.at(x, y + 1, c) - d0;
    if (!em[(long long)y * w + x]) return;
    const int p0 = P.at(x, y, c);
    const int px = P.at(x + 1, y, c) - p0, py = P.at(x, y + 1, c) - p0;
    if (mode != 2 || abs(px - py) > abs(fx - fy)) {
        fx = px;
        fy = py;
    }
}

// X: 2 hi lines of Lw = 2 (wi + 1) complex values; line p hi + y of plane p
__global__ __launch_bounds__(PS_THREADS) void k_ps_rhs(PsImg D, PsImg P, const unsigned char *__restrict__ em, int h, int w,
                                                       int mode, float2 *__restrict__ X)
{
    const int wi = w - 2, hi = h - 2, Lw = 2 * (wi + 1);
    const int j = blockIdx.x * PS_THREADS + threadIdx.x, yy = blockIdx.y;
    if (j >= wi) return;
    const int x = j + 1, y = yy + 1;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int fx, fy, gx, gy, ex, ey;
        ps_field(D, P, em, w, mode, x, y, c, fx, fy);
        ps_field(D, P, em, w, mode, x - 1, y, c, gx, gy);
        ps_field(D, P, em, w, mode, x, y - 1, c, ex, ey);
        int r = (fx - gx) + (fy - ey);
        // the 4-neighbour Laplacian of the destination with its interior zeroed: only frame neighbours count
        if (x == 1) r -= D.at(0, y, c);
        if (x == w - 2) r -= D.at(w - 1, y, c);
        if (y == 1) r -= D.at(x, 0, c);
        if (y == h - 2) r -= D.at(x, h - 1, c);
        v[c] = (float)r;
    }
    float2 *l0 = X + (long long)yy * Lw, *l1 = X + (long long)(hi + yy) * Lw;
    l0[1 + j] = make_float2(v[0], v[1]);
    l0[Lw - 1 - j] = make_float2(-v[0], -v[1]);
    l1[1 + j] = make_float2(v[2], 0.0f);
    l1[Lw - 1 - j] = make_float2(-v[2], 0.0f);
    if (j == 0) l0[0] = l1[0] = make_float2(0.0f, 0.0f);
    if (j == wi - 1) l0[wi + 1] = l1[wi + 1] = make_float2(0.0f, 0.0f);
}

__device__ __forceinline__ float2 ps_dst(float2 f) { return make_float2(-0.5f * f.y, 0.5f * f.x); }   // (i / 2) f

// in: per plane A lines of Lin values, of which elements 1 .. B are used; out: per plane B lines of Lout = 2 (A + 1) values.
// out[p][b][1 + a] = (i / 2) in[p][a][1 + b], odd-extended.
__global__ __launch_bounds__(256) void k_ps_xpose(const float2 *__restrict__ in, int A, int Lin, int B, float2 *__restrict__ out)
{
    __shared__ float2 s[32][33];
    const int Lout = 2 * (A + 1);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int a0 = blockIdx.y * 32, b0 = blockIdx.x * 32;
    const float2 *src = in + (long long)blockIdx.z * A * Lin;
    float2 *dst = out + (long long)blockIdx.z * B * Lout;
    for (int i = ty; i < 32; i += 8)
        if (a0 + i < A && b0 + tx < B) s[i][tx] = ps_dst(src[(long long)(a0 + i) * Lin + 1 + b0 + tx]);
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int b = b0 + i, a = a0 + tx;
        if (b < B && a < A) {
            const float2 v = s[tx][i];
            float2 *l = dst + (long long)b * Lout;
            l[1 + a] = v;
            l[Lout - 1 - a] = make_float2(-v.x, -v.y);
            if (a == 0) l[0] = make_float2(0.0f, 0.0f);
            if (a == A - 1) l[A + 1] = make_float2(0.0f, 0.0f);
        }
    }
}

// F, out: 2 wi lines of Lh = 2 (hi + 1) values (line p wi + k)
__global__ __launch_bounds__(PS_THREADS) void k_ps_eig(const float2 *__restrict__ F, const double *__restrict__ lam, int wi, int hi,
                                                       double scale, float2 *__restrict__ out)
{
    const int Lh = 2 * (hi + 1);
    const int v = blockIdx.x * PS_THREADS + threadIdx.x, line = blockIdx.y;
    if (v >= hi) return;
    const int k = line >= wi ? line - wi : line;
    const float den = (float)((lam[k] + lam[wi + v]) * scale);
    const float2 t = ps_dst(F[(long long)line * Lh + 1 + v]);
    const float2 q = make_float2(__fdiv_rn(t.x, den), __fdiv_rn(t.y, den));
    float2 *l = out + (long long)line * Lh;
    l[1 + v] = q;
    l[Lh - 1 - v] = make_float2(-q.x, -q.y);
    if (v == 0) l[0] = make_float2(0.0f, 0.0f);
    if (v == hi - 1) l[hi + 1] = make_float2(0.0f, 0.0f);
}

__device__ __forceinline__ unsigned char ps_u8(float v)
{
    // NaN (never produced by finite inputs) lands on 0 rather than on an undefined conversion
    return v >= 0.0f ? (unsigned char)(int)fminf(rintf(v), 255.0f) : 0;
}

// F: 2 hi lines of Lw values, or null: the output is the destination
__global__ __launch_bounds__(PS_THREADS) void k_ps_final(const float2 *__restrict__ F, const unsigned char *__restrict__ dest,
                                                         long long dstride, int h, int w, unsigned char *__restrict__ out,
                                                         long long ostride)
{
    const int x = blockIdx.x * PS_THREADS + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    unsigned char *o = out + (long long)y * ostride + x * 3;
    if (!F || x == 0 || y == 0 || x == w - 1 || y == h - 1) {
        const unsigned char *d = dest + (long long)y * dstride + x * 3;
        o[0] = d[0];
        o[1] = d[1];
        o[2] = d[2];
        return;
    }
    const int hi = h - 2, Lw = 2 * (w - 1);
    const float2 z0 = ps_dst(F[(long long)(y - 1) * Lw + x]), z1 = ps_dst(F[(long long)(hi + y - 1) * Lw + x]);
    o[0] = ps_u8(z0.x);
    o[1] = ps_u8(z0.y);
    o[2] = ps_u8(z1.x);
}

// ---- 15 x 15 Gaussian blur, 8.8 fixed point ----------------------------------------------------------------------------------
__constant__ int c_blur15[15] = {1, 3, 6, 12, 20, 29, 37, 40, 37, 29, 20, 12, 6, 3, 1};

__global__ __launch_bounds__(PS_THREADS) void k_blur_rows(const unsigned char *__restrict__ src, long long stride, int h, int w,
                                                          int cn, unsigned short *__restrict__ tmp)
{
    const int e = blockIdx.x * PS_THREADS + threadIdx.x, y = blockIdx.y;
    if (e >= w * cn) return;
    const int x = e / cn, c = e - x * cn;
    const unsigned char *r = src + (long long)y * stride + c;
    int s = 0;
#pragma unroll
    for (int t = 0; t < 15; ++t) s += c_blur15[t] * r[ps_refl101(x + t - 7, w) * cn];
    tmp[(long long)y * w * cn + e] = (unsigned short)s;          // at most 255 * 256
}

__global__ __launch_bounds__(PS_THREADS) void k_blur_cols(const unsigned short *__restrict__ tmp, int h, int w, int cn,
                                                          unsigned char *__restrict__ dst, long long stride)
{
    const int e = blockIdx.x * PS_THREADS + threadIdx.x, y = blockIdx.y;
    const int rowlen = w * cn;
    if (e >= rowlen) return;
    unsigned s = 0;
#pragma unroll
    for (int t = 0; t < 15; ++t) s += (unsigned)c_blur15[t] * tmp[(long long)ps_refl101(y + t - 7, h) * rowlen + e];
    dst[(long long)y * stride + e] = (unsigned char)((s + (1u << 15)) >> 16);
}

// ---- region SSIM sums --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ps_gray_swapped(const unsigned char *q, int cn, int shift)
{
    // cv2.COLOR_BGR2GRAY applied to RGB data: channel 0 takes the blue weight
    if (cn == 1) return q[0];
    return shift == 15 ? (q[2] * 9798 + q[1] * 19235 + q[0] * 3735 + (1 << 14)) >> 15
                       : (q[2] * 4899 + q[1] * 9617 + q[0] * 1868 + (1 << 13)) >> 14;
}

__global__ __launch_bounds__(256) void k_region_sums(const unsigned char *__restrict__ A, long long sa_, const unsigned char *__restrict__ B,
                                                     long long sb_, int h, int w, int cn, int shift,
                                                     unsigned long long *__restrict__ sums)
{
    unsigned long long sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
    for (int i = blockIdx.y; i < h; i += gridDim.y) {
        const unsigned char *ra = A + (long long)i * sa_, *rb = B + (long long)i * sb_;
        unsigned ta = 0, tb = 0, taa = 0, tbb = 0, tab = 0;       // one thread takes at most 2^15 pixels of a row: no overflow
        for (int j = blockIdx.x * 256 + threadIdx.x; j < w; j += gridDim.x * 256) {
            const int a = ps_gray_swapped(ra + (long long)j * cn, cn, shift), b = ps_gray_swapped(rb + (long long)j * cn, cn, shift);
            ta += a;
            tb += b;
            taa += a * a;
            tbb += b * b;
            tab += a * b;
        }
        sa += ta; sb += tb; saa += taa; sbb += tbb; sab += tab;
    }
    for (int o = 32; o > 0; o >>= 1) {
        sa += __shfl_down(sa, o, 64);
        sb += __shfl_down(sb, o, 64);
        saa += __shfl_down(saa, o, 64);
        sbb += __shfl_down(sbb, o, 64);
        sab += __shfl_down(sab, o, 64);
    }
    __shared__ unsigned long long ws[4][5];
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *q = ws[threadIdx.x >> 6];
        q[0] = sa; q[1] = sb; q[2] = saa; q[3] = sbb; q[4] = sab;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int k = threadIdx.x;
        const unsigned long long t = (ws[0][k] + ws[1][k]) + (ws[2][k] + ws[3][k]);
        if (t) atomicAdd(&sums[k], t);                            // integer: exact whatever the order
    }
}

// ---- INTER_LINEAR resize -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PS_THREADS) void k_resize_lin(const unsigned char *__restrict__ src, long long sstride, int h, int w,
                                                           int cn, const LinTab *__restrict__ xt, const LinTab *__restrict__ yt,
                                                           unsigned char *__restrict__ dst, long long dstride, int dw)
{
    const int e = blockIdx.x * PS_THREADS + threadIdx.x, y = blockIdx.y;
    if (e >= dw * cn) return;
    const int x = e / cn, c = e - x * cn;
    const LinTab X = xt[x], Y = yt[y];
    const int x1 = min(X.ofs + 1, w - 1), y1 = min(Y.ofs + 1, h - 1);
    const unsigned char *r0 = src + (long long)Y.ofs * sstride, *r1 = src + (long long)y1 * sstride;
    dst[(long long)y * dstride + e] = (unsigned char)lin_u8(r0, r1, X.ofs * cn + c, x1 * cn + c, X, Y);
}

dim3 row_grid(long long rowlen, int rows) { return dim3((unsigned)((rowlen + PS_THREADS - 1) / PS_THREADS), (unsigned)rows); }

}  // namespace

extern "C" {

int sr_poisson_max_side(void) { return sr_fft_max_len() / 2 + 1; }

int sr_poisson_clone_u8(sr_ctx *ctx, const uint8_t *d_dest, int64_t dest_stride, const uint8_t *d_patch, int64_t patch_stride,
                        const uint8_t *d_mask, int64_t mask_stride, int h, int w, int mode, uint8_t *d_out, int64_t out_stride)
{
    CTX_ENTER(ctx);
    if (!d_dest || !d_patch || !d_mask || !d_out || h < 1 || w < 1 || mode < 1 || mode > 3)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_poisson_clone_u8: bad arguments (mode 1..3)");
    if (dest_stride < (int64_t)w * 3 || patch_stride < (int64_t)w * 3 || out_stride < (int64_t)w * 3 || mask_stride < w)
        return sr_set_error(SR_ERR_SHAPE, "sr_poisson_clone_u8: a stride is below the row length");
    if (h > sr_poisson_max_side() || w > sr_poisson_max_side())
        return sr_set_error(SR_ERR_UNSUPPORTED, "sr_poisson_clone_u8: side above %d", sr_poisson_max_side());
    if (h < 3 || w < 3) {                                         // no interior
        ProfScope ps(ctx, "ps_final");
        hipLaunchKernelGGL(k_ps_final, row_grid(w, h), dim3(PS_THREADS), 0, ctx->stream, (const float2 *)nullptr, d_dest,
                           (long long)dest_stride, h, w, d_out, (long long)out_stride);
        return check_launch("poisson_clone");
    }
    const int wi = w - 2, hi = h - 2, Lw = 2 * (wi + 1), Lh = 2 * (hi + 1);
    const size_t buf = std::max((size_t)2 * hi * sr_fft_work_len(Lw), (size_t)2 * wi * sr_fft_work_len(Lh));
    const size_t b_fft = up256(buf * 8), b_tab = up256(std::max(sr_fft_tab_elems(Lw), sr_fft_tab_elems(Lh)) * 8),
                 b_lam = up256((size_t)(wi + hi) * 8), b_em = up256((size_t)h * w);
    char *ws = nullptr;
    int rc = sr_fft_workspace(ctx, 3 * b_fft + b_tab + b_lam + b_em, &ws);
    if (rc) return rc;
    float2 *bufs[3] = {(float2 *)ws, (float2 *)(ws + b_fft), (float2 *)(ws + 2 * b_fft)};
    float2 *tab = (float2 *)(ws + 3 * b_fft);
    double *lam = (double *)(ws + 3 * b_fft + b_tab);
    unsigned char *em = (unsigned char *)(ws + 3 * b_fft + b_tab + b_lam);
    auto others = [&](const float2 *cur, float2 *&p, float2 *&q) {
        float2 *o[2];
        int k = 0;
        for (float2 *b : bufs)
            if (b != cur) o[k++] = b;
        p = o[0];
        q = o[1];
    };
    const dim3 tr_rows((wi + 31) / 32, (hi + 31) / 32, 2), tr_cols((hi + 31) / 32, (wi + 31) / 32, 2);
    float2 *p, *q, *r;
    {
        ProfScope ps(ctx, "ps_rhs");
        hipLaunchKernelGGL(k_ps_mask, row_grid(w, h), dim3(PS_THREADS), 0, ctx->stream, d_mask, (long long)mask_stride, h, w, em);
        hipLaunchKernelGGL(k_ps_lambda, dim3((wi + hi + 255) / 256), dim3(256), 0, ctx->stream, lam, wi, hi);
        const PsImg D{d_dest, (long long)dest_stride, 0}, P{d_patch, (long long)patch_stride, mode == 3 ? 1 : 0};
        hipLaunchKernelGGL(k_ps_rhs, row_grid(wi, hi), dim3(PS_THREADS), 0, ctx->stream, D, P, (const unsigned char *)em, h, w, mode,
                           bufs[0]);
    }
    {
        ProfScope ps(ctx, "ps_dst_fwd");
        r = sr_fft_lines(ctx, bufs[0], bufs[1], bufs[2], tab, 2LL * hi, Lw, true);
        others(r, p, q);
        hipLaunchKernelGGL(k_ps_xpose, tr_rows, dim3(256), 0, ctx->stream, (const float2 *)r, hi, Lw, wi, p);
        r = sr_fft_lines(ctx, p, r, q, tab, 2LL * wi, Lh, true);
    }
    others(r, p, q);
    {
        ProfScope ps(ctx, "ps_eig");
        const double scale = 0.25 * (double)(wi + 1) * (double)(hi + 1);
        hipLaunchKernelGGL(k_ps_eig, row_grid(hi, 2 * wi), dim3(PS_THREADS), 0, ctx->stream, (const float2 *)r, (const double *)lam, wi,
                           hi, scale, p);
    }
    {
        ProfScope ps(ctx, "ps_dst_inv");
        float2 *x = p;
        r = sr_fft_lines(ctx, x, r, q, tab, 2LL * wi, Lh, true);
        others(r, p, q);
        hipLaunchKernelGGL(k_ps_xpose, tr_cols, dim3(256), 0, ctx->stream, (const float2 *)r, wi, Lh, hi, p);
        r = sr_fft_lines(ctx, p, r, q, tab, 2LL * hi, Lw, true);
    }
    {
        ProfScope ps(ctx, "ps_final");
        hipLaunchKernelGGL(k_ps_final, row_grid(w, h), dim3(PS_THREADS), 0, ctx->stream, (const float2 *)r, d_dest,
                           (long long)dest_stride, h, w, d_out, (long long)out_stride);
    }
    return check_launch("poisson_clone");
}

int sr_gaussian_blur15_u8(sr_ctx *ctx, const uint8_t *d_src, int64_t src_stride, int h, int w, int cn, uint8_t *d_dst,
                          int64_t dst_stride)
{
    CTX_ENTER(ctx);
    if (!d_src || !d_dst || h < 1 || w < 1 || (cn != 1 && cn != 3 && cn != 4))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_gaussian_blur15_u8: bad arguments (cn 1, 3 or 4)");
    if (src_stride < (int64_t)w * cn || dst_stride < (int64_t)w * cn)
        return sr_set_error(SR_ERR_SHAPE, "sr_gaussian_blur15_u8: a stride is below the row length");
    if (h > 65535 || (long long)w * cn > (1LL << 30)) return sr_set_error(SR_ERR_SHAPE, "sr_gaussian_blur15_u8: image too large");
    char *ws = nullptr;
    int rc = sr_fft_workspace(ctx, (size_t)h * w * cn * 2, &ws);
    if (rc) return rc;
    ProfScope ps(ctx, "blur15");
    hipLaunchKernelGGL(k_blur_rows, row_grid((long long)w * cn, h), dim3(PS_THREADS), 0, ctx->stream, d_src, (long long)src_stride, h,
                       w, cn, (unsigned short *)ws);
    hipLaunchKernelGGL(k_blur_cols, row_grid((long long)w * cn, h), dim3(PS_THREADS), 0, ctx->stream, (const unsigned short *)ws, h, w,
                       cn, d_dst, (long long)dst_stride);
    return check_launch("gaussian_blur15");
}

int sr_region_ssim_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w, int cn,
                      int gray_shift, double *h_ssim)
{
    CTX_ENTER(ctx);
    if (!d_a || !d_b || !h_ssim || h < 1 || w < 1 || (cn != 1 && cn != 3 && cn != 4) || (gray_shift != 14 && gray_shift != 15))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_region_ssim_u8: bad arguments");
    if (stride_a < (int64_t)w * cn || stride_b < (int64_t)w * cn)
        return sr_set_error(SR_ERR_SHAPE, "sr_region_ssim_u8: a stride is below the row length");
    if ((long long)h * w > (1LL << 31)) return sr_set_error(SR_ERR_SHAPE, "sr_region_ssim_u8: region above 2^31 pixels");
    void *scr = nullptr;
    int rc = ctx_scratch(ctx, 5 * sizeof(uint64_t), &scr);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(scr, 0, 5 * sizeof(uint64_t), ctx->stream));
    {
        ProfScope ps(ctx, "region_ssim");
        const dim3 grid((unsigned)std::min((w + 255) / 256, 4), (unsigned)std::min(h, 256));
        hipLaunchKernelGGL(k_region_sums, grid, dim3(256), 0, ctx->stream, d_a, (long long)stride_a, d_b, (long long)stride_b, h, w, cn,
                           gray_shift, (unsigned long long *)scr);
    }
    rc = check_launch("region_ssim");
    if (rc) return rc;
    uint64_t s[5];
    HIPCHK(hipMemcpyAsync(s, scr, sizeof(s), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    // _compute_ssim's float64 formula on exact integer moments: one rounding per moment
    const __int128 N = (__int128)h * w;
    const double n = (double)h * (double)w;
    const double mu1 = (double)s[0] / n, mu2 = (double)s[1] / n;
    const double var1 = (double)((__int128)s[2] * N - (__int128)s[0] * s[0]) / (n * n);
    const double var2 = (double)((__int128)s[3] * N - (__int128)s[1] * s[1]) / (n * n);
    const double cov = (double)((__int128)s[4] * N - (__int128)s[0] * s[1]) / (n * n);
    const double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
    *h_ssim = ((2 * mu1 * mu2 + c1) * (2 * cov + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (var1 + var2 + c2));
    return SR_OK;
}

int sr_resize_linear_u8(sr_ctx *ctx, const uint8_t *d_src, int64_t src_stride, int h, int w, int cn, uint8_t *d_dst,
                        int64_t dst_stride, int dh, int dw)
{
    CTX_ENTER(ctx);
    if (!d_src || !d_dst || h < 1 || w < 1 || dh < 1 || dw < 1 || cn < 1 || cn > 4)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_resize_linear_u8: bad arguments");
    if (src_stride < (int64_t)w * cn || dst_stride < (int64_t)dw * cn)
        return sr_set_error(SR_ERR_SHAPE, "sr_resize_linear_u8: a stride is below the row length");
    if (dh > 65535 || (long long)dw * cn > (1LL << 30)) return sr_set_error(SR_ERR_SHAPE, "sr_resize_linear_u8: output too large");
    std::vector<LinTab> tabs;
    linear_table(w, dw, tabs);
    linear_table(h, dh, tabs);
    void *scr = nullptr;
    int rc = ctx_scratch(ctx, sizeof(LinTab) * tabs.size(), &scr);
    if (rc) return rc;
    HIPCHK(upload_small(ctx, scr, tabs.data(), sizeof(LinTab) * tabs.size()));
    {
        ProfScope ps(ctx, "resize_linear");
        hipLaunchKernelGGL(k_resize_lin, row_grid((long long)dw * cn, dh), dim3(PS_THREADS), 0, ctx->stream, d_src,
                           (long long)src_stride, h, w, cn, (const LinTab *)scr, (const LinTab *)scr + dw, d_dst,
                           (long long)dst_stride, dw);
    }
    return check_launch("resize_linear");
}

}  // extern "C"
