// sr_content.hip -- ContentAnalyzer (tiling_module.py:174-370 of the reference) on gfx950: the spectral-residual saliency
// map (:261-289), the local entropy map (:291-321), the forbidden-zone map (:323-370) and the per-tile counts behind
// metadata.roi_flags (:752-757).  Haar faces are a host callable of the Python mirror; MSER text regions come from
// sr_mser.hip (or from a host callable); the boxes of both arrive here as rectangles.
//
//   k_ct_pack        gray plane (cv2.COLOR_BGR2GRAY applied to the RGB data: channel 0 takes the blue weight) as complex
//                    lines
//   sr_fft_lines     rows, k_ct_transpose, columns: the full complex 2-D DFT, left transposed (F^T: W lines of H)
//   k_ct_specmag     M = |F| + 1e-8 (L = log M is never stored)
//   k_ct_residual    the 5x5 mean of L on the fftshift-ed array (index arithmetic; reflect-101 at that array's own border),
//                    R = L - mean as minus the mean of the 25 differences log(M_i / M), conj(exp(R) F / |F|) in place of
//                    F (unit phase where |F| = 0)
//   sr_fft_lines     columns, k_ct_transpose, rows: forward DFT of the conjugate = conjugate of the unscaled inverse
//   k_ct_mag         |.| / (H W)
//   k_ct_blur        5x5 Gaussian [1 4 6 4 1] / 16 (row pass, column pass), reflect-101, with per-block min / max
//   k_ct_minmax      the partials in block order -> min, max (no float atomics: equal inputs give equal bytes)
//   k_ct_norm        astype(u8)((s - min) / (max - min + 1e-8) * 255)
//   k_ct_entropy     one block per window x window cell: 256-bin histogram in LDS (one copy per wave, u32 atomics: exact
//                    counts), H = -sum p log2(p + 1e-10) in fp32 in a fixed tree order, written to the cell
//   k_ct_threshold / k_ct_fill   map = saliency > threshold, OR filled rectangles
//   k_ct_count       non-zero map bytes per rectangle (u64 integer atomics: exact, order-free)
// fp32 throughout, like the high-frequency ratio of sr_commercial.hip whose FFT line engine this file shares (sr_fft.h).
#include <algorithm>
#include <cmath>
#include <vector>

#include "sr_ctx.h"
#include "sr_fft.h"

namespace {

#define CT_THREADS 256
#define CT_NBLK 1024          // blocks of the blur pass = min / max partials
#define CT_ROWBLK 32          // blocks per rectangle of the fill / count kernels
#define CT_MAX_WINDOW 32768   // entropy window: counts stay below 2^31

struct CtRect {
    int x, y, w, h;
};

__device__ __forceinline__ int refl101(int p, int n)
{
    // cv2.borderInterpolate(BORDER_REFLECT_101), repeated reflection for kernels wider than the image
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

// cv2.COLOR_BGR2GRAY on RGB data (tiling_module.py:261: the image is RGB, the code says BGR): R and B weights swapped
__device__ __forceinline__ int gray_swapped(const unsigned char *px, int cn)
{
    return cn == 1 ? px[0] : (px[0] * 3735 + px[1] * 19235 + px[2] * 9798 + (1 << 14)) >> 15;
}

__device__ __forceinline__ float cabs32(float2 f)
{
    return sqrtf(__fadd_rn(__fmul_rn(f.x, f.x), __fmul_rn(f.y, f.y)));
}

__global__ void k_ct_pack(const unsigned char *__restrict__ img, long long stride, int cn, int H, int W,
                          float2 *__restrict__ out)
{
    const long long total = (long long)H * W;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int y = (int)(e / W), x = (int)(e - (long long)y * W);
        out[e] = make_float2((float)gray_swapped(img + (long long)y * stride + (long long)x * cn, cn), 0.0f);
    }
}

// in (rows x cols) -> out (cols x rows), 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void k_ct_transpose(const float2 *__restrict__ in, int rows, int cols, float2 *__restrict__ out)
{
    __shared__ float2 s[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < rows && c0 + tx < cols) s[i][tx] = in[(long long)(r0 + i) * cols + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < cols && r0 + tx < rows) out[(long long)(c0 + i) * rows + r0 + tx] = s[tx][i];
}

__global__ void k_ct_specmag(const float2 *__restrict__ F, long long total, float *__restrict__ M)
{
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
        M[e] = __fadd_rn(cabs32(F[e]), 1e-8f);
}

// F, M: transposed spectrum, element (k, u) at k H + u.  fftshift puts frequency index i at (i + n / 2) mod n.
__global__ __launch_bounds__(CT_THREADS) void k_ct_residual(float2 *__restrict__ F, const float *__restrict__ M, int H, int W)
{
    const long long total = (long long)H * W;
    const int hh = H / 2, hw = W / 2;
    for (long long e = (long long)blockIdx.x * CT_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * CT_THREADS) {
        const int k = (int)(e / H), u = (int)(e - (long long)k * H);
        const int su = u + hh >= H ? u + hh - H : u + hh, sk = k + hw >= W ? k + hw - W : k + hw;
        long long col[5];
        int row[5];
#pragma unroll
        for (int d = 0; d < 5; ++d) {
            int yy = refl101(su + d - 2, H) - hh;
            int xx = refl101(sk + d - 2, W) - hw;
            row[d] = yy < 0 ? yy + H : yy;
            col[d] = (long long)(xx < 0 ? xx + W : xx) * H;
        }
        // R = L - mean = -(1 / 25) sum (L_i - L) with L_i - L = log(M_i / M): a stored fp32 logarithm of 8..25 carries
        // an absolute error of 1e-6, which exp() turns into a relative one; the logarithm of a ratio near 1 does not
        const float mc = M[e];
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) sum = __fadd_rn(sum, logf(__fdiv_rn(M[col[j] + row[i]], mc)));
        const float r = -__fdiv_rn(sum, 25.0f);
        const float a = expf(r);
        const float2 f = F[e];
        const float m = cabs32(f);
        float ux = 1.0f, uy = 0.0f;                     // np.angle(0) = 0
        if (m > 0.0f) {
            ux = __fdiv_rn(f.x, m);
            uy = __fdiv_rn(f.y, m);
        }
        F[e] = make_float2(__fmul_rn(a, ux), -__fmul_rn(a, uy));
    }
}

__global__ void k_ct_mag(const float2 *__restrict__ G, long long total, float inv, float *__restrict__ S)
{
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
        S[e] = __fmul_rn(cabs32(G[e]), inv);
}

__device__ __forceinline__ float tap5(float a, float b, float c, float d, float e)
{
    // [1 4 6 4 1] / 16 the way a symmetric 5-tap filter is evaluated: centre, then the pairs
    return __fadd_rn(__fadd_rn(__fmul_rn(0.375f, c), __fmul_rn(0.25f, __fadd_rn(b, d))), __fmul_rn(0.0625f, __fadd_rn(a, e)));
}

__global__ __launch_bounds__(CT_THREADS) void k_ct_blur(const float *__restrict__ S, int H, int W, float *__restrict__ B,
                                                        float *__restrict__ part)
{
    __shared__ float red[2][CT_THREADS / 64];
    const long long total = (long long)H * W;
    float mn = INFINITY, mx = -INFINITY;
    for (long long e = (long long)blockIdx.x * CT_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * CT_THREADS) {
        const int y = (int)(e / W), x = (int)(e - (long long)y * W);
        int xs[5];
#pragma unroll
        for (int d = 0; d < 5; ++d) xs[d] = refl101(x + d - 2, W);
        float rowv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const float *r = S + (long long)refl101(y + i - 2, H) * W;
            rowv[i] = tap5(r[xs[0]], r[xs[1]], r[xs[2]], r[xs[3]], r[xs[4]]);
        }
        const float v = tap5(rowv[0], rowv[1], rowv[2], rowv[3], rowv[4]);
        B[e] = v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_down(mn, o, 64));
        mx = fmaxf(mx, __shfl_down(mx, o, 64));
    }
    if (lane == 0) {
        red[0][wv] = mn;
        red[1][wv] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CT_THREADS / 64; ++w) {
            mn = fminf(mn, red[0][w]);
            mx = fmaxf(mx, red[1][w]);
        }
        part[2 * blockIdx.x] = mn;
        part[2 * blockIdx.x + 1] = mx;
    }
}

// one wave: the CT_NBLK partials in block order -> mm[0] = min, mm[1] = max
__global__ __launch_bounds__(64) void k_ct_minmax(const float *__restrict__ part, int n, float *__restrict__ mm)
{
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < n; i += 64) {
        mn = fminf(mn, part[2 * i]);
        mx = fmaxf(mx, part[2 * i + 1]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_down(mn, o, 64));
        mx = fmaxf(mx, __shfl_down(mx, o, 64));
    }
    if (threadIdx.x == 0) {
        mm[0] = mn;
        mm[1] = mx;
    }
}

__global__ void k_ct_norm(const float *__restrict__ B, long long total, const float *__restrict__ mm,
                          unsigned char *__restrict__ out)
{
    const float mn = mm[0], den = __fadd_rn(__fsub_rn(mm[1], mn), 1e-8f);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const float v = __fmul_rn(__fdiv_rn(__fsub_rn(B[e], mn), den), 255.0f);
        // 0 <= v <= 255 for finite data; a degenerate plane (NaN) lands on 0 rather than on an undefined conversion
        out[e] = v >= 0.0f ? (unsigned char)(int)fminf(v, 255.0f) : 0;
    }
}

// ---- local entropy ------------------------------------------------------------------------------------------------------
// A block takes one cell at a time.  Each wave counts into its own copy of the histogram: a smooth cell puts most of
// its pixels into a few bins, and the same-address LDS atomics of one wave instruction are serialised -- four copies cut
// the cross-wave part of that queue; the copies are added when the 256 probabilities are formed.
__global__ __launch_bounds__(CT_THREADS) void k_ct_entropy(const unsigned char *__restrict__ img, long long stride, int cn,
                                                           int H, int W, int win, int ncx, long long ncells,
                                                           float *__restrict__ out)
{
    __shared__ unsigned hist[CT_THREADS / 64][256];
    __shared__ float red[CT_THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (long long cell = blockIdx.x; cell < ncells; cell += gridDim.x) {
        const int cy = (int)(cell / ncx), cx = (int)(cell - (long long)cy * ncx);
        const int y0 = cy * win, x0 = cx * win;
        const int ch = min(win, H - y0), cw = min(win, W - x0);
        const int n = ch * cw;
        for (int i = threadIdx.x; i < (CT_THREADS / 64) * 256; i += CT_THREADS) (&hist[0][0])[i] = 0u;
        __syncthreads();
        for (int p = threadIdx.x; p < n; p += CT_THREADS) {
            const int y = p / cw, x = p - y * cw;
            const int g = gray_swapped(img + (long long)(y0 + y) * stride + (long long)(x0 + x) * cn, cn);
            atomicAdd(&hist[wv][g], 1u);
        }
        __syncthreads();
        unsigned c = 0;
#pragma unroll
        for (int w = 0; w < CT_THREADS / 64; ++w) c += hist[w][threadIdx.x];
        // calcHist's float32 counts over their float32 sum; p log2(p + 1e-10) in float32
        const float pr = __fdiv_rn((float)c, (float)n);
        float t = __fmul_rn(pr, log2f(__fadd_rn(pr, 1e-10f)));
        for (int o = 32; o > 0; o >>= 1) t = __fadd_rn(t, __shfl_down(t, o, 64));
        if (lane == 0) red[wv] = t;
        __syncthreads();
        float ent = red[0];
#pragma unroll
        for (int w = 1; w < CT_THREADS / 64; ++w) ent = __fadd_rn(ent, red[w]);
        ent = -ent;
        for (int p = threadIdx.x; p < n; p += CT_THREADS) {
            const int y = p / cw, x = p - y * cw;
            out[(long long)(y0 + y) * W + x0 + x] = ent;
        }
        __syncthreads();                                   // hist and red are reused by the next cell
    }
}

// ---- forbidden map and its counts -------------------------------------------------------------------------------------------
__global__ void k_ct_threshold(const unsigned char *__restrict__ sal, long long total, int thr, unsigned char *__restrict__ map)
{
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
        map[e] = (int)sal[e] > thr ? 1 : 0;
}

// rectangles are inside the map (the host clips them)
__global__ __launch_bounds__(CT_THREADS) void k_ct_fill(const CtRect *__restrict__ rects, int W, unsigned char *__restrict__ map)
{
    const CtRect R = rects[blockIdx.y];
    for (int y = blockIdx.x; y < R.h; y += gridDim.x) {
        unsigned char *row = map + (long long)(R.y + y) * W + R.x;
        for (int x = threadIdx.x; x < R.w; x += CT_THREADS) row[x] = 1;
    }
}

__global__ __launch_bounds__(CT_THREADS) void k_ct_count(const unsigned char *__restrict__ map, long long stride,
                                                         const CtRect *__restrict__ rects,
                                                         unsigned long long *__restrict__ counts)
{
    __shared__ unsigned long long red[CT_THREADS / 64];
    const CtRect R = rects[blockIdx.y];
    unsigned long long s = 0;
    for (int y = blockIdx.x; y < R.h; y += gridDim.x) {
        const unsigned char *row = map + (long long)(R.y + y) * stride + R.x;
        for (int x = threadIdx.x; x < R.w; x += CT_THREADS) s += row[x] != 0;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) red[wv] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CT_THREADS / 64; ++w) s += red[w];
        if (s) atomicAdd(counts + blockIdx.y, s);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
unsigned grid1(long long n, int per = 256, long long cap = 1 << 16)
{
    return (unsigned)std::max(1LL, std::min((n + per - 1) / per, cap));
}

bool bad_image(const void *d_img, int64_t stride, int h, int w, int cn)
{
    return !d_img || h < 1 || w < 1 || (cn != 1 && cn != 3 && cn != 4) || stride < (int64_t)w * cn;
}

// rectangles clipped to the h x w plane, empty ones dropped (keep_all: empty ones kept as 0 x 0 so indices line up)
std::vector<CtRect> clip_rects(const sr_tile_rect *r, int n, int h, int w, bool keep_all)
{
    std::vector<CtRect> out;
    for (int i = 0; i < n; ++i) {
        const long long x1 = std::max(0LL, (long long)r[i].x), y1 = std::max(0LL, (long long)r[i].y);
        const long long x2 = std::min((long long)w, (long long)r[i].x + r[i].w), y2 = std::min((long long)h, (long long)r[i].y + r[i].h);
        if (x2 > x1 && y2 > y1) out.push_back({(int)x1, (int)y1, (int)(x2 - x1), (int)(y2 - y1)});
        else if (keep_all) out.push_back({0, 0, 0, 0});
    }
    return out;
}

}  // namespace

int sr_saliency_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, uint8_t *d_sal)
{
    CTX_ENTER(ctx);
    if (bad_image(d_img, stride, h, w, cn) || !d_sal) return sr_set_error(SR_ERR_INVALID_ARG, "sr_saliency_u8: bad arguments");
    if (h > sr_fft_max_len() || w > sr_fft_max_len())
        return sr_set_error(SR_ERR_UNSUPPORTED, "sr_saliency_u8: DFT side above %d", sr_fft_max_len());
    const long long npx = (long long)h * w;
    const size_t buf = std::max((size_t)h * sr_fft_work_len(w), (size_t)w * sr_fft_work_len(h));
    const size_t b_fft = up256(buf * 8), b_tab = up256(std::max(sr_fft_tab_elems(w), sr_fft_tab_elems(h)) * 8),
                 b_part = up256((size_t)CT_NBLK * 2 * 4 + 2 * 4);
    char *ws = nullptr;
    int rc = sr_fft_workspace(ctx, 3 * b_fft + b_tab + b_part, &ws);
    if (rc) return rc;
    float2 *bufs[3] = {(float2 *)ws, (float2 *)(ws + b_fft), (float2 *)(ws + 2 * b_fft)};
    float2 *tab = (float2 *)(ws + 3 * b_fft);
    float *part = (float *)(ws + 3 * b_fft + b_tab), *mm = part + 2 * CT_NBLK;
    // the two buffers that are not `cur`
    auto others = [&](const float2 *cur, float2 *&p, float2 *&q) {
        float2 *o[2];
        int k = 0;
        for (float2 *b : bufs)
            if (b != cur) o[k++] = b;
        p = o[0];
        q = o[1];
    };
    const dim3 tr_hw((w + 31) / 32, (h + 31) / 32), tr_wh((h + 31) / 32, (w + 31) / 32);
    float2 *p, *q;
    float2 *spec;
    {
        ProfScope ps(ctx, "ct_fft_fwd");
        hipLaunchKernelGGL(k_ct_pack, dim3(grid1(npx)), dim3(256), 0, ctx->stream, d_img, (long long)stride, cn, h, w, bufs[0]);
        float2 *r = sr_fft_lines(ctx, bufs[0], bufs[1], bufs[2], tab, h, w, true);
        others(r, p, q);
        hipLaunchKernelGGL(k_ct_transpose, tr_hw, dim3(256), 0, ctx->stream, (const float2 *)r, h, w, p);
        spec = sr_fft_lines(ctx, p, r, q, tab, w, h, true);
    }
    others(spec, p, q);
    {
        ProfScope ps(ctx, "ct_residual");
        hipLaunchKernelGGL(k_ct_specmag, dim3(grid1(npx)), dim3(256), 0, ctx->stream, (const float2 *)spec, npx, (float *)p);
        hipLaunchKernelGGL(k_ct_residual, dim3(grid1(npx, CT_THREADS)), dim3(CT_THREADS), 0, ctx->stream, spec,
                           (const float *)p, h, w);
    }
    float2 *img2;
    {
        ProfScope ps(ctx, "ct_fft_inv");
        float2 *r = sr_fft_lines(ctx, spec, p, q, tab, w, h, true);
        others(r, p, q);
        hipLaunchKernelGGL(k_ct_transpose, tr_wh, dim3(256), 0, ctx->stream, (const float2 *)r, w, h, p);
        img2 = sr_fft_lines(ctx, p, r, q, tab, h, w, true);
    }
    others(img2, p, q);
    {
        ProfScope ps(ctx, "ct_blur_norm");
        const float inv = (float)(1.0 / ((double)h * (double)w));
        hipLaunchKernelGGL(k_ct_mag, dim3(grid1(npx)), dim3(256), 0, ctx->stream, (const float2 *)img2, npx, inv, (float *)p);
        hipLaunchKernelGGL(k_ct_blur, dim3(CT_NBLK), dim3(CT_THREADS), 0, ctx->stream, (const float *)p, h, w, (float *)q, part);
        hipLaunchKernelGGL(k_ct_minmax, dim3(1), dim3(64), 0, ctx->stream, (const float *)part, CT_NBLK, mm);
        hipLaunchKernelGGL(k_ct_norm, dim3(grid1(npx)), dim3(256), 0, ctx->stream, (const float *)q, npx, (const float *)mm, d_sal);
    }
    return check_launch("saliency");
}

int sr_local_entropy_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, int window, float *d_out)
{
    CTX_ENTER(ctx);
    if (bad_image(d_img, stride, h, w, cn) || !d_out || window < 1 || window > CT_MAX_WINDOW)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_local_entropy_u8: bad arguments (window 1..%d)", CT_MAX_WINDOW);
    if ((long long)h * w > (1LL << 31)) return sr_set_error(SR_ERR_SHAPE, "sr_local_entropy_u8: image above 2^31 pixels");
    const int ncx = (w + window - 1) / window, ncy = (h + window - 1) / window;
    const long long ncells = (long long)ncx * ncy;
    {
        ProfScope ps(ctx, "ct_entropy");
        hipLaunchKernelGGL(k_ct_entropy, dim3(grid1(ncells, 1)), dim3(CT_THREADS), 0, ctx->stream, d_img, (long long)stride, cn, h,
                           w, window, ncx, ncells, d_out);
    }
    return check_launch("local_entropy");
}

int sr_forbidden_map(sr_ctx *ctx, const uint8_t *d_sal, int h, int w, int threshold, const sr_tile_rect *h_rects, int n,
                     uint8_t *d_map)
{
    CTX_ENTER(ctx);
    if (!d_map || h < 1 || w < 1 || n < 0 || (n > 0 && !h_rects))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_forbidden_map: bad arguments");
    for (int i = 0; i < n; ++i)
        if (h_rects[i].w < 0 || h_rects[i].h < 0) return sr_set_error(SR_ERR_INVALID_ARG, "sr_forbidden_map: rectangle %d has a negative size", i);
    const long long npx = (long long)h * w;
    const std::vector<CtRect> rects = clip_rects(h_rects, n, h, w, false);
    ProfScope ps(ctx, "ct_map");
    if (d_sal)
        hipLaunchKernelGGL(k_ct_threshold, dim3(grid1(npx)), dim3(256), 0, ctx->stream, d_sal, npx, threshold, d_map);
    else
        HIPCHK(hipMemsetAsync(d_map, 0, (size_t)npx, ctx->stream));
    if (!rects.empty()) {
        void *d_tab = nullptr;
        int rc = ctx_scratch(ctx, rects.size() * sizeof(CtRect), &d_tab);
        if (rc) return rc;
        HIPCHK(upload_small(ctx, d_tab, rects.data(), rects.size() * sizeof(CtRect)));
        for (size_t i0 = 0; i0 < rects.size(); i0 += 32768) {
            const unsigned m = (unsigned)std::min<size_t>(32768, rects.size() - i0);
            hipLaunchKernelGGL(k_ct_fill, dim3(CT_ROWBLK, m), dim3(CT_THREADS), 0, ctx->stream, (const CtRect *)d_tab + i0, w, d_map);
        }
    }
    return check_launch("forbidden_map");
}

int sr_rect_counts_u8(sr_ctx *ctx, const uint8_t *d_map, int64_t stride, int h, int w, const sr_tile_rect *h_rects, int n,
                      uint64_t *h_counts)
{
    CTX_ENTER(ctx);
    if (!d_map || h < 1 || w < 1 || stride < w || n < 0 || (n > 0 && (!h_rects || !h_counts)))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_rect_counts_u8: bad arguments");
    for (int i = 0; i < n; ++i)
        if (h_rects[i].w < 0 || h_rects[i].h < 0) return sr_set_error(SR_ERR_INVALID_ARG, "sr_rect_counts_u8: rectangle %d has a negative size", i);
    if (n == 0) return SR_OK;
    const std::vector<CtRect> rects = clip_rects(h_rects, n, h, w, true);
    const size_t b_cnt = up256((size_t)n * 8), b_tab = (size_t)n * sizeof(CtRect);
    void *d_s = nullptr;
    int rc = ctx_scratch(ctx, b_cnt + b_tab, &d_s);
    if (rc) return rc;
    unsigned long long *d_cnt = (unsigned long long *)d_s;
    CtRect *d_tab = (CtRect *)((char *)d_s + b_cnt);
    HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)n * 8, ctx->stream));
    HIPCHK(upload_small(ctx, d_tab, rects.data(), b_tab));
    {
        ProfScope ps(ctx, "ct_count");
        for (int i0 = 0; i0 < n; i0 += 32768) {
            const unsigned m = (unsigned)std::min(32768, n - i0);
            hipLaunchKernelGGL(k_ct_count, dim3(CT_ROWBLK, m), dim3(CT_THREADS), 0, ctx->stream, d_map, (long long)stride,
                               (const CtRect *)d_tab + i0, d_cnt + i0);
        }
    }
    rc = check_launch("rect_counts");
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h_counts, d_cnt, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}
