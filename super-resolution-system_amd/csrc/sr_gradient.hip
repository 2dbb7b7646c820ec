// sr_gradient.hip -- BlendingModule.gradient_domain_fusion (blending_module.py:1377-1489, _reconstruct_from_gradients
// :1491-1523) and the module-level compute_blend_quality (:1563-1608) on gfx950.
//
// gradient_domain_fusion, per canvas pixel p and channel c, all in fp32 exactly as the reference's NumPy sequence:
//   gx(p) = sum over the covering tiles in list order of Sobel_x(tile)(p) * w_tile(p)     (w: cosine LUT, reflect-101 Sobel
//   W(p)  = sum of w_tile(p)                                                               at the TILE's borders)
//   Gx = gx / max(W, 1e-6f), Gy likewise; r = cumsum_x(Gx) + cumsum_y(Gy); r / 2 -> clip -> truncate to u8.
// np.cumsum on float32 is a sequential chain, so each (row, channel) and (column, channel) is summed by ONE lane in order.
// Two kernels, the normalised gradients never reach HBM:
//   k_grad_row  a block owns GR_ROWS canvas rows and walks them in chunks of GR_CHUNK row elements: all threads form Gx of
//               the chunk into LDS (parallel, coalesced tile reads), one wave runs the GR_ROWS x cn chains through it, all
//               threads write the prefix sums out as the fp32 plane cx.
//   k_grad_col  a block owns GC_COLS consecutive row elements (x * cn + c) and walks all rows in chunks of GC_ROWS: Gy of the
//               chunk into LDS, one wave (lane = column chain) sums down, all threads finish (cx + cy) / 2 -> u8.
// Byte floor: tiles read once per pass, cx written once and read once, the canvas written once.
//
// compute_blend_quality: k_grad_mag takes the u8 Sobel magnitude sums of the canvas (sum of gx^2 + gy^2 exact in u64, sum of
// sqrt in fp64, per-block partials summed on the host in a fixed order); k_tile_ssim takes per tile the exact integer sums
// of the BGR2GRAY-on-RGB gray ROI and gray tile (resized like cv2.resize INTER_LINEAR when the canvas clips it), from which
// the host finishes _compute_ssim (:855-903) in float64.
#include <algorithm>
#include <cstring>
#include <vector>

#include "sr_ctx.h"
#include "sr_linear.h"

namespace {

enum { GSRC_U8 = 0, GSRC_F32 = 1 };

struct GradTile {
    const void *p;
    long long stride;     // bytes
    int x, y, w, h;       // canvas rectangle of the whole tile (it may reach past the canvas)
    int fw, lut;          // feather width min(h, w) // 8 and offset of its cosine LUT (fw + 1 entries)
};

#define GR_ROWS 16
#define GR_CHUNK 256
#define GC_COLS 64
#define GC_ROWS 64
#define G_MAXLIST 64

__device__ __forceinline__ int refl101(int p, int n)
{
    // n >= 8 for every tile (a smaller side gives the reference a zero feather width); p is at most one step outside
    return p < 0 ? -p : (p >= n ? 2 * n - 2 - p : p);
}

template <int DT>
__device__ __forceinline__ float tile_at(const GradTile &T, int r, int col)
{
    const char *row = (const char *)T.p + (size_t)r * T.stride;
    if (DT == GSRC_U8) return (float)((const unsigned char *)row)[col];
    return ((const float *)row)[col];
}

// Normalised Sobel gradient of canvas pixel (y, x), channel c: AX 0 = d/dx (cv2.Sobel(t, CV_32F, 1, 0, ksize=3)), 1 = d/dy.
// Separable order of OpenCV: the row kernel first, then the column kernel; derivative [-1, 0, 1] = b - a, smoothing
// [1, 2, 1] = (a + c) + 2 b.  Exact for integer-valued tiles; for other float data this order is the restatement's.
template <int DT, int AX>
__device__ __forceinline__ float grad_norm(const GradTile *tl, int m, const float *__restrict__ luts, int y, int x, int c,
                                           int cn)
{
    float acc = 0.0f, wacc = 0.0f;
    for (int i = 0; i < m; ++i) {
        const GradTile &T = tl[i];
        const int ly = y - T.y, lx = x - T.x;
        if ((unsigned)ly >= (unsigned)T.h || (unsigned)lx >= (unsigned)T.w) continue;
        const int ym = refl101(ly - 1, T.h), yp = refl101(ly + 1, T.h);
        const int xm = refl101(lx - 1, T.w) * cn + c, xp = refl101(lx + 1, T.w) * cn + c, x0 = lx * cn + c;
        float g;
        if (AX == 0) {
            const float dm = tile_at<DT>(T, ym, xp) - tile_at<DT>(T, ym, xm);
            const float d0 = tile_at<DT>(T, ly, xp) - tile_at<DT>(T, ly, xm);
            const float dp = tile_at<DT>(T, yp, xp) - tile_at<DT>(T, yp, xm);
            g = (dm + dp) + 2.0f * d0;
        } else {
            const float sm = (tile_at<DT>(T, ym, xm) + tile_at<DT>(T, ym, xp)) + 2.0f * tile_at<DT>(T, ym, x0);
            const float sp = (tile_at<DT>(T, yp, xm) + tile_at<DT>(T, yp, xp)) + 2.0f * tile_at<DT>(T, yp, x0);
            g = sp - sm;
        }
        const int d = min(min(ly, T.h - 1 - ly), min(lx, T.w - 1 - lx));
        const float w = luts[T.lut + min(d, T.fw)];
        acc = acc + g * w;                   // grad += g * w (the product rounded first: -ffp-contract=off)
        wacc = wacc + w;
    }
    return acc / fmaxf(wacc, 1e-6f);         // IEEE division (v_div_scale / v_div_fmas / v_div_fixup)
}

// Wave 0 lists, in list order, the tiles that meet canvas rows [y0, y1) x columns [x0, x1); lanes copy the descriptors into
// LDS.  Returns the count (> G_MAXLIST: the caller walks the whole table instead).
__device__ __forceinline__ int list_tiles(const GradTile *__restrict__ tiles, int n, int y0, int y1, int x0, int x1,
                                          GradTile *s_tiles, int *s_cnt)
{
    __shared__ int s_idx[G_MAXLIST];
    const int tid = threadIdx.x;
    if (tid < 64) {
        int cnt = 0;
        for (int base = 0; base < n; base += 64) {
            const int t = base + tid;
            bool hit = false;
            if (t < n) {
                const GradTile &T = tiles[t];
                hit = T.x < x1 && T.x + T.w > x0 && T.y < y1 && T.y + T.h > y0;
            }
            const unsigned long long mk = __ballot(hit);
            if (hit) {
                const int pos = cnt + __popcll(mk & ((1ull << tid) - 1ull));
                if (pos < G_MAXLIST) s_idx[pos] = t;
            }
            cnt += __popcll(mk);
        }
        if (tid == 0) *s_cnt = cnt;
    }
    __syncthreads();
    const int cnt = *s_cnt;
    if (cnt <= G_MAXLIST && tid < cnt) s_tiles[tid] = tiles[s_idx[tid]];
    __syncthreads();
    return cnt;
}

template <int DT>
__global__ __launch_bounds__(256) void k_grad_row(const GradTile *__restrict__ tiles, int n, const float *__restrict__ luts,
                                                  int H, int W, int cn, float *__restrict__ cx)
{
    __shared__ float buf[GR_ROWS][GR_CHUNK + 1];
    __shared__ GradTile s_tiles[G_MAXLIST];
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    const int y0 = blockIdx.x * GR_ROWS, rows = min(GR_ROWS, H - y0);
    const long long Wc = (long long)W * cn;
    // chain of lane l (wave 0): row l % GR_ROWS, channel l / GR_ROWS; its running sum lives in a register across chunks
    const int cr = tid % GR_ROWS, cc = tid / GR_ROWS;
    const bool chain = tid < 64 && cc < cn && cr < rows;
    float run = 0.0f;
    for (long long e0 = 0; e0 < Wc; e0 += GR_CHUNK) {
        const int ne = (int)min((long long)GR_CHUNK, Wc - e0);
        const int px0 = (int)(e0 / cn), px1 = (int)((e0 + ne - 1) / cn) + 1;
        const int cnt = list_tiles(tiles, n, y0, y0 + rows, px0, px1, s_tiles, &s_cnt);
        const GradTile *tl = cnt <= G_MAXLIST ? s_tiles : tiles;
        const int m = cnt <= G_MAXLIST ? cnt : n;
        if (tid < ne) {
            const long long e = e0 + tid;
            const int x = (int)(e / cn), c = (int)(e - (long long)x * cn);
            for (int r = 0; r < rows; ++r) buf[r][tid] = grad_norm<DT, 0>(tl, m, luts, y0 + r, x, c, cn);
        }
        __syncthreads();
        if (chain) {
            const int j0 = (int)(((cc - e0 % cn) % cn + cn) % cn);
            float *b = buf[cr];
#pragma unroll 8
            for (int j = j0; j < ne; j += cn) {
                run = run + b[j];
                b[j] = run;
            }
        }
        __syncthreads();
        if (tid < ne)
            for (int r = 0; r < rows; ++r) cx[(size_t)(y0 + r) * Wc + e0 + tid] = buf[r][tid];
        // the next chunk's list_tiles begins with a barrier before any thread writes buf again
    }
}

template <int DT>
__global__ __launch_bounds__(256) void k_grad_col(const GradTile *__restrict__ tiles, int n, const float *__restrict__ luts,
                                                  int H, int W, int cn, const float *__restrict__ cx,
                                                  unsigned char *__restrict__ out, long long ostride)
{
    __shared__ float buf[GC_ROWS][GC_COLS + 1];
    __shared__ GradTile s_tiles[G_MAXLIST];
    __shared__ int s_cnt;
    const int tid = threadIdx.x, lane = tid & (GC_COLS - 1), grp = tid / GC_COLS;   // 4 row groups of 64 element lanes
    const long long Wc = (long long)W * cn, e0 = (long long)blockIdx.x * GC_COLS;
    const int ne = (int)min((long long)GC_COLS, Wc - e0);
    const long long e = e0 + lane;
    const int x = (int)(e / cn), c = (int)(e - (long long)x * cn);
    const int px0 = (int)(e0 / cn), px1 = (int)((e0 + ne - 1) / cn) + 1;
    float run = 0.0f;
    for (int y0 = 0; y0 < H; y0 += GC_ROWS) {
        const int rows = min(GC_ROWS, H - y0);
        const int cnt = list_tiles(tiles, n, y0, y0 + rows, px0, px1, s_tiles, &s_cnt);
        const GradTile *tl = cnt <= G_MAXLIST ? s_tiles : tiles;
        const int m = cnt <= G_MAXLIST ? cnt : n;
        if (lane < ne)
            for (int r = grp; r < rows; r += 256 / GC_COLS) buf[r][lane] = grad_norm<DT, 1>(tl, m, luts, y0 + r, x, c, cn);
        __syncthreads();
        if (tid < ne) {                                   // wave 0: one column chain per lane
#pragma unroll 8
            for (int r = 0; r < rows; ++r) {
                run = run + buf[r][tid];
                buf[r][tid] = run;
            }
        }
        __syncthreads();
        if (lane < ne)
            for (int r = grp; r < rows; r += 256 / GC_COLS) {
                const size_t y = (size_t)(y0 + r);
                float v = cx[y * Wc + e] + buf[r][lane];  // result = cumsum_x; result += cumsum_y
                v = v / 2.0f;                             // result /= 2 (exact)
                v = fminf(fmaxf(v, 0.0f), 255.0f);        // np.clip(result, 0, 255).astype(uint8): truncation
                out[y * ostride + e] = (unsigned char)(int)v;
            }
    }
}

// ---- compute_blend_quality -------------------------------------------------------------------------------------------
#define GM_THREADS 256
#define GM_BLOCKS 2048

// Sum over every element of the u8 canvas of s = gx^2 + gy^2 (exact) and of sqrt(s) (fp64; sqrt of an integer below 2^22
// rounded once to double, which is also the correctly rounded fp32 sqrt once narrowed).  Reflect-101 at the canvas border.
template <int CN>
__global__ __launch_bounds__(GM_THREADS) void k_grad_mag(const unsigned char *__restrict__ img, long long stride, int H, int W,
                                                         unsigned long long *__restrict__ part_sq, double *__restrict__ part_mag)
{
    const int Wc = W * CN;
    unsigned long long ssq = 0;
    double smag = 0.0;
    auto refl = [](int p, int n) { return n == 1 ? 0 : (p < 0 ? -p : (p >= n ? 2 * n - 2 - p : p)); };
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const unsigned char *rm = img + (size_t)refl(y - 1, H) * stride, *r0 = img + (size_t)y * stride,
                            *rp = img + (size_t)refl(y + 1, H) * stride;
        unsigned rsq = 0;                    // < 2^22 per element, at most 2^9 elements per thread and row
        double rmag = 0.0;
        for (int e = blockIdx.x * GM_THREADS + threadIdx.x; e < Wc; e += gridDim.x * GM_THREADS) {
            const int x = e / CN, c = e - x * CN;
            const int xm = refl(x - 1, W) * CN + c, xp = refl(x + 1, W) * CN + c;
            const int gx = ((rm[xp] - rm[xm]) + (rp[xp] - rp[xm])) + 2 * (r0[xp] - r0[xm]);
            const int gy = ((rp[xm] + rp[xp]) + 2 * rp[e]) - ((rm[xm] + rm[xp]) + 2 * rm[e]);
            const unsigned sq = (unsigned)(gx * gx + gy * gy);
            rsq += sq;
            rmag += sqrt((double)sq);
        }
        ssq += rsq;
        smag += rmag;
    }
    for (int o = 32; o > 0; o >>= 1) {
        ssq += __shfl_down(ssq, o, 64);
        smag += __shfl_down(smag, o, 64);
    }
    __shared__ unsigned long long ws[GM_THREADS / 64];
    __shared__ double wm[GM_THREADS / 64];
    if ((threadIdx.x & 63) == 0) {
        ws[threadIdx.x >> 6] = ssq;
        wm[threadIdx.x >> 6] = smag;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int b = blockIdx.y * gridDim.x + blockIdx.x;
        part_sq[b] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
        part_mag[b] = (wm[0] + wm[1]) + (wm[2] + wm[3]);
    }
}

struct SsimTile {
    const unsigned char *p;
    long long stride;
    int x, y, w, h;       // canvas position and tile size
    int oh, ow;           // ROI size: the tile clipped by the canvas
    int resize, xtab, ytab;
};

__device__ __forceinline__ int gray_px(int c0, int c1, int c2, int shift)
{
    // cv2.COLOR_BGR2GRAY applied to RGB data: channel 0 takes the blue weight
    return shift == 15 ? (c2 * 9798 + c1 * 19235 + c0 * 3735 + (1 << 14)) >> 15
                       : (c2 * 4899 + c1 * 9617 + c0 * 1868 + (1 << 13)) >> 14;
}

// Per tile: sums of a, b, a^2, b^2, a b over the ROI (a: gray canvas, b: gray tile), one set of atomics per block.
__global__ __launch_bounds__(256) void k_tile_ssim(const SsimTile *__restrict__ tiles, const LinTab *__restrict__ tabs,
                                                   const unsigned char *__restrict__ img, long long stride, int cn, int shift,
                                                   unsigned long long *__restrict__ sums)
{
    const SsimTile T = tiles[blockIdx.z];
    unsigned long long sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
    for (int i = blockIdx.y; i < T.oh; i += gridDim.y) {
        const unsigned char *crow = img + (size_t)(T.y + i) * stride + (size_t)T.x * cn;
        unsigned ta = 0, tb = 0, taa = 0, tbb = 0, tab = 0;       // one row of at most 2^16 pixels: no overflow
        for (int j = blockIdx.x * 256 + threadIdx.x; j < T.ow; j += gridDim.x * 256) {
            const unsigned char *q = crow + (size_t)j * cn;
            const int a = cn == 1 ? q[0] : gray_px(q[0], q[1], q[2], shift);
            int b;
            if (!T.resize) {
                const unsigned char *t = T.p + (size_t)i * T.stride + (size_t)j * cn;
                b = cn == 1 ? t[0] : gray_px(t[0], t[1], t[2], shift);
            } else {
                const LinTab X = tabs[T.xtab + j], Y = tabs[T.ytab + i];
                const int x1 = min(X.ofs + 1, T.w - 1), y1 = min(Y.ofs + 1, T.h - 1);
                const unsigned char *r0 = T.p + (size_t)Y.ofs * T.stride, *r1 = T.p + (size_t)y1 * T.stride;
                int v[3];
                for (int k = 0; k < (cn == 1 ? 1 : 3); ++k) v[k] = lin_u8(r0, r1, X.ofs * cn + k, x1 * cn + k, X, Y);
                b = cn == 1 ? v[0] : gray_px(v[0], v[1], v[2], shift);
            }
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
        unsigned long long *w = ws[threadIdx.x >> 6];
        w[0] = sa; w[1] = sb; w[2] = saa; w[3] = sbb; w[4] = sab;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int k = threadIdx.x;
        const unsigned long long t = (ws[0][k] + ws[1][k]) + (ws[2][k] + ws[3][k]);
        if (t) atomicAdd(&sums[5 * blockIdx.z + k], t);
    }
}

}  // namespace

extern "C" {

int sr_gradient_fusion(sr_ctx *ctx, int dtype, void *const *h_d_tiles, const int64_t *h_strides, const sr_tile_rect *h_rects,
                       int n, int cn, int canvas_h, int canvas_w, uint8_t *d_canvas, int64_t canvas_stride, float *d_work)
{
    CTX_ENTER(ctx);
    if (!h_d_tiles || !h_strides || !h_rects || !d_canvas || !d_work || n < 1 || cn < 1 || cn > 4 || canvas_h < 1 ||
        canvas_w < 1)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_gradient_fusion: bad arguments");
    if (dtype != SR_U8 && dtype != SR_F32)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_gradient_fusion: dtype must be SR_U8 or SR_F32");
    if (canvas_stride < (int64_t)canvas_w * cn) return sr_set_error(SR_ERR_SHAPE, "sr_gradient_fusion: canvas stride too small");
    const int es = dtype == SR_U8 ? 1 : 4;
    std::vector<GradTile> gt(n);
    std::vector<float> luts;
    for (int t = 0; t < n; ++t) {
        const sr_tile_rect &r = h_rects[t];
        if (!h_d_tiles[t] || r.x < 0 || r.y < 0 || r.x >= canvas_w || r.y >= canvas_h)
            return sr_set_error(SR_ERR_INVALID_ARG, "sr_gradient_fusion: tile %d has a bad position (%d, %d)", t, r.x, r.y);
        if (std::min(r.w, r.h) < 8)
            return sr_set_error(SR_ERR_INVALID_ARG,
                                "sr_gradient_fusion: tile %d is %dx%d; min side < 8 gives the reference a zero feather "
                                "width (NaN weights)", t, r.w, r.h);
        if (h_strides[t] < (int64_t)r.w * cn * es)
            return sr_set_error(SR_ERR_SHAPE, "sr_gradient_fusion: tile %d stride too small", t);
        GradTile &G = gt[t];
        G.p = h_d_tiles[t];
        G.stride = h_strides[t];
        G.x = r.x; G.y = r.y; G.w = r.w; G.h = r.h;
        G.fw = std::min(r.w, r.h) / 8;
        G.lut = -1;
        for (int s = 0; s < t; ++s)                      // tiles of one size share a table
            if (gt[s].fw == G.fw) { G.lut = gt[s].lut; break; }
        if (G.lut < 0) {
            G.lut = (int)luts.size();
            luts.resize(luts.size() + G.fw + 1);
            int rc = sr_weight_lut(G.fw, SR_W_COSINE, luts.data() + G.lut);
            if (rc) return rc;
        }
    }
    const size_t b0 = sizeof(GradTile) * (size_t)n, b1 = sizeof(float) * luts.size();
    void *scr = nullptr;
    int rc = ctx_scratch(ctx, up256(b0) + up256(b1), &scr);
    if (rc) return rc;
    char *p0 = (char *)scr, *p1 = p0 + up256(b0);
    HIPCHK(upload_small(ctx, p0, gt.data(), b0));
    HIPCHK(upload_small(ctx, p1, luts.data(), b1));
    const GradTile *d_gt = (const GradTile *)p0;
    const float *d_luts = (const float *)p1;
    {
        ProfScope ps(ctx, "gradient_row");
        dim3 grid((unsigned)((canvas_h + GR_ROWS - 1) / GR_ROWS));
        if (dtype == SR_U8)
            hipLaunchKernelGGL(k_grad_row<GSRC_U8>, grid, dim3(256), 0, ctx->stream, d_gt, n, d_luts, canvas_h, canvas_w, cn, d_work);
        else
            hipLaunchKernelGGL(k_grad_row<GSRC_F32>, grid, dim3(256), 0, ctx->stream, d_gt, n, d_luts, canvas_h, canvas_w, cn, d_work);
    }
    rc = check_launch("gradient_row");
    if (rc) return rc;
    {
        ProfScope ps(ctx, "gradient_col");
        const long long Wc = (long long)canvas_w * cn;
        dim3 grid((unsigned)((Wc + GC_COLS - 1) / GC_COLS));
        if (dtype == SR_U8)
            hipLaunchKernelGGL(k_grad_col<GSRC_U8>, grid, dim3(256), 0, ctx->stream, d_gt, n, d_luts, canvas_h, canvas_w, cn,
                               (const float *)d_work, d_canvas, (long long)canvas_stride);
        else
            hipLaunchKernelGGL(k_grad_col<GSRC_F32>, grid, dim3(256), 0, ctx->stream, d_gt, n, d_luts, canvas_h, canvas_w, cn,
                               (const float *)d_work, d_canvas, (long long)canvas_stride);
    }
    return check_launch("gradient_col");
}

int sr_gradient_stats_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, uint64_t *h_sum_sq,
                         double *h_sum_mag)
{
    CTX_ENTER(ctx);
    if (!d_img || !h_sum_sq || !h_sum_mag || h < 1 || w < 1 || cn < 1 || cn > 4)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_gradient_stats_u8: bad arguments");
    if (stride < (int64_t)w * cn) return sr_set_error(SR_ERR_SHAPE, "sr_gradient_stats_u8: stride smaller than a row");
    if ((long long)w * cn > (1 << 30)) return sr_set_error(SR_ERR_SHAPE, "sr_gradient_stats_u8: row too long");
    // at most 2^9 elements per thread and row: GM_THREADS * 2^9 >= 2^17 elements per block column
    const int bx = std::min(std::max((w * cn + (GM_THREADS << 9) - 1) / (GM_THREADS << 9), std::min((w * cn + GM_THREADS - 1) / GM_THREADS, 8)), 64);
    const int by = std::min(h, GM_BLOCKS / 8);
    const int blocks = bx * by;
    void *scr = nullptr;
    int rc = ctx_scratch(ctx, (size_t)blocks * 16, &scr);
    if (rc) return rc;
    unsigned long long *d_sq = (unsigned long long *)scr;
    double *d_mag = (double *)((char *)scr + (size_t)blocks * 8);
    {
        ProfScope ps(ctx, "gradient_stats");
        const dim3 grid(bx, by);
        auto k = cn == 1 ? k_grad_mag<1> : cn == 2 ? k_grad_mag<2> : cn == 3 ? k_grad_mag<3> : k_grad_mag<4>;
        hipLaunchKernelGGL(k, grid, dim3(GM_THREADS), 0, ctx->stream, d_img, (long long)stride, h, w, d_sq, d_mag);
    }
    rc = check_launch("gradient_stats");
    if (rc) return rc;
    std::vector<unsigned long long> sq(blocks);
    std::vector<double> mag(blocks);
    HIPCHK(hipMemcpyAsync(sq.data(), d_sq, (size_t)blocks * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(mag.data(), d_mag, (size_t)blocks * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    unsigned long long s = 0;
    double m = 0.0;
    for (int b = 0; b < blocks; ++b) {
        s += sq[b];
        m += mag[b];
    }
    *h_sum_sq = s;
    *h_sum_mag = m;
    return SR_OK;
}

int sr_tile_ssim_sums_u8(sr_ctx *ctx, const uint8_t *d_canvas, int64_t canvas_stride, int canvas_h, int canvas_w, int cn,
                         const sr_tile_rect *h_rects, void *const *h_d_tiles, const int64_t *h_strides, int n, int gray_shift,
                         uint64_t *h_sums)
{
    CTX_ENTER(ctx);
    if (!d_canvas || !h_rects || !h_d_tiles || !h_strides || !h_sums || n < 0 || canvas_h < 1 || canvas_w < 1 ||
        (cn != 1 && cn != 3 && cn != 4) || (gray_shift != 14 && gray_shift != 15))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_tile_ssim_sums_u8: bad arguments");
    if (canvas_stride < (int64_t)canvas_w * cn) return sr_set_error(SR_ERR_SHAPE, "sr_tile_ssim_sums_u8: canvas stride too small");
    if (n == 0) return SR_OK;
    std::vector<SsimTile> st(n);
    std::vector<LinTab> tabs;
    int max_oh = 1, max_ow = 1;
    for (int t = 0; t < n; ++t) {
        const sr_tile_rect &r = h_rects[t];
        if (!h_d_tiles[t] || r.w < 1 || r.h < 1 || r.x < 0 || r.y < 0 || r.x >= canvas_w || r.y >= canvas_h)
            return sr_set_error(SR_ERR_INVALID_ARG, "sr_tile_ssim_sums_u8: tile %d has a bad rectangle", t);
        if (h_strides[t] < (int64_t)r.w * cn) return sr_set_error(SR_ERR_SHAPE, "sr_tile_ssim_sums_u8: tile %d stride too small", t);
        SsimTile &S = st[t];
        S.p = (const unsigned char *)h_d_tiles[t];
        S.stride = h_strides[t];
        S.x = r.x; S.y = r.y; S.w = r.w; S.h = r.h;
        S.oh = std::min(r.h, canvas_h - r.y);
        S.ow = std::min(r.w, canvas_w - r.x);
        S.resize = (S.oh != r.h || S.ow != r.w) ? 1 : 0;
        S.xtab = S.ytab = 0;
        if (S.resize) {                      // cv2.resize(tile, (roi_w, roi_h)): the whole tile down to the ROI's size
            S.xtab = (int)tabs.size();
            linear_table(r.w, S.ow, tabs);
            S.ytab = (int)tabs.size();
            linear_table(r.h, S.oh, tabs);
        }
        max_oh = std::max(max_oh, S.oh);
        max_ow = std::max(max_ow, S.ow);
    }
    const size_t b0 = sizeof(SsimTile) * (size_t)n, b1 = sizeof(LinTab) * tabs.size(), b2 = sizeof(uint64_t) * 5 * (size_t)n;
    void *scr = nullptr;
    int rc = ctx_scratch(ctx, up256(b0) + up256(b1) + up256(b2), &scr);
    if (rc) return rc;
    char *p0 = (char *)scr, *p1 = p0 + up256(b0), *p2 = p1 + up256(b1);
    HIPCHK(upload_small(ctx, p0, st.data(), b0));
    if (b1) HIPCHK(upload_small(ctx, p1, tabs.data(), b1));
    HIPCHK(hipMemsetAsync(p2, 0, b2, ctx->stream));
    {
        ProfScope ps(ctx, "tile_ssim");
        dim3 grid((unsigned)std::min((max_ow + 255) / 256, 4), (unsigned)std::min(max_oh, 256), (unsigned)n);
        hipLaunchKernelGGL(k_tile_ssim, grid, dim3(256), 0, ctx->stream, (const SsimTile *)p0, (const LinTab *)p1, d_canvas,
                           (long long)canvas_stride, cn, gray_shift, (unsigned long long *)p2);
    }
    rc = check_launch("tile_ssim");
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h_sums, p2, b2, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // extern "C"
