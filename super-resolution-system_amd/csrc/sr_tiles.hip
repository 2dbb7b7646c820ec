// sr_tiles.hip -- the stand-alone tile kernels on gfx950 and their part of the C ABI in include/sr_hip.h.  Holds
//   * k_pyr_down_hwc, k_pyr_up_hwc              sr_pyr_down, sr_pyr_up, sr_pyr_up_sub, sr_pyr_up_add
//   * k_tile_extract                            sr_tile_extract, sr_tile_extract_pad
//   * k_seam_scan, k_seam_scan_cells            sr_seam_scan
//   * k_feather_merge                           sr_feather_merge, sr_feather_merge_dt
// They use the context (sr_ctx.h), the device helpers of sr_device.h and the INTER_LINEAR tables of sr_linear.h; nothing of
// the blend plan, its arena or its descriptors (sr_engine.hip).
//
// Numerics contract: as in sr_engine.hip, every fp32 expression is evaluated in the order written in oracle/sr_oracle.c
// (build with -ffp-contract=off); the seam scan finishes a window's score in fp64, as the reference does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "sr_ctx.h"
#include "sr_device.h"
#include "sr_linear.h"

// ---------------------------------------------------------------------------------------------
// dense HWC pyramid primitives (API utilities for build_gaussian_pyramid & friends)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pyr_down_hwc(const float *__restrict__ src, int h, int w, int cn,
                                                      float *__restrict__ dst, int ho, int wo)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= wo || y >= ho) return;
    int xi[5], yi[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        xi[k] = reflect101(2 * x + k - 2, w);
        yi[k] = reflect101(2 * y + k - 2, h);
    }
    for (int c = 0; c < cn; ++c) {
        float rowv[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float *r = src + (size_t)yi[k] * w * cn + c;
            rowv[k] = ((r[xi[2] * cn] * 6.0f + (r[xi[1] * cn] + r[xi[3] * cn]) * 4.0f) + r[xi[0] * cn]) + r[xi[4] * cn];
        }
        const float v = ((rowv[2] * 6.0f + (rowv[1] + rowv[3]) * 4.0f) + rowv[0]) + rowv[4];
        dst[((size_t)y * wo + x) * cn + c] = v * (1.0f / 256.0f);
    }
}

__device__ __forceinline__ float up_h_hwc(const float *__restrict__ row, int ws, int cn, int x)
{
    const int sx = x >> 1;
    if (ws == 1) return (x & 1) ? row[0] * 8.0f : row[0] * 6.0f + row[0] * 2.0f;
    if (!(x & 1)) {
        if (sx == 0) return row[0] * 6.0f + row[cn] * 2.0f;
        if (sx == ws - 1) return row[(sx - 1) * cn] + row[sx * cn] * 7.0f;
        return (row[(sx - 1) * cn] + row[sx * cn] * 6.0f) + row[(sx + 1) * cn];
    }
    if (sx == ws - 1) return row[sx * cn] * 8.0f;
    return (row[sx * cn] + row[(sx + 1) * cn]) * 4.0f;
}

// MODE 0: dst = up(src); 1: dst = a - up(src); 2: dst = up(src) + a
template <int MODE>
__global__ __launch_bounds__(256) void k_pyr_up_hwc(const float *__restrict__ src, int hs, int ws, int cn,
                                                    const float *__restrict__ a, float *__restrict__ dst, int hd,
                                                    int wd)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= wd || y >= hd) return;
    const int sy = y >> 1;
    const int yp = min(sy + 1, hs - 1);
    const int ym = (sy - 1 < 0) ? (hs > 1 ? 1 : 0) : sy - 1;
    for (int c = 0; c < cn; ++c) {
        const float r1 = up_h_hwc(src + (size_t)sy * ws * cn + c, ws, cn, x);
        const float r2 = up_h_hwc(src + (size_t)yp * ws * cn + c, ws, cn, x);
        float u;
        if (!(y & 1)) {
            const float r0 = up_h_hwc(src + (size_t)ym * ws * cn + c, ws, cn, x);
            u = ((r0 + r1 * 6.0f) + r2) * (1.0f / 64.0f);
        } else {
            u = ((r1 + r2) * 4.0f) * (1.0f / 64.0f);
        }
        const size_t o = ((size_t)y * wd + x) * cn + c;
        if (MODE == 0) dst[o] = u;
        else if (MODE == 1) dst[o] = a[o] - u;
        else dst[o] = u + a[o];
    }
}

// ---------------------------------------------------------------------------------------------
// tile extract
// ---------------------------------------------------------------------------------------------
struct ExtractDesc {
    int x, y, w, h;
    unsigned char *dst;
    long long dstride;
    int out_w, out_h;
};


// One thread = 16 consecutive bytes of one output row.  Inside the source rectangle that is a straight
// copy: one byte-aligned 16-byte load (the source offset x*cn is arbitrary) and one dword-aligned store;
// bytes in the padded band (and ragged tails) take the per-byte border rule.
__global__ __launch_bounds__(256) void k_tile_extract(const unsigned char *__restrict__ img, long long istride,
                                                      int cn, const ExtractDesc *__restrict__ descs, int pad_mode)
{
    const ExtractDesc D = descs[blockIdx.z];
    const int r = blockIdx.y * 4 + threadIdx.y;
    const long long b0 = ((long long)blockIdx.x * 64 + threadIdx.x) * 16;
    const long long row_bytes = (long long)D.out_w * cn;
    if (r >= D.out_h || b0 >= row_bytes) return;
    unsigned char *d = D.dst + (size_t)r * D.dstride + b0;
    if (r < D.h && b0 + 16 <= (long long)D.w * cn) {
        // 16 bytes at any source / destination alignment (tile x and width are arbitrary): the hardware splits an
        // unaligned access; a dword-aligned destination row gets the aligned store
        const unsigned char *sp = img + (size_t)(D.y + r) * istride + (size_t)D.x * cn + b0;
        const u4_t v = *(const u4_a1_t *)sp;
        if (((((size_t)D.dst) | (size_t)D.dstride) & 3) == 0) *(__attribute__((address_space(1))) u4_a4_t *)d = v;
        else *(__attribute__((address_space(1))) u4_a1_t *)d = v;
        return;
    }
    const int nb = (int)min((long long)16, row_bytes - b0);
    for (int i = 0; i < nb; ++i) {
        const long long bb = b0 + i;
        const int c = (int)(bb / cn), k = (int)(bb - (long long)c * cn);
        if (pad_mode == PAD_CONSTANT && (r >= D.h || c >= D.w)) {
            d[i] = 0;
            continue;
        }
        const int sr = border_index(r, D.h, pad_mode), sc = border_index(c, D.w, pad_mode);
        d[i] = img[(size_t)(D.y + sr) * istride + (size_t)(D.x + sc) * cn + k];
    }
}

// ---------------------------------------------------------------------------------------------
// seam scan
// ---------------------------------------------------------------------------------------------
// detect_seams (blending_module.py:765-853): one thread = one window of one tile.  Gray values (BGR2GRAY applied to
// RGB data, i.e. swapped R/B weights, as the reference does) are integers, so the five window sums are exact; the
// global-statistics SSIM of the window is finished in fp64 and windows below the threshold are appended.
struct SeamTile {
    const unsigned char *p;
    long long stride;
    int x, y, w, h;          // canvas position, size
    int roi_w, roi_h;        // part inside the canvas
    int nwx, nwy;            // windows per row / column
    long long first;         // index of this tile's first window in the flat window numbering
    long long bfirst;        // k_seam_scan_cells: index of this tile's first block, and its blocks per block row
    int nbx, pad;
};
struct SeamRec {
    int tile, x, y, pad;
    double score;
};

__global__ __launch_bounds__(256) void k_seam_scan(const unsigned char *__restrict__ canvas, long long cstride, int cn,
                                                   const SeamTile *__restrict__ tiles, int ntiles, long long nwin,
                                                   int window, int stride, int shift, double threshold, double c1,
                                                   double c2, SeamRec *__restrict__ out, int cap, int *__restrict__ count)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= nwin) return;
    int t = 0;
    while (t + 1 < ntiles && tiles[t + 1].first <= gid) ++t;
    const SeamTile T = tiles[t];
    const long long local = gid - T.first;
    const int wy = (int)(local / T.nwx), wx = (int)(local - (long long)wy * T.nwx);
    const int x0 = wx * stride, y0 = wy * stride;
    long long sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    for (int r = 0; r < window; ++r) {
        const unsigned char *pt = T.p + (size_t)(y0 + r) * T.stride + (size_t)x0 * cn;
        const unsigned char *pc = canvas + (size_t)(T.y + y0 + r) * cstride + (size_t)(T.x + x0) * cn;
        for (int c = 0; c < window; ++c) {
            int a, b;
            if (cn == 1) {
                a = pt[c];
                b = pc[c];
            } else {      // BGR2GRAY on RGB data: first channel gets the blue weight
                a = gray_rgb(pt[3 * c + 2], pt[3 * c + 1], pt[3 * c], shift);
                b = gray_rgb(pc[3 * c + 2], pc[3 * c + 1], pc[3 * c], shift);
            }
            sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
        }
    }
    const double n = (double)window * (double)window;
    const double mu1 = (double)sx / n, mu2 = (double)sy / n;
    const double s1 = (double)sxx / n - mu1 * mu1, s2 = (double)syy / n - mu2 * mu2, s12 = (double)sxy / n - mu1 * mu2;
    const double score = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2));
    if (score < threshold) {
        const int k = atomicAdd(count, 1);
        if (k < cap) {
            SeamRec rec;
            rec.tile = t; rec.x = T.x + x0; rec.y = T.y + y0; rec.pad = 0; rec.score = score;
            out[k] = rec;
        }
    }
}

// The default geometry (16 x 16 windows every 8 pixels: window_size 16, stride window_size // 2, blending_module.py:765-903)
// without the 4x redundancy of one thread per window: a window is 2 x 2 cells of 8 x 8 pixels.  One thread = one cell (gray of
// the 64 pixels of tile and canvas, five 32-bit sums: 64 x 255^2 fits), cells of a 32 x 8 block meet in LDS, then one thread
// = one window (four cells: 256 x 255^2 still fits 32 bits) and the reference's formula in fp64.  Same integers, same
// formula: identical scores.  3.3 -> 0.4 ms for the 4.75 M windows of the 200 MP workload.
#define SEAM_CX 32
#define SEAM_CY 8
template <int CN>
__global__ __launch_bounds__(256) void k_seam_scan_cells(const unsigned char *__restrict__ canvas, long long cstride,
                                                         const SeamTile *__restrict__ tiles, int ntiles, int shift, double threshold,
                                                         double c1, double c2, SeamRec *__restrict__ out, int cap, int *__restrict__ count)
{
    __shared__ unsigned cell[5][SEAM_CY][SEAM_CX + 1];
    int t = 0;
    while (t + 1 < ntiles && tiles[t + 1].bfirst <= (long long)blockIdx.x) ++t;
    const SeamTile T = tiles[t];
    const int lb = (int)((long long)blockIdx.x - T.bfirst), by = lb / T.nbx, bx = lb - by * T.nbx;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int cx = bx * (SEAM_CX - 1) + tx, cy = by * (SEAM_CY - 1) + ty;
    unsigned sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    if (cx <= T.nwx && cy <= T.nwy) {                           // nwx + 1 cells per row: the last window ends at 8 (nwx + 1)
#pragma unroll 2
        for (int r = 0; r < 8; ++r) {
            const unsigned char *pt = T.p + (size_t)(8 * cy + r) * T.stride + (size_t)(8 * cx) * CN;
            const unsigned char *pc = canvas + (size_t)(T.y + 8 * cy + r) * cstride + (size_t)(T.x + 8 * cx) * CN;
            unsigned wa[6], wb[6];
            if (CN == 3) {
                const u3_t a0 = ld_u3_a1_g(pt), a1 = ld_u3_a1_g(pt + 12), b0 = ld_u3_a1_g(pc), b1 = ld_u3_a1_g(pc + 12);
                wa[0] = a0.x; wa[1] = a0.y; wa[2] = a0.z; wa[3] = a1.x; wa[4] = a1.y; wa[5] = a1.z;
                wb[0] = b0.x; wb[1] = b0.y; wb[2] = b0.z; wb[3] = b1.x; wb[4] = b1.y; wb[5] = b1.z;
            } else {
                wa[0] = *(const u1_a1_t *)pt; wa[1] = *(const u1_a1_t *)(pt + 4);
                wb[0] = *(const u1_a1_t *)pc; wb[1] = *(const u1_a1_t *)(pc + 4);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int a, b;
                if (CN == 3) {                                  // BGR2GRAY on RGB data: first channel gets the blue weight
                    const int i0 = 3 * k, i1 = 3 * k + 1, i2 = 3 * k + 2;
                    a = gray_rgb((int)((wa[i2 >> 2] >> (8 * (i2 & 3))) & 0xFFu), (int)((wa[i1 >> 2] >> (8 * (i1 & 3))) & 0xFFu),
                                 (int)((wa[i0 >> 2] >> (8 * (i0 & 3))) & 0xFFu), shift);
                    b = gray_rgb((int)((wb[i2 >> 2] >> (8 * (i2 & 3))) & 0xFFu), (int)((wb[i1 >> 2] >> (8 * (i1 & 3))) & 0xFFu),
                                 (int)((wb[i0 >> 2] >> (8 * (i0 & 3))) & 0xFFu), shift);
                } else {
                    a = (int)((wa[k >> 2] >> (8 * (k & 3))) & 0xFFu);
                    b = (int)((wb[k >> 2] >> (8 * (k & 3))) & 0xFFu);
                }
                sx += (unsigned)a; sy += (unsigned)b;
                sxx += (unsigned)__mul24(a, a); syy += (unsigned)__mul24(b, b); sxy += (unsigned)__mul24(a, b);
            }
        }
    }
    cell[0][ty][tx] = sx; cell[1][ty][tx] = sy; cell[2][ty][tx] = sxx; cell[3][ty][tx] = syy; cell[4][ty][tx] = sxy;
    __syncthreads();
    if (tx >= SEAM_CX - 1 || ty >= SEAM_CY - 1 || cx >= T.nwx || cy >= T.nwy) return;
    unsigned w[5];
#pragma unroll
    for (int m = 0; m < 5; ++m) w[m] = (cell[m][ty][tx] + cell[m][ty][tx + 1]) + (cell[m][ty + 1][tx] + cell[m][ty + 1][tx + 1]);
    const double n = 256.0;
    const double mu1 = (double)w[0] / n, mu2 = (double)w[1] / n;
    const double s1 = (double)w[2] / n - mu1 * mu1, s2 = (double)w[3] / n - mu2 * mu2, s12 = (double)w[4] / n - mu1 * mu2;
    const double score = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2));
    if (score < threshold) {
        const int k = atomicAdd(count, 1);
        if (k < cap) {
            SeamRec rec;
            rec.tile = t; rec.x = T.x + 8 * cx; rec.y = T.y + 8 * cy; rec.pad = 0; rec.score = score;
            out[k] = rec;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// TilingModule.merge_tiles feather path (tiling_module.py:1074-1175), canvas-centric
// ---------------------------------------------------------------------------------------------
struct MergeDev {
    int x, y, src_w, src_h, out_w, out_h;
    int ov_t, ov_b, ov_l, ov_r;
    int resize;          // 1: bilinear resize src -> out
    int xtab, ytab;      // offsets into the LinTab array
    double st, sb, sl, sr;  // np.linspace steps: +1/(ov-1) (top/left), -1/(ov-1) (bottom/right); 0 when ov == 1
};

template <int DT>
__global__ __launch_bounds__(256) void k_feather_merge(const MergeDev *__restrict__ tiles, const TileSrc *__restrict__ srcs,
                                                       const LinTab *__restrict__ tabs, int n, int blending,
                                                       unsigned char *__restrict__ canvas, long long cstride, int ch,
                                                       int cw)
{
    // tiles that touch this 256 x 4 pixel block, in list order (wave 0, ballot-compacted): a canvas pixel is covered by
    // 1-4 of the n tiles, so the per-pixel loop runs over this short list instead of all of them
    __shared__ int s_cnt;
    __shared__ int s_list[64];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    const int bx0 = blockIdx.x * 256, by0 = blockIdx.y * 4;
    if (tid < 64) {
        int cnt = 0;
        for (int base = 0; base < n; base += 64) {
            const int t = base + tid;
            bool hit = false;
            if (t < n) {
                const MergeDev &T = tiles[t];
                hit = T.x < bx0 + 256 && T.x + T.out_w > bx0 && T.y < by0 + 4 && T.y + T.out_h > by0;
            }
            const unsigned long long m = __ballot(hit);
            if (hit) {
                const int pos = cnt + __popcll(m & ((1ull << tid) - 1ull));
                if (pos < 64) s_list[pos] = t;
            }
            cnt += __popcll(m);
        }
        if (tid == 0) s_cnt = cnt;
    }
    __syncthreads();
    const int ncand = s_cnt;
    const bool listed = ncand <= 64;                 // more than 64 tiles over one block: walk all of them
    // one thread = 4 consecutive canvas pixels of one row: the row part of the weight is formed once, unresized tile
    // pixels come in one 12-byte load
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= cw || y >= ch) return;
    const int nx = min(4, cw - x0);
    // Blocks that lie inside ONE unresized u8 tile, beyond its ramps (58 % of a 5 x 5 grid's canvas): weight exactly 1, so
    // acc = p * 1, wacc = 1, p / 1 = p -- the pixel itself: a copy (0.67 -> 0.58 ms for 25 tiles / 200 MP).  Building the
    // tile list once per 16 rows instead of 4, with the descriptors in LDS, was measured too: no change (0.60 ms).
    if (DT == SRC_U8 && ncand == 1) {
        const MergeDev &T = tiles[s_list[0]];
        const int fl = blending ? T.ov_l : 0, fr = blending ? T.ov_r : 0, ft = blending ? T.ov_t : 0, fb = blending ? T.ov_b : 0;
        if (!T.resize && bx0 >= T.x + fl && min(bx0 + 256, cw) <= T.x + T.out_w - fr && by0 >= T.y + ft &&
            min(by0 + 4, ch) <= T.y + T.out_h - fb) {
            const unsigned char *sp = (const unsigned char *)srcs[s_list[0]].p + (size_t)(y - T.y) * srcs[s_list[0]].stride +
                                      (size_t)(x0 - T.x) * 3;
            unsigned char *o = canvas + (size_t)y * cstride + (size_t)x0 * 3;
            if (nx == 4) {
                const u3_t q = ld_u3_a1_g(sp);
                *(__attribute__((address_space(1))) u3_a1_t *)o = q;
            } else {
                for (int i = 0; i < 3 * nx; ++i) o[i] = sp[i];
            }
            return;
        }
    }
    float acc[4][3], wacc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        wacc[k] = 0.f;
        acc[k][0] = acc[k][1] = acc[k][2] = 0.f;
    }
    for (int i = 0; i < (listed ? ncand : n); ++i) {
        const int t = listed ? s_list[i] : i;
        const MergeDev &T = tiles[t];
        const int lx0 = x0 - T.x, ly = y - T.y;
        if (lx0 + nx <= 0 || ly < 0 || lx0 >= T.out_w || ly >= T.out_h) continue;
        // weight[:t] *= linspace(0,1,t); weight[-b:] *= linspace(1,0,b); then columns -- each product in float64,
        // rounded to fp32 (NumPy's in-place multiply of an fp32 array by an fp64 ramp).  Rows first: shared by the 4 px.
        float wy = 1.0f;
        if (blending) {
            if (T.ov_t > 0 && ly < T.ov_t) {
                const double r = (ly == T.ov_t - 1 && T.ov_t > 1) ? 1.0 : (double)ly * T.st + 0.0;
                wy = (float)((double)wy * r);
            }
            if (T.ov_b > 0 && ly >= T.out_h - T.ov_b) {
                const int j = ly - (T.out_h - T.ov_b);
                const double r = (j == T.ov_b - 1 && T.ov_b > 1) ? 0.0 : (double)j * T.sb + 1.0;
                wy = (float)((double)wy * r);
            }
        }
        const unsigned char *base = (const unsigned char *)srcs[t].p;
        const long long st = srcs[t].stride;
        const bool whole = lx0 >= 0 && lx0 + 3 < T.out_w && nx == 4;
        unsigned pix[12];
        if (DT == SRC_U8 && !T.resize && whole) {
            const u3_t q = ld_u3_a1_g(base + (size_t)ly * st + (size_t)lx0 * 3);
            const unsigned wd[3] = {q.x, q.y, q.z};
#pragma unroll
            for (int b = 0; b < 12; ++b) pix[b] = (wd[b >> 2] >> (8 * (b & 3))) & 0xFFu;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lx = lx0 + k;
            if (k >= nx || lx < 0 || lx >= T.out_w) continue;
            float w = wy;
            if (blending) {
                if (T.ov_l > 0 && lx < T.ov_l) {
                    const double r = (lx == T.ov_l - 1 && T.ov_l > 1) ? 1.0 : (double)lx * T.sl + 0.0;
                    w = (float)((double)w * r);
                }
                if (T.ov_r > 0 && lx >= T.out_w - T.ov_r) {
                    const int j = lx - (T.out_w - T.ov_r);
                    const double r = (j == T.ov_r - 1 && T.ov_r > 1) ? 0.0 : (double)j * T.sr + 1.0;
                    w = (float)((double)w * r);
                }
            }
            if (DT == SRC_F32) {
                // float tile data (tiling_module.py:1104-1109: astype(float32), or cv2.resize's float INTER_LINEAR path --
                // rows first, S[x0] * (1 - fx) + S[x1] * fx, then the same between the two rows; parity unpinned)
                if (T.resize) {
                    const LinTab X = tabs[T.xtab + lx], Y = tabs[T.ytab + ly];
                    const int x1 = min(X.ofs + 1, T.src_w - 1), y1 = min(Y.ofs + 1, T.src_h - 1);
                    const float *r0 = (const float *)(base + (size_t)Y.ofs * st), *r1 = (const float *)(base + (size_t)y1 * st);
                    const float ax0 = 1.0f - X.f, ax1 = X.f, ay0 = 1.0f - Y.f, ay1 = Y.f;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float s0 = r0[X.ofs * 3 + c] * ax0 + r0[x1 * 3 + c] * ax1;
                        const float s1 = r1[X.ofs * 3 + c] * ax0 + r1[x1 * 3 + c] * ax1;
                        acc[k][c] += (s0 * ay0 + s1 * ay1) * w;
                    }
                } else {
                    const float *r0 = (const float *)(base + (size_t)ly * st) + (size_t)lx * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[k][c] += r0[c] * w;
                }
            } else if (T.resize) {
                const LinTab X = tabs[T.xtab + lx], Y = tabs[T.ytab + ly];
                const int x1 = min(X.ofs + 1, T.src_w - 1), y1 = min(Y.ofs + 1, T.src_h - 1);
                const unsigned char *r0 = base + (size_t)Y.ofs * st, *r1 = base + (size_t)y1 * st;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int v = lin_u8(r0, r1, X.ofs * 3 + c, x1 * 3 + c, X, Y);
                    acc[k][c] += (float)(unsigned char)v * w;
                }
            } else if (whole) {
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[k][c] += (float)pix[3 * k + c] * w;
            } else {
                const unsigned char *r0 = base + (size_t)ly * st + (size_t)lx * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[k][c] += (float)r0[c] * w;
            }
            wacc[k] += w;
        }
    }
    unsigned ob[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float wv = wacc[k] > 1e-6f ? wacc[k] : 1e-6f;
        float q[3];
        div_shared<3>(acc[k], wv, q);             // the IEEE quotients, one reciprocal per pixel (see the final gather)
#pragma unroll
        for (int c = 0; c < 3; ++c) ob[3 * k + c] = (unsigned)(unsigned char)(int)q[c];   // astype(uint8): truncation, no clip
    }
    unsigned char *o = canvas + (size_t)y * cstride + (size_t)x0 * 3;
    if (nx == 4 && ((cstride & 3) == 0) && ((((size_t)canvas) & 3) == 0)) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
            ((unsigned *)o)[q] = ob[4 * q] | (ob[4 * q + 1] << 8) | (ob[4 * q + 2] << 16) | (ob[4 * q + 3] << 24);
    } else {
        for (int k = 0; k < nx; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) o[3 * k + c] = (unsigned char)ob[3 * k + c];
    }
}

extern "C" {

// ---- tile extract ------------------------------------------------------------------------------
static int extract_impl(sr_ctx *ctx, const uint8_t *d_img, int img_h, int img_w, int cn, int64_t img_stride,
                        const std::vector<ExtractDesc> &descs, int pad_mode, const char *name)
{
    const int n = (int)descs.size();
    if (n == 0) return SR_OK;
    int mw = 0, mh = 0;
    for (auto &d : descs) {
        if (d.x < 0 || d.y < 0 || d.w <= 0 || d.h <= 0 || d.x + d.w > img_w || d.y + d.h > img_h)
            return sr_set_error(SR_ERR_SHAPE, "%s: tile (%d,%d,%d,%d) outside the %dx%d image", name, d.x, d.y, d.w,
                                d.h, img_w, img_h);
        mw = std::max(mw, d.out_w);
        mh = std::max(mh, d.out_h);
    }
    SRCHK(upload_cached(ctx, ctx->extract_tab, descs.data(), sizeof(ExtractDesc) * n));
    const void *scr = ctx->extract_tab.buf.d;
    {
        ProfScope ps(ctx, name);
        const long long chunks = ((long long)mw * cn + 15) / 16;
        dim3 grid((unsigned)((chunks + 63) / 64), (mh + 3) / 4, n), block(64, 4);
        hipLaunchKernelGGL(k_tile_extract, grid, block, 0, ctx->stream, d_img, (long long)img_stride, cn,
                           (const ExtractDesc *)scr, pad_mode);
    }
    return check_launch(name);
}

int sr_tile_extract_pad(sr_ctx *ctx, const uint8_t *d_img, int img_h, int img_w, int cn, int64_t img_stride,
                        const int *h_xywh, int n, int block_size, int pad_mode, uint8_t *d_tiles)
{
    CTX_ENTER(ctx);
    if (!d_img || !h_xywh || !d_tiles || n < 0 || cn < 1 || cn > 4 || block_size <= 0 || pad_mode < 0 || pad_mode > 3)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_tile_extract_pad: bad arguments");
    std::vector<ExtractDesc> descs(n);
    for (int i = 0; i < n; ++i) {
        ExtractDesc &d = descs[i];
        d.x = h_xywh[4 * i];
        d.y = h_xywh[4 * i + 1];
        d.w = h_xywh[4 * i + 2];
        d.h = h_xywh[4 * i + 3];
        if (d.w > block_size || d.h > block_size)
            return sr_set_error(SR_ERR_SHAPE, "sr_tile_extract_pad: tile %d larger than block_size", i);
        d.dst = d_tiles + (size_t)i * block_size * block_size * cn;
        d.dstride = (long long)block_size * cn;
        d.out_w = d.out_h = block_size;
    }
    return extract_impl(ctx, d_img, img_h, img_w, cn, img_stride, descs, pad_mode, "tile_extract_pad");
}

int sr_tile_extract(sr_ctx *ctx, const uint8_t *d_img, int img_h, int img_w, int cn, int64_t img_stride,
                    const int *h_xywh, int n, void *const *h_d_tiles, const int64_t *h_tile_strides)
{
    CTX_ENTER(ctx);
    if (!d_img || !h_xywh || !h_d_tiles || !h_tile_strides || n < 0 || cn < 1 || cn > 4)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_tile_extract: bad arguments");
    std::vector<ExtractDesc> descs(n);
    for (int i = 0; i < n; ++i) {
        ExtractDesc &d = descs[i];
        d.x = h_xywh[4 * i];
        d.y = h_xywh[4 * i + 1];
        d.w = h_xywh[4 * i + 2];
        d.h = h_xywh[4 * i + 3];
        d.dst = (unsigned char *)h_d_tiles[i];
        d.dstride = h_tile_strides[i];
        d.out_w = d.w;
        d.out_h = d.h;
    }
    return extract_impl(ctx, d_img, img_h, img_w, cn, img_stride, descs, PAD_REPLICATE, "tile_extract");
}

// ---- dense pyramid primitives --------------------------------------------------------------------
int sr_pyr_down(sr_ctx *ctx, const float *d_src, int h, int w, int cn, float *d_dst)
{
    CTX_ENTER(ctx);
    if (!d_src || !d_dst || h < 1 || w < 1 || cn < 1 || cn > 4)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_pyr_down: bad arguments");
    const int ho = (h + 1) / 2, wo = (w + 1) / 2;
    {
        ProfScope ps(ctx, "pyr_down_hwc");
        dim3 grid((wo + 63) / 64, (ho + 3) / 4), block(64, 4);
        hipLaunchKernelGGL(k_pyr_down_hwc, grid, block, 0, ctx->stream, d_src, h, w, cn, d_dst, ho, wo);
    }
    return check_launch("pyr_down_hwc");
}

static int pyr_up_impl(sr_ctx *ctx, int mode, const float *d_src, int hs, int ws, int cn, const float *d_a,
                       float *d_dst, int hd, int wd)
{
    if (!d_src || !d_dst || hs < 1 || ws < 1 || cn < 1 || cn > 4 || (mode && !d_a))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_pyr_up: bad arguments");
    if ((wd != 2 * ws && wd != 2 * ws - 1) || (hd != 2 * hs && hd != 2 * hs - 1) || wd < 1 || hd < 1)
        return sr_set_error(SR_ERR_SHAPE, "sr_pyr_up: dst %dx%d is not 2x(-1) of src %dx%d", wd, hd, ws, hs);
    {
        ProfScope ps(ctx, "pyr_up_hwc");
        dim3 grid((wd + 63) / 64, (hd + 3) / 4), block(64, 4);
        if (mode == 0) hipLaunchKernelGGL(k_pyr_up_hwc<0>, grid, block, 0, ctx->stream, d_src, hs, ws, cn, d_a, d_dst, hd, wd);
        else if (mode == 1) hipLaunchKernelGGL(k_pyr_up_hwc<1>, grid, block, 0, ctx->stream, d_src, hs, ws, cn, d_a, d_dst, hd, wd);
        else hipLaunchKernelGGL(k_pyr_up_hwc<2>, grid, block, 0, ctx->stream, d_src, hs, ws, cn, d_a, d_dst, hd, wd);
    }
    return check_launch("pyr_up_hwc");
}

int sr_pyr_up(sr_ctx *ctx, const float *d_src, int hs, int ws, int cn, float *d_dst, int hd, int wd)
{
    CTX_ENTER(ctx);
    return pyr_up_impl(ctx, 0, d_src, hs, ws, cn, nullptr, d_dst, hd, wd);
}

int sr_pyr_up_sub(sr_ctx *ctx, const float *d_a, int h, int w, int cn, const float *d_b, float *d_out)
{
    CTX_ENTER(ctx);
    return pyr_up_impl(ctx, 1, d_b, (h + 1) / 2, (w + 1) / 2, cn, d_a, d_out, h, w);
}

int sr_pyr_up_add(sr_ctx *ctx, const float *d_a, int h, int w, int cn, const float *d_b, float *d_out)
{
    CTX_ENTER(ctx);
    return pyr_up_impl(ctx, 2, d_b, (h + 1) / 2, (w + 1) / 2, cn, d_a, d_out, h, w);
}

// ---- feather merge ------------------------------------------------------------------------------
int sr_feather_merge(sr_ctx *ctx, const sr_merge_tile *h_tiles, int n, void *const *h_d_tiles,
                     const int64_t *h_strides, int blending, uint8_t *d_canvas, int64_t canvas_stride, int canvas_h,
                     int canvas_w)
{
    return sr_feather_merge_dt(ctx, SR_U8, h_tiles, n, h_d_tiles, h_strides, blending, d_canvas, canvas_stride, canvas_h, canvas_w);
}

int sr_feather_merge_dt(sr_ctx *ctx, int dtype, const sr_merge_tile *h_tiles, int n, void *const *h_d_tiles,
                        const int64_t *h_strides, int blending, uint8_t *d_canvas, int64_t canvas_stride, int canvas_h,
                        int canvas_w)
{
    CTX_ENTER(ctx);
    if (!h_tiles || !h_d_tiles || !h_strides || !d_canvas || n < 0 || canvas_h < 1 || canvas_w < 1)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_feather_merge: bad arguments");
    if (dtype != SR_U8 && dtype != SR_F32) return sr_set_error(SR_ERR_INVALID_ARG, "sr_feather_merge: dtype must be SR_U8 or SR_F32");
    const int es = dtype == SR_U8 ? 1 : 4;
    if (canvas_stride < (int64_t)canvas_w * 3) return sr_set_error(SR_ERR_SHAPE, "sr_feather_merge: canvas stride too small");
    std::vector<MergeDev> md(n);
    std::vector<TileSrc> srcs(n);
    std::vector<LinTab> tabs;
    for (int t = 0; t < n; ++t) {
        const sr_merge_tile &m = h_tiles[t];
        if (m.src_w < 1 || m.src_h < 1 || m.out_w < 1 || m.out_h < 1 || m.x < 0 || m.y < 0 || !h_d_tiles[t])
            return sr_set_error(SR_ERR_INVALID_ARG, "sr_feather_merge: tile %d has a bad descriptor", t);
        if (blending && (m.ov_t > m.out_h || m.ov_b > m.out_h || m.ov_l > m.out_w || m.ov_r > m.out_w))
            return sr_set_error(SR_ERR_SHAPE,
                                "sr_feather_merge: tile %d: overlap ramp longer than the tile (NumPy cannot broadcast "
                                "the reference's ramp either)", t);
        MergeDev &D = md[t];
        D.x = m.x; D.y = m.y; D.src_w = m.src_w; D.src_h = m.src_h; D.out_w = m.out_w; D.out_h = m.out_h;
        D.ov_t = std::max(m.ov_t, 0); D.ov_b = std::max(m.ov_b, 0); D.ov_l = std::max(m.ov_l, 0); D.ov_r = std::max(m.ov_r, 0);
        D.resize = (m.src_w != m.out_w || m.src_h != m.out_h) ? 1 : 0;
        D.xtab = D.ytab = 0;
        if (D.resize) {
            D.xtab = (int)tabs.size();
            linear_table(m.src_w, m.out_w, tabs);
            D.ytab = (int)tabs.size();
            linear_table(m.src_h, m.out_h, tabs);
        }
        auto step = [](int ov, double delta) { return ov > 1 ? delta / (double)(ov - 1) : 0.0; };
        D.st = step(D.ov_t, 1.0); D.sb = step(D.ov_b, -1.0); D.sl = step(D.ov_l, 1.0); D.sr = step(D.ov_r, -1.0);
        srcs[t].p = h_d_tiles[t];
        srcs[t].stride = h_strides[t];
        if (h_strides[t] < (int64_t)m.src_w * 3 * es) return sr_set_error(SR_ERR_SHAPE, "sr_feather_merge: tile %d stride too small", t);
    }
    const size_t b0 = sizeof(MergeDev) * (size_t)n, b1 = sizeof(TileSrc) * (size_t)n, b2 = sizeof(LinTab) * tabs.size();
    void *scr = nullptr;
    int rc = ctx_scratch(ctx, up256(b0) + up256(b1) + up256(b2) + 256, &scr);
    if (rc) return rc;
    char *p0 = (char *)scr, *p1 = p0 + up256(b0), *p2 = p1 + up256(b1);
    if (n > 0) {
        HIPCHK(upload_small(ctx, p0, md.data(), b0));
        HIPCHK(upload_small(ctx, p1, srcs.data(), b1));
        if (b2) HIPCHK(upload_small(ctx, p2, tabs.data(), b2));
    }
    {
        ProfScope ps(ctx, "feather_merge");
        dim3 grid((canvas_w + 255) / 256, (canvas_h + 3) / 4), block(64, 4);
        if (dtype == SR_U8)
            hipLaunchKernelGGL(k_feather_merge<SRC_U8>, grid, block, 0, ctx->stream, (const MergeDev *)p0, (const TileSrc *)p1,
                               (const LinTab *)p2, n, blending ? 1 : 0, d_canvas, (long long)canvas_stride, canvas_h, canvas_w);
        else
            hipLaunchKernelGGL(k_feather_merge<SRC_F32>, grid, block, 0, ctx->stream, (const MergeDev *)p0, (const TileSrc *)p1,
                               (const LinTab *)p2, n, blending ? 1 : 0, d_canvas, (long long)canvas_stride, canvas_h, canvas_w);
    }
    return check_launch("feather_merge");
}

// ---- seam scan ------------------------------------------------------------------------------------
int sr_seam_scan(sr_ctx *ctx, const uint8_t *d_canvas, int64_t canvas_stride, int canvas_h, int canvas_w, int cn,
                 const sr_tile_rect *h_rects, void *const *h_d_tiles, const int64_t *h_strides, int n, int window,
                 int stride, int gray_shift, double threshold, sr_seam_record *h_out, int cap, int *h_count)
{
    CTX_ENTER(ctx);
    if (!d_canvas || !h_rects || !h_d_tiles || !h_strides || !h_count || n < 0 || (cap > 0 && !h_out))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_seam_scan: null argument");
    if ((cn != 1 && cn != 3) || window < 1 || stride < 1 || (gray_shift != 14 && gray_shift != 15))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_seam_scan: bad channel count / window / stride / gray_shift");
    *h_count = 0;
    std::vector<SeamTile> st;
    long long nwin = 0, nblk_cells = 0;
    for (int t = 0; t < n; ++t) {
        const sr_tile_rect &r = h_rects[t];
        if (r.x < 0 || r.y < 0 || r.w < 1 || r.h < 1 || !h_d_tiles[t]) return sr_set_error(SR_ERR_INVALID_ARG, "sr_seam_scan: bad tile %d", t);
        SeamTile T;
        T.p = (const unsigned char *)h_d_tiles[t];
        T.stride = h_strides[t];
        T.x = r.x; T.y = r.y; T.w = r.w; T.h = r.h;
        T.roi_w = std::min(r.x + r.w, canvas_w) - r.x;
        T.roi_h = std::min(r.y + r.h, canvas_h) - r.y;
        T.nwx = T.roi_w >= window ? (T.roi_w - window) / stride + 1 : 0;
        T.nwy = T.roi_h >= window ? (T.roi_h - window) / stride + 1 : 0;
        if (T.roi_w <= 0 || T.roi_h <= 0) T.nwx = T.nwy = 0;
        T.first = nwin;
        nwin += (long long)T.nwx * T.nwy;
        T.nbx = (T.nwx + SEAM_CX - 2) / (SEAM_CX - 1);
        T.pad = 0;
        T.bfirst = nblk_cells;
        nblk_cells += (long long)T.nbx * ((T.nwy + SEAM_CY - 2) / (SEAM_CY - 1));
        st.push_back(T);
    }
    if (nwin == 0) return SR_OK;
    const size_t b_tiles = (sizeof(SeamTile) * st.size() + 255) / 256 * 256;
    const size_t b_out = sizeof(SeamRec) * (size_t)std::max(cap, 1);
    void *scr = nullptr;
    int rc = ctx_scratch(ctx, b_tiles + b_out + 512, &scr);
    if (rc) return rc;
    SeamTile *d_t = (SeamTile *)scr;
    int *d_cnt = (int *)((char *)scr + b_tiles);
    SeamRec *d_out = (SeamRec *)((char *)scr + b_tiles + 256);
    HIPCHK(upload_small(ctx, d_t, st.data(), sizeof(SeamTile) * st.size()));
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(int), ctx->stream));
    {
        ProfScope ps(ctx, "seam_scan");
        const double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
        if (window == 16 && stride == 8 && nblk_cells < (1ll << 31)) {         // the reference's default geometry: cell kernel
            const dim3 block(SEAM_CX, SEAM_CY);
            if (cn == 3) hipLaunchKernelGGL(k_seam_scan_cells<3>, dim3((unsigned)nblk_cells), block, 0, ctx->stream, d_canvas, (long long)canvas_stride,
                                            (const SeamTile *)d_t, (int)st.size(), gray_shift, threshold, c1, c2, d_out, cap, d_cnt);
            else hipLaunchKernelGGL(k_seam_scan_cells<1>, dim3((unsigned)nblk_cells), block, 0, ctx->stream, d_canvas, (long long)canvas_stride,
                                    (const SeamTile *)d_t, (int)st.size(), gray_shift, threshold, c1, c2, d_out, cap, d_cnt);
        } else {
            const long long blocks = (nwin + 255) / 256;
            hipLaunchKernelGGL(k_seam_scan, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_canvas, (long long)canvas_stride, cn,
                               (const SeamTile *)d_t, (int)st.size(), nwin, window, stride, gray_shift, threshold, c1, c2, d_out, cap, d_cnt);
        }
    }
    rc = check_launch("seam_scan");
    if (rc) return rc;
    int cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, d_cnt, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    *h_count = cnt;
    const int ncopy = std::min(cnt, cap);
    if (ncopy > 0) {
        static_assert(sizeof(SeamRec) == sizeof(sr_seam_record), "record layouts must match");
        HIPCHK(hipMemcpyAsync(h_out, d_out, sizeof(SeamRec) * (size_t)ncopy, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(stream_sync(ctx));
    }
    return SR_OK;
}

}  // extern "C"
