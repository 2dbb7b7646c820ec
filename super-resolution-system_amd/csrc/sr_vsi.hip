// sr_vsi.hip -- VSI of two u8 images (sr_vsi_u8), with the inspection entries sr_vsi_pool_u8 and sr_vsi_saliency_u8.  The
// definition is in include/sr_hip.h; F, the sizes, the workspace layout, the resize and composite pooling tables, LG, SD and
// every shape refusal are sr_vsi_host.cpp's.
//
//   k_vsi_resize_v / k_vsi_resize_h
//                     the two passes of the antialiased triangle resize to the 256 x 256 grid, over u8 pixels (first pass) or
//                     the float64 intermediate (second pass: 256 x w x 3 or h x 256 x 3 in global memory, 1 / 7 of a u8
//                     source at 1 / 55 and far smaller than an LDS tile scheme's apron at that scale).  The vertical pass
//                     gives a thread one byte column and walks the taps' rows: adjacent lanes read adjacent bytes, and the
//                     twofold overlap of neighbouring windows is the only re-read.  The horizontal pass gives a wave one output:
//                     its lanes stride over the taps (adjacent lanes, adjacent pixels) and a fixed LDS tree adds them.
//   k_vsi_lab / k_vsi_range
//                     the script's RGB2Lab of the 65 536 samples with per-block min / max of a and b, then their tree.
//   k_vsi_centre, k_vsi_dft_cols / k_vsi_dft_rows
//                     FSIM's dense float64 DFT instantiated for n = 256 (index products reduced by a mask), three planes on
//                     the grid's z; the inverse column pass multiplies the spectrum by LG on the way in.
//   k_vsi_sal         SF SD SC per grid sample.
//   k_vsi_up_cols, k_vsi_expand / k_vsi_minmax
//                     the full-resolution map, never stored: the horizontal up-resize of the 256 rows (256 x w float64), then
//                     every sample as the 2 .. 3 vertical taps of its column, reduced to min / max per block and by one tree.
//   k_vsi_band_cols / k_vsi_band_rows
//                     the raw window sums of the map straight from VS256 by the composite tables C_x, C_y.
//   k_vsi_pool<CN>    FSIM's one-pass pooling with VSI's L, M, N coefficients into six int64 planes.
//   k_vsi_score       Scharr on the integer sums, mat2gray of the pooled map, the similarity maps and both sums through a fixed
//                     tree; reduce_partials finishes them: no floating-point atomics, equal inputs give equal bits.
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_ctx.h"
#include "sr_vsi.h"

namespace {

typedef double2 cpx;
constexpr int DT = VSI_DFT_TILE;
constexpr int NMASK = VSI_N - 1;

// ---- the resize to the grid ------------------------------------------------------------------------------------------------------
// out[i][x][c] = sum_k wt[i][k] in[idx[i][k]][x][c], c < 3; grid (ceil(3 wpix / 256), outputs).  PLANAR (wpix = 256): out[c][i][x].
template <typename T, int CN, bool PLANAR>
__global__ __launch_bounds__(VSI_THREADS) void k_vsi_resize_v(const T *__restrict__ in, long long stride, int wpix,
                                                              const double *__restrict__ wt, const int *__restrict__ idx, int taps,
                                                              double *__restrict__ out)
{
    const long long e = (long long)blockIdx.x * VSI_THREADS + threadIdx.x;
    if (e >= 3LL * wpix) return;
    const int x = (int)(e / 3), c = (int)(e - 3LL * x), i = (int)blockIdx.y;
    const double *wr = wt + (size_t)i * taps;
    const int *ir = idx + (size_t)i * taps;
    double acc = 0.0;
    for (int k = 0; k < taps; ++k) {
        const T *row = (const T *)((const char *)in + (size_t)ir[k] * (size_t)stride);
        acc += wr[k] * (double)row[(size_t)x * CN + c];
    }
    if (PLANAR) out[(size_t)c * VSI_NN + (size_t)i * VSI_N + x] = acc;
    else out[((size_t)i * wpix + x) * 3 + c] = acc;
}

// out[r][j][c] = sum_k wt[j][k] in[r][idx[j][k]][c]; grid (rows, 64): a block's four waves own four outputs j of one row.
template <typename T, int CN, bool PLANAR>
__global__ __launch_bounds__(VSI_THREADS) void k_vsi_resize_h(const T *__restrict__ in, long long stride,
                                                              const double *__restrict__ wt, const int *__restrict__ idx, int taps,
                                                              double *__restrict__ out)
{
    __shared__ double sh[3][VSI_THREADS];
    const int t = threadIdx.x, lane = t & 63, j = (int)blockIdx.y * (VSI_THREADS / 64) + (t >> 6);
    const size_t r = blockIdx.x;
    const T *row = (const T *)((const char *)in + r * (size_t)stride);
    const double *wr = wt + (size_t)j * taps;
    const int *ir = idx + (size_t)j * taps;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int k = lane; k < taps; k += 64) {
        const T *px = row + (size_t)ir[k] * CN;
        const double wk = wr[k];
        a0 += wk * (double)px[0];
        a1 += wk * (double)px[1];
        a2 += wk * (double)px[2];
    }
    sh[0][t] = a0;
    sh[1][t] = a1;
    sh[2][t] = a2;
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
        if (lane < s) {
            sh[0][t] += sh[0][t + s];
            sh[1][t] += sh[1][t + s];
            sh[2][t] += sh[2][t + s];
        }
        __syncthreads();
    }
    if (lane != 0) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (PLANAR) out[(size_t)c * VSI_NN + r * VSI_N + j] = sh[c][t];
        else out[(r * VSI_N + j) * 3 + c] = sh[c][t];
    }
}

// ---- Lab and the ranges ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VSI_THREADS) void k_vsi_lab(const double *__restrict__ rgb, double *__restrict__ lab,
                                                         double *__restrict__ rpart)
{
    __shared__ double sh[4][VSI_THREADS];
    const int t = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * VSI_THREADS + t;      // the grid covers 65536 exactly
    double L, A, B;
    vsi_rgb2lab(rgb[i], rgb[VSI_NN + i], rgb[2 * (size_t)VSI_NN + i], &L, &A, &B);
    lab[i] = L;
    lab[VSI_NN + i] = A;
    lab[2 * (size_t)VSI_NN + i] = B;
    sh[0][t] = A;
    sh[1][t] = A;
    sh[2][t] = B;
    sh[3][t] = B;
    __syncthreads();
    for (int s = VSI_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            sh[0][t] = vsi_min(sh[0][t], sh[0][t + s]);
            sh[1][t] = vsi_max(sh[1][t], sh[1][t + s]);
            sh[2][t] = vsi_min(sh[2][t], sh[2][t + s]);
            sh[3][t] = vsi_max(sh[3][t], sh[3][t + s]);
        }
        __syncthreads();
    }
    if (t < 4) rpart[(size_t)blockIdx.x * 4 + t] = sh[t][0];
}

// One block: the tree over the 256 per-block ranges -> range[0 .. 3]
__global__ __launch_bounds__(VSI_THREADS) void k_vsi_range(const double *__restrict__ rpart, double *__restrict__ range)
{
    __shared__ double sh[4][VSI_THREADS];
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 4; ++q) sh[q][t] = rpart[(size_t)t * 4 + q];
    __syncthreads();
    for (int s = VSI_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            sh[0][t] = vsi_min(sh[0][t], sh[0][t + s]);
            sh[1][t] = vsi_max(sh[1][t], sh[1][t + s]);
            sh[2][t] = vsi_min(sh[2][t], sh[2][t + s]);
            sh[3][t] = vsi_max(sh[3][t], sh[3][t + s]);
        }
        __syncthreads();
    }
    if (t < 4) range[t] = sh[t][0];
}

// ---- the dense transform, n = 256 -----------------------------------------------------------------------------------------------
// the transform's input: each plane less its first sample (LG is 0 at DC); grid (256, 3)
__global__ __launch_bounds__(VSI_THREADS) void k_vsi_centre(const double *__restrict__ lab, cpx *__restrict__ out)
{
    const size_t z = blockIdx.y, i = (size_t)blockIdx.x * VSI_THREADS + threadIdx.x;
    const double *pl = lab + z * VSI_NN;
    out[z * VSI_NN + i] = make_double2(pl[i] - pl[0], 0.0);
}

// Along the columns of a row: out[z][m][j] = sum_k in[z][m][k] (lg[m][k]) tw[(k j) mod 256], blockIdx.z = z.
template <bool FILT, bool INV>
__global__ __launch_bounds__(DT * DT) void k_vsi_dft_cols(const cpx *__restrict__ in, const double *__restrict__ lg,
                                                          const cpx *__restrict__ tw, cpx *__restrict__ out)
{
    __shared__ cpx sA[DT][DT], sB[DT][DT + 1];
    const int tx = threadIdx.x & (DT - 1), ty = threadIdx.x / DT;
    const int m = (int)blockIdx.y * DT + ty, j = (int)blockIdx.x * DT + tx;     // the grid covers 256 x 256 exactly
    in += (size_t)blockIdx.z * VSI_NN;
    out += (size_t)blockIdx.z * VSI_NN;
    cpx acc = make_double2(0.0, 0.0);
    for (int k0 = 0; k0 < VSI_N; k0 += DT) {
        const int ka = k0 + tx, kb = k0 + ty;
        const size_t idx = (size_t)m * VSI_N + ka;
        cpx va = in[idx];
        if (FILT) {
            const double f = lg[idx];
            va.x *= f;
            va.y *= f;
        }
        cpx vb = tw[(kb * j) & NMASK];
        if (INV) vb.y = -vb.y;
        sA[ty][tx] = va;
        sB[ty][tx] = vb;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < DT; ++kk) {
            const cpx x = sA[ty][kk], y = sB[kk][tx];
            acc.x += fma(-x.y, y.y, x.x * y.x);
            acc.y += fma(x.x, y.y, x.y * y.x);
        }
        __syncthreads();
    }
    out[(size_t)m * VSI_N + j] = acc;
}

// Down the rows of a column: out[z][i][c] = scale sum_k tw[(i k) mod 256] in[z][k][c], blockIdx.z = z.
template <bool INV>
__global__ __launch_bounds__(DT * DT) void k_vsi_dft_rows(const cpx *__restrict__ in, const cpx *__restrict__ tw, double scale,
                                                          cpx *__restrict__ out)
{
    __shared__ cpx sA[DT][DT], sB[DT][DT + 1];
    const int tx = threadIdx.x & (DT - 1), ty = threadIdx.x / DT;
    const int i = (int)blockIdx.y * DT + ty, c = (int)blockIdx.x * DT + tx;
    in += (size_t)blockIdx.z * VSI_NN;
    out += (size_t)blockIdx.z * VSI_NN;
    cpx acc = make_double2(0.0, 0.0);
    for (int k0 = 0; k0 < VSI_N; k0 += DT) {
        const int ka = k0 + tx, kb = k0 + ty;
        cpx va = tw[(i * ka) & NMASK];
        if (INV) va.y = -va.y;
        sA[ty][tx] = va;
        sB[ty][tx] = in[(size_t)kb * VSI_N + c];
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < DT; ++kk) {
            const cpx x = sA[ty][kk], y = sB[kk][tx];
            acc.x += fma(-x.y, y.y, x.x * y.x);
            acc.y += fma(x.x, y.y, x.y * y.x);
        }
        __syncthreads();
    }
    out[(size_t)i * VSI_N + c] = make_double2(acc.x * scale, acc.y * scale);
}

__global__ __launch_bounds__(VSI_THREADS) void k_vsi_sal(const cpx *__restrict__ resp, const double *__restrict__ lab,
                                                         const double *__restrict__ sd, const double *__restrict__ range,
                                                         double *__restrict__ vs)
{
    const size_t i = (size_t)blockIdx.x * VSI_THREADS + threadIdx.x;
    double sf2 = 0.0;
#pragma unroll
    for (int z = 0; z < 3; ++z) {
        const double v = resp[(size_t)z * VSI_NN + i].x;
        sf2 += v * v;
    }
    vs[i] = vsi_saliency(sf2, sd[i], lab[VSI_NN + i], lab[2 * (size_t)VSI_NN + i], range);
}

// ---- the full-resolution map --------------------------------------------------------------------------------------------------------
// tmp[m][x] = sum_k wt[x][k] vs[m][idx[x][k]]; grid (ceil(w / 256), 256)
__global__ __launch_bounds__(VSI_THREADS) void k_vsi_up_cols(const double *__restrict__ vs, const double *__restrict__ wt,
                                                             const int *__restrict__ idx, int taps, int w, double *__restrict__ tmp)
{
    const long long x = (long long)blockIdx.x * VSI_THREADS + threadIdx.x;
    if (x >= w) return;
    const size_t m = blockIdx.y;
    double acc = 0.0;
    for (int k = 0; k < taps; ++k) acc += wt[(size_t)x * taps + k] * vs[m * VSI_N + idx[(size_t)x * taps + k]];
    tmp[m * (size_t)w + (size_t)x] = acc;
}

// min / max of VS(y, x) = sum_k wt[y][k] tmp[idx[y][k]][x] over a block's 256 columns x VSI_EXPAND_ROWS rows
__global__ __launch_bounds__(VSI_THREADS) void k_vsi_expand(const double *__restrict__ tmp, const double *__restrict__ wt,
                                                            const int *__restrict__ idx, int taps, int h, int w,
                                                            double *__restrict__ mpart)
{
    __shared__ double sh[2][VSI_THREADS];
    const int t = threadIdx.x;
    const long long x = (long long)blockIdx.x * VSI_THREADS + t;
    const int y0 = (int)blockIdx.y * VSI_EXPAND_ROWS, y1 = y0 + VSI_EXPAND_ROWS < h ? y0 + VSI_EXPAND_ROWS : h;
    double mn = INFINITY, mx = -INFINITY;
    if (x < w) {
        for (int y = y0; y < y1; ++y) {
            double acc = 0.0;
            for (int k = 0; k < taps; ++k) acc += wt[(size_t)y * taps + k] * tmp[(size_t)idx[(size_t)y * taps + k] * (size_t)w + (size_t)x];
            mn = vsi_min(mn, acc);
            mx = vsi_max(mx, acc);
        }
    }
    sh[0][t] = mn;
    sh[1][t] = mx;
    __syncthreads();
    for (int s = VSI_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            sh[0][t] = vsi_min(sh[0][t], sh[0][t + s]);
            sh[1][t] = vsi_max(sh[1][t], sh[1][t + s]);
        }
        __syncthreads();
    }
    if (t < 2) mpart[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 + t] = sh[t][0];
}

// One block: the tree over the per-block min / max -> out[0], out[1]
__global__ __launch_bounds__(VSI_THREADS) void k_vsi_minmax(const double *__restrict__ mpart, size_t blocks, double *__restrict__ out)
{
    __shared__ double sh[2][VSI_THREADS];
    const int t = threadIdx.x;
    double mn = INFINITY, mx = -INFINITY;
    for (size_t q = t; q < blocks; q += VSI_THREADS) {
        mn = vsi_min(mn, mpart[q * 2]);
        mx = vsi_max(mx, mpart[q * 2 + 1]);
    }
    sh[0][t] = mn;
    sh[1][t] = mx;
    __syncthreads();
    for (int s = VSI_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            sh[0][t] = vsi_min(sh[0][t], sh[0][t + s]);
            sh[1][t] = vsi_max(sh[1][t], sh[1][t + s]);
        }
        __syncthreads();
    }
    if (t < 2) out[t] = sh[t][0];
}

// tp[m][j] = sum_b cw[j][b] vs[m][lo[j] + b]; grid (ceil(cols / 256), 256).  Past index 255 the weight is 0.
__global__ __launch_bounds__(VSI_THREADS) void k_vsi_band_cols(const double *__restrict__ vs, const double *__restrict__ cw,
                                                               const int *__restrict__ lo, int band, int cols, double *__restrict__ tp)
{
    const long long j = (long long)blockIdx.x * VSI_THREADS + threadIdx.x;
    if (j >= cols) return;
    const size_t m = blockIdx.y;
    const int l = lo[j];
    double acc = 0.0;
    for (int b = 0; b < band; ++b) {
        const int q = l + b < VSI_N ? l + b : VSI_N - 1;
        acc += cw[(size_t)j * band + b] * vs[m * VSI_N + q];
    }
    tp[m * (size_t)cols + (size_t)j] = acc;
}

// pvs[i][j] = sum_b cw[i][b] tp[lo[i] + b][j]; grid (ceil(cols / 256), rows)
__global__ __launch_bounds__(VSI_THREADS) void k_vsi_band_rows(const double *__restrict__ tp, const double *__restrict__ cw,
                                                               const int *__restrict__ lo, int band, int cols, double *__restrict__ pvs)
{
    const long long j = (long long)blockIdx.x * VSI_THREADS + threadIdx.x;
    if (j >= cols) return;
    const size_t i = blockIdx.y;
    const int l = lo[i];
    double acc = 0.0;
    for (int b = 0; b < band; ++b) {
        const int q = l + b < VSI_N ? l + b : VSI_N - 1;
        acc += cw[i * band + b] * tp[(size_t)q * (size_t)cols + (size_t)j];
    }
    pvs[i * (size_t)cols + (size_t)j] = acc;
}

// ---- pooling (FSIM's pass, VSI's planes) ----------------------------------------------------------------------------------------
template <int CN>
__global__ __launch_bounds__(VSI_THREADS) void k_vsi_pool(const unsigned char *__restrict__ a, long long sa,
                                                          const unsigned char *__restrict__ b, long long sb, int h, int w, int F,
                                                          int cols, size_t n, long long *__restrict__ out)
{
    __shared__ int col[6][VSI_THREADS];
    const int t = threadIdx.x;
    const int nout = VSI_THREADS / F;
    const int j0 = (int)blockIdx.x * nout, i = (int)blockIdx.y;
    const long long x = fsim_win_start(j0, F) + t, ys = fsim_win_start(i, F);
    int acc[6] = {0, 0, 0, 0, 0, 0};
    if (t < nout * F && x >= 0 && x < w) {
        const long long y0 = ys < 0 ? 0 : ys, y1 = ys + F < h ? ys + F : h;
        for (long long y = y0; y < y1; ++y) {
            const unsigned char *pa = a + (size_t)y * (size_t)sa + (size_t)x * CN;
            const unsigned char *pb = b + (size_t)y * (size_t)sb + (size_t)x * CN;
            const int r1 = pa[0], g1 = pa[1], b1 = pa[2], r2 = pb[0], g2 = pb[1], b2 = pb[2];
            acc[0] += 6 * r1 + 63 * g1 + 27 * b1;
            acc[1] += 30 * r1 + 4 * g1 - 35 * b1;
            acc[2] += 34 * r1 - 60 * g1 + 17 * b1;
            acc[3] += 6 * r2 + 63 * g2 + 27 * b2;
            acc[4] += 30 * r2 + 4 * g2 - 35 * b2;
            acc[5] += 34 * r2 - 60 * g2 + 17 * b2;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) col[k][t] = acc[k];
    __syncthreads();
    for (int q = t; q < nout * 6; q += VSI_THREADS) {
        const int comp = q / nout, jo = q - comp * nout, j = j0 + jo;
        if (j >= cols) continue;
        long long s = 0;
        for (int k = 0; k < F; ++k) s += col[comp][jo * F + k];
        out[(size_t)comp * n + (size_t)i * (size_t)cols + (size_t)j] = s;
    }
}

// ---- the score -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double vs_at(const long long *__restrict__ y, int r, int c, int rows, int cols)
{
    return (r >= 0 && r < rows && c >= 0 && c < cols) ? (double)y[(size_t)r * (size_t)cols + (size_t)c] : 0.0;
}

// G of conv2(L, dx, 'same'), conv2(L, dy, 'same'): the sums are exact integers (< 2^53), unit16 = 16 * 100 F^2
__device__ __forceinline__ double vs_grad(const long long *__restrict__ y, int r, int c, int rows, int cols, double unit16)
{
    const double a = vs_at(y, r - 1, c - 1, rows, cols), b = vs_at(y, r - 1, c, rows, cols), d = vs_at(y, r - 1, c + 1, rows, cols);
    const double e = vs_at(y, r, c - 1, rows, cols), g = vs_at(y, r, c + 1, rows, cols);
    const double p = vs_at(y, r + 1, c - 1, rows, cols), q = vs_at(y, r + 1, c, rows, cols), s = vs_at(y, r + 1, c + 1, rows, cols);
    const double ix = (3.0 * (s - p) + 10.0 * (g - e) + 3.0 * (d - a)) / unit16;
    const double iy = (3.0 * (s - d) + 10.0 * (q - b) + 3.0 * (p - a)) / unit16;
    return sqrt(ix * ix + iy * iy);
}

__global__ __launch_bounds__(VSI_THREADS) void k_vsi_score(const long long *__restrict__ pool, const double *__restrict__ pvs,
                                                           const int *__restrict__ cover_y, const int *__restrict__ cover_x,
                                                           const double *__restrict__ range, int rows, int cols, size_t n, double ff,
                                                           double *__restrict__ part)
{
    __shared__ double R[2][VSI_THREADS];
    const int t = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * VSI_THREADS + t;
    double v0 = 0.0, v1 = 0.0;
    if (i < n) {
        const int r = (int)(i / (size_t)cols), c = (int)(i - (size_t)r * (size_t)cols);
        const double unit = 100.0 * ff;
        const double mm[4] = {range[4], range[5], range[8 + 4], range[8 + 5]};
        const double g1 = vs_grad(pool, r, c, rows, cols, 16.0 * unit), g2 = vs_grad(pool + 3 * n, r, c, rows, cols, 16.0 * unit);
        vsi_sample(g1, g2, (double)pool[n + i] / unit, (double)pool[4 * n + i] / unit, (double)pool[2 * n + i] / unit,
                   (double)pool[5 * n + i] / unit, pvs[i], pvs[n + i], (double)cover_y[r] * (double)cover_x[c], mm, ff, &v0, &v1);
    }
    R[0][t] = v0;
    R[1][t] = v1;
    __syncthreads();
    for (int s = VSI_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            R[0][t] += R[0][t + s];
            R[1][t] += R[1][t + s];
        }
        __syncthreads();
    }
    if (t < 2) part[(size_t)blockIdx.x * 2 + t] = R[t][0];
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// The workspace of the plan with LG, SD, the twiddles and the tables of its image size in place (built and uploaded when the
// size or the buffer changed).
int vsi_workspace(sr_ctx *ctx, const char *who, const VsiPlan &p, const VsiTables &t, char **ws_out)
{
    bool regrown = false;
    SRCHK(ctx->vsi_ws.reserve(ctx, who, p.total, 0, 1, &regrown));
    char *ws = ctx->vsi_ws.as<char>();
    *ws_out = ws;
    if (!regrown && ctx->vsi_h == p.h && ctx->vsi_w == p.w) return SR_OK;
    ctx->vsi_h = ctx->vsi_w = 0;
    std::vector<double> lg(VSI_NN), sd(VSI_NN), tw(2 * VSI_N);
    vsi_filter(lg.data(), sd.data());
    fsim_twiddles(VSI_N, tw.data());
    HIPCHK(hipMemcpyAsync(ws + p.off_lg, lg.data(), lg.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ws + p.off_sd, sd.data(), sd.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ws + p.off_tw, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const ImrAxis *ax[4] = {&t.sy, &t.sx, &t.uy, &t.ux};
    for (int k = 0; k < 4; ++k) {
        HIPCHK(hipMemcpyAsync(ws + p.off_w[k], ax[k]->w.data(), ax[k]->w.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ws + p.off_idx[k], ax[k]->idx.data(), ax[k]->idx.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                              ctx->stream));
    }
    const VsiBand *bd[2] = {&t.cy, &t.cx};
    for (int k = 0; k < 2; ++k) {
        HIPCHK(hipMemcpyAsync(ws + p.off_w[4 + k], bd[k]->w.data(), bd[k]->w.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ws + p.off_idx[4 + k], bd[k]->lo.data(), bd[k]->lo.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                              ctx->stream));
        HIPCHK(hipMemcpyAsync(ws + p.off_cover[k], bd[k]->cover.data(), bd[k]->cover.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                              ctx->stream));
    }
    HIPCHK(stream_sync(ctx));       // the host tables go out of scope
    ctx->vsi_h = p.h;
    ctx->vsi_w = p.w;
    return SR_OK;
}

template <int CN>
void launch_shrink(sr_ctx *ctx, const VsiPlan &p, const VsiTables &t, char *ws, const unsigned char *img, long long stride)
{
    const double *wy = (const double *)(ws + p.off_w[0]), *wx = (const double *)(ws + p.off_w[1]);
    const int *iy = (const int *)(ws + p.off_idx[0]), *ix = (const int *)(ws + p.off_idx[1]);
    double *tmp = (double *)(ws + p.off_tmp), *rgb = (double *)(ws + p.off_rgb);
    const dim3 thr(VSI_THREADS);
    if (p.order == 0) {
        const dim3 g1((unsigned)((3LL * p.w + VSI_THREADS - 1) / VSI_THREADS), VSI_N), g2(VSI_N, VSI_N / (VSI_THREADS / 64));
        hipLaunchKernelGGL((k_vsi_resize_v<unsigned char, CN, false>), g1, thr, 0, ctx->stream, img, stride, p.w, wy, iy, t.sy.taps, tmp);
        hipLaunchKernelGGL((k_vsi_resize_h<double, 3, true>), g2, thr, 0, ctx->stream, (const double *)tmp,
                           (long long)p.w * 3 * (long long)sizeof(double), wx, ix, t.sx.taps, rgb);
    } else {
        const dim3 g1((unsigned)p.h, VSI_N / (VSI_THREADS / 64)), g2((3 * VSI_N + VSI_THREADS - 1) / VSI_THREADS, VSI_N);
        hipLaunchKernelGGL((k_vsi_resize_h<unsigned char, CN, false>), g1, thr, 0, ctx->stream, img, stride, wx, ix, t.sx.taps, tmp);
        hipLaunchKernelGGL((k_vsi_resize_v<double, 3, true>), g2, thr, 0, ctx->stream, (const double *)tmp,
                           (long long)VSI_N * 3 * (long long)sizeof(double), VSI_N, wy, iy, t.sy.taps, rgb);
    }
}

// VS256, Lab and the a / b range (slot img of off_range) of one image
int vsi_sdsp(sr_ctx *ctx, const VsiPlan &p, const VsiTables &t, char *ws, const unsigned char *d_img, long long stride, int img)
{
    double *rgb = (double *)(ws + p.off_rgb), *lab = (double *)(ws + p.off_lab), *vs = (double *)(ws + p.off_vs256);
    double *range = (double *)(ws + p.off_range) + (size_t)img * 8, *rpart = (double *)(ws + p.off_rpart);
    const double *lg = (const double *)(ws + p.off_lg), *sd = (const double *)(ws + p.off_sd);
    const cpx *tw = (const cpx *)(ws + p.off_tw);
    cpx *c0 = (cpx *)(ws + p.off_c0), *c1 = (cpx *)(ws + p.off_c1);
    const dim3 thr(VSI_THREADS), flat(VSI_NN / VSI_THREADS), tile(DT * DT), grid3(VSI_N / DT, VSI_N / DT, 3);
    {
        ProfScope ps(ctx, "vsi_shrink");
        if (p.cn == 3) launch_shrink<3>(ctx, p, t, ws, d_img, stride);
        else launch_shrink<4>(ctx, p, t, ws, d_img, stride);
    }
    SRCHK(check_launch("vsi_shrink"));
    {
        ProfScope ps(ctx, "vsi_sdsp");
        hipLaunchKernelGGL(k_vsi_lab, flat, thr, 0, ctx->stream, (const double *)rgb, lab, rpart);
        hipLaunchKernelGGL(k_vsi_range, dim3(1), thr, 0, ctx->stream, (const double *)rpart, range);
        hipLaunchKernelGGL(k_vsi_centre, dim3(VSI_NN / VSI_THREADS, 3), thr, 0, ctx->stream, (const double *)lab, c0);
        hipLaunchKernelGGL((k_vsi_dft_cols<false, false>), grid3, tile, 0, ctx->stream, (const cpx *)c0, lg, tw, c1);
        hipLaunchKernelGGL((k_vsi_dft_rows<false>), grid3, tile, 0, ctx->stream, (const cpx *)c1, tw, 1.0, c0);
        hipLaunchKernelGGL((k_vsi_dft_cols<true, true>), grid3, tile, 0, ctx->stream, (const cpx *)c0, lg, tw, c1);
        hipLaunchKernelGGL((k_vsi_dft_rows<true>), grid3, tile, 0, ctx->stream, (const cpx *)c1, tw, 1.0 / (double)VSI_NN, c0);
        hipLaunchKernelGGL(k_vsi_sal, flat, thr, 0, ctx->stream, (const cpx *)c0, (const double *)lab, sd, (const double *)range, vs);
    }
    return check_launch("vsi_sdsp");
}

// min / max of the full-resolution map (slot img of off_range, entries 4 and 5) and its raw window sums (slot img of off_pvs)
int vsi_expand(sr_ctx *ctx, const VsiPlan &p, const VsiTables &t, char *ws, int img)
{
    const double *vs = (const double *)(ws + p.off_vs256);
    double *tmp = (double *)(ws + p.off_tmp), *mpart = (double *)(ws + p.off_mpart);
    double *range = (double *)(ws + p.off_range) + (size_t)img * 8, *pvs = (double *)(ws + p.off_pvs) + (size_t)img * p.n;
    const dim3 thr(VSI_THREADS);
    const unsigned gx = (unsigned)p.expand_gx, gy = (unsigned)p.expand_gy, gc = (unsigned)((p.cols + VSI_THREADS - 1) / VSI_THREADS);
    {
        ProfScope ps(ctx, "vsi_expand");
        hipLaunchKernelGGL(k_vsi_up_cols, dim3(gx, VSI_N), thr, 0, ctx->stream, vs, (const double *)(ws + p.off_w[3]),
                           (const int *)(ws + p.off_idx[3]), t.ux.taps, p.w, tmp);
        hipLaunchKernelGGL(k_vsi_expand, dim3(gx, gy), thr, 0, ctx->stream, (const double *)tmp, (const double *)(ws + p.off_w[2]),
                           (const int *)(ws + p.off_idx[2]), t.uy.taps, p.h, p.w, mpart);
        hipLaunchKernelGGL(k_vsi_minmax, dim3(1), thr, 0, ctx->stream, (const double *)mpart, (size_t)gx * gy, range + 4);
        hipLaunchKernelGGL(k_vsi_band_cols, dim3(gc, VSI_N), thr, 0, ctx->stream, vs, (const double *)(ws + p.off_w[5]),
                           (const int *)(ws + p.off_idx[5]), t.cx.band, p.cols, tmp);
        hipLaunchKernelGGL(k_vsi_band_rows, dim3(gc, (unsigned)p.rows), thr, 0, ctx->stream, (const double *)tmp,
                           (const double *)(ws + p.off_w[4]), (const int *)(ws + p.off_idx[4]), t.cy.band, p.cols, pvs);
    }
    return check_launch("vsi_expand");
}

template <typename... Args>
void launch_pool(int cn, dim3 grid, hipStream_t stream, Args... args)
{
    if (cn == 3) hipLaunchKernelGGL((k_vsi_pool<3>), grid, dim3(VSI_THREADS), 0, stream, args...);
    else hipLaunchKernelGGL((k_vsi_pool<4>), grid, dim3(VSI_THREADS), 0, stream, args...);
}

int stride_args(const char *who, int64_t stride_a, int64_t stride_b, int w, int cn)
{
    const int64_t min_stride = (int64_t)w * cn;
    if (stride_a < min_stride || stride_b < min_stride) return sr_set_error(SR_ERR_SHAPE, "%s: stride smaller than a row", who);
    return SR_OK;
}

}  // namespace

extern "C" {

int sr_vsi_pool_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w, int cn,
                   int F, int64_t *h_out)
{
    // every argument check comes before the context (and so the device) is touched
    if (!d_a || !d_b || !h_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_vsi_pool_u8: null argument");
    if (F == 0) return sr_set_error(SR_ERR_INVALID_ARG, "sr_vsi_pool_u8: F must be 1 .. %d (got 0)", VSI_MAX_F);
    VsiPlan p;
    SRCHK(vsi_plan("sr_vsi_pool_u8", h, w, cn, F, &p, nullptr));
    SRCHK(stride_args("sr_vsi_pool_u8", stride_a, stride_b, w, cn));
    CTX_ENTER(ctx);
    DevTemp sums(ctx);
    const size_t bytes = 6 * p.n * sizeof(long long);
    SRCHK(sums.alloc("sr_vsi_pool_u8", bytes));
    launch_pool(cn, dim3((unsigned)p.pool_gx, (unsigned)p.rows), ctx->stream, (const unsigned char *)d_a, (long long)stride_a,
                (const unsigned char *)d_b, (long long)stride_b, h, w, p.F, p.cols, p.n, sums.as<long long>());
    SRCHK(check_launch("vsi_pool"));
    HIPCHK(hipMemcpyAsync(h_out, sums.d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_vsi_saliency_u8(sr_ctx *ctx, const uint8_t *d_img, int64_t stride, int h, int w, int cn, double *h_lab, double *h_vs256,
                       double *h_range)
{
    if (!d_img) return sr_set_error(SR_ERR_INVALID_ARG, "sr_vsi_saliency_u8: null argument");
    VsiPlan p;
    VsiTables t;
    SRCHK(vsi_plan("sr_vsi_saliency_u8", h, w, cn, 0, &p, &t));
    SRCHK(stride_args("sr_vsi_saliency_u8", stride, stride, w, cn));
    CTX_ENTER(ctx);
    char *ws = nullptr;
    SRCHK(vsi_workspace(ctx, "sr_vsi_saliency_u8", p, t, &ws));
    SRCHK(vsi_sdsp(ctx, p, t, ws, (const unsigned char *)d_img, (long long)stride, 0));
    if (h_lab) HIPCHK(hipMemcpyAsync(h_lab, ws + p.off_lab, 3 * (size_t)VSI_NN * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (h_vs256) HIPCHK(hipMemcpyAsync(h_vs256, ws + p.off_vs256, (size_t)VSI_NN * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (h_range) HIPCHK(hipMemcpyAsync(h_range, ws + p.off_range, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_vsi_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w, int cn,
              sr_vsi_sums *h_out)
{
    if (!d_a || !d_b || !h_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_vsi_u8: null argument");
    VsiPlan p;
    VsiTables t;
    SRCHK(vsi_plan("sr_vsi_u8", h, w, cn, 0, &p, &t));
    SRCHK(stride_args("sr_vsi_u8", stride_a, stride_b, w, cn));
    CTX_ENTER(ctx);
    char *ws = nullptr;
    SRCHK(vsi_workspace(ctx, "sr_vsi_u8", p, t, &ws));
    long long *pool = (long long *)(ws + p.off_pool);
    double *part = (double *)(ws + p.off_part), *buf0 = (double *)(ws + p.off_buf0), *buf1 = (double *)(ws + p.off_buf1);
    const unsigned char *img[2] = {(const unsigned char *)d_a, (const unsigned char *)d_b};
    const long long st[2] = {(long long)stride_a, (long long)stride_b};
    for (int k = 0; k < 2; ++k) {
        SRCHK(vsi_sdsp(ctx, p, t, ws, img[k], st[k], k));
        SRCHK(vsi_expand(ctx, p, t, ws, k));
    }
    {
        ProfScope ps(ctx, "vsi_pool");
        launch_pool(cn, dim3((unsigned)p.pool_gx, (unsigned)p.rows), ctx->stream, img[0], st[0], img[1], st[1], h, w, p.F, p.cols, p.n,
                    pool);
    }
    SRCHK(check_launch("vsi_pool"));
    double h_res[2], h_range[16];
    {
        ProfScope ps(ctx, "vsi_score");
        hipLaunchKernelGGL(k_vsi_score, dim3((unsigned)p.score_blocks), dim3(VSI_THREADS), 0, ctx->stream, (const long long *)pool,
                           (const double *)(ws + p.off_pvs), (const int *)(ws + p.off_cover[0]), (const int *)(ws + p.off_cover[1]),
                           (const double *)(ws + p.off_range), p.rows, p.cols, p.n, (double)p.F * (double)p.F, part);
        const double *sums = reduce_partials(ctx, part, (long long)p.score_blocks, 2, buf0, buf1);
        SRCHK(check_launch("vsi_score"));
        HIPCHK(hipMemcpyAsync(h_res, sums, sizeof(h_res), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipMemcpyAsync(h_range, ws + p.off_range, sizeof(h_range), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    memset(h_out, 0, sizeof(*h_out));
    h_out->sum_s = h_res[0];
    h_out->sum_w = h_res[1];
    h_out->count = (uint64_t)p.n;
    h_out->F = p.F;
    h_out->rows = p.rows;
    h_out->cols = p.cols;
    for (int k = 0; k < 2; ++k)
        for (int q = 0; q < 2; ++q) {
            h_out->a_range[k][q] = h_range[k * 8 + q];
            h_out->b_range[k][q] = h_range[k * 8 + 2 + q];
            h_out->vs_range[k][q] = h_range[k * 8 + 4 + q];
        }
    return SR_OK;
}

}  // extern "C"
