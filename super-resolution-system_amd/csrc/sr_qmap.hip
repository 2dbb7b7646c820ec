// sr_qmap.hip -- per-cell PSNR / SSIM quality maps (sr_quality_map_u8, sr_quality_map_counts).
//
// The squared error and the three SSIM maps of sr_assess_u8 (uniform-7 with the sample covariance, gauss-11 cropped by 5,
// "simple" = the same Gaussian over the full frame with REFLECT_101 and the constants of 255), binned into the cells of a
// separable grid.  A cell is a bin for results, not a crop of the input: the filters read across cell boundaries, so the
// sum over the cells is the global sum sr_assess_u8 returns (up to the order of fp64 additions) and the squared error adds
// up exactly.
//
// Two kernels, no floating-point atomics -- equal inputs give equal bits:
//   k_qmap_cols   a block owns S11_OUT columns and ONE row chunk (a cell row, or a piece of at most S11_ROWS rows of it).  The
//                 Gaussian half is the column march of sr_ssim11.h with the packed u8 window.  This file's own: the columns
//                 are image columns - 5 .. + 250 with REFLECT_101 (the full-frame variant needs the border), so the
//                 horizontal pass is centred on the thread's own column; the uniform-7 variant takes its 7-row box sums
//                 from the same window and its horizontal pass from the integer rows U; the chunk table.  Samples are
//                 added per column in row order; at the end the thread stores its column sums into the slab
//                 ws[sum][chunk][column].
//   k_qmap_cells  a block per cell adds the slab entries of the cell's chunks and columns in a fixed order.
// fp64 throughout, like the rest of the assessment.  A plain separable form: k_assess_march (sr_assess.hip) stays the
// tuned kernel of the global metrics.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_ctx.h"
#include "sr_ssim11.h"

namespace {

enum { QM_SSE = 1, QM_UNIFORM = 2, QM_GAUSS = 4, QM_SIMPLE = 8, QM_ALL_BITS = 15 };

struct QmapParams {
    int h, w, shift, flags, same_c;
    int p_sse, p_u, p_g, p_s;   // slab plane of each selected sum
    long long plane;            // 8-byte words per plane: chunks * w
    double c1a, c2a;            // constants for data_range (uniform / gauss)
    double c1b, c2b;            // constants for 255 (simple)
    double k1u, k2u;            // 49^2 c1a and 48 * 49 c2a: the uniform-7 variant in integer-scaled form
    double k[6];                // k[0] centre tap, k[j] the +-j taps
};

struct QmapRecord {
    unsigned long long sse;
    double ssim_uniform, ssim_gauss, ssim_simple;
};

__device__ __forceinline__ int qm_reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

template <int CN>
__device__ __forceinline__ void qm_load(const unsigned char *__restrict__ pa, const unsigned char *__restrict__ pb, int shift,
                                        unsigned &xy, unsigned &q, unsigned &p, unsigned &sq)
{
    int ga, gb;
    gray_pair<CN>(pa, pb, shift, ga, gb, sq);
    // x and y travel packed: pair sums (<= 510), 7-row sums (<= 1785) and 49-sample sums (<= 12495 < 2^14) stay in their fields
    xy = (unsigned)ga | ((unsigned)gb << 14);
    q = (unsigned)(ga * gb);
    p = (unsigned)(ga * ga + gb * gb);
}

template <int CN>
__global__ __launch_bounds__(S11_TX) void k_qmap_cols(const unsigned char *__restrict__ a, long long sa,
                                                      const unsigned char *__restrict__ b, long long sb, QmapParams P,
                                                      const int2 *__restrict__ chunks, unsigned long long *__restrict__ ws)
{
    __shared__ double F[2][4][S11_TX];
    __shared__ unsigned U[2][3][S11_TX];
    const int t = threadIdx.x;
    const int2 ck = chunks[blockIdx.x];
    const int y0 = ck.x, y1 = ck.y;
    const int mx = (int)blockIdx.y * S11_OUT - S11_R + t;                // the column this thread filters vertically
    const bool own = t >= S11_R && t < S11_TX - S11_R && mx < P.w;       // ... and produces (mx >= 0 there)
    const bool want_g = (P.flags & (QM_GAUSS | QM_SIMPLE)) != 0, want_u = (P.flags & QM_UNIFORM) != 0;
    const size_t col = (size_t)qm_reflect101(mx, P.w) * CN;
    const unsigned char *ca = a + col, *cb = b + col;
    Window11<unsigned> wxy, wq, wp;                                     // rows oy - 5 .. oy + 5 of this column
    unsigned wsq[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) wsq[i] = 0u;
    double sum_u = 0.0, sum_g = 0.0, sum_s = 0.0;
    unsigned sse = 0;                   // at most S11_ROWS * 3 * 255^2 = 2.5e7 per thread
    const double k0 = P.k[0], k1 = P.k[1], k2 = P.k[2], k3 = P.k[3], k4 = P.k[4], k5 = P.k[5];
    const int nrows = (y1 - y0) + 2 * S11_R;
    unsigned nxy, nq, np, nsq;
    {
        const size_t sy = (size_t)qm_reflect101(y0 - S11_R, P.h);
        qm_load<CN>(ca + sy * (size_t)sa, cb + sy * (size_t)sb, P.shift, nxy, nq, np, nsq);
    }
#pragma unroll 1
    for (int lr = 0; lr < nrows; ++lr) {
        wxy.push(nxy);
        wq.push(nq);
        wp.push(np);
#pragma unroll
        for (int i = 0; i < 5; ++i) wsq[i] = wsq[i + 1];
        wsq[5] = nsq;
        {   // the next row is requested before this one is worked on (the last iteration reads its own row again)
            const size_t sy = (size_t)qm_reflect101(y0 - S11_R + min(lr + 1, nrows - 1), P.h);
            qm_load<CN>(ca + sy * (size_t)sa, cb + sy * (size_t)sb, P.shift, nxy, nq, np, nsq);
        }
        if (lr < 2 * S11_R) continue;                                   // block-uniform
        const int oy = y0 + lr - 2 * S11_R;                             // the window's centre row, inside the chunk
        const int pb = lr & 1;
        if (want_g) {
            const double kk[6] = {k0, k1, k2, k3, k4, k5};
            double hv[4];
            s11_col_pass_packed(wxy, wp, wq, kk, hv);
            s11_store_col(F[pb], t, hv);
        }
        if (want_u) {
            unsigned uxy = wxy[2], up = wp[2], uq = wq[2];
#pragma unroll
            for (int i = 3; i <= 8; ++i) { uxy += wxy[i]; up += wp[i]; uq += wq[i]; }
            U[pb][0][t] = uxy; U[pb][1][t] = up; U[pb][2][t] = uq;
        }
        __syncthreads();
        if (!own) continue;
        sse += wsq[0];
        if (want_g) {
            const double kk[6] = {k0, k1, k2, k3, k4, k5};
            double u[4];
            s11_row_pass(F[pb], t, kk, u);
            const bool inner_row = oy >= S11_R && oy < P.h - S11_R;     // block-uniform
            if (P.same_c) {
                const double sv = ssim_quot(u[0], u[1], u[2], u[3], P.c1a, P.c2a);
                sum_s += sv;
                if (inner_row) sum_g += sv;
            } else {
                if (P.flags & QM_SIMPLE) sum_s += ssim_quot(u[0], u[1], u[2], u[3], P.c1b, P.c2b);
                if (inner_row && (P.flags & QM_GAUSS)) sum_g += ssim_quot(u[0], u[1], u[2], u[3], P.c1a, P.c2a);
            }
        }
        if (want_u && oy >= 3 && oy < P.h - 3) {                        // block-uniform
            unsigned t_xy = U[pb][0][t], t_p = U[pb][1][t], t_q = U[pb][2][t];
#pragma unroll
            for (int j = 1; j <= 3; ++j) {
                t_xy += U[pb][0][t - j] + U[pb][0][t + j];
                t_p += U[pb][1][t - j] + U[pb][1][t + j];
                t_q += U[pb][2][t - j] + U[pb][2][t + j];
            }
            // SSIM of the 49-sample window with both fractions scaled to integers (sample covariance, N - 1 = 48):
            //   (2 Sx Sy + 49^2 C1) / (Sx^2 + Sy^2 + 49^2 C1)
            //   (2 (49 Sxy - Sx Sy) + 48*49 C2) / (49 (Sxx + Syy) - (Sx^2 + Sy^2) + 48*49 C2)
            // everything left of the constants is exact 32-bit integer arithmetic (|values| < 3.2e8)
            const int sx = (int)(t_xy & 0x3FFFu), sy = (int)(t_xy >> 14);
            const int sxsy = sx * sy, ss = sx * sx + sy * sy;
            const int ncov = 49 * (int)t_q - sxsy, nvar = 49 * (int)t_p - ss;
            const double a1 = fma(2.0, (double)sxsy, P.k1u), a2 = fma(2.0, (double)ncov, P.k2u);
            const double b1 = (double)ss + P.k1u, b2 = (double)nvar + P.k2u;
            sum_u += (a1 * a2) * ssim_recip(b1 * b2);
        }
    }
    if (!own) return;
    // column validity, once: the full-frame variant counts every image column, the cropped ones lose 5 / 3 per side
    if (!(mx >= S11_R && mx < P.w - S11_R)) sum_g = 0.0;
    if (!(mx >= 3 && mx < P.w - 3)) sum_u = 0.0;
    const size_t at = (size_t)blockIdx.x * (size_t)P.w + (size_t)mx;
    if (P.flags & QM_SSE) ws[(size_t)P.p_sse * (size_t)P.plane + at] = (unsigned long long)sse;
    if (P.flags & QM_UNIFORM) ws[(size_t)P.p_u * (size_t)P.plane + at] = (unsigned long long)__double_as_longlong(sum_u);
    if (P.flags & QM_GAUSS) ws[(size_t)P.p_g * (size_t)P.plane + at] = (unsigned long long)__double_as_longlong(sum_g);
    if (P.flags & QM_SIMPLE) ws[(size_t)P.p_s * (size_t)P.plane + at] = (unsigned long long)__double_as_longlong(sum_s);
}

// One block per cell: thread t adds the slab entries (chunk, column) of the cell with column = x0 + t, x0 + t + 256, ... in
// (chunk, column) order, the 256 thread sums go through a fixed tree.
__global__ __launch_bounds__(256) void k_qmap_cells(const unsigned long long *__restrict__ ws, QmapParams P,
                                                    const int *__restrict__ xe, int gw, const int *__restrict__ cstart,
                                                    QmapRecord *__restrict__ out)
{
    __shared__ double sd[3][256];
    __shared__ unsigned long long si[256];
    const int t = threadIdx.x;
    const int gy = (int)(blockIdx.x / (unsigned)gw), gx = (int)(blockIdx.x - (unsigned)gy * (unsigned)gw);
    const int x0 = xe[gx], x1 = xe[gx + 1], c0 = cstart[gy], c1 = cstart[gy + 1];
    const int planes[3] = {P.p_u, P.p_g, P.p_s};
    const int bits[3] = {QM_UNIFORM, QM_GAUSS, QM_SIMPLE};
    unsigned long long acc_i = 0;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int c = c0; c < c1; ++c) {
        const size_t row = (size_t)c * (size_t)P.w;
        for (int x = x0 + t; x < x1; x += 256) {
            if (P.flags & QM_SSE) acc_i += ws[(size_t)P.p_sse * (size_t)P.plane + row + x];
#pragma unroll
            for (int m = 0; m < 3; ++m)
                if (P.flags & bits[m]) acc[m] += __longlong_as_double((long long)ws[(size_t)planes[m] * (size_t)P.plane + row + x]);
        }
    }
    si[t] = acc_i;
#pragma unroll
    for (int m = 0; m < 3; ++m) sd[m][t] = acc[m];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            si[t] += si[t + s];
#pragma unroll
            for (int m = 0; m < 3; ++m) sd[m][t] += sd[m][t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        QmapRecord r;
        r.sse = si[0];
        r.ssim_uniform = sd[0][0];
        r.ssim_gauss = sd[1][0];
        r.ssim_simple = sd[2][0];
        out[blockIdx.x] = r;
    }
}

int qm_check_edges(const char *scope, const char *axis, const int *e, int n, int size)
{
    if (n < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: the grid needs at least one cell along %s", scope, axis);
    if (!e) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null %s edges", scope, axis);
    if (e[0] != 0 || e[n] != size)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: %s edges must run from 0 to %d (got %d .. %d)", scope, axis, size, e[0], e[n]);
    for (int i = 0; i < n; ++i)
        if (e[i + 1] <= e[i])
            return sr_set_error(SR_ERR_INVALID_ARG, "%s: %s edges must be strictly increasing (edge %d: %d after %d)", scope, axis,
                                i + 1, e[i + 1], e[i]);
    return SR_OK;
}

}  // namespace

extern "C" {

int sr_quality_map_counts(int h, int w, int mode, const int *h_xedges, int gw, const int *h_yedges, int gh, uint64_t *counts)
{
    if (!counts || h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_quality_map_counts: bad arguments");
    int pad;
    if (mode == SR_SSIM_UNIFORM7) pad = 3;
    else if (mode == SR_SSIM_GAUSS11) pad = 5;
    else if (mode == SR_SSIM_SIMPLE) pad = 0;
    else return sr_set_error(SR_ERR_INVALID_ARG, "sr_quality_map_counts: unknown mode %d", mode);
    int rc = qm_check_edges("sr_quality_map_counts", "x", h_xedges, gw, w);
    if (rc) return rc;
    rc = qm_check_edges("sr_quality_map_counts", "y", h_yedges, gh, h);
    if (rc) return rc;
    for (int gy = 0; gy < gh; ++gy) {
        const long long ny = std::max(0, std::min(h_yedges[gy + 1], h - pad) - std::max(h_yedges[gy], pad));
        for (int gx = 0; gx < gw; ++gx) {
            const long long nx = std::max(0, std::min(h_xedges[gx + 1], w - pad) - std::max(h_xedges[gx], pad));
            counts[(size_t)gy * gw + gx] = (uint64_t)(ny * nx);
        }
    }
    return SR_OK;
}

int sr_quality_map_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                      int cn, int gray_shift, double data_range, const int *h_xedges, int gw, const int *h_yedges, int gh,
                      int flags, sr_quality_cell *h_out)
{
    static_assert(sizeof(QmapRecord) == sizeof(sr_quality_cell), "device and ABI records differ");
    // every argument check comes before the context (and so the device) is touched
    if (!d_a || !d_b || !h_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_quality_map_u8: null argument");
    if (h < 1 || w < 1 || (cn != 1 && cn != 3))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_quality_map_u8: need h,w >= 1 and 1 or 3 channels");
    if (gray_shift != 14 && gray_shift != 15) return sr_set_error(SR_ERR_INVALID_ARG, "sr_quality_map_u8: gray_shift must be 14 or 15");
    if (flags & ~QM_ALL_BITS) return sr_set_error(SR_ERR_INVALID_ARG, "sr_quality_map_u8: unknown flag bits 0x%x", flags & ~QM_ALL_BITS);
    int rc = qm_check_edges("sr_quality_map_u8", "x", h_xedges, gw, w);
    if (rc) return rc;
    rc = qm_check_edges("sr_quality_map_u8", "y", h_yedges, gh, h);
    if (rc) return rc;
    if ((int64_t)gh * gw > 0x7FFFFFFFll) return sr_set_error(SR_ERR_UNSUPPORTED, "sr_quality_map_u8: more than 2^31 - 1 cells");
    const int64_t min_stride = (int64_t)w * cn;
    if (stride_a < min_stride || stride_b < min_stride) return sr_set_error(SR_ERR_SHAPE, "sr_quality_map_u8: stride smaller than a row");
    CTX_ENTER(ctx);
    const size_t ncell = (size_t)gh * (size_t)gw;
    if (!(flags & QM_ALL_BITS)) {
        memset(h_out, 0, ncell * sizeof(sr_quality_cell));
        return SR_OK;
    }
    QmapParams P;
    memset(&P, 0, sizeof(P));
    P.h = h; P.w = w; P.shift = gray_shift; P.flags = flags;
    P.c1a = (0.01 * data_range) * (0.01 * data_range);
    P.c2a = (0.03 * data_range) * (0.03 * data_range);
    P.c1b = (0.01 * 255.0) * (0.01 * 255.0);
    P.c2b = (0.03 * 255.0) * (0.03 * 255.0);
    P.same_c = (P.c1a == P.c1b && P.c2a == P.c2b) ? 1 : 0;
    P.k1u = 2401.0 * P.c1a;
    P.k2u = 2352.0 * P.c2a;
    gauss_taps(P.k);
    int nsel = 0;
    if (flags & QM_SSE) P.p_sse = nsel++;
    if (flags & QM_UNIFORM) P.p_u = nsel++;
    if (flags & QM_GAUSS) P.p_g = nsel++;
    if (flags & QM_SIMPLE) P.p_s = nsel++;
    // row chunks: every cell row in equal pieces of at most S11_ROWS rows
    std::vector<int> chunks, cstart((size_t)gh + 1);
    for (int gy = 0; gy < gh; ++gy) {
        cstart[(size_t)gy] = (int)(chunks.size() / 2);
        const int y0 = h_yedges[gy], rows = h_yedges[gy + 1] - y0;
        const int n = (rows + S11_ROWS - 1) / S11_ROWS, step = (rows + n - 1) / n;
        for (int r = 0; r < rows; r += step) {
            chunks.push_back(y0 + r);
            chunks.push_back(y0 + std::min(r + step, rows));
        }
    }
    const size_t nchunk = chunks.size() / 2;
    cstart[(size_t)gh] = (int)nchunk;
    P.plane = (long long)nchunk * (long long)w;
    const size_t off_chunks = 0, off_cstart = up256(chunks.size() * sizeof(int)),
                 off_xe = off_cstart + up256(cstart.size() * sizeof(int)),
                 off_out = off_xe + up256(((size_t)gw + 1) * sizeof(int)), off_ws = off_out + up256(ncell * sizeof(QmapRecord)),
                 total = off_ws + (size_t)nsel * (size_t)P.plane * 8;
    DevTemp ws(ctx);                                    // chunks and cstart are older: they outlive the sync of its destructor
    SRCHK(ws.alloc("sr_quality_map_u8", total));
    char *dev = ws.as<char>();
    HIPCHK(hipMemcpyAsync(dev + off_chunks, chunks.data(), chunks.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(dev + off_cstart, cstart.data(), cstart.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(dev + off_xe, h_xedges, ((size_t)gw + 1) * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, "qmap");
        const dim3 grid((unsigned)nchunk, (unsigned)((w + S11_OUT - 1) / S11_OUT)), block(S11_TX);
        if (cn == 3)
            hipLaunchKernelGGL(k_qmap_cols<3>, grid, block, 0, ctx->stream, d_a, (long long)stride_a, d_b, (long long)stride_b, P,
                               (const int2 *)(dev + off_chunks), (unsigned long long *)(dev + off_ws));
        else
            hipLaunchKernelGGL(k_qmap_cols<1>, grid, block, 0, ctx->stream, d_a, (long long)stride_a, d_b, (long long)stride_b, P,
                               (const int2 *)(dev + off_chunks), (unsigned long long *)(dev + off_ws));
        hipLaunchKernelGGL(k_qmap_cells, dim3((unsigned)ncell), dim3(256), 0, ctx->stream, (const unsigned long long *)(dev + off_ws), P,
                           (const int *)(dev + off_xe), gw, (const int *)(dev + off_cstart), (QmapRecord *)(dev + off_out));
    }
    SRCHK(check_launch("qmap"));
    HIPCHK(hipMemcpyAsync(h_out, dev + off_out, ncell * sizeof(QmapRecord), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // extern "C"
