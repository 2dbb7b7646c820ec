// sr_haarpsi.hip -- the Haar wavelet perceptual similarity index of two u8 images (sr_haarpsi_u8, sr_haarpsi_cells_u8).  The
// definition is in include/sr_hip.h; the per-sample float64 arithmetic (hp_sample) and the pooled integer planes (hp_pool) are
// sr_haarpsi.h's, shared with the host restatement; sizes, the launch, the scratch layout and every shape refusal are
// sr_haarpsi_host.cpp's (haarpsi_plan).
//
// One kernel, one launch, one pass over both images.  Everything up to the coefficients is an exact integer.
// k_haarpsi<CN, SUB>  a block owns HP_TH x HP_TW samples.  It forms the pooled planes of both images for its samples and a halo of
//   3 + o before and 4 - o after into LDS (pixels are read byte by byte: the crop is pointer arithmetic and has any residue; a
//   sample outside the map is zero), luma everywhere, chroma only where the 2 x 2 window reaches.  The luma planes then become
//   their own summed-area tables by two separable running sums in 32-bit integers (rows in segments of HP_SEG, then columns):
//   every box of the six Haar differences is four table reads, and the 8 corner and mid-edge reads of a scale serve V and H
//   both.  In the tile's coordinates the window of sample (li, lj) is centred at (li + 3, lj + 3) whatever o is: the
//   convention only moves the tile's origin.  Each thread takes 4 samples through hp_sample and the block adds the six sums
//   through a fixed tree.  With a map pointer the per-sample (num, den) over the channels are stored too (the per-cell form).
// k_haarpsi_cells     a block per cell adds the cell's samples in a fixed order.
// The per-block partials go through reduce_partials: no floating-point atomics, equal inputs give equal bits.
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "sr_ctx.h"
#include "sr_haarpsi.h"

namespace {

constexpr int HP_SATW = HP_SW + 2;          // a table row: the zero column, HP_SW sums and one word that keeps the pitch odd
constexpr int HP_SEG = 16;                  // columns one thread sums in the row pass
constexpr int HP_NSEG = (HP_SW + HP_SEG - 1) / HP_SEG;
static_assert(HP_SATW % 2 == 1, "an odd pitch keeps the row pass off one LDS bank");
static_assert(2 * HP_SH * HP_NSEG <= HP_THREADS, "one thread per row segment of both images");
static_assert(2 * HP_SW <= HP_THREADS, "one thread per column of both images");
static_assert(HP_THREADS % HP_TW == 0 && (HP_TH * HP_TW) % HP_THREADS == 0, "a thread takes whole samples");

// the six Haar sums of the sample (li, lj) of the tile from the summed-area table T (T[r][c]: rows < r, columns < c)
__device__ __forceinline__ void hp_haar(const unsigned (*T)[HP_SATW], int li, int lj, int (&v)[2][3])
{
    const int m = li + 4, cm = lj + 4;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int hf = 1 << s, t = m - hf, bt = m + hf, c0 = cm - hf, c1 = cm + hf;
        const unsigned tc0 = T[t][c0], tc1 = T[t][c1], bc0 = T[bt][c0], bc1 = T[bt][c1];
        const unsigned mc0 = T[m][c0], mc1 = T[m][c1], tcm = T[t][cm], bcm = T[bt][cm];
        // modulo 2^32 throughout; the results are below 2^26 in magnitude
        v[0][s] = (int)(2u * (mc1 - mc0) - (tc1 - tc0) - (bc1 - bc0));     // rows above minus rows below
        v[1][s] = (int)(2u * (bcm - tcm) - (bc0 - tc0) - (bc1 - tc1));     // columns left minus columns right
    }
}

template <int CN, bool SUB>
__global__ __launch_bounds__(HP_THREADS) void k_haarpsi(const unsigned char *__restrict__ a, long long sa,
                                                        const unsigned char *__restrict__ b, long long sb, int ch, int cw, int mh,
                                                        int mw, int o, int tiles_x, double div, double *__restrict__ part,
                                                        double *__restrict__ map)
{
    constexpr bool COLOUR = CN >= 3;
    __shared__ unsigned T[2][HP_SH + 1][HP_SATW];
    __shared__ int Cp[COLOUR ? 4 : 1][COLOUR ? HP_CH : 1][COLOUR ? HP_CW : 1];      // I, Q of a, then I, Q of b
    __shared__ double R[HP_COMP][HP_THREADS];
    const int t = threadIdx.x;
    const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x);
    const long long i0 = (long long)ty * HP_TH, j0 = (long long)tx * HP_TW;
    for (int idx = t; idx < HP_SATW; idx += HP_THREADS) T[0][0][idx] = T[1][0][idx] = 0u;
    for (int idx = t; idx <= HP_SH; idx += HP_THREADS) T[0][idx][0] = T[1][idx][0] = 0u;
    for (int idx = t; idx < HP_SH * HP_SW; idx += HP_THREADS) {
        const int lr = idx / HP_SW, lc = idx - lr * HP_SW;
        const long long i = i0 - 3 - o + lr, j = j0 - 3 - o + lc;
        int y1 = 0, i1 = 0, q1 = 0, y2 = 0, i2 = 0, q2 = 0;
        if (i >= 0 && i < mh && j >= 0 && j < mw) {
            hp_pool<CN, SUB>(a, sa, ch, cw, o, (int)i, (int)j, y1, i1, q1);
            hp_pool<CN, SUB>(b, sb, ch, cw, o, (int)i, (int)j, y2, i2, q2);
        }
        T[0][lr + 1][lc + 1] = (unsigned)y1;
        T[1][lr + 1][lc + 1] = (unsigned)y2;
        if constexpr (COLOUR) {
            const int cr = lr - 3, cc = lc - 3;
            if (cr >= 0 && cr < HP_CH && cc >= 0 && cc < HP_CW) {
                Cp[0][cr][cc] = i1;
                Cp[1][cr][cc] = q1;
                Cp[2][cr][cc] = i2;
                Cp[3][cr][cc] = q2;
            }
        }
    }
    __syncthreads();
    // rows: a running sum inside every segment, then the segments before it added
    {
        const bool act = t < 2 * HP_SH * HP_NSEG;
        const int img = t / (HP_SH * HP_NSEG), rem = t - img * (HP_SH * HP_NSEG);
        const int row = rem / HP_NSEG + 1, seg = rem - (row - 1) * HP_NSEG;
        const int c_begin = seg * HP_SEG + 1, c_end = c_begin + HP_SEG < HP_SW + 1 ? c_begin + HP_SEG : HP_SW + 1;
        if (act) {
            unsigned run = 0u;
            for (int c = c_begin; c < c_end; ++c) {
                run += T[img][row][c];
                T[img][row][c] = run;
            }
        }
        __syncthreads();
        unsigned before = 0u;
        if (act)
            for (int k = 0; k < seg; ++k) before += T[img][row][(k + 1) * HP_SEG];      // the last column of segment k
        __syncthreads();
        if (act && seg > 0)
            for (int c = c_begin; c < c_end; ++c) T[img][row][c] += before;
        __syncthreads();
    }
    // columns
    if (t < 2 * HP_SW) {
        const int img = t / HP_SW, c = t - img * HP_SW + 1;
        unsigned run = 0u;
        for (int r = 1; r <= HP_SH; ++r) {
            run += T[img][r][c];
            T[img][r][c] = run;
        }
    }
    __syncthreads();
    double acc[HP_COMP] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int lj = t % HP_TW;
#pragma unroll 1
    for (int k = 0; k < HP_TH * HP_TW / HP_THREADS; ++k) {
        const int li = t / HP_TW + k * (HP_THREADS / HP_TW);
        if (i0 + li >= mh || j0 + lj >= mw) continue;
        int va[2][3], vb[2][3];
        hp_haar(T[0], li, lj, va);
        hp_haar(T[1], li, lj, vb);
        int ia = 0, qa = 0, ib = 0, qb = 0;
        if constexpr (COLOUR) {
            ia = (Cp[0][li][lj] + Cp[0][li][lj + 1]) + (Cp[0][li + 1][lj] + Cp[0][li + 1][lj + 1]);
            qa = (Cp[1][li][lj] + Cp[1][li][lj + 1]) + (Cp[1][li + 1][lj] + Cp[1][li + 1][lj + 1]);
            ib = (Cp[2][li][lj] + Cp[2][li][lj + 1]) + (Cp[2][li + 1][lj] + Cp[2][li + 1][lj + 1]);
            qb = (Cp[3][li][lj] + Cp[3][li][lj + 1]) + (Cp[3][li + 1][lj] + Cp[3][li + 1][lj + 1]);
        }
        double n[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0};
        hp_sample<COLOUR>(va, vb, ia, qa, ib, qb, div, n, d);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            acc[c] += n[c];
            acc[3 + c] += d[c];
        }
        if (map) {
            double *m = map + ((size_t)(i0 + li) * (size_t)mw + (size_t)(j0 + lj)) * 2;
            m[0] = (n[0] + n[1]) + n[2];
            m[1] = (d[0] + d[1]) + d[2];
        }
    }
#pragma unroll
    for (int c = 0; c < HP_COMP; ++c) R[c][t] = acc[c];
    __syncthreads();
    for (int s = HP_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int c = 0; c < HP_COMP; ++c) R[c][t] += R[c][t + s];
        }
        __syncthreads();
    }
    if (t < HP_COMP) part[(size_t)blockIdx.x * HP_COMP + t] = R[t][0];
}

struct HpCell {
    double num, den;
};

// je[0 .. gw], ie[0 .. gh]: the cells' first samples (a cell may hold none)
__global__ __launch_bounds__(HP_THREADS) void k_haarpsi_cells(const double *__restrict__ map, int mw, const int *__restrict__ je, int gw,
                                                              const int *__restrict__ ie, HpCell *__restrict__ out)
{
    __shared__ double R[2][HP_THREADS];
    const int t = threadIdx.x;
    const int gy = (int)(blockIdx.x / (unsigned)gw), gx = (int)(blockIdx.x - (unsigned)gy * (unsigned)gw);
    const int j0 = je[gx], nw = je[gx + 1] - j0, i0 = ie[gy], nh = ie[gy + 1] - i0;
    const long long n = (long long)nh * nw;
    double sn = 0.0, sd = 0.0;
    for (long long idx = t; idx < n; idx += HP_THREADS) {
        const long long r = idx / nw, c = idx - r * nw;
        const double *m = map + ((size_t)(i0 + r) * (size_t)mw + (size_t)(j0 + c)) * 2;
        sn += m[0];
        sd += m[1];
    }
    R[0][t] = sn;
    R[1][t] = sd;
    __syncthreads();
    for (int s = HP_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            R[0][t] += R[0][t + s];
            R[1][t] += R[1][t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        HpCell r;
        r.num = R[0][0];
        r.den = R[1][0];
        out[blockIdx.x] = r;
    }
}

int hp_check_edges(const char *scope, const char *axis, const int *e, int n, int size)
{
    if (n < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: the grid needs at least one cell along %s", scope, axis);
    if (!e) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null %s edges", scope, axis);
    if (e[0] != 0 || e[n] != size)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: %s edges must run from 0 to %d, the cropped side (got %d .. %d)", scope, axis,
                            size, e[0], e[n]);
    for (int i = 0; i < n; ++i)
        if (e[i + 1] <= e[i])
            return sr_set_error(SR_ERR_INVALID_ARG, "%s: %s edges must be strictly increasing (edge %d: %d after %d)", scope, axis,
                                i + 1, e[i + 1], e[i]);
    return SR_OK;
}

// what both entry points refuse alike, before the context is touched
int hp_args(const char *scope, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w, int cn,
            int crop_border, int subsample, int convention, const void *h_out, HpPlan *p)
{
    if (!d_a || !d_b || !h_out) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", scope);
    const int rc = haarpsi_plan(scope, h, w, cn, crop_border, subsample, convention, p);
    if (rc) return rc;
    const int64_t min_stride = (int64_t)w * cn;
    if (stride_a < min_stride || stride_b < min_stride) return sr_set_error(SR_ERR_SHAPE, "%s: stride smaller than a row", scope);
    return SR_OK;
}

// The launch and the reduction of its partials; -> the six sums on the device.
const double *hp_launch(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int cn,
                        int crop_border, int subsample, int convention, const HpPlan &p, char *ws, double *map)
{
    double *part = (double *)(ws + p.off_part), *buf0 = (double *)(ws + p.off_buf0), *buf1 = (double *)(ws + p.off_buf1);
    const unsigned char *a = d_a + (size_t)crop_border * (size_t)stride_a + (size_t)crop_border * (size_t)cn;
    const unsigned char *b = d_b + (size_t)crop_border * (size_t)stride_b + (size_t)crop_border * (size_t)cn;
    const long long tiles = (long long)p.tiles_x * p.tiles_y;
    const dim3 grid((unsigned)tiles), block(HP_THREADS);
    const int o = convention == SR_HAARPSI_PYTHON ? 1 : 0;
    const double div = subsample ? 4000.0 : 1000.0;
#define HP_GO(CN, SUB)                                                                                                          \
    hipLaunchKernelGGL((k_haarpsi<CN, SUB>), grid, block, 0, ctx->stream, a, (long long)stride_a, b, (long long)stride_b, p.ch,  \
                       p.cw, p.mh, p.mw, o, p.tiles_x, div, part, map)
    if (subsample) {
        if (cn == 1) HP_GO(1, true);
        else if (cn == 3) HP_GO(3, true);
        else HP_GO(4, true);
    } else {
        if (cn == 1) HP_GO(1, false);
        else if (cn == 3) HP_GO(3, false);
        else HP_GO(4, false);
    }
#undef HP_GO
    return reduce_partials(ctx, part, tiles, HP_COMP, buf0, buf1);
}

}  // namespace

extern "C" {

int sr_haarpsi_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w, int cn,
                  int crop_border, int subsample, int convention, sr_haarpsi_sums *h_out)
{
    // every argument check comes before the context (and so the device) is touched
    HpPlan p;
    SRCHK(hp_args("sr_haarpsi_u8", d_a, stride_a, d_b, stride_b, h, w, cn, crop_border, subsample, convention, h_out, &p));
    CTX_ENTER(ctx);
    SRCHK(ctx->haarpsi_ws.reserve(ctx, "sr_haarpsi_u8", p.total));
    double h_res[HP_COMP];
    {
        ProfScope ps(ctx, "haarpsi");
        const double *sums = hp_launch(ctx, d_a, stride_a, d_b, stride_b, cn, crop_border, subsample, convention, p,
                                       ctx->haarpsi_ws.as<char>(), nullptr);
        SRCHK(check_launch("haarpsi"));
        HIPCHK(hipMemcpyAsync(h_res, sums, sizeof(h_res), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(stream_sync(ctx));
    for (int k = 0; k < 3; ++k) {
        h_out->num[k] = h_res[k];
        h_out->den[k] = h_res[3 + k];
    }
    h_out->channels = p.channels;
    h_out->reserved = 0;
    h_out->count = p.count;
    return SR_OK;
}

int sr_haarpsi_cells_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                        int cn, int crop_border, int subsample, int convention, const int *h_xedges, int gw, const int *h_yedges,
                        int gh, sr_haarpsi_cell *h_out)
{
    static_assert(sizeof(HpCell) == sizeof(sr_haarpsi_cell), "device and ABI records differ");
    HpPlan p;
    SRCHK(hp_args("sr_haarpsi_cells_u8", d_a, stride_a, d_b, stride_b, h, w, cn, crop_border, subsample, convention, h_out, &p));
    SRCHK(hp_check_edges("sr_haarpsi_cells_u8", "x", h_xedges, gw, p.cw));
    SRCHK(hp_check_edges("sr_haarpsi_cells_u8", "y", h_yedges, gh, p.ch));
    constexpr long long HP_MAX_CELLS = (1ll << 24) - 1;
    if ((int64_t)gh * gw > HP_MAX_CELLS)
        return sr_set_error(SR_ERR_UNSUPPORTED, "sr_haarpsi_cells_u8: %lld cells are more than one launch covers (%lld)",
                            (long long)gh * gw, HP_MAX_CELLS);
    // the first sample of every cell: sample i sits at cropped pixel 2 i (or i).  Sized before the context is entered: no
    // exception leaves this function
    std::vector<int> je, ie;
    try {
        je.resize((size_t)gw + 1);
        ie.resize((size_t)gh + 1);
    } catch (const std::bad_alloc &) {
        return sr_set_error(SR_ERR_OOM, "sr_haarpsi_cells_u8: out of host memory for the edges of %d x %d cells", gw, gh);
    }
    CTX_ENTER(ctx);
    for (int g = 0; g <= gw; ++g) je[(size_t)g] = subsample ? (int)(((long long)h_xedges[g] + 1) / 2) : h_xedges[g];
    for (int g = 0; g <= gh; ++g) ie[(size_t)g] = subsample ? (int)(((long long)h_yedges[g] + 1) / 2) : h_yedges[g];
    const size_t ncell = (size_t)gh * (size_t)gw;
    const size_t off_map = p.total, off_je = off_map + up256((size_t)p.count * 2 * sizeof(double)),
                 off_ie = off_je + up256(je.size() * sizeof(int)), off_out = off_ie + up256(ie.size() * sizeof(int)),
                 total = off_out + up256(ncell * sizeof(HpCell));
    SRCHK(ctx->haarpsi_ws.reserve(ctx, "sr_haarpsi_cells_u8", total));
    char *ws = ctx->haarpsi_ws.as<char>();
    HIPCHK(upload_small(ctx, ws + off_je, je.data(), je.size() * sizeof(int)));
    HIPCHK(upload_small(ctx, ws + off_ie, ie.data(), ie.size() * sizeof(int)));
    {
        ProfScope ps(ctx, "haarpsi_cells");
        hp_launch(ctx, d_a, stride_a, d_b, stride_b, cn, crop_border, subsample, convention, p, ws, (double *)(ws + off_map));
        hipLaunchKernelGGL(k_haarpsi_cells, dim3((unsigned)ncell), dim3(HP_THREADS), 0, ctx->stream, (const double *)(ws + off_map),
                           p.mw, (const int *)(ws + off_je), gw, (const int *)(ws + off_ie), (HpCell *)(ws + off_out));
    }
    SRCHK(check_launch("haarpsi_cells"));
    HIPCHK(hipMemcpyAsync(h_out, ws + off_out, ncell * sizeof(HpCell), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // extern "C"
