// sr_deltae.hip -- the per-pixel colour difference of two u8 images, CIEDE2000 or CIE76 (sr_delta_e_u8, sr_delta_e_cells_u8).
// The definition is in include/sr_hip.h; the per-pixel arithmetic (de_lab, de_2000, de_76) is sr_deltae.h's, shared with the
// host restatement; sizes, the launch, the scratch layout and every shape refusal are sr_deltae_host.cpp's (delta_e_plan).
//
// This is fp64 VALU and transcendental work (six cbrt, two atan2, four cos, two sin, one exp and a dozen sqrt and divisions
// per pixel for dE00), not bandwidth work: the pixels are read byte by byte, 6 B per RGB pair.
//   k_deltae<CN, F>      the sums.  A tile is DE_TH rows of DE_TW columns; a thread takes DE_RUN pixels of one row, DE_LANES
//                        apart (neighbouring threads read neighbouring pixels), one at a time so the formula is instantiated
//                        once.  Block b takes tiles b, b + blocks, ...: the assignment depends on the size alone.  The 256
//                        linear values sit in LDS beside the block's histogram (32-bit integer LDS atomics; byte-equal pairs
//                        skip the arithmetic and are counted per thread), which is flushed with 64-bit integer atomics.  The
//                        thread sums go through a fixed LDS tree: one (sum, sum2, max) partial per block.
//   k_deltae_finish      one block adds the partials in a fixed order.
//   k_deltae_cols<CN, F> the per-cell form: a block owns DE_THREADS columns and one row chunk (a cell row, or a piece of at most
//                        DE_CELL_ROWS rows of it); a thread walks down its column and stores the column's sum and max.
//   k_deltae_cells       a block per cell adds the chunk-column entries of the cell in (chunk, column) order.
// No floating-point atomics: equal inputs give equal bits.
#include <algorithm>
#include <cstring>
#include <vector>

#include "sr_ctx.h"
#include "sr_deltae.h"

namespace {

static_assert(DE_THREADS == DE_TABLE, "a block loads the table one entry per thread");

// The dE of the pixel pair at pa, pb; *same tells a byte-equal pair (exactly 0, nothing evaluated).
template <int CN, int F>
__device__ __forceinline__ double de_pixel(const unsigned char *__restrict__ pa, const unsigned char *__restrict__ pb,
                                           const double *T, bool *same)
{
    int r1, g1, b1, r2, g2, b2;
    if constexpr (CN == 1) {
        r1 = g1 = b1 = pa[0];
        r2 = g2 = b2 = pb[0];
    } else {
        r1 = pa[0]; g1 = pa[1]; b1 = pa[2];
        r2 = pb[0]; g2 = pb[1]; b2 = pb[2];
    }
    *same = r1 == r2 && g1 == g2 && b1 == b2;
    if (*same) return 0.0;
    double L1, A1, B1, L2, A2, B2;
    de_lab(T[r1], T[g1], T[b1], L1, A1, B1);
    de_lab(T[r2], T[g2], T[b2], L2, A2, B2);
    if constexpr (F == SR_DELTA_E_76) return de_76(L1, A1, B1, L2, A2, B2);
    return de_2000(L1, A1, B1, L2, A2, B2);
}

template <int CN, int F>
__global__ __launch_bounds__(DE_THREADS) void k_deltae(const unsigned char *__restrict__ a, long long sa,
                                                       const unsigned char *__restrict__ b, long long sb, int ch, int cw,
                                                       int tiles_x, long long tiles, const double *__restrict__ table,
                                                       unsigned long long *__restrict__ hist, double *__restrict__ part,
                                                       char *__restrict__ map, long long map_stride)
{
    __shared__ double T[DE_TABLE];
    __shared__ unsigned H[SR_DELTA_E_BINS];
    __shared__ double R[3][DE_THREADS];
    const int t = threadIdx.x;
    T[t] = table[t];
    for (int i = t; i < SR_DELTA_E_BINS; i += DE_THREADS) H[i] = 0u;
    __syncthreads();
    const int lane = t % DE_LANES, trow = t / DE_LANES;
    double s = 0.0, s2 = 0.0, mx = 0.0;
    unsigned zeros = 0;
#pragma unroll 1
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long ty = tile / tiles_x;
        const int tx = (int)(tile - ty * tiles_x);
        const long long y = ty * DE_TH + trow;
        if (y >= ch) continue;
        const unsigned char *ra = a + (size_t)y * (size_t)sa, *rb = b + (size_t)y * (size_t)sb;
        char *rm = map ? map + (size_t)y * (size_t)map_stride : nullptr;
#pragma unroll 1
        for (int k = 0; k < DE_RUN; ++k) {
            const long long x = (long long)tx * DE_TW + k * DE_LANES + lane;      // the last tile may reach past what an int holds
            if (x >= cw) break;
            bool same;
            const double de = de_pixel<CN, F>(ra + (size_t)x * CN, rb + (size_t)x * CN, T, &same);
            if (rm) *(double *)(rm + (size_t)x * sizeof(double)) = de;
            if (same) {
                ++zeros;
                continue;
            }
            s += de;
            s2 += de * de;
            mx = de > mx ? de : mx;
            atomicAdd(&H[de_bin(de)], 1u);
        }
    }
    if (zeros) atomicAdd(&H[0], zeros);
    R[0][t] = s;
    R[1][t] = s2;
    R[2][t] = mx;
    __syncthreads();
    for (int st = DE_THREADS / 2; st > 0; st >>= 1) {
        if (t < st) {
            R[0][t] += R[0][t + st];
            R[1][t] += R[1][t + st];
            R[2][t] = R[2][t + st] > R[2][t] ? R[2][t + st] : R[2][t];
        }
        __syncthreads();
    }
    for (int i = t; i < SR_DELTA_E_BINS; i += DE_THREADS)
        if (H[i]) atomicAdd(&hist[i], (unsigned long long)H[i]);
    if (t == 0) {
        part[(size_t)blockIdx.x * 3] = R[0][0];
        part[(size_t)blockIdx.x * 3 + 1] = R[1][0];
        part[(size_t)blockIdx.x * 3 + 2] = R[2][0];
    }
}

// One block: thread t adds partials t, t + DE_THREADS, ... in that order, the thread sums go through the fixed tree.
__global__ __launch_bounds__(DE_THREADS) void k_deltae_finish(const double *__restrict__ part, int n, double *__restrict__ out)
{
    __shared__ double R[3][DE_THREADS];
    const int t = threadIdx.x;
    double s = 0.0, s2 = 0.0, mx = 0.0;
    for (int i = t; i < n; i += DE_THREADS) {
        s += part[(size_t)i * 3];
        s2 += part[(size_t)i * 3 + 1];
        const double m = part[(size_t)i * 3 + 2];
        mx = m > mx ? m : mx;
    }
    R[0][t] = s;
    R[1][t] = s2;
    R[2][t] = mx;
    __syncthreads();
    for (int st = DE_THREADS / 2; st > 0; st >>= 1) {
        if (t < st) {
            R[0][t] += R[0][t + st];
            R[1][t] += R[1][t + st];
            R[2][t] = R[2][t + st] > R[2][t] ? R[2][t + st] : R[2][t];
        }
        __syncthreads();
    }
    if (t < 3) out[t] = R[t][0];
}

// ws[0][chunk][column] = the sum, ws[1][chunk][column] = the max of the column's pixels inside the chunk's rows
template <int CN, int F>
__global__ __launch_bounds__(DE_THREADS) void k_deltae_cols(const unsigned char *__restrict__ a, long long sa,
                                                            const unsigned char *__restrict__ b, long long sb, int cw,
                                                            const int2 *__restrict__ chunks, long long plane,
                                                            const double *__restrict__ table, double *__restrict__ ws)
{
    __shared__ double T[DE_TABLE];
    const int t = threadIdx.x;
    T[t] = table[t];
    __syncthreads();
    const int x = (int)blockIdx.y * DE_THREADS + t;
    if (x >= cw) return;
    const int2 ck = chunks[blockIdx.x];
    const unsigned char *ca = a + (size_t)x * CN, *cb = b + (size_t)x * CN;
    double s = 0.0, mx = 0.0;
#pragma unroll 1
    for (int y = ck.x; y < ck.y; ++y) {
        bool same;
        const double de = de_pixel<CN, F>(ca + (size_t)y * (size_t)sa, cb + (size_t)y * (size_t)sb, T, &same);
        if (same) continue;
        s += de;
        mx = de > mx ? de : mx;
    }
    const size_t at = (size_t)blockIdx.x * (size_t)cw + (size_t)x;
    ws[at] = s;
    ws[(size_t)plane + at] = mx;
}

struct DeCell {
    double sum, max;
};

__global__ __launch_bounds__(DE_THREADS) void k_deltae_cells(const double *__restrict__ ws, long long plane, int cw,
                                                             const int *__restrict__ xe, int gw, const int *__restrict__ cstart,
                                                             DeCell *__restrict__ out)
{
    __shared__ double R[2][DE_THREADS];
    const int t = threadIdx.x;
    const int gy = (int)(blockIdx.x / (unsigned)gw), gx = (int)(blockIdx.x - (unsigned)gy * (unsigned)gw);
    const int x0 = xe[gx], x1 = xe[gx + 1], c0 = cstart[gy], c1 = cstart[gy + 1];
    double s = 0.0, mx = 0.0;
    for (int c = c0; c < c1; ++c) {
        const size_t row = (size_t)c * (size_t)cw;
        for (int x = x0 + t; x < x1; x += DE_THREADS) {
            s += ws[row + x];
            const double m = ws[(size_t)plane + row + x];
            mx = m > mx ? m : mx;
        }
    }
    R[0][t] = s;
    R[1][t] = mx;
    __syncthreads();
    for (int st = DE_THREADS / 2; st > 0; st >>= 1) {
        if (t < st) {
            R[0][t] += R[0][t + st];
            R[1][t] = R[1][t + st] > R[1][t] ? R[1][t + st] : R[1][t];
        }
        __syncthreads();
    }
    if (t == 0) {
        DeCell r;
        r.sum = R[0][0];
        r.max = R[1][0];
        out[blockIdx.x] = r;
    }
}

int de_check_edges(const char *scope, const char *axis, const int *e, int n, int size)
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
int de_args(const char *scope, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w, int cn,
            int crop_border, int formula, const void *h_out, DePlan *p)
{
    if (!d_a || !d_b || !h_out) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", scope);
    const int rc = delta_e_plan(scope, h, w, cn, crop_border, formula, p);
    if (rc) return rc;
    const int64_t min_stride = (int64_t)w * cn;
    if (stride_a < min_stride || stride_b < min_stride) return sr_set_error(SR_ERR_SHAPE, "%s: stride smaller than a row", scope);
    return SR_OK;
}

// The context scratch of at least `bytes` with the table at its start (uploaded again whenever the buffer was regrown).
int de_scratch(sr_ctx *ctx, const char *scope, size_t bytes)
{
    bool regrown = false;
    SRCHK(ctx->deltae_ws.reserve(ctx, scope, bytes, 0, 1, &regrown));
    if (regrown || !ctx->deltae_table) {
        double table[DE_TABLE];
        delta_e_table(table);
        ctx->deltae_table = false;
        HIPCHK(upload_small(ctx, ctx->deltae_ws.d, table, sizeof(table)));
        ctx->deltae_table = true;
    }
    return SR_OK;
}

#define DE_DISPATCH(KERNEL, ...)                                                                              \
    do {                                                                                                      \
        if (formula == SR_DELTA_E_2000) {                                                                     \
            if (cn == 1) hipLaunchKernelGGL((KERNEL<1, SR_DELTA_E_2000>), __VA_ARGS__);                       \
            else if (cn == 3) hipLaunchKernelGGL((KERNEL<3, SR_DELTA_E_2000>), __VA_ARGS__);                  \
            else hipLaunchKernelGGL((KERNEL<4, SR_DELTA_E_2000>), __VA_ARGS__);                               \
        } else {                                                                                              \
            if (cn == 1) hipLaunchKernelGGL((KERNEL<1, SR_DELTA_E_76>), __VA_ARGS__);                         \
            else if (cn == 3) hipLaunchKernelGGL((KERNEL<3, SR_DELTA_E_76>), __VA_ARGS__);                    \
            else hipLaunchKernelGGL((KERNEL<4, SR_DELTA_E_76>), __VA_ARGS__);                                 \
        }                                                                                                     \
    } while (0)

}  // namespace

extern "C" {

int sr_delta_e_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w, int cn,
                  int crop_border, int formula, double *d_map, int64_t map_stride, sr_delta_e_sums *h_out)
{
    // every argument check comes before the context (and so the device) is touched
    DePlan p;
    SRCHK(de_args("sr_delta_e_u8", d_a, stride_a, d_b, stride_b, h, w, cn, crop_border, formula, h_out, &p));
    if (d_map) {
        if (((uintptr_t)d_map & 7u) || map_stride % 8 != 0)
            return sr_set_error(SR_ERR_INVALID_ARG, "sr_delta_e_u8: the map and its stride must be multiples of 8 bytes");
        if (map_stride < (int64_t)p.cw * 8) return sr_set_error(SR_ERR_SHAPE, "sr_delta_e_u8: map stride smaller than a row of the cropped image");
    }
    CTX_ENTER(ctx);
    SRCHK(de_scratch(ctx, "sr_delta_e_u8", p.total));
    char *ws = ctx->deltae_ws.as<char>();
    const double *table = (const double *)(ws + p.off_table);
    unsigned long long *hist = (unsigned long long *)(ws + p.off_hist);
    double *result = (double *)(ws + p.off_result), *part = (double *)(ws + p.off_part);
    const unsigned char *a = d_a + (size_t)crop_border * (size_t)stride_a + (size_t)crop_border * (size_t)cn;
    const unsigned char *b = d_b + (size_t)crop_border * (size_t)stride_b + (size_t)crop_border * (size_t)cn;
    double h_res[3];
    {
        ProfScope ps(ctx, "deltae");
        HIPCHK(hipMemsetAsync(hist, 0, SR_DELTA_E_BINS * sizeof(uint64_t), ctx->stream));
        DE_DISPATCH(k_deltae, dim3((unsigned)p.blocks), dim3(DE_THREADS), 0, ctx->stream, a, (long long)stride_a, b, (long long)stride_b,
                    p.ch, p.cw, p.tiles_x, p.tiles, table, hist, part, (char *)d_map, (long long)map_stride);
        hipLaunchKernelGGL(k_deltae_finish, dim3(1), dim3(DE_THREADS), 0, ctx->stream, (const double *)part, p.blocks, result);
        SRCHK(check_launch("deltae"));
        HIPCHK(hipMemcpyAsync(h_res, result, sizeof(h_res), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(h_out->hist, hist, SR_DELTA_E_BINS * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(stream_sync(ctx));
    h_out->count = p.count;
    h_out->sum = h_res[0];
    h_out->sum2 = h_res[1];
    h_out->max = h_res[2];
    return SR_OK;
}

int sr_delta_e_cells_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                        int cn, int crop_border, int formula, const int *h_xedges, int gw, const int *h_yedges, int gh,
                        sr_delta_e_cell *h_out)
{
    static_assert(sizeof(DeCell) == sizeof(sr_delta_e_cell), "device and ABI records differ");
    DePlan p;
    SRCHK(de_args("sr_delta_e_cells_u8", d_a, stride_a, d_b, stride_b, h, w, cn, crop_border, formula, h_out, &p));
    SRCHK(de_check_edges("sr_delta_e_cells_u8", "x", h_xedges, gw, p.cw));
    SRCHK(de_check_edges("sr_delta_e_cells_u8", "y", h_yedges, gh, p.ch));
    // a launch holds fewer than 2^32 threads along x: one block per cell, and one per row chunk
    constexpr long long DE_GRID_X = (1ll << 32) / DE_THREADS - 1;
    if ((int64_t)gh * gw > DE_GRID_X)
        return sr_set_error(SR_ERR_UNSUPPORTED, "sr_delta_e_cells_u8: %lld cells are more than one launch covers (%lld)",
                            (long long)gh * gw, DE_GRID_X);
    long long want_chunks = 0;
    for (int gy = 0; gy < gh; ++gy)
        want_chunks += ((long long)h_yedges[gy + 1] - h_yedges[gy] + DE_CELL_ROWS - 1) / DE_CELL_ROWS;
    if (want_chunks > DE_GRID_X)
        return sr_set_error(SR_ERR_UNSUPPORTED, "sr_delta_e_cells_u8: %lld row chunks (cell rows in pieces of %d rows) are more than "
                            "one launch covers (%lld)", want_chunks, DE_CELL_ROWS, DE_GRID_X);
    if (((long long)p.cw + DE_THREADS - 1) / DE_THREADS > 65535)
        return sr_set_error(SR_ERR_UNSUPPORTED, "sr_delta_e_cells_u8: %d columns after the crop are more than one launch covers (%d)",
                            p.cw, 65535 * DE_THREADS);
    CTX_ENTER(ctx);
    const size_t ncell = (size_t)gh * (size_t)gw;
    // row chunks: every cell row in equal pieces of at most DE_CELL_ROWS rows
    std::vector<int> chunks, cstart((size_t)gh + 1);
    for (int gy = 0; gy < gh; ++gy) {
        cstart[(size_t)gy] = (int)(chunks.size() / 2);
        const int y0 = h_yedges[gy], rows = h_yedges[gy + 1] - y0;
        const long long n = ((long long)rows + DE_CELL_ROWS - 1) / DE_CELL_ROWS, step = (rows + n - 1) / n;
        for (long long r = 0; r < rows; r += step) {
            chunks.push_back(y0 + (int)r);
            chunks.push_back(y0 + (int)std::min<long long>(r + step, rows));
        }
    }
    const size_t nchunk = chunks.size() / 2;
    cstart[(size_t)gh] = (int)nchunk;
    const long long plane = (long long)nchunk * (long long)p.cw;
    const size_t off_chunks = up256(DE_TABLE * sizeof(double)), off_cstart = off_chunks + up256(chunks.size() * sizeof(int)),
                 off_xe = off_cstart + up256(cstart.size() * sizeof(int)), off_out = off_xe + up256(((size_t)gw + 1) * sizeof(int)),
                 off_ws = off_out + up256(ncell * sizeof(DeCell)), total = off_ws + 2 * (size_t)plane * sizeof(double);
    SRCHK(de_scratch(ctx, "sr_delta_e_cells_u8", total));
    char *dev = ctx->deltae_ws.as<char>();
    HIPCHK(upload_small(ctx, dev + off_chunks, chunks.data(), chunks.size() * sizeof(int)));
    HIPCHK(upload_small(ctx, dev + off_cstart, cstart.data(), cstart.size() * sizeof(int)));
    HIPCHK(upload_small(ctx, dev + off_xe, h_xedges, ((size_t)gw + 1) * sizeof(int)));
    const unsigned char *a = d_a + (size_t)crop_border * (size_t)stride_a + (size_t)crop_border * (size_t)cn;
    const unsigned char *b = d_b + (size_t)crop_border * (size_t)stride_b + (size_t)crop_border * (size_t)cn;
    {
        ProfScope ps(ctx, "deltae_cells");
        const dim3 grid((unsigned)nchunk, (unsigned)(((long long)p.cw + DE_THREADS - 1) / DE_THREADS));
        DE_DISPATCH(k_deltae_cols, grid, dim3(DE_THREADS), 0, ctx->stream, a, (long long)stride_a, b, (long long)stride_b, p.cw,
                    (const int2 *)(dev + off_chunks), plane, (const double *)dev, (double *)(dev + off_ws));
        hipLaunchKernelGGL(k_deltae_cells, dim3((unsigned)ncell), dim3(DE_THREADS), 0, ctx->stream, (const double *)(dev + off_ws),
                           plane, p.cw, (const int *)(dev + off_xe), gw, (const int *)(dev + off_cstart), (DeCell *)(dev + off_out));
    }
    SRCHK(check_launch("deltae_cells"));
    HIPCHK(hipMemcpyAsync(h_out, dev + off_out, ncell * sizeof(DeCell), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // extern "C"
