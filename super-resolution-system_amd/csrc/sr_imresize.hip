// sr_imresize.hip -- the device side of MATLAB's bicubic imresize (sr_imresize_u8).  The definition is in include/sr_hip.h; the
// tables, the plan and every shape refusal are host code (sr_imresize_host.cpp, shared through sr_imresize.h).
//   k_imresize<ORDER>  One launch per call.  The first pass runs along axis A (ORDER 0: the height, 1: the width), the second
//     along axis B.  A workgroup owns tile_a x tile_b outputs.  Its second pass reads the unreflected positions
//     [start_b[b0], start_b[b1 - 1] + taps_b) of axis B: at most span_b of them (imr_plan holds the bound against the tables).
//     First pass: for each of those positions (reflected into the image on the fly: a border tile recomputes what it folds
//     onto, so LDS is addressed without a gather) and each of the tile's outputs along A, the taps_a weighted source bytes are
//     added in ascending tap order into a float64 LDS cell.  One barrier.  Second pass: each output adds its taps_b weighted
//     LDS cells in ascending tap order and is stored once.  No float64 intermediate leaves the CU, no atomics; an output's two
//     sums do not depend on the tile it falls in, so neither do its bits.
//   LDS: tile_a * span_b * cn float64, at most IMR_LDS_DOUBLES (48 KB): ORDER 0 as [a][position][c], ORDER 1 as
//     [position][a][c], so that in both passes consecutive threads touch consecutive cells.
// Source pixels are read byte by byte (no alignment assumed) at 64-bit offsets; the destination is written element by element.
#include <cstring>
#include <vector>

#include "sr_ctx.h"
#include "sr_imresize.h"

namespace {

struct ImrArgs {
    const unsigned char *src;
    long long src_stride;
    int h, w, cn;
    void *dst;
    long long dst_stride;
    int dh, dw;
    const double *wa;           // first pass: n_out_a x taps_a weights and reflected source indices
    const int *idxa;
    int taps_a;
    const double *wb;           // second pass: n_out_b x taps_b weights, the unreflected start per output
    const int *startb;
    int taps_b;
    int tile_a, tile_b, span_b;
    int tiles_b;
};

__device__ inline int reflect_dev(long long u, int n)
{
    long long j = (u - 1) % (2LL * n);
    if (j < 0) j += 2LL * n;
    return (int)(j >= n ? 2LL * n - 1 - j : j);
}

template <int OUT>
__device__ inline void store_out(const ImrArgs &A, int oy, int ox, int c, double v)
{
    char *row = (char *)A.dst + (size_t)oy * (size_t)A.dst_stride;
    const size_t e = (size_t)ox * (size_t)A.cn + (size_t)c;
    if constexpr (OUT == SR_IMRESIZE_U8)
        ((unsigned char *)row)[e] = (unsigned char)fmin(255.0, fmax(0.0, floor(v + 0.5)));
    else if constexpr (OUT == SR_IMRESIZE_F32)
        ((float *)row)[e] = (float)v;
    else
        ((double *)row)[e] = v;
}

// sum over k < taps of w[k] * load(k), added in ascending k (the definition's order).  The loads of a chunk of 8, 4 or 2 taps are
// issued before its additions, so that they are in flight together; the chain of additions is the same whatever the chunks.
template <int N, class Load>
__device__ inline void tap_chunk(const double *w, int k, Load load, double &acc)
{
    double v[N];
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = load(k + j);
#pragma unroll
    for (int j = 0; j < N; ++j) acc += w[k + j] * v[j];
}

template <class Load>
__device__ inline double tap_sum(const double *w, int taps, Load load)
{
    double acc = 0.0;
    int k = 0;
    for (; k + 8 <= taps; k += 8) tap_chunk<8>(w, k, load, acc);
    if (k + 4 <= taps) {
        tap_chunk<4>(w, k, load, acc);
        k += 4;
    }
    if (k + 2 <= taps) {
        tap_chunk<2>(w, k, load, acc);
        k += 2;
    }
    if (k < taps) tap_chunk<1>(w, k, load, acc);
    return acc;
}

template <int ORDER, int OUT>
__global__ __launch_bounds__(IMR_THREADS) void k_imresize(const ImrArgs A)
{
    extern __shared__ __attribute__((aligned(16))) double T[];
    const int t = threadIdx.x, cn = A.cn;
    const int n_out_a = ORDER == 0 ? A.dh : A.dw, n_out_b = ORDER == 0 ? A.dw : A.dh;
    const int n_in_b = ORDER == 0 ? A.w : A.h;
    const int ta = (int)blockIdx.x / A.tiles_b, tb = (int)blockIdx.x - ta * A.tiles_b;
    const int a0 = ta * A.tile_a, b0 = tb * A.tile_b;
    const int na = min(A.tile_a, n_out_a - a0), nb = min(A.tile_b, n_out_b - b0);
    const int base = A.startb[b0];
    const int span = min(A.startb[b0 + nb - 1] + A.taps_b - base, A.span_b);   // the plan's bound: never past the LDS rows
    const int taps_a = A.taps_a, taps_b = A.taps_b;
    if constexpr (ORDER == 0) {
        // T[ra][pos * cn + c]: ra an output row of the tile, pos an unreflected source column
        const int rowlen = span * cn, pitch = A.span_b * cn;
        for (int e = t; e < na * rowlen; e += IMR_THREADS) {
            const int ra = e / rowlen, q = e - ra * rowlen, pos = q / cn, c = q - pos * cn;
            const int x = reflect_dev((long long)base + pos, n_in_b);
            const double *wr = A.wa + (size_t)(a0 + ra) * taps_a;
            const int *ir = A.idxa + (size_t)(a0 + ra) * taps_a;
            const unsigned char *col = A.src + (size_t)x * (size_t)cn + (size_t)c;
            const size_t stride = (size_t)A.src_stride;
            T[ra * pitch + q] = tap_sum(wr, taps_a, [&](int k) { return (double)col[(size_t)ir[k] * stride]; });
        }
        __syncthreads();
        const int outlen = nb * cn;
        for (int e = t; e < na * outlen; e += IMR_THREADS) {
            const int ra = e / outlen, q = e - ra * outlen, ob = q / cn, c = q - ob * cn;
            const int s = A.startb[b0 + ob] - base;
            const double *wr = A.wb + (size_t)(b0 + ob) * taps_b;
            const double *cell = T + ra * pitch + s * cn + c;
            store_out<OUT>(A, a0 + ra, b0 + ob, c, tap_sum(wr, taps_b, [&](int k) { return cell[k * cn]; }));
        }
    } else {
        // T[pos][ra * cn + c]: pos an unreflected source row, ra an output column of the tile
        const int rowlen = na * cn, pitch = A.tile_a * cn;
        for (int e = t; e < span * rowlen; e += IMR_THREADS) {
            const int pos = e / rowlen, q = e - pos * rowlen, ra = q / cn, c = q - ra * cn;
            const int y = reflect_dev((long long)base + pos, n_in_b);
            const double *wr = A.wa + (size_t)(a0 + ra) * taps_a;
            const int *ir = A.idxa + (size_t)(a0 + ra) * taps_a;
            const unsigned char *row = A.src + (size_t)y * (size_t)A.src_stride + (size_t)c;
            T[pos * pitch + q] = tap_sum(wr, taps_a, [&](int k) { return (double)row[(size_t)ir[k] * (size_t)cn]; });
        }
        __syncthreads();
        for (int e = t; e < nb * rowlen; e += IMR_THREADS) {
            const int ob = e / rowlen, q = e - ob * rowlen, ra = q / cn, c = q - ra * cn;
            const int s = A.startb[b0 + ob] - base;
            const double *wr = A.wb + (size_t)(b0 + ob) * taps_b;
            const double *cell = T + s * pitch + q;
            store_out<OUT>(A, b0 + ob, a0 + ra, c, tap_sum(wr, taps_b, [&](int k) { return cell[k * pitch]; }));
        }
    }
}

template <int ORDER>
void launch(sr_ctx *ctx, const ImrArgs &A, unsigned grid, size_t lds, int out_type)
{
    if (out_type == SR_IMRESIZE_U8)
        hipLaunchKernelGGL((k_imresize<ORDER, SR_IMRESIZE_U8>), dim3(grid), dim3(IMR_THREADS), lds, ctx->stream, A);
    else if (out_type == SR_IMRESIZE_F32)
        hipLaunchKernelGGL((k_imresize<ORDER, SR_IMRESIZE_F32>), dim3(grid), dim3(IMR_THREADS), lds, ctx->stream, A);
    else
        hipLaunchKernelGGL((k_imresize<ORDER, SR_IMRESIZE_F64>), dim3(grid), dim3(IMR_THREADS), lds, ctx->stream, A);
}

}  // namespace

extern "C" {

int sr_imresize_u8(sr_ctx *ctx, const uint8_t *d_src, int64_t src_stride, int h, int w, int cn, double scale_y, double scale_x,
                   int antialias, int out_type, void *d_dst, int64_t dst_stride, int dh, int dw)
{
    // every argument check comes before the context (and so the device) is touched
    if (!d_src || !d_dst) return sr_set_error(SR_ERR_INVALID_ARG, "sr_imresize_u8: null argument");
    if (out_type != SR_IMRESIZE_U8 && out_type != SR_IMRESIZE_F32 && out_type != SR_IMRESIZE_F64)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_imresize_u8: unknown out_type %d", out_type);
    ImrAxis ay, ax;
    ImrPlan p;
    int rc = imr_plan("sr_imresize_u8", h, w, cn, scale_y, scale_x, dh, dw, antialias, &ay, &ax, &p);
    if (rc) return rc;
    const int64_t elem = out_type == SR_IMRESIZE_U8 ? 1 : out_type == SR_IMRESIZE_F32 ? 4 : 8;
    if (src_stride < (int64_t)w * cn) return sr_set_error(SR_ERR_SHAPE, "sr_imresize_u8: source stride smaller than a row");
    if (dst_stride < (int64_t)dw * cn * elem) return sr_set_error(SR_ERR_SHAPE, "sr_imresize_u8: destination stride smaller than a row");
    if ((uintptr_t)d_dst % (uintptr_t)elem || dst_stride % elem)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_imresize_u8: the destination and its stride must be multiples of %d bytes", (int)elem);
    CTX_ENTER(ctx);
    // both axes' tables in one cached device table: one upload per call, none when the geometry repeats
    std::vector<char> blob(p.total, 0);
    const ImrAxis *axes[2] = {&ay, &ax};
    for (int s = 0; s < 2; ++s) {
        memcpy(blob.data() + p.off_w[s], axes[s]->w.data(), axes[s]->w.size() * sizeof(double));
        memcpy(blob.data() + p.off_idx[s], axes[s]->idx.data(), axes[s]->idx.size() * sizeof(int32_t));
        memcpy(blob.data() + p.off_start[s], axes[s]->start.data(), axes[s]->start.size() * sizeof(int32_t));
    }
    SRCHK(upload_cached(ctx, ctx->imresize_tab, blob.data(), blob.size()));
    const char *tab = ctx->imresize_tab.buf.as<const char>();
    const int sa = p.order == 0 ? 0 : 1, sb = 1 - sa;                  // which table feeds which pass
    ImrArgs A;
    A.src = d_src;
    A.src_stride = (long long)src_stride;
    A.h = h;
    A.w = w;
    A.cn = cn;
    A.dst = d_dst;
    A.dst_stride = (long long)dst_stride;
    A.dh = dh;
    A.dw = dw;
    A.wa = (const double *)(tab + p.off_w[sa]);
    A.idxa = (const int *)(tab + p.off_idx[sa]);
    A.taps_a = axes[sa]->taps;
    A.wb = (const double *)(tab + p.off_w[sb]);
    A.startb = (const int *)(tab + p.off_start[sb]);
    A.taps_b = axes[sb]->taps;
    A.tile_a = p.tile_a;
    A.tile_b = p.tile_b;
    A.span_b = p.span_b;
    A.tiles_b = (int)p.tiles_b;
    {
        ProfScope ps(ctx, "imresize");
        const unsigned grid = (unsigned)(p.tiles_a * p.tiles_b);
        if (p.order == 0) launch<0>(ctx, A, grid, p.lds_bytes, out_type);
        else launch<1>(ctx, A, grid, p.lds_bytes, out_type);
    }
    rc = check_launch("imresize");
    if (rc) return rc;
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // extern "C"
