// sr_dists.hip -- DISTS (Ding, Ma, Wang, Simoncelli 2020: deep image structure and texture similarity) on gfx950.
//
// The feature stack is torchvision VGG16's thirteen convolutions with an L2 (Hann) pooling in place of every max pooling;
// the metric compares, per channel of the image and of the five stage outputs, the global mean, variance and covariance of
// the two images' feature maps.  The convolutions, the tile streaming (halo recomputed per tile, zero padding at the true
// image border only) and the fixed-order fp64 sums are sr_lpips.hip's, shared through sr_vgg_stream.h; what is new here is
// two bandwidth kernels (the pooling and the five per-channel sums) and the stem's input table (ImageNet mean / std).
// The score itself is host arithmetic on 1475 x 5 sums (sr_dists_host.cpp).  The definition is in include/sr_hip.h.
//
// Weights are caller-supplied (sr_dists_create); nothing is fetched.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_vgg_stream.h"

namespace {

constexpr int DS_STAGES = 6;
constexpr int DS_TOTAL = 1475;                    // 3 + 64 + 128 + 256 + 512 + 512
constexpr int DS_BR = 32;                         // rows of the own rectangle one k_ds_stats block covers (x 64 columns)

// The stem table of DISTS: (u8 / 255 - mean_c) / std_c in these fp32 operations.
struct DistsTable {
    float m0, m1, m2, s0, s1, s2;
    __device__ float operator()(int c, int v) const
    {
        const float x = (float)v / 255.0f;
        const float mu = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
        return (x - mu) / sd;
    }
};

// L2 pooling: y(Y, X) = sqrtf(sum_{j,i} g_j g_i x(2Y - 1 + j, 2X - 1 + i)^2 + 1e-12f), g = (1/4, 1/2, 1/4), all fp32: x * x
// rounded once, the nine terms (each an exact product by a power of two) added in row-major tap order onto 0, then the
// epsilon, then a correctly rounded square root.  (Y, X) are global indices of the output activation; taps outside the true
// extent H_in x W_in of the input activation are the layer's zero padding -- inside a tiled forward the buffer holds real
// neighbour data there, which is read.
__global__ __launch_bounds__(256) void k_ds_l2pool(const float *__restrict__ in, long long in_plane, int in_pitch, int in_ya,
                                                   int in_xa, int H_in, int W_in, float *__restrict__ out, long long out_plane,
                                                   int out_pitch, int out_ya, int out_xa, int rows, int cols)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, c = blockIdx.z;
    if (x >= cols || y >= rows) return;
    const float *p = in + (size_t)c * in_plane;
    const int gy0 = (out_ya + y) * 2 - 1, gx0 = (out_xa + x) * 2 - 1;
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int gy = gy0 + j;
        const bool yok = gy >= 0 && gy < H_in;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int gx = gx0 + i;
            float v = 0.0f;
            if (yok && gx >= 0 && gx < W_in) v = p[(size_t)(gy - in_ya) * in_pitch + (gx - in_xa)];
            const float g = (j == 1 ? 0.5f : 0.25f) * (i == 1 ? 0.5f : 0.25f);
            s += g * (v * v);
        }
    }
    out[(size_t)c * out_plane + (size_t)y * out_pitch + x] = sqrtf(s + 1e-12f);
}

// Five block sums -> part[(5 c + k) * nblk + blk]: wave reduction, then the four waves in ascending order.
__device__ __forceinline__ void ds_block_out(double (&v)[5], int c, double *__restrict__ part)
{
    __shared__ double ws[4][5];
    const int tid = threadIdx.y * 64 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        v[k] = lp_wave_sum(v[k]);
        if ((tid & 63) == 0) ws[tid >> 6][k] = v[k];
    }
    __syncthreads();
    if (tid < 5) {
        const size_t nblk = (size_t)gridDim.x * gridDim.y, blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        part[((size_t)c * 5 + tid) * nblk + blk] = ((ws[0][tid] + ws[1][tid]) + ws[2][tid]) + ws[3][tid];
    }
}

// The five sums (a, b, a^2, b^2, a b) of one channel (grid z) over the tile's own rectangle [y0, y0 + rows) x [x0, x0 + cols)
// of a tapped activation of both images: fp32 values converted to double, products in double.  A block covers 64 columns x
// DS_BR rows; a thread adds its rows in ascending order.  Each plane is read once, rows of 64 consecutive floats per wave.
__global__ __launch_bounds__(256) void k_ds_stats(const float *__restrict__ fa, const float *__restrict__ fb, long long plane,
                                                  int pitch, int y0, int x0, int rows, int cols, double *__restrict__ part)
{
    const int x = blockIdx.x * 64 + threadIdx.x, c = blockIdx.z;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (x < cols) {
        const int yb = blockIdx.y * DS_BR, ye = min(yb + DS_BR, rows);
        for (int y = yb + threadIdx.y; y < ye; y += 4) {
            const size_t o = (size_t)c * plane + (size_t)(y0 + y) * pitch + (x0 + x);
            const double a = (double)fa[o], b = (double)fb[o];
            v[0] += a;
            v[1] += b;
            v[2] += a * a;
            v[3] += b * b;
            v[4] += a * b;
        }
    }
    ds_block_out(v, c, part);
}

// Stage 0: the same five sums of the u8 values of image channel z (gray repeated, alpha dropped) over the tile's own
// rectangle of the image, as 64-bit integers inside a block (a whole-image sum of v^2 stays below 255^2 2^31 < 2^53, so the
// doubles that carry the block sums on are exact integers too: no order matters).
__global__ __launch_bounds__(256) void k_ds_stats_u8(const unsigned char *__restrict__ ia, long long stride_a,
                                                     const unsigned char *__restrict__ ib, long long stride_b, int cn, int y0,
                                                     int x0, int rows, int cols, double *__restrict__ part)
{
    const int x = blockIdx.x * 64 + threadIdx.x, c = blockIdx.z;
    const int cs = cn == 1 ? 0 : c;
    unsigned long long u[5] = {0, 0, 0, 0, 0};
    if (x < cols) {
        const int yb = blockIdx.y * DS_BR, ye = min(yb + DS_BR, rows);
        for (int y = yb + threadIdx.y; y < ye; y += 4) {
            const unsigned a = ia[(size_t)(y0 + y) * stride_a + (size_t)(x0 + x) * cn + cs];
            const unsigned b = ib[(size_t)(y0 + y) * stride_b + (size_t)(x0 + x) * cn + cs];
            u[0] += a;
            u[1] += b;
            u[2] += a * a;
            u[3] += b * b;
            u[4] += a * b;
        }
    }
    double v[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = (double)u[k];       // at most 8 x 255^2 per thread
    ds_block_out(v, c, part);
}

}  // namespace

struct sr_dists_model {
    sr_ctx *ctx = nullptr;
    std::vector<LpLayer> layers;
    std::vector<DevBuf> d_w, d_b;     // per convolution: weights in the kernel's layout, bias
    float mean[3], stdv[3];
    DevBuf buf[2][2];                 // [image][ping-pong] activation buffers
    DevBuf d_acc;                     // 1475 x 5 sums
    DevBuf d_part;                    // per-block partials of one stats launch
    void release_device()
    {
        for (auto *v : {&d_w, &d_b})
            for (auto &p : *v) p.release();
        for (auto &im : buf)
            for (auto &p : im) p.release();
        d_acc.release();
        d_part.release();
    }
};

static LiveSet g_ds_live;

static const int DS_CH[DS_STAGES] = {3, 64, 128, 256, 512, 512};

static void ds_launch_l2pool(hipStream_t st, const float *src, long long in_plane, int in_pitch, int in_ya, int in_xa, int H_in,
                             int W_in, float *dst, long long out_plane, int out_pitch, int out_ya, int out_xa, int rows, int cols,
                             int C)
{
    const dim3 grid((cols + 63) / 64, (rows + 3) / 4, C);
    hipLaunchKernelGGL(k_ds_l2pool, grid, dim3(64, 4), 0, st, src, in_plane, in_pitch, in_ya, in_xa, H_in, W_in, dst, out_plane,
                       out_pitch, out_ya, out_xa, rows, cols);
}

extern "C" {

int sr_dists_create(sr_ctx *ctx, const float *const *h_conv_w, const float *const *h_conv_b, const float *h_mean,
                    const float *h_std, sr_dists_model **out)
{
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_create: null out");
    *out = nullptr;
    if (!h_conv_w || !h_conv_b) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_create: null weight tables (13 convolutions)");
    for (int i = 0; i < 13; ++i)
        if (!h_conv_w[i] || !h_conv_b[i]) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_create: null weight array %d", i);
    const float def_mean[3] = {0.485f, 0.456f, 0.406f}, def_std[3] = {0.229f, 0.224f, 0.225f};
    for (int c = 0; c < 3; ++c) {
        const float m = h_mean ? h_mean[c] : def_mean[c], s = h_std ? h_std[c] : def_std[c];
        if (!std::isfinite(m) || !std::isfinite(s) || s == 0.0f) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_create: mean / std must be finite, std non-zero");
    }
    CTX_ENTER(ctx);
    sr_dists_model *M = new sr_dists_model();
    M->ctx = ctx;
    ds_arch(M->layers);
    for (int c = 0; c < 3; ++c) {
        M->mean[c] = h_mean ? h_mean[c] : def_mean[c];
        M->stdv[c] = h_std ? h_std[c] : def_std[c];
    }
    g_ds_live.insert(M);
    auto drop = [&](int rc) {                               // the error is set
        sr_dists_destroy(M);
        return rc;
    };
    for (auto &l : M->layers) {
        if (l.kind != LP_CONV) continue;
        const float *w = h_conv_w[l.widx], *b = h_conv_b[l.widx];
        std::vector<float> arranged;
        if (l.cin == 3) {                                   // stem: [c][tap][cout]
            arranged.resize((size_t)64 * 3 * 9);
            for (int co = 0; co < 64; ++co)
                for (int c = 0; c < 3; ++c)
                    for (int t = 0; t < 9; ++t) arranged[((size_t)c * 9 + t) * 64 + co] = w[((size_t)co * 3 + c) * 9 + t];
        } else {                                            // MFMA: [cout tile][chunk][c in chunk][tap][64]
            arranged = arrange_mfma_weights(w, b, l.cout, l.cin, 9, 8, 64).w;     // cout % 64 == 0: the bias needs no padding
        }
        int rc;
        if ((rc = upload_floats(ctx, "sr_dists_create: weights", arranged.data(), arranged.size(), M->d_w)) ||
            (rc = upload_floats(ctx, "sr_dists_create: bias", b, (size_t)l.cout, M->d_b)))
            return drop(rc);
    }
    if (int rc = M->d_acc.reserve(ctx, "sr_dists_create: accumulators", (size_t)DS_TOTAL * 5 * sizeof(double))) return drop(rc);
    *out = M;
    return SR_OK;
}

int sr_dists_destroy(sr_dists_model *m)
{
    if (!m) return SR_OK;
    if (!g_ds_live.erase(m)) return SR_OK;
    if (ctx_is_live(m->ctx)) {
        Guard g(m->ctx);
        (void)hipStreamSynchronize(m->ctx->stream);
        m->release_device();
    }
    delete m;
    return SR_OK;
}

int sr_dists_tile_count(int h, int w, int tile, int *n_tiles)
{
    if (!n_tiles || h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_tile_count: null output or a side below 1");
    if (tile <= 0) { *n_tiles = 1; return SR_OK; }
    if (tile % 16) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists: tile size must be a multiple of 16 (the network's total stride)");
    *n_tiles = ((h + tile - 1) / tile) * ((w + tile - 1) / tile);
    return SR_OK;
}

int sr_dists_tile_plan(int h, int w, int tile, int tile_index, int *n_act, int *h_plan, int64_t *buffer_floats)
{
    if (!n_act || !h_plan || !buffer_floats) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_tile_plan: null argument");
    int ntiles = 0;
    int rc = sr_dists_tile_count(h, w, tile, &ntiles);
    if (rc) return rc;
    if (tile_index < 0 || tile_index >= ntiles) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_tile_plan: tile %d of %d", tile_index, ntiles);
    std::vector<LpLayer> L;
    ds_arch(L);
    LpGeom G;
    if (!lp_geometry(L, h, w, G)) return sr_set_error(SR_ERR_SHAPE, "sr_dists_tile_plan: no geometry for a %dx%d image", w, h);
    static_assert(LP_PLAN_FIELDS == SR_LPIPS_PLAN_FIELDS, "plan record layout");
    long long floats = 0;
    lp_plan_records(L, G, tile, tile_index, n_act, h_plan, &floats);      // 18 activations
    *buffer_floats = (int64_t)floats;
    return SR_OK;
}

int sr_dists_u8(sr_dists_model *m, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w,
                int cn, int tile, int tile_begin, int tile_end, double *h_sums)
{
    // every refusal before the model is looked at, the model before any device call
    if (!d_a || !d_b || !h_sums) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_u8: null argument");
    if (cn != 1 && cn != 3 && cn != 4) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_u8: 1, 3 or 4 channels");
    int ntiles = 0;
    int rc = sr_dists_tile_count(h, w, tile, &ntiles);
    if (rc) return rc;
    if (stride_a < (int64_t)w * cn || stride_b < (int64_t)w * cn) return sr_set_error(SR_ERR_SHAPE, "sr_dists_u8: stride smaller than a row");
    if (!g_ds_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_u8: null or destroyed model");
    sr_ctx *ctx = m->ctx;
    CTX_ENTER(ctx);
    LpGeom G;
    if (!lp_geometry(m->layers, h, w, G)) return sr_set_error(SR_ERR_SHAPE, "sr_dists_u8: no geometry for a %dx%d image", w, h);
    int tiles_x, tiles_y;
    lp_tile_grid(h, w, tile, tiles_x, tiles_y);
    ntiles = tiles_x * tiles_y;
    if (tile_end < 0 || tile_end > ntiles) tile_end = ntiles;
    tile_begin = std::max(tile_begin, 0);
    HIPCHK(hipMemsetAsync(m->d_acc.d, 0, (size_t)DS_TOTAL * 5 * sizeof(double), ctx->stream));
    const std::vector<LpLayer> &L = m->layers;
    const dim3 blk(64, 4);
    int ch0[DS_STAGES];                       // first channel of a stage in the 1475
    for (int k = 0, c = 0; k < DS_STAGES; c += DS_CH[k], ++k) ch0[k] = c;
    const DistsTable tab{m->mean[0], m->mean[1], m->mean[2], m->stdv[0], m->stdv[1], m->stdv[2]};
    for (int ti = tile_begin; ti < tile_end; ++ti) {
        // ranges and buffer geometry per activation (activation 0 is read from the image itself); the guarded convolution and
        // the pooling read inside the needed range only, so a buffer holds exactly C * plane floats
        LpPlan P;
        lp_plan(L, G, tile, ti, P);
        const std::vector<Range> &ny = P.ny, &oy = P.oy, &nx = P.nx, &ox = P.ox;
        const std::vector<int> &pitch = P.pitch;
        const std::vector<long long> &plane = P.plane;
        rc = ensure_activation_buffers(ctx, &m->buf[0][0], 4, P.need_floats, "sr_dists_u8");
        if (rc) return rc;
        int cur = 0;                       // ping-pong index of the current activation (both images in step)
        for (size_t li = 0; li < L.size(); ++li) {
            const LpLayer &l = L[li];
            const int ai = G.act_of_layer[li];
            if (l.kind == LP_TAP) {
                const Range ry = oy[ai], rx = ox[ai];
                if (ry.empty() || rx.empty()) continue;
                const int C = DS_CH[l.tap];
                const dim3 grid((rx.n() + 63) / 64, (ry.n() + DS_BR - 1) / DS_BR, C);
                const size_t nblk = (size_t)grid.x * grid.y, npart = nblk * C * 5;
                SRCHK(m->d_part.reserve(ctx, "sr_dists_u8", npart * sizeof(double)));
                ProfScope ps(ctx, "dists_stats");
                if (ai == 0)
                    hipLaunchKernelGGL(k_ds_stats_u8, grid, blk, 0, ctx->stream, d_a, (long long)stride_a, d_b, (long long)stride_b, cn,
                                       ry.a, rx.a, ry.n(), rx.n(), m->d_part.as<double>());
                else
                    hipLaunchKernelGGL(k_ds_stats, grid, blk, 0, ctx->stream, m->buf[0][cur].as<float>(), m->buf[1][cur].as<float>(), plane[ai], pitch[ai],
                                       ry.a - ny[ai].a, rx.a - nx[ai].a, ry.n(), rx.n(), m->d_part.as<double>());
                hipLaunchKernelGGL(k_lp_accum, dim3(C * 5), dim3(256), 0, ctx->stream, m->d_part.as<double>(), (long long)nblk,
                                   m->d_acc.as<double>() + (size_t)ch0[l.tap] * 5);
                continue;
            }
            const int ao = ai + 1;
            const int rows = ny[ao].n(), cols = nx[ao].n();
            if (rows <= 0 || cols <= 0) { cur ^= (ai > 0); continue; }
            const int nxt = ai == 0 ? 0 : cur ^ 1;
            for (int im = 0; im < 2; ++im) {
                const float *src = ai == 0 ? nullptr : m->buf[im][cur].as<float>();
                float *dst = m->buf[im][nxt].as<float>();
                if (l.kind == LP_L2POOL) {
                    ProfScope ps(ctx, "dists_l2pool");
                    ds_launch_l2pool(ctx->stream, src, plane[ai], pitch[ai], ny[ai].a, nx[ai].a, G.H[ai], G.W[ai], dst, plane[ao],
                                     pitch[ao], ny[ao].a, nx[ao].a, rows, cols, G.C[ao]);
                } else if (ai == 0) {
                    ProfScope ps(ctx, "dists_conv_stem");
                    const uint8_t *img = im == 0 ? d_a : d_b;
                    const long long st = im == 0 ? stride_a : stride_b;
                    const dim3 grid((cols + 63) / 64, (rows + 3) / 4);
                    hipLaunchKernelGGL((k_lp_conv_stem<3, 1, 1, DistsTable>), grid, blk, 0, ctx->stream, img, st, cn, h, w, m->d_w[l.widx].as<const float>(),
                                       m->d_b[l.widx].as<const float>(), tab, dst, ny[ao].a, nx[ao].a, rows, cols, pitch[ao], plane[ao]);
                } else {
                    ProfScope ps(ctx, "dists_conv_mfma");
                    const dim3 grid((cols + 31) / 32, (rows + 7) / 8, l.cout / 64);
                    hipLaunchKernelGGL((k_lp_conv_mfma<3, 8>), grid, dim3(256), 0, ctx->stream, src, plane[ai], pitch[ai], ny[ai].a,
                                       nx[ai].a, ny[ai].n(), nx[ai].n(), G.H[ai], G.W[ai], l.cin, m->d_w[l.widx].as<const float>(), m->d_b[l.widx].as<const float>(), dst, plane[ao], pitch[ao],
                                       ny[ao].a, nx[ao].a, rows, cols);
                }
            }
            cur = nxt;
        }
        rc = check_launch("dists");
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(h_sums, m->d_acc.d, (size_t)DS_TOTAL * 5 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_dists_l2pool_f32(sr_ctx *ctx, const float *d_in, int C, int H, int W, float *d_out)
{
    if (!d_in || !d_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_l2pool_f32: null argument");
    if (C < 1 || C > 65535 || H < 1 || W < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_l2pool_f32: C in 1 .. 65535, H and W at least 1");
    CTX_ENTER(ctx);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    ds_launch_l2pool(ctx->stream, d_in, (long long)H * W, W, 0, 0, H, W, d_out, (long long)Ho * Wo, Wo, 0, 0, Ho, Wo, C);
    int rc = check_launch("dists_l2pool");
    if (rc) return rc;
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // extern "C"
