// sr_lpips.hip -- LPIPS (quality_assessment_module.py:419-465 calculate_lpips, :197-224 _to_lpips_tensor) on gfx950.
//
// The reference delegates to the third-party package `lpips` (>= 0.1.4, requirements.txt:16): AlexNet / VGG16 feature
// stacks, unit-normalised channel vectors, squared difference, learned 1x1 `lin` weights, spatial mean, sum over five
// taps.  This is the one dense contraction of the tile -> blend -> assess path, so -- unlike everything in
// sr_engine.hip and sr_assess.hip -- it runs on the matrix cores: every convolution with Cin >= 64 is an implicit GEMM on
// v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate: the reference's arithmetic is torch fp32, there is no reduced
// precision anywhere).  The two 3-channel stem convolutions are a direct VALU kernel that also applies the u8 -> [-1, 1]
// -> ScalingLayer preprocessing, so the fp32 input tensor is never materialised.
//
// Memory: activations are planar fp32 [C][rows][pitch].  A 200 MP image does not fit (relu1_1 alone is 51 GB per
// image), so the image is streamed in square tiles of the INPUT; each tile recomputes the receptive-field halo its
// outputs need (90 px for VGG16), and zero padding is applied per layer at the true image border only, so every
// feature value equals the untiled forward's.  Per tap layer a tile contributes the sum over its own (disjoint)
// part of the feature map; the sums are fp64 and deterministic (fixed block order).
//
// Weights are caller-supplied (sr_lpips_create); nothing is fetched.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_vgg_stream.h"

namespace {

// The stem table of LPIPS: ((u8 / 255) * 2 - 1 - shift_c) / scale_c, the ScalingLayer output, in these fp32 operations.
struct LpipsTable {
    float sh0, sh1, sh2, sc0, sc1, sc2;
    __device__ float operator()(int c, int v) const
    {
        const float t = (float)v / 255.0f;
        const float u = t * 2.0f - 1.0f;
        const float sh = c == 0 ? sh0 : (c == 1 ? sh1 : sh2), sc = c == 0 ? sc0 : (c == 1 ? sc1 : sc2);
        return (u - sh) / sc;
    }
};

// MaxPool2d(K, S), no padding, floor mode: every window lies inside the input range by construction.
template <int K, int S>
__global__ __launch_bounds__(256) void k_lp_pool(const float *__restrict__ in, long long in_plane, int in_pitch, int in_ya,
                                                 int in_xa, float *__restrict__ out, long long out_plane, int out_pitch,
                                                 int out_ya, int out_xa, int rows, int cols)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, c = blockIdx.z;
    if (x >= cols || y >= rows) return;
    const float *p = in + (size_t)c * in_plane + (size_t)((out_ya + y) * S - in_ya) * in_pitch + ((out_xa + x) * S - in_xa);
    float m = p[0];
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int i = 0; i < K; ++i) m = fmaxf(m, p[(size_t)j * in_pitch + i]);
    out[(size_t)c * out_plane + (size_t)y * out_pitch + x] = m;
}

// One LPIPS tap over the tile's own part of the feature map: per pixel
//   sum_c lin_c * (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2        (normalize_tensor, lpips.py)
// in fp32 like the package, summed over pixels in fp64 -> one partial per block.
__global__ __launch_bounds__(256) void k_lp_tap(const float *__restrict__ fa, const float *__restrict__ fb, long long plane,
                                                int pitch, int C, const float *__restrict__ lin, int y0, int x0, int rows,
                                                int cols, double *__restrict__ part)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    double v = 0.0;
    if (x < cols && y < rows) {
        const size_t o = (size_t)(y0 + y) * pitch + (x0 + x);
        float sa = 0.0f, sb = 0.0f;
        for (int c = 0; c < C; ++c) {
            const float a = fa[(size_t)c * plane + o], b = fb[(size_t)c * plane + o];
            sa += a * a;
            sb += b * b;
        }
        const float na = sqrtf(sa) + 1e-10f, nb = sqrtf(sb) + 1e-10f;
        float s = 0.0f;
        for (int c = 0; c < C; ++c) {
            const float a = fa[(size_t)c * plane + o] / na, b = fb[(size_t)c * plane + o] / nb;
            const float d = a - b;
            s += lin[c] * (d * d);
        }
        v = (double)s;
    }
    v = lp_wave_sum(v);
    __shared__ double ws[4];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    if ((tid & 63) == 0) ws[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

}  // namespace

struct sr_lpips_model {
    sr_ctx *ctx = nullptr;
    int net = 0;
    std::vector<LpLayer> layers;
    std::vector<DevBuf> d_w, d_b;     // per convolution: weights in the kernel's layout, bias
    std::vector<DevBuf> d_lin;        // per tap
    int tap_c[5] = {0, 0, 0, 0, 0};
    float shift[3], scale[3];
    DevBuf buf[2][2];                 // [image][ping-pong] activation buffers
    DevBuf d_acc;                     // 5 layer sums
    DevBuf d_part;                    // per-block partials of one tap launch
    void release_device()
    {
        for (auto *v : {&d_w, &d_b, &d_lin})
            for (auto &p : *v) p.release();
        for (auto &im : buf)
            for (auto &p : im) p.release();
        d_acc.release();
        d_part.release();
    }
};

static LiveSet g_lp_live;

extern "C" {

int sr_lpips_create(sr_ctx *ctx, int net, const float *const *h_conv_w, const float *const *h_conv_b, int n_conv,
                    const float *const *h_lin_w, int n_lin, const float *h_shift, const float *h_scale,
                    sr_lpips_model **out)
{
    CTX_ENTER(ctx);
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_lpips_create: null out");
    *out = nullptr;
    if (net != SR_LPIPS_ALEX && net != SR_LPIPS_VGG) return sr_set_error(SR_ERR_INVALID_ARG, "sr_lpips_create: net must be SR_LPIPS_ALEX or SR_LPIPS_VGG");
    sr_lpips_model *M = new sr_lpips_model();
    M->ctx = ctx;
    M->net = net;
    lp_arch(net == SR_LPIPS_ALEX, M->layers);
    int want_conv = 0;
    for (auto &l : M->layers) want_conv += l.kind == LP_CONV;
    if (!h_conv_w || !h_conv_b || !h_lin_w || n_conv != want_conv || n_lin != 5) {
        delete M;
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_lpips_create: net %d needs %d convolutions and 5 lin layers", net, want_conv);
    }
    const float def_shift[3] = {-0.030f, -0.088f, -0.188f}, def_scale[3] = {0.458f, 0.448f, 0.450f};
    for (int c = 0; c < 3; ++c) {
        M->shift[c] = h_shift ? h_shift[c] : def_shift[c];
        M->scale[c] = h_scale ? h_scale[c] : def_scale[c];
    }
    g_lp_live.insert(M);
    auto drop = [&](int rc) {                               // the error is set
        sr_lpips_destroy(M);
        return rc;
    };
    auto fail = [&](int code, const char *what) { return drop(sr_set_error(code, "sr_lpips_create: %s", what)); };
    int tapc = 3, ti = 0;
    for (auto &l : M->layers) {
        if (l.kind == LP_CONV) tapc = l.cout;
        if (l.kind == LP_TAP) M->tap_c[ti++] = tapc;
    }
    for (auto &l : M->layers) {
        if (l.kind != LP_CONV) continue;
        const float *w = h_conv_w[l.widx], *b = h_conv_b[l.widx];
        if (!w || !b) return fail(SR_ERR_INVALID_ARG, "null weight array");
        const int T = l.k * l.k;
        std::vector<float> arranged;
        if (l.cin == 3) {                                   // stem: [c][tap][cout]
            if (l.cout != 64) return fail(SR_ERR_UNSUPPORTED, "stem convolution must have 64 outputs");
            arranged.resize((size_t)l.cout * l.cin * T);
            for (int co = 0; co < l.cout; ++co)
                for (int c = 0; c < 3; ++c)
                    for (int t = 0; t < T; ++t) arranged[((size_t)c * T + t) * 64 + co] = w[((size_t)co * 3 + c) * T + t];
        } else {                                            // MFMA: [cout tile][chunk][c in chunk][tap][64]
            const int CC = l.k == 3 ? 8 : 4;
            if (l.cout % 64 || l.cin % CC || l.s != 1 || (l.k != 3 && l.k != 5) || l.p != l.k / 2)
                return fail(SR_ERR_UNSUPPORTED, "convolution shape outside the MFMA kernel's cases");
            arranged = arrange_mfma_weights(w, b, l.cout, l.cin, T, CC, 64).w;     // cout % 64 == 0: the bias needs no padding
        }
        int rc;
        if ((rc = upload_floats(ctx, "sr_lpips_create: weights", arranged.data(), arranged.size(), M->d_w)) ||
            (rc = upload_floats(ctx, "sr_lpips_create: bias", b, (size_t)l.cout, M->d_b)))
            return drop(rc);
    }
    for (int i = 0; i < 5; ++i) {
        if (!h_lin_w[i]) return fail(SR_ERR_INVALID_ARG, "null lin array");
        if (int rc = upload_floats(ctx, "sr_lpips_create: lin", h_lin_w[i], (size_t)M->tap_c[i], M->d_lin)) return drop(rc);
    }
    if (int rc = M->d_acc.reserve(ctx, "sr_lpips_create: accumulators", 5 * sizeof(double))) return drop(rc);
    *out = M;
    return SR_OK;
}

int sr_lpips_destroy(sr_lpips_model *m)
{
    if (!m) return SR_OK;
    if (!g_lp_live.erase(m)) return SR_OK;
    if (ctx_is_live(m->ctx)) {
        Guard g(m->ctx);
        (void)hipStreamSynchronize(m->ctx->stream);
        m->release_device();
    }
    delete m;
    return SR_OK;
}

int sr_lpips_layer_sizes(int net, int h, int w, int *h_hw)
{
    if (!h_hw || (net != SR_LPIPS_ALEX && net != SR_LPIPS_VGG)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_lpips_layer_sizes: bad arguments");
    std::vector<LpLayer> L;
    lp_arch(net == SR_LPIPS_ALEX, L);
    LpGeom G;
    if (h < 1 || w < 1 || !lp_geometry(L, h, w, G)) return sr_set_error(SR_ERR_SHAPE, "sr_lpips: %dx%d image is too small for the network", w, h);
    for (size_t li = 0; li < L.size(); ++li)
        if (L[li].kind == LP_TAP) {
            h_hw[2 * L[li].tap] = G.H[G.act_of_layer[li]];
            h_hw[2 * L[li].tap + 1] = G.W[G.act_of_layer[li]];
        }
    return SR_OK;
}

int sr_lpips_tile_count(int h, int w, int tile, int *n_tiles)
{
    if (!n_tiles || h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_lpips_tile_count: bad arguments");
    if (tile <= 0) { *n_tiles = 1; return SR_OK; }
    if (tile % 16) return sr_set_error(SR_ERR_INVALID_ARG, "sr_lpips: tile size must be a multiple of 16 (the networks' total stride)");
    *n_tiles = ((h + tile - 1) / tile) * ((w + tile - 1) / tile);
    return SR_OK;
}

int sr_lpips_tile_plan(int net, int h, int w, int tile, int tile_index, int *n_act, int *h_plan, int64_t *buffer_floats)
{
    if (!n_act || !h_plan || !buffer_floats || (net != SR_LPIPS_ALEX && net != SR_LPIPS_VGG))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_lpips_tile_plan: bad arguments");
    int ntiles = 0;
    int rc = sr_lpips_tile_count(h, w, tile, &ntiles);
    if (rc) return rc;
    if (tile_index < 0 || tile_index >= ntiles) return sr_set_error(SR_ERR_INVALID_ARG, "sr_lpips_tile_plan: tile %d of %d", tile_index, ntiles);
    std::vector<LpLayer> L;
    lp_arch(net == SR_LPIPS_ALEX, L);
    LpGeom G;
    if (!lp_geometry(L, h, w, G)) return sr_set_error(SR_ERR_SHAPE, "sr_lpips: %dx%d image is too small for the network", w, h);
    static_assert(LP_PLAN_FIELDS == SR_LPIPS_PLAN_FIELDS, "plan record layout");
    long long floats = 0;
    lp_plan_records(L, G, tile, tile_index, n_act, h_plan, &floats);      // 8 (AlexNet) or 18 (VGG16) activations
    *buffer_floats = (int64_t)floats;
    return SR_OK;
}

int sr_lpips_u8(sr_lpips_model *m, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h,
                int w, int cn, int tile, int tile_begin, int tile_end, double *h_layer_sums)
{
    if (!g_lp_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_lpips_u8: null or destroyed model");
    sr_ctx *ctx = m->ctx;
    CTX_ENTER(ctx);
    if (!d_a || !d_b || !h_layer_sums) return sr_set_error(SR_ERR_INVALID_ARG, "sr_lpips_u8: null argument");
    if (cn != 1 && cn != 3 && cn != 4) return sr_set_error(SR_ERR_INVALID_ARG, "sr_lpips_u8: 1, 3 or 4 channels");
    if (stride_a < (int64_t)w * cn || stride_b < (int64_t)w * cn) return sr_set_error(SR_ERR_SHAPE, "sr_lpips_u8: stride smaller than a row");
    int ntiles = 0;
    int rc = sr_lpips_tile_count(h, w, tile, &ntiles);
    if (rc) return rc;
    LpGeom G;
    if (!lp_geometry(m->layers, h, w, G)) return sr_set_error(SR_ERR_SHAPE, "sr_lpips_u8: %dx%d image is too small for the network", w, h);
    int tiles_x, tiles_y;
    lp_tile_grid(h, w, tile, tiles_x, tiles_y);
    ntiles = tiles_x * tiles_y;
    if (tile_end < 0 || tile_end > ntiles) tile_end = ntiles;
    tile_begin = std::max(tile_begin, 0);
    HIPCHK(hipMemsetAsync(m->d_acc.d, 0, 5 * sizeof(double), ctx->stream));
    const std::vector<LpLayer> &L = m->layers;
    const dim3 blk(64, 4);
    for (int ti = tile_begin; ti < tile_end; ++ti) {
        // ranges and buffer geometry per activation (activation 0 is read from the image itself): sr_lpips_tile_plan's
        LpPlan P;
        lp_plan(L, G, tile, ti, P);
        const std::vector<Range> &ny = P.ny, &oy = P.oy, &nx = P.nx, &ox = P.ox;
        const std::vector<int> &pitch = P.pitch;
        const std::vector<long long> &plane = P.plane;
        rc = ensure_activation_buffers(ctx, &m->buf[0][0], 4, P.need_floats, "sr_lpips_u8");
        if (rc) return rc;
        int cur = 0;                       // ping-pong index of the current activation (both images in step)
        for (size_t li = 0; li < L.size(); ++li) {
            const LpLayer &l = L[li];
            const int ai = G.act_of_layer[li];
            if (l.kind == LP_TAP) {
                const Range ry = oy[ai], rx = ox[ai];
                if (ry.empty() || rx.empty()) continue;
                const dim3 grid((rx.n() + 63) / 64, (ry.n() + 3) / 4);
                const size_t nblk = (size_t)grid.x * grid.y;
                SRCHK(m->d_part.reserve(ctx, "sr_lpips_u8", nblk * sizeof(double)));
                ProfScope ps(ctx, "lpips_tap");
                hipLaunchKernelGGL(k_lp_tap, grid, blk, 0, ctx->stream, m->buf[0][cur].as<float>(), m->buf[1][cur].as<float>(), plane[ai], pitch[ai],
                                   G.C[ai], m->d_lin[l.tap].as<const float>(), ry.a - ny[ai].a, rx.a - nx[ai].a, ry.n(), rx.n(), m->d_part.as<double>());
                hipLaunchKernelGGL(k_lp_accum, dim3(1), dim3(256), 0, ctx->stream, m->d_part.as<double>(), (long long)nblk, m->d_acc.as<double>() + l.tap);
                continue;
            }
            const int ao = ai + 1;
            const int rows = ny[ao].n(), cols = nx[ao].n();
            if (rows <= 0 || cols <= 0) { cur ^= (ai > 0); continue; }
            const int nxt = ai == 0 ? 0 : cur ^ 1;
            for (int im = 0; im < 2; ++im) {
                const float *src = ai == 0 ? nullptr : m->buf[im][cur].as<float>();
                float *dst = m->buf[im][nxt].as<float>();
                if (l.kind == LP_POOL) {
                    ProfScope ps(ctx, "lpips_pool");
                    const dim3 grid((cols + 63) / 64, (rows + 3) / 4, G.C[ao]);
                    if (l.k == 2) hipLaunchKernelGGL((k_lp_pool<2, 2>), grid, blk, 0, ctx->stream, src, plane[ai], pitch[ai], ny[ai].a, nx[ai].a, dst, plane[ao], pitch[ao], ny[ao].a, nx[ao].a, rows, cols);
                    else hipLaunchKernelGGL((k_lp_pool<3, 2>), grid, blk, 0, ctx->stream, src, plane[ai], pitch[ai], ny[ai].a, nx[ai].a, dst, plane[ao], pitch[ao], ny[ao].a, nx[ao].a, rows, cols);
                } else if (ai == 0) {
                    ProfScope ps(ctx, "lpips_conv_stem");
                    const uint8_t *img = im == 0 ? d_a : d_b;
                    const long long st = im == 0 ? stride_a : stride_b;
                    const dim3 grid((cols + 63) / 64, (rows + 3) / 4);
                    const LpipsTable tab{m->shift[0], m->shift[1], m->shift[2], m->scale[0], m->scale[1], m->scale[2]};
#define STEM_ARGS img, st, cn, h, w, m->d_w[l.widx].as<const float>(), m->d_b[l.widx].as<const float>(), tab, dst, ny[ao].a, nx[ao].a, rows, cols, pitch[ao], plane[ao]
                    if (l.k == 3) hipLaunchKernelGGL((k_lp_conv_stem<3, 1, 1, LpipsTable>), grid, blk, 0, ctx->stream, STEM_ARGS);
                    else hipLaunchKernelGGL((k_lp_conv_stem<11, 4, 2, LpipsTable>), grid, blk, 0, ctx->stream, STEM_ARGS);
#undef STEM_ARGS
                } else {
                    ProfScope ps(ctx, "lpips_conv_mfma");
                    const dim3 grid((cols + 31) / 32, (rows + 7) / 8, l.cout / 64);
#define CONV_ARGS src, plane[ai], pitch[ai], ny[ai].a, nx[ai].a, ny[ai].n(), nx[ai].n(), G.H[ai], G.W[ai], l.cin, m->d_w[l.widx].as<const float>(), m->d_b[l.widx].as<const float>(), dst, \
                  plane[ao], pitch[ao], ny[ao].a, nx[ao].a, rows, cols
                    if (l.k == 3) hipLaunchKernelGGL((k_lp_conv_mfma<3, 8>), grid, dim3(256), 0, ctx->stream, CONV_ARGS);
                    else hipLaunchKernelGGL((k_lp_conv_mfma<5, 4>), grid, dim3(256), 0, ctx->stream, CONV_ARGS);
#undef CONV_ARGS
                }
            }
            cur = nxt;
        }
        rc = check_launch("lpips");
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(h_layer_sums, m->d_acc.d, 5 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // extern "C"
