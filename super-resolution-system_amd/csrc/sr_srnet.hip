// sr_srnet.hip -- local super-resolution backend: the compact "VGG-style" SR network (the family Real-ESRGAN ships as
// SRVGGNetCompact) on gfx950.  Stage 2 of the reference is a remote API client; this is the pipeline's own learned upscaler.
//
//   layer 0        3 x 3 convolution 3 -> F straight from the u8 image (x = u8 / 255), per-channel slope activation
//   layers 1 .. D  3 x 3 convolutions F -> F, per-channel slope activation          (y >= 0 ? y : a[c] * y)
//   layer D + 1    3 x 3 convolution F -> 3 s^2, no activation, fused with PixelShuffle(s), the nearest-upsampled input
//                  (one fp32 add) and the store: HWC fp32 unclamped, or HWC u8 rintf(clamp(o, 0, 1) * 255)
//
// Everything is fp32 (fp32 in, fp32 accumulate): the F -> F and F -> 3 s^2 layers are implicit GEMMs on
// v_mfma_f32_32x32x2_f32 (the mainloop of sr_conv_mfma.h, shared with sr_lpips.hip, sr_resnet.hip and sr_rrdb.hip), the 3 -> F
// head is a direct VALU kernel.  The 3 s^2-channel tensor is never written.  What the three SR backends share around the
// mainloop -- the head frame, store_hwc, the backward extent rule, the models' lifetime -- is sr_net_common.h; this file holds the
// network's own kernels and epilogues, its geometry policy and its layer walk.
//
// Memory: activations are planar fp32 [F][rows][pitch] in two ping-pong buffers owned by the model.  The image is walked in
// square sub-tiles of the INPUT; a sub-tile recomputes a halo of D + 2 input pixels (layer k's valid extent is the sub-tile
// grown by D + 1 - k, clipped to the image), and zero padding is applied per layer at the true image border only, so every
// value equals the unstreamed forward's.
//
// Determinism: the summation orders are those of sr_conv_mfma.h (conv_mfma_mainloop, head_accumulate); neither depends on
// where the output lies in a block or a sub-tile: streamed and unstreamed results are bit-equal.
//
// Weights are caller-supplied (sr_srnet_create); nothing is fetched.
#include <cstring>
#include <vector>

#include "sr_net_common.h"

namespace {

constexpr int SN_DEFAULT_TILE = 2048;      // tile = 0: one pipeline tile is one sub-tile (no halo recompute)

// The per-channel activation.  Not leaky(y, slope[co]): the slope is loaded for negative values only, as it always was -- an
// unconditional load costs the body kernel 40 VGPRs and a wave per SIMD.
__device__ __forceinline__ float sn_act(float y, const float *__restrict__ slope, int co) { return y >= 0.0f ? y : slope[co] * y; }

// ---------------------------------------------------------------------------------------------------------------
// Head (3 -> F) from the u8 image: one thread = one output pixel x 64 output channels (blockIdx.z: 64-cout tile).
// x = u8 / 255 (tabulated in LDS with exactly that fp32 division) through head_accumulate, then the per-channel slope.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sn_head(const unsigned char *__restrict__ img, long long stride, int H, int W,
                                                 const float *__restrict__ wt, const float *__restrict__ bias,
                                                 const float *__restrict__ slope, float *__restrict__ out, int ya, int xa,
                                                 int rows, int cols, int pitch, long long plane)
{
    __shared__ float lut[256];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    lut[tid] = (float)tid / 255.0f;
    __syncthreads();
    slope += (int)blockIdx.z * 64;
    head_frame<0>(img, stride, H, W, wt, bias, lut, out, ya, xa, rows, cols, pitch, plane, [&](int co, float y) { return sn_act(y, slope, co); });
}

// What the fused tail needs beside the convolution's own arguments.
struct SnTail {
    const unsigned char *img;      // u8 source (the nearest-upsampled base)
    long long img_stride;
    void *dst;                     // HWC output, u8 or fp32
    long long dst_stride;          // bytes
};

// ---------------------------------------------------------------------------------------------------------------
// 3 x 3 implicit-GEMM convolution on v_mfma_f32_32x32x2_f32, stride 1, zero padding 1 at the image border.
//   conv_mfma_mainloop<3, 8, NC2, true> (sr_conv_mfma.h) plus an epilogue; NC2 = 32-cout halves per block.
//   S == 0: body layer, NC2 = 2, epilogue = per-channel slope, planar store.
//   S >= 1: tail layer, couts 3 S^2 zero-padded to 32 NC2; epilogue = pixel shuffle + base add + HWC store (U8: clamp,
//           scale, round half even).  out_ya / out_xa are then the sub-tile's own origin in the image.
// ---------------------------------------------------------------------------------------------------------------
template <int NC2, int S, bool U8>
__global__ __launch_bounds__(256) void k_sn_conv(const float *__restrict__ in, long long in_plane, int in_pitch, int in_ya,
                                                 int in_xa, int in_rows, int in_cols, int H_in, int W_in, int cin, const float *__restrict__ wslab,
                                                 const float *__restrict__ bias, const float *__restrict__ slope,
                                                 float *__restrict__ out, long long out_plane, int out_pitch, int out_ya,
                                                 int out_xa, int rows, int cols, SnTail tail)
{
    constexpr int NC = NC2 * 32;
    const MfmaLane ln = mfma_lane();
    const int half = ln.half, ct = ln.ct;
    f32x16 acc[NC2][2];
    conv_mfma_mainloop<3, 8, NC2, true>(ln, in, in_plane, in_pitch, in_ya, in_xa, in_rows, in_cols, H_in, W_in, cin, wslab, bias, out_ya,
                                        out_xa, acc);
    const int col = ln.ox0 + ln.l32;
    if (col >= cols) return;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        const int row = ln.oy0 + 2 * ln.wave + pr;
        if (row >= rows) continue;
        if constexpr (S == 0) {                            // slope activation, planar store
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    const float y = acc[c2][pr][r];
                    out[(size_t)co * out_plane + (size_t)row * out_pitch + col] = sn_act(y, slope, co);
                }
        } else {                                           // pixel shuffle + nearest base + HWC store
            const int gy = out_ya + row, gx = out_xa + col;
            const unsigned char *px = tail.img + (size_t)gy * tail.img_stride + (size_t)gx * 3;
            const float x0 = (float)px[0] / 255.0f, x1 = (float)px[1] / 255.0f, x2 = (float)px[2] / 255.0f;
            char *drow = (char *)tail.dst + (size_t)gy * S * tail.dst_stride;
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = mfma_cout(c2, r, half);
                    if (co >= 3 * S * S) continue;
                    const int c = co / (S * S), rem = co % (S * S), dy = rem / S, dx = rem % S;
                    const float o = acc[c2][pr][r] + (c == 0 ? x0 : (c == 1 ? x1 : x2));
                    const size_t e = ((size_t)gx * S + dx) * 3 + c;
                    store_hwc<U8>(drow + (size_t)dy * tail.dst_stride, e, o);
                }
        }
    }
}

struct SnGeom {
    int tile = 0, tiles_x = 0, tiles_y = 0, halo = 0;
    int rows = 0, pitch = 0;          // activation buffer of the padded sub-tile
    long long plane = 0;
};

int sn_check_arch(const char *who, int n_feat, int n_body, int scale)
{
    if ((n_feat != 64 && n_feat != 128 && n_feat != 192 && n_feat != 256) || n_body < 0 || n_body > 64 || scale < 1 || scale > 4)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d features, %d body convolutions, scale %d is outside F in {64, 128, 192, 256}, "
                            "0 <= D <= 64, 1 <= s <= 4", who, n_feat, n_body, scale);
    return SR_OK;
}

// The extent rule's view of the D + 2 convolutions: no replication, one resolution (layer k's valid extent is the sub-tile grown
// by D + 1 - k, clipped to the image).
std::vector<ExtStep> sn_steps(int n_body) { return std::vector<ExtStep>(n_body + 2, ExtStep{1, 1}); }

// Host only: sub-tile grid and buffer geometry of an h x w input.
int sn_geometry(const char *who, int h, int w, int n_body, int scale, int tile, SnGeom &g)
{
    const int rc = check_sr_geometry(who, h, w, scale, tile < 0, "tile");
    if (rc) return rc;
    g.tile = tile == 0 ? SN_DEFAULT_TILE : tile;
    g.halo = backward_halo(sn_steps(n_body).data(), n_body + 2);
    g.tiles_x = (w + g.tile - 1) / g.tile;
    g.tiles_y = (h + g.tile - 1) / g.tile;
    g.rows = (int)std::min<long long>((long long)std::min(g.tile, h) + 2 * g.halo, h);
    const int cols = (int)std::min<long long>((long long)std::min(g.tile, w) + 2 * g.halo, w);
    g.pitch = (int)pad4(cols);
    g.plane = (long long)g.rows * g.pitch;
    if (g.plane * 8 > INT_MAX)        // the convolution indexes one 8-channel chunk of a buffer with 32-bit offsets
        return sr_set_error(SR_ERR_SHAPE, "%s: a sub-tile of %d x %d activations is too large; use a smaller tile", who, g.pitch, g.rows);
    return SR_OK;
}

}  // namespace

struct sr_srnet_model : SrModelBase {
    int F = 0, D = 0, S = 0;
    std::vector<DevBuf> d_slope;              // per layer 0 .. D (d_w, d_b: 0 .. D + 1; no slope for the tail)
    DevBuf buf[2];                            // ping-pong activation buffers
    void release_device()
    {
        for (auto &p : d_slope) p.release();
        for (auto &b : buf) b.release();
        release_base();
    }
};

static LiveSet g_sn_live;

template <int S, bool U8>
static void sn_launch_tail(dim3 grid, hipStream_t st, const float *src, long long plane, int pitch, int in_ya, int in_xa, int in_rows,
                           int in_cols, int h, int w, int F, const float *dw, const float *db, int ya, int xa, int rows, int cols, SnTail tail)
{
    constexpr int NC2 = 3 * S * S > 32 ? 2 : 1;
    hipLaunchKernelGGL((k_sn_conv<NC2, S, U8>), grid, dim3(256), 0, st, src, plane, pitch, in_ya, in_xa, in_rows, in_cols, h, w, F, dw, db,
                       (const float *)nullptr, (float *)nullptr, 0LL, 0, ya, xa, rows, cols, tail);
}

static int sn_forward(sr_srnet_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride,
                      int tile, bool u8, const char *who)
{
    if (!g_sn_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    sr_ctx *ctx = m->ctx;
    CTX_ENTER(ctx);
    const int F = m->F, D = m->D, S = m->S;
    int rc = check_sr_forward_args(who, d_src, src_stride, w, d_dst, dst_stride, S, u8);
    if (rc) return rc;
    SnGeom g;
    rc = sn_geometry(who, h, w, D, S, tile, g);
    if (rc) return rc;
    rc = ensure_activation_buffers(ctx, m->buf, 2, (size_t)g.plane * F, who);
    if (rc) return rc;
    const SnTail tail = {d_src, (long long)src_stride, d_dst, (long long)dst_stride};
    const std::vector<ExtStep> steps = sn_steps(D);
    std::vector<int> ea, eb, fa, fb;                       // per layer: rows [ea, eb), columns [fa, fb)
    for (int ty = 0; ty < g.tiles_y; ++ty)
        for (int tx = 0; tx < g.tiles_x; ++tx) {
            const int y0 = ty * g.tile, y1 = std::min(y0 + g.tile, h), x0 = tx * g.tile, x1 = std::min(x0 + g.tile, w);
            backward_extents(steps.data(), D + 2, 1, y0, y1, h, ea, eb);
            backward_extents(steps.data(), D + 2, 1, x0, x1, w, fa, fb);
            int ya, xa, rows, cols;
            auto ext = [&](int k) { ya = ea[k]; xa = fa[k]; rows = eb[k] - ya; cols = fb[k] - xa; };
            ext(0);
            const int pitch = (int)pad4(cols);
            const long long plane = (long long)rows * pitch;      // <= g.plane: one geometry for every layer of the sub-tile
            int cur = 0;
            {
                ProfScope ps(ctx, "srnet_head");
                hipLaunchKernelGGL(k_sn_head, dim3((cols + 63) / 64, (rows + 3) / 4, F / 64), dim3(64, 4), 0, ctx->stream, d_src,
                                   (long long)src_stride, h, w, m->w(0), m->b(0), m->d_slope[0].as<const float>(), m->buf[0].as<float>(), ya, xa, rows,
                                   cols, pitch, plane);
            }
            int in_ya = ya, in_xa = xa, in_rows = rows, in_cols = cols;
            for (int k = 1; k <= D; ++k) {
                ext(k);
                ProfScope ps(ctx, "srnet_body");
                hipLaunchKernelGGL((k_sn_conv<2, 0, false>), dim3((cols + 31) / 32, (rows + 7) / 8, F / 64), dim3(256), 0, ctx->stream,
                                   m->buf[cur].as<float>(), plane, pitch, in_ya, in_xa, in_rows, in_cols, h, w, F, m->w(k), m->b(k), m->d_slope[k].as<const float>(),
                                   m->buf[cur ^ 1].as<float>(), plane, pitch, ya, xa, rows, cols, SnTail{nullptr, 0, nullptr, 0});
                cur ^= 1;
                in_ya = ya; in_xa = xa; in_rows = rows; in_cols = cols;
            }
            ext(D + 1);
            {
                ProfScope ps(ctx, "srnet_tail");
                const dim3 grid((cols + 31) / 32, (rows + 7) / 8, 1);
                using TailFn = decltype(&sn_launch_tail<1, false>);
                static const TailFn launch[4][2] = {{sn_launch_tail<1, false>, sn_launch_tail<1, true>},
                                                    {sn_launch_tail<2, false>, sn_launch_tail<2, true>},
                                                    {sn_launch_tail<3, false>, sn_launch_tail<3, true>},
                                                    {sn_launch_tail<4, false>, sn_launch_tail<4, true>}};
                launch[S - 1][u8 ? 1 : 0](grid, ctx->stream, m->buf[cur].as<float>(), plane, pitch, in_ya, in_xa, in_rows, in_cols, h, w, F, m->w(D + 1),
                                  m->b(D + 1), ya, xa, rows, cols, tail);
            }
            rc = check_launch(who);
            if (rc) return rc;
        }
    return SR_OK;
}

// The self-ensemble over sn_forward (driver: sr_ensemble.hip).
static int sn_ensemble(sr_srnet_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride, int tile,
                       int mask, bool u8, const char *who)
{
    const int rc = sr_ens_check_mask(who, mask);
    if (rc) return rc;
    if (tile < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: %s must be >= 1, or 0 for the library's choice", who, "tile");
    if (!g_sn_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    return ens_run(who, *m, m->S, [&](const uint8_t *s, int64_t ss, int hh, int ww, float *d, int64_t ds) {
        return sn_forward(m, s, ss, hh, ww, d, ds, tile, false, who);
    }, d_src, src_stride, h, w, d_dst, dst_stride, mask, u8);
}

extern "C" {

int sr_srnet_create(sr_ctx *ctx, int n_feat, int n_body, int scale, const float *const *h_w, const float *const *h_b,
                    const float *const *h_slope, sr_srnet_model **out)
{
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_srnet_create: null out");
    *out = nullptr;
    int rc = sn_check_arch("sr_srnet_create", n_feat, n_body, scale);       // host decision, before any device call
    if (rc) return rc;
    const int F = n_feat, D = n_body, S = scale, nl = D + 2;
    if ((rc = check_weight_tables("sr_srnet_create", "layer", nl, nl, h_w, h_b, h_slope, D + 1))) return rc;
    CTX_ENTER(ctx);
    sr_srnet_model *M = new sr_srnet_model();
    M->ctx = ctx;
    M->F = F; M->D = D; M->S = S;
    g_sn_live.insert(M);
    const int tail_c = 3 * S * S, tail_nc = tail_c > 32 ? 64 : 32;
    for (int k = 0; k < nl; ++k) {
        MfmaWeights a;
        if (k == 0) a = {arrange_head_weights(h_w[k], F), std::vector<float>(h_b[k], h_b[k] + F)};
        else a = arrange_mfma_weights(h_w[k], h_b[k], k <= D ? F : tail_c, F, 9, 8, k <= D ? 64 : tail_nc);
        rc = upload_conv("sr_srnet_create", *M, a);
        if (!rc && k <= D) rc = upload_floats(ctx, "sr_srnet_create", h_slope[k], F, M->d_slope);
        if (rc) {
            sr_srnet_destroy(M);
            return rc;
        }
    }
    *out = M;
    return SR_OK;
}

int sr_srnet_destroy(sr_srnet_model *m)
{
    return destroy_model(m, g_sn_live);
}

int sr_srnet_plan(int h, int w, int n_feat, int n_body, int scale, int tile, int *halo, int *n_tiles, size_t *workspace_bytes)
{
    int rc = sn_check_arch("sr_srnet_plan", n_feat, n_body, scale);
    if (rc) return rc;
    SnGeom g;
    rc = sn_geometry("sr_srnet_plan", h, w, n_body, scale, tile, g);
    if (rc) return rc;
    if (halo) *halo = g.halo;
    if (n_tiles) *n_tiles = g.tiles_x * g.tiles_y;
    if (workspace_bytes) *workspace_bytes = (size_t)2 * n_feat * (size_t)g.plane * sizeof(float);
    return SR_OK;
}

int sr_srnet_u8(sr_srnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride,
                int tile)
{
    return sn_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tile, true, "sr_srnet_u8");
}

int sr_srnet_f32(sr_srnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride,
                 int tile)
{
    return sn_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tile, false, "sr_srnet_f32");
}

int sr_srnet_ens_u8(sr_srnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride,
                    int tile, int mask)
{
    return sn_ensemble(model, d_src, src_stride, h, w, d_dst, dst_stride, tile, mask, true, "sr_srnet_ens_u8");
}

int sr_srnet_ens_f32(sr_srnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride,
                     int tile, int mask)
{
    return sn_ensemble(model, d_src, src_stride, h, w, d_dst, dst_stride, tile, mask, false, "sr_srnet_ens_f32");
}

}  // extern "C"
