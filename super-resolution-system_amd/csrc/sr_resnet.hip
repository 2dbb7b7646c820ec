// sr_resnet.hip -- local super-resolution backend: the classic residual family (BasicSR's MSRResNet = SRResNet without batch
// norm, and EDSR baseline / large) on gfx950.
//
//   head        3 x 3 convolution 3 -> F from the u8 image, x[c] = (u8 / 255 - mean[c]) * range, slope a_head   -> h
//   blocks      B x { t' = relu(conv1(t));  t = fmaf(res_scale, conv2(t'), t) }
//   long skip   t = conv_after_body(t) + h                                                  (EDSR)
//   upsampling  per stage: 3 x 3 convolution F -> F r^2, PixelShuffle(r) into planar fp32 at r x the resolution, slope a_up
//   HR conv     3 x 3 convolution F -> F at full resolution, slope a_hr                      (MSRResNet)
//   last conv   3 x 3 convolution F -> 3 at full resolution, o[c] = y[c] / range + mean[c] (+ the bilinear base), HWC store
//
// Everything is fp32 (fp32 in, fp32 accumulate).  Every F-input convolution is one implicit-GEMM kernel on
// v_mfma_f32_32x32x2_f32 (the mainloop of sr_conv_mfma.h, shared with sr_lpips.hip, sr_srnet.hip and sr_rrdb.hip), templated on
// its epilogue; the 3 -> F head is the direct VALU kernel of k_sn_head with the input affine added.  What the three SR backends
// share around the mainloop -- the head frame, leaky / skip_offset / store_hwc, the backward extent rule, the planar tensor, the
// convolution launch, the models' lifetime -- is sr_net_common.h; this file holds the network's own kernels and epilogues,
// its op list, its tile policy and its layer walk.
//
// Memory: activations are planar fp32 [F][rows][pitch] in three buffers owned by the model (in, out, and the skip / h).  The
// image is walked in square sub-tiles of the INPUT.  Every layer's extent is derived backwards from the sub-tile's output
// rectangle: grown by one per convolution, divided by r (rounded outwards) across a shuffle, clipped to the layer's image;
// zero padding is applied at the true image border only, so every value equals the unstreamed forward's.  A block's output
// overwrites its skip in place (each thread reads exactly the element it then writes) unless that skip is the h a long skip
// still needs.
//
// Determinism: the summation orders are those of sr_conv_mfma.h (conv_mfma_mainloop, head_accumulate); a skip add is one fmaf
// after the chain.  The order does not depend on where the output lies in a block or a sub-tile.
//
// Weights are caller-supplied (sr_resnet_create); nothing is fetched.
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_net_common.h"

namespace {

constexpr size_t RN_WORKSPACE_CAP = (size_t)1 << 30;   // tile = 0: the largest sub-tile whose three buffers stay under 1 GiB
constexpr int RN_MAX_TILE = 2048, RN_TILE_STEP = 32;

// ---------------------------------------------------------------------------------------------------------------
// Head (3 -> F) from the u8 image: k_sn_head with the input affine and one scalar slope.  One thread = one output pixel x
// 64 output channels (blockIdx.z: 64-cout tile).  x[c] = (u8 / 255 - mean[c]) * range inside the image, 0 outside (zero is
// padded after the affine); the 3 x 256 values are tabulated in LDS with exactly that fp32 arithmetic.
// ---------------------------------------------------------------------------------------------------------------
struct RnAffine {
    float mean[3];
    float range;
};

__global__ __launch_bounds__(256) void k_rn_head(const unsigned char *__restrict__ img, long long stride, int H, int W,
                                                 const float *__restrict__ wt, const float *__restrict__ bias, float slope,
                                                 RnAffine af, float *__restrict__ out, int ya, int xa, int rows, int cols,
                                                 int pitch, long long plane)
{
    __shared__ float lut[3][256];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    {
        const float v = (float)tid / 255.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) lut[c][tid] = (v - af.mean[c]) * af.range;
    }
    __syncthreads();
    head_frame<256>(img, stride, H, W, wt, bias, &lut[0][0], out, ya, xa, rows, cols, pitch, plane, [&](int, float y) { return leaky(y, slope); });
}

// The epilogues of k_rn_conv.
enum { RN_SLOPE = 0, RN_SKIP = 1, RN_SHUF2 = 2, RN_SHUF3 = 3, RN_LAST_F32 = 4, RN_LAST_U8 = 5 };

// What an epilogue needs beside the convolution's own arguments.
struct RnEpi {
    float slope;                   // RN_SLOPE, RN_SHUF*: y >= 0 ? y : slope * y
    float res_scale;               // RN_SKIP: fmaf(res_scale, y, skip)
    const float *skip;             // RN_SKIP: planar, element (c, gy, gx) at skip[c * skip_plane + (gy - skip_ya) * skip_pitch + gx - skip_xa]
    long long skip_plane;          //          (may be the output buffer itself: a thread reads the element it then writes)
    int skip_pitch, skip_ya, skip_xa;
    // RN_LAST_*
    const unsigned char *img;      // u8 source of the bilinear base, h x w x 3
    long long img_stride;
    int h, w, bilinear;
    float rscale;                  // (float)(1.0 / s): the base's source coordinate is rscale * (Y + 0.5) - 0.5, clamped at 0
    RnAffine af;
    void *dst;                     // HWC output, u8 or fp32
    long long dst_stride;          // bytes
};

// One channel of the bilinear base (torch's align_corners=False arithmetic, written out in include/sr_hip.h).
__device__ __forceinline__ float rn_bilinear(const unsigned char *r0, const unsigned char *r1, int x0, int x1, int c, float ly0, float ly1,
                                             float lx0, float lx1)
{
    const float p00 = (float)r0[(size_t)x0 * 3 + c] / 255.0f, p01 = (float)r0[(size_t)x1 * 3 + c] / 255.0f;
    const float p10 = (float)r1[(size_t)x0 * 3 + c] / 255.0f, p11 = (float)r1[(size_t)x1 * 3 + c] / 255.0f;
    return ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11);
}

// ---------------------------------------------------------------------------------------------------------------
// 3 x 3 implicit-GEMM convolution on v_mfma_f32_32x32x2_f32, stride 1, zero padding 1 at the image border.
//   conv_mfma_mainloop<3, 8, NC2, true> (sr_conv_mfma.h) plus an epilogue; NC2 = 32-cout halves per block (2, the last
//   convolution 1).
//   RN_SLOPE     slope, planar store
//   RN_SKIP      fmaf(res_scale, y, skip), planar store
//   RN_SHUF2/3   couts F r^2 in tiles of 64; cout co goes to channel co / r^2 at (r row + (co % r^2) / r, r col + co % r) of
//                the planar output at r x the resolution (origin r out_ya, r out_xa), then slope
//   RN_LAST_*    the 3 couts zero-padded to 32; output affine, optional bilinear base, HWC store (u8: clamp, scale, round half
//                even); out_ya / out_xa are then coordinates in the full-resolution image
// ---------------------------------------------------------------------------------------------------------------
template <int NC2, int EPI>
__global__ __launch_bounds__(256) void k_rn_conv(const float *__restrict__ in, long long in_plane, int in_pitch, int in_ya, int in_xa,
                                                 int in_rows, int in_cols, int H_in, int W_in, int cin, const float *__restrict__ wslab,
                                                 const float *__restrict__ bias, float *out, long long out_plane, int out_pitch,
                                                 int out_ya, int out_xa, int rows, int cols, RnEpi ep)
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
        if constexpr (EPI == RN_SLOPE) {
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    const float y = acc[c2][pr][r];
                    out[(size_t)co * out_plane + (size_t)row * out_pitch + col] = leaky(y, ep.slope);
                }
        } else if constexpr (EPI == RN_SKIP) {
            const size_t so = skip_offset(out_ya + row, out_xa + col, ep.skip_ya, ep.skip_xa, ep.skip_pitch);
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    const float sk = ep.skip[(size_t)co * ep.skip_plane + so];
                    out[(size_t)co * out_plane + (size_t)row * out_pitch + col] = fmaf(ep.res_scale, acc[c2][pr][r], sk);
                }
        } else if constexpr (EPI == RN_SHUF2 || EPI == RN_SHUF3) {
            constexpr int R = EPI == RN_SHUF2 ? 2 : 3;
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    const int c = co / (R * R), rem = co % (R * R), dy = rem / R, dx = rem % R;
                    const float y = acc[c2][pr][r];
                    out[(size_t)c * out_plane + ((size_t)row * R + dy) * out_pitch + (size_t)col * R + dx] = leaky(y, ep.slope);
                }
        } else {                                           // output affine + bilinear base + HWC store
            if (half != 0) continue;                       // couts 0 .. 2 live in registers 0 .. 2 of the lower half-wave
            const int gy = out_ya + row, gx = out_xa + col;
            float base[3] = {0.0f, 0.0f, 0.0f};
            if (ep.bilinear) {
                const float sy = fmaxf(ep.rscale * ((float)gy + 0.5f) - 0.5f, 0.0f), sx = fmaxf(ep.rscale * ((float)gx + 0.5f) - 0.5f, 0.0f);
                const int y0 = min((int)sy, ep.h - 1), x0 = min((int)sx, ep.w - 1);
                const int y1 = y0 + (y0 < ep.h - 1 ? 1 : 0), x1 = x0 + (x0 < ep.w - 1 ? 1 : 0);
                const float ly1 = sy - (float)y0, lx1 = sx - (float)x0, ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
                const unsigned char *r0 = ep.img + (size_t)y0 * ep.img_stride, *r1 = ep.img + (size_t)y1 * ep.img_stride;
#pragma unroll
                for (int c = 0; c < 3; ++c) base[c] = rn_bilinear(r0, r1, x0, x1, c, ly0, ly1, lx0, lx1);
            }
            char *d = (char *)ep.dst + (size_t)gy * ep.dst_stride;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float o = acc[0][pr][c] / ep.af.range + ep.af.mean[c];
                if (ep.bilinear) o = o + base[c];
                store_hwc<EPI == RN_LAST_U8>(d, (size_t)gx * 3 + c, o);
            }
        }
    }
}

// One convolution of the network, in forward order.
struct RnOp {
    int kind;          // OP_* below
    int r;             // shuffle factor of an upsampling stage, else 1
    int lvl;           // resolution level of the convolution itself: 0 = input, 1 / 2 = after the first / second shuffle
    float slope;
    int skip;          // 0 none, 1 the block's input, 2 h (the long skip)
};
enum { OP_HEAD = 0, OP_CONV = 1, OP_SKIP = 2, OP_UP = 3, OP_LAST = 4 };

int rn_check_desc(const char *who, const sr_resnet_desc *d)
{
    if (!d) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null description", who);
    const int F = d->n_feat;
    if ((F != 64 && F != 128 && F != 192 && F != 256) || d->n_blocks < 0 || d->n_blocks > 64 || d->scale < 1 || d->scale > 4)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d features, %d residual blocks, scale %d is outside F in {64, 128, 192, 256}, "
                            "0 <= B <= 64, 1 <= s <= 4", who, F, d->n_blocks, d->scale);
    if ((d->long_skip | d->conv_hr | d->bilinear_base) & ~1)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: long_skip, conv_hr and bilinear_base are 0 or 1", who);
    const float v[] = {d->a_head, d->a_up, d->a_hr, d->res_scale, d->mean[0], d->mean[1], d->mean[2], d->range};
    for (float x : v)
        if (!std::isfinite(x)) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: slopes, res_scale, mean and range must be finite", who);
    if (d->range == 0.0f) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: range must not be 0", who);
    return SR_OK;
}

// head, (conv1, conv2) x B, [conv_after_body], upsampling stages, [conv_hr], conv_last
std::vector<RnOp> rn_build_ops(const sr_resnet_desc &d)
{
    std::vector<RnOp> ops;
    ops.push_back({OP_HEAD, 1, 0, d.a_head, 0});
    for (int i = 0; i < d.n_blocks; ++i) {
        ops.push_back({OP_CONV, 1, 0, 0.0f, 0});
        ops.push_back({OP_SKIP, 1, 0, 1.0f, 1});
    }
    if (d.long_skip) ops.push_back({OP_SKIP, 1, 0, 1.0f, 2});
    int lvl = 0;
    if (d.scale == 4) {
        ops.push_back({OP_UP, 2, lvl++, d.a_up, 0});
        ops.push_back({OP_UP, 2, lvl++, d.a_up, 0});
    } else if (d.scale > 1) {
        ops.push_back({OP_UP, d.scale, lvl++, d.a_up, 0});
    }
    if (d.conv_hr) ops.push_back({OP_CONV, 1, lvl, d.a_hr, 0});
    ops.push_back({OP_LAST, 1, lvl, 1.0f, 0});
    return ops;
}

// Resolution multiplier of a level for this scale.
int rn_mult(int scale, int lvl) { return lvl == 0 ? 1 : (scale == 4 ? (lvl == 1 ? 2 : 4) : scale); }

// The extent rule's view of the ops (backward_extents, backward_halo: sr_net_common.h).
std::vector<ExtStep> rn_steps(const std::vector<RnOp> &ops, int scale)
{
    std::vector<ExtStep> steps;
    for (const RnOp &op : ops) steps.push_back({op.r, rn_mult(scale, op.lvl)});
    return steps;
}

struct RnGeom {
    int tile = 0, tiles_x = 0, tiles_y = 0, halo = 0;
    long long plane = 0;              // largest planar activation (rows x pitch) any layer of any sub-tile stores
};

// Host only: sub-tile grid and buffer geometry of an h x w input.
int rn_geometry(const char *who, const sr_resnet_desc &d, const std::vector<RnOp> &ops, int h, int w, int tile, RnGeom &g)
{
    const int s = d.scale, rc = check_sr_geometry(who, h, w, s, tile < 0, "tile");
    if (rc) return rc;
    const std::vector<ExtStep> steps = rn_steps(ops, s);
    g.halo = backward_halo(steps.data(), (int)steps.size());
    if (tile == 0) {                  // the largest multiple of 32 whose three F (s (tile + 2 halo))^2 buffers fit the cap
        tile = RN_TILE_STEP;
        for (int t = RN_MAX_TILE; t > RN_TILE_STEP; t -= RN_TILE_STEP) {
            const size_t side = (size_t)s * (t + 2 * g.halo);
            if (3 * (size_t)d.n_feat * side * side * sizeof(float) <= RN_WORKSPACE_CAP) {
                tile = t;
                break;
            }
        }
    }
    g.tile = tile;
    g.tiles_x = (w + tile - 1) / tile;
    g.tiles_y = (h + tile - 1) / tile;
    // the extents of an axis depend on that axis alone: per layer, the tallest and the widest sub-tile make its largest plane
    const size_t n = ops.size();
    std::vector<long long> rows(n, 0), pitch(n, 0);
    std::vector<int> a, b;
    for (int ty = 0; ty < g.tiles_y; ++ty) {
        backward_extents(steps.data(), (int)n, s, ty * tile, (int)std::min<long long>((long long)ty * tile + tile, h), h, a, b);
        for (size_t i = 0; i < n; ++i) rows[i] = std::max(rows[i], (long long)(b[i] - a[i]) * ops[i].r);
    }
    for (int tx = 0; tx < g.tiles_x; ++tx) {
        backward_extents(steps.data(), (int)n, s, tx * tile, (int)std::min<long long>((long long)tx * tile + tile, w), w, a, b);
        for (size_t i = 0; i < n; ++i) pitch[i] = std::max(pitch[i], pad4((long long)(b[i] - a[i]) * ops[i].r));
    }
    g.plane = 0;
    for (size_t i = 0; i + 1 < n; ++i) g.plane = std::max(g.plane, rows[i] * pitch[i]);     // the last convolution stores no plane
    if (g.plane * 8 > INT_MAX)        // the convolution indexes one 8-channel chunk of a buffer with 32-bit offsets
        return sr_set_error(SR_ERR_SHAPE, "%s: a sub-tile of %lld activations per channel is too large; use a smaller tile", who, g.plane);
    return SR_OK;
}

// A planar tensor held in buffer buf of the model.
struct RnTen : PlanarTen {
    int buf = -1;
};

}  // namespace

struct sr_resnet_model : SrModelBase {         // d_w, d_b: per op
    sr_resnet_desc d{};
    std::vector<RnOp> ops;
    DevBuf buf[3];
    void release_device()
    {
        for (auto &b : buf) b.release();
        release_base();
    }
};

static LiveSet g_rn_live;

static int rn_forward(sr_resnet_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride,
                      int tile, bool u8, const char *who)
{
    if (!g_rn_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    sr_ctx *ctx = m->ctx;
    CTX_ENTER(ctx);
    const int F = m->d.n_feat, S = m->d.scale;
    int rc = check_sr_forward_args(who, d_src, src_stride, w, d_dst, dst_stride, S, u8);
    if (rc) return rc;
    RnGeom g;
    rc = rn_geometry(who, m->d, m->ops, h, w, tile, g);
    if (rc) return rc;
    rc = ensure_activation_buffers(ctx, m->buf, 3, (size_t)g.plane * F, who);
    if (rc) return rc;
    const std::vector<RnOp> &ops = m->ops;
    const size_t n = ops.size();
    const std::vector<ExtStep> steps = rn_steps(ops, S);
    const RnAffine af = {{m->d.mean[0], m->d.mean[1], m->d.mean[2]}, m->d.range};
    RnEpi ep0{};
    ep0.slope = 1.0f;
    ep0.res_scale = 1.0f;
    ep0.img = d_src;
    ep0.img_stride = (long long)src_stride;
    ep0.h = h;
    ep0.w = w;
    ep0.bilinear = m->d.bilinear_base;
    ep0.rscale = (float)(1.0 / S);
    ep0.af = af;
    ep0.dst = d_dst;
    ep0.dst_stride = (long long)dst_stride;
    std::vector<std::vector<int>> ya(g.tiles_y), yb(g.tiles_y), xa(g.tiles_x), xb(g.tiles_x);
    for (int ty = 0; ty < g.tiles_y; ++ty) backward_extents(steps.data(), (int)n, S, ty * g.tile, (int)std::min<long long>((long long)ty * g.tile + g.tile, h), h, ya[ty], yb[ty]);
    for (int tx = 0; tx < g.tiles_x; ++tx) backward_extents(steps.data(), (int)n, S, tx * g.tile, (int)std::min<long long>((long long)tx * g.tile + g.tile, w), w, xa[tx], xb[tx]);
    auto other = [](int x, int y) {                        // a buffer that is neither x nor y
        for (int i = 0; i < 3; ++i)
            if (i != x && i != y) return i;
        return 0;
    };
    for (int ty = 0; ty < g.tiles_y; ++ty)
        for (int tx = 0; tx < g.tiles_x; ++tx) {
            RnTen t, hten;                                 // the running activation; h while a long skip still needs it
            int h_buf = -1;
            RnTen blk;                                     // the input of the current residual block
            for (size_t i = 0; i < n; ++i) {
                const RnOp &op = ops[i];
                const int oya = ya[ty][i], oxa = xa[tx][i], rows = yb[ty][i] - oya, cols = xb[tx][i] - oxa;
                const int mult = rn_mult(S, op.lvl), H_in = h * mult, W_in = w * mult;
                // where a freshly laid out result goes: r x the convolution's own extent
                auto fresh = [&](int b) {
                    RnTen o;
                    static_cast<PlanarTen &>(o) = planar_tensor(m->buf[b].as<float>(), oya * op.r, oxa * op.r, rows * op.r, cols * op.r);
                    o.buf = b;
                    return o;
                };
                RnEpi ep = ep0;
                ep.slope = op.slope;
                if (op.kind == OP_HEAD) {
                    ProfScope ps(ctx, "resnet_head");
                    t = fresh(0);
                    hipLaunchKernelGGL(k_rn_head, dim3((cols + 63) / 64, (rows + 3) / 4, F / 64), dim3(64, 4), 0, ctx->stream, d_src,
                                       (long long)src_stride, h, w, m->w(i), m->b(i), op.slope, af, t.p, oya, oxa, rows, cols, t.pitch,
                                       t.plane);
                    if (m->d.long_skip) {
                        hten = t;
                        h_buf = t.buf;
                    }
                    blk = t;
                } else if (op.kind == OP_CONV) {
                    ProfScope ps(ctx, op.lvl == 0 ? "resnet_body" : "resnet_hr");
                    blk = t;                               // a block's first convolution: its input is the block's skip
                    RnTen o = fresh(other(t.buf, h_buf));
                    launch_conv(k_rn_conv<2, RN_SLOPE>, ctx->stream, t, H_in, W_in, F, F / 64, m->w(i), m->b(i), o.p, o.plane, o.pitch, oya, oxa, rows,
                                           cols, ep);
                    t = o;
                } else if (op.kind == OP_SKIP) {
                    ProfScope ps(ctx, "resnet_body");
                    const RnTen &sk = op.skip == 2 ? hten : blk;
                    RnTen o;
                    if (op.skip == 2 || sk.buf == h_buf) {
                        o = fresh(other(t.buf, h_buf));    // h stays whole for the long skip (or is read here for the last time)
                    } else {                               // in place over the skip: the sub-rectangle of its layout
                        o = sk;
                        o.p = sk.p + (size_t)(oya - sk.ya) * sk.pitch + (oxa - sk.xa);
                        o.ya = oya; o.xa = oxa; o.rows = rows; o.cols = cols;
                    }
                    ep.res_scale = op.skip == 2 ? 1.0f : m->d.res_scale;
                    ep.skip = sk.p;
                    ep.skip_plane = sk.plane;
                    ep.skip_pitch = sk.pitch;
                    ep.skip_ya = sk.ya;
                    ep.skip_xa = sk.xa;
                    launch_conv(k_rn_conv<2, RN_SKIP>, ctx->stream, t, H_in, W_in, F, F / 64, m->w(i), m->b(i), o.p, o.plane, o.pitch, oya, oxa, rows,
                                          cols, ep);
                    t = o;
                    if (op.skip == 2) h_buf = -1;
                } else if (op.kind == OP_UP) {
                    ProfScope ps(ctx, "resnet_up");
                    RnTen o = fresh(other(t.buf, -1));
                    if (op.r == 2)
                        launch_conv(k_rn_conv<2, RN_SHUF2>, ctx->stream, t, H_in, W_in, F, F * 4 / 64, m->w(i), m->b(i), o.p, o.plane, o.pitch, oya, oxa,
                                               rows, cols, ep);
                    else
                        launch_conv(k_rn_conv<2, RN_SHUF3>, ctx->stream, t, H_in, W_in, F, F * 9 / 64, m->w(i), m->b(i), o.p, o.plane, o.pitch, oya, oxa,
                                               rows, cols, ep);
                    t = o;
                } else {
                    ProfScope ps(ctx, "resnet_last");
                    if (u8)
                        launch_conv(k_rn_conv<1, RN_LAST_U8>, ctx->stream, t, H_in, W_in, F, 1, m->w(i), m->b(i), nullptr, 0LL, 0, oya, oxa, rows, cols, ep);
                    else
                        launch_conv(k_rn_conv<1, RN_LAST_F32>, ctx->stream, t, H_in, W_in, F, 1, m->w(i), m->b(i), nullptr, 0LL, 0, oya, oxa, rows, cols, ep);
                }
            }
            rc = check_launch(who);
            if (rc) return rc;
        }
    return SR_OK;
}

// The self-ensemble over rn_forward (driver: sr_ensemble.hip).
static int rn_ensemble(sr_resnet_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride, int tile,
                       int mask, bool u8, const char *who)
{
    const int rc = sr_ens_check_mask(who, mask);
    if (rc) return rc;
    if (tile < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: %s must be >= 1, or 0 for the library's choice", who, "tile");
    if (!g_rn_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    return ens_run(who, *m, m->d.scale, [&](const uint8_t *s, int64_t ss, int hh, int ww, float *d, int64_t ds) {
        return rn_forward(m, s, ss, hh, ww, d, ds, tile, false, who);
    }, d_src, src_stride, h, w, d_dst, dst_stride, mask, u8);
}

extern "C" {

int sr_resnet_create(sr_ctx *ctx, const sr_resnet_desc *desc, const float *const *h_w, const float *const *h_b, int n_conv,
                     sr_resnet_model **out)
{
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_resnet_create: null out");
    *out = nullptr;
    int rc = rn_check_desc("sr_resnet_create", desc);                       // host decision, before any device call
    if (rc) return rc;
    std::vector<RnOp> ops = rn_build_ops(*desc);
    if ((rc = check_weight_tables("sr_resnet_create", "convolution", (int)ops.size(), n_conv, h_w, h_b))) return rc;
    CTX_ENTER(ctx);
    sr_resnet_model *M = new sr_resnet_model();
    M->ctx = ctx;
    M->d = *desc;
    M->ops = ops;
    g_rn_live.insert(M);
    const int F = desc->n_feat;
    for (int k = 0; k < n_conv; ++k) {
        const bool last = ops[k].kind == OP_LAST;
        MfmaWeights a;
        if (ops[k].kind == OP_HEAD) a = {arrange_head_weights(h_w[k], F), std::vector<float>(h_b[k], h_b[k] + F)};
        else a = arrange_mfma_weights(h_w[k], h_b[k], last ? 3 : F * ops[k].r * ops[k].r, F, 9, 8, last ? 32 : 64);
        if ((rc = upload_conv("sr_resnet_create", *M, a))) {
            sr_resnet_destroy(M);
            return rc;
        }
    }
    *out = M;
    return SR_OK;
}

int sr_resnet_destroy(sr_resnet_model *m)
{
    return destroy_model(m, g_rn_live);
}

int sr_resnet_plan(const sr_resnet_desc *desc, int h, int w, int tile, int *halo, int *n_tiles, size_t *workspace_bytes)
{
    int rc = rn_check_desc("sr_resnet_plan", desc);
    if (rc) return rc;
    RnGeom g;
    rc = rn_geometry("sr_resnet_plan", *desc, rn_build_ops(*desc), h, w, tile, g);
    if (rc) return rc;
    if (halo) *halo = g.halo;
    if (n_tiles) *n_tiles = g.tiles_x * g.tiles_y;
    if (workspace_bytes) *workspace_bytes = (size_t)3 * desc->n_feat * (size_t)g.plane * sizeof(float);
    return SR_OK;
}

int sr_resnet_u8(sr_resnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride,
                 int tile)
{
    return rn_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tile, true, "sr_resnet_u8");
}

int sr_resnet_f32(sr_resnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride,
                  int tile)
{
    return rn_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tile, false, "sr_resnet_f32");
}

int sr_resnet_ens_u8(sr_resnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride,
                     int tile, int mask)
{
    return rn_ensemble(model, d_src, src_stride, h, w, d_dst, dst_stride, tile, mask, true, "sr_resnet_ens_u8");
}

int sr_resnet_ens_f32(sr_resnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride,
                      int tile, int mask)
{
    return rn_ensemble(model, d_src, src_stride, h, w, d_dst, dst_stride, tile, mask, false, "sr_resnet_ens_f32");
}

}  // extern "C"
