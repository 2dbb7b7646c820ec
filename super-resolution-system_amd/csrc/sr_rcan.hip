// sr_rcan.hip -- local super-resolution backend: BasicSR's RCAN (residual channel attention network, Zhang et al. 2018) at
// scales 1 .. 4 on gfx950.
//
//   head        3 x 3 convolution 3 -> F from the u8 image, x[c] = (u8 / 255 - mean[c]) * range, no activation   -> h
//   group x G   t = group input;  RCAB x B;  t = conv(t) + group input
//     RCAB      y1 = relu(conv(t));  y2 = conv(y1);  m[c] = mean of y2[c] over the WHOLE image;
//               s = sigmoid(W2 relu(W1 m + b1) + b2)  (two 1 x 1 convolutions, F -> R -> F);  t = fmaf(res_scale, y2 * s[c], t)
//   long skip   f = conv_after_body(t) + h
//   upsampling  per stage: 3 x 3 convolution F -> F r^2, PixelShuffle(r) into planar fp32 at r x the resolution
//   last conv   3 x 3 convolution F -> 3 at full resolution, o[c] = y[c] / range + mean[c], HWC store
//
// Everything is fp32 (fp32 in, fp32 accumulate) except the channel attention, which is float64 from the fp32 planes.  Every
// F-input 3 x 3 convolution is the implicit-GEMM mainloop of sr_conv_mfma.h (v_mfma_f32_32x32x2_f32, shared with sr_lpips.hip,
// sr_srnet.hip, sr_resnet.hip and sr_rrdb.hip) behind one of the epilogues below; the 3 -> F head is head_accumulate with the
// input affine tabulated.  What the SR backends share around the mainloop is sr_net_common.h.
//
// RCAN is not local: an RCAB's output at one pixel depends on the mean of y2 over every pixel.  So the image is not streamed
// through the trunk; there are two phases.
//   trunk phase  the whole h x w image is ONE piece: head, the G groups, conv_after_body.  FIVE planar fp32 buffers of F planes
//                (rows x columns padded to 4): h (which conv_after_body's add-skip store turns into f in place), the group
//                input, t, y1 and y2.  The first RCAB of a group writes t into a buffer of its own, so that the group input stays
//                whole; the others, and the group convolution's add-skip store over the group input, run in place (a thread reads
//                exactly the element it then writes).  Per RCAB: two convolutions, the row-chunk sums of y2 (k_rc_rowsum), the
//                attention (k_rc_attention, one block) and the scale-and-skip pass (k_rc_scale) -- four kinds of launches on one
//                stream, nothing returns to the host.
//   tail phase   after f nothing is global: the upsampling stages and conv_last run in tail x tail sub-pieces of the input over
//                their backward extents (backward_extents, as sr_rrdb.hip's tail phase), two F-plane ping-pong buffers.
//
// The three kernels of the channel attention (k_rc_rowsum, k_rc_attention, k_rc_scale) are sr_chan_attn.h, shared with
// sr_hat.hip's CAB.
// The channel mean (the order every restatement follows): the image's rows are cut into chunks of RC_ROWS = 32.  One block of
// 256 threads per (channel, chunk): thread t adds, in float64, rows ascending and within a row the columns t, t + 256, ..
// ascending -- valid pixels only, never a padded column; the 256 sums are then folded in LDS, a[t] += a[t + k] for
// k = 128, 64, .. 1.  The attention kernel adds a channel's chunk sums in ascending chunk order to S, and
// m[c] = (float)(S / (double)(h w)).  No atomics.  Then z1[j] = max(b1[j] + sum_c w1[j][c] m[c], 0) and
// z[c] = b2[c] + sum_j w2[c][j] z1[j] in float64, ascending index, each term one rounded multiply and one rounded add (the
// first layer's products of two fp32 values are exact), and s[c] = (float)(1 / (1 + exp(-z[c]))).
//
// Determinism: the summation orders of the convolutions are those of sr_conv_mfma.h; a skip is one fmaf (or add) after the
// chain; the mean's order is fixed by (h, w) alone.  Nothing depends on tail.  Equal inputs give equal bits.
//
// Weights are caller-supplied (sr_rcan_create); nothing is fetched.
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_chan_attn.h"
#include "sr_net_common.h"

namespace {

constexpr size_t RC_TRUNK_CAP = SR_RCAN_TRUNK_CAP;     // the five trunk buffers of one image stay under 16 GiB (a policy)
constexpr int RC_TRUNK_BUFS = 5, RC_DEFAULT_TAIL = 256;         // RC_ROWS: sr_chan_attn.h
constexpr int RC_MAX_ROWS = 65535 * 4;                 // rows of one launch: the head's grid is rows / 4 blocks high
constexpr int RC_MAX_G = 16, RC_MAX_B = 32;

struct RcAffine {
    float mean[3];
    float range;
};

// ---------------------------------------------------------------------------------------------------------------
// Head (3 -> F) from the u8 image, as k_rn_head without a slope: x[c] = (u8 / 255 - mean[c]) * range inside the image, 0
// outside (zero is padded after the affine); the 3 x 256 values are tabulated in LDS with exactly that fp32 arithmetic.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rc_head(const unsigned char *__restrict__ img, long long stride, int H, int W,
                                                 const float *__restrict__ wt, const float *__restrict__ bias, RcAffine af,
                                                 float *__restrict__ out, int ya, int xa, int rows, int cols, int pitch, long long plane)
{
    __shared__ float lut[3][256];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    {
        const float v = (float)tid / 255.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) lut[c][tid] = (v - af.mean[c]) * af.range;
    }
    __syncthreads();
    head_frame<256>(img, stride, H, W, wt, bias, &lut[0][0], out, ya, xa, rows, cols, pitch, plane, [](int, float y) { return y; });
}

// The epilogues of k_rc_conv.
enum { RC_RELU = 0, RC_PLAIN = 1, RC_ADD = 2, RC_SHUF2 = 3, RC_SHUF3 = 4, RC_LAST_F32 = 5, RC_LAST_U8 = 6 };

// What an epilogue needs beside the convolution's own arguments.
struct RcEpi {
    const float *skip;             // RC_ADD: planar, element (c, gy, gx) at skip[c * skip_plane + (gy - skip_ya) * skip_pitch + gx - skip_xa]
    long long skip_plane;          //         (may be the output buffer itself: a thread reads the element it then writes)
    int skip_pitch, skip_ya, skip_xa;
    RcAffine af;                   // RC_LAST_*
    void *dst;                     // RC_LAST_*: HWC output, u8 or fp32
    long long dst_stride;          // bytes
};

// ---------------------------------------------------------------------------------------------------------------
// 3 x 3 implicit-GEMM convolution on v_mfma_f32_32x32x2_f32, stride 1, zero padding 1 at the image border.
//   conv_mfma_mainloop<3, 8, NC2, true> (sr_conv_mfma.h) plus an epilogue; NC2 = 32-cout halves per block (2, the last
//   convolution 1).
//   RC_RELU      y > 0 ? y : +0, planar store                                          (an RCAB's first convolution)
//   RC_PLAIN     planar store                                                          (an RCAB's second convolution)
//   RC_ADD       y + skip, planar store                                                (group convolution, conv_after_body)
//   RC_SHUF2/3   couts F r^2 in tiles of 64; cout co goes to channel co / r^2 at (r row + (co % r^2) / r, r col + co % r) of
//                the planar output at r x the resolution (origin r out_ya, r out_xa); sr_resnet.hip's RN_SHUF* without a slope
//   RC_LAST_*    the 3 couts zero-padded to 32; o = y / range + mean, HWC store (u8: clamp, scale, round half even); out_ya /
//                out_xa are coordinates in the full-resolution image; sr_resnet.hip's RN_LAST_* without the bilinear base
// ---------------------------------------------------------------------------------------------------------------
template <int NC2, int EPI>
__global__ __launch_bounds__(256) void k_rc_conv(const float *__restrict__ in, long long in_plane, int in_pitch, int in_ya, int in_xa,
                                                 int in_rows, int in_cols, int H_in, int W_in, int cin, const float *__restrict__ wslab,
                                                 const float *__restrict__ bias, float *out, long long out_plane, int out_pitch,
                                                 int out_ya, int out_xa, int rows, int cols, RcEpi ep)
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
        if constexpr (EPI == RC_RELU || EPI == RC_PLAIN) {
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    float y = acc[c2][pr][r];
                    if constexpr (EPI == RC_RELU) y = y > 0.0f ? y : 0.0f;
                    out[(size_t)co * out_plane + (size_t)row * out_pitch + col] = y;
                }
        } else if constexpr (EPI == RC_ADD) {
            const size_t so = skip_offset(out_ya + row, out_xa + col, ep.skip_ya, ep.skip_xa, ep.skip_pitch);
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    const float sk = ep.skip[(size_t)co * ep.skip_plane + so];
                    out[(size_t)co * out_plane + (size_t)row * out_pitch + col] = acc[c2][pr][r] + sk;
                }
        } else if constexpr (EPI == RC_SHUF2 || EPI == RC_SHUF3) {
            constexpr int R = EPI == RC_SHUF2 ? 2 : 3;
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    const int c = co / (R * R), rem = co % (R * R), dy = rem / R, dx = rem % R;
                    out[(size_t)c * out_plane + ((size_t)row * R + dy) * out_pitch + (size_t)col * R + dx] = acc[c2][pr][r];
                }
        } else {                                           // output affine + HWC store
            if (half != 0) continue;                       // couts 0 .. 2 live in registers 0 .. 2 of the lower half-wave
            const int gy = out_ya + row, gx = out_xa + col;
            char *d = (char *)ep.dst + (size_t)gy * ep.dst_stride;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float o = acc[0][pr][c] / ep.af.range + ep.af.mean[c];
                store_hwc<EPI == RC_LAST_U8>(d, (size_t)gx * 3 + c, o);
            }
        }
    }
}

int rc_check_desc(const char *who, const sr_rcan_desc *d)
{
    if (!d) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null description", who);
    const int F = d->n_feat;
    if ((F != 64 && F != 128 && F != 192 && F != 256) || d->n_squeeze < 1 || d->n_squeeze > F || d->n_groups < 1 || d->n_groups > RC_MAX_G ||
        d->n_blocks < 0 || d->n_blocks > RC_MAX_B || d->scale < 1 || d->scale > 4)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d features, squeeze width %d, %d groups of %d blocks, scale %d is outside "
                            "F in {64, 128, 192, 256}, 1 <= R <= F, 1 <= G <= 16, 0 <= B <= 32, 1 <= s <= 4",
                            who, F, d->n_squeeze, d->n_groups, d->n_blocks, d->scale);
    const float v[] = {d->res_scale, d->mean[0], d->mean[1], d->mean[2], d->range};
    for (float x : v)
        if (!std::isfinite(x)) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: res_scale, mean and range must be finite", who);
    if (d->range == 0.0f) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: range must not be 0", who);
    return SR_OK;
}

// The tables of sr_rcan_create in forward order: head, per group (per RCAB conv, conv, att1, att3) and the group convolution,
// conv_after_body, the upsampling stages, conv_last.
enum { T_HEAD = 0, T_CONV = 1, T_ATT1 = 2, T_ATT3 = 3, T_UP = 4, T_LAST = 5 };
struct RcTable {
    int kind, r;                   // r: shuffle factor of an upsampling stage, else 1
};

std::vector<RcTable> rc_tables(const sr_rcan_desc &d)
{
    std::vector<RcTable> t;
    t.push_back({T_HEAD, 1});
    for (int g = 0; g < d.n_groups; ++g) {
        for (int b = 0; b < d.n_blocks; ++b)
            for (int k : {T_CONV, T_CONV, T_ATT1, T_ATT3}) t.push_back({k, 1});
        t.push_back({T_CONV, 1});
    }
    t.push_back({T_CONV, 1});
    if (d.scale == 4) {
        t.push_back({T_UP, 2});
        t.push_back({T_UP, 2});
    } else if (d.scale > 1) {
        t.push_back({T_UP, d.scale});
    }
    t.push_back({T_LAST, 1});
    return t;
}

// The extent rule's view of the tail phase's convolutions: the upsampling stages and conv_last (the halo is 1, 2 or 3).
std::vector<ExtStep> rc_tail_steps(int scale)
{
    std::vector<ExtStep> s;
    if (scale == 4) {
        s.push_back({2, 1});
        s.push_back({2, 2});
    } else if (scale > 1) {
        s.push_back({scale, 1});
    }
    s.push_back({1, scale});
    return s;
}

struct RcGeom {
    int tail = 0, halo = 0, chunks = 0;
    long long tail_tiles = 0;
    long long plane0 = 0, plane_t = 0;                  // a trunk plane, the largest plane of a tail buffer
    size_t workspace_bytes = 0;
};

// Host only: buffer geometry and the tail's sub-piece grid of an h x w input.
int rc_geometry(const char *who, const sr_rcan_desc &d, int h, int w, int tail, RcGeom &g)
{
    const int S = d.scale, F = d.n_feat, rc = check_sr_geometry(who, h, w, S, tail < 0, "tail");
    if (rc) return rc;
    if (tail == 0) tail = RC_DEFAULT_TAIL;
    g.tail = tail;
    g.plane0 = (long long)h * pad4(w);
    g.chunks = (h + RC_ROWS - 1) / RC_ROWS;
    if (g.plane0 * 8 > INT_MAX)       // the convolution indexes one 8-channel chunk of a buffer with 32-bit offsets
        return sr_set_error(SR_ERR_SHAPE, "%s: an image of %lld activations per channel is too large (the trunk is one piece)", who, g.plane0);
    const size_t per_pixel = (size_t)RC_TRUNK_BUFS * F * sizeof(float);
    if ((size_t)g.plane0 * per_pixel > RC_TRUNK_CAP) {
        const long long fit = (long long)(RC_TRUNK_CAP / per_pixel);
        return sr_set_error(SR_ERR_SHAPE, "%s: the trunk of a %dx%d input is one piece of %d buffers of %d planes, %zu bytes per pixel, above "
                            "the %d GiB cap: at F = %d the largest input that fits has %lld pixels (about %.1f MP)", who, w, h, RC_TRUNK_BUFS, F,
                            per_pixel, (int)(RC_TRUNK_CAP >> 30), F, fit, (double)fit / 1e6);
    }
    if (h > RC_MAX_ROWS) return sr_set_error(SR_ERR_SHAPE, "%s: %d rows are more than one launch covers (%d)", who, h, RC_MAX_ROWS);
    const std::vector<ExtStep> steps = rc_tail_steps(S);
    const int n = (int)steps.size();
    g.halo = backward_halo(steps.data(), n);
    std::vector<int> a, b;
    long long rows_t = 0, pitch_t = 0, cnt[2] = {0, 0};
    for (int axis = 0; axis < 2; ++axis) {
        const int len = axis == 0 ? h : w;
        for (long long lo = 0; lo < len; lo += tail) {
            backward_extents(steps.data(), n, S, (int)lo, (int)std::min<long long>(lo + tail, len), len, a, b);
            long long m = 0;
            for (int i = 0; i + 1 < n; ++i) m = std::max(m, (long long)(b[i] - a[i]) * steps[i].r);    // conv_last stores no plane
            if (axis == 0) rows_t = std::max(rows_t, m);
            else pitch_t = std::max(pitch_t, pad4(m));
            ++cnt[axis];
        }
    }
    g.tail_tiles = cnt[0] * cnt[1];
    if (g.tail_tiles > INT_MAX) return sr_set_error(SR_ERR_SHAPE, "%s: %lld tail sub-pieces overflow int; use a larger tail", who, g.tail_tiles);
    g.plane_t = rows_t * pitch_t;
    if (g.plane_t * 8 > INT_MAX || rows_t > 2LL * RC_MAX_ROWS)
        return sr_set_error(SR_ERR_SHAPE, "%s: a tail sub-piece of %lld activations per channel is too large; use a smaller tail", who, g.plane_t);
    g.workspace_bytes = ((size_t)RC_TRUNK_BUFS * F * (size_t)g.plane0 + (size_t)2 * F * (size_t)g.plane_t) * sizeof(float) +
                        (size_t)F * g.chunks * sizeof(double) + (size_t)F * sizeof(float);
    return SR_OK;
}

}  // namespace

struct sr_rcan_model : SrModelBase {           // d_w, d_b: per table (rc_tables)
    sr_rcan_desc d{};
    std::vector<RcTable> tables;
    DevBuf trunk[RC_TRUNK_BUFS];              // h / f, two that rotate as group input and t, y1, y2
    DevBuf tailbuf[2];
    DevBuf red;                               // F x chunks float64 chunk sums, then s[F]
    void release_device()
    {
        for (auto &b : trunk) b.release();
        for (DevBuf *b : {&tailbuf[0], &tailbuf[1], &red}) b->release();
        release_base();
    }
};

static LiveSet g_rc_live;

static int rc_forward(sr_rcan_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride, int tail,
                      bool u8, const char *who)
{
    if (!g_rc_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    sr_ctx *ctx = m->ctx;
    CTX_ENTER(ctx);
    const int F = m->d.n_feat, R = m->d.n_squeeze, G = m->d.n_groups, B = m->d.n_blocks, S = m->d.scale;
    int rc = check_sr_forward_args(who, d_src, src_stride, w, d_dst, dst_stride, S, u8);
    if (rc) return rc;
    RcGeom g;
    rc = rc_geometry(who, m->d, h, w, tail, g);
    if (rc) return rc;
    if ((rc = ensure_activation_buffers(ctx, m->trunk, RC_TRUNK_BUFS, (size_t)g.plane0 * F, who))) return rc;
    if ((rc = ensure_activation_buffers(ctx, m->tailbuf, 2, (size_t)g.plane_t * F, who))) return rc;
    const size_t part_bytes = (size_t)F * g.chunks * sizeof(double);
    SRCHK(m->red.reserve(ctx, who, part_bytes + (size_t)F * sizeof(float)));
    double *part = m->red.as<double>();
    float *s = m->red.as<float>(part_bytes);
    hipStream_t st = ctx->stream;
    RcEpi ep{};
    ep.af = {{m->d.mean[0], m->d.mean[1], m->d.mean[2]}, m->d.range};
    ep.dst = d_dst;
    ep.dst_stride = (long long)dst_stride;
    // ---- trunk phase: the whole image, every tensor in one layout ----
    const PlanarTen L = planar_tensor(nullptr, 0, 0, h, w);
    auto ten = [&](float *base) { PlanarTen t = L; t.p = base; return t; };
    ep.skip_plane = L.plane;
    ep.skip_pitch = L.pitch;
    float *Hb = m->trunk[0].as<float>(), *f0 = m->trunk[1].as<float>(), *f1 = m->trunk[2].as<float>();
    float *Y1 = m->trunk[3].as<float>(), *Y2 = m->trunk[4].as<float>();
    auto conv = [&](auto kernel, const char *name, float *in, int k, float *out, const float *skip) {
        ProfScope ps(ctx, name);
        RcEpi e = ep;
        e.skip = skip;
        launch_conv(kernel, st, ten(in), h, w, F, F / 64, m->w(k), m->b(k), out, L.plane, L.pitch, 0, 0, h, w, e);
    };
    {
        ProfScope ps(ctx, "rcan_head");
        hipLaunchKernelGGL(k_rc_head, dim3((w + 63) / 64, (h + 3) / 4, F / 64), dim3(64, 4), 0, st, d_src, (long long)src_stride, h, w, m->w(0),
                           m->b(0), ep.af, Hb, 0, 0, h, w, L.pitch, L.plane);
    }
    int k = 1;
    float *gin = Hb;                                       // the group input; f1 is free only while it is still h
    const long long plane4 = L.plane / 4;
    for (int gi = 0; gi < G; ++gi) {
        float *t = gin;
        for (int b = 0; b < B; ++b, k += 4) {
            conv(k_rc_conv<2, RC_RELU>, "rcan_conv", t, k, Y1, nullptr);
            conv(k_rc_conv<2, RC_PLAIN>, "rcan_conv", Y1, k + 1, Y2, nullptr);
            rc_attention(st, ctx, Y2, L.plane, L.pitch, h, w, F, R, m->w(k + 2), m->b(k + 2), m->w(k + 3), m->b(k + 3), part, s, nullptr);
            ProfScope ps(ctx, "rcan_scale");
            float *o = b == 0 ? f0 : t;                    // the group's first RCAB leaves the group input whole
            hipLaunchKernelGGL(k_rc_scale, dim3((unsigned)((plane4 + 255) / 256), F), dim3(256), 0, st, (const float4 *)Y2, s, (const float4 *)t,
                               (float4 *)o, plane4, m->d.res_scale);
            t = o;
        }
        if (B > 0 && gin != Hb) {                          // in place over the group input
            conv(k_rc_conv<2, RC_ADD>, "rcan_conv", t, k, gin, gin);
        } else if (B > 0) {                                // the first group: h stays whole for the long skip
            conv(k_rc_conv<2, RC_ADD>, "rcan_conv", t, k, f1, gin);
            gin = f1;
        } else if (gin == Hb) {                            // B = 0: the convolution reads what it would overwrite
            conv(k_rc_conv<2, RC_ADD>, "rcan_conv", gin, k, f0, gin);
            gin = f0;
            f0 = f1;
        } else {
            conv(k_rc_conv<2, RC_ADD>, "rcan_conv", gin, k, f0, gin);
            std::swap(gin, f0);
        }
        ++k;
    }
    conv(k_rc_conv<2, RC_ADD>, "rcan_conv", gin, k, Hb, Hb);      // f = conv_after_body(t) + h, in place over h
    ++k;
    rc = check_launch(who);
    if (rc) return rc;
    // ---- tail phase: sub-pieces of the input over their own backward extents ----
    const std::vector<ExtStep> steps = rc_tail_steps(S);
    const int n = (int)steps.size();
    const PlanarTen f = ten(Hb);
    std::vector<int> ya, yb, xa, xb;
    for (int sy = 0; sy < h; sy = (int)std::min<long long>((long long)sy + g.tail, h))
        for (int sx = 0; sx < w; sx = (int)std::min<long long>((long long)sx + g.tail, w)) {
            backward_extents(steps.data(), n, S, sy, (int)std::min<long long>((long long)sy + g.tail, h), h, ya, yb);
            backward_extents(steps.data(), n, S, sx, (int)std::min<long long>((long long)sx + g.tail, w), w, xa, xb);
            PlanarTen t = f;
            for (int i = 0; i < n; ++i) {
                const int rows = yb[i] - ya[i], cols = xb[i] - xa[i], mult = steps[i].mult, r = steps[i].r;
                if (i + 1 < n) {
                    ProfScope ps(ctx, "rcan_up");
                    const PlanarTen o = planar_tensor(m->tailbuf[i & 1].as<float>(), ya[i] * r, xa[i] * r, rows * r, cols * r);
                    if (r == 2)
                        launch_conv(k_rc_conv<2, RC_SHUF2>, st, t, h * mult, w * mult, F, F * 4 / 64, m->w(k + i), m->b(k + i), o.p, o.plane, o.pitch,
                                    ya[i], xa[i], rows, cols, ep);
                    else
                        launch_conv(k_rc_conv<2, RC_SHUF3>, st, t, h * mult, w * mult, F, F * 9 / 64, m->w(k + i), m->b(k + i), o.p, o.plane, o.pitch,
                                    ya[i], xa[i], rows, cols, ep);
                    t = o;
                } else {
                    ProfScope ps(ctx, "rcan_last");
                    if (u8)
                        launch_conv(k_rc_conv<1, RC_LAST_U8>, st, t, h * mult, w * mult, F, 1, m->w(k + i), m->b(k + i), nullptr, 0LL, 0, ya[i], xa[i],
                                    rows, cols, ep);
                    else
                        launch_conv(k_rc_conv<1, RC_LAST_F32>, st, t, h * mult, w * mult, F, 1, m->w(k + i), m->b(k + i), nullptr, 0LL, 0, ya[i], xa[i],
                                    rows, cols, ep);
                }
            }
            rc = check_launch(who);
            if (rc) return rc;
        }
    return SR_OK;
}

// The self-ensemble over rc_forward (driver: sr_ensemble.hip).  A flip or a transpose permutes the pixels of every plane, so the
// pooled mean of a member is the mean of that member's own planes: nothing special is needed.
static int rc_ensemble(sr_rcan_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride, int tail,
                       int mask, bool u8, const char *who)
{
    const int rc = sr_ens_check_mask(who, mask);
    if (rc) return rc;
    if (tail < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: %s must be >= 1, or 0 for the library's choice", who, "tail");
    if (!g_rc_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    return ens_run(who, *m, m->d.scale, [&](const uint8_t *s, int64_t ss, int hh, int ww, float *d, int64_t ds) {
        return rc_forward(m, s, ss, hh, ww, d, ds, tail, false, who);
    }, d_src, src_stride, h, w, d_dst, dst_stride, mask, u8);
}

extern "C" {

int sr_rcan_create(sr_ctx *ctx, const sr_rcan_desc *desc, const float *const *h_w, const float *const *h_b, int n_tables, sr_rcan_model **out)
{
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_rcan_create: null out");
    *out = nullptr;
    int rc = rc_check_desc("sr_rcan_create", desc);                         // host decision, before any device call
    if (rc) return rc;
    const std::vector<RcTable> tables = rc_tables(*desc);
    if ((rc = check_weight_tables("sr_rcan_create", "table", (int)tables.size(), n_tables, h_w, h_b))) return rc;
    CTX_ENTER(ctx);
    sr_rcan_model *M = new sr_rcan_model();
    M->ctx = ctx;
    M->d = *desc;
    M->tables = tables;
    g_rc_live.insert(M);
    const int F = desc->n_feat, R = desc->n_squeeze;
    for (int k = 0; k < n_tables; ++k) {
        const RcTable &t = tables[k];
        MfmaWeights a;
        if (t.kind == T_HEAD) a = {arrange_head_weights(h_w[k], F), std::vector<float>(h_b[k], h_b[k] + F)};
        else if (t.kind == T_ATT1) a = {std::vector<float>(h_w[k], h_w[k] + (size_t)R * F), std::vector<float>(h_b[k], h_b[k] + R)};
        else if (t.kind == T_ATT3) a = {std::vector<float>(h_w[k], h_w[k] + (size_t)F * R), std::vector<float>(h_b[k], h_b[k] + F)};
        else if (t.kind == T_LAST) a = arrange_mfma_weights(h_w[k], h_b[k], 3, F, 9, 8, 32);
        else a = arrange_mfma_weights(h_w[k], h_b[k], F * t.r * t.r, F, 9, 8, 64);
        if ((rc = upload_conv("sr_rcan_create", *M, a))) {
            sr_rcan_destroy(M);
            return rc;
        }
    }
    *out = M;
    return SR_OK;
}

int sr_rcan_destroy(sr_rcan_model *m)
{
    return destroy_model(m, g_rc_live);
}

int sr_rcan_plan(const sr_rcan_desc *desc, int h, int w, int tail, int *halo, int *n_tail_tiles, size_t *workspace_bytes)
{
    int rc = rc_check_desc("sr_rcan_plan", desc);
    if (rc) return rc;
    RcGeom g;
    rc = rc_geometry("sr_rcan_plan", *desc, h, w, tail, g);
    if (rc) return rc;
    if (halo) *halo = g.halo;
    if (n_tail_tiles) *n_tail_tiles = (int)g.tail_tiles;
    if (workspace_bytes) *workspace_bytes = g.workspace_bytes;
    return SR_OK;
}

int sr_rcan_u8(sr_rcan_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride, int tail)
{
    return rc_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tail, true, "sr_rcan_u8");
}

int sr_rcan_f32(sr_rcan_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride, int tail)
{
    return rc_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tail, false, "sr_rcan_f32");
}

int sr_rcan_ens_u8(sr_rcan_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride, int tail,
                   int mask)
{
    return rc_ensemble(model, d_src, src_stride, h, w, d_dst, dst_stride, tail, mask, true, "sr_rcan_ens_u8");
}

int sr_rcan_ens_f32(sr_rcan_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride, int tail,
                    int mask)
{
    return rc_ensemble(model, d_src, src_stride, h, w, d_dst, dst_stride, tail, mask, false, "sr_rcan_ens_f32");
}

int sr_rcan_attention_f32(sr_ctx *ctx, const float *d_x, int64_t plane_stride, int64_t row_stride, int n_feat, int n_squeeze, int h, int w,
                          const float *h_w1, const float *h_b1, const float *h_w2, const float *h_b2, float *h_mean, float *h_s)
{
    const char *who = "sr_rcan_attention_f32";
    if (!d_x || !h_w1 || !h_b1 || !h_w2 || !h_b2 || !h_mean || !h_s) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    const int F = n_feat, R = n_squeeze;
    if (F < 1 || F > 256 || R < 1 || R > F) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d channels, squeeze width %d is outside 1 <= R <= F <= 256", who, F, R);
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_SHAPE, "%s: %dx%d image", who, w, h);
    if (row_stride < (int64_t)w * 4 || plane_stride < row_stride * h) return sr_set_error(SR_ERR_SHAPE, "%s: a stride is smaller than what it spans", who);
    if (row_stride % 4 || plane_stride % 4 || (uintptr_t)d_x % 4)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: the pointer and the strides must be multiples of 4 bytes", who);
    CTX_ENTER(ctx);
    const int chunks = (h + RC_ROWS - 1) / RC_ROWS;
    // [chunk sums F x chunks f64][w1 R F][b1 R][w2 F R][b2 F][mean F][s F]
    const size_t part_bytes = (size_t)F * chunks * sizeof(double), nw = (size_t)R * F;
    DevTemp tmp(ctx);
    SRCHK(tmp.alloc(who, part_bytes + (2 * nw + R + 3 * (size_t)F) * sizeof(float)));
    float *w1 = tmp.as<float>(part_bytes), *b1 = w1 + nw, *w2 = b1 + R, *b2 = w2 + nw, *mean = b2 + F, *s = mean + F;
    HIPCHK(hipMemcpyAsync(w1, h_w1, nw * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(b1, h_b1, R * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(w2, h_w2, nw * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(b2, h_b2, F * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    rc_attention(ctx->stream, ctx, d_x, plane_stride / 4, row_stride / 4, h, w, F, R, w1, b1, w2, b2, tmp.as<double>(), s, mean);
    SRCHK(check_launch(who));
    HIPCHK(hipMemcpyAsync(h_mean, mean, F * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h_s, s, F * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // extern "C"
