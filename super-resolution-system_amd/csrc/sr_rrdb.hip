// sr_rrdb.hip -- local super-resolution backend: BasicSR's RRDBNet (ESRGAN, RealESRGAN_x4plus with 23 blocks,
// RealESRGAN_x4plus_anime_6B with 6) at scale 4 on gfx950.
//
//   head        3 x 3 convolution 3 -> F from the u8 image, x = u8 / 255, no activation                  -> h
//   RRDB x B    three dense blocks, then t_i = fmaf(beta, u, t_{i-1})
//     dense     x_k = act(conv_k(cat(x, x_1 .. x_{k-1}))), k = 1 .. 4 (F + (k - 1) G -> G);  out = fmaf(beta, conv_5(cat(x, x_1 .. x_4)), x)
//   trunk end   f = conv_body(t_B) + h
//   upsampling  nearest x 2, act(conv_up1);  nearest x 2, act(conv_up2)
//   HR convs    act(conv_hr), conv_last F -> 3 at 4 x the resolution, HWC store
//
// Everything is fp32 (fp32 in, fp32 accumulate).  Every F-input convolution is the implicit-GEMM mainloop of sr_conv_mfma.h
// (v_mfma_f32_32x32x2_f32, shared with sr_lpips.hip, sr_srnet.hip and sr_resnet.hip) behind one of the epilogues below; the
// 3 -> F head is head_accumulate with the u8 / 255 table.  What the three SR backends share around the mainloop -- the head
// frame, leaky / skip_offset / store_hwc, the backward extent rule, the planar tensor, the convolution launch, the models'
// lifetime -- is sr_net_common.h; this file holds the network's own kernels and epilogues, its two-phase geometry and its layer walk.
//
// Dense buffer: one planar fp32 buffer of F + 4 G planes.  Planar activations make a dense block's concatenation
// cat(x, x_1 .. x_k) "the first F + k G planes of one buffer": convolution k reads planes [0, F + (k - 1) G) and writes planes
// [F + (k - 1) G, F + k G) -- disjoint ranges, no hazard -- and convolution 5 writes fmaf(beta, y, x) into planes [0, F) of the
// NEXT dense buffer.  Three dense buffers rotate through an RRDB: block d works in buffer d, the third block's convolution 5
// writes fmaf(beta, fmaf(beta, y, x), r) in place over r = planes [0, F) of buffer 0 (each thread reads exactly the element it
// then writes).  h lives in a buffer of F planes of its own until conv_body has added it.  Trunk planes per piece:
// 3 (F + 4 G) + F at the input resolution, plus 4 F (F planes at 2 x) for f.
//
// Two phases.  The head reads 15 B + 4 input pixels beyond a piece's edge, which no 4 x layer could afford to carry, so the
// image is walked twice over:
//   trunk phase  tile x tile pieces of the input: head, the B RRDBs and conv_body over the backward extents of the piece; every
//                trunk tensor of a piece has ONE layout (the head's extent: origin, pitch, plane) and an op writes the
//                sub-rectangle that is its own extent.  conv_body stores f replicated 2 x 2, so the nearest-upsampled tensor is
//                what conv_up1 reads and the mainloop is the unchanged one.
//   tail phase   each trunk piece is walked in tail x tail sub-pieces of the input: conv_up1 (replicating store again),
//                conv_up2, conv_hr and conv_last over the sub-piece's own backward extents -- subsets of what the trunk piece
//                stored.  Only tail-sized 4 x buffers exist (two of F planes, ping-pong).
// Extent rule (as sr_resnet.hip): backwards from the piece's output rectangle, divided by r (rounded outwards) across a
// replication (r = 2 for conv_body and conv_up1), grown by one per convolution, clipped to the layer's image.  Zero padding is
// applied at the true image border only, so every value equals the unstreamed forward's and every (tile, tail) gives the same
// bits.
//
// Determinism: the summation orders are those of sr_conv_mfma.h over the channels of the CONCATENATION; a skip is one fmaf (or
// add) after the chain.  Nothing depends on the position in a block, a trunk piece or a tail piece.
//
// Weights are caller-supplied (sr_rrdb_create); nothing is fetched.
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_net_common.h"

namespace {

constexpr size_t RR_TRUNK_CAP = SR_RRDB_TRUNK_CAP;     // tile = 0: the largest trunk piece whose buffers stay under 16 GiB (a policy)
constexpr int RR_MAX_TILE = 2048, RR_TILE_STEP = 32, RR_DEFAULT_TAIL = 256;

// ---------------------------------------------------------------------------------------------------------------
// Head (3 -> F) from the u8 image, as k_sn_head: one thread = one output pixel x 64 output channels (blockIdx.z: 64-cout
// tile), x = u8 / 255 tabulated in LDS with exactly that fp32 division, 0 outside the image.  No activation.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rr_head(const unsigned char *__restrict__ img, long long stride, int H, int W,
                                                 const float *__restrict__ wt, const float *__restrict__ bias,
                                                 float *__restrict__ out, int ya, int xa, int rows, int cols, int pitch, long long plane)
{
    __shared__ float lut[256];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    lut[tid] = (float)tid / 255.0f;
    __syncthreads();
    head_frame<0>(img, stride, H, W, wt, bias, lut, out, ya, xa, rows, cols, pitch, plane, [](int, float y) { return y; });
}

// The epilogues of k_rr_conv.
enum { RR_ACT = 0, RR_SKIP = 1, RR_SKIP2 = 2, RR_REP_SKIP = 3, RR_REP_ACT = 4, RR_LAST_F32 = 5, RR_LAST_U8 = 6 };

// What an epilogue needs beside the convolution's own arguments.
struct RrEpi {
    float slope;                   // RR_ACT, RR_REP_ACT: y >= 0 ? y : slope * y
    float beta;                    // RR_SKIP: fmaf(beta, y, skip);  RR_SKIP2: fmaf(beta, fmaf(beta, y, skip), skip2)
    const float *skip, *skip2;     // planar, one layout: element (c, gy, gx) at [c * skip_plane + (gy - skip_ya) * skip_pitch + gx - skip_xa]
    long long skip_plane;          // (skip2 may be the output itself: a thread reads the element it then writes);  RR_REP_SKIP: y + skip
    int skip_pitch, skip_ya, skip_xa;
    void *dst;                     // RR_LAST_*: HWC output, u8 or fp32
    long long dst_stride;          // bytes
};

// ---------------------------------------------------------------------------------------------------------------
// 3 x 3 implicit-GEMM convolution on v_mfma_f32_32x32x2_f32, stride 1, zero padding 1 at the image border.
//   conv_mfma_mainloop<3, 8, NC2, true> (sr_conv_mfma.h) plus an epilogue; NC2 = 32-cout halves per block (G = 32 and the last
//   convolution 1, everything else 2); cin is a runtime argument (the planes of the concatenation read so far).
//   RR_ACT        slope, planar store
//   RR_SKIP       fmaf(beta, y, skip), planar store                                   (dense blocks 1 and 2, convolution 5)
//   RR_SKIP2      fmaf(beta, fmaf(beta, y, skip), skip2), planar store                (dense block 3, convolution 5)
//   RR_REP_SKIP   y + skip, stored 2 x 2 replicated: value (row, col) goes to (2 row + {0, 1}, 2 col + {0, 1}) of the planar
//                 output at twice the resolution (origin 2 out_ya, 2 out_xa)          (conv_body)
//   RR_REP_ACT    slope, stored 2 x 2 replicated                                      (conv_up1)
//   RR_LAST_*     the 3 couts zero-padded to 32; HWC store (u8: clamp, scale, round half even); out_ya / out_xa are
//                 coordinates in the full-resolution image
// ---------------------------------------------------------------------------------------------------------------
template <int NC2, int EPI>
__global__ __launch_bounds__(256) void k_rr_conv(const float *__restrict__ in, long long in_plane, int in_pitch, int in_ya, int in_xa,
                                                 int in_rows, int in_cols, int H_in, int W_in, int cin, const float *__restrict__ wslab,
                                                 const float *__restrict__ bias, float *out, long long out_plane, int out_pitch,
                                                 int out_ya, int out_xa, int rows, int cols, RrEpi ep)
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
        if constexpr (EPI == RR_ACT) {
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    const float y = acc[c2][pr][r];
                    out[(size_t)co * out_plane + (size_t)row * out_pitch + col] = leaky(y, ep.slope);
                }
        } else if constexpr (EPI == RR_SKIP || EPI == RR_SKIP2) {
            const size_t so = skip_offset(out_ya + row, out_xa + col, ep.skip_ya, ep.skip_xa, ep.skip_pitch);
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    float v = fmaf(ep.beta, acc[c2][pr][r], ep.skip[(size_t)co * ep.skip_plane + so]);
                    if constexpr (EPI == RR_SKIP2) v = fmaf(ep.beta, v, ep.skip2[(size_t)co * ep.skip_plane + so]);
                    out[(size_t)co * out_plane + (size_t)row * out_pitch + col] = v;
                }
        } else if constexpr (EPI == RR_REP_SKIP || EPI == RR_REP_ACT) {
            const size_t so = skip_offset(out_ya + row, out_xa + col, ep.skip_ya, ep.skip_xa, ep.skip_pitch);
            const size_t oo = (size_t)(2 * row) * out_pitch + 2 * col;     // out_pitch and out_plane are even: 8-byte aligned
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    float v = acc[c2][pr][r];
                    if constexpr (EPI == RR_REP_SKIP) v = v + ep.skip[(size_t)co * ep.skip_plane + so];
                    else v = leaky(v, ep.slope);
                    float *o = out + (size_t)co * out_plane + oo;
                    const float2 vv = make_float2(v, v);
                    *(float2 *)o = vv;
                    *(float2 *)(o + out_pitch) = vv;
                }
        } else {                                           // HWC store
            if (half != 0) continue;                       // couts 0 .. 2 live in registers 0 .. 2 of the lower half-wave
            const int gy = out_ya + row, gx = out_xa + col;
            char *d = (char *)ep.dst + (size_t)gy * ep.dst_stride;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                store_hwc<EPI == RR_LAST_U8>(d, (size_t)gx * 3 + c, acc[0][pr][c]);
            }
        }
    }
}

int rr_check_desc(const char *who, const sr_rrdb_desc *d)
{
    if (!d) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null description", who);
    const int F = d->n_feat, G = d->n_grow;
    if ((F != 64 && F != 128 && F != 192 && F != 256) || (G != 32 && G != 64) || d->n_blocks < 0 || d->n_blocks > 32)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d features, growth %d, %d blocks is outside F in {64, 128, 192, 256}, "
                            "G in {32, 64}, 0 <= B <= 32", who, F, G, d->n_blocks);
    if (d->scale != 4)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: scale %d: only the x4 network (the x2 / x1 variants put a pixel-unshuffle in front "
                            "of conv_first)", who, d->scale);
    if (!std::isfinite(d->slope) || !std::isfinite(d->res_scale))
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: slope and res_scale must be finite", who);
    return SR_OK;
}

// Convolutions in forward order: head, 15 per RRDB, conv_body, conv_up1, conv_up2, conv_hr, conv_last.
int rr_n_conv(int B) { return 1 + 15 * B + 5; }
// Replication factor behind convolution i (conv_body and conv_up1 store 2 x 2) and its resolution multiplier.
int rr_rep(int n, int i) { return (i == n - 5 || i == n - 4) ? 2 : 1; }
int rr_mult(int n, int i) { return i >= n - 3 ? 4 : (i == n - 4 ? 2 : 1); }

// The extent rule's view of the n convolutions (backward_extents, backward_halo: sr_net_common.h; the halo is 15 B + 4).
std::vector<ExtStep> rr_steps(int n)
{
    std::vector<ExtStep> steps(n);
    for (int i = 0; i < n; ++i) steps[i] = {rr_rep(n, i), rr_mult(n, i)};
    return steps;
}

// One axis: the piece [lo, hi) of an axis of len input pixels -> per convolution the range [a[i], b[i]) of its output.
void rr_extents(const std::vector<ExtStep> &steps, int lo, int hi, int len, std::vector<int> &a, std::vector<int> &b)
{
    backward_extents(steps.data(), (int)steps.size(), 4, lo, hi, len, a, b);
}

struct RrGeom {
    int tile = 0, tail = 0, tiles_x = 0, tiles_y = 0, halo = 0;
    long long tail_tiles = 0;
    long long plane0 = 0, plane2 = 0, plane4 = 0;       // largest plane of a trunk tensor, of f at 2 x, of a 4 x tail tensor
    size_t trunk_floats = 0, workspace_floats = 0;
};

// Largest trunk planes over the pieces of one tile size: the extents of an axis depend on that axis alone, so the tallest and
// the widest piece make the largest plane.
void rr_trunk_planes(const std::vector<ExtStep> &steps, int h, int w, int tile, long long &plane0, long long &plane2)
{
    const int n = (int)steps.size();
    std::vector<int> a, b;
    long long rows0 = 0, rows2 = 0, pitch0 = 0, pitch2 = 0;
    for (long long lo = 0; lo < h; lo += tile) {
        rr_extents(steps, (int)lo, (int)std::min<long long>(lo + tile, h), h, a, b);
        rows0 = std::max(rows0, (long long)b[0] - a[0]);
        rows2 = std::max(rows2, 2LL * (b[n - 5] - a[n - 5]));
    }
    for (long long lo = 0; lo < w; lo += tile) {
        rr_extents(steps, (int)lo, (int)std::min<long long>(lo + tile, w), w, a, b);
        pitch0 = std::max(pitch0, pad4((long long)b[0] - a[0]));
        pitch2 = std::max(pitch2, pad4(2LL * (b[n - 5] - a[n - 5])));
    }
    plane0 = rows0 * pitch0;
    plane2 = rows2 * pitch2;
}

size_t rr_trunk_floats(const sr_rrdb_desc &d, long long plane0, long long plane2)
{
    return (size_t)(3 * (d.n_feat + 4 * d.n_grow) + d.n_feat) * (size_t)plane0 + (size_t)d.n_feat * (size_t)plane2;
}

// Host only: piece grids and buffer geometry of an h x w input.
int rr_geometry(const char *who, const sr_rrdb_desc &d, int h, int w, int tile, int tail, RrGeom &g)
{
    const int rc = check_sr_geometry(who, h, w, 4, tile < 0 || tail < 0, "tile and tail");
    if (rc) return rc;
    const int n = rr_n_conv(d.n_blocks);
    const std::vector<ExtStep> steps = rr_steps(n);
    g.halo = backward_halo(steps.data(), n);
    if (tile == 0) {                  // the largest multiple of 32 whose trunk buffers, as laid out for this image, fit the cap
        tile = RR_TILE_STEP;
        for (int t = RR_MAX_TILE; t > RR_TILE_STEP; t -= RR_TILE_STEP) {
            long long p0, p2;
            rr_trunk_planes(steps, h, w, t, p0, p2);
            if (rr_trunk_floats(d, p0, p2) * sizeof(float) <= RR_TRUNK_CAP) {
                tile = t;
                break;
            }
        }
    }
    if (tail == 0) tail = RR_DEFAULT_TAIL;
    g.tile = tile;
    g.tail = tail;
    g.tiles_x = (int)(((long long)w + tile - 1) / tile);
    g.tiles_y = (int)(((long long)h + tile - 1) / tile);
    rr_trunk_planes(steps, h, w, tile, g.plane0, g.plane2);
    // tail sub-pieces: every trunk piece is walked from its own origin
    std::vector<int> a, b;
    long long rows4 = 0, pitch4 = 0, cnt_y = 0, cnt_x = 0;
    for (int axis = 0; axis < 2; ++axis) {
        const int len = axis == 0 ? h : w;
        for (long long lo = 0; lo < len; lo += tile) {
            const long long hi = std::min<long long>(lo + tile, len);
            for (long long s = lo; s < hi; s += tail) {
                rr_extents(steps, (int)s, (int)std::min<long long>(s + tail, hi), len, a, b);
                long long m = 0;
                for (int i = n - 4; i < n - 1; ++i) m = std::max(m, (long long)(b[i] - a[i]) * rr_rep(n, i));   // conv_last stores no plane
                if (axis == 0) { rows4 = std::max(rows4, m); ++cnt_y; }
                else { pitch4 = std::max(pitch4, pad4(m)); ++cnt_x; }
            }
        }
    }
    // sub-pieces per trunk row x per trunk column: the grid is a product, and so is its count
    g.tail_tiles = cnt_y * cnt_x;
    if (g.tail_tiles > INT_MAX) return sr_set_error(SR_ERR_SHAPE, "%s: %lld tail sub-pieces overflow int; use a larger tail", who, g.tail_tiles);
    g.plane4 = rows4 * pitch4;
    const long long dense = g.plane0, big = std::max(std::max(g.plane0, g.plane2), g.plane4);
    if (big * 8 > INT_MAX || dense * 8 > INT_MAX)     // the convolution indexes one 8-channel chunk of a buffer with 32-bit offsets
        return sr_set_error(SR_ERR_SHAPE, "%s: a piece of %lld activations per channel is too large; use a smaller tile / tail", who, big);
    g.trunk_floats = rr_trunk_floats(d, g.plane0, g.plane2);
    g.workspace_floats = g.trunk_floats + (size_t)2 * d.n_feat * (size_t)g.plane4;
    return SR_OK;
}

}  // namespace

struct sr_rrdb_model : SrModelBase {
    sr_rrdb_desc d{};
    DevBuf dense[3];
    DevBuf hbuf;                              // h, until conv_body has added it
    DevBuf f2;                                // f replicated to 2 x: what the trunk phase leaves to the tail phase
    DevBuf tailbuf[2];
    void release_device()
    {
        for (DevBuf *b : {&dense[0], &dense[1], &dense[2], &hbuf, &f2, &tailbuf[0], &tailbuf[1]}) b->release();
        release_base();
    }
};

static LiveSet g_rr_live;

static int rr_forward(sr_rrdb_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride,
                      int tile, int tail, bool u8, const char *who)
{
    if (!g_rr_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    sr_ctx *ctx = m->ctx;
    CTX_ENTER(ctx);
    const int F = m->d.n_feat, G = m->d.n_grow, B = m->d.n_blocks, n = rr_n_conv(B), DP = F + 4 * G;
    int rc = check_sr_forward_args(who, d_src, src_stride, w, d_dst, dst_stride, 4, u8);
    if (rc) return rc;
    RrGeom g;
    rc = rr_geometry(who, m->d, h, w, tile, tail, g);
    if (rc) return rc;
    if ((rc = ensure_activation_buffers(ctx, m->dense, 3, (size_t)g.plane0 * DP, who))) return rc;
    if ((rc = ensure_activation_buffers(ctx, &m->hbuf, 1, (size_t)g.plane0 * F, who))) return rc;
    if ((rc = ensure_activation_buffers(ctx, &m->f2, 1, (size_t)g.plane2 * F, who))) return rc;
    if ((rc = ensure_activation_buffers(ctx, m->tailbuf, 2, (size_t)g.plane4 * F, who))) return rc;
    hipStream_t st = ctx->stream;
    const std::vector<ExtStep> steps = rr_steps(n);
    RrEpi ep0{};
    ep0.slope = m->d.slope;
    ep0.beta = m->d.res_scale;
    ep0.dst = d_dst;
    ep0.dst_stride = (long long)dst_stride;
    std::vector<int> ya, yb, xa, xb, sya, syb, sxa, sxb;
    for (int ty = 0; ty < g.tiles_y; ++ty)
        for (int tx = 0; tx < g.tiles_x; ++tx) {
            const int py0 = (int)((long long)ty * g.tile), py1 = (int)std::min<long long>((long long)py0 + g.tile, h);
            const int px0 = (int)((long long)tx * g.tile), px1 = (int)std::min<long long>((long long)px0 + g.tile, w);
            rr_extents(steps, py0, py1, h, ya, yb);
            rr_extents(steps, px0, px1, w, xa, xb);
            // ---- trunk phase: every tensor of the piece in the head's layout ----
            const PlanarTen L = planar_tensor(nullptr, ya[0], xa[0], yb[0] - ya[0], xb[0] - xa[0]);
            auto ten = [&](float *base) { PlanarTen t = L; t.p = base; return t; };
            auto at = [&](float *base, int i) { return base + (size_t)(ya[i] - L.ya) * L.pitch + (xa[i] - L.xa); };
            RrEpi ep = ep0;
            ep.skip_plane = L.plane;
            ep.skip_pitch = L.pitch;
            ep.skip_ya = L.ya;
            ep.skip_xa = L.xa;
            {
                ProfScope ps(ctx, "rrdb_head");
                // h goes to planes [0, F) of dense buffer 0 (the first dense block's x) and, where an RRDB will overwrite that in
                // place, to its own buffer as well (conv_body adds it)
                for (float *o : {m->dense[0].as<float>(), B > 0 ? m->hbuf.as<float>() : (float *)nullptr})
                    if (o)
                        hipLaunchKernelGGL(k_rr_head, dim3((L.cols + 63) / 64, (L.rows + 3) / 4, F / 64), dim3(64, 4), 0, st, d_src,
                                           (long long)src_stride, h, w, m->w(0), m->b(0), o, L.ya, L.xa, L.rows, L.cols, L.pitch, L.plane);
            }
            int i = 1;
            for (int blk = 0; blk < B; ++blk)
                for (int db = 0; db < 3; ++db) {
                    float *D = m->dense[db].as<float>();
                    // The guard is the buffer's stored extent (the head's).  Planes of x_j hold stale values outside convolution
                    // j's extent; by the extent rule (each extent is the next one grown by one, clipped) these reach only masked
                    // outputs, and an output depends on its own pixel's patch alone.
                    const PlanarTen in = ten(D);
                    for (int k = 1; k <= 4; ++k, ++i) {
                        ProfScope ps(ctx, "rrdb_dense");
                        const int cin = F + (k - 1) * G, rows = yb[i] - ya[i], cols = xb[i] - xa[i];
                        float *o = at(D + (size_t)cin * L.plane, i);
                        if (G == 32)
                            launch_conv(k_rr_conv<1, RR_ACT>, st, in, h, w, cin, 1, m->w(i), m->b(i), o, L.plane, L.pitch, ya[i], xa[i], rows, cols, ep);
                        else
                            launch_conv(k_rr_conv<2, RR_ACT>, st, in, h, w, cin, 1, m->w(i), m->b(i), o, L.plane, L.pitch, ya[i], xa[i], rows, cols, ep);
                    }
                    ProfScope ps(ctx, "rrdb_blockout");
                    const int rows = yb[i] - ya[i], cols = xb[i] - xa[i];
                    ep.skip = D;
                    if (db < 2) {
                        launch_conv(k_rr_conv<2, RR_SKIP>, st, in, h, w, DP, F / 64, m->w(i), m->b(i), at(m->dense[db + 1].as<float>(), i), L.plane, L.pitch, ya[i],
                                              xa[i], rows, cols, ep);
                    } else {                               // in place over the RRDB's input r
                        ep.skip2 = m->dense[0].as<float>();
                        launch_conv(k_rr_conv<2, RR_SKIP2>, st, in, h, w, DP, F / 64, m->w(i), m->b(i), at(m->dense[0].as<float>(), i), L.plane, L.pitch, ya[i],
                                               xa[i], rows, cols, ep);
                    }
                    ++i;
                }
            // conv_body + h, replicated to 2 x
            const PlanarTen f2 = planar_tensor(m->f2.as<float>(), 2 * ya[i], 2 * xa[i], 2 * (yb[i] - ya[i]), 2 * (xb[i] - xa[i]));
            {
                ProfScope ps(ctx, "rrdb_bodyup");
                ep.skip = B > 0 ? m->hbuf.as<float>() : m->dense[0].as<float>();
                launch_conv(k_rr_conv<2, RR_REP_SKIP>, st, ten(m->dense[0].as<float>()), h, w, F, F / 64, m->w(i), m->b(i), f2.p, f2.plane, f2.pitch, ya[i], xa[i],
                                          yb[i] - ya[i], xb[i] - xa[i], ep);
            }
            rc = check_launch(who);
            if (rc) return rc;
            // ---- tail phase: sub-pieces of this trunk piece ----
            const int u1 = n - 4, u2 = n - 3, hr = n - 2, la = n - 1;
            for (int sy = py0; sy < py1; sy = (int)std::min<long long>((long long)sy + g.tail, py1))
                for (int sx = px0; sx < px1; sx = (int)std::min<long long>((long long)sx + g.tail, px1)) {
                    rr_extents(steps, sy, (int)std::min<long long>((long long)sy + g.tail, py1), h, sya, syb);
                    rr_extents(steps, sx, (int)std::min<long long>((long long)sx + g.tail, px1), w, sxa, sxb);
                    auto rows = [&](int k) { return syb[k] - sya[k]; };
                    auto cols = [&](int k) { return sxb[k] - sxa[k]; };
                    const PlanarTen a = planar_tensor(m->tailbuf[0].as<float>(), 2 * sya[u1], 2 * sxa[u1], 2 * rows(u1), 2 * cols(u1));
                    const PlanarTen b = planar_tensor(m->tailbuf[1].as<float>(), sya[u2], sxa[u2], rows(u2), cols(u2));
                    const PlanarTen c = planar_tensor(m->tailbuf[0].as<float>(), sya[hr], sxa[hr], rows(hr), cols(hr));
                    {
                        ProfScope ps(ctx, "rrdb_bodyup");
                        launch_conv(k_rr_conv<2, RR_REP_ACT>, st, f2, 2 * h, 2 * w, F, F / 64, m->w(u1), m->b(u1), a.p, a.plane, a.pitch, sya[u1], sxa[u1],
                                                 rows(u1), cols(u1), ep);
                        launch_conv(k_rr_conv<2, RR_ACT>, st, a, 4 * h, 4 * w, F, F / 64, m->w(u2), m->b(u2), b.p, b.plane, b.pitch, sya[u2], sxa[u2],
                                             rows(u2), cols(u2), ep);
                    }
                    {
                        ProfScope ps(ctx, "rrdb_hr");
                        launch_conv(k_rr_conv<2, RR_ACT>, st, b, 4 * h, 4 * w, F, F / 64, m->w(hr), m->b(hr), c.p, c.plane, c.pitch, sya[hr], sxa[hr],
                                             rows(hr), cols(hr), ep);
                    }
                    {
                        ProfScope ps(ctx, "rrdb_last");
                        if (u8)
                            launch_conv(k_rr_conv<1, RR_LAST_U8>, st, c, 4 * h, 4 * w, F, 1, m->w(la), m->b(la), nullptr, 0LL, 0, sya[la], sxa[la], rows(la),
                                                     cols(la), ep);
                        else
                            launch_conv(k_rr_conv<1, RR_LAST_F32>, st, c, 4 * h, 4 * w, F, 1, m->w(la), m->b(la), nullptr, 0LL, 0, sya[la], sxa[la], rows(la),
                                                      cols(la), ep);
                    }
                    rc = check_launch(who);
                    if (rc) return rc;
                }
        }
    return SR_OK;
}

// The self-ensemble over rr_forward (driver: sr_ensemble.hip).
static int rr_ensemble(sr_rrdb_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride, int tile,
                       int tail, int mask, bool u8, const char *who)
{
    const int rc = sr_ens_check_mask(who, mask);
    if (rc) return rc;
    if (tile < 0 || tail < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: %s must be >= 1, or 0 for the library's choice", who, "tile and tail");
    if (!g_rr_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    return ens_run(who, *m, 4, [&](const uint8_t *s, int64_t ss, int hh, int ww, float *d, int64_t ds) {
        return rr_forward(m, s, ss, hh, ww, d, ds, tile, tail, false, who);
    }, d_src, src_stride, h, w, d_dst, dst_stride, mask, u8);
}

extern "C" {

int sr_rrdb_create(sr_ctx *ctx, const sr_rrdb_desc *desc, const float *const *h_w, const float *const *h_b, int n_conv, sr_rrdb_model **out)
{
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_rrdb_create: null out");
    *out = nullptr;
    int rc = rr_check_desc("sr_rrdb_create", desc);                         // host decision, before any device call
    if (rc) return rc;
    const int F = desc->n_feat, G = desc->n_grow, n = rr_n_conv(desc->n_blocks);
    if ((rc = check_weight_tables("sr_rrdb_create", "convolution", n, n_conv, h_w, h_b))) return rc;
    CTX_ENTER(ctx);
    sr_rrdb_model *M = new sr_rrdb_model();
    M->ctx = ctx;
    M->d = *desc;
    g_rr_live.insert(M);
    for (int k = 0; k < n; ++k) {
        MfmaWeights a;
        if (k == 0) {
            a = {arrange_head_weights(h_w[k], F), std::vector<float>(h_b[k], h_b[k] + F)};
        } else if (k < n - 5) {
            const int j = (k - 1) % 5;                     // convolution j + 1 of its dense block
            if (j < 4) a = arrange_mfma_weights(h_w[k], h_b[k], G, F + j * G, 9, 8, G);
            else a = arrange_mfma_weights(h_w[k], h_b[k], F, F + 4 * G, 9, 8, 64);
        } else if (k < n - 1) {
            a = arrange_mfma_weights(h_w[k], h_b[k], F, F, 9, 8, 64);
        } else {
            a = arrange_mfma_weights(h_w[k], h_b[k], 3, F, 9, 8, 32);
        }
        if ((rc = upload_conv("sr_rrdb_create", *M, a))) {
            sr_rrdb_destroy(M);
            return rc;
        }
    }
    *out = M;
    return SR_OK;
}

int sr_rrdb_destroy(sr_rrdb_model *m)
{
    return destroy_model(m, g_rr_live);
}

int sr_rrdb_plan(const sr_rrdb_desc *desc, int h, int w, int tile, int tail, int *halo, int *n_tiles, int *n_tail_tiles,
                 size_t *workspace_bytes)
{
    int rc = rr_check_desc("sr_rrdb_plan", desc);
    if (rc) return rc;
    RrGeom g;
    rc = rr_geometry("sr_rrdb_plan", *desc, h, w, tile, tail, g);
    if (rc) return rc;
    if (halo) *halo = g.halo;
    if (n_tiles) *n_tiles = g.tiles_x * g.tiles_y;
    if (n_tail_tiles) *n_tail_tiles = (int)g.tail_tiles;
    if (workspace_bytes) *workspace_bytes = g.workspace_floats * sizeof(float);
    return SR_OK;
}

int sr_rrdb_u8(sr_rrdb_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride, int tile,
               int tail)
{
    return rr_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tile, tail, true, "sr_rrdb_u8");
}

int sr_rrdb_f32(sr_rrdb_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride, int tile,
                int tail)
{
    return rr_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tile, tail, false, "sr_rrdb_f32");
}

int sr_rrdb_ens_u8(sr_rrdb_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride, int tile,
                   int tail, int mask)
{
    return rr_ensemble(model, d_src, src_stride, h, w, d_dst, dst_stride, tile, tail, mask, true, "sr_rrdb_ens_u8");
}

int sr_rrdb_ens_f32(sr_rrdb_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride, int tile,
                    int tail, int mask)
{
    return rr_ensemble(model, d_src, src_stride, h, w, d_dst, dst_stride, tile, tail, mask, false, "sr_rrdb_ens_f32");
}

}  // extern "C"
