// sr_swin_common.h -- what the Swin-trunk backends (sr_swinir.hip, sr_hat.hip, sr_swin2sr.hip) share on the device side: the
// symmetric reflection (SwinIR, Swin2SR), the head from a padded u8 image, the LayerNorm -- and the LayerNorm behind a skip
// (Swin2SR) --, the linear layers and the 3 x 3 convolutions (sr_conv_mfma.h's mainloop behind their epilogues) and the weight
// arrangement -- and, below them, the frame of a family around its own blocks: the model base and its workspace
// (SwModelBase, sw_reserve, sw_fill_workspace), the trunk phase's steps (SwTrunk), the forward (sw_forward_frame), the tail phase
// (sw_run_tail), the create (sw_create, sw_arrange_shared), the ensemble wrapper, the bias gather, the launch by head width and
// the inspection calls of the attention kernels.  A family keeps its kernels, the body of one group, its own table kinds and
// its entry points.  Everything sits in an anonymous namespace: every unit that includes this header gets its own copy of
// the kernels, exactly as if they were written there.  Internal: nothing here is part of the C ABI.
#pragma once
#include <array>
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_net_common.h"
#include "sr_swinir.h"

namespace {

struct SwAffine {
    float mean[3];
    float range;
};

// Head (3 -> C) from the padded u8 image, as k_rc_head: the 3 x 256 input values tabulated with the contract's fp32 arithmetic.
__global__ __launch_bounds__(256) void k_sw_head(const unsigned char *__restrict__ img, long long stride, int H, int W,
                                                 const float *__restrict__ wt, const float *__restrict__ bias, SwAffine af,
                                                 float *__restrict__ out, int rows, int cols, int pitch, long long plane)
{
    __shared__ float lut[3][256];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    {
        const float v = (float)tid / 255.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) lut[c][tid] = (v - af.mean[c]) * af.range;
    }
    __syncthreads();
    head_frame<256>(img, stride, H, W, wt, bias, &lut[0][0], out, 0, 0, rows, cols, pitch, plane, [](int, float y) { return y; });
}

// ---------------------------------------------------------------------------------------------------------------
// Symmetric reflection of the u8 image to Hp x Wp (dense, 3 Wp bytes per row): padded index i reads m = i mod 2 n,
// m < n ? m : 2 n - 1 - m (np.pad mode 'symmetric': the edge pixel repeated, period 2 n).  One thread per output byte.  A
// template (launched as k_sw_reflect<>) so that only a unit that launches it carries it: SwinIR and Swin2SR, not HAT.
// ---------------------------------------------------------------------------------------------------------------
template <typename Px = unsigned char>
__global__ __launch_bounds__(256) void k_sw_reflect(const Px *__restrict__ img, long long stride, int h, int w, Px *__restrict__ out, int hp,
                                                    int wp)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)hp * wp * 3) return;
    const int c = (int)(i % 3), x = (int)((i / 3) % wp), y = (int)(i / (3LL * wp));
    int my = y % (2 * h), mx = x % (2 * w);
    if (my >= h) my = 2 * h - 1 - my;
    if (mx >= w) mx = 2 * w - 1 - mx;
    out[i] = img[(size_t)my * stride + (size_t)mx * 3 + c];
}

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm over the C channels of every token of a planar tensor, one thread per token (coalesced across tokens):
//   mean = (sum_c (double)x[c]) / C;  var = (sum_c ((double)x[c] - mean)^2) / C   (float64, channels ascending, two passes,
//   the square rounded before it is added);  y[c] = (float)(((double)x[c] - mean) * (1 / sqrt(var + 1e-5)) * gamma[c] + beta[c])
//   -- every operation a rounded float64 one, left to right, one rounding to fp32 at the end.  Planes C .. Cp - 1 get +0.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sw_layernorm(const float *__restrict__ x, long long plane, long long pitch, int rows, int cols, int C,
                                                      int Cp, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                      float *__restrict__ out, long long oplane, long long opitch)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)rows * cols) return;
    const int y = (int)(idx / cols), xx = (int)(idx % cols);
    const float *p = x + (size_t)y * pitch + xx;
    float *o = out + (size_t)y * opitch + xx;
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += (double)p[(size_t)c * plane];
    const double mean = s / (double)C;
    double v = 0.0;
    for (int c = 0; c < C; ++c) {
        const double d = (double)p[(size_t)c * plane] - mean;
        v += d * d;
    }
    const double rstd = 1.0 / sqrt(v / (double)C + 1e-5);
    for (int c = 0; c < C; ++c) o[(size_t)c * oplane] = (float)(((double)p[(size_t)c * plane] - mean) * rstd * (double)gamma[c] + (double)beta[c]);
    for (int c = C; c < Cp; ++c) o[(size_t)c * oplane] = 0.0f;
}

// The same LayerNorm behind a skip (Swin2SR's post-norm): out[c] = skip[c] + (float)LN(x)[c] -- LN(.) rounded to fp32, then one
// fp32 add.  out may be skip itself (a thread reads exactly the element it then writes); x must be neither.  Planes C .. Cp - 1
// of out get +0.  A template (launched as k_sw_layernorm_add<>) so that only a unit that launches it carries it.
template <typename Skip = float>
__global__ __launch_bounds__(256) void k_sw_layernorm_add(const float *__restrict__ x, long long plane, long long pitch, int rows, int cols, int C,
                                                          int Cp, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                          const Skip *skip, long long splane, long long spitch, float *out,
                                                          long long oplane, long long opitch)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)rows * cols) return;
    const int y = (int)(idx / cols), xx = (int)(idx % cols);
    const float *p = x + (size_t)y * pitch + xx;
    const Skip *sk = skip + (size_t)y * spitch + xx;
    float *o = out + (size_t)y * opitch + xx;
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += (double)p[(size_t)c * plane];
    const double mean = s / (double)C;
    double v = 0.0;
    for (int c = 0; c < C; ++c) {
        const double d = (double)p[(size_t)c * plane] - mean;
        v += d * d;
    }
    const double rstd = 1.0 / sqrt(v / (double)C + 1e-5);
    for (int c = 0; c < C; ++c) {
        const float ln = (float)(((double)p[(size_t)c * plane] - mean) * rstd * (double)gamma[c] + (double)beta[c]);
        o[(size_t)c * oplane] = sk[(size_t)c * splane] + ln;
    }
    for (int c = C; c < Cp; ++c) o[(size_t)c * oplane] = 0.0f;
}

// What an epilogue needs beside the convolution's own arguments.
struct SwEpi {
    const float *skip;             // *_ADD: planar, element (c, gy, gx) at skip[c * skip_plane + (gy - skip_ya) * skip_pitch + gx - skip_xa]
    long long skip_plane;          //        (may be the output buffer itself: a thread reads the element it then writes)
    int skip_pitch, skip_ya, skip_xa;
    float slope;                   // SW_ACT, SW_REP_ACT
    float qscale;                  // SL_QKV: couts below nq are multiplied by it
    int nq;
    int s;                         // SW_LAST_*: the shuffle factor of the HWC store (1: none)
    SwAffine af;                   // SW_LAST_*
    void *dst;                     // SW_LAST_*: HWC output, u8 or fp32
    long long dst_stride;          // bytes
};

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// ---------------------------------------------------------------------------------------------------------------
// A linear layer over the tokens of a planar tensor: conv_mfma_mainloop<1, SW_LIN_CC, 2, true> plus an epilogue.
//   SL_PLAIN   planar store
//   SL_QKV     couts below ep.nq (the q third) times ep.qscale -- one fp32 multiply after the bias-first sum -- planar store
//   SL_GELU    0.5 y (1 + erff(y * 0.70710678f)), planar store                       (fc1)
//   SL_ADD     y + skip, planar store                                                (proj, fc2)
// ---------------------------------------------------------------------------------------------------------------
enum { SL_PLAIN = 0, SL_QKV = 1, SL_GELU = 2, SL_ADD = 3 };

template <int EPI>
__global__ __launch_bounds__(256) void k_sw_lin(const float *__restrict__ in, long long in_plane, int in_pitch, int in_ya, int in_xa, int in_rows,
                                                int in_cols, int H_in, int W_in, int cin, const float *__restrict__ wslab,
                                                const float *__restrict__ bias, float *out, long long out_plane, int out_pitch, int out_ya,
                                                int out_xa, int rows, int cols, SwEpi ep)
{
    constexpr int NC2 = 2, NC = 64;
    const MfmaLane ln = mfma_lane();
    const int half = ln.half, ct = ln.ct;
    f32x16 acc[NC2][2];
    conv_mfma_mainloop<1, SW_LIN_CC, NC2, true>(ln, in, in_plane, in_pitch, in_ya, in_xa, in_rows, in_cols, H_in, W_in, cin, wslab, bias, out_ya,
                                                out_xa, acc);
    const int col = ln.ox0 + ln.l32;
    if (col >= cols) return;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        const int row = ln.oy0 + 2 * ln.wave + pr;
        if (row >= rows) continue;
        const size_t so = EPI == SL_ADD ? skip_offset(out_ya + row, out_xa + col, ep.skip_ya, ep.skip_xa, ep.skip_pitch) : 0;
#pragma unroll
        for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = ct * NC + mfma_cout(c2, r, half);
                float y = acc[c2][pr][r];
                if constexpr (EPI == SL_QKV) y = co < ep.nq ? y * ep.qscale : y;
                if constexpr (EPI == SL_GELU) y = gelu_erf(y);
                if constexpr (EPI == SL_ADD) y = y + ep.skip[(size_t)co * ep.skip_plane + so];
                out[(size_t)co * out_plane + (size_t)row * out_pitch + col] = y;
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 3 x 3 convolution: conv_mfma_mainloop<3, 8, NC2, true> plus an epilogue; NC2 = 32-cout halves per block.
//   SW_ADD       y + skip, planar store                                     (an RSTB's convolution, conv_after_body)
//   SW_ACT       y >= 0 ? y : slope y, planar store                         (conv_before_upsample, conv_up2, conv_hr)
//   SW_REP_ACT   the same stored 2 x 2 replicated at twice the resolution   (nearest+conv: conv_before_upsample, conv_up1)
//   SW_SHUF2/3   PixelShuffle(r) into the planar output at r x the resolution, as sr_rcan.hip's RC_SHUF*
//   SW_LAST_*    one cout tile; cout co < 3 s^2 is channel co / s^2 at (s row + (co % s^2) / s, s col + co % s) of the HWC
//                output (s = ep.s; 1: conv_last), o = y / range + mean (u8: clamp, scale, round half even)
//   SW_GELU      gelu_erf(y), planar store                                  (HAT: the CAB's first convolution)
//   SW_PLAIN     planar store                                               (HAT: the CAB's second convolution)
// ---------------------------------------------------------------------------------------------------------------
enum { SW_ADD = 0, SW_ACT = 1, SW_REP_ACT = 2, SW_SHUF2 = 3, SW_SHUF3 = 4, SW_LAST_F32 = 5, SW_LAST_U8 = 6, SW_GELU = 7, SW_PLAIN = 8 };

template <int NC2, int EPI>
__global__ __launch_bounds__(256) void k_sw_conv(const float *__restrict__ in, long long in_plane, int in_pitch, int in_ya, int in_xa,
                                                 int in_rows, int in_cols, int H_in, int W_in, int cin, const float *__restrict__ wslab,
                                                 const float *__restrict__ bias, float *out, long long out_plane, int out_pitch,
                                                 int out_ya, int out_xa, int rows, int cols, SwEpi ep)
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
        if constexpr (EPI == SW_ADD) {
            const size_t so = skip_offset(out_ya + row, out_xa + col, ep.skip_ya, ep.skip_xa, ep.skip_pitch);
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    const float sk = ep.skip[(size_t)co * ep.skip_plane + so];
                    out[(size_t)co * out_plane + (size_t)row * out_pitch + col] = acc[c2][pr][r] + sk;
                }
        } else if constexpr (EPI == SW_ACT) {
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    out[(size_t)co * out_plane + (size_t)row * out_pitch + col] = leaky(acc[c2][pr][r], ep.slope);
                }
        } else if constexpr (EPI == SW_GELU || EPI == SW_PLAIN) {
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    float y = acc[c2][pr][r];
                    if constexpr (EPI == SW_GELU) y = gelu_erf(y);
                    out[(size_t)co * out_plane + (size_t)row * out_pitch + col] = y;
                }
        } else if constexpr (EPI == SW_REP_ACT) {
            const size_t oo = (size_t)(2 * row) * out_pitch + 2 * col;     // out_pitch and out_plane are even: 8-byte aligned
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    const float v = leaky(acc[c2][pr][r], ep.slope);
                    float *o = out + (size_t)co * out_plane + oo;
                    const float2 vv = make_float2(v, v);
                    *(float2 *)o = vv;
                    *(float2 *)(o + out_pitch) = vv;
                }
        } else if constexpr (EPI == SW_SHUF2 || EPI == SW_SHUF3) {
            constexpr int R = EPI == SW_SHUF2 ? 2 : 3;
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + mfma_cout(c2, r, half);
                    const int c = co / (R * R), rem = co % (R * R), dy = rem / R, dx = rem % R;
                    out[(size_t)c * out_plane + ((size_t)row * R + dy) * out_pitch + (size_t)col * R + dx] = acc[c2][pr][r];
                }
        } else {                                           // output affine + shuffled HWC store
            const int s = ep.s, ss = s * s;
            const int gy = (out_ya + row) * s, gx = (out_xa + col) * s;
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = mfma_cout(c2, r, half);
                    if (co >= 3 * ss) continue;
                    const int c = co / ss, rem = co % ss, dy = rem / s, dx = rem % s;
                    const float mean = c == 0 ? ep.af.mean[0] : (c == 1 ? ep.af.mean[1] : ep.af.mean[2]);
                    const float o = acc[c2][pr][r] / ep.af.range + mean;
                    char *d = (char *)ep.dst + (size_t)(gy + dy) * ep.dst_stride;
                    store_hwc<EPI == SW_LAST_U8>(d, (size_t)(gx + dx) * 3 + c, o);
                }
        }
    }
}

inline void sw_launch_layernorm(hipStream_t st, const float *x, long long plane, long long pitch, int rows, int cols, int C, int Cp,
                                const float *gamma, const float *beta, float *out, long long oplane, long long opitch)
{
    const long long n = (long long)rows * cols;
    hipLaunchKernelGGL(k_sw_layernorm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, plane, pitch, rows, cols, C, Cp, gamma, beta, out,
                       oplane, opitch);
}

// Convolution weights [cout][cin][T] with cin zero-padded to cin_pad -> the mainloop's layout.
inline MfmaWeights sw_arrange(const float *w, const float *b, int cout, int cin, int T, int cin_pad, int CC, int NC)
{
    std::vector<float> p((size_t)cout * cin_pad * T, 0.0f);
    for (int co = 0; co < cout; ++co)
        std::memcpy(&p[(size_t)co * cin_pad * T], w + (size_t)co * cin * T, (size_t)cin * T * sizeof(float));
    return arrange_mfma_weights(p.data(), b, cout, cin_pad, T, CC, NC);
}

// What the inspection entry points check of a planar view.
inline int sw_check_view(const char *who, const void *p, int64_t plane_stride, int64_t row_stride, int h, int w)
{
    if (row_stride < (int64_t)w * 4 || plane_stride < row_stride * h) return sr_set_error(SR_ERR_SHAPE, "%s: a stride is smaller than what it spans", who);
    if (row_stride % 4 || plane_stride % 4 || (uintptr_t)p % 4)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: the pointers and the strides must be multiples of 4 bytes", who);
    if (row_stride / 4 > INT_MAX) return sr_set_error(SR_ERR_SHAPE, "%s: a row stride beyond int", who);
    return SR_OK;
}

// ===============================================================================================================
// The frame of a family: the model, the workspace, the trunk phase around the family's own blocks, the tail phase, the
// create, the ensemble and the inspection calls.  A family's model derives from SwModelBase and adds
//   d                                       its description (n_feat, n_heads, n_hidden, n_groups, depth, scale, mean, range)
//   SHUFFLE_ONLY                            whether its reconstruction is always the pixelshuffle one
//   PROJECTED                               whether a 1 x 1 projection follows the head and every group's convolution (Swin2SR)
//   check_desc, table_list, bias_table      (static) its description check, its tables, the kinds whose bias entry is ignored
//   geometry, tail_steps                    its plan
// Everything is resolved at compile time: no std::function and no virtual call on the launch path.
// ===============================================================================================================
struct SwModelBase : SrModelBase {             // d_w, d_b: per table
    std::vector<SwTable> tables;
    DevBuf trunk[5];                          // H, R, X, A and (HAT) U: the first SwGeom::trunk_bufs are in use
    DevBuf tbuf;                              // HAT: the CAB's middle tensor
    DevBuf qbuf;                              // qkv / hidden
    DevBuf tailbuf[2];
    DevBuf img;                               // the reflected u8 image
    DevBuf red;                               // HAT: C x chunks float64 chunk sums, then s[C]
    std::array<DevBuf *, 11> buffers()
    {
        return {&trunk[0], &trunk[1], &trunk[2], &trunk[3], &trunk[4], &tbuf, &qbuf, &tailbuf[0], &tailbuf[1], &img, &red};
    }
    void release_device()
    {
        for (DevBuf *b : buffers()) b->release();
        release_base();
    }
};

inline int sw_reserve(SwModelBase *m, const SwGeom &g, const char *who)
{
    sr_ctx *ctx = m->ctx;
    int rc;
    if ((rc = ensure_activation_buffers(ctx, m->trunk, g.trunk_bufs, (size_t)g.plane0 * g.cp, who))) return rc;
    if (g.tp && (rc = ensure_activation_buffers(ctx, &m->tbuf, 1, (size_t)g.plane0 * g.tp, who))) return rc;
    if ((rc = ensure_activation_buffers(ctx, &m->qbuf, 1, (size_t)g.plane0 * g.qp, who))) return rc;
    if (g.plane_t && (rc = ensure_activation_buffers(ctx, m->tailbuf, 2, (size_t)g.plane_t * SW_MID, who))) return rc;
    SRCHK(m->img.reserve(ctx, who, (size_t)g.plane0 * 3));
    if (g.red_bytes) SRCHK(m->red.reserve(ctx, who, g.red_bytes));
    return SR_OK;
}

template <typename Model>
int sw_fill_workspace(const char *who, LiveSet &live, Model *m, int h, int w, int tail, int byte)
{
    if (!live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    sr_ctx *ctx = m->ctx;
    CTX_ENTER_AS(ctx, who);
    SwGeom g;
    int rc = m->geometry(who, h, w, tail, g);
    if (rc) return rc;
    if ((rc = sw_reserve(m, g, who))) return rc;
    for (DevBuf *b : m->buffers())
        if (b->d) HIPCHK(hipMemsetAsync(b->d, byte, b->cap, ctx->stream));
    return SR_OK;
}

struct SwNames {                               // a family's profile scopes
    const char *head, *ln, *linear, *conv, *tail;
};

// The trunk phase: the whole padded image, every tensor in one layout L; table k's arrays are m->w(k), m->b(k).
struct SwTrunk {
    sr_ctx *ctx;
    hipStream_t st;
    SwModelBase *m;
    SwNames nm;
    PlanarTen L;
    SwEpi ep;
    int hp, wp, C, Cp, hidp, qkvp;
    float *Hb, *Rb, *Xb, *Ab, *Qb;             // h then f;  the group's input then output;  the running x;  LN / attention output;  qkv / hidden
    PlanarTen ten(float *base) const
    {
        PlanarTen t = L;
        t.p = base;
        return t;
    }
    template <typename Kernel>
    void lin(Kernel kernel, float *in, int cin, int k, int cout_planes, float *out, const float *skip) const
    {
        ProfScope ps(ctx, nm.linear);
        SwEpi e = ep;
        e.skip = skip;
        launch_conv(kernel, st, ten(in), hp, wp, cin, cout_planes / 64, m->w(k), m->b(k), out, L.plane, L.pitch, 0, 0, hp, wp, e);
    }
    void conv(float *in, int k, float *out, const float *skip) const
    {
        ProfScope ps(ctx, nm.conv);
        SwEpi e = ep;
        e.skip = skip;
        launch_conv(k_sw_conv<2, SW_ADD>, st, ten(in), hp, wp, Cp, Cp / 64, m->w(k), m->b(k), out, L.plane, L.pitch, 0, 0, hp, wp, e);
    }
    void norm(float *in, int k, float *out) const
    {
        ProfScope ps(ctx, nm.ln);
        sw_launch_layernorm(st, in, L.plane, L.pitch, hp, wp, C, Cp, m->w(k), m->b(k), out, L.plane, L.pitch);
    }
    template <typename Kernel>
    void conv_with(Kernel kernel, float *in, int k, float *out, const float *skip) const   // a C -> C convolution behind another epilogue
    {
        ProfScope ps(ctx, nm.conv);
        SwEpi e = ep;
        e.skip = skip;
        launch_conv(kernel, st, ten(in), hp, wp, Cp, Cp / 64, m->w(k), m->b(k), out, L.plane, L.pitch, 0, 0, hp, wp, e);
    }
    void qkv(int k) const { lin(k_sw_lin<SL_QKV>, Ab, Cp, k, qkvp, Qb, nullptr); }            // A -> Q
    void proj(int k, const float *x) const { lin(k_sw_lin<SL_ADD>, Ab, Cp, k, Cp, Xb, x); }   // X = x + proj(A)
    void mlp(int k) const                                  // x = x + fc2(gelu(fc1(LN2(x)))) on X; tables k, k + 1, k + 2
    {
        norm(Xb, k, Ab);
        lin(k_sw_lin<SL_GELU>, Ab, Cp, k + 1, hidp, Qb, nullptr);
        lin(k_sw_lin<SL_ADD>, Qb, hidp, k + 2, Cp, Xb, Xb);
    }
    template <typename Reflect>
    void head(Reflect reflect, const uint8_t *d_src, int64_t src_stride, int h, int w) const   // the family's reflection, then table 0 -> H
    {
        ProfScope ps(ctx, nm.head);
        unsigned char *img = m->img.as<unsigned char>();
        const long long n = (long long)hp * wp * 3;
        hipLaunchKernelGGL(reflect, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_src, (long long)src_stride, h, w, img, hp, wp);
        hipLaunchKernelGGL(k_sw_head, dim3((wp + 63) / 64, (hp + 3) / 4, Cp / 64), dim3(64, 4), 0, st, img, (long long)wp * 3, hp, wp, m->w(0), m->b(0),
                           ep.af, Hb, hp, wp, L.pitch, L.plane);
    }
};

// The tail phase: sub-pieces of the input over their own backward extents; the tables from k on.  SHUFFLE_ONLY leaves out the
// launches only the other two reconstructions have (a unit that never runs them does not carry their kernels).
template <bool SHUFFLE_ONLY>
int sw_run_tail(const SwTrunk &T, const std::vector<SwStep> &steps, int k, int S, int h, int w, int tail, bool u8, const char *who)
{
    SwModelBase *m = T.m;
    const int n = (int)steps.size(), hp = T.hp, wp = T.wp;
    const PlanarTen f = T.ten(T.Hb);
    std::vector<int> ya, yb, xa, xb;
    int rc;
    for (int sy = 0; sy < h; sy = (int)std::min<long long>((long long)sy + tail, h))
        for (int sx = 0; sx < w; sx = (int)std::min<long long>((long long)sx + tail, w)) {
            sw_backward_extents(steps.data(), n, S, sy, (int)std::min<long long>((long long)sy + tail, h), hp, ya, yb);
            sw_backward_extents(steps.data(), n, S, sx, (int)std::min<long long>((long long)sx + tail, w), wp, xa, xb);
            PlanarTen t = f;
            ProfScope ps(T.ctx, T.nm.tail);
            for (int i = 0; i < n; ++i) {
                const int rows = yb[i] - ya[i], cols = xb[i] - xa[i], mult = steps[i].mult, r = steps[i].r, kt = k + i;
                const int kind = m->tables[kt].kind, cin = i == 0 ? T.Cp : SW_MID;
                SwEpi e = T.ep;
                e.slope = kind == SW_T_CBU ? 0.01f : 0.2f;  // read by SW_ACT and SW_REP_ACT alone
                e.s = r;
                if (i + 1 < n) {
                    const PlanarTen o = planar_tensor(m->tailbuf[i & 1].as<float>(), ya[i] * r, xa[i] * r, rows * r, cols * r);
                    auto go = [&](auto kernel, int tiles) {
                        launch_conv(kernel, T.st, t, hp * mult, wp * mult, cin, tiles, m->w(kt), m->b(kt), o.p, o.plane, o.pitch, ya[i], xa[i], rows, cols, e);
                    };
                    if (kind == SW_T_UP && r == 2) go(k_sw_conv<2, SW_SHUF2>, 4);
                    else if (kind == SW_T_UP) go(k_sw_conv<2, SW_SHUF3>, 9);
                    else if constexpr (SHUFFLE_ONLY) go(k_sw_conv<2, SW_ACT>, 1);
                    else r == 2 ? go(k_sw_conv<2, SW_REP_ACT>, 1) : go(k_sw_conv<2, SW_ACT>, 1);
                    t = o;
                } else {
                    auto go = [&](auto kernel) {
                        launch_conv(kernel, T.st, t, hp * mult, wp * mult, cin, 1, m->w(kt), m->b(kt), nullptr, 0LL, 0, ya[i], xa[i], rows, cols, e);
                    };
                    bool wide = false;                     // more than 32 couts: pixelshuffledirect at scale 4
                    if constexpr (!SHUFFLE_ONLY) wide = 3 * r * r > 32;
                    if (!wide) u8 ? go(k_sw_conv<1, SW_LAST_U8>) : go(k_sw_conv<1, SW_LAST_F32>);
                    else if constexpr (!SHUFFLE_ONLY) u8 ? go(k_sw_conv<2, SW_LAST_U8>) : go(k_sw_conv<2, SW_LAST_F32>);
                }
            }
            if ((rc = check_launch(who))) return rc;
        }
    return SR_OK;
}

// A family's forward: everything but its groups.  group(T, g, k) runs the blocks of one group from the group's input T.Rb,
// advances k past their tables and returns where the group's x lies; fn: the name a dead context is reported under.
template <typename Model, typename Reflect, typename Group>
int sw_forward_frame(const char *fn, LiveSet &live, Model *m, const SwNames &nm, Reflect reflect, const uint8_t *d_src, int64_t src_stride, int h,
                     int w, void *d_dst, int64_t dst_stride, int tail, bool u8, const char *who, Group group)
{
    if (!live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    sr_ctx *ctx = m->ctx;
    CTX_ENTER_AS(ctx, fn);
    const auto &D = m->d;
    const int C = D.n_feat, S = D.scale;
    int rc = check_sr_forward_args(who, d_src, src_stride, w, d_dst, dst_stride, S, u8);
    if (rc) return rc;
    SwGeom g;
    if ((rc = m->geometry(who, h, w, tail, g))) return rc;
    if ((rc = sw_reserve(m, g, who))) return rc;
    SwTrunk T{};
    T.ctx = ctx;
    T.st = ctx->stream;
    T.m = m;
    T.nm = nm;
    T.L = planar_tensor(nullptr, 0, 0, g.hp, g.wp);
    T.ep.af = {{D.mean[0], D.mean[1], D.mean[2]}, D.range};
    T.ep.dst = d_dst;
    T.ep.dst_stride = (long long)dst_stride;
    T.ep.s = 1;
    T.ep.nq = C;
    T.ep.qscale = 1.0f / sqrtf((float)(C / D.n_heads));
    T.ep.skip_plane = T.L.plane;
    T.ep.skip_pitch = T.L.pitch;
    T.hp = g.hp, T.wp = g.wp, T.C = C, T.Cp = g.cp, T.hidp = sw_pad64(D.n_hidden), T.qkvp = sw_pad64(3 * C);
    T.Hb = m->trunk[0].template as<float>(), T.Rb = m->trunk[1].template as<float>(), T.Xb = m->trunk[2].template as<float>();
    T.Ab = m->trunk[3].template as<float>(), T.Qb = m->qbuf.template as<float>();
    T.head(reflect, d_src, src_stride, h, w);
    int k = 1;
    if constexpr (Model::PROJECTED) {                      // Swin2SR: e = P_0 h + b, a 1 x 1 convolution, ahead of the first LayerNorm
        T.lin(k_sw_lin<SL_PLAIN>, T.Hb, T.Cp, k++, T.Cp, T.Ab, nullptr);
        T.norm(T.Ab, k++, T.Rb);
    } else {
        T.norm(T.Hb, k++, T.Rb);
    }
    for (int gi = 0; gi < D.n_groups; ++gi) {
        float *x = group(T, g, k);
        if constexpr (Model::PROJECTED) {                  // r = P_i(conv(x)) + r: the convolution into A, the projection in place over r
            T.conv_with(k_sw_conv<2, SW_PLAIN>, x, k++, T.Ab, nullptr);
            T.lin(k_sw_lin<SL_ADD>, T.Ab, T.Cp, k++, T.Cp, T.Rb, T.Rb);
        } else {
            T.conv(x, k++, T.Rb, T.Rb);                    // in place over the group's input
        }
    }
    T.norm(T.Rb, k++, T.Ab);
    T.conv(T.Ab, k++, T.Hb, T.Hb);                         // f = conv_after_body(.) + h, in place over h
    if ((rc = check_launch(who))) return rc;
    return sw_run_tail<Model::SHUFFLE_ONLY>(T, m->tail_steps(), k, S, h, w, g.tail, u8, who);
}

// The self-ensemble over a family's forward fwd (driver: sr_ensemble.hip): every member is padded and windowed on its own.
template <typename Model, typename Forward>
int sw_ensemble(LiveSet &live, Model *m, Forward fwd, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride,
                int tail, int mask, bool u8, const char *who)
{
    const int rc = sr_ens_check_mask(who, mask);
    if (rc) return rc;
    if (tail < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: %s must be >= 1, or 0 for the library's choice", who, "tail");
    if (!live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    return ens_run(who, *m, m->d.scale, [&](const uint8_t *s, int64_t ss, int hh, int ww, float *d, int64_t ds) {
        return fwd(m, s, ss, hh, ww, d, ds, tail, false, who);
    }, d_src, src_stride, h, w, d_dst, dst_stride, mask, u8);
}

// The tables of the kinds both families have -> the kernels' layouts; false: the kind is the family's own.
inline bool sw_arrange_shared(const SwTable &t, const float *w, const float *b, int C, int hidden, MfmaWeights &a)
{
    const int Cp = sw_pad64(C);
    switch (t.kind) {
    case SW_T_HEAD: {
        std::vector<float> wpad((size_t)Cp * 27, 0.0f);
        std::memcpy(wpad.data(), w, (size_t)C * 27 * sizeof(float));
        a.w = arrange_head_weights(wpad.data(), Cp);
        a.b.assign(Cp, 0.0f);
        std::memcpy(a.b.data(), b, (size_t)C * sizeof(float));
        return true;
    }
    case SW_T_LN:
        a = {std::vector<float>(w, w + C), std::vector<float>(b, b + C)};
        return true;
    case SW_T_QKV: case SW_T_PROJ: case SW_T_FC1:
        a = sw_arrange(w, b, t.cout, t.cin, 1, Cp, SW_LIN_CC, 64);
        return true;
    case SW_T_FC2:
        a = sw_arrange(w, b, t.cout, t.cin, 1, sw_pad64(hidden), SW_LIN_CC, 64);
        return true;
    case SW_T_CONV: case SW_T_CBU:
        a = sw_arrange(w, b, t.cout, t.cin, 9, Cp, 8, 64);
        return true;
    case SW_T_UP:
        a = sw_arrange(w, b, t.cout, t.cin, 9, SW_MID, 8, 64);
        return true;
    case SW_T_LAST:
        a = sw_arrange(w, b, t.cout, t.cin, 9, SW_MID, 8, 32);
        return true;
    }
    return false;
}

// The body of a family's create.  pre(): what the family checks of its further arguments before the context is entered;
// own(t, w, b, a): arranges a table of one of the family's own kinds and returns true, or returns false.
template <typename Model, typename Desc, typename Pre, typename Own>
int sw_create(const char *who, sr_ctx *ctx, const Desc *desc, const float *const *h_w, const float *const *h_b, int n_tables, LiveSet &live,
              Model **out, Pre pre, Own own)
{
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null out", who);
    *out = nullptr;
    int rc = Model::check_desc(who, desc);                                  // host decision, before any device call
    if (rc) return rc;
    const std::vector<SwTable> tables = Model::table_list(*desc);
    if (!h_w || !h_b) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null weight table", who);
    if (n_tables != (int)tables.size())
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: this description has %d tables, %d given", who, (int)tables.size(), n_tables);
    for (int k = 0; k < n_tables; ++k)
        if (!h_w[k] || (!h_b[k] && !Model::bias_table(tables[k].kind))) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null array of table %d", who, k);
    if ((rc = pre())) return rc;
    CTX_ENTER_AS(ctx, who);
    Model *M = new Model();
    M->ctx = ctx;
    M->d = *desc;
    M->tables = tables;
    live.insert(M);
    for (int k = 0; k < n_tables; ++k) {
        MfmaWeights a;
        if (!own(tables[k], h_w[k], h_b[k], a)) sw_arrange_shared(tables[k], h_w[k], h_b[k], desc->n_feat, desc->n_hidden, a);
        if ((rc = upload_conv(who, *M, a))) {
            destroy_model(M, live);
            return rc;
        }
    }
    *out = M;
    return SR_OK;
}

// A bias table [rows][heads] gathered through idx [nq][nk] to [head][key j][query i].
inline std::vector<float> sw_gather_bias(const float *table, const int *idx, int nk, int nq, int heads)
{
    std::vector<float> g((size_t)heads * nk * nq);
    for (int hd = 0; hd < heads; ++hd)
        for (int j = 0; j < nk; ++j)
            for (int i = 0; i < nq; ++i) g[((size_t)hd * nk + j) * nq + i] = table[(size_t)idx[i * nk + j] * heads + hd];
    return g;
}

inline std::vector<float> sw_gather_window_bias(const float *table, int win, int heads)     // through sw_rel_index(win)
{
    std::vector<int> rel((size_t)win * win * win * win);
    sw_rel_index(win, rel.data());
    return sw_gather_bias(table, rel.data(), win * win, win * win, heads);
}

// One of four instantiations of an attention kernel by the head width d (their LDS holds d rounded up to a multiple of 8).
template <typename Kernel, typename... Args>
void sw_launch_by_d(int d, Kernel k8, Kernel k16, Kernel k24, Kernel k32, dim3 grid, dim3 block, hipStream_t st, Args... args)
{
    const Kernel kernel = d <= 8 ? k8 : d <= 16 ? k16 : d <= 24 ? k24 : k32;
    hipLaunchKernelGGL(kernel, grid, block, 0, st, args...);
}

// The inspection entry points of the attention kernels: first the arguments every one of them checks first ...
inline int sw_check_attention_args(const char *who, const void *d_qkv, const void *h_table, const void *d_out, int C, int n_heads)
{
    if (!d_qkv || !h_table || !d_out) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    if (C < 1 || C > 256 || n_heads < 1 || C % n_heads || C / n_heads > 32)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d channels in %d heads is outside C <= 256, heads of at most 32 channels", who, C, n_heads);
    return SR_OK;
}

inline int sw_check_windows(const char *who, int hp, int wp, int win)
{
    if (hp < win || wp < win || hp % win || wp % win)
        return sr_set_error(SR_ERR_SHAPE, "%s: a %dx%d tensor is not made of %d x %d windows", who, wp, hp, win, win);
    return SR_OK;
}

// ... then, once the family's own checks have passed: the two views, the index [nq][nk] of the bias table (index(idx) -> rc),
// the upload of the gathered table, launch(stream, qkv, plane, pitch, bias, out, oplane, opitch) with the strides in floats,
// and the sync.
template <typename Index, typename Launch>
int sw_run_attention(const char *who, sr_ctx *ctx, const float *d_qkv, int64_t plane_stride, int64_t row_stride, int n_heads, int hp, int wp,
                     const float *h_table, int nk, int nq, float *d_out, int64_t out_plane_stride, int64_t out_row_stride, Index index,
                     Launch launch)
{
    int rc;
    if ((rc = sw_check_view(who, d_qkv, plane_stride, row_stride, hp, wp))) return rc;
    if ((rc = sw_check_view(who, d_out, out_plane_stride, out_row_stride, hp, wp))) return rc;
    std::vector<int> idx((size_t)nq * nk);
    if ((rc = index(idx.data()))) return rc;
    CTX_ENTER_AS(ctx, who);
    const std::vector<float> g = sw_gather_bias(h_table, idx.data(), nk, nq, n_heads);
    DevTemp tmp(ctx);
    SRCHK(tmp.alloc(who, g.size() * sizeof(float)));
    HIPCHK(hipMemcpyAsync(tmp.d, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    launch(ctx->stream, d_qkv, (long long)(plane_stride / 4), (int)(row_stride / 4), tmp.as<float>(), d_out, (long long)(out_plane_stride / 4),
           (int)(out_row_stride / 4));
    SRCHK(check_launch(who));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // namespace
