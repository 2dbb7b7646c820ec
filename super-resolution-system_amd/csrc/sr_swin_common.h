// sr_swin_common.h -- what the Swin-trunk backends (sr_swinir.hip, sr_hat.hip) share on the device side: the head from a padded
// u8 image, the LayerNorm, the linear layers and the 3 x 3 convolutions (sr_conv_mfma.h's mainloop behind their epilogues) and
// the weight arrangement.  Everything sits in an anonymous namespace: every unit that includes this header gets its own copy of
// the kernels, exactly as if they were written there.  Internal: nothing here is part of the C ABI.
#pragma once
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

}  // namespace
