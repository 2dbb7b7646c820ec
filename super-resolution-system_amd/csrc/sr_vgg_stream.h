// sr_vgg_stream.h -- what the tile-streamed feature-stack metrics (sr_lpips.hip, sr_dists.hip) share: the layer tables and their
// per-tile range algebra (sr_vgg_ranges.h, host only), the u8 stem convolution (parameterised by the formula of its 3 x 256 input table), the fp32-MFMA
// convolution + ReLU, and the fixed-order partial accumulate.  Internal: nothing here is part of the C ABI.  Everything sits in
// an unnamed namespace: each including unit owns its copy of the kernels.
#pragma once
#include <algorithm>
#include <vector>

#include "sr_conv_mfma.h"
#include "sr_vgg_ranges.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// Stem convolution (Cin = 3) straight from the u8 image: one thread = one output pixel x 64 output channels.
// The network input of channel c at u8 value v is tab(c, v) inside the image, 0 outside (Conv2d zero padding acts on the
// preprocessed value).  Tab is the metric's preprocessing, a device functor of fp32 operations; the 3 x 256 possible values
// are tabulated in LDS once per block with exactly those operations.  Weights are laid out [c][tap][64] so the 64
// multipliers of one input value are wave-uniform (scalar loads), the inner loop is 64 v_fmac with an SGPR operand.
// ---------------------------------------------------------------------------------------------------------------
template <int KS, int S, int P, typename Tab>
__global__ __launch_bounds__(256) void k_lp_conv_stem(const unsigned char *__restrict__ img, long long stride, int cn,
                                                      int H, int W, const float *__restrict__ wt,
                                                      const float *__restrict__ bias, Tab tab, float *__restrict__ out, int ya,
                                                      int xa, int rows, int cols, int pitch, long long plane)
{
    __shared__ float lut[3][256];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    for (int i = tid; i < 768; i += 256) {
        const int c = i >> 8, v = i & 255;
        lut[c][v] = tab(c, v);
    }
    __syncthreads();
    const int lx = blockIdx.x * 64 + threadIdx.x, ly = blockIdx.y * 4 + threadIdx.y;
    if (lx >= cols || ly >= rows) return;
    const int oy = ya + ly, ox = xa + lx;
    float acc[64];
#pragma unroll
    for (int co = 0; co < 64; ++co) acc[co] = bias[co];
    constexpr int T = KS * KS;
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        const int cs = cn == 1 ? 0 : c;              // gray is repeated, alpha (cn == 4) is dropped
#pragma unroll 1
        for (int ky = 0; ky < KS; ++ky) {
            const int gy = oy * S - P + ky;
            const bool yok = gy >= 0 && gy < H;
            const unsigned char *row = img + (size_t)(yok ? gy : 0) * stride;
#pragma unroll 1
            for (int kx = 0; kx < KS; ++kx) {
                const int gx = ox * S - P + kx;
                float v = 0.0f;
                if (yok && gx >= 0 && gx < W) v = lut[c][row[(size_t)gx * cn + cs]];
                const float *wp = wt + ((size_t)c * T + ky * KS + kx) * 64;
#pragma unroll
                for (int co = 0; co < 64; ++co) acc[co] = fmaf(wp[co], v, acc[co]);
            }
        }
    }
    float *o = out + (size_t)ly * pitch + lx;
#pragma unroll
    for (int co = 0; co < 64; ++co) o[(size_t)co * plane] = fmaxf(acc[co], 0.0f);
}

// ---------------------------------------------------------------------------------------------------------------
// Implicit-GEMM convolution + bias + ReLU on v_mfma_f32_32x32x2_f32, stride 1, KS x KS, zero padding P = KS / 2:
// conv_mfma_mainloop<KS, CC, 2, true> (sr_conv_mfma.h states the GEMM view, the block shape, the LDS staging and the
// summation order) plus a ReLU epilogue.  Block = 4 waves = 8 output rows x 32 columns x 64 couts.  GUARD is on: the input
// buffer holds in_rows x in_cols (the needed range of the tile), and a partial block at the edge of a tile would otherwise
// stage elements past it -- past the allocation itself where the activation is the largest of the tile.  Only masked outputs
// read those elements, so the guard changes no result.
// ---------------------------------------------------------------------------------------------------------------
template <int KS, int CC>
__global__ __launch_bounds__(256) void k_lp_conv_mfma(const float *__restrict__ in, long long in_plane, int in_pitch,
                                                      int in_ya, int in_xa, int in_rows, int in_cols, int H_in, int W_in, int cin,
                                                      const float *__restrict__ wslab, const float *__restrict__ bias,
                                                      float *__restrict__ out, long long out_plane, int out_pitch,
                                                      int out_ya, int out_xa, int rows, int cols)
{
    const MfmaLane ln = mfma_lane();
    f32x16 acc[2][2];
    conv_mfma_mainloop<KS, CC, 2, true>(ln, in, in_plane, in_pitch, in_ya, in_xa, in_rows, in_cols, H_in, W_in, cin, wslab, bias, out_ya, out_xa, acc);
    // epilogue: ReLU, masked store
    const int col = ln.ox0 + ln.l32;
    if (col >= cols) return;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        const int row = ln.oy0 + 2 * ln.wave + pr;
        if (row >= rows) continue;
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = ln.ct * 64 + mfma_cout(c2, r, ln.half);
                out[(size_t)co * out_plane + (size_t)row * out_pitch + col] = fmaxf(acc[c2][pr][r], 0.0f);
            }
    }
}

__device__ __forceinline__ double lp_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// acc[j] += sum(part[j * n .. (j + 1) * n)) in a fixed order, one block per output j = blockIdx.x
__global__ __launch_bounds__(256) void k_lp_accum(const double *__restrict__ part, long long n, double *__restrict__ acc)
{
    __shared__ double sh[256];
    part += (size_t)blockIdx.x * n;
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) s += part[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) acc[blockIdx.x] += sh[0];
}

}  // namespace
