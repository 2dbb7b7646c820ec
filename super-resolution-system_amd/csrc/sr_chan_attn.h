// sr_chan_attn.h -- the channel attention that sr_rcan.hip (an RCAB) and sr_hat.hip (a CAB) share: the float64 channel mean in a
// fixed order, the two 1 x 1 layers with the sigmoid, and the scale-and-skip pass.  Everything sits in an anonymous namespace:
// every unit that includes this header gets its own copy of the kernels, exactly as if they were written there.  Internal.
//
// The channel mean (the order every restatement follows): the image's rows are cut into chunks of RC_ROWS = 32.  One block of
// 256 threads per (channel, chunk): thread t adds, in float64, rows ascending and within a row the columns t, t + 256, ..
// ascending -- valid pixels only, never a padded column; the 256 sums are then folded in LDS, a[t] += a[t + k] for
// k = 128, 64, .. 1.  The attention kernel adds a channel's chunk sums in ascending chunk order to S, and
// m[c] = (float)(S / (double)(h w)).  No atomics.  Then z1[j] = max(b1[j] + sum_c w1[j][c] m[c], 0) and
// z[c] = b2[c] + sum_j w2[c][j] z1[j] in float64, ascending index, each term one rounded multiply and one rounded add (the
// first layer's products of two fp32 values are exact), and s[c] = (float)(1 / (1 + exp(-z[c]))).
#pragma once
#include <cmath>

#include "sr_net_common.h"

namespace {

constexpr int RC_ROWS = 32;

// ---------------------------------------------------------------------------------------------------------------
// Row-chunk sums of a planar tensor, float64.  grid (chunks, F), block 256: block (k, c) sums plane c over the rows
// [k RC_ROWS, min((k + 1) RC_ROWS, h)) and the columns [0, w) in the order written at the top of this file and stores
// part[c * chunks + k].  plane / pitch in floats.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rc_rowsum(const float *__restrict__ x, long long plane, long long pitch, int h, int w,
                                                   double *__restrict__ part)
{
    __shared__ double a[256];
    const int t = threadIdx.x, k = blockIdx.x, c = blockIdx.y;
    const int r0 = k * RC_ROWS, r1 = min(r0 + RC_ROWS, h);
    const float *p = x + (size_t)c * plane;
    double s = 0.0;
    for (int r = r0; r < r1; ++r) {
        const float *row = p + (size_t)r * pitch;
        for (int col = t; col < w; col += 256) s += (double)row[col];
    }
    a[t] = s;
    __syncthreads();
#pragma unroll
    for (int k2 = 128; k2 >= 1; k2 >>= 1) {
        if (t < k2) a[t] += a[t + k2];
        __syncthreads();
    }
    if (t == 0) part[(size_t)c * gridDim.x + k] = a[0];
}

// ---------------------------------------------------------------------------------------------------------------
// The channel attention of one block, one block of 256 threads (F <= 256, R <= F): the ordered sum of a channel's chunk sums,
// the mean, the two 1 x 1 layers and the sigmoid in float64; s[F] (and mean[F] where asked) to device memory.
// w1 [R][F], w2 [F][R] dense fp32.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rc_attention(const double *__restrict__ part, int chunks, double count, int F, int R,
                                                      const float *__restrict__ w1, const float *__restrict__ b1,
                                                      const float *__restrict__ w2, const float *__restrict__ b2,
                                                      float *__restrict__ s_out, float *__restrict__ mean_out)
{
    __shared__ float m[256];
    __shared__ double z1[256];
    const int t = threadIdx.x;
    if (t < F) {
        const double *p = part + (size_t)t * chunks;
        double S = 0.0;
        for (int k = 0; k < chunks; ++k) S += p[k];
        m[t] = (float)(S / count);
        if (mean_out) mean_out[t] = m[t];
    }
    __syncthreads();
    if (t < R) {
        double z = (double)b1[t];
        for (int c = 0; c < F; ++c) z += (double)w1[(size_t)t * F + c] * (double)m[c];
        z1[t] = z > 0.0 ? z : 0.0;
    }
    __syncthreads();
    if (t < F) {
        double z = (double)b2[t];
        for (int j = 0; j < R; ++j) z += (double)w2[(size_t)t * R + j] * z1[j];
        s_out[t] = (float)(1.0 / (1.0 + exp(-z)));
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Scale-and-skip: out[c] = fmaf(res_scale, y2[c] * s[c], t[c]) over whole planes (padded columns included: they are never
// read as pixels), four floats per thread; the product is rounded to fp32 first.  grid (ceil(plane4 / 256), F); out may be t.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rc_scale(const float4 *__restrict__ y2, const float *__restrict__ s, const float4 *t, float4 *out,
                                                  long long plane4, float res_scale)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= plane4) return;
    const size_t e = (size_t)blockIdx.y * plane4 + i;
    const float sc = s[blockIdx.y];
    const float4 y = y2[e], v = t[e];
    float4 o;
    o.x = fmaf(res_scale, y.x * sc, v.x);
    o.y = fmaf(res_scale, y.y * sc, v.y);
    o.z = fmaf(res_scale, y.z * sc, v.z);
    o.w = fmaf(res_scale, y.w * sc, v.w);
    out[e] = o;
}

// The reduction and the attention of one block on x (F planes): part gets F x chunks doubles, s (and mean, if not null) F floats.
// reduce_name / att_name: the profiler scopes of the two launches.
inline void rc_attention(hipStream_t st, sr_ctx *ctx, const float *x, long long plane, long long pitch, int h, int w, int F, int R,
                         const float *w1, const float *b1, const float *w2, const float *b2, double *part, float *s, float *mean,
                         const char *reduce_name = "rcan_reduce", const char *att_name = "rcan_attention")
{
    const int chunks = (h + RC_ROWS - 1) / RC_ROWS;
    {
        ProfScope ps(ctx, reduce_name);
        hipLaunchKernelGGL(k_rc_rowsum, dim3(chunks, F), dim3(256), 0, st, x, plane, pitch, h, w, part);
    }
    ProfScope ps(ctx, att_name);
    hipLaunchKernelGGL(k_rc_attention, dim3(1), dim3(256), 0, st, part, chunks, (double)h * (double)w, F, R, w1, b1, w2, b2, s, mean);
}

}  // namespace
