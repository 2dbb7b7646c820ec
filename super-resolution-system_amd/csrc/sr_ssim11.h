// sr_ssim11.h -- the Gaussian-11 (sigma 1.5) SSIM column march shared by sr_qmap.hip (per-cell maps), sr_msssim.hip (MS-SSIM)
// and sr_srbench.hip (SR-benchmark PSNR / SSIM), and the SSIM quotient, taps and gray pair load they share with sr_assess.hip.
//
// The march: a block of S11_TX threads owns one chunk of rows; each thread owns a column and walks down the chunk.
//   Window11<T>       rows lr - 10 .. lr of the thread's column in registers, exact values.  Three forms are in use:
//                       packed u8      x | y << 14 in one dword (pair sums <= 510 stay in their fields), x y and x^2 + y^2 as
//                                      unsigned                                                           33 registers
//                       16-bit sums    x, y, x y as unsigned, x^2 + y^2 as fp64; the pair sum of two x y can pass 2^32 and is
//                                      widened first (MS-SSIM levels >= 1)                                55 registers
//                       26-bit luma    x, y as unsigned, x y and x^2 + y^2 as fp64 (SR_BENCH_Y)           66 registers
//   s11_col_pass[_packed]  the vertical pass over the windows: the centre tap plus five pair sums, six fp64 products per map.
//   s11_store_col     the four vertical results of a row go into F[4][S11_TX]; the caller keeps two such rows, selected by
//                     row parity, so one barrier per row is enough.
//   s11_row_pass      the horizontal pass over those rows, 44 consecutive doubles per map sample.
//   ssim_terms        the terms of the SSIM quotient: l cs, and cs beside it from the same reciprocal.
//   s11_block_sum2    the block's S11_TX column sums of two components through a fixed tree: no floating-point atomics.
// Every expression is evaluated in the order written (the build has -ffp-contract=off): equal inputs give equal bits.
// Host side: the normalised taps, the chunk cut, the scratch layout of the per-block partials.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "sr_ctx.h"

constexpr int S11_TX = 256;                  // threads = columns a block filters vertically
constexpr int S11_R = 5;                     // radius of the Gaussian
constexpr int S11_SIDE = 2 * S11_R + 1;
constexpr int S11_OUT = S11_TX - 2 * S11_R;  // columns a block produces (even: a pooled pair never straddles two blocks)
constexpr int S11_ROWS = 128;                // longest chunk of map rows (10 halo rows on top: 8 %)
constexpr int S11_ROWS_MIN = 16;             // shortest chunk a small map is cut into ...
constexpr int S11_BLOCKS = 1024;             // ... to reach this many blocks

// ---- device ------------------------------------------------------------------------------------------------------------------

// 1 / d for the SSIM quotient: hardware estimate + one Newton step (relative error ~1e-15; the metric's bar is 1e-9
// against the oracle, 1e-4 against the reference), d a product of positive SSIM terms
__device__ __forceinline__ double ssim_recip(double d)
{
    const double r = __builtin_amdgcn_rcp(d);
    return fma(fma(-d, r, 1.0), r, r);
}

// The four terms of one window's SSIM, l cs = (a1 a2) / (b1 b2) and cs = a2 / b2 = (a2 b1) / (b1 b2): spq = uxx + uyy,
// dpq = uxy.  One reciprocal of b1 b2 serves both.
struct SsimTerms {
    double a1, a2, b1, b2;
};

__device__ __forceinline__ SsimTerms ssim_terms(double ux, double uy, double spq, double dpq, double c1, double c2)
{
    const double uxuy = ux * uy, uu = fma(ux, ux, uy * uy);
    const double a1 = fma(2.0, uxuy, c1), a2 = fma(2.0, dpq - uxuy, c2);
    const double b1 = uu + c1, b2 = (spq - uu) + c2;
    return {a1, a2, b1, b2};
}

__device__ __forceinline__ double ssim_quot(double ux, double uy, double spq, double dpq, double c1, double c2)
{
    const SsimTerms s = ssim_terms(ux, uy, spq, dpq, c1, c2);
    return (s.a1 * s.a2) * ssim_recip(s.b1 * s.b2);
}

// Two u8 pixels as integer gray (cv2.cvtColor's fixed point, shift = its fractional bits) and their squared difference
// over the channels.
template <int CN>
__device__ __forceinline__ void gray_pair(const unsigned char *__restrict__ pa, const unsigned char *__restrict__ pb, int shift,
                                          int &ga, int &gb, unsigned &sq)
{
    if (CN == 1) {
        ga = pa[0];
        gb = pb[0];
        const int d = ga - gb;
        sq = (unsigned)(d * d);
    } else {
        const int r0 = pa[0], g0 = pa[1], b0 = pa[2], r1 = pb[0], g1 = pb[1], b1 = pb[2];
        if (shift == 15) {
            ga = (r0 * 9798 + g0 * 19235 + b0 * 3735 + (1 << 14)) >> 15;
            gb = (r1 * 9798 + g1 * 19235 + b1 * 3735 + (1 << 14)) >> 15;
        } else {
            ga = (r0 * 4899 + g0 * 9617 + b0 * 1868 + (1 << 13)) >> 14;
            gb = (r1 * 4899 + g1 * 9617 + b1 * 1868 + (1 << 13)) >> 14;
        }
        const int dr = r0 - r1, dg = g0 - g1, db = b0 - b1;
        sq = (unsigned)(dr * dr + dg * dg + db * db);
    }
}

// The last 11 rows of one column, oldest first.  Every index is a constant once the loops are unrolled: the rows are
// registers.  T is unsigned or double.
template <typename T>
struct Window11 {
    T v[S11_SIDE] = {};

    __device__ __forceinline__ void push(T x)
    {
#pragma unroll
        for (int i = 0; i < S11_SIDE - 1; ++i) v[i] = v[i + 1];
        v[S11_SIDE - 1] = x;
    }
    __device__ __forceinline__ T operator[](int i) const { return v[i]; }
};

// Vertical pass of the packed u8 form -> h = E[x], E[y], E[x^2 + y^2], E[x y] of the column (in that order everywhere).
// Pair sums are integer adds, one for both images.
__device__ __forceinline__ void s11_col_pass_packed(const Window11<unsigned> &wxy, const Window11<unsigned> &wp,
                                                    const Window11<unsigned> &wq, const double (&kk)[6], double (&h)[4])
{
    h[0] = (double)(wxy[S11_R] & 0x3FFFu) * kk[0];
    h[1] = (double)(wxy[S11_R] >> 14) * kk[0];
    h[2] = (double)wp[S11_R] * kk[0];
    h[3] = (double)wq[S11_R] * kk[0];
#pragma unroll
    for (int j = 1; j <= S11_R; ++j) {
        const unsigned sxy = wxy[S11_R - j] + wxy[S11_R + j];
        h[0] = fma((double)(sxy & 0x3FFFu), kk[j], h[0]);
        h[1] = fma((double)(sxy >> 14), kk[j], h[1]);
        h[2] = fma((double)(wp[S11_R - j] + wp[S11_R + j]), kk[j], h[2]);
        h[3] = fma((double)(wq[S11_R - j] + wq[S11_R + j]), kk[j], h[3]);
    }
}

// The same for x and y in windows of their own (pair sums < 2^32) and x^2 + y^2, x y as unsigned or fp64.  WIDEN_Q: the
// rows of wq are converted before the add, for integers whose pair sum can pass 2^32.
template <bool WIDEN_Q, typename TP, typename TQ>
__device__ __forceinline__ void s11_col_pass(const Window11<unsigned> &wx, const Window11<unsigned> &wy, const Window11<TP> &wp,
                                             const Window11<TQ> &wq, const double (&kk)[6], double (&h)[4])
{
    h[0] = (double)wx[S11_R] * kk[0];
    h[1] = (double)wy[S11_R] * kk[0];
    h[2] = (double)wp[S11_R] * kk[0];
    h[3] = (double)wq[S11_R] * kk[0];
#pragma unroll
    for (int j = 1; j <= S11_R; ++j) {
        h[0] = fma((double)(wx[S11_R - j] + wx[S11_R + j]), kk[j], h[0]);
        h[1] = fma((double)(wy[S11_R - j] + wy[S11_R + j]), kk[j], h[1]);
        h[2] = fma((double)(wp[S11_R - j] + wp[S11_R + j]), kk[j], h[2]);
        if constexpr (WIDEN_Q) h[3] = fma((double)wq[S11_R - j] + (double)wq[S11_R + j], kk[j], h[3]);
        else h[3] = fma((double)(wq[S11_R - j] + wq[S11_R + j]), kk[j], h[3]);
    }
}

// the vertical results of thread t's column go into its row of LDS
__device__ __forceinline__ void s11_store_col(double (*F)[S11_TX], int t, const double (&h)[4])
{
    F[0][t] = h[0]; F[1][t] = h[1]; F[2][t] = h[2]; F[3][t] = h[3];
}

// horizontal pass centred on column c of the row (c - 5 .. c + 5 must lie inside it)
__device__ __forceinline__ void s11_row_pass(const double (*F)[S11_TX], int c, const double (&kk)[6], double (&u)[4])
{
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        double acc = F[m][c] * kk[0];
#pragma unroll
        for (int j = 1; j <= S11_R; ++j) acc = fma(F[m][c - j] + F[m][c + j], kk[j], acc);
        u[m] = acc;
    }
}

// The block's S11_TX pairs (v0, v1) through a fixed tree; thread 0 stores the two sums to out[0], out[1].  sd0, sd1: S11_TX
// doubles of LDS each, which may be the rows the march used (the barrier in front makes them free).
__device__ __forceinline__ void s11_block_sum2(double *sd0, double *sd1, int t, double v0, double v1, double *__restrict__ out)
{
    __syncthreads();
    sd0[t] = v0;
    sd1[t] = v1;
    __syncthreads();
    for (int s = S11_TX / 2; s > 0; s >>= 1) {
        if (t < s) {
            sd0[t] += sd0[t + s];
            sd1[t] += sd1[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[0] = sd0[0];
        out[1] = sd1[0];
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------

// k6[0] the centre tap, k6[j] the +-j taps of the normalised kernel
inline void gauss_taps(double *k6)
{
    double k[11], sum = 0.0;
    for (int i = 0; i < 11; ++i) {
        const double x = i - 5;
        k[i] = std::exp(-0.5 / (1.5 * 1.5) * x * x);     // scipy.ndimage._gaussian_kernel1d(sigma=1.5, radius=5)
        sum += k[i];
    }
    for (int j = 0; j <= 5; ++j) k6[j] = k[5 + j] / sum;
}

// Chunks of at most S11_ROWS map rows; a small map takes shorter ones (down to S11_ROWS_MIN) until it has S11_BLOCKS blocks:
// a block walks its rows one after the other, so a small map cut into a few long chunks would take as long as a chunk takes
// on an empty chip.  The cut depends on the size alone, never on the device: equal bits everywhere.
// mh: map rows; per_chunk: blocks that share a chunk (column blocks x planes); even_step: chunks must start on even rows.
struct ChunkCut {
    int step, count;            // map rows per chunk, chunks
};

inline ChunkCut s11_chunk_cut(int mh, long long per_chunk, bool even_step)
{
    int rows = S11_ROWS;
    while (rows > S11_ROWS_MIN && (long long)((mh + rows - 1) / rows) * per_chunk < S11_BLOCKS) rows /= 2;
    const int n = (mh + rows - 1) / rows;
    int step = (mh + n - 1) / n;
    if (even_step) step = (step + 1) & ~1;
    return {step, (mh + step - 1) / step};
}

// Scratch of a two-component reduction over nblk blocks, from byte offset `off` on: the per-block partials and the two
// ping-pong buffers of reduce_partials.
struct PartialsLayout {
    size_t off_part, off_buf0, off_buf1, end;
};

inline PartialsLayout s11_partials_layout(size_t off, size_t nblk)
{
    const size_t part = up256(nblk * 2 * sizeof(double)), buf = up256((nblk / 1024 + 2) * 2 * sizeof(double));
    return {off, off + part, off + part + buf, off + part + 2 * buf};
}
