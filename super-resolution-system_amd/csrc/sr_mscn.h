// sr_mscn.h -- the MSCN core that NIQE (sr_niqe.hip, sr_niqe_host.cpp) and BRISQUE (sr_brisque.hip, sr_brisque_host.cpp) share.
// Host side (every includer): the two plans and the crop refusals in front of them, the window, the Gamma-ratio table with its
// argmin, and the AGGD fit up to (alpha, ls, rs).  Device side (the .hip units): the luma, the exact half-plane kernel, the
// horizontal and the vertical pass of the 7 x 7 window, the register-window march that runs them down an LDS tile, the 25
// quantities of one position and the block sum.  There is one copy of each operation, so "equal bits" between the metrics, and
// between BRISQUE's march and its halo, is a property of the code and not of its upkeep.  What differs stays with its unit:
// NIQE's replicate halo, block-local roll and typed records; BRISQUE's zero padding, halo of m and whole-plane roll.
// Internal: nothing here is part of the C ABI.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "sr_internal.h"

constexpr int NQ_BLOCK = 96;        // block side at scale 1 (48 at scale 2)
constexpr int NQ_R = 3;             // MSCN window radius: 7 taps
constexpr int NQ_FEAT = 36;
constexpr int NQ_GAM_N = 9801;      // gam = 0.2 + 0.001 t, t = 0 .. 9800

struct NqPlan {
    int H, W;                       // the kept plane: multiples of 96
    int nby, nbx;
    size_t off_half, off_rec;       // context scratch: the int32 half plane, then 2 nby nbx records
    size_t total;
};

// Every shape refusal of sr_niqe_plan; scope names the caller in the message.
int nq_plan(const char *scope, int h, int w, int cn, int crop_border, NqPlan *p);
// k_i = g_i / sum g, g_i = exp(-i^2 / (2 s^2)), s = 7 / 6, i = -3 .. 3.
void nq_window(double k[2 * NQ_R + 1]);

constexpr int BQ_TILE = 64;         // side of the tile of m one workgroup of k_brisque_moments owns
constexpr int BQ_MIN = 16;          // the least side after the crop
constexpr int BQ_Q = 25;            // quantities of a scale: five moments of five X

struct BqPlan {
    int H, W, H2, W2;               // the cropped plane and its half plane (sides rounded up)
    long long nt[2];                // tiles per scale
    size_t off_half, off_part[2], off_buf0, off_buf1;   // context scratch: the half plane, the partials, the reduction's buffers
    size_t total;
};

// Every shape refusal of sr_brisque_plan; scope names the caller in the message.
int bq_plan(const char *scope, int h, int w, int cn, int crop_border, BqPlan *p);

// What both plans refuse, and the sides ch x cw that the crop leaves (each at least min_side).
inline int mscn_crop(const char *scope, int h, int w, int cn, int crop_border, int min_side, long long *ch, long long *cw)
{
    if (cn != 1 && cn != 3) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need 1 or 3 channels (got %d)", scope, cn);
    if (crop_border < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: crop_border must be >= 0 (got %d)", scope, crop_border);
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need h, w >= 1", scope);
    *ch = (long long)h - 2LL * crop_border;
    *cw = (long long)w - 2LL * crop_border;
    if (*ch < min_side || *cw < min_side)
        return sr_set_error(SR_ERR_SHAPE, "%s: image %dx%d with crop_border %d leaves %lldx%lld: both sides must be at least %d "
                            "after the crop", scope, w, h, crop_border, std::max(*cw, 0LL), std::max(*ch, 0LL), min_side);
    return SR_OK;
}

inline double nq_gam_at(int t) { return 0.2 + 0.001 * (double)t; }

// Gamma(2 / gam)^2 / (Gamma(1 / gam) Gamma(3 / gam)) over the grid (r: the AGGD fits) and its reciprocal form
// Gamma(1 / gam) Gamma(3 / gam) / Gamma(2 / gam)^2 (rinv: BRISQUE's GGD fit), built once
struct NqGamTable {
    std::vector<double> r, rinv;
    bool ascending = true;
    NqGamTable() : r(NQ_GAM_N), rinv(NQ_GAM_N)
    {
        for (int t = 0; t < NQ_GAM_N; ++t) {
            const double g = nq_gam_at(t), g2 = std::tgamma(2.0 / g);
            r[t] = g2 * g2 / (std::tgamma(1.0 / g) * std::tgamma(3.0 / g));
            rinv[t] = std::tgamma(1.0 / g) * std::tgamma(3.0 / g) / (g2 * g2);
            if (t && !(r[t] > r[t - 1])) ascending = false;
        }
    }
};

inline const NqGamTable &nq_gam_table()
{
    static const NqGamTable T;
    return T;
}

// argmin_t (r[t] - R)^2, the first on a tie.  The table ascends strictly, so the minimum lies beside R's insertion point: the
// same squared differences are compared there as a scan of the whole table would compare (which is what runs if it did not).
inline int nq_gam_argmin(double R)
{
    const NqGamTable &T = nq_gam_table();
    int lo = 0, hi = NQ_GAM_N - 1;
    if (T.ascending) {
        const int p = (int)(std::lower_bound(T.r.begin(), T.r.end(), R) - T.r.begin());
        lo = std::max(p - 2, 0);
        hi = std::min(p + 2, NQ_GAM_N - 1);
    }
    int best = lo;
    double bd = (T.r[lo] - R) * (T.r[lo] - R);
    for (int t = lo + 1; t <= hi; ++t) {
        const double d = (T.r[t] - R) * (T.r[t] - R);
        if (d < bd) {
            bd = d;
            best = t;
        }
    }
    return best;
}

// The AGGD fit of one X over n elements as far as the metrics agree: the shape and the two root mean squares.  All NaN when a
// side of 0 is empty or R is NaN.  Each metric forms its own features from these (they are rounding contracts of their own).
struct MscnAggd {
    double alpha, ls, rs;
};

inline MscnAggd mscn_aggd(const sr_niqe_moments &m, double n)
{
    const double nan = std::nan("");
    if (m.n_neg == 0 || m.n_pos == 0) return {nan, nan, nan};
    const double ls = std::sqrt(m.ssq_neg / (double)m.n_neg), rs = std::sqrt(m.ssq_pos / (double)m.n_pos);
    const double g = ls / rs;
    const double ma = m.sabs / n;
    const double rhat = ma * ma / ((m.ssq_neg + m.ssq_pos) / n);
    const double g2 = g * g;
    const double R = rhat * (g2 * g + 1.0) * (g + 1.0) / ((g2 + 1.0) * (g2 + 1.0));
    if (!(R == R)) return {nan, nan, nan};
    return {nq_gam_at(nq_gam_argmin(R)), ls, rs};
}

#ifdef HIP_INCLUDE_HIP_HIP_RUNTIME_H   // the .hip units (they include sr_ctx.h first); the host units have no device code
namespace {                            // each unit gets its own copies of the kernel and of the entry point's tail

// the plane's value at a pixel: MATLAB's uint8 rgb2ycbcr luma (SR_BENCH_Y_ROUND: half up, 16 .. 235) for PX = 3, the byte for 1
template <int PX>
__device__ __forceinline__ unsigned nq_luma(const unsigned char *p)
{
    if constexpr (PX == 3)
        return (2u * (65481u * p[0] + 128553u * p[1] + 24966u * p[2] + 4080000u) + 255000u) / 510000u;
    else
        return p[0];
}

struct MscnWindow {
    double k[2 * NQ_R + 1];
};

constexpr int MH_H = 24, MH_W = 48;         // outputs of one k_mscn_half block: both divide 48
constexpr int MH_T = 256;

// The exact half-resolution plane.  A block owns MH_H x MH_W outputs.  It reads its (2 MH_H + 6) x (2 MH_W + 6) inputs once
// (luma on the fly for PX = 3, indices reflected at the plane's edge) into LDS, runs the 8-tap pass along the rows into a second
// LDS tile and along the columns out of it, and writes int32 = 65536 x the result at pitch W2.  Integer arithmetic only: taps
// {-3, -9, 29, 111, 111, 29, -9, -3}, |row pass| <= 255 * 304, |result| <= 255 * 304^2 < 2^25.
// GUARD = false (NIQE): both sides are multiples of 96, every block is whole.  GUARD = true (BRISQUE): a plane of any size, the
// grid covers ceil(H / 2) x ceil(W / 2) outputs with partial blocks and every store is bounds-guarded; inputs of outputs that do
// not exist are clamped into the plane after the reflection (they are read, never used).
template <int PX, bool GUARD>
__global__ __launch_bounds__(MH_T) void k_mscn_half(const unsigned char *__restrict__ img, long long stride, int H, int W, int H2,
                                                    int W2, int *__restrict__ out)
{
    constexpr int IH = 2 * MH_H + 6, IW = 2 * MH_W + 6;
    __shared__ unsigned short I[IH][IW];
    __shared__ int R[IH][MH_W];
    const int t = threadIdx.x;
    const int oy0 = (int)blockIdx.y * MH_H, ox0 = (int)blockIdx.x * MH_W;
    for (int e = t; e < IH * IW; e += MH_T) {
        const int r = e / IW, c = e - r * IW;
        int y = 2 * oy0 - 3 + r, x = 2 * ox0 - 3 + c;
        y = y < 0 ? -y - 1 : (y >= H ? 2 * H - 1 - y : y);
        x = x < 0 ? -x - 1 : (x >= W ? 2 * W - 1 - x : x);
        if constexpr (GUARD) {
            y = min(max(y, 0), H - 1);      // only inputs of outputs beyond H2 x W2 need it
            x = min(max(x, 0), W - 1);
        }
        I[r][c] = (unsigned short)nq_luma<PX>(img + (size_t)y * (size_t)stride + (size_t)x * PX);
    }
    __syncthreads();
    for (int e = t; e < IH * MH_W; e += MH_T) {
        const int r = e / MH_W, c = e - r * MH_W;
        const unsigned short *p = &I[r][2 * c];
        R[r][c] = 111 * ((int)p[3] + (int)p[4]) + 29 * ((int)p[2] + (int)p[5]) - 9 * ((int)p[1] + (int)p[6]) - 3 * ((int)p[0] + (int)p[7]);
    }
    __syncthreads();
    for (int e = t; e < MH_H * MH_W; e += MH_T) {
        const int r = e / MH_W, c = e - r * MH_W;
        if constexpr (GUARD)
            if (oy0 + r >= H2 || ox0 + c >= W2) continue;
        const int v = 111 * (R[2 * r + 3][c] + R[2 * r + 4][c]) + 29 * (R[2 * r + 2][c] + R[2 * r + 5][c]) -
                      9 * (R[2 * r + 1][c] + R[2 * r + 6][c]) - 3 * (R[2 * r][c] + R[2 * r + 7][c]);
        out[(size_t)(oy0 + r) * (size_t)W2 + (size_t)(ox0 + c)] = v;
    }
}

// gray levels per integer of a scale's plane: the image's bytes, the half plane's 65536ths
template <int SCALE>
constexpr double MSCN_UNIT = SCALE == 1 ? 1.0 : 1.0 / 65536.0;

// The horizontal pass of one row, I and I^2: taps added in ascending order.  px(i) is the integer at pixel i of the row's window.
template <int SCALE, typename Px>
__device__ __forceinline__ void mscn_hpass(const double *k, Px px, double &hm, double &hq)
{
    double v = (double)px(0) * MSCN_UNIT<SCALE>;                        // exact, and so is v * v (|integer| < 2^25)
    hm = k[0] * v;
    hq = k[0] * (v * v);
#pragma unroll
    for (int i = 1; i < 7; ++i) {
        v = (double)px(i) * MSCN_UNIT<SCALE>;
        hm += k[i] * v;
        hq += k[i] * (v * v);
    }
}

// The vertical pass over seven rows of the horizontal one: mu, sigma, and m of the position whose own integer is `centre`.
template <int SCALE, typename T>
__device__ __forceinline__ double mscn_vpass(const double *k, const double *wm, const double *wq, T centre, double &sigma)
{
    double mu = k[0] * wm[0], q = k[0] * wq[0];
#pragma unroll
    for (int j = 1; j < 7; ++j) {
        mu += k[j] * wm[j];
        q += k[j] * wq[j];
    }
    sigma = sqrt(fabs(q - mu * mu));
    const double v = (double)centre * MSCN_UNIT<SCALE>;
    return (v - mu) / (sigma + 1.0);
}

// One thread's march down RS rows of column c of an LDS tile of integers with its 3-pixel halo (I: its rows; position (r, c)
// is I[r + 3][c + 3]), from row r0 on: the horizontal pass of one tile row enters a 7-row register window, the vertical pass
// over the window gives emit(r, m, sigma).  The 6 window rows above r0 are recomputed, so no horizontal-pass row is stored.
template <int SCALE, int RS, typename Row, typename Emit>
__device__ __forceinline__ void mscn_march(const Row *I, int c, int r0, const double *k, Emit emit)
{
    double wm[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, wq[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int it = 0; it < RS + 2 * NQ_R; ++it) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            wm[j] = wm[j + 1];
            wq[j] = wq[j + 1];
        }
        const auto *p = &I[r0 + it][c];
        mscn_hpass<SCALE>(k, [p](int i) { return p[i]; }, wm[6], wq[6]);
        if (it < 2 * NQ_R) continue;
        const int r = r0 + it - 2 * NQ_R;
        double sigma;
        const double m = mscn_vpass<SCALE>(k, wm, wq, I[r + NQ_R][c + NQ_R], sigma);
        emit(r, m, sigma);
    }
}

// The 25 quantities of one position: five moments of X = a and of a times its four rolled neighbours.
__device__ __forceinline__ void mscn_accumulate(double *acc, double a, double left, double up, double up_left, double up_right)
{
    const double X[5] = {a, a * left, a * up, a * up_left, a * up_right};
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const double x = X[s], xx = x * x;
        acc[5 * s + 0] += x < 0.0 ? 1.0 : 0.0;                          // counts stay exact integers in fp64
        acc[5 * s + 1] += x > 0.0 ? 1.0 : 0.0;
        acc[5 * s + 2] += x < 0.0 ? xx : 0.0;
        acc[5 * s + 3] += x > 0.0 ? xx : 0.0;
        acc[5 * s + 4] += fabs(x);
    }
}

// Q quantities per thread summed over the workgroup in a fixed order: down each wave by shuffles, lane 0 to red, one barrier,
// then the waves in ascending order.  Thread t < Q returns quantity t's sum; the others return 0.
template <int NWAVE, int Q>
__device__ __forceinline__ double mscn_block_sum(const double *acc, double (*red)[Q], int t)
{
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        double v = acc[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    double v = 0.0;
    if (t < Q) {
        v = red[0][t];
        for (int w = 1; w < NWAVE; ++w) v += red[w][t];
    }
    return v;
}

// The tail of sr_niqe_half_plane / sr_brisque_half_plane (scope: "sr_niqe" / "sr_brisque"), entered with the context current:
// the H2 x W2 int32 plane at the head of the metric's scratch to the host.  H2 < 1: no call has left a plane there.
inline int mscn_half_plane(sr_ctx *ctx, const char *scope, const void *buffer, int H2, int W2, int32_t *h_out)
{
    if (H2 < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s_half_plane: no %s_u8 call has completed on this context", scope, scope);
    HIPCHK(hipMemcpyAsync(h_out, buffer, (size_t)H2 * (size_t)W2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // namespace
#endif
