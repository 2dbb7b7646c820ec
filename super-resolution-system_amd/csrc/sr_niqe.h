// sr_niqe.h -- what the NIQE kernels (sr_niqe.hip) take from the host unit (sr_niqe_host.cpp): the plan and the MSCN window;
// and what BRISQUE (sr_brisque.hip, sr_brisque_host.cpp) shares with NIQE: the luma, the window, the Gamma-ratio table and
// its argmin, and its own plan.  Internal: nothing here is part of the C ABI.
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

#ifdef HIP_INCLUDE_HIP_HIP_RUNTIME_H   // the .hip units (they include sr_ctx.h first); the host units have no device code
// the plane's value at a pixel: MATLAB's uint8 rgb2ycbcr luma (SR_BENCH_Y_ROUND: half up, 16 .. 235) for PX = 3, the byte for 1
template <int PX>
__device__ __forceinline__ unsigned nq_luma(const unsigned char *p)
{
    if constexpr (PX == 3)
        return (2u * (65481u * p[0] + 128553u * p[1] + 24966u * p[2] + 4080000u) + 255000u) / 510000u;
    else
        return p[0];
}
#endif
