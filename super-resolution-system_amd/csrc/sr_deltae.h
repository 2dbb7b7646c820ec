// sr_deltae.h -- what the host unit (sr_deltae_host.cpp: the plan, the linearisation table, the host restatement, the
// histogram values, every refusal) and the kernels (sr_deltae.hip) of the colour difference share.  The definition is in
// include/sr_hip.h.  The per-pixel arithmetic is written ONCE, here, for the host and the device alike: the same expressions
// in the same order (the build has fp contraction off), so the two differ only by the math library behind cbrt / atan2 /
// sin / cos / exp.  Internal: nothing here is part of the C ABI.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "sr_internal.h"

#if defined(__HIP__)        // spelled as attributes: the host unit is compiled without the HIP runtime header
#define DE_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define DE_HD inline
#endif

constexpr int DE_THREADS = 256;             // threads of every block
constexpr int DE_LANES = 64;                // threads side by side in a tile row
constexpr int DE_RUN = 4;                   // pixels per thread and tile, DE_LANES apart
constexpr int DE_TW = DE_LANES * DE_RUN;    // 256 columns ...
constexpr int DE_TH = DE_THREADS / DE_LANES;    // ... by 4 rows: one tile
constexpr int DE_MAX_BLOCKS = 2048;         // blocks of the sums launch at most: block b takes tiles b, b + blocks, ...
constexpr int DE_CELL_ROWS = 64;            // longest row chunk of the per-cell column march
constexpr int DE_TABLE = 256;

struct DePlan {
    int ch, cw;                             // the cropped size
    uint64_t count;
    int tiles_x;
    long long tiles;
    int blocks;                             // min(tiles, DE_MAX_BLOCKS): depends on the size alone
    // context scratch: the table, the histogram, the three results, then the per-block partials (sum, sum2, max)
    size_t off_table, off_hist, off_result, off_part, total;
};

// Every refusal of a call that depends on shape, channels, crop and formula, then the launch and the scratch layout.
int delta_e_plan(const char *scope, int h, int w, int cn, int crop_border, int formula, DePlan *p);
// The 256 linear values of the sRGB bytes, in double.
void delta_e_table(double *table);

// f of the Lab transform
DE_HD double de_f(double t) { return t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0; }

// scikit-image's rgb2lab of one pixel whose three bytes are already linearised
DE_HD void de_lab(double lr, double lg, double lb, double &L, double &A, double &B)
{
    const double x = (0.412453 * lr + 0.357580 * lg) + 0.180423 * lb;
    const double y = (0.212671 * lr + 0.715160 * lg) + 0.072169 * lb;
    const double z = (0.019334 * lr + 0.119193 * lg) + 0.950227 * lb;
    const double fx = de_f(x / 0.95047), fy = de_f(y), fz = de_f(z / 1.08883);
    L = 116.0 * fy - 16.0;
    A = 500.0 * (fx - fy);
    B = 200.0 * (fy - fz);
}

DE_HD double de_76(double L1, double a1, double b1, double L2, double a2, double b2)
{
    const double dL = L2 - L1, da = a2 - a1, db = b2 - b1;
    return sqrt((dL * dL + da * da) + db * db);
}

DE_HD double de_pow7(double c)
{
    const double c2 = c * c, c4 = c2 * c2;
    return (c4 * c2) * c;
}

// scikit-image 0.18.3's deltaE_ciede2000 with kL = kC = kH = 1, term for term
DE_HD double de_2000(double L1, double a1, double b1, double L2, double a2, double b2)
{
    constexpr double PI = 3.141592653589793, TWO_PI = 2.0 * PI, RAD = PI / 180.0, DEG = 180.0 / PI;
    constexpr double P25_7 = 6103515625.0;
    const double cbar = 0.5 * (sqrt(a1 * a1 + b1 * b1) + sqrt(a2 * a2 + b2 * b2));
    const double c7 = de_pow7(cbar);
    const double scale = 1.0 + 0.5 * (1.0 - sqrt(c7 / (c7 + P25_7)));
    const double a1p = a1 * scale, a2p = a2 * scale;
    const double C1 = sqrt(a1p * a1p + b1 * b1), C2 = sqrt(a2p * a2p + b2 * b2);
    double h1 = atan2(b1, a1p), h2 = atan2(b2, a2p);
    if (h1 < 0.0) h1 += TWO_PI;
    if (h2 < 0.0) h2 += TWO_PI;
    // lightness
    const double lbar = 0.5 * (L1 + L2);
    const double tmp = (lbar - 50.0) * (lbar - 50.0);
    const double SL = 1.0 + 0.015 * tmp / sqrt(20.0 + tmp);
    const double L_term = (L2 - L1) / SL;
    // chroma
    const double cbp = 0.5 * (C1 + C2);
    const double SC = 1.0 + 0.045 * cbp;
    const double C_term = (C2 - C1) / SC;
    // hue
    const double h_diff = h2 - h1, h_sum = h1 + h2, CC = C1 * C2;
    double dH = h_diff;
    if (h_diff > PI) dH -= TWO_PI;
    if (h_diff < -PI) dH += TWO_PI;
    if (CC == 0.0) dH = 0.0;
    const double dH_term = 2.0 * sqrt(CC) * sin(dH / 2.0);
    double hbar = h_sum;
    if (CC != 0.0 && fabs(h_diff) > PI) hbar += h_sum < TWO_PI ? TWO_PI : -TWO_PI;
    if (CC == 0.0) hbar *= 2.0;
    hbar *= 0.5;
    const double T = (((1.0 - 0.17 * cos(hbar - 30.0 * RAD)) + 0.24 * cos(2.0 * hbar)) + 0.32 * cos(3.0 * hbar + 6.0 * RAD)) -
                     0.20 * cos(4.0 * hbar - 63.0 * RAD);
    const double SH = 1.0 + 0.015 * cbp * T;
    const double H_term = dH_term / SH;
    // rotation
    const double d7 = de_pow7(cbp);
    const double Rc = 2.0 * sqrt(d7 / (d7 + P25_7));
    const double u = (hbar * DEG - 275.0) / 25.0;
    const double dtheta = (30.0 * RAD) * exp(-(u * u));
    const double R_term = -sin(2.0 * dtheta) * Rc * C_term * H_term;
    const double e2 = ((L_term * L_term + C_term * C_term) + H_term * H_term) + R_term;
    return sqrt(e2 > 0.0 ? e2 : 0.0);
}

// the histogram bin of a value
DE_HD int de_bin(double v)
{
    const double s = 16.0 * v;
    return s < (double)(SR_DELTA_E_BINS - 1) ? (int)s : SR_DELTA_E_BINS - 1;      // the open last bin takes everything else
}
