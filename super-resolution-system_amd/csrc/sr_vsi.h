// sr_vsi.h -- what the host unit (sr_vsi_host.cpp: the plan, F, the triangle resize tables of the four axes and the composite
// pooling tables, the log-Gabor and centre-prior planes, the value, every refusal, the host restatement) and the kernels
// (sr_vsi.hip) of VSI share.  The definition is in include/sr_hip.h.  Internal: nothing here is part of the C ABI.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "sr_fsim.h"
#include "sr_imresize.h"
#include "sr_internal.h"

constexpr int VSI_N = 256;                  // side of the SDSP grid
constexpr int VSI_NN = VSI_N * VSI_N;
constexpr int VSI_MIN_SIDE = 16;
constexpr int VSI_THREADS = 256;            // every kernel's block; the pooling's row segment (as FSIM's)
constexpr int VSI_MAX_F = VSI_THREADS;      // one window fits a segment
constexpr int VSI_DFT_TILE = 16;
constexpr int VSI_EXPAND_ROWS = 64;         // full-resolution rows of one block of the min / max pass
constexpr double VSI_OMEGA0 = 0.021, VSI_SIGMA_F = 1.34, VSI_SIGMA_D = 145.0, VSI_SIGMA_C = 0.001;
constexpr double VSI_C1 = 1.27, VSI_C2 = 386.0, VSI_C3 = 130.0, VSI_ALPHA = 0.40, VSI_BETA = 0.02;

#if defined(__HIP__)
#define VSI_HD __host__ __device__
#else
#define VSI_HD
#endif

// Re(s_c^0.02): |z|^0.02, times cos(0.02 pi) for a negative z (the principal complex power)
VSI_HD inline double vsi_chroma_weight(double z)
{
    const double p = pow(fabs(z), VSI_BETA);
    return z < 0.0 ? p * cos(VSI_BETA * 3.14159265358979323846) : p;
}

VSI_HD inline double vsi_sim(double u, double v, double k) { return (2.0 * u * v + k) / (u * u + v * v + k); }

// the script's own RGB2Lab of one sample (r, g, b in 0 .. 255, not integers after the resize)
VSI_HD inline void vsi_rgb2lab(double r, double g, double b, double *L, double *A, double *B)
{
    double c[3] = {r / 255.0, g / 255.0, b / 255.0};
    for (int k = 0; k < 3; ++k) c[k] = c[k] <= 0.04045 ? c[k] / 12.92 : pow((c[k] + 0.055) / 1.055, 2.4);
    double x = 0.4124564 * c[0] + 0.3575761 * c[1] + 0.1804375 * c[2];
    const double y = 0.2126729 * c[0] + 0.7151522 * c[1] + 0.0721750 * c[2];
    double z = 0.0193339 * c[0] + 0.1191920 * c[1] + 0.9503041 * c[2];
    x = x / 0.950456;
    z = z / 1.088754;
    const double fx = x > 0.008856 ? cbrt(x) : 7.787 * x + 16.0 / 116.0;
    const double fy = y > 0.008856 ? cbrt(y) : 7.787 * y + 16.0 / 116.0;
    const double fz = z > 0.008856 ? cbrt(z) : 7.787 * z + 16.0 / 116.0;
    *L = 116.0 * fy - 16.0;
    *A = 500.0 * (fx - fy);
    *B = 200.0 * (fy - fz);
}

// SF SD SC of one grid sample: sf2 = the sum of the three squared filter responses, range = min a, max a, min b, max b
VSI_HD inline double vsi_saliency(double sf2, double sd, double a, double b, const double *range)
{
    const double an = (a - range[0]) / (range[1] - range[0]), bn = (b - range[2]) / (range[3] - range[2]);
    const double sc = 1.0 - exp(-(an * an + bn * bn) / (VSI_SIGMA_C * VSI_SIGMA_C));
    return sqrt(sf2) * sd * sc;
}

// One pooled sample's two addends: lmn1, lmn2 the int64 window sums of L, M, N 100 of both images at the sample, g1, g2 the
// gradient magnitudes, p1, p2 the raw window sums of the full-resolution maps, cover the in-image samples of the window,
// mm = min VS1, max VS1, min VS2, max VS2, ff = F^2.
VSI_HD inline void vsi_sample(double g1, double g2, double m1, double m2, double n1, double n2, double p1, double p2, double cover,
                              const double *mm, double ff, double *s, double *wgt)
{
    const double v1 = ((p1 - mm[0] * cover) / (mm[1] - mm[0])) / ff, v2 = ((p2 - mm[2] * cover) / (mm[3] - mm[2])) / ff;
    // fmax drops a NaN: a flat map's 0 / 0 must reach the sums
    const double vm = (v1 != v1 || v2 != v2) ? v1 + v2 : (v1 > v2 ? v1 : v2);
    const double s_vs = vsi_sim(v1, v2, VSI_C1), s_g = vsi_sim(g1, g2, VSI_C2);
    const double s_c = vsi_sim(m1, m2, VSI_C3) * vsi_sim(n1, n2, VSI_C3);
    *s = pow(s_g, VSI_ALPHA) * s_vs * vsi_chroma_weight(s_c) * vm;
    *wgt = vm;
}

// min / max that keep a NaN
VSI_HD inline double vsi_min(double a, double b) { return (a != a || b != b) ? a + b : (a < b ? a : b); }
VSI_HD inline double vsi_max(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }

// A composite axis of the pooled map: sample i is sum_b w[i * band + b] V[lo[i] + b] -- the up-resize rows of the in-image
// part of window i added up (weight 0 past the last index in use); cover[i] counts those rows.
struct VsiBand {
    int n_out = 0, band = 0;
    std::vector<double> w;
    std::vector<int32_t> lo, cover;
};

struct VsiTables {
    ImrAxis sy, sx;                         // the shrink h -> 256, w -> 256
    ImrAxis uy, ux;                         // the up-resize 256 -> h, 256 -> w
    VsiBand cy, cx;                         // ... pooled by F along each axis
};

struct VsiPlan {
    int h, w, cn, F;
    int rows, cols;                         // the pooled plane
    size_t n;                               // rows * cols
    int pool_gx;                            // column blocks of the pooling launch (rows on the grid's y)
    int order;                              // the shrink: 0 the vertical pass first, 1 the horizontal (imresize's rule)
    int expand_gx, expand_gy;               // blocks of the min / max pass
    size_t score_blocks;
    // byte offsets into the workspace
    size_t off_pool;                        // int64 [2 images][L, M, N][n]
    size_t off_lg, off_sd, off_tw;          // double [65536] each, then the 256 complex forward twiddles
    size_t off_w[6], off_idx[6];            // sy, sx, uy, ux: weights and reflected indices; cy, cx: weights and lo
    size_t off_cover[2];                    // int32 cover of cy, cx
    size_t off_tmp;                         // double: the shrink's intermediate, then the expand's 256 x w, then 256 x cols
    size_t off_rgb, off_lab;                // double [3][65536] each
    size_t off_c0, off_c1;                  // complex [3][65536] each: the transform's ping and pong
    size_t off_vs256;                       // double [65536]
    size_t off_range;                       // double [2 images][8]: min a, max a, min b, max b, min VS, max VS
    size_t off_rpart;                       // double [256][4]: per-block ranges of a and b
    size_t off_mpart;                       // double [expand_gx * expand_gy][2]
    size_t off_pvs;                         // double [2 images][n]: raw window sums of the full-resolution map
    size_t off_part, off_buf0, off_buf1;    // the score's per-block partials (2 sums) and their reduction
    size_t total;
};

// Every refusal of a call that depends on the shape, then the sizes, the axis tables and the workspace layout.  F = 0: the
// metric's own F with its bounds (cn 3 or 4, sides >= 16, F <= 256) and every table; F >= 1: the pooling's inspection form,
// which bounds F alone and builds no table (t may be null).
int vsi_plan(const char *scope, int h, int w, int cn, int F, VsiPlan *p, VsiTables *t);
// LG and SD on the 256 x 256 grid (either may be null), LG as the transform indexes it (DC first)
void vsi_filter(double *lg, double *sd);
// One triangle axis (imresize 'bilinear', antialiased when it shrinks)
int vsi_axis(const char *scope, int n_in, int n_out, ImrAxis *a);
