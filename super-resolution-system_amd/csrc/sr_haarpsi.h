// sr_haarpsi.h -- what the host unit (sr_haarpsi_host.cpp: the plan, the host restatement, the values, every refusal) and the
// kernels (sr_haarpsi.hip) of HaarPSI share.  The definition is in include/sr_hip.h.  The per-sample float64 arithmetic is
// written ONCE, here, for the host and the device alike: the same expressions in the same order (the build has fp contraction
// off), so the two differ only by the math library behind exp.  Internal: nothing here is part of the C ABI.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "sr_internal.h"

#if defined(__HIP__)        // spelled as attributes: the host unit is compiled without the HIP runtime header
#define HP_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define HP_HD inline
#endif

constexpr int HP_MIN_SIDE = 2;
constexpr int HP_TW = 64, HP_TH = 16;       // samples one block owns
constexpr int HP_THREADS = 256;
constexpr int HP_HALO = 7;                  // 3 + o samples before and 4 - o after a tile: the 8 x 8 window of scale 3
constexpr int HP_SH = HP_TH + HP_HALO, HP_SW = HP_TW + HP_HALO;     // the luma planes a block holds
constexpr int HP_CH = HP_TH + 1, HP_CW = HP_TW + 1;                 // the chroma planes: the 2 x 2 window alone
constexpr int HP_COMP = 6;                  // num[3], den[3]
constexpr double HP_C = 30.0, HP_ALPHA = 4.2;

struct HpPlan {
    int ch, cw;                             // the cropped size
    int mh, mw;                             // the sample map: the half size with subsampling, else the cropped size
    int channels;                           // 2 (gray) or 3 (colour)
    uint64_t count;
    int tiles_x, tiles_y;
    size_t off_part, off_buf0, off_buf1, total;     // context scratch: the per-block partials and their reduction
};

// Every refusal of a call that depends on shape, channels, crop and the two switches, then the launch and the scratch layout.
int haarpsi_plan(const char *scope, int h, int w, int cn, int crop_border, int subsample, int convention, HpPlan *p);

// 1000 Y, 1000 I, 1000 Q of one pixel (exact integers)
HP_HD int hp_y(int r, int g, int b) { return 299 * r + 587 * g + 114 * b; }
HP_HD int hp_i(int r, int g, int b) { return 596 * r - 274 * g - 322 * b; }
HP_HD int hp_q(int r, int g, int b) { return 211 * r - 523 * g + 312 * b; }

// Sample (i, j) of the three integer planes of one image whose cropped rectangle starts at img: the 2 x 2 sum at pixel
// (2 i - o, 2 j - o) with zero outside the rectangle (SUB), or pixel (i, j) itself.  The caller keeps (i, j) inside the map.
template <int CN, bool SUB>
HP_HD void hp_pool(const unsigned char *img, long long stride, int ch, int cw, int o, int i, int j, int &y, int &ci, int &cq)
{
    y = ci = cq = 0;
    constexpr int N = SUB ? 2 : 1;
#pragma unroll
    for (int dy = 0; dy < N; ++dy) {
        const int r = SUB ? 2 * i - o + dy : i;
        if (r < 0 || r >= ch) continue;
        const unsigned char *row = img + (size_t)r * (size_t)stride;
#pragma unroll
        for (int dx = 0; dx < N; ++dx) {
            const int c = SUB ? 2 * j - o + dx : j;
            if (c < 0 || c >= cw) continue;
            const unsigned char *p = row + (size_t)c * CN;
            if constexpr (CN == 1) {
                y += 1000 * p[0];
            } else {
                const int R = p[0], G = p[1], B = p[2];
                y += hp_y(R, G, B);
                ci += hp_i(R, G, B);
                cq += hp_q(R, G, B);
            }
        }
    }
}

// |v| / unit, rounded once
HP_HD double hp_coef(int v, double unit) { return (double)(v < 0 ? -v : v) / unit; }

HP_HD double hp_sim(double a, double b) { return (2.0 * a * b + HP_C) / ((a * a + b * b) + HP_C); }

HP_HD double hp_sigmoid(double ls) { return 1.0 / (1.0 + exp(-HP_ALPHA * ls)); }

// One sample.  va[d][s], vb[d][s]: the integer Haar sums of the two images (d = 0: row difference V, 1: column difference H;
// s = 0 .. 2); ia, qa, ib, qb: the integer 2 x 2 chroma sums (COLOUR only); div: 1000 or 4000.  Stores w sigma(LS) in num[ch]
// and w in den[ch] for the 2 or 3 channels.
template <bool COLOUR>
HP_HD void hp_sample(const int (&va)[2][3], const int (&vb)[2][3], int ia, int qa, int ib, int qb, double div, double *num,
                     double *den)
{
    double w[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const double a1 = hp_coef(va[d][0], div * 2.0), b1 = hp_coef(vb[d][0], div * 2.0);
        const double a2 = hp_coef(va[d][1], div * 4.0), b2 = hp_coef(vb[d][1], div * 4.0);
        const double a3 = hp_coef(va[d][2], div * 8.0), b3 = hp_coef(vb[d][2], div * 8.0);
        w[d] = a3 > b3 ? a3 : b3;
        const double ls = 0.5 * (hp_sim(a1, b1) + hp_sim(a2, b2));
        num[d] = w[d] * hp_sigmoid(ls);
        den[d] = w[d];
    }
    if constexpr (COLOUR) {
        const double ls = 0.5 * (hp_sim(hp_coef(ia, div * 4.0), hp_coef(ib, div * 4.0)) +
                                 hp_sim(hp_coef(qa, div * 4.0), hp_coef(qb, div * 4.0)));
        const double wc = 0.5 * (w[0] + w[1]);
        num[2] = wc * hp_sigmoid(ls);
        den[2] = wc;
    }
}
