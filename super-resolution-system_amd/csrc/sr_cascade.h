// sr_cascade.h -- what sr_cascade.hip (planes, summed-area tables, window evaluation on the GPU) and sr_cascade_host.cpp
// (model checks and packing, the scale list and plan, every refusal, the canonical order, the grouping, the host
// restatement) share: the packed model, the plan, and the evaluation of one window, which both sides compile from the one
// text below (integer arithmetic, float32 additions, float64 products and sums without contraction: the same bits on both).
// Internal: nothing here is part of the C ABI.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "sr_internal.h"

#ifdef __HIP__
#include <hip/hip_runtime.h>
#define CC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define CC_HD inline
#endif

#define CC_MAX_PIXELS (1LL << 24)            // like MSER
#define CC_MAX_INDEX 2147483647LL             // samples, table elements and positions of a pyramid: the kernels index in int32
#define CC_MIN_SIDE 3                        // the 3 x 3 LBP grid and the normalisation rectangle (1, 1, W0 - 2, H0 - 2)
#define CC_MAX_SIDE 255                      // coordinates pack into bytes; a box sum of squares stays below 2^32
#define CC_MAX_STAGES 4096
#define CC_MAX_STUMPS 65536
#define CC_STUMP_WORDS 12
#define CC_DENSE_STUMPS 64                   // the leading stages evaluated densely from LDS hold at most this many stumps
#define CC_DENSE_STAGES 64                   // ... and are at most this many (a stage may hold no stump at all)
#define CC_MAGIC 0x43534344u

// A packed stump, CC_STUMP_WORDS 32-bit words, its feature resolved into it (x | y << 8 | w << 16 | h << 24):
//   LBP : [0] the top-left block, [1..8] the subset words, [9] leaf 0, [10] leaf 1
//   HAAR: [0] the rectangle count, [1] threshold, [2] leaf 0, [3] leaf 1, [4 + 2 i] rectangle i, [5 + 2 i] its weight
struct CcStage {
    int first, count;                        // stumps [first, first + count)
    float thr;
    int pad;
};

struct sr_cascade {
    unsigned magic = CC_MAGIC;
    sr_cascade_info info{};
    std::vector<CcStage> stages;
    std::vector<uint32_t> stumps;
    int dense_stages = 0, dense_stumps = 0;  // the leading stages of the dense kernel (0: the first stage alone is too long)
};

// One scale as the kernels see it (offsets: bytes into the planes, elements into a table, indices of the flattened lists).
struct CcScale {
    int sw, sh, step, nx, ny;
    int pix_off, tab_off, pos_off, row_off, col_off;
    int pad0, pad1;
};

// The plan of one call.  Workspace sections start at multiples of 256 bytes and every section is written before it is read.
struct CcPlan {
    std::vector<sr_cascade_scale> scales;
    std::vector<CcScale> dev;
    long long npx = 0, plane_px = 0, table_el = 0, positions = 0, rows = 0, cols = 0;
    size_t off_gray = 0;      // u8  [npx]        g
    size_t off_planes = 0;    // u8  [plane_px]   the scaled planes, scale after scale
    size_t off_tab = 0;       // u32 [table_el]   summed-area tables, (sw + 1) x (sh + 1) per scale, wrapping
    size_t off_sq = 0;        // u32 [table_el]   HAAR: the tables of squares
    size_t off_stumps = 0, off_stages = 0, off_scales = 0;
    size_t off_ctr = 0;       // u32 [64]         [0] survivors of the dense stages, [1] detections
    size_t off_surv = 0;      // u32 [positions]  position indices that passed the dense stages
    size_t off_cand = 0;      // u32 [positions]  position indices of the detections (any order; the host sorts them)
    size_t total = 0;
};

bool cascade_is_live(const sr_cascade *m);
// Every refusal of the arguments (SR_ERR_UNSUPPORTED / SR_ERR_INVALID_ARG), the scale list and the layout.
int cascade_plan(const char *who, const sr_cascade *m, int h, int w, const sr_cascade_params *p, CcPlan *out);
// A plan of the scale-0 plane alone with the given step (the stage map).
int cascade_plan_map(const char *who, const sr_cascade *m, int h, int w, int step, CcPlan *out);
// Position indices (sorted: scale, y, x) -> candidates.
void cascade_candidates(const CcPlan &pl, const uint32_t *pos, size_t n, sr_tile_rect *out);

CC_HD float cc_f32(uint32_t v)
{
    float f;
    __builtin_memcpy(&f, &v, 4);
    return f;
}

// Box sum of [x, x + w) x [y, y + h) from a (sw + 1)-pitched table; the unsigned differences wrap back to the true sum.
CC_HD uint32_t cc_box(const uint32_t *T, int pitch, int x, int y, int w, int h)
{
    const uint32_t *p = T + y * pitch + x;
    return p[0] - p[w] - p[h * pitch] + p[h * pitch + w];
}

// true: the stump takes leaf 0
CC_HD bool cc_lbp_first(const uint32_t *st, const uint32_t *T, int pitch, int x, int y)
{
    const uint32_t r = st[0];
    const int bw = (int)(r >> 16 & 255u), bh = (int)(r >> 24);
    const uint32_t *p = T + (y + (int)(r >> 8 & 255u)) * pitch + x + (int)(r & 255u);
    uint32_t P[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) P[i][j] = p[i * bh * pitch + j * bw];
#define CC_B(i, j) (P[i][j] - P[i][j + 1] - P[i + 1][j] + P[i + 1][j + 1])
    const uint32_t c = CC_B(1, 1);
    const uint32_t code = (uint32_t)(CC_B(0, 0) >= c) << 7 | (uint32_t)(CC_B(0, 1) >= c) << 6 | (uint32_t)(CC_B(0, 2) >= c) << 5 |
                          (uint32_t)(CC_B(1, 2) >= c) << 4 | (uint32_t)(CC_B(2, 2) >= c) << 3 | (uint32_t)(CC_B(2, 1) >= c) << 2 |
                          (uint32_t)(CC_B(2, 0) >= c) << 1 | (uint32_t)(CC_B(1, 0) >= c);
#undef CC_B
    return (st[1 + (code >> 5)] >> (code & 31u) & 1u) != 0u;
}

CC_HD bool cc_haar_first(const uint32_t *st, const uint32_t *T, int pitch, int x, int y, double nf)
{
    const int n = (int)st[0];
    double val = 0.0;
    for (int i = 0; i < n; ++i) {
        const uint32_t r = st[4 + 2 * i];
        const uint32_t s = cc_box(T, pitch, x + (int)(r & 255u), y + (int)(r >> 8 & 255u), (int)(r >> 16 & 255u), (int)(r >> 24));
        const double prod = (double)cc_f32(st[5 + 2 * i]) * (double)s;
        val = i ? val + prod : prod;
    }
    const double lim = (double)cc_f32(st[1]) * nf;
    return val < lim;
}

// nf of the window at (x, y): from the rectangle (1, 1, W0 - 2, H0 - 2)
CC_HD double cc_norm(const uint32_t *T, const uint32_t *S, int pitch, int x, int y, int W0, int H0)
{
    const long long A = (long long)(W0 - 2) * (H0 - 2);
    const long long s = cc_box(T, pitch, x + 1, y + 1, W0 - 2, H0 - 2), q = cc_box(S, pitch, x + 1, y + 1, W0 - 2, H0 - 2);
    const long long v = A * q - s * s;
    return v > 0 ? sqrt((double)v) : 1.0;
}

// Stages [s0, s1) on the window at (x, y): how many of them it passes before the first it fails.  stumps points at the stump
// numbered stump_base (the dense kernel holds the leading stumps in LDS, the tail reads the whole table).
CC_HD int cc_run(const CcStage *stages, const uint32_t *stumps, int stump_base, int s0, int s1, int type, const uint32_t *T,
                 const uint32_t *S, int pitch, int x, int y, int W0, int H0)
{
    const double nf = type == SR_CASCADE_HAAR ? cc_norm(T, S, pitch, x, y, W0, H0) : 1.0;
    for (int s = s0; s < s1; ++s) {
        const CcStage g = stages[s];
        float sum = 0.f;
        for (int k = 0; k < g.count; ++k) {
            const uint32_t *st = stumps + (size_t)(g.first - stump_base + k) * CC_STUMP_WORDS;
            if (type == SR_CASCADE_HAAR) sum = sum + cc_f32(st[cc_haar_first(st, T, pitch, x, y, nf) ? 2 : 3]);
            else sum = sum + cc_f32(st[cc_lbp_first(st, T, pitch, x, y) ? 9 : 10]);
        }
        if (sum < g.thr) return s - s0;
    }
    return s1 - s0;
}

// One sample of the scaled plane (sw x sh) of the gray plane g (w x h): the exact-integer bilinear rule of the definition.
CC_HD int cc_resample(const unsigned char *g, int w, int h, int sw, int sh, int x, int y)
{
    const long long nx = (2LL * x + 1) * w - sw, dx = 2LL * sw, ny = (2LL * y + 1) * h - sh, dy = 2LL * sh;
    const long long ix = nx / dx, rx = nx - ix * dx, iy = ny / dy, ry = ny - iy * dy;      // nx, ny >= 0: sw <= w, sh <= h
    const int x0 = (int)(ix < w - 1 ? ix : w - 1), x1 = (int)(ix + 1 < w - 1 ? ix + 1 : w - 1);
    const int y0 = (int)(iy < h - 1 ? iy : h - 1), y1 = (int)(iy + 1 < h - 1 ? iy + 1 : h - 1);
    const unsigned char *r0 = g + (size_t)y0 * w, *r1 = g + (size_t)y1 * w;
    const long long acc = (dy - ry) * ((dx - rx) * r0[x0] + rx * r0[x1]) + ry * ((dx - rx) * r1[x0] + rx * r1[x1]);
    const long long D = dx * dy;
    return (int)((acc + D / 2) / D);
}
