// sr_fsim.h -- what the host unit (sr_fsim_host.cpp: the plan, F, the filter planes and their sums, the twiddle tables, the
// value, every refusal) and the kernels (sr_fsim.hip) of FSIM / FSIMc share.  The definition is in include/sr_hip.h.
// Internal: nothing here is part of the C ABI.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "sr_internal.h"

constexpr int FSIM_MIN_SIDE = 16;           // of the images, and of a plane handed to sr_fsim_pc_f64
constexpr int FSIM_MAX_SIDE = 2048;         // longest pooled side: the dense transform costs rows * cols * (rows + cols)
constexpr int FSIM_SCALES = 4, FSIM_ORIENTS = 4;
constexpr int FSIM_POOL_THREADS = 256;      // threads = source columns of a pooling block: its row segment
constexpr int FSIM_MAX_F = FSIM_POOL_THREADS;   // one window fits a segment
constexpr int FSIM_DFT_TILE = 16;           // outputs per side and products per step of a transform block (16 x 16 threads)
constexpr int FSIM_THREADS = 256;           // the per-sample kernels, the histogram and the score
constexpr int FSIM_HIST_BLOCKS = 64;        // most blocks of a histogram launch
constexpr double FSIM_T1 = 0.85, FSIM_T2 = 160.0, FSIM_T34 = 200.0, FSIM_LAMBDA = 0.03;
constexpr double FSIM_EPSILON = 1e-4, FSIM_K = 2.0;

// windows of the pooling a block of FSIM_POOL_THREADS source columns holds: 256, 128, 85, 64, 51, ... 1
constexpr int fsim_pool_out(int F) { return FSIM_POOL_THREADS / F; }
// first source index of window i along an axis (can be negative: indices outside contribute 0); the window has F entries
constexpr long long fsim_win_start(long long i, int F) { return i * F + F / 2 - F + 1; }

// Re((si sq)^0.03): |z|^0.03, times cos(0.03 pi) for a negative product (the principal complex power)
#if defined(__HIP__)
__host__ __device__
#endif
inline double fsim_chroma_weight(double si, double sq)
{
    const double z = si * sq;
    const double p = pow(fabs(z), FSIM_LAMBDA);
    return z < 0.0 ? p * cos(FSIM_LAMBDA * 3.14159265358979323846) : p;
}

struct FsimPlan {
    int h, w, cn, F;
    int rows, cols;                         // the pooled plane
    size_t n;                               // rows * cols
    int pool_gx;                            // column blocks of the pooling launch (rows on the grid's y)
    size_t score_blocks;
    // byte offsets into the workspace
    size_t off_pool;                        // int64 [2 images][Y, I, Q][n]
    size_t off_filt;                        // double logGabor[4][n], then spread[4][n]
    size_t off_tw_r, off_tw_c;              // complex forward twiddles of both axes
    size_t off_plane;                       // double [n]: the float64 Y plane of the image at work
    size_t off_spec;                        // complex [n]: its spectrum
    size_t off_half;                        // complex [4][n]: the row-transformed planes (the forward pass uses the first)
    size_t off_eo;                          // complex [4][n]: EO of the four scales of one orientation (forward: the input)
    size_t off_pc;                          // double [2][n]
    size_t off_energy_all, off_an_all, off_energy, off_e2;   // double [n] each (e2: the keys of the median)
    size_t off_hist;                        // uint32 [2][256], then the select state
    size_t off_med;                         // double [2 images][4 medians, 4 thresholds]
    size_t off_part, off_buf0, off_buf1;    // the score's per-block partials (3 sums) and their reduction
    size_t total;
};

// F of an image (section 2 of the definition)
int fsim_auto_f(int h, int w);
// Every refusal of a call that depends on the shape, then the sizes and the workspace layout.  F = 0: the metric's own F
// with its bounds (sides >= 16, pooled sides <= 2048); F >= 1: the inspection form, which bounds F alone.
int fsim_plan(const char *scope, int h, int w, int cn, int F, FsimPlan *p);
// The layout for a plane handed in as float64 (sr_fsim_pc_f64): h = rows, w = cols, F = 1.
int fsim_plan_plane(const char *scope, int rows, int cols, FsimPlan *p);
// logGabor[4][rows * cols], spread[4][rows * cols] (either may be null) and EM_n, S2, Sij of the four orientations.
void fsim_filters(int rows, int cols, double *log_gabor, double *spread, double *em, double *s2, double *sij);
// (cos, -sin)(2 pi j / n), j = 0 .. n - 1, interleaved: the forward table; the inverse conjugates it
void fsim_twiddles(int n, double *tw);
