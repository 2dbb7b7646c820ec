// sr_vif.h -- what the host unit (sr_vif_host.cpp: plans, windows, values, every refusal) and the kernels (sr_vif.hip,
// sr_gmsd.hip) of VIF and GMSD share.  The definitions are in include/sr_hip.h.  Internal: nothing here is part of the C ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sr_internal.h"

// ---- VIF ---------------------------------------------------------------------------------------------------------------------
constexpr int VIF_SCALES = 4;
constexpr int VIF_MAX_TAPS = 17;
constexpr int VIF_MIN_SIDE = 41;            // one sample at scale 4
constexpr int VIF_TX_U8 = 256;              // threads = columns of a block of the two kernels that read the u8 images
constexpr int VIF_TX_F64 = 128;             // ... of the kernels that read the float64 planes of scales 2 .. 4
constexpr int VIF_ROWS = 128;               // longest chunk of rows a block marches down
constexpr int VIF_ROWS_MIN = 16;            // shortest chunk a small plane is cut into ...
constexpr int VIF_BLOCKS = 1024;            // ... to reach this many blocks
constexpr int VIF_GRID_Y = 65535;           // column blocks of one launch, at most

// window side of scale s (0-based): 17, 9, 5, 3
constexpr int vif_taps(int s) { return (16 >> s) + 1; }
// map columns a block of tx threads produces with an n-tap window (k_vif_stats): 240 | 120, 124, 126
constexpr int vif_stats_out(int tx, int n) { return tx - (n - 1); }
// decimated columns a block of tx threads produces with an n-tap window (k_vif_down): 124 | 62, 63
constexpr int vif_down_out(int tx, int n) { return (tx - n) / 2 + 1; }

struct VifLaunch {
    int tx, step, gx, gy;                   // threads, rows per chunk, chunks, column blocks
};

struct VifScale {
    int n;                                  // taps
    int h, w;                               // the scale's planes
    int mh, mw;                             // its map (valid region)
    uint64_t count;
    VifLaunch stats;                        // the launch that sums this scale
    VifLaunch down;                         // the launch that makes its planes from the scale before (s >= 1)
    size_t off_x, off_y;                    // its float64 planes in the scratch (s >= 1)
};

struct VifPlan {
    int ch, cw;                             // the cropped size
    VifScale s[VIF_SCALES];
    size_t nblk;                            // most blocks of a stats launch
    size_t off_part, off_buf0, off_buf1, total;
};

// Every refusal of a VIF call that depends on the shape, then the sizes, launches and scratch layout.
int vif_plan(const char *scope, int h, int w, int cn, int crop_border, int mode, VifPlan *p);
// The n = vif_taps(s) normalised taps of scale s (0-based).
void vif_window(int s, double *taps);

// ---- GMSD --------------------------------------------------------------------------------------------------------------------
constexpr int GMSD_MIN_SIDE = 4;
constexpr int GMSD_TW = 64, GMSD_TH = 16;   // samples of the half-size map one block owns
constexpr int GMSD_THREADS = 256;

struct GmsdPlan {
    int ch, cw;                             // the cropped size
    int h2, w2;                             // the half-size map
    uint64_t count;
    int tiles_x, tiles_y;
    size_t off_part, off_buf0, off_buf1, total;
};

int gmsd_plan(const char *scope, int h, int w, int cn, int crop_border, int mode, GmsdPlan *p);
