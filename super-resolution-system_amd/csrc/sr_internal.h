// Internal declarations shared by sr_host.cpp (pure host bookkeeping), the blend planner (sr_blend_plan.cpp plans with
// them) and the device sources (every .hip file reports errors through sr_set_error).
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>

#include "sr_hip.h"

#define SR_MAX_LEVELS 16

int sr_set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// Sections of a device workspace start at multiples of 256 bytes.
inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct SrWin {
    int a, b;  // [a, b)
    bool empty() const { return a >= b; }
};

// Row windows of one tile for a canvas row range (see DESIGN.md "strip windows").
struct SrTileLevels {
    int nl;                           // levels actually built (>= 1)
    int H[SR_MAX_LEVELS], W[SR_MAX_LEVELS];
    SrWin gw[SR_MAX_LEVELS];          // rows of G_i (i == 0: rows of the input tile) that are read
    SrWin rw[SR_MAX_LEVELS];          // rows of R_i that are produced (i >= 1)
    SrWin cw;                         // tile-local rows the final gather reads
};

void sr_level_dims(int h, int w, int levels, int *nl, int *H, int *W);
void sr_plan_windows(int tile_h, int tile_w, int tile_y, int levels, int row_begin, int row_end,
                     int canvas_h, SrTileLevels *out);

// Geometric self-ensemble (sr_host.cpp plans, sr_ensemble.hip runs): members of a mask and the workspace of one call.  The
// workspace is one allocation of three sections, each starting at a multiple of 256 bytes: the accumulator (H x W x 3 fp32,
// H = h scale, W = w scale), one forward output (H x W, and W x H when a transposing member is in use) and the transformed u8
// input (h x w and / or w x h; absent when member 0 is the only one).  A row of r bytes has a stride of r rounded up to 16.
struct SrEnsLayout {
    int n = 0;                        // members in use
    int members[8] = {0};             // ascending
    size_t acc_off = 0, y_off = 0, in_off = 0, total = 0;
};
inline long long sr_ens_row_stride(long long row_bytes) { return (row_bytes + 15) / 16 * 16; }
// SR_ERR_INVALID_ARG for a mask outside 1..255.
int sr_ens_check_mask(const char *who, int mask);
// Every host-side refusal of sr_ens_plan; who names the caller in the message.
int sr_ens_layout(const char *who, int h, int w, int scale, int mask, SrEnsLayout *out);
