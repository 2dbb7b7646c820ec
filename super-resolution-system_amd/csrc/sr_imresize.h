// sr_imresize.h -- what the host unit (sr_imresize_host.cpp: tables, plan, every refusal) and the kernel (sr_imresize.hip) of
// MATLAB's bicubic imresize share.  The definition is in include/sr_hip.h.  Internal: nothing here is part of the C ABI.
#pragma once
#include <cstdint>
#include <vector>

#include "sr_internal.h"

constexpr int IMR_THREADS = 256;            // threads of one workgroup
constexpr int IMR_MAX_TAPS = 66;            // ceil(4 * 16) + 2
constexpr int IMR_LDS_DOUBLES = 6144;       // the float64 intermediate of one workgroup: 48 KB, three workgroups per CU
constexpr int IMR_TILE_A_MAX = 32;          // outputs of a tile along the first pass's axis, at most

// One axis: the normalised weights, the reflected 0-based indices and, per output, the unreflected 1-based index of its
// first kept tap (tap k of output i reads the unreflected index start[i] + k; idx holds its reflection).
struct ImrAxis {
    int n_in = 0, n_out = 0, taps = 0;
    double scale = 0.0;
    std::vector<double> w;
    std::vector<int32_t> idx, start;
};

// The geometry of one call.  The first pass runs along axis A (order 0: the height), the second along axis B.  A workgroup
// owns tile_a x tile_b outputs; its second pass reads at most span_b unreflected positions of axis B, an upper bound that
// depends on (scale, taps, tile_b) only and that imr_plan checks against the tables.
struct ImrPlan {
    int order = 0;
    int tile_a = 0, tile_b = 0, span_b = 0;
    long long tiles_a = 0, tiles_b = 0;
    size_t lds_bytes = 0;
    size_t off_w[2] = {0, 0}, off_idx[2] = {0, 0}, off_start[2] = {0, 0}, total = 0;   // [0]: the height's tables, [1]: the width's
};

// 0-based reflection of the 1-based unreflected index u on an axis of n samples (MATLAB's symmetric padding, any distance)
inline int imr_reflect(long long u, int n)
{
    long long j = (u - 1) % (2LL * n);
    if (j < 0) j += 2LL * n;
    return (int)(j >= n ? 2LL * n - 1 - j : j);
}

// Every refusal of one axis, then its tables.  scope names the caller in the message.
int imr_axis(const char *scope, int n_in, int n_out, double scale, int antialias, ImrAxis *a);
// The same contribution rule with the kernel named and no [1/16, 16] range on the scale: the cubic (support 4: what imr_axis
// builds) or the triangle t(x) = max(0, 1 - |x|) (support 2: imresize's 'bilinear', which VSI resizes by; sr_vsi_host.cpp).
// trim drops the taps that are zero for every output at both ends (imr_axis does); without it all P = ceil(kw) + 2 stay.
enum ImrKernel { IMR_CUBIC = 0, IMR_TRIANGLE = 1 };
int imr_axis_kernel(const char *scope, int n_in, int n_out, double scale, int antialias, ImrKernel kernel, bool trim, ImrAxis *a);
// Every shape refusal of a call, both axes' tables and the geometry.
int imr_plan(const char *scope, int h, int w, int cn, double scale_y, double scale_x, int dh, int dw, int antialias, ImrAxis *ay,
             ImrAxis *ax, ImrPlan *p);
