// sr_linear.h -- cv::resize INTER_LINEAR on u8 data (half-pixel centres, 11-bit fixed-point coefficients), shared by
// TilingModule.merge_tiles' resize branch (k_feather_merge, sr_tiles.hip) and compute_blend_quality's resize of a tile
// clipped by the canvas (sr_gradient.hip).  Internal: nothing here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

struct LinTab {
    int ofs;       // left / top source index (clamped)
    short a0, a1;  // 11-bit coefficients of cv::resize INTER_LINEAR (u8 data)
    float f;       // the fraction itself (float data: coefficients 1 - f and f)
};

// Appends the n_dst entries of one axis (source length n_src) to `tab`.
static inline void linear_table(int n_src, int n_dst, std::vector<LinTab> &tab)
{
    const size_t base = tab.size();
    tab.resize(base + n_dst);
    const double scale = 1.0 / ((double)n_dst / (double)n_src);
    for (int d = 0; d < n_dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= (float)s;
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= n_src - 1) { f = 0.f; s = n_src - 1; }
        LinTab &t = tab[base + d];
        t.ofs = s;
        t.a0 = (short)rintf((1.0f - f) * 2048.0f);
        t.a1 = (short)rintf(f * 2048.0f);
        t.f = f;
    }
}

// One u8 output sample: r0 / r1 are the source rows Y.ofs and min(Y.ofs + 1, h - 1), i0 / i1 the byte offsets of the
// element in columns X.ofs and min(X.ofs + 1, w - 1).
__device__ __forceinline__ int lin_u8(const unsigned char *r0, const unsigned char *r1, int i0, int i1, const LinTab &X,
                                      const LinTab &Y)
{
    const int s0 = (int)r0[i0] * X.a0 + (int)r0[i1] * X.a1;
    const int s1 = (int)r1[i0] * X.a0 + (int)r1[i1] * X.a1;
    return (((Y.a0 * (s0 >> 4)) >> 16) + ((Y.a1 * (s1 >> 4)) >> 16) + 2) >> 2;
}
