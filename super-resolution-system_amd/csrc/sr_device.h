// sr_device.h -- device helpers shared by sr_engine.hip (blend engine), sr_tiles.hip (stand-alone tile kernels),
// sr_assess.hip (quality assessment), sr_msssim.hip and sr_srbench.hip (the SSIM helpers those share are in sr_ssim11.h):
// border rules, vector load / store typedefs, the integer RGB -> gray of
// cv2.cvtColor, the tile-source descriptor with its data-type tags, and the shared-reciprocal division.
#pragma once
#include <hip/hip_runtime.h>

enum { PAD_MIRROR = 0, PAD_REPLICATE = 1, PAD_REFLECT = 2, PAD_CONSTANT = 3 };

__device__ __forceinline__ int border_index(int p, int n, int mode)
{
    if (p >= 0 && p < n) return p;
    if (mode == PAD_REPLICATE) return p < 0 ? 0 : n - 1;
    if (n == 1) return 0;
    const int delta = (mode == PAD_MIRROR) ? 1 : 0;
    while (p < 0 || p >= n) {
        if (p < 0) p = -p - 1 + delta;
        else p = n - 1 - (p - n) - delta;
    }
    return p;
}

__device__ __forceinline__ int reflect101(int p, int n) { return border_index(p, n, PAD_MIRROR); }

// Vector load / store helpers.  The *_aN typedefs carry a reduced alignment so the compiler may emit one wide
// global_load for an address that is only float- (or byte-) aligned; gfx950 handles those in hardware.
typedef float f4_t __attribute__((ext_vector_type(4)));
typedef float f2_t __attribute__((ext_vector_type(2)));
typedef unsigned u4_t __attribute__((ext_vector_type(4)));
typedef unsigned u3_t __attribute__((ext_vector_type(3)));
typedef unsigned u2_t __attribute__((ext_vector_type(2)));
typedef f4_t f4_a4_t __attribute__((aligned(4)));    // 4 floats at any float-aligned address
typedef f2_t f2_a8_t __attribute__((aligned(8)));
typedef u3_t u3_a1_t __attribute__((aligned(1)));    // 12 bytes at any address
typedef u4_t u4_a1_t __attribute__((aligned(1)));    // 16 bytes at any address
typedef u4_t u4_a4_t __attribute__((aligned(4)));
typedef unsigned u1_a1_t __attribute__((aligned(1)));

__device__ __forceinline__ f4_t ld_f4_a4(const float *p) { return *(const f4_a4_t *)p; }
__device__ __forceinline__ f4_t ld_f4(const float *p) { return *(const f4_t *)p; }
__device__ __forceinline__ void st_f4(float *p, f4_t v) { *(f4_t *)p = v; }
__device__ __forceinline__ u3_t ld_u3_a1(const void *p) { return *(const u3_a1_t *)p; }
// Same through a global-address-space pointer: for addresses that come out of a descriptor table in memory (tile
// pointers), where the compiler would otherwise emit flat_load (both wait counters, aperture check).
__device__ __forceinline__ u3_t ld_u3_a1_g(const void *p)
{
    return *(const __attribute__((address_space(1))) u3_a1_t *)p;
}

// cv2.cvtColor(RGB2GRAY) of u8 data in fixed point; shift = the fractional bits (15, or 14) the caller's OpenCV uses.
__device__ __forceinline__ int gray_rgb(int r, int g, int b, int shift)
{
    return shift == 15 ? (r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15
                       : (r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14;
}

// Level-0 data of one tile (row 0, possibly virtual) and its row stride in bytes; the SRC_* tags select how a kernel
// reads it (SRC_PLANAR, SRC_LUT: the engine's pyrDown sources).
struct TileSrc {
    const void *p;
    long long stride;
};

enum { SRC_U8 = 0, SRC_F32 = 1, SRC_PLANAR = 2, SRC_LUT = 3 };

// a / w for the channels of one pixel, IEEE-correct: exactly the fma chain the compiler emits for an fp32 division
// (rcp, one Newton step, quotient, two residual corrections) without the v_div_scale / v_div_fixup wrapping, which is
// the identity for these operands (w in [1e-6, n_tiles], |a| a few thousand at most) -- and with the reciprocal
// refined once per pixel instead of once per channel.
template <int CN>
__device__ __forceinline__ void div_shared(const float (&a)[CN], float w, float (&q)[CN])
{
    float r = __builtin_amdgcn_rcpf(w);
    r = fmaf(fmaf(-w, r, 1.0f), r, r);
    if (CN == 3) {
        // channels 0 and 1 as one packed pair (v_pk_mul / v_pk_fma: the same fma chain per element), channel 2 scalar
        f2_t a01, nw, rr;
        a01.x = a[0]; a01.y = a[1];
        nw.x = nw.y = -w;
        rr.x = rr.y = r;
        f2_t t = a01 * rr;
        t = __builtin_elementwise_fma(__builtin_elementwise_fma(nw, t, a01), rr, t);
        t = __builtin_elementwise_fma(__builtin_elementwise_fma(nw, t, a01), rr, t);
        q[0] = t.x;
        q[1] = t.y;
        float t2 = a[2] * r;
        t2 = fmaf(fmaf(-w, t2, a[2]), r, t2);
        q[2] = fmaf(fmaf(-w, t2, a[2]), r, t2);
        return;
    }
#pragma unroll
    for (int c = 0; c < CN; ++c) {
        float t = a[c] * r;
        t = fmaf(fmaf(-w, t, a[c]), r, t);
        q[c] = fmaf(fmaf(-w, t, a[c]), r, t);
    }
}
