// sr_net_common.h -- what the five local SR backends (sr_srnet.hip, sr_resnet.hip, sr_rrdb.hip, sr_rcan.hip, sr_swinir.hip) share around the convolution
// mainloop of sr_conv_mfma.h: the head frame and the per-element pieces of their epilogues, the planar-tensor and
// backward-extent geometry of their layer walks, and the lifetime of their models.  sr_lpips.hip needs none of it and includes
// the mainloop header alone.  Internal: nothing here is part of the C ABI.
// Not here: a frame for the convolution epilogue's (pr, c2, r) loop nest.  Moved into a function template it is optimised before
// it is inlined, the kernels' register counts move, and k_rn_conv / k_rr_conv cross an occupancy step that costs
// time; the nest stays written out in each kernel.
#pragma once
#include <algorithm>
#include <climits>
#include <functional>

#include "sr_conv_mfma.h"

// ---- device side --------------------------------------------------------------------------------------------------

__device__ __forceinline__ float leaky(float y, float slope) { return y >= 0.0f ? y : slope * y; }

// Offset of pixel (gy, gx) inside one plane of a planar tensor with origin (ya, xa).
__device__ __forceinline__ size_t skip_offset(int gy, int gx, int ya, int xa, int pitch) { return (size_t)(gy - ya) * pitch + (gx - xa); }

// Element e of an HWC output row: fp32 as it is, u8 clamped to [0, 1], scaled, rounded half to even.
template <bool U8>
__device__ __forceinline__ void store_hwc(char *d, size_t e, float o)
{
    if constexpr (U8) ((unsigned char *)d)[e] = (unsigned char)rintf(fminf(fmaxf(o, 0.0f), 1.0f) * 255.0f);
    else ((float *)d)[e] = o;
}

// The head frame (block 64 x 4, blockIdx.z: 64-cout tile): thread -> pixel, head_accumulate, then act(cout inside the tile,
// value) into the 64 planes.  The kernel fills its table and synchronises before the call.
template <int LUT_CS, typename Act>
__device__ __forceinline__ void head_frame(const unsigned char *__restrict__ img, long long stride, int H, int W,
                                           const float *__restrict__ wt, const float *__restrict__ bias, const float *lut,
                                           float *__restrict__ out, int ya, int xa, int rows, int cols, int pitch, long long plane, Act &&act)
{
    const int lx = blockIdx.x * 64 + threadIdx.x, ly = blockIdx.y * 4 + threadIdx.y, ct = blockIdx.z;
    if (lx >= cols || ly >= rows) return;
    float acc[64];
    head_accumulate<LUT_CS>(img, stride, H, W, wt, bias, ct, lut, ya + ly, xa + lx, acc);
    float *o = out + (size_t)ct * 64 * plane + (size_t)ly * pitch + lx;
#pragma unroll
    for (int co = 0; co < 64; ++co) o[(size_t)co * plane] = act(co, acc[co]);
}

// ---- host side ----------------------------------------------------------------------------------------------------

inline long long pad4(long long v) { return (v + 3) / 4 * 4; }

// A planar tensor: element (c, gy, gx) at p[c * plane + (gy - ya) * pitch + gx - xa]; rows x cols is what the buffer holds.
struct PlanarTen {
    float *p = nullptr;
    int ya = 0, xa = 0, rows = 0, cols = 0, pitch = 0;
    long long plane = 0;
};

inline PlanarTen planar_tensor(float *p, int ya, int xa, int rows, int cols)
{
    PlanarTen t;
    t.p = p; t.ya = ya; t.xa = xa; t.rows = rows; t.cols = cols;
    t.pitch = (int)pad4(cols);
    t.plane = (long long)rows * t.pitch;
    return t;
}

// One convolution of a layer walk, as the extent rule sees it: the replication (shuffle) factor behind it and the resolution
// multiplier of its own output.
struct ExtStep {
    int r, mult;
};

// One axis of the backward extent rule: the piece [lo, hi) of an axis of len input pixels, out_mult x at the output -> per
// convolution the half-open range [a[i], b[i]) of its output at its own resolution: backwards, divided by r (rounded outwards),
// then grown by one and clipped to the layer's image.
inline void backward_extents(const ExtStep *steps, int n, int out_mult, int lo, int hi, int len, std::vector<int> &a, std::vector<int> &b)
{
    a.resize(n);
    b.resize(n);
    long long na = (long long)lo * out_mult, nb = (long long)hi * out_mult;
    for (int i = n - 1; i >= 0; --i) {
        const int r = steps[i].r;
        na = na / r;                                       // outward: floor, ceil
        nb = (nb + r - 1) / r;
        a[i] = (int)na;
        b[i] = (int)nb;
        na = std::max(na - 1, 0LL);
        nb = std::min(nb + 1, (long long)len * steps[i].mult);
    }
}

// Input pixels a piece reads beyond its own edge: the rule above without clipping.
inline int backward_halo(const ExtStep *steps, int n)
{
    int g = 0;
    for (int i = n - 1; i >= 0; --i) g = (g + steps[i].r - 1) / steps[i].r + 1;
    return g;
}

// The convolution launch of sr_resnet.hip, sr_rrdb.hip, sr_rcan.hip, sr_swinir.hip and sr_hat.hip.  in: the tensor read (its first cin planes); out: pointer to the
// element (cout 0, ya, xa) of the output -- or, for a replicating or shuffling epilogue, of the output at its own resolution.
template <typename Kernel, typename Epi>
inline void launch_conv(Kernel kernel, hipStream_t st, const PlanarTen &in, int H_in, int W_in, int cin, int ncout_tiles, const float *dw,
                        const float *db, float *out, long long out_plane, int out_pitch, int ya, int xa, int rows, int cols, const Epi &ep)
{
    hipLaunchKernelGGL(kernel, dim3((cols + 31) / 32, (rows + 7) / 8, ncout_tiles), dim3(256), 0, st, in.p, in.plane, in.pitch, in.ya, in.xa,
                       in.rows, in.cols, H_in, W_in, cin, dw, db, out, out_plane, out_pitch, ya, xa, rows, cols, ep);
}

// What every *_geometry checks first; what = "tile" or "tile and tail", negative = one of them is below 0.
inline int check_sr_geometry(const char *who, int h, int w, int scale, bool negative, const char *what)
{
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_SHAPE, "%s: %dx%d image", who, w, h);
    if (negative) return sr_set_error(SR_ERR_INVALID_ARG, "%s: %s must be >= 1, or 0 for the library's choice", who, what);
    if ((long long)h * scale > INT_MAX || (long long)w * scale * 3 > INT_MAX)
        return sr_set_error(SR_ERR_SHAPE, "%s: a %dx%d output (x%d) overflows int", who, w, h, scale);
    return SR_OK;
}

// What every model holds.
struct SrModelBase {
    sr_ctx *ctx = nullptr;
    std::vector<DevBuf> d_w, d_b;             // per convolution
    DevBuf ens_ws;                            // workspace of the geometric self-ensemble (sr_ensemble.hip), grown on demand
    const float *w(int i) const { return d_w[i].as<const float>(); }
    const float *b(int i) const { return d_b[i].as<const float>(); }
    // Every model adds a release_device() of its own that ends with this one (destroy_model calls it).
    void release_base()
    {
        for (auto &p : d_w) p.release();
        for (auto &p : d_b) p.release();
        ens_ws.release();
    }
};

// The geometric self-ensemble over one family's forward (sr_ensemble.hip; the definition is in include/sr_hip.h).
// fwd(d_src, src_stride, h, w, d_dst, dst_stride) is the family's fp32 forward with its own tile arguments bound; m is live.
using EnsForward = std::function<int(const uint8_t *, int64_t, int, int, float *, int64_t)>;
int ens_run(const char *who, SrModelBase &m, int scale, const EnsForward &fwd, const uint8_t *d_src, int64_t src_stride, int h, int w,
            void *d_dst, int64_t dst_stride, int mask, bool u8);

// The caller's tables of a *_create: n entries each, given as n_given; the first n_s entries of the optional third table too.
inline int check_weight_tables(const char *who, const char *what, int n, int n_given, const float *const *h_w, const float *const *h_b,
                               const float *const *h_s = nullptr, int n_s = 0)
{
    if (!h_w || !h_b || (n_s && !h_s)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null weight table", who);
    if (n_given != n) return sr_set_error(SR_ERR_INVALID_ARG, "%s: this description has %d convolutions, %d given", who, n, n_given);
    for (int k = 0; k < n; ++k)
        if (!h_w[k] || !h_b[k] || (k < n_s && !h_s[k])) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null array of %s %d", who, what, k);
    return SR_OK;
}

// Appends one convolution's arranged weights and bias to the model; on failure the error is set and the caller destroys m.
inline int upload_conv(const char *who, SrModelBase &m, const MfmaWeights &a)
{
    SRCHK(upload_floats(m.ctx, who, a.w.data(), a.w.size(), m.d_w));
    SRCHK(upload_floats(m.ctx, who, a.b.data(), a.b.size(), m.d_b));
    return SR_OK;
}

// The body of every *_destroy: m->release_device() with the stream drained and the context's device current.  A model that
// outlives its context only goes: the context's device memory is no longer this library's to free.
template <typename Model>
inline int destroy_model(Model *m, LiveSet &live)
{
    if (!m) return SR_OK;
    if (!live.erase(m)) return SR_OK;
    if (ctx_is_live(m->ctx)) {
        Guard g(m->ctx);
        (void)hipStreamSynchronize(m->ctx->stream);
        m->release_device();
    }
    delete m;
    return SR_OK;
}
