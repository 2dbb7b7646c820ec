// sr_conv_mfma.h -- the fp32 implicit-GEMM convolution shared by sr_lpips.hip, sr_srnet.hip, sr_resnet.hip, sr_rrdb.hip, sr_rcan.hip and sr_swinir.hip: one device
// mainloop, one 3 -> F head accumulate, and the host helpers around them (weight layouts, upload, the live-model set, the
// activation buffers, the forward calls' argument checks).  Internal: nothing here is part of the C ABI.
#pragma once
#include <cstdint>
#include <set>
#include <vector>

#include "sr_ctx.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));

// Where a thread of the 256-thread convolution block sits.
struct MfmaLane {
    int wave, l32, half;           // wave 0 .. 3 of the block, lane & 31 (pixel / cout column), lane >> 5 (k-half)
    int ox0, oy0, ct;              // block origin inside the output range, cout tile
};

__device__ __forceinline__ MfmaLane mfma_lane()
{
    const int tid = threadIdx.x, lane = tid & 63;
    return {tid >> 6, lane & 31, lane >> 5, (int)blockIdx.x * 32, (int)blockIdx.y * 8, (int)blockIdx.z};
}

// The cout (inside its tile) that register r of 32-cout half c2 holds on a lane of k-half `half`.
__host__ __device__ constexpr int mfma_cout(int c2, int r, int half) { return c2 * 32 + (r & 3) + 8 * (r >> 2) + 4 * half; }

// ---------------------------------------------------------------------------------------------------------------
// Implicit-GEMM convolution + bias on v_mfma_f32_32x32x2_f32, stride 1, KS x KS, zero padding P = KS / 2.
//   GEMM view: D[cout][pixel] = sum_k W[cout][k] * X[k][pixel], k = (cin, tap).
//   A operand = weights (lane l: cout l & 31, k-half l >> 5), B operand = input pixels (lane l: pixel l & 31, k-half
//   l >> 5); the accumulator then holds pixel l & 31 on the lane and 16 couts in its registers (mfma_cout), so every
//   store instruction of a planar epilogue writes two contiguous 128-byte row segments of two output planes.
//   Block = 4 waves = 8 output rows x 32 columns x NC = 32 NC2 couts; wave w owns rows 2w, 2w + 1 and all NC2 32-cout
//   halves (2 NC2 32 x 32 accumulators; four of them, 64 VGPRs, at NC2 = 2).  Cin is walked in chunks of CC channels: the
//   input patch [CC][8 + KS - 1][32 + KS - 1] and the weight slab [CC][KS*KS][NC] are staged in LDS, the k-half of a lane
//   selects the channel parity, so the per-step LDS addresses are lane base + compile-time immediates.
//   Per k-step a wave issues 2 + NC2 LDS dword reads for 2 NC2 MFMAs (256 matrix-pipe cycles at NC2 = 2): the kernel is
//   matrix-pipe bound by a wide margin; global loads of the next chunk are in flight during the MFMAs of the current one.
// The input is a planar buffer covering rows [in_ya, ..) x cols [in_xa, ..) of the layer's global index space; taps
// outside the image extent (H_in, W_in) read as zero -- that is the layer's own zero padding, also in the interior
// of a tiled forward where the buffer holds real neighbour data instead.  GUARD: the buffer holds in_rows x in_cols only,
// and staged-patch elements beyond it (read by masked outputs alone) are zero instead of loads past the buffer.
// Weights: wslab is [cout tile][chunk][c in chunk][tap][NC] (arrange_mfma_weights), bias is padded to whole tiles.
// Summation order (the determinism contract every bit-exact test rests on): one output value is its bias, then for
// channel pairs (2p, 2p + 1) ascending, for taps ascending, one two-term MFMA step (even channel, then odd channel).
// MFMA issue order: pair cp ascending, tap t ascending, c2 ascending, row 0 then row 1.  The order does not depend on
// where the output lies in a block or a sub-tile.
// The result is left in acc[c2][row of the wave's pair]; the caller's epilogue masks (col < cols, row < rows) and stores.
// ---------------------------------------------------------------------------------------------------------------
template <int KS, int CC, int NC2, bool GUARD>
__device__ __forceinline__ void conv_mfma_mainloop(const MfmaLane &ln, const float *__restrict__ in, long long in_plane, int in_pitch,
                                                   int in_ya, int in_xa, int in_rows, int in_cols, int H_in, int W_in, int cin,
                                                   const float *__restrict__ wslab, const float *__restrict__ bias, int out_ya,
                                                   int out_xa, f32x16 (&acc)[NC2][2])
{
    constexpr int T = KS * KS, P = KS / 2, NC = NC2 * 32;
    constexpr int PH = 8 + KS - 1, PW = 32 + KS - 1;
    constexpr int NPATCH = CC * PH * PW, NW4 = CC * T * NC / 4;        // patch floats, weight float4s per chunk
    constexpr int PE = (NPATCH + 255) / 256, WE = (NW4 + 255) / 256;   // per-thread staging counts
    __shared__ __attribute__((aligned(16))) float s_patch[NPATCH];
    __shared__ __attribute__((aligned(16))) float s_w[CC * T * NC];
    const int tid = threadIdx.x;
    const int wave = ln.wave, l32 = ln.l32, half = ln.half, ox0 = ln.ox0, oy0 = ln.oy0, ct = ln.ct;
    const int nchunk = cin / CC;

    // staging map of this thread: patch element e -> (channel, row, col) is the same for every chunk
    int p_off[PE];
    unsigned p_ok = 0;
#pragma unroll
    for (int i = 0; i < PE; ++i) {
        const int e = tid + i * 256;
        const int c = e / (PH * PW), r = (e / PW) % PH, x = e % PW;
        const int gy = out_ya + oy0 - P + r, gx = out_xa + ox0 - P + x;   // global index in the input layer
        // inside the image (else: zero padding) and inside what the input buffer holds (beyond it only masked outputs read)
        bool ok = e < NPATCH && gy >= 0 && gy < H_in && gx >= 0 && gx < W_in;
        if constexpr (GUARD) ok = ok && gy >= in_ya && gy - in_ya < in_rows && gx >= in_xa && gx - in_xa < in_cols;
        p_off[i] = ok ? (int)((long long)c * in_plane + (long long)(gy - in_ya) * in_pitch + (gx - in_xa)) : 0;
        if (ok) p_ok |= 1u << i;
    }
    const f4v *wsrc = (const f4v *)(wslab + (size_t)ct * nchunk * (CC * T * NC));

#pragma unroll
    for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float b = bias[ct * NC + mfma_cout(c2, r, half)];
            acc[c2][0][r] = b;
            acc[c2][1][r] = b;
        }

    float pv[PE];
    f4v wv[WE];
    auto load_chunk = [&](int ch) {
        const float *ib = in + (size_t)ch * CC * in_plane;
#pragma unroll
        for (int i = 0; i < PE; ++i) pv[i] = (p_ok >> i) & 1u ? ib[p_off[i]] : 0.0f;
        const f4v *wb = wsrc + (size_t)ch * NW4;
#pragma unroll
        for (int i = 0; i < WE; ++i) {
            const int e = tid + i * 256;
            wv[i] = e < NW4 ? wb[e] : f4v{0.f, 0.f, 0.f, 0.f};
        }
    };
    load_chunk(0);
    // lane bases: the k-half selects the odd channel of a pair
    const float *a_base = s_w + half * (T * NC) + l32;
    const float *b_base = s_patch + half * (PH * PW) + (2 * wave) * PW + l32;
#pragma unroll 1
    for (int ch = 0; ch < nchunk; ++ch) {
        __syncthreads();                                   // the previous chunk has been consumed
#pragma unroll
        for (int i = 0; i < PE; ++i) {
            const int e = tid + i * 256;
            if (e < NPATCH) s_patch[e] = pv[i];
        }
#pragma unroll
        for (int i = 0; i < WE; ++i) {
            const int e = tid + i * 256;
            if (e < NW4) ((f4v *)s_w)[e] = wv[i];
        }
        __syncthreads();
        if (ch + 1 < nchunk) load_chunk(ch + 1);           // in flight under the MFMAs below
#pragma unroll
        for (int cp = 0; cp < CC / 2; ++cp)
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int dy = t / KS, dx = t % KS;
                const float b0 = b_base[2 * cp * PH * PW + dy * PW + dx], b1 = b_base[2 * cp * PH * PW + (dy + 1) * PW + dx];
#pragma unroll
                for (int c2 = 0; c2 < NC2; ++c2) {
                    const float a = a_base[(2 * cp * T + t) * NC + c2 * 32];
                    acc[c2][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[c2][0], 0, 0, 0);
                    acc[c2][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[c2][1], 0, 0, 0);
                }
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Head (3 -> F) from the u8 image, one thread = output pixel (oy, ox) x the 64 couts of tile ct: acc = bias, then channels
// ascending, then the 9 taps ascending, as fmaf.  The input value of channel c is lut[c * LUT_CS + u8] inside the image
// (LUT_CS = 0: one table for the three channels), 0 outside (the layer's zero padding).  Weights are
// [cout tile][c][tap][64] (arrange_head_weights): the 64 multipliers of one input value are wave-uniform.
// ---------------------------------------------------------------------------------------------------------------
template <int LUT_CS>
__device__ __forceinline__ void head_accumulate(const unsigned char *__restrict__ img, long long stride, int H, int W,
                                                const float *__restrict__ wt, const float *__restrict__ bias, int ct, const float *lut,
                                                int oy, int ox, float (&acc)[64])
{
    wt += (size_t)ct * 27 * 64;
    bias += ct * 64;
#pragma unroll
    for (int co = 0; co < 64; ++co) acc[co] = bias[co];
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
#pragma unroll 1
        for (int ky = 0; ky < 3; ++ky) {
            const int gy = oy - 1 + ky;
            const bool yok = gy >= 0 && gy < H;
            const unsigned char *row = img + (size_t)(yok ? gy : 0) * stride;
#pragma unroll 1
            for (int kx = 0; kx < 3; ++kx) {
                const int gx = ox - 1 + kx;
                float v = 0.0f;
                if (yok && gx >= 0 && gx < W) v = lut[c * LUT_CS + row[(size_t)gx * 3 + c]];
                const float *wp = wt + ((size_t)c * 9 + ky * 3 + kx) * 64;
#pragma unroll
                for (int co = 0; co < 64; ++co) acc[co] = fmaf(wp[co], v, acc[co]);
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------

// Head weights [cout][3][9] -> [cout tile][c][tap][64]; F is a multiple of 64.
inline std::vector<float> arrange_head_weights(const float *w, int F)
{
    std::vector<float> a((size_t)F * 27);
    for (int co = 0; co < F; ++co)
        for (int c = 0; c < 3; ++c)
            for (int t = 0; t < 9; ++t) a[(((size_t)(co / 64) * 3 + c) * 9 + t) * 64 + co % 64] = w[((size_t)co * 3 + c) * 9 + t];
    return a;
}

struct MfmaWeights {
    std::vector<float> w, b;       // [cout tile][chunk][c in chunk][tap][NC] and the bias, couts zero-padded to whole tiles
};

// Convolution weights [cout][cin][T] -> the layout of conv_mfma_mainloop; cin is a multiple of CC.
inline MfmaWeights arrange_mfma_weights(const float *w, const float *b, int cout, int cin, int T, int CC, int NC)
{
    const int nct = (cout + NC - 1) / NC, nch = cin / CC;
    MfmaWeights m;
    m.w.assign((size_t)nct * NC * cin * T, 0.0f);
    m.b.assign((size_t)nct * NC, 0.0f);
    for (int co = 0; co < cout; ++co) {
        m.b[co] = b[co];
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < T; ++t)
                m.w[((((size_t)(co / NC) * nch + ci / CC) * CC + ci % CC) * T + t) * NC + co % NC] = w[((size_t)co * cin + ci) * T + t];
    }
    return m;
}

// Device copy of n floats, appended to dst (so a failed create releases it with the rest); on failure the error is set.
inline int upload_floats(sr_ctx *ctx, const char *who, const float *src, size_t n, std::vector<DevBuf> &dst)
{
    dst.emplace_back();
    SRCHK(dst.back().reserve(ctx, who, n * sizeof(float)));
    HIPCHK(hipMemcpy(dst.back().d, src, n * sizeof(float), hipMemcpyHostToDevice));
    return SR_OK;
}

// The models of one kind that exist: a handle is checked against it before it is dereferenced.
class LiveSet {
    std::mutex mu_;
    std::set<const void *> live_;

public:
    void insert(const void *p)
    {
        std::lock_guard<std::mutex> lk(mu_);
        live_.insert(p);
    }
    bool erase(const void *p)
    {
        std::lock_guard<std::mutex> lk(mu_);
        return live_.erase(p) != 0;
    }
    bool contains(const void *p)
    {
        std::lock_guard<std::mutex> lk(mu_);
        return p && live_.count(p) != 0;
    }
};

// Grow a model's n activation buffers to need_floats each (never shrinks): sync, free all, allocate all.  The n grow together
// and the last is allocated last, so its capacity tells whether all of them are large enough.
inline int ensure_activation_buffers(sr_ctx *ctx, DevBuf *bufs, int n, size_t need_floats, const char *who)
{
    if (need_floats * sizeof(float) <= bufs[n - 1].cap) return SR_OK;
    HIPCHK(stream_sync(ctx));
    for (int i = 0; i < n; ++i) bufs[i].release();
    for (int i = 0; i < n; ++i) SRCHK(bufs[i].reserve(ctx, who, need_floats * sizeof(float)));
    return SR_OK;
}

// What sr_srnet_*, sr_resnet_* and sr_rrdb_* forwards check of their image arguments: HWC u8 source of w pixels per row, HWC
// destination (u8 or fp32) of w * scale.
inline int check_sr_forward_args(const char *who, const void *d_src, int64_t src_stride, int w, const void *d_dst, int64_t dst_stride,
                                 int scale, bool u8)
{
    if (!d_src || !d_dst) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    if (src_stride < (int64_t)w * 3) return sr_set_error(SR_ERR_SHAPE, "%s: source stride smaller than a row", who);
    if (dst_stride < (int64_t)w * scale * 3 * (u8 ? 1 : 4)) return sr_set_error(SR_ERR_SHAPE, "%s: destination stride smaller than a row", who);
    if (!u8 && (dst_stride % 4 || (uintptr_t)d_dst % 4))
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: fp32 destination pointer and stride must be multiples of 4 bytes", who);
    return SR_OK;
}
