// sr_srnet.hip -- local super-resolution backend: the compact "VGG-style" SR network (the family Real-ESRGAN ships as
// SRVGGNetCompact) on gfx950.  Stage 2 of the reference is a remote API client; this is the pipeline's own learned upscaler.
//
//   layer 0        3 x 3 convolution 3 -> F straight from the u8 image (x = u8 / 255), per-channel slope activation
//   layers 1 .. D  3 x 3 convolutions F -> F, per-channel slope activation          (y >= 0 ? y : a[c] * y)
//   layer D + 1    3 x 3 convolution F -> 3 s^2, no activation, fused with PixelShuffle(s), the nearest-upsampled input
//                  (one fp32 add) and the store: HWC fp32 unclamped, or HWC u8 rintf(clamp(o, 0, 1) * 255)
//
// Everything is fp32 (fp32 in, fp32 accumulate): the F -> F and F -> 3 s^2 layers are implicit GEMMs on
// v_mfma_f32_32x32x2_f32 with the tiling of sr_lpips.hip's k_lp_conv_mfma (a sibling kernel: the LPIPS instruction stream is
// left alone), the 3 -> F head is a direct VALU kernel.  The 3 s^2-channel tensor is never written.
//
// Memory: activations are planar fp32 [F][rows][pitch] in two ping-pong buffers owned by the model.  The image is walked in
// square sub-tiles of the INPUT; a sub-tile recomputes a halo of D + 2 input pixels (layer k's valid extent is the sub-tile
// grown by D + 1 - k, clipped to the image), and zero padding is applied per layer at the true image border only, so every
// value equals the unstreamed forward's.
//
// Determinism: one output value is bias, then for channel pairs (2p, 2p + 1) ascending, for taps ascending, one
// two-term MFMA step (even channel, then odd channel); the head is bias, then channels ascending, then taps, as fmaf.  The
// order does not depend on where the output lies in a block or a sub-tile: streamed and unstreamed results are bit-equal.
//
// Weights are caller-supplied (sr_srnet_create); nothing is fetched.
#include <algorithm>
#include <climits>
#include <cstring>
#include <set>
#include <vector>

#include "sr_ctx.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int SN_DEFAULT_TILE = 2048;      // tile = 0: one pipeline tile is one sub-tile (no halo recompute)

// ---------------------------------------------------------------------------------------------------------------
// Head (3 -> F) from the u8 image: one thread = one output pixel x 64 output channels (blockIdx.z: 64-cout tile).
// x = u8 / 255 inside the image, 0 outside (the layer's zero padding); the 256 values are tabulated in LDS with exactly
// that fp32 division.  Weights are [cout tile][c][tap][64]: the 64 multipliers of one input value are wave-uniform.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sn_head(const unsigned char *__restrict__ img, long long stride, int H, int W,
                                                 const float *__restrict__ wt, const float *__restrict__ bias,
                                                 const float *__restrict__ slope, float *__restrict__ out, int ya, int xa,
                                                 int rows, int cols, int pitch, long long plane)
{
    __shared__ float lut[256];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    lut[tid] = (float)tid / 255.0f;
    __syncthreads();
    const int lx = blockIdx.x * 64 + threadIdx.x, ly = blockIdx.y * 4 + threadIdx.y, ct = blockIdx.z;
    if (lx >= cols || ly >= rows) return;
    const int oy = ya + ly, ox = xa + lx;
    wt += (size_t)ct * 27 * 64;
    bias += ct * 64;
    slope += ct * 64;
    float acc[64];
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
                if (yok && gx >= 0 && gx < W) v = lut[row[(size_t)gx * 3 + c]];
                const float *wp = wt + ((size_t)c * 9 + ky * 3 + kx) * 64;
#pragma unroll
                for (int co = 0; co < 64; ++co) acc[co] = fmaf(wp[co], v, acc[co]);
            }
        }
    }
    float *o = out + (size_t)ct * 64 * plane + (size_t)ly * pitch + lx;
#pragma unroll
    for (int co = 0; co < 64; ++co) {
        const float y = acc[co];
        o[(size_t)co * plane] = y >= 0.0f ? y : slope[co] * y;
    }
}

// What the fused tail needs beside the convolution's own arguments.
struct SnTail {
    const unsigned char *img;      // u8 source (the nearest-upsampled base)
    long long img_stride;
    void *dst;                     // HWC output, u8 or fp32
    long long dst_stride;          // bytes
};

// ---------------------------------------------------------------------------------------------------------------
// 3 x 3 implicit-GEMM convolution on v_mfma_f32_32x32x2_f32, stride 1, zero padding 1 at the image border.
//   GEMM view, operand layout, block shape (4 waves = 8 output rows x 32 columns, wave w owns rows 2w, 2w + 1) and LDS
//   staging are those of k_lp_conv_mfma<3, 8> (sr_lpips.hip); NC2 = 32-cout halves per block.
//   S == 0: body layer, NC2 = 2, epilogue = per-channel slope, planar store.
//   S >= 1: tail layer, couts 3 S^2 zero-padded to 32 NC2; epilogue = pixel shuffle + base add + HWC store (U8: clamp,
//           scale, round half even).  out_ya / out_xa are then the sub-tile's own origin in the image.
// ---------------------------------------------------------------------------------------------------------------
template <int NC2, int S, bool U8>
__global__ __launch_bounds__(256) void k_sn_conv(const float *__restrict__ in, long long in_plane, int in_pitch, int in_ya,
                                                 int in_xa, int in_rows, int in_cols, int H_in, int W_in, int cin, const float *__restrict__ wslab,
                                                 const float *__restrict__ bias, const float *__restrict__ slope,
                                                 float *__restrict__ out, long long out_plane, int out_pitch, int out_ya,
                                                 int out_xa, int rows, int cols, SnTail tail)
{
    constexpr int CC = 8, T = 9, NC = NC2 * 32;
    constexpr int PH = 8 + 2, PW = 32 + 2;
    constexpr int NPATCH = CC * PH * PW, NW4 = CC * T * NC / 4;        // patch floats, weight float4s per chunk
    constexpr int PE = (NPATCH + 255) / 256, WE = (NW4 + 255) / 256;   // per-thread staging counts
    __shared__ __attribute__((aligned(16))) float s_patch[NPATCH];
    __shared__ __attribute__((aligned(16))) float s_w[CC * T * NC];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, l32 = lane & 31, half = lane >> 5;
    const int ox0 = blockIdx.x * 32, oy0 = blockIdx.y * 8;              // block origin inside the output range
    const int ct = blockIdx.z;                                          // cout tile of NC
    const int nchunk = cin / CC;

    // staging map of this thread: patch element e -> (channel, row, col) is the same for every chunk
    int p_off[PE];
    unsigned p_ok = 0;
#pragma unroll
    for (int i = 0; i < PE; ++i) {
        const int e = tid + i * 256;
        const int c = e / (PH * PW), r = (e / PW) % PH, x = e % PW;
        const int gy = out_ya + oy0 - 1 + r, gx = out_xa + ox0 - 1 + x;   // global index in the input layer
        // inside the image (else: zero padding) and inside what the input buffer holds (beyond it only masked outputs read)
        const bool ok = e < NPATCH && gy >= 0 && gy < H_in && gx >= 0 && gx < W_in && gy >= in_ya && gy - in_ya < in_rows &&
                        gx >= in_xa && gx - in_xa < in_cols;
        p_off[i] = ok ? (int)((long long)c * in_plane + (long long)(gy - in_ya) * in_pitch + (gx - in_xa)) : 0;
        if (ok) p_ok |= 1u << i;
    }
    const f4v *wsrc = (const f4v *)(wslab + (size_t)ct * nchunk * (CC * T * NC));

    f32x16 acc[NC2][2];
#pragma unroll
    for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float b = bias[ct * NC + c2 * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
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
                const int dy = t / 3, dx = t % 3;
                const float b0 = b_base[2 * cp * PH * PW + dy * PW + dx], b1 = b_base[2 * cp * PH * PW + (dy + 1) * PW + dx];
#pragma unroll
                for (int c2 = 0; c2 < NC2; ++c2) {
                    const float a = a_base[(2 * cp * T + t) * NC + c2 * 32];
                    acc[c2][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[c2][0], 0, 0, 0);
                    acc[c2][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[c2][1], 0, 0, 0);
                }
            }
    }
    const int col = ox0 + l32;
    if (col >= cols) return;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        const int row = oy0 + 2 * wave + pr;
        if (row >= rows) continue;
        if constexpr (S == 0) {                            // slope activation, planar store
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * NC + c2 * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const float y = acc[c2][pr][r];
                    out[(size_t)co * out_plane + (size_t)row * out_pitch + col] = y >= 0.0f ? y : slope[co] * y;
                }
        } else {                                           // pixel shuffle + nearest base + HWC store
            const int gy = out_ya + row, gx = out_xa + col;
            const unsigned char *px = tail.img + (size_t)gy * tail.img_stride + (size_t)gx * 3;
            const float x0 = (float)px[0] / 255.0f, x1 = (float)px[1] / 255.0f, x2 = (float)px[2] / 255.0f;
            char *drow = (char *)tail.dst + (size_t)gy * S * tail.dst_stride;
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = c2 * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (co >= 3 * S * S) continue;
                    const int c = co / (S * S), rem = co % (S * S), dy = rem / S, dx = rem % S;
                    const float o = acc[c2][pr][r] + (c == 0 ? x0 : (c == 1 ? x1 : x2));
                    const size_t e = ((size_t)gx * S + dx) * 3 + c;
                    char *d = drow + (size_t)dy * tail.dst_stride;
                    if constexpr (U8) ((unsigned char *)d)[e] = (unsigned char)rintf(fminf(fmaxf(o, 0.0f), 1.0f) * 255.0f);
                    else ((float *)d)[e] = o;
                }
        }
    }
}

struct SnGeom {
    int tile = 0, tiles_x = 0, tiles_y = 0, halo = 0;
    int rows = 0, pitch = 0;          // activation buffer of the padded sub-tile
    long long plane = 0;
};

int sn_check_arch(const char *who, int n_feat, int n_body, int scale)
{
    if ((n_feat != 64 && n_feat != 128 && n_feat != 192 && n_feat != 256) || n_body < 0 || n_body > 64 || scale < 1 || scale > 4)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d features, %d body convolutions, scale %d is outside F in {64, 128, 192, 256}, "
                            "0 <= D <= 64, 1 <= s <= 4", who, n_feat, n_body, scale);
    return SR_OK;
}

// Host only: sub-tile grid and buffer geometry of an h x w input.
int sn_geometry(const char *who, int h, int w, int n_body, int scale, int tile, SnGeom &g)
{
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_SHAPE, "%s: %dx%d image", who, w, h);
    if (tile < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: tile must be >= 1, or 0 for the library's choice", who);
    if ((long long)h * scale > INT_MAX || (long long)w * scale * 3 > INT_MAX)
        return sr_set_error(SR_ERR_SHAPE, "%s: a %dx%d output (x%d) overflows int", who, w, h, scale);
    g.tile = tile == 0 ? SN_DEFAULT_TILE : tile;
    g.halo = n_body + 2;
    g.tiles_x = (w + g.tile - 1) / g.tile;
    g.tiles_y = (h + g.tile - 1) / g.tile;
    g.rows = (int)std::min<long long>((long long)std::min(g.tile, h) + 2 * g.halo, h);
    const int cols = (int)std::min<long long>((long long)std::min(g.tile, w) + 2 * g.halo, w);
    g.pitch = (cols + 3) / 4 * 4;
    g.plane = (long long)g.rows * g.pitch;
    if (g.plane * 8 > INT_MAX)        // the convolution indexes one 8-channel chunk of a buffer with 32-bit offsets
        return sr_set_error(SR_ERR_SHAPE, "%s: a sub-tile of %d x %d activations is too large; use a smaller tile", who, g.pitch, g.rows);
    return SR_OK;
}

}  // namespace

struct sr_srnet_model {
    sr_ctx *ctx = nullptr;
    int F = 0, D = 0, S = 0;
    std::vector<float *> d_w, d_b, d_slope;   // per layer 0 .. D + 1 (no slope for the tail)
    float *buf[2] = {nullptr, nullptr};       // ping-pong activation buffers
    size_t buf_floats = 0;
};

static std::mutex g_sn_mu;
static std::set<const void *> g_sn_live;

static bool sn_is_live(const sr_srnet_model *m)
{
    std::lock_guard<std::mutex> lk(g_sn_mu);
    return m && g_sn_live.count(m) != 0;
}

template <int S, bool U8>
static void sn_launch_tail(dim3 grid, hipStream_t st, const float *src, long long plane, int pitch, int in_ya, int in_xa, int in_rows,
                           int in_cols, int h, int w, int F, const float *dw, const float *db, int ya, int xa, int rows, int cols, SnTail tail)
{
    constexpr int NC2 = 3 * S * S > 32 ? 2 : 1;
    hipLaunchKernelGGL((k_sn_conv<NC2, S, U8>), grid, dim3(256), 0, st, src, plane, pitch, in_ya, in_xa, in_rows, in_cols, h, w, F, dw, db,
                       (const float *)nullptr, (float *)nullptr, 0LL, 0, ya, xa, rows, cols, tail);
}

static int sn_forward(sr_srnet_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride,
                      int tile, bool u8, const char *who)
{
    if (!sn_is_live(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    sr_ctx *ctx = m->ctx;
    CTX_ENTER(ctx);
    if (!d_src || !d_dst) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    SnGeom g;
    int rc = sn_geometry(who, h, w, m->D, m->S, tile, g);
    if (rc) return rc;
    const int F = m->F, D = m->D, S = m->S;
    const int64_t esz = u8 ? 1 : 4;
    if (src_stride < (int64_t)w * 3) return sr_set_error(SR_ERR_SHAPE, "%s: source stride smaller than a row", who);
    if (dst_stride < (int64_t)w * S * 3 * esz) return sr_set_error(SR_ERR_SHAPE, "%s: destination stride smaller than a row", who);
    if (!u8 && (dst_stride % 4 || (uintptr_t)d_dst % 4))
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: fp32 destination pointer and stride must be multiples of 4 bytes", who);
    const size_t need_floats = (size_t)g.plane * F;
    if (need_floats > m->buf_floats) {
        HIPCHK(stream_sync(ctx));
        for (auto &p : m->buf) {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
        m->buf_floats = 0;
        for (auto &p : m->buf) {
            hipError_t e = hipMalloc((void **)&p, need_floats * sizeof(float));
            if (e != hipSuccess)
                return sr_set_error(e == hipErrorOutOfMemory ? SR_ERR_OOM : SR_ERR_HIP,
                                    "%s: activation buffers (2 x %zu MB; use a smaller tile): %s", who, need_floats * 4 >> 20,
                                    hipGetErrorString(e));
        }
        m->buf_floats = need_floats;
    }
    const SnTail tail = {d_src, (long long)src_stride, d_dst, (long long)dst_stride};
    for (int ty = 0; ty < g.tiles_y; ++ty)
        for (int tx = 0; tx < g.tiles_x; ++tx) {
            const int y0 = ty * g.tile, y1 = std::min(y0 + g.tile, h), x0 = tx * g.tile, x1 = std::min(x0 + g.tile, w);
            // extent of layer k's output: the sub-tile grown by D + 1 - k, clipped to the image
            auto ext = [&](int k, int &ya, int &xa, int &rows, int &cols) {
                const int gr = D + 1 - k;
                ya = std::max(y0 - gr, 0);
                xa = std::max(x0 - gr, 0);
                rows = std::min(y1 + gr, h) - ya;
                cols = std::min(x1 + gr, w) - xa;
            };
            int ya, xa, rows, cols;
            ext(0, ya, xa, rows, cols);
            const int pitch = (cols + 3) / 4 * 4;
            const long long plane = (long long)rows * pitch;      // <= g.plane: one geometry for every layer of the sub-tile
            int cur = 0;
            {
                ProfScope ps(ctx, "srnet_head");
                hipLaunchKernelGGL(k_sn_head, dim3((cols + 63) / 64, (rows + 3) / 4, F / 64), dim3(64, 4), 0, ctx->stream, d_src,
                                   (long long)src_stride, h, w, m->d_w[0], m->d_b[0], m->d_slope[0], m->buf[0], ya, xa, rows,
                                   cols, pitch, plane);
            }
            int in_ya = ya, in_xa = xa, in_rows = rows, in_cols = cols;
            for (int k = 1; k <= D; ++k) {
                ext(k, ya, xa, rows, cols);
                ProfScope ps(ctx, "srnet_body");
                hipLaunchKernelGGL((k_sn_conv<2, 0, false>), dim3((cols + 31) / 32, (rows + 7) / 8, F / 64), dim3(256), 0, ctx->stream,
                                   m->buf[cur], plane, pitch, in_ya, in_xa, in_rows, in_cols, h, w, F, m->d_w[k], m->d_b[k], m->d_slope[k],
                                   m->buf[cur ^ 1], plane, pitch, ya, xa, rows, cols, SnTail{nullptr, 0, nullptr, 0});
                cur ^= 1;
                in_ya = ya; in_xa = xa; in_rows = rows; in_cols = cols;
            }
            ext(D + 1, ya, xa, rows, cols);
            {
                ProfScope ps(ctx, "srnet_tail");
                const dim3 grid((cols + 31) / 32, (rows + 7) / 8, 1);
#define SN_TAIL(SC)                                                                                                            \
    if (u8) sn_launch_tail<SC, true>(grid, ctx->stream, m->buf[cur], plane, pitch, in_ya, in_xa, in_rows, in_cols, h, w, F, m->d_w[D + 1],       \
                                     m->d_b[D + 1], ya, xa, rows, cols, tail);                                                 \
    else sn_launch_tail<SC, false>(grid, ctx->stream, m->buf[cur], plane, pitch, in_ya, in_xa, in_rows, in_cols, h, w, F, m->d_w[D + 1],         \
                                   m->d_b[D + 1], ya, xa, rows, cols, tail)
                switch (S) {
                case 1: SN_TAIL(1); break;
                case 2: SN_TAIL(2); break;
                case 3: SN_TAIL(3); break;
                default: SN_TAIL(4); break;
                }
#undef SN_TAIL
            }
            rc = check_launch(who);
            if (rc) return rc;
        }
    return SR_OK;
}

extern "C" {

int sr_srnet_create(sr_ctx *ctx, int n_feat, int n_body, int scale, const float *const *h_w, const float *const *h_b,
                    const float *const *h_slope, sr_srnet_model **out)
{
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_srnet_create: null out");
    *out = nullptr;
    int rc = sn_check_arch("sr_srnet_create", n_feat, n_body, scale);       // host decision, before any device call
    if (rc) return rc;
    if (!h_w || !h_b || !h_slope) return sr_set_error(SR_ERR_INVALID_ARG, "sr_srnet_create: null weight table");
    const int F = n_feat, D = n_body, S = scale, nl = D + 2;
    for (int k = 0; k < nl; ++k)
        if (!h_w[k] || !h_b[k] || (k <= D && !h_slope[k])) return sr_set_error(SR_ERR_INVALID_ARG, "sr_srnet_create: null array of layer %d", k);
    CTX_ENTER(ctx);
    sr_srnet_model *M = new sr_srnet_model();
    M->ctx = ctx;
    M->F = F; M->D = D; M->S = S;
    {
        std::lock_guard<std::mutex> lk(g_sn_mu);
        g_sn_live.insert(M);
    }
    auto fail = [&](int code, const char *what) {
        sr_set_error(code, "sr_srnet_create: %s", what);
        sr_srnet_destroy(M);
        return code;
    };
    auto upload = [&](const std::vector<float> &v, std::vector<float *> &dst) {
        float *d = nullptr;
        if (hipMalloc((void **)&d, v.size() * sizeof(float)) != hipSuccess) return SR_ERR_OOM;
        dst.push_back(d);
        return hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess ? SR_OK : SR_ERR_HIP;
    };
    const int tail_c = 3 * S * S, tail_nc = tail_c > 32 ? 64 : 32;
    for (int k = 0; k < nl; ++k) {
        const float *w = h_w[k];
        std::vector<float> arranged, b;
        if (k == 0) {                                            // head: [cout tile][c][tap][64]
            arranged.resize((size_t)F * 27);
            for (int co = 0; co < F; ++co)
                for (int c = 0; c < 3; ++c)
                    for (int t = 0; t < 9; ++t)
                        arranged[(((size_t)(co / 64) * 3 + c) * 9 + t) * 64 + co % 64] = w[((size_t)co * 3 + c) * 9 + t];
            b.assign(h_b[k], h_b[k] + F);
        } else {                                                 // MFMA: [cout tile][chunk][c in chunk][tap][NC], zero-padded couts
            const int cout = k <= D ? F : tail_c, NC = k <= D ? 64 : tail_nc, nct = k <= D ? F / 64 : 1, nch = F / 8;
            arranged.assign((size_t)nct * NC * F * 9, 0.0f);
            b.assign((size_t)nct * NC, 0.0f);
            for (int co = 0; co < cout; ++co) {
                b[co] = h_b[k][co];
                for (int ci = 0; ci < F; ++ci)
                    for (int t = 0; t < 9; ++t)
                        arranged[(((((size_t)(co / NC) * nch + ci / 8) * 8 + ci % 8) * 9 + t) * NC) + co % NC] =
                            w[((size_t)co * F + ci) * 9 + t];
            }
        }
        if ((rc = upload(arranged, M->d_w)) != SR_OK) return fail(rc, "weight upload");
        if ((rc = upload(b, M->d_b)) != SR_OK) return fail(rc, "bias upload");
        if (k <= D && (rc = upload(std::vector<float>(h_slope[k], h_slope[k] + F), M->d_slope)) != SR_OK) return fail(rc, "slope upload");
    }
    *out = M;
    return SR_OK;
}

int sr_srnet_destroy(sr_srnet_model *m)
{
    if (!m) return SR_OK;
    {
        std::lock_guard<std::mutex> lk(g_sn_mu);
        if (!g_sn_live.erase(m)) return SR_OK;
    }
    if (ctx_is_live(m->ctx)) {
        Guard g(m->ctx);
        (void)hipStreamSynchronize(m->ctx->stream);
        for (auto p : m->d_w) if (p) (void)hipFree(p);
        for (auto p : m->d_b) if (p) (void)hipFree(p);
        for (auto p : m->d_slope) if (p) (void)hipFree(p);
        for (auto p : m->buf) if (p) (void)hipFree(p);
    }
    delete m;
    return SR_OK;
}

int sr_srnet_plan(int h, int w, int n_feat, int n_body, int scale, int tile, int *halo, int *n_tiles, size_t *workspace_bytes)
{
    int rc = sn_check_arch("sr_srnet_plan", n_feat, n_body, scale);
    if (rc) return rc;
    SnGeom g;
    rc = sn_geometry("sr_srnet_plan", h, w, n_body, scale, tile, g);
    if (rc) return rc;
    if (halo) *halo = g.halo;
    if (n_tiles) *n_tiles = g.tiles_x * g.tiles_y;
    if (workspace_bytes) *workspace_bytes = (size_t)2 * n_feat * (size_t)g.plane * sizeof(float);
    return SR_OK;
}

int sr_srnet_u8(sr_srnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride,
                int tile)
{
    return sn_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tile, true, "sr_srnet_u8");
}

int sr_srnet_f32(sr_srnet_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride,
                 int tile)
{
    return sn_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tile, false, "sr_srnet_f32");
}

}  // extern "C"
