// sr_hat.hip -- local super-resolution backend: HAT (Chen et al., "Activating More Pixels in Image Super-Resolution
// Transformer", CVPR 2023; resi_connection '1conv', no absolute position embedding, patch size 1, window 16, overlap ratio 0.5,
// upsampler pixelshuffle) at scales 2 .. 4 on gfx950.  The definition is in include/sr_hip.h ("HAT").
//
//   input       the u8 image extended by reflection WITHOUT the edge pixel (F.pad 'reflect') to Hp x Wp (multiples of 16)
//   head        3 x 3 convolution 3 -> C, x[c] = (u8 / 255 - mean[c]) * range                                   -> h
//   deep        r = LN(h);  per RHAG: x = r, D HABs on x, one OCAB, r = conv(x) + r;  then LN(r)
//     HAB       y = LN1(x);  a = proj(window attention 16 x 16 of y, shift 0 / 8);  u = conv(gelu(conv(y)));
//               s = sigmoid(W2 relu(W1 mean(u) + b1) + b2);  x = fmaf(conv_scale, u * s, x + a);  x = x + fc2(gelu(fc1(LN2(x))))
//     OCAB      y = LN1(x);  the 256 queries of a window attend to the 576 keys of its 24 x 24 neighbourhood (zero k and v
//               outside the image, not masked);  x = x + proj(.);  x = x + fc2(gelu(fc1(LN2(x))))
//   long skip   f = conv_after_body(LN(r)) + h
//   tail        SwinIR's pixelshuffle reconstruction, o[c] = y[c] / range + mean[c], cropped
//
// Everything is fp32 except the LayerNorm statistics and the CAB's channel attention (float64).  The head, the LayerNorm, the
// linear layers, the 3 x 3 convolutions and the weight arrangement are sr_swin_common.h (shared with sr_swinir.hip); the
// channel mean, the attention and the scale-and-skip pass are sr_chan_attn.h (shared with sr_rcan.hip); the reconstruction
// runs in tail x tail sub-pieces exactly as sr_swinir.hip's.  New here: the two attention kernels and the reflection.
//
// Trunk phase: the padded image is ONE piece in seven planar fp32 buffers of Hp x Wp planes: H (h, then f in place), R (the
// RHAG's input, then its output in place), X (the running x), A (LayerNorm output, then the attention output in place of it),
// U (the CAB's output) -- Cp planes each --, T (the CAB's middle tensor, n_mid rounded up to 64 planes) and Q (qkv, then the
// MLP's hidden tensor).  4 (5 Cp + Tp + Qp) bytes per pixel: 6400 at C = 180, n_mid 60, hidden 360.  In a HAB the CAB runs first
// (it reads LN1's output in A), then qkv, then the attention overwrites A.  Every kernel that writes a tensor writes all its
// planes (padded couts are 0, the attention kernels store explicit zeros), so nothing the workspace held before enters a value.
//
// The two attention kernels (k_hat_attention, k_hat_oca): one workgroup of 256 threads per (window, head), thread = query; a
// thread holds its q and its output accumulators in registers.  A window has 256 (576) keys, too many scores for registers, so
// the kernel makes THREE SWEEPS over the keys and recomputes the score in each -- by the same instruction sequence, so the three
// values of a score are the same bits: sweep 1 takes the maximum, sweep 2 the sum of e_j = expf(a_j - max), sweep 3 forms
// p_j = e_j / sum and adds p_j v_j.  In every sweep the keys pass through LDS in chunks of 128 (192) as [channel][key], channels
// zero-padded to DP -- K in every sweep, V in the third -- so that a workgroup holds 32 (48) KiB at DP = 32 and several share a
// CU; keys are read as broadcast float4 over four neighbours.  The roll, the partition and the region mask (the enlarged
// window's position and its zero keys) are index arithmetic.
//
// Summation orders (the contract): convolutions and linear layers as sr_conv_mfma.h; the attention's dot product starts at +0
// and is an fmaf chain over d ascending; the bias and then (window attention, shift 8) the mask are added to it (two adds); the
// maximum is exact; the sum of e_j runs over the keys ascending from +0; p_j = e_j / sum (the division comes BEFORE the p v sum);
// the p v sum is an fmaf chain over the keys ascending from +0.  The CAB's mean is sr_chan_attn.h's; the combine is one rounded
// product u * s and one fmaf(conv_scale, ., x + a).  No atomics.  Nothing depends on tail.  Equal inputs give equal bits.
//
// Weights are caller-supplied (sr_hat_create); nothing is fetched.
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_chan_attn.h"
#include "sr_hat.h"
#include "sr_net_common.h"
#include "sr_swin_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// Reflection of the u8 image to Hp x Wp without the edge pixel (dense, 3 Wp bytes per row): padded index i reads
// m = i mod (2 n - 2), m < n ? m : 2 n - 2 - m (F.pad mode 'reflect', continued periodically where the pad is longer than
// the side); n = 1 repeats the single pixel.  One thread per output byte.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ht_reflect(int i, int n)
{
    if (n == 1) return 0;
    const int m = i % (2 * n - 2);
    return m < n ? m : 2 * n - 2 - m;
}

__global__ __launch_bounds__(256) void k_hat_reflect(const unsigned char *__restrict__ img, long long stride, int h, int w,
                                                     unsigned char *__restrict__ out, int hp, int wp)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)hp * wp * 3) return;
    const int c = (int)(i % 3), x = (int)((i / 3) % wp), y = (int)(i / (3LL * wp));
    out[i] = img[(size_t)ht_reflect(y, h) * stride + (size_t)ht_reflect(x, w) * 3 + c];
}

// Region of coordinate v of the shifted image along an axis of length L (calculate_mask's three slices).
__device__ __forceinline__ int ht_region(int v, int L) { return v < L - HT_WIN ? 0 : (v < L - HT_SHIFT ? 1 : 2); }

// ---------------------------------------------------------------------------------------------------------------
// The three sweeps of one query over NK keys, which pass through LDS CH keys at a time.  q: the query's DP channels (zero
// beyond d);  Ks, Vs: LDS, [DP][CH], zero beyond d;  bp: the gathered bias of this query, key j at bp[j * HT_TOK];
// load(c, with_v): fills Ks (and Vs) with the keys [c CH, (c + 1) CH), barriers included;  masked(j): whether -100 is added to the
// score of key j.  o: the DP output accumulators.  Keys ascend across the chunks and inside them, so the orders are those of one
// pass over all NK keys.
// ---------------------------------------------------------------------------------------------------------------
template <int DP, int CH, typename Masked>
__device__ __forceinline__ void ht_score4(const float (&q)[DP], const float *Ks, const float *bp, int j0, int j4, Masked masked, float (&a)[4])
{
    a[0] = a[1] = a[2] = a[3] = 0.0f;
#pragma unroll
    for (int dd = 0; dd < DP; ++dd) {
        const f4v k4 = *(const f4v *)&Ks[dd * CH + 4 * j4];
        a[0] = fmaf(q[dd], k4.x, a[0]);
        a[1] = fmaf(q[dd], k4.y, a[1]);
        a[2] = fmaf(q[dd], k4.z, a[2]);
        a[3] = fmaf(q[dd], k4.w, a[3]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int j = j0 + 4 * j4 + u;
        a[u] = a[u] + bp[(size_t)j * HT_TOK];
        if (masked(j)) a[u] = a[u] + -100.0f;
    }
}

template <int DP, int NK, int CH, typename Load, typename Masked>
__device__ __forceinline__ void ht_sweeps(const float (&q)[DP], const float *Ks, const float *Vs, const float *bp, Load load, Masked masked,
                                          float (&o)[DP])
{
    static_assert(NK % CH == 0 && CH % 4 == 0, "whole chunks of whole float4");
    constexpr int NCH = NK / CH;
    float a[4];
    float mx = -INFINITY;
#pragma unroll 1
    for (int c = 0; c < NCH; ++c) {                        // sweep 1: the maximum
        load(c, false);
#pragma unroll 1
        for (int j4 = 0; j4 < CH / 4; ++j4) {
            ht_score4<DP, CH>(q, Ks, bp, c * CH, j4, masked, a);
            mx = fmaxf(fmaxf(mx, a[0]), fmaxf(a[1], fmaxf(a[2], a[3])));
        }
    }
    float sum = 0.0f;
#pragma unroll 1
    for (int c = 0; c < NCH; ++c) {                        // sweep 2: the sum of e_j, keys ascending
        load(c, false);
#pragma unroll 1
        for (int j4 = 0; j4 < CH / 4; ++j4) {
            ht_score4<DP, CH>(q, Ks, bp, c * CH, j4, masked, a);
#pragma unroll
            for (int u = 0; u < 4; ++u) sum += expf(a[u] - mx);
        }
    }
#pragma unroll
    for (int dd = 0; dd < DP; ++dd) o[dd] = 0.0f;
#pragma unroll 1
    for (int c = 0; c < NCH; ++c) {                        // sweep 3: p_j = e_j / sum, then the p v chains, keys ascending
        load(c, true);
#pragma unroll 1
        for (int j4 = 0; j4 < CH / 4; ++j4) {
            ht_score4<DP, CH>(q, Ks, bp, c * CH, j4, masked, a);
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = expf(a[u] - mx) / sum;
#pragma unroll
            for (int dd = 0; dd < DP; ++dd) {
                const f4v v4 = *(const f4v *)&Vs[dd * CH + 4 * j4];
                float acc = o[dd];
                acc = fmaf(a[0], v4.x, acc);
                acc = fmaf(a[1], v4.y, acc);
                acc = fmaf(a[2], v4.z, acc);
                acc = fmaf(a[3], v4.w, acc);
                o[dd] = acc;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// What tells the two attentions apart: the number of keys, how many of them lie in LDS at a time, and (in ht_attend) where key
// j lies and whether it is masked.
//   HtWindow    the 256 keys are the window's own tokens, in two chunks of 128 (eight rows): 32 KiB at DP = 32 and four workgroups
//               per CU, measured against one chunk of 256 (64 KiB, two workgroups: 1.34 x the time) and four of 64 (1.14 x)
//   HtOverlap   the 576 keys of the enlarged window, in three chunks of 192 (eight rows): 48 KiB at DP = 32 instead of 144
// ---------------------------------------------------------------------------------------------------------------
struct HtWindow {
    static constexpr int NK = HT_TOK, CH = HT_TOK / 2;
    static constexpr bool OCA = false;
};
struct HtOverlap {
    static constexpr int NK = HT_KEYS, CH = HT_KEYS / 3;
    static constexpr bool OCA = true;
};

// ---------------------------------------------------------------------------------------------------------------
// One head of one 16 x 16 window per workgroup (block 256, thread = query token; grid (windows, heads)); the orders are at the
// top of this file.  qkv planar: q of channel c in plane c (already scaled), k in plane C + c, v in plane 2 C + c.  bias: the
// table gathered to [head][key j][query i] (coalesced across the lanes).  DP: the head width d rounded up to a multiple of 8.
// Query token (wy, wx) of window (by, bx) is pixel ((16 by + wy + shift) mod Hp, (16 bx + wx + shift) mod Wp), read there and
// written back there (the OCA: shift 0).  The keys pass through LDS in chunks per sweep -- K in every sweep, V in the third.
//   window attention   key j is token j of the same window; with a shift, -100 where the regions of query and key differ
//   OCA                key (ky, kx), 0 <= ky, kx < 24, is pixel (16 by - 4 + ky, 16 bx - 4 + kx); a key outside the Hp x Wp image
//                      has k = v = 0 exactly and is NOT masked: its score is 0 + bias, it takes its share of the softmax and adds
//                      nothing to the output
// Writes channels [head d, (head + 1) d) of out; head 0 also writes +0 into the planes C .. Cp - 1.
// ---------------------------------------------------------------------------------------------------------------
template <int DP, typename A>
__device__ __forceinline__ void ht_attend(const float *__restrict__ qkv, long long plane, int pitch, int Hp, int Wp, int C, int d, int shift,
                                          const float *__restrict__ bias, float *__restrict__ out, long long oplane, int opitch, int Cp)
{
    constexpr int CH = A::CH;
    __shared__ __attribute__((aligned(16))) float Ks[DP * CH];
    __shared__ __attribute__((aligned(16))) float Vs[DP * CH];
    const int t = threadIdx.x, head = blockIdx.y, nwx = Wp / HT_WIN;
    const int by = blockIdx.x / nwx, bx = blockIdx.x % nwx;
    const int sy = by * HT_WIN + (t >> 4), sx = bx * HT_WIN + (t & 15);        // in the shifted image
    int py = sy + shift, px = sx + shift;                                      // in the image
    if (py >= Hp) py -= Hp;
    if (px >= Wp) px -= Wp;
    const float *base = qkv + (size_t)(head * d) * plane;
    const float *qp = base + (size_t)py * pitch + px;
    float q[DP], o[DP];
#pragma unroll
    for (int dd = 0; dd < DP; ++dd) q[dd] = dd < d ? qp[(size_t)dd * plane] : 0.0f;
    auto load = [&](int c, bool with_v) {
        __syncthreads();                                   // the chunk before this one has been consumed
        if (t < CH) {
            const int j = c * CH + t;
            int ky, kx;
            bool in = true;
            if constexpr (A::OCA) {
                ky = by * HT_WIN - HT_OFF + j / HT_EXT;
                kx = bx * HT_WIN - HT_OFF + j % HT_EXT;
                in = ky >= 0 && ky < Hp && kx >= 0 && kx < Wp;
            } else {
                ky = by * HT_WIN + (j >> 4) + shift;
                kx = bx * HT_WIN + (j & 15) + shift;
                if (ky >= Hp) ky -= Hp;
                if (kx >= Wp) kx -= Wp;
            }
            const float *kp = base + (size_t)C * plane + (size_t)(in ? ky : 0) * pitch + (in ? kx : 0);
            const float *vp = kp + (size_t)C * plane;
#pragma unroll 4                                           // fully unrolled, the loads in flight cost 170 .. 255 VGPRs
            for (int dd = 0; dd < DP; ++dd) {
                const bool rd = in && dd < d;
                Ks[dd * CH + t] = rd ? kp[(size_t)dd * plane] : 0.0f;
                if (with_v) Vs[dd * CH + t] = rd ? vp[(size_t)dd * plane] : 0.0f;
            }
        }
        __syncthreads();
    };
    const float *bp = bias + (size_t)head * (A::NK * HT_TOK) + t;
    const int ri = 3 * ht_region(sy, Hp) + ht_region(sx, Wp);
    auto masked = [&](int j) {
        if constexpr (A::OCA) return false;
        else return shift != 0 && 3 * ht_region(by * HT_WIN + (j >> 4), Hp) + ht_region(bx * HT_WIN + (j & 15), Wp) != ri;
    };
    ht_sweeps<DP, A::NK, CH>(q, Ks, Vs, bp, load, masked, o);
    float *op = out + (size_t)(head * d) * oplane + (size_t)py * opitch + px;
#pragma unroll
    for (int dd = 0; dd < DP; ++dd)
        if (dd < d) op[(size_t)dd * oplane] = o[dd];
    if (head == 0) {
        float *zp = out + (size_t)py * opitch + px;
        for (int c = C; c < Cp; ++c) zp[(size_t)c * oplane] = 0.0f;
    }
}

template <int DP>
__global__ __launch_bounds__(256) void k_hat_attention(const float *__restrict__ qkv, long long plane, int pitch, int Hp, int Wp, int C, int d,
                                                       int shift, const float *__restrict__ bias, float *__restrict__ out, long long oplane,
                                                       int opitch, int Cp)
{
    ht_attend<DP, HtWindow>(qkv, plane, pitch, Hp, Wp, C, d, shift, bias, out, oplane, opitch, Cp);
}

template <int DP>
__global__ __launch_bounds__(256) void k_hat_oca(const float *__restrict__ qkv, long long plane, int pitch, int Hp, int Wp, int C, int d,
                                                 int shift, const float *__restrict__ bias, float *__restrict__ out, long long oplane, int opitch,
                                                 int Cp)
{
    ht_attend<DP, HtOverlap>(qkv, plane, pitch, Hp, Wp, C, d, 0, bias, out, oplane, opitch, Cp);
}

// The launch of either kernel (A: HtWindow, with shift 0 or 8, or HtOverlap, shift 0).
template <typename A>
void ht_launch(hipStream_t st, const float *qkv, long long plane, int pitch, int hp, int wp, int C, int heads, int shift, const float *bias,
               float *out, long long oplane, int opitch, int Cp)
{
    const int d = C / heads;
    const dim3 grid((hp / HT_WIN) * (wp / HT_WIN), heads), block(HT_TOK);
    auto go = [&](auto window, auto overlap) {
        if constexpr (A::OCA) hipLaunchKernelGGL(overlap, grid, block, 0, st, qkv, plane, pitch, hp, wp, C, d, shift, bias, out, oplane, opitch, Cp);
        else hipLaunchKernelGGL(window, grid, block, 0, st, qkv, plane, pitch, hp, wp, C, d, shift, bias, out, oplane, opitch, Cp);
    };
    if (d <= 8) go(k_hat_attention<8>, k_hat_oca<8>);
    else if (d <= 16) go(k_hat_attention<16>, k_hat_oca<16>);
    else if (d <= 24) go(k_hat_attention<24>, k_hat_oca<24>);
    else go(k_hat_attention<32>, k_hat_oca<32>);
}

// A bias table [rows][heads] gathered through idx [256][nk] to [head][key j][query i].
std::vector<float> ht_gather_bias(const float *table, const int *idx, int nk, int heads)
{
    std::vector<float> g((size_t)heads * nk * HT_TOK);
    for (int hd = 0; hd < heads; ++hd)
        for (int j = 0; j < nk; ++j)
            for (int i = 0; i < HT_TOK; ++i) g[((size_t)hd * nk + j) * HT_TOK + i] = table[(size_t)idx[i * nk + j] * heads + hd];
    return g;
}

}  // namespace

struct sr_hat_model : SrModelBase {            // d_w, d_b: per table (ht_tables)
    sr_hat_desc d{};
    std::vector<SwTable> tables;
    DevBuf trunk[5];                          // H, R, X, A, U
    DevBuf tbuf;                              // the CAB's middle tensor
    DevBuf qbuf;                              // qkv / hidden
    DevBuf tailbuf[2];
    DevBuf img;                               // the reflected u8 image
    DevBuf red;                               // C x chunks float64 chunk sums, then s[C]
    void release_device()
    {
        for (auto &b : trunk) b.release();
        for (DevBuf *b : {&tailbuf[0], &tailbuf[1], &tbuf, &qbuf, &img, &red}) b->release();
        release_base();
    }
};

static LiveSet g_ht_live;

static int ht_reserve(sr_hat_model *m, const HtGeom &g, const char *who)
{
    sr_ctx *ctx = m->ctx;
    int rc;
    if ((rc = ensure_activation_buffers(ctx, m->trunk, 5, (size_t)g.plane0 * g.cp, who))) return rc;
    if ((rc = ensure_activation_buffers(ctx, &m->tbuf, 1, (size_t)g.plane0 * g.tp, who))) return rc;
    if ((rc = ensure_activation_buffers(ctx, &m->qbuf, 1, (size_t)g.plane0 * g.qp, who))) return rc;
    if (g.plane_t && (rc = ensure_activation_buffers(ctx, m->tailbuf, 2, (size_t)g.plane_t * SW_MID, who))) return rc;
    SRCHK(m->img.reserve(ctx, who, (size_t)g.plane0 * 3));
    SRCHK(m->red.reserve(ctx, who, (size_t)m->d.n_feat * g.chunks * sizeof(double) + (size_t)m->d.n_feat * sizeof(float)));
    return SR_OK;
}

static int ht_forward(sr_hat_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride, int tail,
                      bool u8, const char *who)
{
    if (!g_ht_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    sr_ctx *ctx = m->ctx;
    CTX_ENTER(ctx);
    const sr_hat_desc &D = m->d;
    const int C = D.n_feat, heads = D.n_heads, S = D.scale, R = D.n_squeeze;
    int rc = check_sr_forward_args(who, d_src, src_stride, w, d_dst, dst_stride, S, u8);
    if (rc) return rc;
    HtGeom g;
    if ((rc = ht_geometry(who, D, h, w, tail, g))) return rc;
    if ((rc = ht_reserve(m, g, who))) return rc;
    const int hp = g.hp, wp = g.wp, Cp = g.cp, Tp = g.tp, hidp = sw_pad64(D.n_hidden), qkvp = sw_pad64(3 * C);
    hipStream_t st = ctx->stream;
    SwEpi ep{};
    ep.af = {{D.mean[0], D.mean[1], D.mean[2]}, D.range};
    ep.dst = d_dst;
    ep.dst_stride = (long long)dst_stride;
    ep.s = 1;
    ep.nq = C;
    ep.qscale = 1.0f / sqrtf((float)(C / heads));
    // ---- trunk phase: the whole padded image, every tensor in one layout ----
    const PlanarTen L = planar_tensor(nullptr, 0, 0, hp, wp);
    auto ten = [&](float *base) { PlanarTen t = L; t.p = base; return t; };
    ep.skip_plane = L.plane;
    ep.skip_pitch = L.pitch;
    float *Hb = m->trunk[0].as<float>(), *Rb = m->trunk[1].as<float>(), *Xb = m->trunk[2].as<float>(), *Ab = m->trunk[3].as<float>();
    float *Ub = m->trunk[4].as<float>(), *Tb = m->tbuf.as<float>(), *Qb = m->qbuf.as<float>();
    unsigned char *img = m->img.as<unsigned char>();
    const size_t part_bytes = (size_t)C * g.chunks * sizeof(double);
    double *part = m->red.as<double>();
    float *sc = m->red.as<float>(part_bytes);
    const long long plane4 = L.plane / 4;
    auto lin = [&](auto kernel, float *in, int cin, int k, int cout_planes, float *out, const float *skip) {
        ProfScope ps(ctx, "hat_linear");
        SwEpi e = ep;
        e.skip = skip;
        launch_conv(kernel, st, ten(in), hp, wp, cin, cout_planes / 64, m->w(k), m->b(k), out, L.plane, L.pitch, 0, 0, hp, wp, e);
    };
    auto conv = [&](float *in, int k, float *out, const float *skip) {
        ProfScope ps(ctx, "hat_conv");
        SwEpi e = ep;
        e.skip = skip;
        launch_conv(k_sw_conv<2, SW_ADD>, st, ten(in), hp, wp, Cp, Cp / 64, m->w(k), m->b(k), out, L.plane, L.pitch, 0, 0, hp, wp, e);
    };
    auto norm = [&](float *in, int k, float *out) {
        ProfScope ps(ctx, "hat_ln");
        sw_launch_layernorm(st, in, L.plane, L.pitch, hp, wp, C, Cp, m->w(k), m->b(k), out, L.plane, L.pitch);
    };
    auto mlp = [&](int k) {                                // x = x + fc2(gelu(fc1(LN2(x)))) on X; tables k, k + 1, k + 2
        norm(Xb, k, Ab);
        lin(k_sw_lin<SL_GELU>, Ab, Cp, k + 1, hidp, Qb, nullptr);
        lin(k_sw_lin<SL_ADD>, Qb, hidp, k + 2, Cp, Xb, Xb);
    };
    {
        ProfScope ps(ctx, "hat_head");
        const long long n = (long long)g.plane0 * 3;
        hipLaunchKernelGGL(k_hat_reflect, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_src, (long long)src_stride, h, w, img, hp, wp);
        hipLaunchKernelGGL(k_sw_head, dim3((wp + 63) / 64, (hp + 3) / 4, Cp / 64), dim3(64, 4), 0, st, img, (long long)wp * 3, hp, wp, m->w(0), m->b(0),
                           ep.af, Hb, hp, wp, L.pitch, L.plane);
    }
    int k = 1;
    norm(Hb, k++, Rb);
    for (int gi = 0; gi < D.n_groups; ++gi) {
        float *x = Rb;                                     // the first layer reads the RHAG's input and writes X
        for (int j = 0; j < D.depth; ++j, k += 11) {
            norm(x, k, Ab);
            {                                              // the CAB on LN1's output, before the attention takes A
                ProfScope ps(ctx, "hat_cab_conv");
                launch_conv(k_sw_conv<2, SW_GELU>, st, ten(Ab), hp, wp, Cp, Tp / 64, m->w(k + 4), m->b(k + 4), Tb, L.plane, L.pitch, 0, 0, hp, wp, ep);
                launch_conv(k_sw_conv<2, SW_PLAIN>, st, ten(Tb), hp, wp, Tp, Cp / 64, m->w(k + 5), m->b(k + 5), Ub, L.plane, L.pitch, 0, 0, hp, wp, ep);
            }
            rc_attention(st, ctx, Ub, L.plane, L.pitch, hp, wp, C, R, m->w(k + 6), m->b(k + 6), m->w(k + 7), m->b(k + 7), part, sc, nullptr,
                         "hat_cab_reduce", "hat_cab_attention");
            lin(k_sw_lin<SL_QKV>, Ab, Cp, k + 1, qkvp, Qb, nullptr);
            {
                ProfScope ps(ctx, "hat_attention");
                ht_launch<HtWindow>(st, Qb, L.plane, L.pitch, hp, wp, C, heads, j % 2 ? HT_SHIFT : 0, m->w(k + 2), Ab, L.plane, L.pitch, Cp);
            }
            lin(k_sw_lin<SL_ADD>, Ab, Cp, k + 3, Cp, Xb, x);
            x = Xb;
            {
                ProfScope ps(ctx, "hat_cab_scale");
                hipLaunchKernelGGL(k_rc_scale, dim3((unsigned)((plane4 + 255) / 256), C), dim3(256), 0, st, (const float4 *)Ub, sc, (const float4 *)Xb,
                                   (float4 *)Xb, plane4, D.conv_scale);
            }
            mlp(k + 8);
        }
        norm(x, k, Ab);                                    // the OCAB
        lin(k_sw_lin<SL_QKV>, Ab, Cp, k + 1, qkvp, Qb, nullptr);
        {
            ProfScope ps(ctx, "hat_oca");
            ht_launch<HtOverlap>(st, Qb, L.plane, L.pitch, hp, wp, C, heads, 0, m->w(k + 2), Ab, L.plane, L.pitch, Cp);
        }
        lin(k_sw_lin<SL_ADD>, Ab, Cp, k + 3, Cp, Xb, x);
        x = Xb;
        mlp(k + 4);
        k += 7;
        conv(x, k++, Rb, Rb);                              // in place over the RHAG's input
    }
    norm(Rb, k++, Ab);
    conv(Ab, k++, Hb, Hb);                                 // f = conv_after_body(.) + h, in place over h
    if ((rc = check_launch(who))) return rc;
    // ---- tail phase: sub-pieces of the input over their own backward extents (as sr_swinir.hip's pixelshuffle tail) ----
    const std::vector<SwStep> steps = ht_tail_steps(D);
    const int n = (int)steps.size();
    const PlanarTen f = ten(Hb);
    std::vector<int> ya, yb, xa, xb;
    for (int sy = 0; sy < h; sy = (int)std::min<long long>((long long)sy + g.tail, h))
        for (int sx = 0; sx < w; sx = (int)std::min<long long>((long long)sx + g.tail, w)) {
            sw_backward_extents(steps.data(), n, S, sy, (int)std::min<long long>((long long)sy + g.tail, h), hp, ya, yb);
            sw_backward_extents(steps.data(), n, S, sx, (int)std::min<long long>((long long)sx + g.tail, w), wp, xa, xb);
            PlanarTen t = f;
            ProfScope ps(ctx, "hat_tail");
            for (int i = 0; i < n; ++i) {
                const int rows = yb[i] - ya[i], cols = xb[i] - xa[i], mult = steps[i].mult, r = steps[i].r, kt = k + i;
                const int kind = m->tables[kt].kind, cin = i == 0 ? Cp : SW_MID;
                SwEpi e = ep;
                e.slope = 0.01f;
                e.s = r;
                if (i + 1 < n) {
                    const PlanarTen o = planar_tensor(m->tailbuf[i & 1].as<float>(), ya[i] * r, xa[i] * r, rows * r, cols * r);
                    auto go = [&](auto kernel, int tiles) {
                        launch_conv(kernel, st, t, hp * mult, wp * mult, cin, tiles, m->w(kt), m->b(kt), o.p, o.plane, o.pitch, ya[i], xa[i], rows, cols, e);
                    };
                    if (kind == SW_T_UP && r == 2) go(k_sw_conv<2, SW_SHUF2>, 4);
                    else if (kind == SW_T_UP) go(k_sw_conv<2, SW_SHUF3>, 9);
                    else go(k_sw_conv<2, SW_ACT>, 1);
                    t = o;
                } else {
                    auto go = [&](auto kernel) {
                        launch_conv(kernel, st, t, hp * mult, wp * mult, cin, 1, m->w(kt), m->b(kt), nullptr, 0LL, 0, ya[i], xa[i], rows, cols, e);
                    };
                    if (u8) go(k_sw_conv<1, SW_LAST_U8>);
                    else go(k_sw_conv<1, SW_LAST_F32>);
                }
            }
            if ((rc = check_launch(who))) return rc;
        }
    return SR_OK;
}

// The self-ensemble over ht_forward (driver: sr_ensemble.hip): every member is reflected, padded and windowed on its own.
static int ht_ensemble(sr_hat_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride, int tail,
                       int mask, bool u8, const char *who)
{
    const int rc = sr_ens_check_mask(who, mask);
    if (rc) return rc;
    if (tail < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: %s must be >= 1, or 0 for the library's choice", who, "tail");
    if (!g_ht_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    return ens_run(who, *m, m->d.scale, [&](const uint8_t *s, int64_t ss, int hh, int ww, float *d, int64_t ds) {
        return ht_forward(m, s, ss, hh, ww, d, ds, tail, false, who);
    }, d_src, src_stride, h, w, d_dst, dst_stride, mask, u8);
}

// What the two inspection entry points share: the checks of the description of one attention call.
static int ht_check_attention(const char *who, int C, int n_heads, int hp, int wp)
{
    if (C < 1 || C > 256 || n_heads < 1 || C % n_heads || C / n_heads > 32)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d channels in %d heads is outside C <= 256, heads of at most 32 channels", who, C, n_heads);
    if (hp < HT_WIN || wp < HT_WIN || hp % HT_WIN || wp % HT_WIN)
        return sr_set_error(SR_ERR_SHAPE, "%s: a %dx%d tensor is not made of %d x %d windows", who, wp, hp, HT_WIN, HT_WIN);
    return SR_OK;
}

extern "C" {

int sr_hat_create(sr_ctx *ctx, const sr_hat_desc *desc, const float *const *h_w, const float *const *h_b, int n_tables, const int *h_rpi_oca,
                  sr_hat_model **out)
{
    const char *who = "sr_hat_create";
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null out", who);
    *out = nullptr;
    int rc = ht_check_desc(who, desc);                                      // host decision, before any device call
    if (rc) return rc;
    const std::vector<SwTable> tables = ht_tables(*desc);
    if (!h_w || !h_b) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null weight table", who);
    if (n_tables != (int)tables.size())
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: this description has %d tables, %d given", who, (int)tables.size(), n_tables);
    for (int k = 0; k < n_tables; ++k) {
        const bool rpb = tables[k].kind == SW_T_RPB || tables[k].kind == HT_T_RPB_OCA;
        if (!h_w[k] || (!h_b[k] && !rpb)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null array of table %d", who, k);
    }
    std::vector<int> rel(HT_TOK * HT_TOK), oca(HT_TOK * HT_KEYS);
    ht_rel_index(rel.data());
    if (h_rpi_oca) {
        if ((rc = ht_wrap_oca_index(who, h_rpi_oca, oca.data()))) return rc;
    } else {
        ht_oca_index(oca.data());
    }
    CTX_ENTER(ctx);
    sr_hat_model *M = new sr_hat_model();
    M->ctx = ctx;
    M->d = *desc;
    M->tables = tables;
    g_ht_live.insert(M);
    const int C = desc->n_feat, Cp = sw_pad64(C), hidp = sw_pad64(desc->n_hidden), Tp = sw_pad64(desc->n_mid), R = desc->n_squeeze;
    for (int k = 0; k < n_tables; ++k) {
        const SwTable &t = tables[k];
        MfmaWeights a;
        switch (t.kind) {
        case SW_T_HEAD: {
            std::vector<float> wpad((size_t)Cp * 27, 0.0f);
            std::memcpy(wpad.data(), h_w[k], (size_t)C * 27 * sizeof(float));
            a.w = arrange_head_weights(wpad.data(), Cp);
            a.b.assign(Cp, 0.0f);
            std::memcpy(a.b.data(), h_b[k], (size_t)C * sizeof(float));
            break;
        }
        case SW_T_LN:
            a = {std::vector<float>(h_w[k], h_w[k] + C), std::vector<float>(h_b[k], h_b[k] + C)};
            break;
        case SW_T_RPB:
            a = {ht_gather_bias(h_w[k], rel.data(), HT_TOK, desc->n_heads), std::vector<float>(1, 0.0f)};
            break;
        case HT_T_RPB_OCA:
            a = {ht_gather_bias(h_w[k], oca.data(), HT_KEYS, desc->n_heads), std::vector<float>(1, 0.0f)};
            break;
        case SW_T_QKV: case SW_T_PROJ: case SW_T_FC1:
            a = sw_arrange(h_w[k], h_b[k], t.cout, t.cin, 1, Cp, SW_LIN_CC, 64);
            break;
        case SW_T_FC2:
            a = sw_arrange(h_w[k], h_b[k], t.cout, t.cin, 1, hidp, SW_LIN_CC, 64);
            break;
        case SW_T_CONV: case SW_T_CBU: case HT_T_CAB0:
            a = sw_arrange(h_w[k], h_b[k], t.cout, t.cin, 9, Cp, 8, 64);
            break;
        case HT_T_CAB2:
            a = sw_arrange(h_w[k], h_b[k], t.cout, t.cin, 9, Tp, 8, 64);
            break;
        case HT_T_ATT1:
            a = {std::vector<float>(h_w[k], h_w[k] + (size_t)R * C), std::vector<float>(h_b[k], h_b[k] + R)};
            break;
        case HT_T_ATT3:
            a = {std::vector<float>(h_w[k], h_w[k] + (size_t)C * R), std::vector<float>(h_b[k], h_b[k] + C)};
            break;
        case SW_T_LAST:
            a = sw_arrange(h_w[k], h_b[k], t.cout, t.cin, 9, SW_MID, 8, 32);
            break;
        default:                                                            // SW_T_UP
            a = sw_arrange(h_w[k], h_b[k], t.cout, t.cin, 9, SW_MID, 8, 64);
        }
        if ((rc = upload_conv(who, *M, a))) {
            sr_hat_destroy(M);
            return rc;
        }
    }
    *out = M;
    return SR_OK;
}

int sr_hat_destroy(sr_hat_model *m)
{
    return destroy_model(m, g_ht_live);
}

int sr_hat_u8(sr_hat_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride, int tail)
{
    return ht_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tail, true, "sr_hat_u8");
}

int sr_hat_f32(sr_hat_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride, int tail)
{
    return ht_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tail, false, "sr_hat_f32");
}

int sr_hat_ens_u8(sr_hat_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride, int tail,
                  int mask)
{
    return ht_ensemble(model, d_src, src_stride, h, w, d_dst, dst_stride, tail, mask, true, "sr_hat_ens_u8");
}

int sr_hat_ens_f32(sr_hat_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride, int tail,
                   int mask)
{
    return ht_ensemble(model, d_src, src_stride, h, w, d_dst, dst_stride, tail, mask, false, "sr_hat_ens_f32");
}

int sr_hat_fill_workspace(sr_hat_model *m, int h, int w, int tail, int byte)
{
    const char *who = "sr_hat_fill_workspace";
    if (!g_ht_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    sr_ctx *ctx = m->ctx;
    CTX_ENTER(ctx);
    HtGeom g;
    int rc = ht_geometry(who, m->d, h, w, tail, g);
    if (rc) return rc;
    if ((rc = ht_reserve(m, g, who))) return rc;
    for (DevBuf *b : {&m->trunk[0], &m->trunk[1], &m->trunk[2], &m->trunk[3], &m->trunk[4], &m->tbuf, &m->qbuf, &m->tailbuf[0], &m->tailbuf[1],
                      &m->img, &m->red})
        if (b->d) HIPCHK(hipMemsetAsync(b->d, byte, b->cap, ctx->stream));
    return SR_OK;
}

int sr_hat_attention_f32(sr_ctx *ctx, const float *d_qkv, int64_t plane_stride, int64_t row_stride, int n_feat, int n_heads, int hp, int wp,
                         int shift, const float *h_table, float *d_out, int64_t out_plane_stride, int64_t out_row_stride)
{
    const char *who = "sr_hat_attention_f32";
    if (!d_qkv || !h_table || !d_out) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = ht_check_attention(who, n_feat, n_heads, hp, wp))) return rc;
    if (shift != 0 && shift != HT_SHIFT) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: shift %d (supported: 0, %d)", who, shift, HT_SHIFT);
    if ((rc = sw_check_view(who, d_qkv, plane_stride, row_stride, hp, wp))) return rc;
    if ((rc = sw_check_view(who, d_out, out_plane_stride, out_row_stride, hp, wp))) return rc;
    CTX_ENTER(ctx);
    std::vector<int> rel(HT_TOK * HT_TOK);
    ht_rel_index(rel.data());
    const std::vector<float> g = ht_gather_bias(h_table, rel.data(), HT_TOK, n_heads);
    DevTemp tmp(ctx);
    SRCHK(tmp.alloc(who, g.size() * sizeof(float)));
    HIPCHK(hipMemcpyAsync(tmp.d, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    ht_launch<HtWindow>(ctx->stream, d_qkv, plane_stride / 4, (int)(row_stride / 4), hp, wp, n_feat, n_heads, shift, tmp.as<float>(), d_out,
                        out_plane_stride / 4, (int)(out_row_stride / 4), n_feat);
    SRCHK(check_launch(who));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_hat_oca_f32(sr_ctx *ctx, const float *d_qkv, int64_t plane_stride, int64_t row_stride, int n_feat, int n_heads, int hp, int wp,
                   const float *h_table, const int *h_index, float *d_out, int64_t out_plane_stride, int64_t out_row_stride)
{
    const char *who = "sr_hat_oca_f32";
    if (!d_qkv || !h_table || !d_out) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = ht_check_attention(who, n_feat, n_heads, hp, wp))) return rc;
    if ((rc = sw_check_view(who, d_qkv, plane_stride, row_stride, hp, wp))) return rc;
    if ((rc = sw_check_view(who, d_out, out_plane_stride, out_row_stride, hp, wp))) return rc;
    std::vector<int> oca(HT_TOK * HT_KEYS);
    if (h_index) {
        if ((rc = ht_wrap_oca_index(who, h_index, oca.data()))) return rc;
    } else {
        ht_oca_index(oca.data());
    }
    CTX_ENTER(ctx);
    const std::vector<float> g = ht_gather_bias(h_table, oca.data(), HT_KEYS, n_heads);
    DevTemp tmp(ctx);
    SRCHK(tmp.alloc(who, g.size() * sizeof(float)));
    HIPCHK(hipMemcpyAsync(tmp.d, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    ht_launch<HtOverlap>(ctx->stream, d_qkv, plane_stride / 4, (int)(row_stride / 4), hp, wp, n_feat, n_heads, 0, tmp.as<float>(), d_out,
                  out_plane_stride / 4, (int)(out_row_stride / 4), n_feat);
    SRCHK(check_launch(who));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // extern "C"
