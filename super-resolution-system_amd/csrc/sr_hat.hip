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
// channel mean, the attention and the scale-and-skip pass are sr_chan_attn.h (shared with sr_rcan.hip).  The frame around the
// blocks is sr_swin_common.h's too: the model's buffers, the trunk phase's steps, the tail phase (sw_run_tail: SwinIR's
// pixelshuffle reconstruction in tail x tail sub-pieces), the create, the ensemble and the inspection calls.  This file keeps
// the two attention kernels, the reflection, the body of one RHAG, HAT's own table kinds and the entry points.
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
    if constexpr (A::OCA)
        sw_launch_by_d(d, k_hat_oca<8>, k_hat_oca<16>, k_hat_oca<24>, k_hat_oca<32>, grid, block, st, qkv, plane, pitch, hp, wp, C, d, shift, bias, out,
                       oplane, opitch, Cp);
    else
        sw_launch_by_d(d, k_hat_attention<8>, k_hat_attention<16>, k_hat_attention<24>, k_hat_attention<32>, grid, block, st, qkv, plane, pitch, hp,
                       wp, C, d, shift, bias, out, oplane, opitch, Cp);
}

// The index of an OCAB's bias table: the caller's (checked and wrapped) or the default formula.
int ht_oca_index_of(const char *who, const int *h_index, int *idx)
{
    if (h_index) return ht_wrap_oca_index(who, h_index, idx);
    ht_oca_index(idx);
    return SR_OK;
}

}  // namespace

struct sr_hat_model : SwModelBase {            // trunk[4] is U (the CAB's output); tbuf and red are in use
    sr_hat_desc d{};
    static constexpr bool SHUFFLE_ONLY = true;
    static constexpr bool PROJECTED = false;
    static int check_desc(const char *who, const sr_hat_desc *desc) { return ht_check_desc(who, desc); }
    static std::vector<SwTable> table_list(const sr_hat_desc &desc) { return ht_tables(desc); }
    static bool bias_table(int kind) { return kind == SW_T_RPB || kind == HT_T_RPB_OCA; }
    int geometry(const char *who, int h, int w, int tail, SwGeom &g) const { return ht_geometry(who, d, h, w, tail, g); }
    std::vector<SwStep> tail_steps() const { return ht_tail_steps(d); }
};

static LiveSet g_ht_live;

static int ht_forward(sr_hat_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride, int tail,
                      bool u8, const char *who)
{
    static const SwNames names{"hat_head", "hat_ln", "hat_linear", "hat_conv", "hat_tail"};
    return sw_forward_frame(__func__, g_ht_live, m, names, k_hat_reflect, d_src, src_stride, h, w, d_dst, dst_stride, tail, u8, who,
                            [m](const SwTrunk &T, const SwGeom &g, int &k) {      // one RHAG: D HABs of 11 tables, one OCAB of 7
        const sr_hat_desc &D = m->d;
        const int hp = T.hp, wp = T.wp, C = T.C, Cp = T.Cp, heads = D.n_heads;
        const PlanarTen &L = T.L;
        float *Ub = m->trunk[4].as<float>(), *Tb = m->tbuf.as<float>();
        double *part = m->red.as<double>();
        float *sc = m->red.as<float>((size_t)C * g.chunks * sizeof(double));
        const long long plane4 = L.plane / 4;
        float *x = T.Rb;                                   // the first layer reads the RHAG's input and writes X
        for (int j = 0; j < D.depth; ++j, k += 11) {
            T.norm(x, k, T.Ab);
            {                                              // the CAB on LN1's output, before the attention takes A
                ProfScope ps(T.ctx, "hat_cab_conv");
                launch_conv(k_sw_conv<2, SW_GELU>, T.st, T.ten(T.Ab), hp, wp, Cp, g.tp / 64, m->w(k + 4), m->b(k + 4), Tb, L.plane, L.pitch, 0, 0, hp, wp,
                            T.ep);
                launch_conv(k_sw_conv<2, SW_PLAIN>, T.st, T.ten(Tb), hp, wp, g.tp, Cp / 64, m->w(k + 5), m->b(k + 5), Ub, L.plane, L.pitch, 0, 0, hp, wp,
                            T.ep);
            }
            rc_attention(T.st, T.ctx, Ub, L.plane, L.pitch, hp, wp, C, D.n_squeeze, m->w(k + 6), m->b(k + 6), m->w(k + 7), m->b(k + 7), part, sc,
                         nullptr, "hat_cab_reduce", "hat_cab_attention");
            T.qkv(k + 1);
            {
                ProfScope ps(T.ctx, "hat_attention");
                ht_launch<HtWindow>(T.st, T.Qb, L.plane, L.pitch, hp, wp, C, heads, j % 2 ? HT_SHIFT : 0, m->w(k + 2), T.Ab, L.plane, L.pitch, Cp);
            }
            T.proj(k + 3, x);
            x = T.Xb;
            {
                ProfScope ps(T.ctx, "hat_cab_scale");
                hipLaunchKernelGGL(k_rc_scale, dim3((unsigned)((plane4 + 255) / 256), C), dim3(256), 0, T.st, (const float4 *)Ub, sc,
                                   (const float4 *)T.Xb, (float4 *)T.Xb, plane4, D.conv_scale);
            }
            T.mlp(k + 8);
        }
        T.norm(x, k, T.Ab);                                // the OCAB
        T.qkv(k + 1);
        {
            ProfScope ps(T.ctx, "hat_oca");
            ht_launch<HtOverlap>(T.st, T.Qb, L.plane, L.pitch, hp, wp, C, heads, 0, m->w(k + 2), T.Ab, L.plane, L.pitch, Cp);
        }
        T.proj(k + 3, x);
        x = T.Xb;
        T.mlp(k + 4);
        k += 7;
        return x;
    });
}

extern "C" {

int sr_hat_create(sr_ctx *ctx, const sr_hat_desc *desc, const float *const *h_w, const float *const *h_b, int n_tables, const int *h_rpi_oca,
                  sr_hat_model **out)
{
    const char *who = "sr_hat_create";
    std::vector<int> oca(HT_TOK * HT_KEYS);
    return sw_create(who, ctx, desc, h_w, h_b, n_tables, g_ht_live, out, [&] { return ht_oca_index_of(who, h_rpi_oca, oca.data()); },
                     [&](const SwTable &t, const float *w, const float *b, MfmaWeights &a) {
        const int C = desc->n_feat, R = desc->n_squeeze;
        if (t.kind == SW_T_RPB) a = {sw_gather_window_bias(w, HT_WIN, desc->n_heads), std::vector<float>(1, 0.0f)};
        else if (t.kind == HT_T_RPB_OCA) a = {sw_gather_bias(w, oca.data(), HT_KEYS, HT_TOK, desc->n_heads), std::vector<float>(1, 0.0f)};
        else if (t.kind == HT_T_CAB0) a = sw_arrange(w, b, t.cout, t.cin, 9, sw_pad64(C), 8, 64);
        else if (t.kind == HT_T_CAB2) a = sw_arrange(w, b, t.cout, t.cin, 9, sw_pad64(desc->n_mid), 8, 64);
        else if (t.kind == HT_T_ATT1) a = {std::vector<float>(w, w + (size_t)R * C), std::vector<float>(b, b + R)};
        else if (t.kind == HT_T_ATT3) a = {std::vector<float>(w, w + (size_t)C * R), std::vector<float>(b, b + C)};
        else return false;
        return true;
    });
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
    return sw_ensemble(g_ht_live, model, ht_forward, d_src, src_stride, h, w, d_dst, dst_stride, tail, mask, true, "sr_hat_ens_u8");
}

int sr_hat_ens_f32(sr_hat_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride, int tail,
                   int mask)
{
    return sw_ensemble(g_ht_live, model, ht_forward, d_src, src_stride, h, w, d_dst, dst_stride, tail, mask, false, "sr_hat_ens_f32");
}

int sr_hat_fill_workspace(sr_hat_model *m, int h, int w, int tail, int byte)
{
    return sw_fill_workspace("sr_hat_fill_workspace", g_ht_live, m, h, w, tail, byte);
}

int sr_hat_attention_f32(sr_ctx *ctx, const float *d_qkv, int64_t plane_stride, int64_t row_stride, int n_feat, int n_heads, int hp, int wp,
                         int shift, const float *h_table, float *d_out, int64_t out_plane_stride, int64_t out_row_stride)
{
    const char *who = "sr_hat_attention_f32";
    int rc;
    if ((rc = sw_check_attention_args(who, d_qkv, h_table, d_out, n_feat, n_heads))) return rc;
    if ((rc = sw_check_windows(who, hp, wp, HT_WIN))) return rc;
    if (shift != 0 && shift != HT_SHIFT) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: shift %d (supported: 0, %d)", who, shift, HT_SHIFT);
    return sw_run_attention(who, ctx, d_qkv, plane_stride, row_stride, n_heads, hp, wp, h_table, HT_TOK, HT_TOK, d_out, out_plane_stride,
                            out_row_stride, [](int *idx) { sw_rel_index(HT_WIN, idx); return SR_OK; },
                            [&](hipStream_t st, const float *qkv, long long plane, int pitch, const float *bias, float *out, long long oplane, int opitch) {
        ht_launch<HtWindow>(st, qkv, plane, pitch, hp, wp, n_feat, n_heads, shift, bias, out, oplane, opitch, n_feat);
    });
}

int sr_hat_oca_f32(sr_ctx *ctx, const float *d_qkv, int64_t plane_stride, int64_t row_stride, int n_feat, int n_heads, int hp, int wp,
                   const float *h_table, const int *h_index, float *d_out, int64_t out_plane_stride, int64_t out_row_stride)
{
    const char *who = "sr_hat_oca_f32";
    int rc;
    if ((rc = sw_check_attention_args(who, d_qkv, h_table, d_out, n_feat, n_heads))) return rc;
    if ((rc = sw_check_windows(who, hp, wp, HT_WIN))) return rc;
    return sw_run_attention(who, ctx, d_qkv, plane_stride, row_stride, n_heads, hp, wp, h_table, HT_KEYS, HT_TOK, d_out, out_plane_stride,
                            out_row_stride, [&](int *idx) { return ht_oca_index_of(who, h_index, idx); },
                            [&](hipStream_t st, const float *qkv, long long plane, int pitch, const float *bias, float *out, long long oplane, int opitch) {
        ht_launch<HtOverlap>(st, qkv, plane, pitch, hp, wp, n_feat, n_heads, 0, bias, out, oplane, opitch, n_feat);
    });
}

}  // extern "C"
