// sr_swin2sr.hip -- local super-resolution backend: Swin2SR (Conde et al. 2022; SwinV2 cosine attention with a continuous
// position bias, post-norm; resi_connection '1conv', patch size 1, window 8) on gfx950, as the `transformers` package computes
// it.  The definition is in include/sr_hip.h ("Swin2SR").
//
//   input       SwinIR's: the u8 image extended by symmetric reflection to Hp x Wp (k_sw_reflect)
//   head        3 x 3 convolution 3 -> C                                                                          -> h
//   embedding   e = P_0 h + b (1 x 1, C -> C);  r = LN(e)
//   stage       x = r;  D layers on x;  r = P_i(conv3x3(x)) + r
//     layer     qkv = W x + b on x itself (no pre-norm, no k bias, q unscaled);  cosine window attention (shift 0 / 4);
//               x = x + LN1(proj(.));  x = x + LN2(fc2(gelu(fc1(x))))
//   long skip   f = conv_after_body(LN(r)) + h
//   tail        SwinIR's three reconstructions
//
// This file keeps the cosine window attention, the body of one stage, Swin2SR's own table kinds and the entry points; the
// reflection, the head, the LayerNorm with and without a skip, the linear layers, the 3 x 3 convolutions, the tail phase and the
// frame around the stages are sr_swin_common.h, shared with sr_swinir.hip and sr_hat.hip.  The trunk fits SwinIR's five buffers:
// qkv X -> Q;  attention Q -> A;  proj A -> Q's first Cp planes;  LN + skip -> X;  fc1 X -> Q;  fc2 Q -> A;  LN + skip -> X.  The
// first layer of a stage reads its x and its skip from R and writes X, so that R stays whole; every later LN + skip runs in place
// over X.  The stage's convolution goes to A and P_i adds r in place over R.  Every kernel that writes a tensor writes all its
// planes (the LN + skip and the attention store explicit zeros into the planes C .. Cp - 1).
//
// Cosine attention (k_s2_attention): one wave per (window, head), lane = token, as k_sw_attention.  The lane that owns a token
// forms ss = sum q^2 (an fmaf chain over dd ascending from +0), n = sqrtf(ss), and stores q / fmaxf(n, 1e-12f) into LDS -- k
// likewise -- so that the score loop is SwinIR's; then a = s * scale_h (one multiply) + bias, + mask_value where SwinIR's region
// rule masks, the exact maximum, expf(a - max), the sum over keys ascending, the division, the p v fmaf chain.  scale_h (the
// clamped exp of logit_scale) and the bias (the cpb MLP's table, gathered to [head][key][query]) come from the host
// (sr_swin2sr_host.cpp).  No atomics.  Equal inputs give equal bits.  Registers: DESIGN.md, "Swin2SR".
//
// Weights are caller-supplied (sr_swin2sr_create); nothing is fetched.
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_net_common.h"
#include "sr_swin2sr.h"
#include "sr_swin_common.h"

namespace {

// Region of coordinate v of the shifted image along an axis of length L (SwinIR's rule: calculate_mask's three slices).
__device__ __forceinline__ int s2_region(int v, int L) { return v < L - SW_WIN ? 0 : (v < L - SW_SHIFT ? 1 : 2); }

// ---------------------------------------------------------------------------------------------------------------
// Cosine window attention of one head of one 8 x 8 window per wave (block 64; grid (windows, heads)); the orders are at the top
// of this file.  qkv planar: q of channel c in plane c, k in plane C + c, v in plane 2 C + c.  bias: [head][key j][query i];
// scale: [head].  DP: the head width d rounded up to a multiple of 8 (the LDS size).  Writes channels [head d, (head + 1) d) of
// out; head 0 also writes +0 into the planes C .. Cp - 1.
// ---------------------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(64) void k_s2_attention(const float *__restrict__ qkv, long long plane, int pitch, int Hp, int Wp, int C, int d,
                                                     int shift, const float *__restrict__ bias, const float *__restrict__ scale,
                                                     float mask_value, float *__restrict__ out, long long oplane, int opitch, int Cp)
{
    __shared__ __attribute__((aligned(16))) float Ks[DP * SW_TOK];
    __shared__ __attribute__((aligned(16))) float QVs[DP * SW_TOK];            // q while the scores are formed, then v
    const int t = threadIdx.x, head = blockIdx.y, nwx = Wp / SW_WIN;
    const int by = blockIdx.x / nwx, bx = blockIdx.x % nwx;
    const int sy = by * SW_WIN + (t >> 3), sx = bx * SW_WIN + (t & 7);        // in the shifted image
    int py = sy + shift, px = sx + shift;                                      // in the image
    if (py >= Hp) py -= Hp;
    if (px >= Wp) px -= Wp;
    const float *qp = qkv + (size_t)(head * d) * plane + (size_t)py * pitch + px;
    const float *kp = qp + (size_t)C * plane, *vp = kp + (size_t)C * plane;
    // the token's own lane: the raw values into its LDS column and the two sums of squares, then the division in place
    float qs = 0.0f, ks = 0.0f;
#pragma unroll 1
    for (int dd = 0; dd < d; ++dd) {
        const float qv = qp[(size_t)dd * plane], kv = kp[(size_t)dd * plane];
        qs = fmaf(qv, qv, qs);
        ks = fmaf(kv, kv, ks);
        QVs[dd * SW_TOK + t] = qv;
        Ks[dd * SW_TOK + t] = kv;
    }
    const float qn = fmaxf(sqrtf(qs), 1e-12f), kn = fmaxf(sqrtf(ks), 1e-12f);
#pragma unroll 1
    for (int dd = 0; dd < d; ++dd) {
        QVs[dd * SW_TOK + t] = QVs[dd * SW_TOK + t] / qn;
        Ks[dd * SW_TOK + t] = Ks[dd * SW_TOK + t] / kn;
    }
    __syncthreads();
    // the channel loop stays rolled, as k_sw_attention's: it holds the 64 scores and one channel's 16 float4 of k
    float s[SW_TOK];
#pragma unroll
    for (int j = 0; j < SW_TOK; ++j) s[j] = 0.0f;
#pragma unroll 1
    for (int dd = 0; dd < d; ++dd) {
        const float qv = QVs[dd * SW_TOK + t];
#pragma unroll
        for (int j4 = 0; j4 < SW_TOK / 4; ++j4) {
            const f4v k4 = *(const f4v *)&Ks[dd * SW_TOK + 4 * j4];
            s[4 * j4] = fmaf(qv, k4.x, s[4 * j4]);
            s[4 * j4 + 1] = fmaf(qv, k4.y, s[4 * j4 + 1]);
            s[4 * j4 + 2] = fmaf(qv, k4.z, s[4 * j4 + 2]);
            s[4 * j4 + 3] = fmaf(qv, k4.w, s[4 * j4 + 3]);
        }
    }
    __syncthreads();                                       // q has been consumed: its place takes v
#pragma unroll 1
    for (int dd = 0; dd < d; ++dd) QVs[dd * SW_TOK + t] = vp[(size_t)dd * plane];
    __syncthreads();
    const float *Vs = QVs;
    const float *bp = bias + (size_t)head * (SW_TOK * SW_TOK) + t;
    const float sc = scale[head];
    const int ri = 3 * s2_region(sy, Hp) + s2_region(sx, Wp);
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < SW_TOK; ++j) {
        float a = s[j] * sc + bp[j * SW_TOK];
        if (shift) {
            const int rj = 3 * s2_region(by * SW_WIN + (j >> 3), Hp) + s2_region(bx * SW_WIN + (j & 7), Wp);
            if (rj != ri) a = a + mask_value;
        }
        s[j] = a;
        mx = fmaxf(mx, a);
    }
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < SW_TOK; ++j) {
        s[j] = expf(s[j] - mx);
        sum += s[j];
    }
#pragma unroll
    for (int j = 0; j < SW_TOK; ++j) s[j] = s[j] / sum;
    float *op = out + (size_t)(head * d) * oplane + (size_t)py * opitch + px;
#pragma unroll 1
    for (int dd = 0; dd < d; ++dd) {
        float a = 0.0f;
#pragma unroll
        for (int j4 = 0; j4 < SW_TOK / 4; ++j4) {
            const f4v v4 = *(const f4v *)&Vs[dd * SW_TOK + 4 * j4];
            a = fmaf(s[4 * j4], v4.x, a);
            a = fmaf(s[4 * j4 + 1], v4.y, a);
            a = fmaf(s[4 * j4 + 2], v4.z, a);
            a = fmaf(s[4 * j4 + 3], v4.w, a);
        }
        op[(size_t)dd * oplane] = a;
    }
    if (head == 0) {
        float *zp = out + (size_t)py * opitch + px;
        for (int c = C; c < Cp; ++c) zp[(size_t)c * oplane] = 0.0f;
    }
}

void s2_launch_attention(hipStream_t st, const float *qkv, long long plane, int pitch, int hp, int wp, int C, int heads, int shift,
                         const float *bias, const float *scale, float mask_value, float *out, long long oplane, int opitch, int Cp)
{
    const int d = C / heads;
    sw_launch_by_d(d, k_s2_attention<8>, k_s2_attention<16>, k_s2_attention<24>, k_s2_attention<32>, dim3((hp / SW_WIN) * (wp / SW_WIN), heads),
                   dim3(SW_TOK), st, qkv, plane, pitch, hp, wp, C, d, shift, bias, scale, mask_value, out, oplane, opitch, Cp);
}

void s2_launch_layernorm_add(hipStream_t st, const float *x, long long plane, long long pitch, int rows, int cols, int C, int Cp,
                                    const float *gamma, const float *beta, const float *skip, long long splane, long long spitch, float *out,
                                    long long oplane, long long opitch)
{
    const long long n = (long long)rows * cols;
    hipLaunchKernelGGL(k_sw_layernorm_add<>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, plane, pitch, rows, cols, C, Cp, gamma, beta,
                       skip, splane, spitch, out, oplane, opitch);
}

// out = skip + LN(in) with table k's gamma and beta, every tensor in the trunk's layout; out may be skip.
void s2_norm_add(const SwTrunk &T, float *in, int k, const float *skip, float *out)
{
    ProfScope ps(T.ctx, T.nm.ln);
    s2_launch_layernorm_add(T.st, in, T.L.plane, T.L.pitch, T.hp, T.wp, T.C, T.Cp, T.m->w(k), T.m->b(k), skip, T.L.plane, T.L.pitch, out, T.L.plane,
                            T.L.pitch);
}

}  // namespace

struct sr_swin2sr_model : SwModelBase {
    sr_swin2sr_desc d{};
    static constexpr bool SHUFFLE_ONLY = false;
    static constexpr bool PROJECTED = true;
    static int check_desc(const char *who, const sr_swin2sr_desc *desc) { return s2_check_desc(who, desc); }
    static std::vector<SwTable> table_list(const sr_swin2sr_desc &desc) { return s2_tables(desc); }
    static bool bias_table(int kind) { return kind == S2_T_LOGIT || kind == S2_T_CPB2; }
    int geometry(const char *who, int h, int w, int tail, SwGeom &g) const { return s2_geometry(who, d, h, w, tail, g); }
    std::vector<SwStep> tail_steps() const { return s2_tail_steps(d); }
};

static LiveSet g_s2_live;

static int s2_forward(sr_swin2sr_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride, int tail,
                      bool u8, const char *who)
{
    static const SwNames names{"swin2sr_head", "swin2sr_ln", "swin2sr_linear", "swin2sr_conv", "swin2sr_tail"};
    return sw_forward_frame(__func__, g_s2_live, m, names, k_sw_reflect<>, d_src, src_stride, h, w, d_dst, dst_stride, tail, u8, who,
                            [m](const SwTrunk &T, const SwGeom &, int &k) {       // the layers of one stage, 9 tables each
        float *x = T.Rb;                                   // the first layer reads the stage's input and writes X
        for (int j = 0; j < m->d.depth; ++j, k += S2_LAYER_TABLES) {
            T.lin(k_sw_lin<SL_PLAIN>, x, T.Cp, k, T.qkvp, T.Qb, nullptr);                  // qkv on x itself
            {
                ProfScope ps(T.ctx, "swin2sr_attention");
                s2_launch_attention(T.st, T.Qb, T.L.plane, T.L.pitch, T.hp, T.wp, T.C, m->d.n_heads, j % 2 ? SW_SHIFT : 0, m->w(k + 3), m->b(k + 3),
                                    m->d.mask_value, T.Ab, T.L.plane, T.L.pitch, T.Cp);
            }
            T.lin(k_sw_lin<SL_PLAIN>, T.Ab, T.Cp, k + 4, T.Cp, T.Qb, nullptr);             // proj -> Q's first Cp planes
            s2_norm_add(T, T.Qb, k + 5, x, T.Xb);                                              // x = x + LN1(.)
            x = T.Xb;
            T.lin(k_sw_lin<SL_GELU>, T.Xb, T.Cp, k + 6, T.hidp, T.Qb, nullptr);
            T.lin(k_sw_lin<SL_PLAIN>, T.Qb, T.hidp, k + 7, T.Cp, T.Ab, nullptr);
            s2_norm_add(T, T.Ab, k + 8, T.Xb, T.Xb);                                           // x = x + LN2(.), in place
        }
        return x;
    });
}

extern "C" {

int sr_swin2sr_create(sr_ctx *ctx, const sr_swin2sr_desc *desc, const float *const *h_w, const float *const *h_b, int n_tables,
                      sr_swin2sr_model **out)
{
    const char *who = "sr_swin2sr_create";
    int k = 0;                                             // own() sees every table once, in order
    return sw_create(who, ctx, desc, h_w, h_b, n_tables, g_s2_live, out,
                     [&] { return s2_check_tables(who, *desc, s2_tables(*desc), h_w, h_b); },
                     [&](const SwTable &t, const float *w, const float *b, MfmaWeights &a) {
        const int at = k++;
        if (t.kind == S2_T_LOGIT || t.kind == S2_T_CPB1) {
            a = {std::vector<float>(1, 0.0f), std::vector<float>(1, 0.0f)};        // read with S2_T_CPB2, two tables on
        } else if (t.kind == S2_T_CPB2) {                  // the gathered bias [head][key][query] and scale_h
            const int heads = desc->n_heads;
            std::vector<float> table((size_t)SW_REL * heads), scale(heads);
            s2_cpb_table(h_w[at - 1], h_b[at - 1], w, heads, table.data());
            s2_logit_scale(h_w[at - 2], heads, scale.data());
            a = {sw_gather_window_bias(table.data(), SW_WIN, heads), scale};
        } else if (t.kind == SW_T_UPD) {
            a = sw_arrange(w, b, t.cout, t.cin, 9, sw_pad64(desc->n_feat), 8, t.cout > 32 ? 64 : 32);
        } else if (t.kind == SW_T_C64) {
            a = sw_arrange(w, b, t.cout, t.cin, 9, SW_MID, 8, 64);
        } else {
            return false;
        }
        return true;
    });
}

int sr_swin2sr_destroy(sr_swin2sr_model *m)
{
    return destroy_model(m, g_s2_live);
}

int sr_swin2sr_u8(sr_swin2sr_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride, int tail)
{
    return s2_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tail, true, "sr_swin2sr_u8");
}

int sr_swin2sr_f32(sr_swin2sr_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride, int tail)
{
    return s2_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tail, false, "sr_swin2sr_f32");
}

int sr_swin2sr_ens_u8(sr_swin2sr_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride,
                      int tail, int mask)
{
    return sw_ensemble(g_s2_live, model, s2_forward, d_src, src_stride, h, w, d_dst, dst_stride, tail, mask, true, "sr_swin2sr_ens_u8");
}

int sr_swin2sr_ens_f32(sr_swin2sr_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride,
                       int tail, int mask)
{
    return sw_ensemble(g_s2_live, model, s2_forward, d_src, src_stride, h, w, d_dst, dst_stride, tail, mask, false, "sr_swin2sr_ens_f32");
}

int sr_swin2sr_fill_workspace(sr_swin2sr_model *m, int h, int w, int tail, int byte)
{
    return sw_fill_workspace("sr_swin2sr_fill_workspace", g_s2_live, m, h, w, tail, byte);
}

int sr_swin2sr_layernorm_add_f32(sr_ctx *ctx, const float *d_x, int64_t plane_stride, int64_t row_stride, int n_feat, int h, int w,
                                 const float *h_gamma, const float *h_beta, const float *d_skip, int64_t skip_plane_stride,
                                 int64_t skip_row_stride, float *d_out, int64_t out_plane_stride, int64_t out_row_stride)
{
    const char *who = "sr_swin2sr_layernorm_add_f32";
    if (!d_x || !h_gamma || !h_beta || !d_skip || !d_out) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    const int C = n_feat;
    if (C < 1 || C > 256) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d channels is outside 1 <= C <= 256", who, C);
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_SHAPE, "%s: %dx%d image", who, w, h);
    if (d_x == d_out || d_x == d_skip) return sr_set_error(SR_ERR_INVALID_ARG, "%s: the normalised tensor must be neither the skip nor the output", who);
    int rc;
    if ((rc = sw_check_view(who, d_x, plane_stride, row_stride, h, w))) return rc;
    if ((rc = sw_check_view(who, d_skip, skip_plane_stride, skip_row_stride, h, w))) return rc;
    if ((rc = sw_check_view(who, d_out, out_plane_stride, out_row_stride, h, w))) return rc;
    if (d_skip == d_out && (skip_plane_stride != out_plane_stride || skip_row_stride != out_row_stride))
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: in place over the skip needs the skip's strides", who);
    CTX_ENTER(ctx);
    DevTemp tmp(ctx);
    SRCHK(tmp.alloc(who, 2 * (size_t)C * sizeof(float)));
    float *gm = tmp.as<float>(), *bt = gm + C;
    HIPCHK(hipMemcpyAsync(gm, h_gamma, C * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(bt, h_beta, C * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    s2_launch_layernorm_add(ctx->stream, d_x, plane_stride / 4, row_stride / 4, h, w, C, C, gm, bt, d_skip, skip_plane_stride / 4,
                            skip_row_stride / 4, d_out, out_plane_stride / 4, out_row_stride / 4);
    SRCHK(check_launch(who));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_swin2sr_attention_f32(sr_ctx *ctx, const float *d_qkv, int64_t plane_stride, int64_t row_stride, int n_feat, int n_heads, int hp, int wp,
                             int shift, const float *h_table, const float *h_scale, float mask_value, float *d_out, int64_t out_plane_stride,
                             int64_t out_row_stride)
{
    const char *who = "sr_swin2sr_attention_f32";
    int rc;
    if ((rc = sw_check_attention_args(who, d_qkv, h_table, d_out, n_feat, n_heads))) return rc;
    if (!h_scale) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    if (shift != 0 && shift != SW_SHIFT) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: shift %d (supported: 0, %d)", who, shift, SW_SHIFT);
    if (!std::isfinite(mask_value)) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: mask_value must be finite", who);
    if ((rc = sw_check_windows(who, hp, wp, SW_WIN))) return rc;
    if ((rc = sw_check_view(who, d_qkv, plane_stride, row_stride, hp, wp))) return rc;
    if ((rc = sw_check_view(who, d_out, out_plane_stride, out_row_stride, hp, wp))) return rc;
    CTX_ENTER_AS(ctx, who);
    std::vector<float> g = sw_gather_window_bias(h_table, SW_WIN, n_heads);       // then the scales behind the bias
    const size_t nb = g.size();
    g.insert(g.end(), h_scale, h_scale + n_heads);
    DevTemp tmp(ctx);
    SRCHK(tmp.alloc(who, g.size() * sizeof(float)));
    HIPCHK(hipMemcpyAsync(tmp.d, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    s2_launch_attention(ctx->stream, d_qkv, (long long)(plane_stride / 4), (int)(row_stride / 4), hp, wp, n_feat, n_heads, shift, tmp.as<float>(),
                        tmp.as<float>() + nb, mask_value, d_out, (long long)(out_plane_stride / 4), (int)(out_row_stride / 4), n_feat);
    SRCHK(check_launch(who));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // extern "C"
