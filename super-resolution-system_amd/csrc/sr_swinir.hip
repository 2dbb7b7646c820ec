// sr_swinir.hip -- local super-resolution backend: BasicSR's SwinIR (Liang et al. 2021; resi_connection '1conv', no absolute
// position embedding, patch size 1, window 8) at scales 1 .. 4 on gfx950.  The definition is in include/sr_hip.h ("SwinIR").
//
//   input       the u8 image extended by symmetric reflection to Hp x Wp (multiples of 8): a small u8 pass of its own
//               (k_sw_reflect), so that the head is the other families' head_frame on a plain image
//   head        3 x 3 convolution 3 -> C, x[c] = (u8 / 255 - mean[c]) * range                                   -> h
//   deep        r = LN(h);  per RSTB: x = r, D Swin layers on x, r = conv(x) + r;  then LN(r)
//     layer     a = LN1(x);  qkv = W a + b (q scaled by d^-1/2);  window attention (shift 0 / 4 for even / odd layers);
//               x = x + proj(.);  x = x + fc2(gelu(fc1(LN2(x))))
//   long skip   f = conv_after_body(LN(r)) + h
//   tail        pixelshuffle / pixelshuffledirect / nearest+conv reconstruction, o[c] = y[c] / range + mean[c], cropped
//
// Everything is fp32 except the LayerNorm statistics (float64).  Every 3 x 3 convolution is conv_mfma_mainloop<3, 8, NC2, true>
// (sr_conv_mfma.h, v_mfma_f32_32x32x2_f32) behind an epilogue of k_sw_conv; every linear layer is the same mainloop with
// KS = 1 and CC = 32 behind an epilogue of k_sw_lin (a token is a pixel of a planar tensor, a linear layer a 1 x 1 convolution).
// CC = 32: a 1 x 1 step issues one ninth of a 3 x 3's MFMAs per channel pair, so with CC = 8 a chunk would be 16 MFMAs per wave
// between two barriers; 32 channels give 64 (the 3 x 3 mainloop: 144) for a 32 KiB patch and an 8 KiB weight slab in LDS.
//
// Channel padding: the mainloop walks cin in chunks and cout in tiles of 64, and C, 3 C and the hidden width are multiples of
// neither.  Every planar buffer therefore carries its channel count rounded up to 64 (Cp; 3 C and hidden likewise), the weight
// tables are zero-padded, and every kernel that writes a tensor writes ALL its planes: a convolution's padded couts are
// bias 0 + sum of 0 x finite = 0, the LayerNorm and the attention store explicit zeros, gelu(0) = 0.  No padded plane is ever
// read before it was written by the same forward, so the workspace's earlier content (DevBuf memory is not cleared) cannot
// enter a value -- 0 x NaN would be NaN.
//
// Shifted windows make a pixel depend on ever farther pixels (up to 12 per layer pair), so the trunk is not streamed: two phases,
// as sr_rcan.hip.
//   trunk phase  the padded image is ONE piece, in five planar fp32 buffers of Hp x Wp planes: H (h, then f in place), R (the
//                RSTB's input, then its output in place), X (the running x), A (LayerNorm output, then the attention output in
//                place of it -- they are different launches) -- Cp planes each -- and Q (qkv, then the MLP's hidden tensor):
//                max(pad64(3 C), pad64(hidden)) planes.  4 (4 Cp + Qp) bytes per pixel: 5376 at C = 180, hidden 360.
//                The first layer of an RSTB writes x into X with the skip read from R, so that R stays whole; every later
//                add-skip runs in place (a thread reads exactly the element it then writes).
//   tail phase   after f nothing is global: the reconstruction runs in tail x tail sub-pieces of the (unpadded) input over their
//                backward extents inside the padded image, two 64-plane ping-pong buffers.  The crop to (h s) x (w s) is the
//                choice of sub-pieces: nothing beyond it is computed for the last convolution.
//
// Window attention (k_sw_attention): one wave per (window, head), lane = query token.  The roll and the window partition are
// index arithmetic: token (wy, wx) of window (by, bx) is pixel ((8 by + wy + shift) mod Hp, (8 bx + wx + shift) mod Wp), read
// there and written back there.  q and k of the window lie in LDS as [channel][token] (conflict-free to write; a lane reads
// its own q, and k as broadcast float4 over four tokens), the 64 scores in registers; once the scores are formed v takes q's
// place.  The region of a token of the shifted image follows from its coordinates before the roll back: v < L - 8 -> 0,
// v < L - 4 -> 1, else 2 per axis.  94 .. 142 VGPRs, no spills (tools/kernel_regs.sh; DESIGN.md, "SwinIR").
//
// Summation orders (the contract): convolutions and linear layers as sr_conv_mfma.h (bias, channel pairs ascending, taps
// ascending, even then odd channel); the attention's dot product starts at +0 and is an fmaf chain over d ascending; the bias
// and then the mask are added to it (two adds); the softmax maximum is exact, e_j = expf(a_j - max), the sum of e_j runs over
// keys ascending from +0, p_j = e_j / sum (the division comes BEFORE the a v sum, as torch's softmax), and the a v sum is an
// fmaf chain over keys ascending from +0.  No atomics.  Nothing depends on tail.  Equal inputs give equal bits.
//
// The reflection, the head, the LayerNorm, the linear layers, the 3 x 3 convolutions (k_sw_reflect, k_sw_head, k_sw_layernorm,
// k_sw_lin, k_sw_conv), the weight arrangement and the whole frame around a family's blocks (the model's buffers, the trunk and
// the tail phase, the create, the ensemble, the inspection calls) are sr_swin_common.h, shared with sr_hat.hip and
// sr_swin2sr.hip; this file keeps the window attention, the body of one RSTB, SwinIR's own table kinds and the entry points.
//
// Weights are caller-supplied (sr_swinir_create); nothing is fetched.
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_net_common.h"
#include "sr_swin_common.h"

namespace {

// Region of coordinate v of the shifted image along an axis of length L (calculate_mask's three slices).
__device__ __forceinline__ int sw_region(int v, int L) { return v < L - SW_WIN ? 0 : (v < L - SW_SHIFT ? 1 : 2); }

// ---------------------------------------------------------------------------------------------------------------
// Window attention of one head of one 8 x 8 window per wave (block 64; grid (windows, heads)); the orders are at the top of
// this file.  qkv planar: q of channel c in plane c (already scaled), k in plane C + c, v in plane 2 C + c.  bias: the table
// gathered to [head][key j][query i] (coalesced across the lanes).  DP: the head width d rounded up to a multiple of 8 (the LDS size).
// Writes channels [head d, (head + 1) d) of out; head 0 also writes +0 into the planes C .. Cp - 1.
// ---------------------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(64) void k_sw_attention(const float *__restrict__ qkv, long long plane, int pitch, int Hp, int Wp, int C, int d,
                                                     int shift, const float *__restrict__ bias, float *__restrict__ out, long long oplane,
                                                     int opitch, int Cp)
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
#pragma unroll
    for (int dd = 0; dd < DP; ++dd)
        if (dd < d) {
            QVs[dd * SW_TOK + t] = qp[(size_t)dd * plane];
            Ks[dd * SW_TOK + t] = kp[(size_t)dd * plane];
        }
    __syncthreads();
    // the channel loop stays rolled: unrolled, the compiler hoists every LDS read of the phase and the kernel needs 256 VGPRs
    // and AGPR copies (one wave per SIMD); rolled it holds the 64 scores and one channel's 16 float4 of k
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
#pragma unroll
    for (int dd = 0; dd < DP; ++dd)
        if (dd < d) QVs[dd * SW_TOK + t] = vp[(size_t)dd * plane];
    __syncthreads();
    const float *Vs = QVs;
    const float *bp = bias + (size_t)head * (SW_TOK * SW_TOK) + t;
    const int ri = 3 * sw_region(sy, Hp) + sw_region(sx, Wp);
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < SW_TOK; ++j) {
        float a = s[j] + bp[j * SW_TOK];
        if (shift) {
            const int rj = 3 * sw_region(by * SW_WIN + (j >> 3), Hp) + sw_region(bx * SW_WIN + (j & 7), Wp);
            if (rj != ri) a = a + -100.0f;
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

void sw_launch_attention(hipStream_t st, const float *qkv, long long plane, int pitch, int hp, int wp, int C, int heads, int shift,
                         const float *bias, float *out, long long oplane, int opitch, int Cp)
{
    const int d = C / heads;
    sw_launch_by_d(d, k_sw_attention<8>, k_sw_attention<16>, k_sw_attention<24>, k_sw_attention<32>, dim3((hp / SW_WIN) * (wp / SW_WIN), heads),
                   dim3(SW_TOK), st, qkv, plane, pitch, hp, wp, C, d, shift, bias, out, oplane, opitch, Cp);
}

}  // namespace

struct sr_swinir_model : SwModelBase {
    sr_swinir_desc d{};
    static constexpr bool SHUFFLE_ONLY = false;
    static constexpr bool PROJECTED = false;
    static int check_desc(const char *who, const sr_swinir_desc *desc) { return sw_check_desc(who, desc); }
    static std::vector<SwTable> table_list(const sr_swinir_desc &desc) { return sw_tables(desc); }
    static bool bias_table(int kind) { return kind == SW_T_RPB; }
    int geometry(const char *who, int h, int w, int tail, SwGeom &g) const { return sw_geometry(who, d, h, w, tail, g); }
    std::vector<SwStep> tail_steps() const { return sw_tail_steps(d); }
};

static LiveSet g_sw_live;

static int sw_forward(sr_swinir_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride, int tail,
                      bool u8, const char *who)
{
    static const SwNames names{"swinir_head", "swinir_ln", "swinir_linear", "swinir_conv", "swinir_tail"};
    return sw_forward_frame(__func__, g_sw_live, m, names, k_sw_reflect<>, d_src, src_stride, h, w, d_dst, dst_stride, tail, u8, who,
                            [m](const SwTrunk &T, const SwGeom &, int &k) {       // one RSTB: D Swin layers, 7 tables each
        float *x = T.Rb;                                   // the first layer reads the RSTB's input and writes X
        for (int j = 0; j < m->d.depth; ++j, k += 7) {
            T.norm(x, k, T.Ab);
            T.qkv(k + 1);
            {
                ProfScope ps(T.ctx, "swinir_attention");
                sw_launch_attention(T.st, T.Qb, T.L.plane, T.L.pitch, T.hp, T.wp, T.C, m->d.n_heads, j % 2 ? SW_SHIFT : 0, m->w(k + 2), T.Ab,
                                    T.L.plane, T.L.pitch, T.Cp);
            }
            T.proj(k + 3, x);
            x = T.Xb;
            T.mlp(k + 4);
        }
        return x;
    });
}

extern "C" {

int sr_swinir_create(sr_ctx *ctx, const sr_swinir_desc *desc, const float *const *h_w, const float *const *h_b, int n_tables,
                     sr_swinir_model **out)
{
    return sw_create("sr_swinir_create", ctx, desc, h_w, h_b, n_tables, g_sw_live, out, [] { return SR_OK; },
                     [&](const SwTable &t, const float *w, const float *b, MfmaWeights &a) {
        if (t.kind == SW_T_RPB) a = {sw_gather_window_bias(w, SW_WIN, desc->n_heads), std::vector<float>(1, 0.0f)};
        else if (t.kind == SW_T_UPD) a = sw_arrange(w, b, t.cout, t.cin, 9, sw_pad64(desc->n_feat), 8, t.cout > 32 ? 64 : 32);
        else if (t.kind == SW_T_C64) a = sw_arrange(w, b, t.cout, t.cin, 9, SW_MID, 8, 64);
        else return false;
        return true;
    });
}

int sr_swinir_destroy(sr_swinir_model *m)
{
    return destroy_model(m, g_sw_live);
}

int sr_swinir_u8(sr_swinir_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride, int tail)
{
    return sw_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tail, true, "sr_swinir_u8");
}

int sr_swinir_f32(sr_swinir_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride, int tail)
{
    return sw_forward(model, d_src, src_stride, h, w, d_dst, dst_stride, tail, false, "sr_swinir_f32");
}

int sr_swinir_ens_u8(sr_swinir_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, uint8_t *d_dst, int64_t dst_stride,
                     int tail, int mask)
{
    return sw_ensemble(g_sw_live, model, sw_forward, d_src, src_stride, h, w, d_dst, dst_stride, tail, mask, true, "sr_swinir_ens_u8");
}

int sr_swinir_ens_f32(sr_swinir_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride,
                      int tail, int mask)
{
    return sw_ensemble(g_sw_live, model, sw_forward, d_src, src_stride, h, w, d_dst, dst_stride, tail, mask, false, "sr_swinir_ens_f32");
}

int sr_swinir_fill_workspace(sr_swinir_model *m, int h, int w, int tail, int byte)
{
    return sw_fill_workspace("sr_swinir_fill_workspace", g_sw_live, m, h, w, tail, byte);
}

int sr_swinir_layernorm_f32(sr_ctx *ctx, const float *d_x, int64_t plane_stride, int64_t row_stride, int n_feat, int h, int w,
                            const float *h_gamma, const float *h_beta, float *d_out, int64_t out_plane_stride, int64_t out_row_stride)
{
    const char *who = "sr_swinir_layernorm_f32";
    if (!d_x || !h_gamma || !h_beta || !d_out) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    const int C = n_feat;
    if (C < 1 || C > 256) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d channels is outside 1 <= C <= 256", who, C);
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_SHAPE, "%s: %dx%d image", who, w, h);
    int rc;
    if ((rc = sw_check_view(who, d_x, plane_stride, row_stride, h, w))) return rc;
    if ((rc = sw_check_view(who, d_out, out_plane_stride, out_row_stride, h, w))) return rc;
    CTX_ENTER(ctx);
    DevTemp tmp(ctx);
    SRCHK(tmp.alloc(who, 2 * (size_t)C * sizeof(float)));
    float *gm = tmp.as<float>(), *bt = gm + C;
    HIPCHK(hipMemcpyAsync(gm, h_gamma, C * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(bt, h_beta, C * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    sw_launch_layernorm(ctx->stream, d_x, plane_stride / 4, row_stride / 4, h, w, C, C, gm, bt, d_out, out_plane_stride / 4, out_row_stride / 4);
    SRCHK(check_launch(who));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_swinir_attention_f32(sr_ctx *ctx, const float *d_qkv, int64_t plane_stride, int64_t row_stride, int n_feat, int n_heads, int hp, int wp,
                            int shift, const float *h_table, float *d_out, int64_t out_plane_stride, int64_t out_row_stride)
{
    const char *who = "sr_swinir_attention_f32";
    int rc;
    if ((rc = sw_check_attention_args(who, d_qkv, h_table, d_out, n_feat, n_heads))) return rc;
    if (shift != 0 && shift != SW_SHIFT) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: shift %d (supported: 0, %d)", who, shift, SW_SHIFT);
    if ((rc = sw_check_windows(who, hp, wp, SW_WIN))) return rc;
    return sw_run_attention(who, ctx, d_qkv, plane_stride, row_stride, n_heads, hp, wp, h_table, SW_TOK, SW_TOK, d_out, out_plane_stride,
                            out_row_stride, [](int *idx) { sw_rel_index(SW_WIN, idx); return SR_OK; },
                            [&](hipStream_t st, const float *qkv, long long plane, int pitch, const float *bias, float *out, long long oplane, int opitch) {
        sw_launch_attention(st, qkv, plane, pitch, hp, wp, n_feat, n_heads, shift, bias, out, oplane, opitch, n_feat);
    });
}

}  // extern "C"
