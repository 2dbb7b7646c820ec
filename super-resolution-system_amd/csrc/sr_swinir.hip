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
// The head, the LayerNorm, the linear layers, the 3 x 3 convolutions (k_sw_head, k_sw_layernorm, k_sw_lin, k_sw_conv) and the
// weight arrangement are sr_swin_common.h, shared with sr_hat.hip; this file keeps the reflection, the window attention, the
// model and the forward.
//
// Weights are caller-supplied (sr_swinir_create); nothing is fetched.
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_net_common.h"
#include "sr_swin_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// Symmetric reflection of the u8 image to Hp x Wp (dense, 3 Wp bytes per row): padded index i reads m = i mod 2 n,
// m < n ? m : 2 n - 1 - m (np.pad mode 'symmetric': the edge pixel repeated, period 2 n).  One thread per output byte.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sw_reflect(const unsigned char *__restrict__ img, long long stride, int h, int w,
                                                    unsigned char *__restrict__ out, int hp, int wp)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)hp * wp * 3) return;
    const int c = (int)(i % 3), x = (int)((i / 3) % wp), y = (int)(i / (3LL * wp));
    int my = y % (2 * h), mx = x % (2 * w);
    if (my >= h) my = 2 * h - 1 - my;
    if (mx >= w) mx = 2 * w - 1 - mx;
    out[i] = img[(size_t)my * stride + (size_t)mx * 3 + c];
}

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
    const dim3 grid((hp / SW_WIN) * (wp / SW_WIN), heads), block(SW_TOK);
    if (d <= 8) hipLaunchKernelGGL(k_sw_attention<8>, grid, block, 0, st, qkv, plane, pitch, hp, wp, C, d, shift, bias, out, oplane, opitch, Cp);
    else if (d <= 16) hipLaunchKernelGGL(k_sw_attention<16>, grid, block, 0, st, qkv, plane, pitch, hp, wp, C, d, shift, bias, out, oplane, opitch, Cp);
    else if (d <= 24) hipLaunchKernelGGL(k_sw_attention<24>, grid, block, 0, st, qkv, plane, pitch, hp, wp, C, d, shift, bias, out, oplane, opitch, Cp);
    else hipLaunchKernelGGL(k_sw_attention<32>, grid, block, 0, st, qkv, plane, pitch, hp, wp, C, d, shift, bias, out, oplane, opitch, Cp);
}

// The bias table [225][heads] gathered to [head][key j][query i].
std::vector<float> sw_gather_bias(const float *table, int heads)
{
    std::vector<int> rel(SW_TOK * SW_TOK);
    sw_rel_index(rel.data());
    std::vector<float> g((size_t)heads * SW_TOK * SW_TOK);
    for (int hd = 0; hd < heads; ++hd)
        for (int j = 0; j < SW_TOK; ++j)
            for (int i = 0; i < SW_TOK; ++i) g[((size_t)hd * SW_TOK + j) * SW_TOK + i] = table[(size_t)rel[i * SW_TOK + j] * heads + hd];
    return g;
}

}  // namespace

struct sr_swinir_model : SrModelBase {         // d_w, d_b: per table (sw_tables)
    sr_swinir_desc d{};
    std::vector<SwTable> tables;
    DevBuf trunk[4];                          // H, R, X, A
    DevBuf qbuf;                              // qkv / hidden
    DevBuf tailbuf[2];
    DevBuf img;                               // the reflected u8 image
    void release_device()
    {
        for (auto &b : trunk) b.release();
        for (DevBuf *b : {&tailbuf[0], &tailbuf[1], &qbuf, &img}) b->release();
        release_base();
    }
};

static LiveSet g_sw_live;

static int sw_reserve(sr_swinir_model *m, const SwGeom &g, const char *who)
{
    sr_ctx *ctx = m->ctx;
    int rc;
    if ((rc = ensure_activation_buffers(ctx, m->trunk, 4, (size_t)g.plane0 * g.cp, who))) return rc;
    if ((rc = ensure_activation_buffers(ctx, &m->qbuf, 1, (size_t)g.plane0 * g.qp, who))) return rc;
    if (g.plane_t && (rc = ensure_activation_buffers(ctx, m->tailbuf, 2, (size_t)g.plane_t * SW_MID, who))) return rc;
    SRCHK(m->img.reserve(ctx, who, (size_t)g.plane0 * 3));
    return SR_OK;
}

static int sw_forward(sr_swinir_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride, int tail,
                      bool u8, const char *who)
{
    if (!g_sw_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    sr_ctx *ctx = m->ctx;
    CTX_ENTER(ctx);
    const sr_swinir_desc &D = m->d;
    const int C = D.n_feat, heads = D.n_heads, S = D.scale;
    int rc = check_sr_forward_args(who, d_src, src_stride, w, d_dst, dst_stride, S, u8);
    if (rc) return rc;
    SwGeom g;
    if ((rc = sw_geometry(who, D, h, w, tail, g))) return rc;
    if ((rc = sw_reserve(m, g, who))) return rc;
    const int hp = g.hp, wp = g.wp, Cp = g.cp, hidp = sw_pad64(D.n_hidden), qkvp = sw_pad64(3 * C);
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
    float *Qb = m->qbuf.as<float>();
    unsigned char *img = m->img.as<unsigned char>();
    auto lin = [&](auto kernel, float *in, int cin, int k, int cout_planes, float *out, const float *skip) {
        ProfScope ps(ctx, "swinir_linear");
        SwEpi e = ep;
        e.skip = skip;
        launch_conv(kernel, st, ten(in), hp, wp, cin, cout_planes / 64, m->w(k), m->b(k), out, L.plane, L.pitch, 0, 0, hp, wp, e);
    };
    auto conv = [&](float *in, int k, float *out, const float *skip) {
        ProfScope ps(ctx, "swinir_conv");
        SwEpi e = ep;
        e.skip = skip;
        launch_conv(k_sw_conv<2, SW_ADD>, st, ten(in), hp, wp, Cp, Cp / 64, m->w(k), m->b(k), out, L.plane, L.pitch, 0, 0, hp, wp, e);
    };
    auto norm = [&](float *in, int k, float *out) {
        ProfScope ps(ctx, "swinir_ln");
        sw_launch_layernorm(st, in, L.plane, L.pitch, hp, wp, C, Cp, m->w(k), m->b(k), out, L.plane, L.pitch);
    };
    {
        ProfScope ps(ctx, "swinir_head");
        const long long n = (long long)g.plane0 * 3;
        hipLaunchKernelGGL(k_sw_reflect, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_src, (long long)src_stride, h, w, img, hp, wp);
        hipLaunchKernelGGL(k_sw_head, dim3((wp + 63) / 64, (hp + 3) / 4, Cp / 64), dim3(64, 4), 0, st, img, (long long)wp * 3, hp, wp, m->w(0), m->b(0),
                           ep.af, Hb, hp, wp, L.pitch, L.plane);
    }
    int k = 1;
    norm(Hb, k++, Rb);
    for (int gi = 0; gi < D.n_groups; ++gi) {
        float *x = Rb;                                     // the first layer reads the RSTB's input and writes X
        for (int j = 0; j < D.depth; ++j, k += 7) {
            norm(x, k, Ab);
            lin(k_sw_lin<SL_QKV>, Ab, Cp, k + 1, qkvp, Qb, nullptr);
            {
                ProfScope ps(ctx, "swinir_attention");
                sw_launch_attention(st, Qb, L.plane, L.pitch, hp, wp, C, heads, j % 2 ? SW_SHIFT : 0, m->w(k + 2), Ab, L.plane, L.pitch, Cp);
            }
            lin(k_sw_lin<SL_ADD>, Ab, Cp, k + 3, Cp, Xb, x);
            x = Xb;
            norm(x, k + 4, Ab);
            lin(k_sw_lin<SL_GELU>, Ab, Cp, k + 5, hidp, Qb, nullptr);
            lin(k_sw_lin<SL_ADD>, Qb, hidp, k + 6, Cp, Xb, Xb);
        }
        conv(x, k++, Rb, Rb);                              // in place over the RSTB's input
    }
    norm(Rb, k++, Ab);
    conv(Ab, k++, Hb, Hb);                                 // f = conv_after_body(.) + h, in place over h
    if ((rc = check_launch(who))) return rc;
    // ---- tail phase: sub-pieces of the input over their own backward extents ----
    const std::vector<SwStep> steps = sw_tail_steps(D);
    const int n = (int)steps.size();
    const PlanarTen f = ten(Hb);
    std::vector<int> ya, yb, xa, xb;
    for (int sy = 0; sy < h; sy = (int)std::min<long long>((long long)sy + g.tail, h))
        for (int sx = 0; sx < w; sx = (int)std::min<long long>((long long)sx + g.tail, w)) {
            sw_backward_extents(steps.data(), n, S, sy, (int)std::min<long long>((long long)sy + g.tail, h), hp, ya, yb);
            sw_backward_extents(steps.data(), n, S, sx, (int)std::min<long long>((long long)sx + g.tail, w), wp, xa, xb);
            PlanarTen t = f;
            ProfScope ps(ctx, "swinir_tail");
            for (int i = 0; i < n; ++i) {
                const int rows = yb[i] - ya[i], cols = xb[i] - xa[i], mult = steps[i].mult, r = steps[i].r, kt = k + i;
                const int kind = m->tables[kt].kind, cin = i == 0 ? Cp : SW_MID;
                SwEpi e = ep;
                e.slope = kind == SW_T_CBU ? 0.01f : 0.2f;
                e.s = r;
                if (i + 1 < n) {
                    const PlanarTen o = planar_tensor(m->tailbuf[i & 1].as<float>(), ya[i] * r, xa[i] * r, rows * r, cols * r);
                    auto go = [&](auto kernel, int tiles) {
                        launch_conv(kernel, st, t, hp * mult, wp * mult, cin, tiles, m->w(kt), m->b(kt), o.p, o.plane, o.pitch, ya[i], xa[i], rows, cols, e);
                    };
                    if (kind == SW_T_UP && r == 2) go(k_sw_conv<2, SW_SHUF2>, 4);
                    else if (kind == SW_T_UP) go(k_sw_conv<2, SW_SHUF3>, 9);
                    else if (r == 2) go(k_sw_conv<2, SW_REP_ACT>, 1);
                    else go(k_sw_conv<2, SW_ACT>, 1);
                    t = o;
                } else {
                    auto go = [&](auto kernel) {
                        launch_conv(kernel, st, t, hp * mult, wp * mult, cin, 1, m->w(kt), m->b(kt), nullptr, 0LL, 0, ya[i], xa[i], rows, cols, e);
                    };
                    const bool wide = 3 * r * r > 32;
                    if (u8) wide ? go(k_sw_conv<2, SW_LAST_U8>) : go(k_sw_conv<1, SW_LAST_U8>);
                    else wide ? go(k_sw_conv<2, SW_LAST_F32>) : go(k_sw_conv<1, SW_LAST_F32>);
                }
            }
            if ((rc = check_launch(who))) return rc;
        }
    return SR_OK;
}

// The self-ensemble over sw_forward (driver: sr_ensemble.hip): every member is padded and windowed on its own.
static int sw_ensemble(sr_swinir_model *m, const uint8_t *d_src, int64_t src_stride, int h, int w, void *d_dst, int64_t dst_stride, int tail,
                       int mask, bool u8, const char *who)
{
    const int rc = sr_ens_check_mask(who, mask);
    if (rc) return rc;
    if (tail < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: %s must be >= 1, or 0 for the library's choice", who, "tail");
    if (!g_sw_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    return ens_run(who, *m, m->d.scale, [&](const uint8_t *s, int64_t ss, int hh, int ww, float *d, int64_t ds) {
        return sw_forward(m, s, ss, hh, ww, d, ds, tail, false, who);
    }, d_src, src_stride, h, w, d_dst, dst_stride, mask, u8);
}

extern "C" {

int sr_swinir_create(sr_ctx *ctx, const sr_swinir_desc *desc, const float *const *h_w, const float *const *h_b, int n_tables,
                     sr_swinir_model **out)
{
    const char *who = "sr_swinir_create";
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null out", who);
    *out = nullptr;
    int rc = sw_check_desc(who, desc);                                      // host decision, before any device call
    if (rc) return rc;
    const std::vector<SwTable> tables = sw_tables(*desc);
    if (!h_w || !h_b) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null weight table", who);
    if (n_tables != (int)tables.size())
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: this description has %d tables, %d given", who, (int)tables.size(), n_tables);
    for (int k = 0; k < n_tables; ++k)
        if (!h_w[k] || (!h_b[k] && tables[k].kind != SW_T_RPB)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null array of table %d", who, k);
    CTX_ENTER(ctx);
    sr_swinir_model *M = new sr_swinir_model();
    M->ctx = ctx;
    M->d = *desc;
    M->tables = tables;
    g_sw_live.insert(M);
    const int C = desc->n_feat, Cp = sw_pad64(C), hidp = sw_pad64(desc->n_hidden);
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
            a = {sw_gather_bias(h_w[k], desc->n_heads), std::vector<float>(1, 0.0f)};
            break;
        case SW_T_QKV: case SW_T_PROJ: case SW_T_FC1:
            a = sw_arrange(h_w[k], h_b[k], t.cout, t.cin, 1, Cp, SW_LIN_CC, 64);
            break;
        case SW_T_FC2:
            a = sw_arrange(h_w[k], h_b[k], t.cout, t.cin, 1, hidp, SW_LIN_CC, 64);
            break;
        case SW_T_CONV: case SW_T_CBU:
            a = sw_arrange(h_w[k], h_b[k], t.cout, t.cin, 9, Cp, 8, 64);
            break;
        case SW_T_UPD:
            a = sw_arrange(h_w[k], h_b[k], t.cout, t.cin, 9, Cp, 8, t.cout > 32 ? 64 : 32);
            break;
        case SW_T_LAST:
            a = sw_arrange(h_w[k], h_b[k], t.cout, t.cin, 9, SW_MID, 8, 32);
            break;
        default:                                                            // SW_T_UP, SW_T_C64
            a = sw_arrange(h_w[k], h_b[k], t.cout, t.cin, 9, SW_MID, 8, 64);
        }
        if ((rc = upload_conv(who, *M, a))) {
            sr_swinir_destroy(M);
            return rc;
        }
    }
    *out = M;
    return SR_OK;
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
    return sw_ensemble(model, d_src, src_stride, h, w, d_dst, dst_stride, tail, mask, true, "sr_swinir_ens_u8");
}

int sr_swinir_ens_f32(sr_swinir_model *model, const uint8_t *d_src, int64_t src_stride, int h, int w, float *d_dst, int64_t dst_stride,
                      int tail, int mask)
{
    return sw_ensemble(model, d_src, src_stride, h, w, d_dst, dst_stride, tail, mask, false, "sr_swinir_ens_f32");
}

int sr_swinir_fill_workspace(sr_swinir_model *m, int h, int w, int tail, int byte)
{
    const char *who = "sr_swinir_fill_workspace";
    if (!g_sw_live.contains(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed model", who);
    sr_ctx *ctx = m->ctx;
    CTX_ENTER(ctx);
    SwGeom g;
    int rc = sw_geometry(who, m->d, h, w, tail, g);
    if (rc) return rc;
    if ((rc = sw_reserve(m, g, who))) return rc;
    for (DevBuf *b : {&m->trunk[0], &m->trunk[1], &m->trunk[2], &m->trunk[3], &m->qbuf, &m->tailbuf[0], &m->tailbuf[1], &m->img})
        if (b->d) HIPCHK(hipMemsetAsync(b->d, byte, b->cap, ctx->stream));
    return SR_OK;
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
    if (!d_qkv || !h_table || !d_out) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    const int C = n_feat;
    if (C < 1 || C > 256 || n_heads < 1 || C % n_heads || C / n_heads > 32)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d channels in %d heads is outside C <= 256, heads of at most 32 channels", who, C, n_heads);
    if (shift != 0 && shift != SW_SHIFT) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: shift %d (supported: 0, %d)", who, shift, SW_SHIFT);
    if (hp < SW_WIN || wp < SW_WIN || hp % SW_WIN || wp % SW_WIN)
        return sr_set_error(SR_ERR_SHAPE, "%s: a %dx%d tensor is not made of %d x %d windows", who, wp, hp, SW_WIN, SW_WIN);
    int rc;
    if ((rc = sw_check_view(who, d_qkv, plane_stride, row_stride, hp, wp))) return rc;
    if ((rc = sw_check_view(who, d_out, out_plane_stride, out_row_stride, hp, wp))) return rc;
    CTX_ENTER(ctx);
    const std::vector<float> g = sw_gather_bias(h_table, n_heads);
    DevTemp tmp(ctx);
    SRCHK(tmp.alloc(who, g.size() * sizeof(float)));
    HIPCHK(hipMemcpyAsync(tmp.d, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    sw_launch_attention(ctx->stream, d_qkv, plane_stride / 4, (int)(row_stride / 4), hp, wp, C, n_heads, shift, tmp.as<float>(), d_out,
                        out_plane_stride / 4, (int)(out_row_stride / 4), C);
    SRCHK(check_launch(who));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

}  // extern "C"
