// sr_ensemble.hip -- geometric self-ensemble of the local SR backends (the "+" results of the SR literature: Timofte et al.,
// Lim et al.): the network runs on the eight flips / rotations T_k of the input, every output is mapped back by T_k^-1 and the
// outputs are averaged.  The definition (transforms, member order, the fp32 sum and the fp32 division) is in include/sr_hip.h;
// the forwards themselves are the families' own (sr_srnet.hip, sr_resnet.hip, sr_rrdb.hip) and are not touched.
//
// Three bandwidth passes, HBM -> HBM:
//   k_d4<uint8_t>       T_k of the u8 input (input resolution)
//   k_d4<float, ADD>    acc = T_k^-1(y) for the first member, acc = acc + T_k^-1(y) after it (output resolution)
//   k_ens_finish        o = acc / n -> HWC fp32, or HWC u8 by the forwards' rule (store_hwc)
// T_k^-1 is itself a member of the group: T_5 and T_6 are each other's inverses, the other six are their own.  So one kernel,
// "dst = T_k(src)", serves both directions.
//
// k_d4: a block moves one TP x TP pixel tile through LDS.  A pixel is 3 elements (3 or 12 bytes), so the tile is addressed by
// ELEMENT: row a of the tile is 3 TP consecutive elements of a source row, read by consecutive lanes (full coalesced row
// segments) and stored to lds[a * PITCH + e].  The destination is then written row by row, again consecutive lanes on
// consecutive elements of a destination row; lane e = 3 c + ch fetches lds[a * PITCH + 3 b + ch] with (a, b) the source pixel of
// destination pixel (r, c).  Without a transpose a is fixed and b = +-c: consecutive LDS words.  With a transpose b is fixed and
// a = +-c, so the lanes stride by PITCH: fp32 uses PITCH = 3 TP + 3 = 99 words, PITCH = 3 (mod 32), which puts lane e on bank
// +-(3 c) + ch -- 32 distinct banks for the 32 lanes of a ds_read_b32 group, no conflict in either direction.  u8 uses
// PITCH = 196 bytes = 49 words (odd: the 11 pixel rows a 32-lane group touches fall on distinct banks).
// Every offset into an image is formed in 64 bits (size_t row * stride); only pixel indices inside a row are int.
#include <vector>

#include "sr_net_common.h"

namespace {

template <typename T> struct D4Tile;
template <> struct D4Tile<uint8_t> { static constexpr int TP = 64, PITCH = 196; };
template <> struct D4Tile<float> { static constexpr int TP = 32, PITCH = 99; };
constexpr int D4_THREADS = 192;           // 3 x 64 elements: one row of the u8 tile, two rows of the fp32 tile per pass

// dst = T_k(src), src h x w pixels; dst is w x h for k & 4.  ADD: dst = dst + T_k(src).
// T_k(x)[p][q] = x[fi(i)][fj(j)], (p, q) = k & 4 ? (j, i) : (i, j), fi = the vertical flip for k & 2, fj the horizontal one for
// k & 1.  Tiles are cut in (i, j); gridDim.y may be smaller than the number of tile rows.
template <typename T, bool ADD>
__global__ __launch_bounds__(D4_THREADS) void k_d4(const T *__restrict__ src, long long src_stride, int h, int w, int k, T *dst,
                                                   long long dst_stride, int tiles_y)
{
    constexpr int TP = D4Tile<T>::TP, PITCH = D4Tile<T>::PITCH, RW = TP * 3, RPP = D4_THREADS / RW;
    __shared__ T lds[TP * PITCH];
    const int e = threadIdx.x % RW, rr = threadIdx.x / RW, c = e / 3, ch = e - 3 * c;
    const int j0 = blockIdx.x * TP, tw = min(TP, w - j0);
    const bool fv = k & 2, fh = k & 1, tr = k & 4;
    const int pj0 = fh ? w - j0 - tw : j0;                       // first source column of the tile
    for (int ty = blockIdx.y; ty < tiles_y; ty += gridDim.y) {
        const int i0 = ty * TP, th = min(TP, h - i0);
        const int pi0 = fv ? h - i0 - th : i0;                   // first source row
        if (c < tw)
            for (int a = rr; a < th; a += RPP)
                lds[a * PITCH + e] = ((const T *)((const char *)src + (size_t)(pi0 + a) * src_stride))[(size_t)pj0 * 3 + e];
        __syncthreads();
        const int nrows = tr ? tw : th, ncols = tr ? th : tw, dr0 = tr ? j0 : i0, dc0 = tr ? i0 : j0;
        if (c < ncols)
            for (int r = rr; r < nrows; r += RPP) {
                const int il = tr ? c : r, jl = tr ? r : c;
                const int a = fv ? th - 1 - il : il, b = fh ? tw - 1 - jl : jl;
                T v = lds[a * PITCH + b * 3 + ch];
                T *d = (T *)((char *)dst + (size_t)(dr0 + r) * dst_stride) + ((size_t)dc0 * 3 + e);
                if constexpr (ADD) v = *d + v;
                *d = v;
            }
        __syncthreads();
    }
}

// o = acc / n (a correctly rounded fp32 division: the build has no fast-math and keeps HIP's default IEEE divide), stored by
// the forwards' rule.  One thread per element of a row, rows strided by gridDim.y.
template <bool U8>
__global__ __launch_bounds__(256) void k_ens_finish(const float *acc, long long acc_stride, int H, long long row_elems, float n,
                                                    void *dst, long long dst_stride)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= row_elems) return;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const float o = ((const float *)((const char *)acc + (size_t)y * acc_stride))[e] / n;
        store_hwc<U8>((char *)dst + (size_t)y * dst_stride, (size_t)e, o);
    }
}

constexpr int GRID_Y_MAX = 65535;

inline int d4_inverse(int k) { return k == 5 ? 6 : (k == 6 ? 5 : k); }

template <typename T, bool ADD>
void launch_d4(sr_ctx *ctx, const T *src, int64_t src_stride, int h, int w, int k, T *dst, int64_t dst_stride)
{
    constexpr int TP = D4Tile<T>::TP;
    const int tiles_y = (h + TP - 1) / TP;
    hipLaunchKernelGGL((k_d4<T, ADD>), dim3((w + TP - 1) / TP, std::min(tiles_y, GRID_Y_MAX)), dim3(D4_THREADS), 0, ctx->stream, src,
                       (long long)src_stride, h, w, k, dst, (long long)dst_stride, tiles_y);
}

// acc (H x W) = or += T_k^-1(y), y being H x W, or W x H for k & 4.
void launch_acc(sr_ctx *ctx, const float *y, int64_t y_stride, int H, int W, int k, bool first, float *acc, int64_t acc_stride)
{
    const int yh = (k & 4) ? W : H, yw = (k & 4) ? H : W;
    if (first) launch_d4<float, false>(ctx, y, y_stride, yh, yw, d4_inverse(k), acc, acc_stride);
    else launch_d4<float, true>(ctx, y, y_stride, yh, yw, d4_inverse(k), acc, acc_stride);
}

void launch_finish(sr_ctx *ctx, const float *acc, int64_t acc_stride, int H, int W, int n, void *dst, int64_t dst_stride, bool u8)
{
    const long long row = (long long)W * 3;
    const dim3 grid((unsigned)((row + 255) / 256), std::min(H, GRID_Y_MAX));
    if (u8) hipLaunchKernelGGL(k_ens_finish<true>, grid, dim3(256), 0, ctx->stream, acc, (long long)acc_stride, H, row, (float)n, dst, (long long)dst_stride);
    else hipLaunchKernelGGL(k_ens_finish<false>, grid, dim3(256), 0, ctx->stream, acc, (long long)acc_stride, H, row, (float)n, dst, (long long)dst_stride);
}

// One image argument: rows x row_bytes at stride; fp32: pointer and stride multiples of 4.
int check_image(const char *who, const char *what, const void *p, int64_t stride, long long row_bytes, bool f32)
{
    if (stride < row_bytes) return sr_set_error(SR_ERR_SHAPE, "%s: %s stride smaller than a row", who, what);
    if (f32 && stride % 4) return sr_set_error(SR_ERR_SHAPE, "%s: fp32 %s stride must be a multiple of 4 bytes", who, what);
    if (f32 && (uintptr_t)p % 4) return sr_set_error(SR_ERR_INVALID_ARG, "%s: fp32 %s pointer must be a multiple of 4 bytes", who, what);
    return SR_OK;
}

bool overlaps(const void *a, int64_t a_stride, long long a_rows, long long a_row_bytes, const void *b, int64_t b_stride, long long b_rows,
              long long b_row_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)((a_rows - 1) * a_stride + a_row_bytes);
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)((b_rows - 1) * b_stride + b_row_bytes);
    return a0 < b1 && b0 < a1;
}

int check_side(const char *who, int h, int w)
{
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_SHAPE, "%s: %dx%d image", who, w, h);
    if ((long long)w * 3 > INT_MAX || (long long)h * 3 > INT_MAX) return sr_set_error(SR_ERR_SHAPE, "%s: a %dx%d image overflows int", who, w, h);
    return SR_OK;
}

int finish_entry(const char *who, sr_ctx *ctx, const float *d_acc, int64_t acc_stride, int H, int W, int n, void *d_dst, int64_t dst_stride, bool u8)
{
    if (!d_acc || !d_dst) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    if (n < 1 || n > 8) return sr_set_error(SR_ERR_INVALID_ARG, "%s: n %d is outside 1..8", who, n);
    int rc = check_side(who, H, W);
    if (rc) return rc;
    if ((rc = check_image(who, "accumulator", d_acc, acc_stride, (long long)W * 12, true))) return rc;
    if ((rc = check_image(who, "destination", d_dst, dst_stride, (long long)W * (u8 ? 3 : 12), !u8))) return rc;
    CTX_ENTER(ctx);
    ProfScope ps(ctx, "ens_finish");
    launch_finish(ctx, d_acc, acc_stride, H, W, n, d_dst, dst_stride, u8);
    return check_launch(who);
}

}  // namespace

int ens_run(const char *who, SrModelBase &m, int scale, const EnsForward &fwd, const uint8_t *d_src, int64_t src_stride, int h, int w,
            void *d_dst, int64_t dst_stride, int mask, bool u8)
{
    sr_ctx *ctx = m.ctx;
    CTX_ENTER(ctx);
    if (!d_src || !d_dst) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    SrEnsLayout L;
    int rc = sr_ens_layout(who, h, w, scale, mask, &L);
    if (rc) return rc;
    if ((rc = check_image(who, "source", d_src, src_stride, (long long)w * 3, false))) return rc;
    if ((rc = check_image(who, "destination", d_dst, dst_stride, (long long)w * scale * (u8 ? 3 : 12), !u8))) return rc;
    if ((rc = ensure_activation_buffers(ctx, &m.ens_ws, 1, (L.total + 3) / 4, who))) return rc;
    char *ws = m.ens_ws.as<char>();
    float *acc = (float *)(ws + L.acc_off), *y = (float *)(ws + L.y_off);
    uint8_t *in = (uint8_t *)(ws + L.in_off);
    const int H = h * scale, W = w * scale;
    const int64_t acc_stride = sr_ens_row_stride((long long)W * 12);
    for (int i = 0; i < L.n; ++i) {
        const int k = L.members[i];
        const int hk = (k & 4) ? w : h, wk = (k & 4) ? h : w;
        const uint8_t *src_k = d_src;
        int64_t stride_k = src_stride;
        if (k != 0) {                                          // T_0 is the identity: the forward reads the caller's image
            ProfScope ps(ctx, "ens_d4");
            stride_k = sr_ens_row_stride((long long)wk * 3);
            launch_d4<uint8_t, false>(ctx, d_src, src_stride, h, w, k, in, stride_k);
            src_k = in;
        }
        const int64_t y_stride = sr_ens_row_stride((long long)wk * scale * 12);
        if ((rc = fwd(src_k, stride_k, hk, wk, y, y_stride))) return rc;
        ProfScope ps(ctx, "ens_acc");
        launch_acc(ctx, y, y_stride, H, W, k, i == 0, acc, acc_stride);
    }
    {
        ProfScope ps(ctx, "ens_finish");
        launch_finish(ctx, acc, acc_stride, H, W, L.n, d_dst, dst_stride, u8);
    }
    return check_launch(who);
}

extern "C" {

int sr_d4_u8(sr_ctx *ctx, const uint8_t *d_src, int64_t src_stride, int h, int w, int k, uint8_t *d_dst, int64_t dst_stride)
{
    const char *who = "sr_d4_u8";
    if (!d_src || !d_dst) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    if (k < 0 || k > 7) return sr_set_error(SR_ERR_INVALID_ARG, "%s: k %d is outside 0..7", who, k);
    int rc = check_side(who, h, w);
    if (rc) return rc;
    const int hd = (k & 4) ? w : h, wd = (k & 4) ? h : w;
    if ((rc = check_image(who, "source", d_src, src_stride, (long long)w * 3, false))) return rc;
    if ((rc = check_image(who, "destination", d_dst, dst_stride, (long long)wd * 3, false))) return rc;
    if (overlaps(d_src, src_stride, h, (long long)w * 3, d_dst, dst_stride, hd, (long long)wd * 3))
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: the destination overlaps the source", who);
    CTX_ENTER(ctx);
    ProfScope ps(ctx, "ens_d4");
    launch_d4<uint8_t, false>(ctx, d_src, src_stride, h, w, k, d_dst, dst_stride);
    return check_launch(who);
}

int sr_d4_acc_f32(sr_ctx *ctx, const float *d_y, int64_t y_stride, int H, int W, int k, int first, float *d_acc, int64_t acc_stride)
{
    const char *who = "sr_d4_acc_f32";
    if (!d_y || !d_acc) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    if (k < 0 || k > 7) return sr_set_error(SR_ERR_INVALID_ARG, "%s: k %d is outside 0..7", who, k);
    int rc = check_side(who, H, W);
    if (rc) return rc;
    const int yh = (k & 4) ? W : H, yw = (k & 4) ? H : W;
    if ((rc = check_image(who, "source", d_y, y_stride, (long long)yw * 12, true))) return rc;
    if ((rc = check_image(who, "accumulator", d_acc, acc_stride, (long long)W * 12, true))) return rc;
    if (overlaps(d_y, y_stride, yh, (long long)yw * 12, d_acc, acc_stride, H, (long long)W * 12))
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: the accumulator overlaps the source", who);
    CTX_ENTER(ctx);
    ProfScope ps(ctx, "ens_acc");
    launch_acc(ctx, d_y, y_stride, H, W, k, first != 0, d_acc, acc_stride);
    return check_launch(who);
}

int sr_ens_finish_f32(sr_ctx *ctx, const float *d_acc, int64_t acc_stride, int H, int W, int n, float *d_dst, int64_t dst_stride)
{
    return finish_entry("sr_ens_finish_f32", ctx, d_acc, acc_stride, H, W, n, d_dst, dst_stride, false);
}

int sr_ens_finish_u8(sr_ctx *ctx, const float *d_acc, int64_t acc_stride, int H, int W, int n, uint8_t *d_dst, int64_t dst_stride)
{
    return finish_entry("sr_ens_finish_u8", ctx, d_acc, acc_stride, H, W, n, d_dst, dst_stride, true);
}

}  // extern "C"
