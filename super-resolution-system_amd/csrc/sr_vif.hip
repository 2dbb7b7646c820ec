// sr_vif.hip -- VIF in the pixel domain over four scales (sr_vif_u8), MATLAB's vifp_mscale.  The definition is in
// include/sr_hip.h; sizes, launches, scratch layout and every shape refusal are sr_vif_host.cpp's (vif_plan).
//
// Two kernels, both a column march: a block of TX threads owns TX consecutive columns of a plane and one chunk of rows; each
// thread keeps the last N rows of its column (N = 17, 9, 5, 3 taps) in registers as float64, filters them vertically, puts the
// result into one of two LDS rows (selected by parity, so one barrier per row is enough) and the threads that own an output
// filter that row horizontally.  The filter is separable and every sum runs tap 0 .. N - 1 in the order written (the build
// has -ffp-contract=off): equal inputs give equal bits.
//   k_vif_stats<N, SRC, PX, TX>  the five windowed moments W*x, W*y, W*(x x), W*(y y), W*(x y) of a scale over its valid
//     region -- the three products are formed again for every row of the window, which is cheaper than three more windows of
//     registers --, then the per-sample functional (two log10) and the block's two sums through a fixed tree.
//   k_vif_down<N, SRC, PX, TX>   the planes of the next scale: the same march with the NEXT scale's window on x and y alone,
//     evaluated at even rows and even columns only.
//   SRC says what a plane is read from: the u8 image (the plane as it is, MATLAB's rounded luma, or the exact luma
//   X / 255000, read byte by byte: the crop is pointer arithmetic and has any residue), or a float64 plane in the scratch.
// 7 launches and 4 reductions per call; the per-scale sums come back with one copy each.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "sr_ctx.h"
#include "sr_device.h"
#include "sr_vif.h"

namespace {

enum { VS_PLANE = 0, VS_YROUND = 1, VS_Y = 2, VS_F64 = 3 };     // what a kernel instantiation reads

struct VifParams {
    int h, w;                   // the plane that is read
    int oh, ow;                 // k_vif_down: the plane that is written
    int step;                   // output rows per chunk
    double k[VIF_MAX_TAPS];     // the taps, 0 .. N - 1
};

__device__ __forceinline__ unsigned vif_x(const unsigned char *p)
{
    return 65481u * p[0] + 128553u * p[1] + 24966u * p[2] + 4080000u;    // = 255000 Y, <= 59 925 000
}

template <int SRC>
__device__ __forceinline__ double vif_load(const unsigned char *__restrict__ p)
{
    if constexpr (SRC == VS_PLANE) return (double)p[0];
    else if constexpr (SRC == VS_YROUND) return (double)((2u * vif_x(p) + 255000u) / 510000u);
    else if constexpr (SRC == VS_Y) return (double)vif_x(p) / 255000.0;
    else return *(const double *)p;
}

template <int SRC, int PX>
constexpr int vif_elem() { return SRC == VS_F64 ? (int)sizeof(double) : PX; }

// the block's TX pairs through a fixed tree; thread 0 stores the two sums
template <int TX>
__device__ __forceinline__ void vif_block_sum2(double *sd0, double *sd1, int t, double v0, double v1, double *__restrict__ out)
{
    __syncthreads();
    sd0[t] = v0;
    sd1[t] = v1;
    __syncthreads();
    for (int s = TX / 2; s > 0; s >>= 1) {
        if (t < s) {
            sd0[t] += sd0[t + s];
            sd1[t] += sd1[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[0] = sd0[0];
        out[1] = sd1[0];
    }
}

// one sample of vifp_mscale, the steps in MATLAB's order; sigma_nsq = 2
__device__ __forceinline__ void vif_sample(double mu1, double mu2, double exx, double eyy, double exy, double &num, double &den)
{
    double s1 = exx - mu1 * mu1, s2 = eyy - mu2 * mu2;
    const double s12 = exy - mu1 * mu2;
    if (s1 < 0.0) s1 = 0.0;
    if (s2 < 0.0) s2 = 0.0;
    double g = s12 / (s1 + 1e-10);
    double sv = s2 - g * s12;
    if (s1 < 1e-10) {
        g = 0.0;
        sv = s2;
        s1 = 0.0;
    }
    if (s2 < 1e-10) {
        g = 0.0;
        sv = 0.0;
    }
    if (g < 0.0) {
        sv = s2;
        g = 0.0;
    }
    if (sv <= 1e-10) sv = 1e-10;
    num += log10(1.0 + g * g * s1 / (sv + 2.0));
    den += log10(1.0 + s1 / 2.0);
}

template <int N, int SRC, int PX, int TX>
__global__ __launch_bounds__(TX) void k_vif_stats(const unsigned char *__restrict__ a, long long sa,
                                                  const unsigned char *__restrict__ b, long long sb, VifParams P,
                                                  double *__restrict__ part)
{
    constexpr int OUT = vif_stats_out(TX, N);
    __shared__ double F[2][5][TX];
    const int t = threadIdx.x;
    const int mh = P.h - (N - 1);                                        // map rows
    const int y0 = (int)blockIdx.x * P.step, y1 = min(y0 + P.step, mh);  // this chunk's map rows = its first input rows
    const int c = (int)blockIdx.y * OUT + t;                             // the column this thread filters vertically
    const bool in = c < P.w;
    const bool own = t < OUT && c <= P.w - N;                            // ... and the map column it produces
    const size_t coff = (size_t)(in ? c : 0) * vif_elem<SRC, PX>();
    const unsigned char *ca = a + coff, *cb = b + coff;
    double wx[N], wy[N];
#pragma unroll
    for (int i = 0; i < N; ++i) wx[i] = wy[i] = 0.0;
    double num = 0.0, den = 0.0;
    const int nrows = (y1 - y0) + (N - 1);                               // input rows y0 .. y1 + N - 2 (< h)
    double nx = 0.0, ny = 0.0;
    if (in) {
        nx = vif_load<SRC>(ca + (size_t)y0 * (size_t)sa);
        ny = vif_load<SRC>(cb + (size_t)y0 * (size_t)sb);
    }
#pragma unroll 1
    for (int lr = 0; lr < nrows; ++lr) {
#pragma unroll
        for (int i = 0; i < N - 1; ++i) {
            wx[i] = wx[i + 1];
            wy[i] = wy[i + 1];
        }
        wx[N - 1] = nx;
        wy[N - 1] = ny;
        if (in) {   // the next row is requested before this one is worked on (the last iteration reads its own row again)
            const size_t sy = (size_t)(y0 + min(lr + 1, nrows - 1));
            nx = vif_load<SRC>(ca + sy * (size_t)sa);
            ny = vif_load<SRC>(cb + sy * (size_t)sb);
        }
        if (lr < N - 1) continue;                                        // block-uniform
        const int pb = lr & 1;
        {
            double v0 = wx[0] * P.k[0], v1 = wy[0] * P.k[0], v2 = (wx[0] * wx[0]) * P.k[0], v3 = (wy[0] * wy[0]) * P.k[0],
                   v4 = (wx[0] * wy[0]) * P.k[0];
#pragma unroll
            for (int i = 1; i < N; ++i) {
                const double k = P.k[i];
                v0 = fma(wx[i], k, v0);
                v1 = fma(wy[i], k, v1);
                v2 = fma(wx[i] * wx[i], k, v2);
                v3 = fma(wy[i] * wy[i], k, v3);
                v4 = fma(wx[i] * wy[i], k, v4);
            }
            F[pb][0][t] = v0; F[pb][1][t] = v1; F[pb][2][t] = v2; F[pb][3][t] = v3; F[pb][4][t] = v4;
        }
        __syncthreads();
        if (!own) continue;
        double u[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            double acc = F[pb][m][t] * P.k[0];
#pragma unroll
            for (int j = 1; j < N; ++j) acc = fma(F[pb][m][t + j], P.k[j], acc);
            u[m] = acc;
        }
        vif_sample(u[0], u[1], u[2], u[3], u[4], num, den);
    }
    // columns that produce nothing add 0
    vif_block_sum2<TX>(&F[0][0][0], &F[0][1][0], t, num, den, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2);
}

template <int N, int SRC, int PX, int TX>
__global__ __launch_bounds__(TX) void k_vif_down(const unsigned char *__restrict__ a, long long sa,
                                                 const unsigned char *__restrict__ b, long long sb, VifParams P,
                                                 double *__restrict__ ox, double *__restrict__ oy)
{
    constexpr int DOUT = vif_down_out(TX, N);
    __shared__ double F[2][2][TX];
    const int t = threadIdx.x;
    const int o0 = (int)blockIdx.x * P.step, o1 = min(o0 + P.step, P.oh);   // this chunk's output rows; input rows from 2 o0
    const int c = (int)blockIdx.y * (2 * DOUT) + t;                      // the input column this thread filters vertically
    const bool in = c < P.w;
    const int oc = (int)blockIdx.y * DOUT + t;                           // the output column it produces (input column 2 oc)
    const bool own = t < DOUT && oc < P.ow;
    const size_t coff = (size_t)(in ? c : 0) * vif_elem<SRC, PX>();
    const unsigned char *ca = a + coff, *cb = b + coff;
    double wx[N], wy[N];
#pragma unroll
    for (int i = 0; i < N; ++i) wx[i] = wy[i] = 0.0;
    const int r0 = 2 * o0, nrows = 2 * (o1 - o0 - 1) + N;                // input rows r0 .. r0 + nrows - 1 (< h)
    double nx = 0.0, ny = 0.0;
    if (in) {
        nx = vif_load<SRC>(ca + (size_t)r0 * (size_t)sa);
        ny = vif_load<SRC>(cb + (size_t)r0 * (size_t)sb);
    }
#pragma unroll 1
    for (int lr = 0; lr < nrows; ++lr) {
#pragma unroll
        for (int i = 0; i < N - 1; ++i) {
            wx[i] = wx[i + 1];
            wy[i] = wy[i + 1];
        }
        wx[N - 1] = nx;
        wy[N - 1] = ny;
        if (in) {
            const size_t sy = (size_t)(r0 + min(lr + 1, nrows - 1));
            nx = vif_load<SRC>(ca + sy * (size_t)sa);
            ny = vif_load<SRC>(cb + sy * (size_t)sb);
        }
        const int e = lr - (N - 1);                                      // the window's first row, from r0
        if (e < 0 || (e & 1)) continue;                                  // block-uniform: every second row is kept
        const int orow = e >> 1, pb = orow & 1;
        {
            double v0 = wx[0] * P.k[0], v1 = wy[0] * P.k[0];
#pragma unroll
            for (int i = 1; i < N; ++i) {
                v0 = fma(wx[i], P.k[i], v0);
                v1 = fma(wy[i], P.k[i], v1);
            }
            F[pb][0][t] = v0;
            F[pb][1][t] = v1;
        }
        __syncthreads();
        if (!own) continue;
        double u0 = F[pb][0][2 * t] * P.k[0], u1 = F[pb][1][2 * t] * P.k[0];
#pragma unroll
        for (int j = 1; j < N; ++j) {
            u0 = fma(F[pb][0][2 * t + j], P.k[j], u0);
            u1 = fma(F[pb][1][2 * t + j], P.k[j], u1);
        }
        const size_t o = (size_t)(o0 + orow) * (size_t)P.ow + (size_t)oc;
        ox[o] = u0;
        oy[o] = u1;
    }
}

template <int N, int SRC, int PX, int TX>
void launch_stats(sr_ctx *ctx, const VifLaunch &l, const void *a, long long sa, const void *b, long long sb, const VifParams &P,
                  double *part)
{
    hipLaunchKernelGGL((k_vif_stats<N, SRC, PX, TX>), dim3((unsigned)l.gx, (unsigned)l.gy), dim3(TX), 0, ctx->stream,
                       (const unsigned char *)a, sa, (const unsigned char *)b, sb, P, part);
}

template <int N, int SRC, int PX, int TX>
void launch_down(sr_ctx *ctx, const VifLaunch &l, const void *a, long long sa, const void *b, long long sb, const VifParams &P,
                 double *ox, double *oy)
{
    hipLaunchKernelGGL((k_vif_down<N, SRC, PX, TX>), dim3((unsigned)l.gx, (unsigned)l.gy), dim3(TX), 0, ctx->stream,
                       (const unsigned char *)a, sa, (const unsigned char *)b, sb, P, ox, oy);
}

// the parameters of a launch that filters with the window of scale s (0-based)
VifParams make_params(const VifScale &in, const VifScale *out, int s, int step)
{
    VifParams P;
    memset(&P, 0, sizeof(P));
    P.h = in.h;
    P.w = in.w;
    if (out) {
        P.oh = out->h;
        P.ow = out->w;
    }
    P.step = step;
    vif_window(s, P.k);
    return P;
}

}  // namespace

extern "C" int sr_vif_u8(sr_ctx *ctx, const uint8_t *d_ref, int64_t stride_ref, const uint8_t *d_dist, int64_t stride_dist, int h,
                         int w, int cn, int crop_border, int mode, sr_vif_scale *h_out)
{
    // every argument check comes before the context (and so the device) is touched
    if (!d_ref || !d_dist || !h_out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_vif_u8: null argument");
    VifPlan p;
    int rc = vif_plan("sr_vif_u8", h, w, cn, crop_border, mode, &p);
    if (rc) return rc;
    const int64_t min_stride = (int64_t)w * cn;
    if (stride_ref < min_stride || stride_dist < min_stride)
        return sr_set_error(SR_ERR_SHAPE, "sr_vif_u8: stride smaller than a row");
    CTX_ENTER(ctx);
    SRCHK(ctx->vif_ws.reserve(ctx, "sr_vif_u8", p.total));
    char *ws = ctx->vif_ws.as<char>();
    double *part = (double *)(ws + p.off_part), *buf0 = (double *)(ws + p.off_buf0), *buf1 = (double *)(ws + p.off_buf1);
    // the crop: rows [cb, h - cb), columns [cb, w - cb) of both images
    const unsigned char *a = d_ref + (size_t)crop_border * (size_t)stride_ref + (size_t)crop_border * (size_t)cn;
    const unsigned char *b = d_dist + (size_t)crop_border * (size_t)stride_dist + (size_t)crop_border * (size_t)cn;
    const long long sa = stride_ref, sb = stride_dist;
    double h_res[VIF_SCALES][2];
    {
        ProfScope ps(ctx, "vif");
        static const char *const scale_names[VIF_SCALES] = {"vif_scale1", "vif_scale2", "vif_scale3", "vif_scale4"};
        for (int s = 0; s < VIF_SCALES; ++s) {
            const VifScale &v = p.s[s];
            ProfScope pss(ctx, scale_names[s]);        // the scale's planes, sums and reduction
            if (s == 1) {          // scale 2's planes from the u8 images
                const VifParams P = make_params(p.s[0], &v, s, v.down.step);
                double *ox = (double *)(ws + v.off_x), *oy = (double *)(ws + v.off_y);
                if (mode == SR_BENCH_Y) launch_down<9, VS_Y, 3, VIF_TX_U8>(ctx, v.down, a, sa, b, sb, P, ox, oy);
                else if (mode == SR_BENCH_Y_ROUND) launch_down<9, VS_YROUND, 3, VIF_TX_U8>(ctx, v.down, a, sa, b, sb, P, ox, oy);
                else launch_down<9, VS_PLANE, 1, VIF_TX_U8>(ctx, v.down, a, sa, b, sb, P, ox, oy);
            } else if (s > 1) {    // the next planes from the float64 planes before
                const VifScale &u = p.s[s - 1];
                const VifParams P = make_params(u, &v, s, v.down.step);
                const long long su = (long long)u.w * (long long)sizeof(double);
                double *ox = (double *)(ws + v.off_x), *oy = (double *)(ws + v.off_y);
                if (s == 2) launch_down<5, VS_F64, 1, VIF_TX_F64>(ctx, v.down, ws + u.off_x, su, ws + u.off_y, su, P, ox, oy);
                else launch_down<3, VS_F64, 1, VIF_TX_F64>(ctx, v.down, ws + u.off_x, su, ws + u.off_y, su, P, ox, oy);
            }
            const VifParams P = make_params(v, nullptr, s, v.stats.step);
            if (s == 0) {
                if (mode == SR_BENCH_Y) launch_stats<17, VS_Y, 3, VIF_TX_U8>(ctx, v.stats, a, sa, b, sb, P, part);
                else if (mode == SR_BENCH_Y_ROUND) launch_stats<17, VS_YROUND, 3, VIF_TX_U8>(ctx, v.stats, a, sa, b, sb, P, part);
                else launch_stats<17, VS_PLANE, 1, VIF_TX_U8>(ctx, v.stats, a, sa, b, sb, P, part);
            } else {
                const long long sv = (long long)v.w * (long long)sizeof(double);
                const char *px = ws + v.off_x, *py = ws + v.off_y;
                if (s == 1) launch_stats<9, VS_F64, 1, VIF_TX_F64>(ctx, v.stats, px, sv, py, sv, P, part);
                else if (s == 2) launch_stats<5, VS_F64, 1, VIF_TX_F64>(ctx, v.stats, px, sv, py, sv, P, part);
                else launch_stats<3, VS_F64, 1, VIF_TX_F64>(ctx, v.stats, px, sv, py, sv, P, part);
            }
            const double *sums = reduce_partials(ctx, part, (long long)v.stats.gx * v.stats.gy, 2, buf0, buf1);
            rc = check_launch("vif");
            if (rc) return rc;
            // in stream order: the copy is done before the next scale writes the partials again
            HIPCHK(hipMemcpyAsync(h_res[s], sums, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    HIPCHK(stream_sync(ctx));
    for (int s = 0; s < VIF_SCALES; ++s) {
        h_out[s].num = h_res[s][0];
        h_out[s].den = h_res[s][1];
        h_out[s].count = p.s[s].count;
    }
    return SR_OK;
}
