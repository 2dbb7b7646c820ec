// sr_fsim.hip -- FSIM / FSIMc of two u8 images (sr_fsim_u8), with the inspection entries sr_fsim_pool_u8 and sr_fsim_pc_f64.
// The definition is in include/sr_hip.h; F, the sizes, the workspace layout, the filter planes with EM_n / S2 / Sij, the
// twiddle tables and every shape refusal are sr_fsim_host.cpp's.
//
//   k_fsim_pool<CN>   the one pass over the images.  A block owns one pooled row and a segment of FSIM_POOL_THREADS source
//                     columns, which holds floor(256 / F) whole windows: thread t walks down the F source rows of its column
//                     (adjacent lanes read adjacent pixels) and keeps the six column sums Y, I, Q x 2 images as int32
//                     (< 2^31: F <= 256), LDS takes them, and one thread per (plane, window) adds its F columns in int64.
//                     Window = stride, so no source byte is read twice.
//   k_fsim_dft_cols / k_fsim_dft_rows
//                     the float64 2-D DFT as two dense passes, each a complex matrix product against the twiddle table
//                     tw[(index product) mod length]: 16 x 16 outputs per block, 16 products per step through LDS, every
//                     output's products added in ascending index order with fma -- a plain FMA loop, not the MFMA form.  The
//                     inverse conjugates the table.  The filtered form of the column pass multiplies the spectrum by
//                     spread_o once and by the four logGabor_s on the way into four accumulators: one read of the spectrum
//                     makes the four scales' planes of an orientation.
//   k_fsim_energy     per sample of one orientation: sumE, sumO, sumAn, Energy, |EO_0|^2 (the median's key), AnAll.
//   k_fsim_hist / k_fsim_select
//                     the exact median: an 8-pass radix select over the bit patterns of the non-negative float64 keys
//                     (monotone as uint64), integer histograms in LDS and global memory, both middle ranks at once; the last
//                     select forms the median and the threshold T on the device, so an orientation needs no host round trip.
//   k_fsim_clamp      EnergyAll += max(Energy - T, 0); the last orientation divides by AnAll.
//   k_fsim_score      Scharr on the pooled integer sums, the similarity maps and the three sums through a fixed tree;
//                     reduce_partials finishes them: no floating-point atomics, equal inputs give equal bits.
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_ctx.h"
#include "sr_fsim.h"

namespace {

typedef double2 cpx;
constexpr int DT = FSIM_DFT_TILE;

struct SelectState {
    unsigned long long prefix[2];
    unsigned rank[2];
};

// ---- pooling -----------------------------------------------------------------------------------------------------------------
template <int CN>
__global__ __launch_bounds__(FSIM_POOL_THREADS) void k_fsim_pool(const unsigned char *__restrict__ a, long long sa,
                                                                 const unsigned char *__restrict__ b, long long sb, int h, int w,
                                                                 int F, int cols, size_t n, long long *__restrict__ out)
{
    __shared__ int col[6][FSIM_POOL_THREADS];
    const int t = threadIdx.x;
    const int nout = FSIM_POOL_THREADS / F;
    const int j0 = (int)blockIdx.x * nout, i = (int)blockIdx.y;
    const long long x = fsim_win_start(j0, F) + t, ys = fsim_win_start(i, F);
    int acc[6] = {0, 0, 0, 0, 0, 0};
    if (t < nout * F && x >= 0 && x < w) {
        const long long y0 = ys < 0 ? 0 : ys, y1 = ys + F < h ? ys + F : h;
        for (long long y = y0; y < y1; ++y) {
            const unsigned char *pa = a + (size_t)y * (size_t)sa + (size_t)x * CN;
            const unsigned char *pb = b + (size_t)y * (size_t)sb + (size_t)x * CN;
            if constexpr (CN == 1) {
                acc[0] += 1000 * (int)pa[0];
                acc[3] += 1000 * (int)pb[0];
            } else {
                const int r1 = pa[0], g1 = pa[1], b1 = pa[2], r2 = pb[0], g2 = pb[1], b2 = pb[2];
                acc[0] += 299 * r1 + 587 * g1 + 114 * b1;
                acc[1] += 596 * r1 - 274 * g1 - 322 * b1;
                acc[2] += 211 * r1 - 523 * g1 + 312 * b1;
                acc[3] += 299 * r2 + 587 * g2 + 114 * b2;
                acc[4] += 596 * r2 - 274 * g2 - 322 * b2;
                acc[5] += 211 * r2 - 523 * g2 + 312 * b2;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) col[k][t] = acc[k];
    __syncthreads();
    for (int q = t; q < nout * 6; q += FSIM_POOL_THREADS) {
        const int comp = q / nout, jo = q - comp * nout, j = j0 + jo;
        if (j >= cols) continue;
        long long s = 0;
        for (int k = 0; k < F; ++k) s += col[comp][jo * F + k];
        out[(size_t)comp * n + (size_t)i * (size_t)cols + (size_t)j] = s;
    }
}

// the float64 Y plane of one image: the window sum over 1000 F^2
__global__ __launch_bounds__(FSIM_THREADS) void k_fsim_plane(const long long *__restrict__ sums, size_t n, double unit,
                                                             double *__restrict__ plane)
{
    const size_t i = (size_t)blockIdx.x * FSIM_THREADS + threadIdx.x;
    if (i < n) plane[i] = (double)sums[i] / unit;
}

// the transform's input: the plane less its first sample (every filter is 0 at DC)
__global__ __launch_bounds__(FSIM_THREADS) void k_fsim_centre(const double *__restrict__ plane, size_t n, cpx *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * FSIM_THREADS + threadIdx.x;
    if (i < n) out[i] = make_double2(plane[i] - plane[0], 0.0);
}

// ---- the dense transform -------------------------------------------------------------------------------------------------------
// Along the columns of a row: out[z][m][j] = sum_k in'[z][m][k] tw[(k j) mod cols], blockIdx.z = z.
// FILT: one input plane, four outputs: in'[z] = in spread lg[z]; z runs inside the block.
template <bool FILT, bool INV>
__global__ __launch_bounds__(DT * DT) void k_fsim_dft_cols(const cpx *__restrict__ in, const double *__restrict__ lg,
                                                           const double *__restrict__ sp, const cpx *__restrict__ tw, int rows,
                                                           int cols, size_t n, cpx *__restrict__ out)
{
    constexpr int NB = FILT ? FSIM_SCALES : 1;
    __shared__ cpx sA[DT][DT], sB[DT][DT + 1];
    __shared__ double sF[NB][DT][DT];
    const int tx = threadIdx.x & (DT - 1), ty = threadIdx.x / DT;
    const int m = (int)blockIdx.y * DT + ty, j = (int)blockIdx.x * DT + tx;
    if (!FILT) {
        in += (size_t)blockIdx.z * n;
        out += (size_t)blockIdx.z * n;
    }
    cpx acc[NB];
#pragma unroll
    for (int z = 0; z < NB; ++z) acc[z] = make_double2(0.0, 0.0);
    for (int k0 = 0; k0 < cols; k0 += DT) {
        const int ka = k0 + tx, kb = k0 + ty;
        cpx va = make_double2(0.0, 0.0), vb = make_double2(0.0, 0.0);
        double f[NB];
#pragma unroll
        for (int z = 0; z < NB; ++z) f[z] = 0.0;
        if (m < rows && ka < cols) {
            const size_t idx = (size_t)m * (size_t)cols + (size_t)ka;
            va = in[idx];
            if (FILT) {
                const double s = sp[idx];
                va.x *= s;
                va.y *= s;
#pragma unroll
                for (int z = 0; z < NB; ++z) f[z] = lg[(size_t)z * n + idx];
            }
        }
        if (kb < cols && j < cols) {
            vb = tw[(int)(((long long)kb * j) % cols)];
            if (INV) vb.y = -vb.y;
        }
        sA[ty][tx] = va;
        sB[ty][tx] = vb;
        if (FILT) {
#pragma unroll
            for (int z = 0; z < NB; ++z) sF[z][ty][tx] = f[z];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < DT; ++kk) {
            const cpx x = sA[ty][kk], y = sB[kk][tx];
            const double px = fma(-x.y, y.y, x.x * y.x), py = fma(x.x, y.y, x.y * y.x);
            if (FILT) {
#pragma unroll
                for (int z = 0; z < NB; ++z) {
                    const double g = sF[z][ty][kk];
                    acc[z].x = fma(g, px, acc[z].x);
                    acc[z].y = fma(g, py, acc[z].y);
                }
            } else {
                acc[0].x += px;
                acc[0].y += py;
            }
        }
        __syncthreads();
    }
    if (m < rows && j < cols) {
#pragma unroll
        for (int z = 0; z < NB; ++z) out[(size_t)z * n + (size_t)m * (size_t)cols + (size_t)j] = acc[z];
    }
}

// Down the rows of a column: out[z][i][c] = scale sum_k tw[(i k) mod rows] in[z][k][c], blockIdx.z = z.
template <bool INV>
__global__ __launch_bounds__(DT * DT) void k_fsim_dft_rows(const cpx *__restrict__ in, const cpx *__restrict__ tw, int rows,
                                                           int cols, size_t n, double scale, cpx *__restrict__ out)
{
    __shared__ cpx sA[DT][DT], sB[DT][DT + 1];
    const int tx = threadIdx.x & (DT - 1), ty = threadIdx.x / DT;
    const int i = (int)blockIdx.y * DT + ty, c = (int)blockIdx.x * DT + tx;
    in += (size_t)blockIdx.z * n;
    out += (size_t)blockIdx.z * n;
    cpx acc = make_double2(0.0, 0.0);
    for (int k0 = 0; k0 < rows; k0 += DT) {
        const int ka = k0 + tx, kb = k0 + ty;
        cpx va = make_double2(0.0, 0.0), vb = make_double2(0.0, 0.0);
        if (i < rows && ka < rows) {
            va = tw[(int)(((long long)i * ka) % rows)];
            if (INV) va.y = -va.y;
        }
        if (kb < rows && c < cols) vb = in[(size_t)kb * (size_t)cols + (size_t)c];
        sA[ty][tx] = va;
        sB[ty][tx] = vb;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < DT; ++kk) {
            const cpx x = sA[ty][kk], y = sB[kk][tx];
            acc.x += fma(-x.y, y.y, x.x * y.x);
            acc.y += fma(x.x, y.y, x.y * y.x);
        }
        __syncthreads();
    }
    if (i < rows && c < cols) out[(size_t)i * (size_t)cols + (size_t)c] = make_double2(acc.x * scale, acc.y * scale);
}

// ---- energy, median, threshold -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FSIM_THREADS) void k_fsim_energy(const cpx *__restrict__ eo, size_t n, int first,
                                                              double *__restrict__ energy, double *__restrict__ e2,
                                                              double *__restrict__ an_all)
{
    const size_t i = (size_t)blockIdx.x * FSIM_THREADS + threadIdx.x;
    if (i >= n) return;
    double e[FSIM_SCALES], o[FSIM_SCALES], sum_e = 0.0, sum_o = 0.0, sum_an = 0.0, an0 = 0.0;
#pragma unroll
    for (int s = 0; s < FSIM_SCALES; ++s) {
        const cpx v = eo[(size_t)s * n + i];
        e[s] = v.x;
        o[s] = v.y;
        const double an = hypot(v.x, v.y);
        if (s == 0) an0 = an;
        sum_an += an;
        sum_e += v.x;
        sum_o += v.y;
    }
    const double xen = sqrt(sum_e * sum_e + sum_o * sum_o) + FSIM_EPSILON;
    const double me = sum_e / xen, mo = sum_o / xen;
    double en = 0.0;
#pragma unroll
    for (int s = 0; s < FSIM_SCALES; ++s) en = en + e[s] * me + o[s] * mo - fabs(e[s] * mo - o[s] * me);
    energy[i] = en;
    e2[i] = an0 * an0;
    an_all[i] = first ? sum_an : an_all[i] + sum_an;
}

// pass p looks at bits [56 - 8 p, 64 - 8 p) of the keys that match the bits already chosen, for both ranks
__global__ __launch_bounds__(FSIM_THREADS) void k_fsim_hist(const unsigned long long *__restrict__ keys, size_t n, int pass,
                                                            const SelectState *__restrict__ st, unsigned *__restrict__ hist)
{
    __shared__ unsigned sh[2][256];
    const int t = threadIdx.x;
    sh[0][t] = 0;
    sh[1][t] = 0;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    unsigned long long p0 = 0, p1 = 0;
    if (pass > 0) {
        p0 = st->prefix[0];
        p1 = st->prefix[1];
    }
    for (size_t i = (size_t)blockIdx.x * FSIM_THREADS + t; i < n; i += (size_t)gridDim.x * FSIM_THREADS) {
        const unsigned long long key = keys[i];
        const unsigned d = (unsigned)(key >> shift) & 255u;
        const unsigned long long hi = pass > 0 ? key >> (shift + 8) : 0ull;
        if (hi == p0) atomicAdd(&sh[0][d], 1u);
        if (hi == p1) atomicAdd(&sh[1][d], 1u);
    }
    __syncthreads();
    if (sh[0][t]) atomicAdd(&hist[t], sh[0][t]);
    if (sh[1][t]) atomicAdd(&hist[256 + t], sh[1][t]);
}

// One block: picks the digit of both ranks, clears the histograms for the next pass; the last pass (7) writes the median and T.
__global__ __launch_bounds__(FSIM_THREADS) void k_fsim_select(unsigned *__restrict__ hist, SelectState *__restrict__ st, int pass,
                                                              size_t n, double em, double s2, double sij,
                                                              double *__restrict__ med_out, double *__restrict__ t_out)
{
    __shared__ unsigned sh[2][256];
    const int t = threadIdx.x;
    sh[0][t] = hist[t];
    sh[1][t] = hist[256 + t];
    hist[t] = 0;
    hist[256 + t] = 0;
    __syncthreads();
    if (t != 0) return;
    SelectState s;
    if (pass == 0) {
        s.prefix[0] = s.prefix[1] = 0;
        s.rank[0] = (unsigned)((n - 1) / 2);
        s.rank[1] = (unsigned)(n / 2);
    } else {
        s = *st;
    }
    for (int q = 0; q < 2; ++q) {
        unsigned cum = 0;
        int d = 0;
        for (; d < 255; ++d) {
            if (cum + sh[q][d] > s.rank[q]) break;
            cum += sh[q][d];
        }
        s.prefix[q] = (s.prefix[q] << 8) | (unsigned long long)d;
        s.rank[q] -= cum;
    }
    *st = s;
    if (pass != 7) return;
    const double med = (__longlong_as_double((long long)s.prefix[0]) + __longlong_as_double((long long)s.prefix[1])) / 2.0;
    const double pi = 3.14159265358979323846;
    const double noise = (-med / log(0.5)) / em;
    const double tau = sqrt((2.0 * noise * s2 + 4.0 * noise * sij) / 2.0);
    *med_out = med;
    *t_out = (tau * sqrt(pi / 2.0) + FSIM_K * sqrt((2.0 - pi / 2.0) * (tau * tau))) / 1.7;
}

__global__ __launch_bounds__(FSIM_THREADS) void k_fsim_clamp(const double *__restrict__ energy, const double *__restrict__ thr,
                                                             size_t n, int first, int last, double *__restrict__ energy_all,
                                                             const double *__restrict__ an_all, double *__restrict__ pc)
{
    const size_t i = (size_t)blockIdx.x * FSIM_THREADS + threadIdx.x;
    if (i >= n) return;
    const double d = energy[i] - *thr;
    const double v = d > 0.0 ? d : 0.0;
    const double ea = first ? v : energy_all[i] + v;
    energy_all[i] = ea;
    if (last) pc[i] = ea / an_all[i];
}

// ---- the score -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double fs_at(const long long *__restrict__ y, int r, int c, int rows, int cols)
{
    return (r >= 0 && r < rows && c >= 0 && c < cols) ? (double)y[(size_t)r * (size_t)cols + (size_t)c] : 0.0;
}

// G of conv2(Y, dx, 'same'), conv2(Y, dy, 'same'): the sums are exact integers (< 2^53), unit16 = 16 * 1000 F^2
__device__ __forceinline__ double fs_grad(const long long *__restrict__ y, int r, int c, int rows, int cols, double unit16)
{
    const double a = fs_at(y, r - 1, c - 1, rows, cols), b = fs_at(y, r - 1, c, rows, cols), d = fs_at(y, r - 1, c + 1, rows, cols);
    const double e = fs_at(y, r, c - 1, rows, cols), g = fs_at(y, r, c + 1, rows, cols);
    const double p = fs_at(y, r + 1, c - 1, rows, cols), q = fs_at(y, r + 1, c, rows, cols), s = fs_at(y, r + 1, c + 1, rows, cols);
    const double ix = (3.0 * (s - p) + 10.0 * (g - e) + 3.0 * (d - a)) / unit16;
    const double iy = (3.0 * (s - d) + 10.0 * (q - b) + 3.0 * (p - a)) / unit16;
    return sqrt(ix * ix + iy * iy);
}

__device__ __forceinline__ double fs_sim(double u, double v, double k) { return (2.0 * u * v + k) / (u * u + v * v + k); }

__global__ __launch_bounds__(FSIM_THREADS) void k_fsim_score(const long long *__restrict__ pool, const double *__restrict__ pc,
                                                             int rows, int cols, size_t n, double unit,
                                                             double *__restrict__ part)
{
    __shared__ double R[3][FSIM_THREADS];
    const int t = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * FSIM_THREADS + t;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0;
    if (i < n) {
        const int r = (int)(i / (size_t)cols), c = (int)(i - (size_t)r * (size_t)cols);
        const double g1 = fs_grad(pool, r, c, rows, cols, 16.0 * unit), g2 = fs_grad(pool + 3 * n, r, c, rows, cols, 16.0 * unit);
        const double pc1 = pc[i], pc2 = pc[n + i];
        // fmax drops a NaN: a flat plane's 0 / 0 must reach the sums
        const double pcm = (pc1 != pc1 || pc2 != pc2) ? pc1 + pc2 : (pc1 > pc2 ? pc1 : pc2);
        const double s = fs_sim(g1, g2, FSIM_T2) * fs_sim(pc1, pc2, FSIM_T1);
        const double si = fs_sim((double)pool[n + i] / unit, (double)pool[4 * n + i] / unit, FSIM_T34);
        const double sq = fs_sim((double)pool[2 * n + i] / unit, (double)pool[5 * n + i] / unit, FSIM_T34);
        v0 = s * pcm;
        v1 = s * fsim_chroma_weight(si, sq) * pcm;
        v2 = pcm;
    }
    R[0][t] = v0;
    R[1][t] = v1;
    R[2][t] = v2;
    __syncthreads();
    for (int s = FSIM_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            R[0][t] += R[0][t + s];
            R[1][t] += R[1][t + s];
            R[2][t] += R[2][t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        part[(size_t)blockIdx.x * 3] = R[0][0];
        part[(size_t)blockIdx.x * 3 + 1] = R[1][0];
        part[(size_t)blockIdx.x * 3 + 2] = R[2][0];
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
unsigned blocks_of(size_t n) { return (unsigned)((n + FSIM_THREADS - 1) / FSIM_THREADS); }

// The workspace of the plan, with the filters and twiddles of its pooled size in place (built and uploaded when the size or
// the buffer changed).
int fsim_workspace(sr_ctx *ctx, const char *who, const FsimPlan &p, char **ws_out)
{
    bool regrown = false;
    SRCHK(ctx->fsim_ws.reserve(ctx, who, p.total, 0, 1, &regrown));
    char *ws = ctx->fsim_ws.as<char>();
    *ws_out = ws;
    if (!regrown && ctx->fsim_rows == p.rows && ctx->fsim_cols == p.cols) return SR_OK;
    ctx->fsim_rows = ctx->fsim_cols = 0;
    std::vector<double> filt(8 * p.n), tw_r(2 * (size_t)p.rows), tw_c(2 * (size_t)p.cols);
    fsim_filters(p.rows, p.cols, filt.data(), filt.data() + 4 * p.n, ctx->fsim_consts, ctx->fsim_consts + 4, ctx->fsim_consts + 8);
    fsim_twiddles(p.rows, tw_r.data());
    fsim_twiddles(p.cols, tw_c.data());
    HIPCHK(hipMemcpyAsync(ws + p.off_filt, filt.data(), filt.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ws + p.off_tw_r, tw_r.data(), tw_r.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ws + p.off_tw_c, tw_c.data(), tw_c.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(stream_sync(ctx));       // the host tables go out of scope
    ctx->fsim_rows = p.rows;
    ctx->fsim_cols = p.cols;
    return SR_OK;
}

// PC of the float64 plane at off_plane into slot img of off_pc; medians and thresholds into slot img of off_med.
int fsim_pc(sr_ctx *ctx, const FsimPlan &p, char *ws, int img)
{
    const size_t n = p.n;
    const int rows = p.rows, cols = p.cols;
    const double *plane = (const double *)(ws + p.off_plane);
    const double *lg = (const double *)(ws + p.off_filt), *sp = lg + 4 * n;
    const cpx *tw_r = (const cpx *)(ws + p.off_tw_r), *tw_c = (const cpx *)(ws + p.off_tw_c);
    cpx *spec = (cpx *)(ws + p.off_spec), *half = (cpx *)(ws + p.off_half), *eo = (cpx *)(ws + p.off_eo);
    double *pc = (double *)(ws + p.off_pc) + (size_t)img * n;
    double *energy_all = (double *)(ws + p.off_energy_all), *an_all = (double *)(ws + p.off_an_all);
    double *energy = (double *)(ws + p.off_energy), *e2 = (double *)(ws + p.off_e2);
    unsigned *hist = (unsigned *)(ws + p.off_hist);
    SelectState *st = (SelectState *)(ws + p.off_hist + 2 * 256 * sizeof(unsigned));
    double *med = (double *)(ws + p.off_med) + (size_t)img * 8;
    const dim3 tile(DT * DT), grid1((cols + DT - 1) / DT, (rows + DT - 1) / DT, 1), grid4(grid1.x, grid1.y, FSIM_SCALES);
    const unsigned nb = blocks_of(n), hb = nb < (unsigned)FSIM_HIST_BLOCKS ? nb : (unsigned)FSIM_HIST_BLOCKS;
    // every select leaves the histograms clear for the next pass; the first pass of a plane does not rely on the last call
    HIPCHK(hipMemsetAsync(hist, 0, 2 * 256 * sizeof(unsigned), ctx->stream));
    {
        ProfScope ps(ctx, "fsim_dft");
        hipLaunchKernelGGL(k_fsim_centre, dim3(nb), dim3(FSIM_THREADS), 0, ctx->stream, plane, n, eo);
        hipLaunchKernelGGL((k_fsim_dft_cols<false, false>), grid1, tile, 0, ctx->stream, (const cpx *)eo, lg, sp, tw_c, rows, cols, n,
                           half);
        hipLaunchKernelGGL((k_fsim_dft_rows<false>), grid1, tile, 0, ctx->stream, (const cpx *)half, tw_r, rows, cols, n, 1.0, spec);
    }
    for (int o = 0; o < FSIM_ORIENTS; ++o) {
        {
            ProfScope ps(ctx, "fsim_dft");
            hipLaunchKernelGGL((k_fsim_dft_cols<true, true>), grid1, tile, 0, ctx->stream, (const cpx *)spec, lg, sp + (size_t)o * n,
                               tw_c, rows, cols, n, half);
            hipLaunchKernelGGL((k_fsim_dft_rows<true>), grid4, tile, 0, ctx->stream, (const cpx *)half, tw_r, rows, cols, n,
                               1.0 / (double)n, eo);
        }
        {
            ProfScope ps(ctx, "fsim_rest");
            hipLaunchKernelGGL(k_fsim_energy, dim3(nb), dim3(FSIM_THREADS), 0, ctx->stream, (const cpx *)eo, n, o == 0, energy, e2,
                               an_all);
        }
        {
            ProfScope ps(ctx, "fsim_median");
            for (int pass = 0; pass < 8; ++pass) {
                hipLaunchKernelGGL(k_fsim_hist, dim3(hb), dim3(FSIM_THREADS), 0, ctx->stream, (const unsigned long long *)e2, n, pass,
                                   (const SelectState *)st, hist);
                hipLaunchKernelGGL(k_fsim_select, dim3(1), dim3(FSIM_THREADS), 0, ctx->stream, hist, st, pass, n, ctx->fsim_consts[o],
                                   ctx->fsim_consts[4 + o], ctx->fsim_consts[8 + o], med + o, med + 4 + o);
            }
        }
        {
            ProfScope ps(ctx, "fsim_rest");
            hipLaunchKernelGGL(k_fsim_clamp, dim3(nb), dim3(FSIM_THREADS), 0, ctx->stream, (const double *)energy,
                               (const double *)(med + 4 + o), n, o == 0, o == FSIM_ORIENTS - 1, energy_all, (const double *)an_all, pc);
        }
    }
    return check_launch("fsim_pc");
}

template <typename... Args>
void launch_pool(int cn, dim3 grid, hipStream_t stream, Args... args)
{
    if (cn == 1) hipLaunchKernelGGL((k_fsim_pool<1>), grid, dim3(FSIM_POOL_THREADS), 0, stream, args...);
    else if (cn == 3) hipLaunchKernelGGL((k_fsim_pool<3>), grid, dim3(FSIM_POOL_THREADS), 0, stream, args...);
    else hipLaunchKernelGGL((k_fsim_pool<4>), grid, dim3(FSIM_POOL_THREADS), 0, stream, args...);
}

int pair_args(const char *who, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int w, int cn,
              const void *out)
{
    if (!d_a || !d_b || !out) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    const int64_t min_stride = (int64_t)w * cn;
    if (stride_a < min_stride || stride_b < min_stride) return sr_set_error(SR_ERR_SHAPE, "%s: stride smaller than a row", who);
    return SR_OK;
}

}  // namespace

extern "C" {

int sr_fsim_pool_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w, int cn,
                    int F, int64_t *h_out)
{
    // every argument check comes before the context (and so the device) is touched
    if (F == 0) return sr_set_error(SR_ERR_INVALID_ARG, "sr_fsim_pool_u8: F must be 1 .. %d (got 0)", FSIM_MAX_F);
    FsimPlan p;
    SRCHK(fsim_plan("sr_fsim_pool_u8", h, w, cn, F, &p));
    SRCHK(pair_args("sr_fsim_pool_u8", d_a, stride_a, d_b, stride_b, w, cn, h_out));
    CTX_ENTER(ctx);
    DevTemp sums(ctx);
    const size_t bytes = 6 * p.n * sizeof(long long);
    SRCHK(sums.alloc("sr_fsim_pool_u8", bytes));
    launch_pool(cn, dim3((unsigned)p.pool_gx, (unsigned)p.rows), ctx->stream, (const unsigned char *)d_a, (long long)stride_a,
                (const unsigned char *)d_b, (long long)stride_b, h, w, p.F, p.cols, p.n, sums.as<long long>());
    SRCHK(check_launch("fsim_pool"));
    HIPCHK(hipMemcpyAsync(h_out, sums.d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    return SR_OK;
}

int sr_fsim_pc_f64(sr_ctx *ctx, const double *d_plane, int rows, int cols, double *d_pc, double *h_median, double *h_T)
{
    if (!d_plane || !d_pc) return sr_set_error(SR_ERR_INVALID_ARG, "sr_fsim_pc_f64: null argument");
    FsimPlan p;
    SRCHK(fsim_plan_plane("sr_fsim_pc_f64", rows, cols, &p));
    CTX_ENTER(ctx);
    char *ws = nullptr;
    SRCHK(fsim_workspace(ctx, "sr_fsim_pc_f64", p, &ws));
    HIPCHK(hipMemcpyAsync(ws + p.off_plane, d_plane, p.n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    SRCHK(fsim_pc(ctx, p, ws, 0));
    HIPCHK(hipMemcpyAsync(d_pc, ws + p.off_pc, p.n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    double h_med[8];
    HIPCHK(hipMemcpyAsync(h_med, ws + p.off_med, sizeof(h_med), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stream_sync(ctx));
    if (h_median) memcpy(h_median, h_med, 4 * sizeof(double));
    if (h_T) memcpy(h_T, h_med + 4, 4 * sizeof(double));
    return SR_OK;
}

int sr_fsim_u8(sr_ctx *ctx, const uint8_t *d_a, int64_t stride_a, const uint8_t *d_b, int64_t stride_b, int h, int w, int cn,
               sr_fsim_sums *h_out)
{
    FsimPlan p;
    SRCHK(fsim_plan("sr_fsim_u8", h, w, cn, 0, &p));
    SRCHK(pair_args("sr_fsim_u8", d_a, stride_a, d_b, stride_b, w, cn, h_out));
    CTX_ENTER(ctx);
    char *ws = nullptr;
    SRCHK(fsim_workspace(ctx, "sr_fsim_u8", p, &ws));
    long long *pool = (long long *)(ws + p.off_pool);
    double *part = (double *)(ws + p.off_part), *buf0 = (double *)(ws + p.off_buf0), *buf1 = (double *)(ws + p.off_buf1);
    const double unit = 1000.0 * (double)p.F * (double)p.F;
    {
        ProfScope ps(ctx, "fsim_pool");
        launch_pool(cn, dim3((unsigned)p.pool_gx, (unsigned)p.rows), ctx->stream, (const unsigned char *)d_a, (long long)stride_a,
                    (const unsigned char *)d_b, (long long)stride_b, h, w, p.F, p.cols, p.n, pool);
    }
    SRCHK(check_launch("fsim_pool"));
    for (int img = 0; img < 2; ++img) {
        {
            ProfScope ps(ctx, "fsim_rest");
            hipLaunchKernelGGL(k_fsim_plane, dim3(blocks_of(p.n)), dim3(FSIM_THREADS), 0, ctx->stream,
                               (const long long *)(pool + (size_t)img * 3 * p.n), p.n, unit, (double *)(ws + p.off_plane));
        }
        SRCHK(fsim_pc(ctx, p, ws, img));
    }
    double h_res[3];
    {
        ProfScope ps(ctx, "fsim_rest");
        hipLaunchKernelGGL(k_fsim_score, dim3((unsigned)p.score_blocks), dim3(FSIM_THREADS), 0, ctx->stream, (const long long *)pool,
                           (const double *)(ws + p.off_pc), p.rows, p.cols, p.n, unit, part);
        const double *sums = reduce_partials(ctx, part, (long long)p.score_blocks, 3, buf0, buf1);
        SRCHK(check_launch("fsim_score"));
        HIPCHK(hipMemcpyAsync(h_res, sums, sizeof(h_res), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(stream_sync(ctx));
    memset(h_out, 0, sizeof(*h_out));
    h_out->sum_s = h_res[0];
    h_out->sum_sc = h_res[1];
    h_out->sum_pcm = h_res[2];
    h_out->count = (uint64_t)p.n;
    h_out->F = p.F;
    h_out->rows = p.rows;
    h_out->cols = p.cols;
    return SR_OK;
}

}  // extern "C"
