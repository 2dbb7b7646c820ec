// sr_vsi_host.cpp -- the host side of VSI: F, the pooled size, the triangle resize tables of the four axes (imr_axis_kernel:
// sr_imresize_host.cpp's rule with the triangle), the composite pooling tables, the workspace layout (vsi_plan: every shape
// refusal), the log-Gabor and centre-prior planes, the value, and the float64 restatement of the whole metric on host memory
// in the kernels' formulation (sr_vsi_host_u8).  Pure host code: nothing here touches the device, so the unit also links into
// a stand-alone program (tools/sanitize/vsi_driver.cpp, with sr_imresize_host.cpp and sr_fsim_host.cpp).  The definition is in
// include/sr_hip.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <vector>

#include "sr_vsi.h"

namespace {

constexpr double VSI_NAN = std::numeric_limits<double>::quiet_NaN();
constexpr int VSI_MAX_SIDE = 1 << 20;       // of an image: the axis tables and the launches are sized by the sides

// The composite axis of the pooled map: the up-resize rows of the in-image part of every window added up.
void build_band(const ImrAxis &u, int F, int n_pool, VsiBand *b)
{
    const int n_full = u.n_out, taps = u.taps;
    b->n_out = n_pool;
    b->lo.assign(n_pool, 0);
    b->cover.assign(n_pool, 0);
    std::vector<int32_t> hi(n_pool, 0);
    int band = 1;
    for (int i = 0; i < n_pool; ++i) {
        const long long s = fsim_win_start(i, F);
        const long long y0 = std::max(s, 0LL), y1 = std::min(s + F, (long long)n_full);
        int lo = VSI_N, top = -1;
        for (long long y = y0; y < y1; ++y)
            for (int k = 0; k < taps; ++k) {
                const int m = u.idx[(size_t)y * taps + k];
                lo = std::min(lo, m);
                top = std::max(top, m);
            }
        if (top < 0) lo = top = 0;          // an empty window (not reached: ceil(n / F) windows all meet the image)
        b->lo[i] = lo;
        hi[i] = top;
        b->cover[i] = (int32_t)std::max(0LL, y1 - y0);
        band = std::max(band, top - lo + 1);
    }
    b->band = band;
    b->w.assign((size_t)n_pool * band, 0.0);
    for (int i = 0; i < n_pool; ++i) {
        const long long s = fsim_win_start(i, F);
        const long long y0 = std::max(s, 0LL), y1 = std::min(s + F, (long long)n_full);
        double *row = &b->w[(size_t)i * band];
        for (long long y = y0; y < y1; ++y)
            for (int k = 0; k < taps; ++k) row[u.idx[(size_t)y * taps + k] - b->lo[i]] += u.w[(size_t)y * taps + k];
    }
}

void layout(VsiPlan *p, const VsiTables *t)
{
    const size_t n = p->n, d = sizeof(double), NN = VSI_NN;
    size_t off = 0;
    auto take = [&off](size_t bytes) {
        const size_t at = off;
        off += up256(bytes);
        return at;
    };
    p->off_pool = take(6 * n * sizeof(int64_t));
    p->score_blocks = (n + VSI_THREADS - 1) / VSI_THREADS;
    if (t) {
        p->off_lg = take(NN * d);
        p->off_sd = take(NN * d);
        p->off_tw = take(VSI_N * 2 * d);
        const ImrAxis *ax[4] = {&t->sy, &t->sx, &t->uy, &t->ux};
        for (int k = 0; k < 4; ++k) {
            p->off_w[k] = take(ax[k]->w.size() * d);
            p->off_idx[k] = take(ax[k]->idx.size() * sizeof(int32_t));
        }
        const VsiBand *bd[2] = {&t->cy, &t->cx};
        for (int k = 0; k < 2; ++k) {
            p->off_w[4 + k] = take(bd[k]->w.size() * d);
            p->off_idx[4 + k] = take(bd[k]->lo.size() * sizeof(int32_t));
            p->off_cover[k] = take(bd[k]->cover.size() * sizeof(int32_t));
        }
        const size_t first = p->order == 0 ? (size_t)VSI_N * (size_t)p->w * 3 : (size_t)p->h * VSI_N * 3;
        p->off_tmp = take(std::max(first, (size_t)VSI_N * (size_t)std::max(p->w, p->cols)) * d);
        p->off_rgb = take(3 * NN * d);
        p->off_lab = take(3 * NN * d);
        p->off_c0 = take(3 * NN * 2 * d);
        p->off_c1 = take(3 * NN * 2 * d);
        p->off_vs256 = take(NN * d);
        p->off_range = take(2 * 8 * d);
        p->off_rpart = take((size_t)(VSI_NN / VSI_THREADS) * 4 * d);
        p->off_mpart = take((size_t)p->expand_gx * (size_t)p->expand_gy * 2 * d);
        p->off_pvs = take(2 * n * d);
        p->off_part = take(p->score_blocks * 2 * d);
        const size_t buf = (p->score_blocks / 1024 + 2) * 2 * d;
        p->off_buf0 = take(buf);
        p->off_buf1 = take(buf);
    }
    p->total = off;
}

typedef std::vector<double> dvec;

// out[z][i][c] (ROWS) or out[z][m][j] (columns of a row) of one 256 x 256 complex plane, interleaved re / im
void dft_pass(const double *in, const double *tw, bool rows, bool inv, const double *filt, double scale, double *out)
{
    const int N = VSI_N;
    std::vector<double> acc(2 * (size_t)N);
    for (int a = 0; a < N; ++a) {           // the row (column pass) or the column (row pass) at work
        std::fill(acc.begin(), acc.end(), 0.0);
        for (int k = 0; k < N; ++k) {
            const size_t at = rows ? (size_t)k * N + a : (size_t)a * N + k;
            double xr = in[2 * at], xi = in[2 * at + 1];
            if (filt) {
                xr *= filt[at];
                xi *= filt[at];
            }
            if (xr == 0.0 && xi == 0.0) continue;
            for (int j = 0; j < N; ++j) {
                const int q = (k * j) & (N - 1);
                const double tr = tw[2 * q], ti = inv ? -tw[2 * q + 1] : tw[2 * q + 1];
                acc[2 * j] += xr * tr - xi * ti;
                acc[2 * j + 1] += xr * ti + xi * tr;
            }
        }
        for (int j = 0; j < N; ++j) {
            const size_t at = rows ? (size_t)j * N + a : (size_t)a * N + j;
            out[2 * at] = acc[2 * j] * scale;
            out[2 * at + 1] = acc[2 * j + 1] * scale;
        }
    }
}

struct HostTables {
    dvec lg, sd, tw;
};

// Lab, VS256 and the a / b ranges of one image
void host_saliency(const unsigned char *img, long long stride, const VsiPlan &p, const VsiTables &t, const HostTables &ht,
                   dvec *lab, dvec *vs256, double *range)
{
    const int N = VSI_N, cn = p.cn, h = p.h, w = p.w;
    dvec rgb(3 * (size_t)VSI_NN), tmp;
    if (p.order == 0) {
        tmp.assign((size_t)N * w * 3, 0.0);
        for (int i = 0; i < N; ++i)
            for (int x = 0; x < w; ++x)
                for (int c = 0; c < 3; ++c) {
                    double acc = 0.0;
                    for (int k = 0; k < t.sy.taps; ++k)
                        acc += t.sy.w[(size_t)i * t.sy.taps + k] *
                               (double)img[(size_t)t.sy.idx[(size_t)i * t.sy.taps + k] * (size_t)stride + (size_t)x * cn + c];
                    tmp[((size_t)i * w + x) * 3 + c] = acc;
                }
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j)
                for (int c = 0; c < 3; ++c) {
                    double acc = 0.0;
                    for (int k = 0; k < t.sx.taps; ++k)
                        acc += t.sx.w[(size_t)j * t.sx.taps + k] * tmp[((size_t)i * w + t.sx.idx[(size_t)j * t.sx.taps + k]) * 3 + c];
                    rgb[(size_t)c * VSI_NN + (size_t)i * N + j] = acc;
                }
    } else {
        tmp.assign((size_t)h * N * 3, 0.0);
        for (int y = 0; y < h; ++y)
            for (int j = 0; j < N; ++j)
                for (int c = 0; c < 3; ++c) {
                    double acc = 0.0;
                    for (int k = 0; k < t.sx.taps; ++k)
                        acc += t.sx.w[(size_t)j * t.sx.taps + k] *
                               (double)img[(size_t)y * (size_t)stride + (size_t)t.sx.idx[(size_t)j * t.sx.taps + k] * cn + c];
                    tmp[((size_t)y * N + j) * 3 + c] = acc;
                }
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j)
                for (int c = 0; c < 3; ++c) {
                    double acc = 0.0;
                    for (int k = 0; k < t.sy.taps; ++k)
                        acc += t.sy.w[(size_t)i * t.sy.taps + k] * tmp[((size_t)t.sy.idx[(size_t)i * t.sy.taps + k] * N + j) * 3 + c];
                    rgb[(size_t)c * VSI_NN + (size_t)i * N + j] = acc;
                }
    }
    lab->assign(3 * (size_t)VSI_NN, 0.0);
    double *L = lab->data(), *A = L + VSI_NN, *B = A + VSI_NN;
    for (int i = 0; i < VSI_NN; ++i) vsi_rgb2lab(rgb[i], rgb[VSI_NN + i], rgb[2 * (size_t)VSI_NN + i], &L[i], &A[i], &B[i]);
    range[0] = range[1] = A[0];
    range[2] = range[3] = B[0];
    for (int i = 1; i < VSI_NN; ++i) {
        range[0] = std::min(range[0], A[i]);
        range[1] = std::max(range[1], A[i]);
        range[2] = std::min(range[2], B[i]);
        range[3] = std::max(range[3], B[i]);
    }
    dvec c0(2 * (size_t)VSI_NN), c1(2 * (size_t)VSI_NN), sf2((size_t)VSI_NN, 0.0);
    for (int z = 0; z < 3; ++z) {
        const double *pl = L + (size_t)z * VSI_NN;
        for (int i = 0; i < VSI_NN; ++i) {
            c0[2 * (size_t)i] = pl[i] - pl[0];
            c0[2 * (size_t)i + 1] = 0.0;
        }
        dft_pass(c0.data(), ht.tw.data(), false, false, nullptr, 1.0, c1.data());
        dft_pass(c1.data(), ht.tw.data(), true, false, nullptr, 1.0, c0.data());
        dft_pass(c0.data(), ht.tw.data(), false, true, ht.lg.data(), 1.0, c1.data());
        dft_pass(c1.data(), ht.tw.data(), true, true, nullptr, 1.0 / (double)VSI_NN, c0.data());
        for (int i = 0; i < VSI_NN; ++i) sf2[i] += c0[2 * (size_t)i] * c0[2 * (size_t)i];
    }
    vs256->assign((size_t)VSI_NN, 0.0);
    for (int i = 0; i < VSI_NN; ++i) (*vs256)[i] = vsi_saliency(sf2[i], ht.sd[i], A[i], B[i], range);
}

// min / max of the full-resolution map (mm[0], mm[1]) and the raw window sums pvs[rows * cols]
void host_expand(const dvec &vs, const VsiPlan &p, const VsiTables &t, double *mm, dvec *pvs)
{
    const int N = VSI_N, h = p.h, w = p.w;
    dvec tmp((size_t)N * w);
    for (int m = 0; m < N; ++m)
        for (int x = 0; x < w; ++x) {
            double acc = 0.0;
            for (int k = 0; k < t.ux.taps; ++k) acc += t.ux.w[(size_t)x * t.ux.taps + k] * vs[(size_t)m * N + t.ux.idx[(size_t)x * t.ux.taps + k]];
            tmp[(size_t)m * w + x] = acc;
        }
    double mn = 0.0, mx = 0.0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            double acc = 0.0;
            for (int k = 0; k < t.uy.taps; ++k) acc += t.uy.w[(size_t)y * t.uy.taps + k] * tmp[(size_t)t.uy.idx[(size_t)y * t.uy.taps + k] * w + x];
            if (y == 0 && x == 0) mn = mx = acc;
            mn = vsi_min(mn, acc);
            mx = vsi_max(mx, acc);
        }
    mm[0] = mn;
    mm[1] = mx;
    dvec tp((size_t)N * p.cols);
    for (int m = 0; m < N; ++m)
        for (int j = 0; j < p.cols; ++j) {
            double acc = 0.0;
            for (int b = 0; b < t.cx.band; ++b)
                acc += t.cx.w[(size_t)j * t.cx.band + b] * vs[(size_t)m * N + std::min(t.cx.lo[j] + b, N - 1)];
            tp[(size_t)m * p.cols + j] = acc;
        }
    pvs->assign(p.n, 0.0);
    for (int i = 0; i < p.rows; ++i)
        for (int j = 0; j < p.cols; ++j) {
            double acc = 0.0;
            for (int b = 0; b < t.cy.band; ++b)
                acc += t.cy.w[(size_t)i * t.cy.band + b] * tp[(size_t)std::min(t.cy.lo[i] + b, N - 1) * p.cols + j];
            (*pvs)[(size_t)i * p.cols + j] = acc;
        }
}

void host_pool(const unsigned char *img, long long stride, const VsiPlan &p, std::vector<long long> *out)
{
    out->assign(3 * p.n, 0);
    for (int i = 0; i < p.rows; ++i)
        for (int j = 0; j < p.cols; ++j) {
            const long long ys = fsim_win_start(i, p.F), xs = fsim_win_start(j, p.F);
            long long l = 0, m = 0, n = 0;
            for (long long y = std::max(ys, 0LL); y < std::min(ys + p.F, (long long)p.h); ++y)
                for (long long x = std::max(xs, 0LL); x < std::min(xs + p.F, (long long)p.w); ++x) {
                    const unsigned char *px = img + (size_t)y * (size_t)stride + (size_t)x * p.cn;
                    const int r = px[0], g = px[1], b = px[2];
                    l += 6 * r + 63 * g + 27 * b;
                    m += 30 * r + 4 * g - 35 * b;
                    n += 34 * r - 60 * g + 17 * b;
                }
            const size_t at = (size_t)i * p.cols + j;
            (*out)[at] = l;
            (*out)[p.n + at] = m;
            (*out)[2 * p.n + at] = n;
        }
}

double at0(const long long *y, int r, int c, int rows, int cols)
{
    return (r >= 0 && r < rows && c >= 0 && c < cols) ? (double)y[(size_t)r * (size_t)cols + (size_t)c] : 0.0;
}

double grad(const long long *y, int r, int c, int rows, int cols, double unit16)
{
    const double a = at0(y, r - 1, c - 1, rows, cols), b = at0(y, r - 1, c, rows, cols), d = at0(y, r - 1, c + 1, rows, cols);
    const double e = at0(y, r, c - 1, rows, cols), g = at0(y, r, c + 1, rows, cols);
    const double p = at0(y, r + 1, c - 1, rows, cols), q = at0(y, r + 1, c, rows, cols), s = at0(y, r + 1, c + 1, rows, cols);
    const double ix = (3.0 * (s - p) + 10.0 * (g - e) + 3.0 * (d - a)) / unit16;
    const double iy = (3.0 * (s - d) + 10.0 * (q - b) + 3.0 * (p - a)) / unit16;
    return std::sqrt(ix * ix + iy * iy);
}

int host_run(const unsigned char *a, long long sa, const unsigned char *b, long long sb, const VsiPlan &p, const VsiTables &t,
             sr_vsi_sums *out)
{
    HostTables ht;
    ht.lg.resize(VSI_NN);
    ht.sd.resize(VSI_NN);
    ht.tw.resize(2 * VSI_N);
    vsi_filter(ht.lg.data(), ht.sd.data());
    fsim_twiddles(VSI_N, ht.tw.data());
    const unsigned char *img[2] = {a, b};
    const long long st[2] = {sa, sb};
    std::vector<long long> pool[2];
    dvec pvs[2];
    double mm[4];
    memset(out, 0, sizeof(*out));
    for (int k = 0; k < 2; ++k) {
        dvec lab, vs;
        double range[4];
        host_saliency(img[k], st[k], p, t, ht, &lab, &vs, range);
        host_expand(vs, p, t, mm + 2 * k, &pvs[k]);
        host_pool(img[k], st[k], p, &pool[k]);
        out->a_range[k][0] = range[0];
        out->a_range[k][1] = range[1];
        out->b_range[k][0] = range[2];
        out->b_range[k][1] = range[3];
        out->vs_range[k][0] = mm[2 * k];
        out->vs_range[k][1] = mm[2 * k + 1];
    }
    const double ff = (double)p.F * (double)p.F, unit = 100.0 * ff;
    double sum_s = 0.0, sum_w = 0.0;
    for (int r = 0; r < p.rows; ++r)
        for (int c = 0; c < p.cols; ++c) {
            const size_t i = (size_t)r * p.cols + c;
            const double g1 = grad(pool[0].data(), r, c, p.rows, p.cols, 16.0 * unit);
            const double g2 = grad(pool[1].data(), r, c, p.rows, p.cols, 16.0 * unit);
            double s = 0.0, wg = 0.0;
            vsi_sample(g1, g2, (double)pool[0][p.n + i] / unit, (double)pool[1][p.n + i] / unit, (double)pool[0][2 * p.n + i] / unit,
                       (double)pool[1][2 * p.n + i] / unit, pvs[0][i], pvs[1][i], (double)t.cy.cover[r] * (double)t.cx.cover[c], mm, ff,
                       &s, &wg);
            sum_s += s;
            sum_w += wg;
        }
    out->sum_s = sum_s;
    out->sum_w = sum_w;
    out->count = (uint64_t)p.n;
    out->F = p.F;
    out->rows = p.rows;
    out->cols = p.cols;
    return SR_OK;
}

}  // namespace

int vsi_axis(const char *scope, int n_in, int n_out, ImrAxis *a)
{
    if (n_in < 1 || n_out < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: sides must be >= 1 (got %d -> %d)", scope, n_in, n_out);
    return imr_axis_kernel(scope, n_in, n_out, (double)n_out / (double)n_in, 1, IMR_TRIANGLE, false, a);
}

int vsi_plan(const char *scope, int h, int w, int cn, int F, VsiPlan *p, VsiTables *t)
{
    if (cn != 1 && cn != 3 && cn != 4) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need 3 (RGB) or 4 (RGBA) channels (got %d)", scope, cn);
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need h, w >= 1", scope);
    if (cn == 1)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: VSI is defined for colour images: a gray image has no a / b range (got 1 channel)",
                            scope);
    const bool own = F == 0;
    if (own) {
        if (!t) return sr_set_error(SR_ERR_INVALID_ARG, "%s: internal: no room for the tables", scope);
        if (h < VSI_MIN_SIDE || w < VSI_MIN_SIDE)
            return sr_set_error(SR_ERR_SHAPE, "%s: image %dx%d: both sides must be at least %d", scope, w, h, VSI_MIN_SIDE);
        if (h > VSI_MAX_SIDE || w > VSI_MAX_SIDE)
            return sr_set_error(SR_ERR_UNSUPPORTED, "%s: image %dx%d: a side above %d is not supported", scope, w, h, VSI_MAX_SIDE);
        F = fsim_auto_f(h, w);
        if (F > VSI_MAX_F)
            return sr_set_error(SR_ERR_UNSUPPORTED, "%s: image %dx%d pools by F = %d: F above %d is not supported", scope, w, h, F,
                                VSI_MAX_F);
    } else if (F < 1 || F > VSI_MAX_F) {
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: F must be 1 .. %d (got %d)", scope, VSI_MAX_F, F);
    }
    memset(p, 0, sizeof(*p));
    p->h = h;
    p->w = w;
    p->cn = cn;
    p->F = F;
    p->rows = (int)(((long long)h + F - 1) / F);
    p->cols = (int)(((long long)w + F - 1) / F);
    p->n = (size_t)p->rows * (size_t)p->cols;
    const int out = VSI_THREADS / F;
    p->pool_gx = (p->cols + out - 1) / out;
    if (p->rows > 65535)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d pooled rows are more than one launch covers (65535)", scope, p->rows);
    if (own) {
        // imresize's order: the smaller scale first, a tie the vertical pass (scale = 256 / side)
        p->order = h >= w ? 0 : 1;
        p->expand_gx = (w + VSI_THREADS - 1) / VSI_THREADS;
        p->expand_gy = (h + VSI_EXPAND_ROWS - 1) / VSI_EXPAND_ROWS;
        try {
            int rc = vsi_axis(scope, h, VSI_N, &t->sy);
            if (!rc) rc = vsi_axis(scope, w, VSI_N, &t->sx);
            if (!rc) rc = vsi_axis(scope, VSI_N, h, &t->uy);
            if (!rc) rc = vsi_axis(scope, VSI_N, w, &t->ux);
            if (rc) return rc;
            build_band(t->uy, F, p->rows, &t->cy);
            build_band(t->ux, F, p->cols, &t->cx);
        } catch (const std::bad_alloc &) {
            return sr_set_error(SR_ERR_OOM, "%s: out of host memory for the tables of a %dx%d image", scope, w, h);
        }
    }
    layout(p, own ? t : nullptr);
    return SR_OK;
}

void vsi_filter(double *lg, double *sd)
{
    const int N = VSI_N, half = N / 2;
    for (int r = 0; r < N; ++r)
        for (int c = 0; c < N; ++c) {
            const size_t i = (size_t)r * N + c;
            if (lg) {
                // index r of the ifftshifted axis holds the centred index (r + 128) mod 256
                double u1 = (double)((c + half) % N - half) / (double)N, u2 = (double)((r + half) % N - half) / (double)N;
                if (u1 * u1 + u2 * u2 > 0.25) u1 = u2 = 0.0;
                const double r0 = std::sqrt(u1 * u1 + u2 * u2);
                if (i == 0 || r0 == 0.0) {
                    lg[i] = 0.0;
                } else {
                    const double l = std::log(r0 / VSI_OMEGA0);
                    lg[i] = std::exp(-(l * l) / (2.0 * VSI_SIGMA_F * VSI_SIGMA_F));
                }
            }
            if (sd) {
                const double dy = (double)(r + 1 - half), dx = (double)(c + 1 - half);
                sd[i] = std::exp(-(dy * dy + dx * dx) / (VSI_SIGMA_D * VSI_SIGMA_D));
            }
        }
}

extern "C" {

int sr_vsi_plan(int h, int w, int cn, int *F, int *rows, int *cols, size_t *workspace_bytes)
{
    VsiPlan p;
    VsiTables t;
    const int rc = vsi_plan("sr_vsi_plan", h, w, cn, 0, &p, &t);
    if (rc) return rc;
    if (F) *F = p.F;
    if (rows) *rows = p.rows;
    if (cols) *cols = p.cols;
    if (workspace_bytes) *workspace_bytes = p.total;
    return SR_OK;
}

int sr_vsi_filter(double *lg, double *sd)
{
    vsi_filter(lg, sd);
    return SR_OK;
}

int sr_vsi_resize_weights(int n_in, int n_out, int cap, int *taps, double *w, int32_t *idx)
{
    if (!taps || (w == nullptr) != (idx == nullptr))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_vsi_resize_weights: taps is null, or only one of w and idx");
    ImrAxis a;
    const int rc = vsi_axis("sr_vsi_resize_weights", n_in, n_out, &a);
    if (rc) return rc;
    *taps = a.taps;
    if (!w) return SR_OK;
    if (cap < a.taps) return sr_set_error(SR_ERR_INVALID_ARG, "sr_vsi_resize_weights: room for %d taps, %d needed", cap, a.taps);
    memcpy(w, a.w.data(), a.w.size() * sizeof(double));
    memcpy(idx, a.idx.data(), a.idx.size() * sizeof(int32_t));
    return SR_OK;
}

double sr_vsi_value(const sr_vsi_sums *sums)
{
    if (!sums) {
        sr_set_error(SR_ERR_INVALID_ARG, "sr_vsi_value: null record");
        return VSI_NAN;
    }
    return sums->sum_s / sums->sum_w;       // 0 / 0 is NaN
}

double sr_vsi_chroma_weight(double s_c) { return vsi_chroma_weight(s_c); }

int sr_vsi_host_u8(const uint8_t *a, int64_t stride_a, const uint8_t *b, int64_t stride_b, int h, int w, int cn, sr_vsi_sums *out)
{
    if (!a || !b || !out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_vsi_host_u8: null argument");
    VsiPlan p;
    VsiTables t;
    const int rc = vsi_plan("sr_vsi_host_u8", h, w, cn, 0, &p, &t);
    if (rc) return rc;
    const int64_t min_stride = (int64_t)w * cn;
    if (stride_a < min_stride || stride_b < min_stride) return sr_set_error(SR_ERR_SHAPE, "sr_vsi_host_u8: stride smaller than a row");
    try {
        return host_run(a, stride_a, b, stride_b, p, t, out);
    } catch (const std::bad_alloc &) {
        return sr_set_error(SR_ERR_OOM, "sr_vsi_host_u8: out of host memory for a %dx%d image", w, h);
    }
}

}  // extern "C"
