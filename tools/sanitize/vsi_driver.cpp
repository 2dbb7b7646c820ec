// vsi_driver.cpp -- stand-alone driver for the sanitizer run of the host side of VSI (tests/test_vsi_sanitize.py): compiled
// with csrc/sr_vsi_host.cpp and the two host units it calls (sr_imresize_host.cpp for the contribution rule, sr_fsim_host.cpp
// for F and the twiddles) under -fsanitize=address,undefined, it takes sr_vsi_plan, the axis tables, LG / SD, the value and
// sr_vsi_host_u8 through every refusal and through shapes on both sides of every threshold with exact-size heap buffers, and
// checks each plan the way the kernels use it: every table index lies inside its source, every band inside the 256 grid
// samples, every section inside the workspace and none overlaps the next.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sr_vsi.h"

static char g_err[512] = "";

// sr_host.cpp owns this in the library; the driver links the host units alone
int sr_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define REQUIRE(cond)                                                                     \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            fprintf(stderr, "vsi_driver: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

static int check_axis(const ImrAxis &a, int n_in, int n_out)
{
    REQUIRE(a.n_in == n_in && a.n_out == n_out && a.taps >= 1);
    REQUIRE(a.w.size() == (size_t)n_out * a.taps && a.idx.size() == a.w.size());
    for (int i = 0; i < n_out; ++i) {
        double s = 0.0;
        for (int k = 0; k < a.taps; ++k) {
            const size_t at = (size_t)i * a.taps + k;
            REQUIRE(a.idx[at] >= 0 && a.idx[at] < n_in && a.w[at] >= 0.0);
            s += a.w[at];
        }
        REQUIRE(std::fabs(s - 1.0) <= 1e-14);
    }
    return 0;
}

static int check_band(const VsiBand &b, int n_pool, int n_full, int F)
{
    REQUIRE(b.n_out == n_pool && b.band >= 1 && b.band <= VSI_N);
    REQUIRE(b.w.size() == (size_t)n_pool * b.band && b.lo.size() == (size_t)n_pool && b.cover.size() == (size_t)n_pool);
    long long covered = 0;
    for (int i = 0; i < n_pool; ++i) {
        REQUIRE(b.lo[i] >= 0 && b.lo[i] < VSI_N && b.cover[i] >= 1 && b.cover[i] <= F);
        covered += b.cover[i];
        double s = 0.0;
        for (int k = 0; k < b.band; ++k) {
            const double v = b.w[(size_t)i * b.band + k];
            REQUIRE(v >= 0.0 && (v == 0.0 || b.lo[i] + k < VSI_N));         // weight 0 past the grid's last sample
            s += v;
        }
        REQUIRE(std::fabs(s - (double)b.cover[i]) <= 1e-12 * F);            // every up-resize row sums to 1
    }
    // the windows tile the axis from floor(F / 2) - F + 1 on: all of it when the last window reaches the end
    REQUIRE(covered <= n_full && covered >= n_full - F);
    return 0;
}

static int check_plan(const VsiPlan &p, const VsiTables &t)
{
    const size_t n = p.n, d = sizeof(double), NN = VSI_NN;
    REQUIRE(n == (size_t)p.rows * (size_t)p.cols && p.order == (p.h >= p.w ? 0 : 1));
    if (check_axis(t.sy, p.h, VSI_N) || check_axis(t.sx, p.w, VSI_N) || check_axis(t.uy, VSI_N, p.h) || check_axis(t.ux, VSI_N, p.w)) return 1;
    if (check_band(t.cy, p.rows, p.h, p.F) || check_band(t.cx, p.cols, p.w, p.F)) return 1;
    const size_t first = p.order == 0 ? (size_t)VSI_N * p.w * 3 : (size_t)p.h * VSI_N * 3;
    const size_t tmp = std::max(first, (size_t)VSI_N * (size_t)p.w);
    const size_t off[] = {p.off_pool, p.off_lg, p.off_sd, p.off_tw, p.off_w[0], p.off_idx[0], p.off_w[1], p.off_idx[1], p.off_w[2],
                          p.off_idx[2], p.off_w[3], p.off_idx[3], p.off_w[4], p.off_idx[4], p.off_cover[0], p.off_w[5], p.off_idx[5],
                          p.off_cover[1], p.off_tmp, p.off_rgb, p.off_lab, p.off_c0, p.off_c1, p.off_vs256, p.off_range, p.off_rpart,
                          p.off_mpart, p.off_pvs, p.off_part, p.off_buf0, p.off_buf1, p.total};
    const size_t need[] = {6 * n * 8, NN * d, NN * d, 2 * VSI_N * d, t.sy.w.size() * d, t.sy.idx.size() * 4, t.sx.w.size() * d,
                           t.sx.idx.size() * 4, t.uy.w.size() * d, t.uy.idx.size() * 4, t.ux.w.size() * d, t.ux.idx.size() * 4,
                           t.cy.w.size() * d, (size_t)p.rows * 4, (size_t)p.rows * 4, t.cx.w.size() * d, (size_t)p.cols * 4,
                           (size_t)p.cols * 4, tmp * d, 3 * NN * d, 3 * NN * d, 6 * NN * d, 6 * NN * d, NN * d, 16 * d, 256 * 4 * d,
                           (size_t)p.expand_gx * p.expand_gy * 2 * d, 2 * n * d, p.score_blocks * 2 * d,
                           ((p.score_blocks + 1023) / 1024) * 2 * d, ((p.score_blocks + 1023) / 1024) * 2 * d};
    for (int k = 0; k < 31; ++k) REQUIRE(off[k] % 256 == 0 && off[k] + need[k] <= off[k + 1]);
    REQUIRE(p.score_blocks * VSI_THREADS >= n && (p.score_blocks - 1) * VSI_THREADS < n);
    REQUIRE((long long)p.expand_gx * VSI_THREADS >= p.w && (long long)p.expand_gy * VSI_EXPAND_ROWS >= p.h && p.expand_gy <= 65535);
    const int out = VSI_THREADS / p.F;
    REQUIRE(out >= 1 && (long long)p.pool_gx * out >= p.cols && (long long)(p.pool_gx - 1) * out < p.cols && p.rows <= 65535);
    return 0;
}

static int one(int h, int w, int cn)
{
    int F = 0, rows = 0, cols = 0;
    size_t bytes = 0;
    const int rc = sr_vsi_plan(h, w, cn, &F, &rows, &cols, &bytes);
    if (cn == 1) {
        REQUIRE(rc == SR_ERR_UNSUPPORTED);
        return 0;
    }
    if (h < VSI_MIN_SIDE || w < VSI_MIN_SIDE) {
        REQUIRE(rc == SR_ERR_SHAPE);
        return 0;
    }
    const int f = fsim_auto_f(h, w);
    if (h > (1 << 20) || w > (1 << 20) || f > VSI_MAX_F || ((long long)h + f - 1) / f > 65535) {
        REQUIRE(rc == SR_ERR_UNSUPPORTED);
        return 0;
    }
    REQUIRE(rc == SR_OK && F == f && rows == (h + f - 1) / f && cols == (w + f - 1) / f);
    REQUIRE(sr_vsi_plan(h, w, cn, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    VsiPlan p;
    VsiTables t;
    REQUIRE(vsi_plan("driver", h, w, cn, 0, &p, &t) == SR_OK && p.total == bytes);
    return check_plan(p, t);
}

int main()
{
    const int sides[] = {1, 15, 16, 17, 255, 256, 257, 383, 384, 641, 14142, 65700, (1 << 20) + 1, 2147483647};
    for (int h : sides)
        for (int w : sides)
            if (one(h, w, 3)) return 1;
    if (one(17, 384, 4) || one(641, 16, 4) || one(64, 64, 1) || one(8, 64, 1) || one(65600, 1 << 20, 3)) return 1;
    // the inspection form of the pooling: any F in 1 .. 256 on any size, no table
    for (int F : {1, 2, 3, 8, 85, 86, 200, 256})
        for (int h : {1, 13, 300})
            for (int w : {1, 19, 255, 257, 610}) {
                VsiPlan p;
                REQUIRE(vsi_plan("driver", h, w, 3, F, &p, nullptr) == SR_OK && p.F == F);
                REQUIRE(p.rows == (h + F - 1) / F && p.cols == (w + F - 1) / F && p.total >= 6 * p.n * 8);
            }
    {
        VsiPlan p;
        REQUIRE(vsi_plan("driver", 64, 64, 3, 257, &p, nullptr) == SR_ERR_INVALID_ARG);
        REQUIRE(vsi_plan("driver", 64, 64, 3, -1, &p, nullptr) == SR_ERR_INVALID_ARG);
        REQUIRE(vsi_plan("driver", 64, 64, 3, 0, &p, nullptr) == SR_ERR_INVALID_ARG);         // the metric's form needs room for tables
        REQUIRE(vsi_plan("driver", 70000, 8, 3, 1, &p, nullptr) == SR_ERR_UNSUPPORTED);       // rows of one launch
    }
    // refusals
    REQUIRE(sr_vsi_plan(64, 64, 2, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_vsi_plan(64, 64, 0, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_vsi_plan(0, 64, 3, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_vsi_plan(64, -5, 3, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    // axis tables into exact-size buffers
    for (int n_in : {1, 2, 16, 255, 256, 257, 2000, 14142})
        for (int n_out : {1, 16, 17, 255, 256, 257, 641}) {
            int taps = 0;
            REQUIRE(sr_vsi_resize_weights(n_in, n_out, 0, &taps, nullptr, nullptr) == SR_OK && taps >= 1);
            std::vector<double> w((size_t)n_out * taps);
            std::vector<int32_t> idx((size_t)n_out * taps);
            REQUIRE(sr_vsi_resize_weights(n_in, n_out, taps, &taps, w.data(), idx.data()) == SR_OK);
            REQUIRE(sr_vsi_resize_weights(n_in, n_out, taps - 1, &taps, w.data(), idx.data()) == SR_ERR_INVALID_ARG);
            REQUIRE(sr_vsi_resize_weights(n_in, n_out, taps, &taps, w.data(), nullptr) == SR_ERR_INVALID_ARG);
            for (size_t k = 0; k < idx.size(); ++k) REQUIRE(idx[k] >= 0 && idx[k] < n_in);
        }
    {
        int taps = 0;
        REQUIRE(sr_vsi_resize_weights(2000, 256, 0, &taps, nullptr, nullptr) == SR_OK && taps == 18);
        REQUIRE(sr_vsi_resize_weights(256, 16, 0, &taps, nullptr, nullptr) == SR_OK && taps == 34);
        REQUIRE(sr_vsi_resize_weights(256, 256, 0, &taps, nullptr, nullptr) == SR_OK && taps == 4);       // P: no tap is trimmed
        REQUIRE(sr_vsi_resize_weights(0, 256, 0, &taps, nullptr, nullptr) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_vsi_resize_weights(256, 0, 0, &taps, nullptr, nullptr) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_vsi_resize_weights(256, 16, 0, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    }
    // LG and SD into exact-size buffers, each alone too
    {
        std::vector<double> lg(VSI_NN), sd(VSI_NN);
        REQUIRE(sr_vsi_filter(lg.data(), sd.data()) == SR_OK && sr_vsi_filter(lg.data(), nullptr) == SR_OK);
        REQUIRE(sr_vsi_filter(nullptr, sd.data()) == SR_OK && sr_vsi_filter(nullptr, nullptr) == SR_OK);
        REQUIRE(lg[0] == 0.0 && lg[(size_t)128 * VSI_N + 128] == 0.0 && sd[(size_t)127 * VSI_N + 127] == 1.0);
        for (int i = 0; i < VSI_NN; ++i) REQUIRE(lg[i] >= 0.0 && lg[i] <= 1.0 && sd[i] > 0.0 && sd[i] <= 1.0);
    }
    // values
    {
        sr_vsi_sums rec = {};
        rec.sum_s = 3.0;
        rec.sum_w = 4.0;
        REQUIRE(sr_vsi_value(&rec) == 0.75 && std::isnan(sr_vsi_value(nullptr)));
        rec.sum_s = rec.sum_w = 0.0;
        REQUIRE(std::isnan(sr_vsi_value(&rec)));
        REQUIRE(sr_vsi_chroma_weight(1.0) == 1.0 && sr_vsi_chroma_weight(0.0) == 0.0);
        REQUIRE(std::fabs(sr_vsi_chroma_weight(-0.25) - std::pow(0.25, 0.02) * std::cos(0.02 * 3.14159265358979323846)) <= 1e-16);
    }
    // the whole metric on exact-size heap images: both pass orders, a side that shrinks in the up-resize, F = 2, four channels
    // behind a stride, a black pair
    const int shapes[][3] = {{17, 33, 4}, {40, 16, 3}, {384, 390, 3}};
    for (const auto &sh : shapes) {
        const int h = sh[0], w = sh[1], cn = sh[2];
        const size_t stride = (size_t)w * cn + (cn == 4 ? 5 : 0);
        std::vector<unsigned char> a(stride * (h - 1) + (size_t)w * cn), b(a.size());
        uint32_t s = 12345u + (uint32_t)(h * 131 + w);
        for (size_t i = 0; i < a.size(); ++i) {
            s = s * 1664525u + 1013904223u;
            a[i] = (unsigned char)(s >> 24);
            b[i] = (unsigned char)((s >> 16) & 0xFF);
        }
        sr_vsi_sums ab = {}, aa = {};
        REQUIRE(sr_vsi_host_u8(a.data(), (int64_t)stride, b.data(), (int64_t)stride, h, w, cn, &ab) == SR_OK);
        const double v = sr_vsi_value(&ab);
        REQUIRE(v > 0.0 && v < 1.0);
        if (cn == 4) {
            REQUIRE(sr_vsi_host_u8(a.data(), (int64_t)stride, a.data(), (int64_t)stride, h, w, cn, &aa) == SR_OK);
            REQUIRE(std::fabs(sr_vsi_value(&aa) - 1.0) <= 1e-12);
        }
        REQUIRE(ab.F == fsim_auto_f(h, w) && ab.count == (uint64_t)ab.rows * ab.cols && ab.vs_range[0][0] < ab.vs_range[0][1]);
        REQUIRE(sr_vsi_host_u8(a.data(), (int64_t)w * cn - 1, b.data(), (int64_t)stride, h, w, cn, &ab) == SR_ERR_SHAPE);
        REQUIRE(sr_vsi_host_u8(nullptr, (int64_t)stride, b.data(), (int64_t)stride, h, w, cn, &ab) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_vsi_host_u8(a.data(), (int64_t)stride, b.data(), (int64_t)stride, h, w, cn, nullptr) == SR_ERR_INVALID_ARG);
    }
    {
        std::vector<unsigned char> z((size_t)24 * 31 * 3, 0);
        sr_vsi_sums rec = {};
        REQUIRE(sr_vsi_host_u8(z.data(), 93, z.data(), 93, 24, 31, 3, &rec) == SR_OK && std::isnan(sr_vsi_value(&rec)));
        REQUIRE(sr_vsi_host_u8(z.data(), 31, z.data(), 31, 24, 31, 1, &rec) == SR_ERR_UNSUPPORTED);
        REQUIRE(sr_vsi_host_u8(z.data(), 93, z.data(), 93, 15, 31, 3, &rec) == SR_ERR_SHAPE);
    }
    printf("vsi-driver-ok\n");
    return 0;
}
