// vif_gmsd_driver.cpp -- stand-alone driver for the sanitizer run of the host side of VIF and GMSD
// (tests/test_vif_sanitize.py): compiled with csrc/sr_vif_host.cpp alone under -fsanitize=address,undefined, it takes
// sr_vif_plan, sr_vif_window, sr_vif_value, sr_gmsd_plan and sr_gmsd_value through sizes, crops, modes and every refusal with
// exact-size heap buffers, and checks each plan the way the kernels use it: every launch covers its plane, every plane and the
// partials lie inside the scratch and do not overlap.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "sr_vif.h"

static char g_err[512] = "";

// sr_host.cpp owns this in the library; the driver links sr_vif_host.cpp alone
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
            fprintf(stderr, "vif_gmsd_driver: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

static int covers(const VifLaunch &l, int rows, int cols, int per_block)
{
    REQUIRE(l.step >= 1 && l.gx >= 1 && l.gy >= 1);
    REQUIRE((long long)l.gx * l.step >= rows && (long long)(l.gx - 1) * l.step < rows);     // no empty chunk
    REQUIRE((long long)l.gy * per_block >= cols && (long long)(l.gy - 1) * per_block < cols);
    REQUIRE(l.step <= VIF_ROWS);
    return 0;
}

static int one_vif(int h, int w, int cn, int cb, int mode)
{
    std::vector<int> sh(VIF_SCALES), sw(VIF_SCALES);
    std::vector<uint64_t> cnt(VIF_SCALES);
    size_t bytes = 0;
    const int rc = sr_vif_plan(h, w, cn, cb, mode, sh.data(), sw.data(), cnt.data(), &bytes);
    const long long ch = (long long)h - 2LL * cb, cw = (long long)w - 2LL * cb;
    if (ch < VIF_MIN_SIDE || cw < VIF_MIN_SIDE) {
        REQUIRE(rc == SR_ERR_SHAPE);
        return 0;
    }
    REQUIRE(rc == SR_OK);
    REQUIRE(sr_vif_plan(h, w, cn, cb, mode, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    VifPlan p;
    REQUIRE(vif_plan("driver", h, w, cn, cb, mode, &p) == SR_OK);
    REQUIRE(p.total == bytes);
    size_t end = 0;
    for (int s = 0; s < VIF_SCALES; ++s) {
        const VifScale &v = p.s[s];
        REQUIRE(v.n == (16 >> s) + 1 && v.h == sh[s] && v.w == sw[s] && v.count == cnt[s]);
        REQUIRE(v.mh >= 1 && v.mw >= 1 && v.count == (uint64_t)v.mh * (uint64_t)v.mw);
        if (covers(v.stats, v.mh, v.mw, vif_stats_out(v.stats.tx, v.n))) return 1;
        REQUIRE((size_t)v.stats.gx * v.stats.gy <= p.nblk);
        if (s == 0) continue;
        const VifScale &u = p.s[s - 1];
        REQUIRE(v.h == (u.h - (v.n - 1) + 1) / 2 && v.w == (u.w - (v.n - 1) + 1) / 2);
        REQUIRE(2 * (v.h - 1) + v.n - 1 <= u.h - 1 && 2 * (v.w - 1) + v.n - 1 <= u.w - 1);     // the last window lies inside
        if (covers(v.down, v.h, v.w, vif_down_out(v.down.tx, v.n))) return 1;
        const size_t plane = (size_t)v.h * (size_t)v.w * sizeof(double);
        REQUIRE(v.off_x % 256 == 0 && v.off_y % 256 == 0 && v.off_x >= end && v.off_y >= v.off_x + plane);
        end = v.off_y + plane;
    }
    REQUIRE(p.off_part % 256 == 0 && p.off_part >= end && p.off_buf0 >= p.off_part + p.nblk * 2 * sizeof(double));
    REQUIRE(p.off_buf1 >= p.off_buf0 + ((p.nblk + 1023) / 1024) * 2 * sizeof(double) && p.total >= p.off_buf1 + (p.off_buf1 - p.off_buf0));
    return 0;
}

static int one_gmsd(int h, int w, int cn, int cb, int mode)
{
    int mh = 0, mw = 0;
    uint64_t cnt = 0;
    size_t bytes = 0;
    const int rc = sr_gmsd_plan(h, w, cn, cb, mode, &mh, &mw, &cnt, &bytes);
    const long long ch = (long long)h - 2LL * cb, cw = (long long)w - 2LL * cb;
    if (ch < GMSD_MIN_SIDE || cw < GMSD_MIN_SIDE) {
        REQUIRE(rc == SR_ERR_SHAPE);
        return 0;
    }
    REQUIRE(rc == SR_OK && mh == (ch + 1) / 2 && mw == (cw + 1) / 2 && cnt == (uint64_t)mh * (uint64_t)mw);
    REQUIRE(sr_gmsd_plan(h, w, cn, cb, mode, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    GmsdPlan p;
    REQUIRE(gmsd_plan("driver", h, w, cn, cb, mode, &p) == SR_OK);
    REQUIRE(p.tiles_x * GMSD_TW >= mw && (p.tiles_x - 1) * GMSD_TW < mw && p.tiles_y * GMSD_TH >= mh && (p.tiles_y - 1) * GMSD_TH < mh);
    REQUIRE(p.total == bytes && p.off_buf0 >= (size_t)p.tiles_x * p.tiles_y * 2 * sizeof(double));
    return 0;
}

int main()
{
    const int sides[] = {1, 3, 4, 5, 7, 40, 41, 42, 43, 57, 64, 97, 130, 255, 256, 257, 264, 265, 520, 521, 1052, 4097, 20011};
    for (int h : sides)
        for (int w : sides)
            for (int cb = 0; cb <= 3; ++cb)
                for (int mode = 0; mode < 3; ++mode) {
                    const int cn = mode == SR_BENCH_CHANNELS ? 1 : 3;
                    if (one_vif(h, w, cn, cb, mode) || one_gmsd(h, w, cn, cb, mode)) return 1;
                }
    // the largest sides an int holds: the sizes are formed in 64 bits
    REQUIRE(sr_vif_plan(2147483647, 41, 1, 0, 0, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    REQUIRE(sr_vif_plan(41, 2147483647, 1, 0, 0, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);      // one launch's columns
    REQUIRE(sr_vif_plan(2147483647, 2147483647, 3, 1073741800, 1, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    REQUIRE(sr_gmsd_plan(2147483647, 2147483647, 1, 0, 0, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    REQUIRE(sr_gmsd_plan(2147483647, 4, 1, 0, 0, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    // The chunk cut on both sides of the VIF_BLOCKS threshold (one column block): 131100 rows give every chunk length from
    // VIF_ROWS down to VIF_ROWS_MIN over the four scales, 130960 rows stay one block short at every scale and take the next
    // shorter chunk.  tests/test_gpu_vif.py runs both shapes.
    {
        VifPlan t, u;
        REQUIRE(vif_plan("driver", 131100, 41, 1, 0, 0, &t) == SR_OK && vif_plan("driver", 130960, 41, 1, 0, 0, &u) == SR_OK);
        const int want_t[VIF_SCALES] = {128, 64, 32, 16}, want_u[VIF_SCALES] = {64, 32, 16, 16};
        for (int s = 0; s < VIF_SCALES; ++s) {
            REQUIRE(t.s[s].stats.gy == 1 && t.s[s].stats.step == want_t[s] && t.s[s].stats.gx >= VIF_BLOCKS);
            REQUIRE(u.s[s].stats.gy == 1 && u.s[s].stats.step == want_u[s]);
            REQUIRE((u.s[s].mh + 2 * want_u[s] - 1) / (2 * want_u[s]) < VIF_BLOCKS || want_u[s] == VIF_ROWS_MIN);
        }
        REQUIRE(u.s[3].stats.gx == VIF_BLOCKS - 1);
        REQUIRE(t.s[1].down.step == 64 && t.s[2].down.step == 32 && t.s[3].down.step == 16);
    }
    // refusals
    REQUIRE(sr_vif_plan(64, 64, 2, 0, 0, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_vif_plan(64, 64, 3, 0, 0, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_vif_plan(64, 64, 1, 0, 1, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_vif_plan(64, 64, 3, -1, 1, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_vif_plan(64, 64, 3, 0, 3, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_vif_plan(0, 64, 3, 0, 1, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_gmsd_plan(64, 64, 3, 0, 0, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    // windows into exact-size buffers
    for (int s = 1; s <= VIF_SCALES; ++s) {
        const int n = (32 >> s) + 1;
        std::vector<double> t((size_t)n);
        REQUIRE(sr_vif_window(s, t.data()) == SR_OK);
        double sum = 0.0;
        for (int k = 0; k < n; ++k) {
            REQUIRE(t[k] > 0.0 && t[k] == t[n - 1 - k]);
            sum += t[k];
        }
        REQUIRE(std::fabs(sum - 1.0) <= 1e-15);
    }
    REQUIRE(sr_vif_window(0, nullptr) == SR_ERR_INVALID_ARG && sr_vif_window(5, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_vif_window(1, nullptr) == SR_ERR_INVALID_ARG);
    // values
    std::vector<sr_vif_scale> rec(VIF_SCALES);
    for (int s = 0; s < VIF_SCALES; ++s) rec[s] = {1.0 + s, 2.0 + s, 10};
    REQUIRE(sr_vif_value(rec.data(), VIF_SCALES) == 10.0 / 14.0);
    REQUIRE(std::isnan(sr_vif_value(rec.data(), 3)) && std::isnan(sr_vif_value(nullptr, VIF_SCALES)));
    for (int s = 0; s < VIF_SCALES; ++s) rec[s] = {0.0, 0.0, 10};
    REQUIRE(std::isnan(sr_vif_value(rec.data(), VIF_SCALES)));
    sr_gmsd_sums g = {6.0, 14.0, 3};                                    // d = 1, 2, 3: variance 1
    REQUIRE(sr_gmsd_value(&g) == 1.0);
    g = {3.0, 3.0, 3};
    REQUIRE(sr_gmsd_value(&g) == 0.0);
    g = {1.0, 1.0, 1};
    REQUIRE(std::isnan(sr_gmsd_value(&g)) && std::isnan(sr_gmsd_value(nullptr)));
    printf("vif-gmsd-driver-ok\n");
    return 0;
}
