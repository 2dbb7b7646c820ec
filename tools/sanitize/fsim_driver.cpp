// fsim_driver.cpp -- stand-alone driver for the sanitizer run of the host side of FSIM (tests/test_fsim_sanitize.py): compiled
// with csrc/sr_fsim_host.cpp alone under -fsanitize=address,undefined, it takes sr_fsim_plan, sr_fsim_filters, sr_fsim_value,
// sr_fsim_chroma_weight and the twiddle tables through sizes up to the largest an int holds and every refusal with exact-size
// heap buffers, and checks each plan the way the kernels use it: the pooling launch covers the pooled plane, every window
// lies inside a block's segment, every section lies inside the workspace and none overlaps the next.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sr_fsim.h"

static char g_err[512] = "";

// sr_host.cpp owns this in the library; the driver links sr_fsim_host.cpp alone
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
            fprintf(stderr, "fsim_driver: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

static int check_layout(const FsimPlan &p)
{
    const size_t n = p.n, d = sizeof(double);
    REQUIRE(n == (size_t)p.rows * (size_t)p.cols);
    const size_t off[] = {p.off_pool, p.off_filt, p.off_tw_r, p.off_tw_c, p.off_plane, p.off_spec, p.off_half, p.off_eo, p.off_pc,
                          p.off_energy_all, p.off_an_all, p.off_energy, p.off_e2, p.off_hist, p.off_med, p.off_part, p.off_buf0,
                          p.off_buf1, p.total};
    const size_t need[] = {6 * n * 8, 8 * n * d, (size_t)p.rows * 2 * d, (size_t)p.cols * 2 * d, n * d, 2 * n * d, 8 * n * d, 8 * n * d,
                           2 * n * d, n * d, n * d, n * d, n * d, 2 * 256 * 4 + 24, 16 * d, p.score_blocks * 3 * d,
                           ((p.score_blocks + 1023) / 1024) * 3 * d, ((p.score_blocks + 1023) / 1024) * 3 * d};
    for (int k = 0; k < 18; ++k) REQUIRE(off[k] % 256 == 0 && off[k] + need[k] <= off[k + 1]);
    REQUIRE(p.score_blocks * FSIM_THREADS >= n && (p.score_blocks - 1) * FSIM_THREADS < n);
    // the pooling launch: pool_gx blocks of floor(256 / F) windows cover the columns; a block's windows lie in its segment
    const int out = fsim_pool_out(p.F);
    REQUIRE(out >= 1 && (long long)p.pool_gx * out >= p.cols && (long long)(p.pool_gx - 1) * out < p.cols);
    REQUIRE(out * p.F <= FSIM_POOL_THREADS);
    REQUIRE(fsim_win_start(p.rows - 1, p.F) < p.h && fsim_win_start(p.cols - 1, p.F) < p.w);      // no window is empty
    REQUIRE(fsim_win_start(0, p.F) + p.F - 1 >= 0);
    return 0;
}

static int one(int h, int w, int cn)
{
    int F = 0, rows = 0, cols = 0;
    size_t bytes = 0;
    const int rc = sr_fsim_plan(h, w, cn, &F, &rows, &cols, &bytes);
    if (h < FSIM_MIN_SIDE || w < FSIM_MIN_SIDE) {
        REQUIRE(rc == SR_ERR_SHAPE);
        return 0;
    }
    const int f = fsim_auto_f(h, w);
    REQUIRE(f == (int)std::floor((double)(h < w ? h : w) / 256.0 + 0.5) || f == 1);
    const long long lr = ((long long)h + f - 1) / f, lc = ((long long)w + f - 1) / f;
    if (f > FSIM_MAX_F || lr > FSIM_MAX_SIDE || lc > FSIM_MAX_SIDE) {
        REQUIRE(rc == SR_ERR_UNSUPPORTED);
        return 0;
    }
    REQUIRE(rc == SR_OK && F == f && rows == lr && cols == lc);
    REQUIRE(sr_fsim_plan(h, w, cn, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    FsimPlan p;
    REQUIRE(fsim_plan("driver", h, w, cn, 0, &p) == SR_OK && p.total == bytes);
    return check_layout(p);
}

int main()
{
    const int sides[] = {1, 15, 16, 17, 23, 64, 255, 256, 383, 384, 385, 639, 640, 895, 896, 2048, 2049, 4097, 20011, 524288, 2147483647};
    for (int h : sides)
        for (int w : sides)
            for (int cn : {1, 3, 4})
                if (one(h, w, cn)) return 1;
    REQUIRE(fsim_auto_f(383, 9999) == 1 && fsim_auto_f(384, 9999) == 2 && fsim_auto_f(9999, 639) == 2 && fsim_auto_f(640, 640) == 3);
    REQUIRE(fsim_auto_f(895, 900) == 3 && fsim_auto_f(896, 900) == 4 && fsim_auto_f(16, 16) == 1);
    // the inspection form: any F in 1 .. 256 on any size
    for (int F : {1, 2, 3, 4, 5, 8, 85, 86, 128, 129, 200, 256})
        for (int h : {1, 13, 16, 300})
            for (int w : {1, 19, 255, 256, 257, 610}) {
                FsimPlan p;
                REQUIRE(fsim_plan("driver", h, w, 3, F, &p) == SR_OK && p.F == F);
                REQUIRE(p.rows == (h + F - 1) / F && p.cols == (w + F - 1) / F);
                if (check_layout(p)) return 1;
            }
    {
        FsimPlan p;
        REQUIRE(fsim_plan("driver", 64, 64, 3, 257, &p) == SR_ERR_INVALID_ARG && fsim_plan("driver", 64, 64, 3, -1, &p) == SR_ERR_INVALID_ARG);
        REQUIRE(fsim_plan("driver", 70000, 8, 1, 1, &p) == SR_ERR_UNSUPPORTED);       // rows of one launch
        REQUIRE(fsim_plan_plane("driver", 15, 16, &p) == SR_ERR_SHAPE && fsim_plan_plane("driver", 16, 2049, &p) == SR_ERR_UNSUPPORTED);
        REQUIRE(fsim_plan_plane("driver", 2048, 2048, &p) == SR_OK && p.F == 1 && p.rows == 2048 && p.cols == 2048);
        if (check_layout(p)) return 1;
    }
    // refusals
    REQUIRE(sr_fsim_plan(64, 64, 2, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_fsim_plan(64, 64, 0, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_fsim_plan(0, 64, 3, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_fsim_plan(64, -5, 3, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_fsim_plan(15, 64, 3, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    REQUIRE(sr_fsim_plan(100, 2049, 3, nullptr, nullptr, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
    REQUIRE(sr_fsim_filters(15, 16, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    REQUIRE(sr_fsim_filters(16, 2049, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
    // filters into exact-size buffers, every combination of outputs; odd, even and mixed sides
    const int shapes[][2] = {{16, 16}, {17, 23}, {16, 19}, {33, 32}, {64, 65}};
    for (const auto &sh : shapes) {
        const int rows = sh[0], cols = sh[1];
        const size_t n = (size_t)rows * cols;
        std::vector<double> lg(4 * n), sp(4 * n), em(4), s2(4), sij(4), em2(4), s22(4), sij2(4);
        REQUIRE(sr_fsim_filters(rows, cols, lg.data(), sp.data(), em.data(), s2.data(), sij.data()) == SR_OK);
        REQUIRE(sr_fsim_filters(rows, cols, nullptr, nullptr, em2.data(), s22.data(), sij2.data()) == SR_OK);
        REQUIRE(sr_fsim_filters(rows, cols, lg.data(), nullptr, nullptr, nullptr, nullptr) == SR_OK);
        REQUIRE(sr_fsim_filters(rows, cols, nullptr, sp.data(), nullptr, nullptr, nullptr) == SR_OK);
        for (int o = 0; o < 4; ++o) {
            REQUIRE(em[o] == em2[o] && s2[o] == s22[o] && sij[o] == sij2[o]);
            REQUIRE(em[o] > 0.0 && s2[o] > 0.0 && std::isfinite(sij[o]));
            REQUIRE(sp[o * n] > 0.0 && sp[o * n] <= 1.0);
        }
        for (int s = 0; s < 4; ++s) {
            REQUIRE(lg[s * n] == 0.0);                                  // DC
            for (size_t i = 0; i < n; ++i) REQUIRE(lg[s * n + i] >= 0.0 && lg[s * n + i] <= 1.0 && sp[s * n + i] > 0.0 && sp[s * n + i] <= 1.0);
        }
    }
    // twiddles into exact-size buffers
    for (int n : {1, 2, 16, 17, 383, 2048}) {
        std::vector<double> tw(2 * (size_t)n);
        fsim_twiddles(n, tw.data());
        REQUIRE(tw[0] == 1.0 && tw[1] == 0.0);
        for (int j = 0; j < n; ++j) REQUIRE(std::fabs(tw[2 * j] * tw[2 * j] + tw[2 * j + 1] * tw[2 * j + 1] - 1.0) <= 4e-16);
        if (n % 4 == 0) REQUIRE(tw[2 * (n / 4)] == 0.0 || std::fabs(tw[2 * (n / 4)]) < 1e-16);
        if (n % 2 == 0) REQUIRE(tw[2 * (n / 2)] == -1.0);
    }
    // values
    sr_fsim_sums rec = {3.0, 2.0, 4.0, 10, 1, 2, 5, 0};
    double v = 0.0, vc = 0.0;
    REQUIRE(sr_fsim_value(&rec, &v, &vc) == SR_OK && v == 0.75 && vc == 0.5);
    REQUIRE(sr_fsim_value(&rec, nullptr, nullptr) == SR_OK && sr_fsim_value(nullptr, &v, &vc) == SR_ERR_INVALID_ARG);
    rec.sum_s = rec.sum_sc = rec.sum_pcm = 0.0;
    REQUIRE(sr_fsim_value(&rec, &v, &vc) == SR_OK && std::isnan(v) && std::isnan(vc));
    REQUIRE(sr_fsim_chroma_weight(1.0, 1.0) == 1.0 && sr_fsim_chroma_weight(0.0, 0.5) == 0.0);
    REQUIRE(std::fabs(sr_fsim_chroma_weight(-0.5, 0.5) - std::pow(0.25, 0.03) * std::cos(0.03 * 3.14159265358979323846)) <= 1e-16);
    REQUIRE(sr_fsim_chroma_weight(-0.5, -0.5) == std::pow(0.25, 0.03));
    printf("fsim-driver-ok\n");
    return 0;
}
