// brisque_driver.cpp -- stand-alone driver for the sanitizer run of the host side of BRISQUE (tests/test_brisque_sanitize.py):
// compiled with csrc/sr_brisque_host.cpp alone under -fsanitize=address,undefined, it takes seeded scale records through
// sr_brisque_features -> sr_brisque_score with exact-size heap buffers, degenerate records and every refusal included.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "sr_internal.h"

static char g_err[512] = "";

// sr_host.cpp owns this in the library; the driver links sr_brisque_host.cpp alone
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
            fprintf(stderr, "brisque_driver: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

// moments of n samples of an asymmetric generalised-Gaussian-like variable
static sr_niqe_moments draw_moments(std::mt19937_64 &rng, int n, double shape)
{
    std::normal_distribution<double> nd(0.0, 1.0);
    std::uniform_real_distribution<double> ud(0.5, 1.5);
    const double ls = ud(rng), rs = ud(rng);
    sr_niqe_moments m = {0, 0, 0.0, 0.0, 0.0};
    for (int i = 0; i < n; ++i) {
        double v = nd(rng);
        v = (v < 0 ? -ls : rs) * std::pow(std::fabs(v), shape);
        if (v < 0) {
            ++m.n_neg;
            m.ssq_neg += v * v;
        } else if (v > 0) {
            ++m.n_pos;
            m.ssq_pos += v * v;
        }
        m.sabs += std::fabs(v);
    }
    return m;
}

int main()
{
    std::mt19937_64 rng(20261019);
    int H = 0, W = 0, H2 = 0, W2 = 0;
    size_t bytes = 0;
    REQUIRE(sr_brisque_plan(200, 301, 3, 3, &H, &W, &H2, &W2, &bytes) == SR_OK && H == 194 && W == 295 && H2 == 97 && W2 == 148);
    REQUIRE(bytes >= (size_t)(97 * 148 * 4) + (20 + 6) * 25 * sizeof(double));
    REQUIRE(sr_brisque_plan(16, 16, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    REQUIRE(sr_brisque_plan(15, 16, 1, 0, &H, &W, &H2, &W2, &bytes) == SR_ERR_SHAPE);
    REQUIRE(sr_brisque_plan(16, 17, 1, 1, &H, &W, &H2, &W2, &bytes) == SR_ERR_SHAPE);
    REQUIRE(sr_brisque_plan(200, 200, 2, 0, &H, &W, &H2, &W2, &bytes) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_brisque_plan(200, 200, 3, -1, &H, &W, &H2, &W2, &bytes) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_brisque_plan(0, 200, 3, 0, &H, &W, &H2, &W2, &bytes) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_brisque_plan(2147483647, 2147483647, 3, 1073741820, &H, &W, &H2, &W2, &bytes) == SR_ERR_SHAPE);
    REQUIRE(sr_brisque_plan(2147483647, 2147483647, 3, 0, &H, &W, &H2, &W2, &bytes) == SR_OK && H2 == 1073741824);

    std::vector<sr_brisque_record> rec(2);
    for (int s = 0; s < 2; ++s) {
        rec[s].n = s == 0 ? 9216 : 2304;
        for (int x = 0; x < 5; ++x) rec[s].x[x] = draw_moments(rng, (int)rec[s].n, 0.7 + 0.1 * x);
    }
    std::vector<double> feat(36);
    REQUIRE(sr_brisque_features(rec.data(), feat.data()) == SR_OK);
    for (int k = 0; k < 36; ++k) REQUIRE(std::isfinite(feat[k]));
    REQUIRE(feat[0] >= 0.2 && feat[0] <= 10.0 && feat[1] > 0.0 && feat[4] > 0.0 && feat[5] > 0.0);
    REQUIRE(sr_brisque_features(nullptr, feat.data()) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_brisque_features(rec.data(), nullptr) == SR_ERR_INVALID_ARG);
    {   // degenerate records
        std::vector<sr_brisque_record> bad = rec;
        std::vector<double> f(36);
        bad[0].x[0] = {0, 0, 0.0, 0.0, 0.0};                            // a flat plane: no GGD
        bad[0].x[2].n_neg = 0;                                          // no negative sample
        bad[1].x[4].n_pos = 0;                                          // no positive sample
        bad[1].x[1] = {1152, 1152, 1152.0, 1152.0, 2304.0};             // above the table
        bad[1].x[3] = {1, 2303, 1e-300, 1e300, 1e154};                  // extreme ratios
        bad[1].x[0] = {1152, 1152, 1.152e12, 1.152e12, 2304.0};         // the GGD ratio far above its table
        REQUIRE(sr_brisque_features(bad.data(), f.data()) == SR_OK);
        REQUIRE(std::isnan(f[0]) && std::isnan(f[1]) && std::isnan(f[6]) && std::isnan(f[18 + 14]));
        REQUIRE(f[18 + 2] == 0.2 + 0.001 * 9800 && f[18] == 0.2 && !std::isnan(f[2]));
        bad[0].n = 0;
        REQUIRE(sr_brisque_features(bad.data(), f.data()) == SR_ERR_INVALID_ARG);
    }

    // the regressor: exact-size buffers
    const int n_sv = 17;
    std::uniform_real_distribution<double> ud(-1.0, 1.0);
    std::vector<double> sv((size_t)n_sv * 36), coef(n_sv), fmin(36), fmax(36);
    for (double &v : sv) v = ud(rng);
    for (double &v : coef) v = 10.0 * ud(rng);
    for (int k = 0; k < 36; ++k) {
        fmin[k] = feat[k] - 1.0 - ud(rng) * 0.5;
        fmax[k] = feat[k] + 1.0 + ud(rng) * 0.5;
    }
    const double s0 = sr_brisque_score(feat.data(), sv.data(), coef.data(), n_sv, 0.05, -40.0, fmin.data(), fmax.data(), -1.0, 1.0);
    REQUIRE(std::isfinite(s0));
    {   // by hand
        double want = 0.0;
        for (int i = 0; i < n_sv; ++i) {
            double d2 = 0.0;
            for (int k = 0; k < 36; ++k) {
                const double x = -1.0 + 2.0 * (feat[k] - fmin[k]) / (fmax[k] - fmin[k]);
                d2 += (sv[(size_t)i * 36 + k] - x) * (sv[(size_t)i * 36 + k] - x);
            }
            want += coef[i] * std::exp(-0.05 * d2);
        }
        REQUIRE(std::fabs(s0 - (want + 40.0)) <= 1e-12 * std::fabs(s0));
    }
    {   // a zero-range feature scales to 0; a NaN feature gives NaN
        std::vector<double> lo = fmin, f = feat;
        lo[7] = fmax[7];
        REQUIRE(std::isfinite(sr_brisque_score(feat.data(), sv.data(), coef.data(), n_sv, 0.05, 0.0, lo.data(), fmax.data(), -1.0, 1.0)));
        f[35] = std::nan("");
        REQUIRE(std::isnan(sr_brisque_score(f.data(), sv.data(), coef.data(), n_sv, 0.05, 0.0, fmin.data(), fmax.data(), -1.0, 1.0)));
    }
    const double inf = std::numeric_limits<double>::infinity();
    REQUIRE(std::isnan(sr_brisque_score(nullptr, sv.data(), coef.data(), n_sv, 0.05, 0.0, fmin.data(), fmax.data(), -1.0, 1.0)));
    REQUIRE(std::isnan(sr_brisque_score(feat.data(), sv.data(), coef.data(), n_sv, 0.05, 0.0, nullptr, fmax.data(), -1.0, 1.0)));
    REQUIRE(std::isnan(sr_brisque_score(feat.data(), sv.data(), coef.data(), 0, 0.05, 0.0, fmin.data(), fmax.data(), -1.0, 1.0)));
    REQUIRE(std::isnan(sr_brisque_score(feat.data(), sv.data(), coef.data(), n_sv, 0.0, 0.0, fmin.data(), fmax.data(), -1.0, 1.0)));
    REQUIRE(std::isnan(sr_brisque_score(feat.data(), sv.data(), coef.data(), n_sv, inf, 0.0, fmin.data(), fmax.data(), -1.0, 1.0)));
    REQUIRE(std::isnan(sr_brisque_score(feat.data(), sv.data(), coef.data(), n_sv, std::nan(""), 0.0, fmin.data(), fmax.data(), -1.0, 1.0)));
    printf("brisque-driver-ok %.17g\n", s0);
    return 0;
}
