// niqe_driver.cpp -- stand-alone driver for the sanitizer run of the host side of NIQE (tests/test_niqe_sanitize.py): compiled
// with csrc/sr_niqe_host.cpp alone under -fsanitize=address,undefined, it takes seeded block records through
// sr_niqe_features -> sr_niqe_fit -> sr_niqe_score with exact-size heap buffers, degenerate records and every refusal included.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "sr_internal.h"

static char g_err[512] = "";

// sr_host.cpp owns this in the library; the driver links sr_niqe_host.cpp alone
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
            fprintf(stderr, "niqe_driver: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
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
    std::mt19937_64 rng(20260607);
    int H = 0, W = 0, nby = 0, nbx = 0;
    size_t bytes = 0;
    REQUIRE(sr_niqe_plan(200, 301, 3, 3, &H, &W, &nby, &nbx, &bytes) == SR_OK && H == 192 && W == 288 && nby == 2 && nbx == 3);
    REQUIRE(bytes >= (size_t)(96 * 144 * 4 + 12 * sizeof(sr_niqe_block)));
    REQUIRE(sr_niqe_plan(96, 96, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    REQUIRE(sr_niqe_plan(95, 96, 1, 0, &H, &W, &nby, &nbx, &bytes) == SR_ERR_SHAPE);
    REQUIRE(sr_niqe_plan(200, 200, 2, 0, &H, &W, &nby, &nbx, &bytes) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_niqe_plan(200, 200, 3, -1, &H, &W, &nby, &nbx, &bytes) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_niqe_plan(2147483647, 2147483647, 3, 1073741800, &H, &W, &nby, &nbx, &bytes) == SR_ERR_SHAPE);
    REQUIRE(sr_niqe_plan(2147483647, 2147483647, 3, 0, &H, &W, &nby, &nbx, &bytes) == SR_OK && nby == 22369621);

    // three "images" of 20, 24 and 1 blocks
    const int counts[3] = {20, 24, 1};
    std::vector<std::vector<double>> feats, sharps;
    for (int img = 0; img < 3; ++img) {
        const int nb = counts[img];
        std::vector<sr_niqe_block> rec((size_t)2 * nb);
        for (int s = 0; s < 2; ++s)
            for (int b = 0; b < nb; ++b) {
                sr_niqe_block &r = rec[(size_t)s * nb + b];
                for (int x = 0; x < 5; ++x) r.x[x] = draw_moments(rng, s == 0 ? 9216 : 2304, 0.6 + 0.05 * ((b + x) % 20));
                r.sum_sigma = 9216.0 * (10.0 + (double)((b * 7 + img) % 11));
            }
        if (img == 0) {                                     // degenerate records
            rec[3].x[2].n_neg = 0;                          // no negative sample
            rec[(size_t)nb + 5].x[0].n_pos = 0;             // no positive sample
            rec[7].x[4] = {0, 0, 0.0, 0.0, 0.0};            // an all-zero block
            rec[8].x[1] = {4608, 4608, 4608.0, 4608.0, 9216.0};             // above the table
            rec[9].x[1] = {4608, 4608, 4.608e12, 4.608e12, 9216.0};         // below the table
            rec[10].x[3] = {1, 9215, 1e-300, 1e300, 1e154};                 // extreme ratios
        }
        std::vector<double> f((size_t)nb * 36), sh((size_t)nb);
        REQUIRE(sr_niqe_features(rec.data(), nb, f.data()) == SR_OK);
        for (int b = 0; b < nb; ++b) sh[b] = rec[b].sum_sigma / 9216.0;
        if (img == 0) {
            REQUIRE(std::isnan(f[3 * 36 + 6]) && std::isnan(f[5 * 36 + 18]) && std::isnan(f[7 * 36 + 14]));
            REQUIRE(f[8 * 36 + 2] == 0.2 + 0.001 * 9800 && f[9 * 36 + 2] == 0.2);
            REQUIRE(!std::isnan(f[0]) && !std::isnan(f[35]));
        }
        feats.push_back(f);
        sharps.push_back(sh);
    }
    REQUIRE(sr_niqe_features(nullptr, 1, feats[0].data()) == SR_ERR_INVALID_ARG);

    // pooled fit: exact-size buffers
    std::vector<double> rows, sharp;
    std::vector<int64_t> off = {0};
    for (int img = 0; img < 3; ++img) {
        rows.insert(rows.end(), feats[img].begin(), feats[img].end());
        sharp.insert(sharp.end(), sharps[img].begin(), sharps[img].end());
        off.push_back(off.back() + counts[img]);
    }
    std::vector<double> mu(36), cov(36 * 36);
    int64_t used = -1;
    REQUIRE(sr_niqe_fit(rows.data(), sharp.data(), off.data(), 3, 0.0, mu.data(), cov.data(), &used) == SR_OK);
    REQUIRE(used >= 37 && used <= 45);
    for (int a = 0; a < 36; ++a) {
        REQUIRE(std::isfinite(mu[a]) && cov[a * 36 + a] > 0.0);
        for (int b = 0; b < 36; ++b) REQUIRE(cov[a * 36 + b] == cov[b * 36 + a]);
    }
    REQUIRE(sr_niqe_fit(rows.data(), sharp.data(), off.data(), 3, 0.0, mu.data(), cov.data(), nullptr) == SR_OK);
    REQUIRE(sr_niqe_fit(rows.data(), sharp.data(), off.data(), 3, 0.99, mu.data(), cov.data(), &used) == SR_ERR_SHAPE && used < 37);
    REQUIRE(sr_niqe_fit(rows.data(), sharp.data(), off.data(), 0, 0.75, mu.data(), cov.data(), &used) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_niqe_fit(rows.data(), sharp.data(), off.data(), 3, 1.0, mu.data(), cov.data(), &used) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_niqe_fit(rows.data(), sharp.data(), off.data(), 3, 0.0, mu.data(), cov.data(), &used) == SR_OK);

    // scores: a clean image, one with NaN rows, a rank-deficient sum of covariances, too few rows, no rows
    const double s1 = sr_niqe_score(feats[1].data(), counts[1], mu.data(), cov.data());
    REQUIRE(std::isfinite(s1) && s1 >= 0.0);
    const double s0 = sr_niqe_score(feats[0].data(), counts[0], mu.data(), cov.data());
    REQUIRE(std::isfinite(s0) && s0 >= 0.0);
    {
        std::vector<double> f = feats[1], c = cov, m = mu;
        for (int b = 0; b < counts[1]; ++b) f[(size_t)b * 36 + 9] = f[(size_t)b * 36 + 5];
        for (int a = 0; a < 36; ++a) c[a * 36 + 9] = c[a * 36 + 5];
        for (int a = 0; a < 36; ++a) c[9 * 36 + a] = c[5 * 36 + a];
        m[9] = m[5];
        const double s = sr_niqe_score(f.data(), counts[1], m.data(), c.data());
        REQUIRE(std::isfinite(s) && s >= 0.0);
    }
    REQUIRE(std::isnan(sr_niqe_score(feats[2].data(), counts[2], mu.data(), cov.data())));
    REQUIRE(std::isnan(sr_niqe_score(feats[2].data(), 0, mu.data(), cov.data())));
    REQUIRE(std::isnan(sr_niqe_score(nullptr, 1, mu.data(), cov.data())));
    {
        std::vector<double> zero(36 * 36, 0.0), f(2 * 36, 1.0);          // every eigenvalue 0: nothing is kept, the score is 0
        const double s = sr_niqe_score(f.data(), 2, mu.data(), zero.data());
        REQUIRE(s == 0.0);
    }
    printf("niqe-driver-ok %.17g %.17g\n", s0, s1);
    return 0;
}
