// dists_driver.cpp -- stand-alone driver for the sanitizer run of the host side of DISTS (tests/test_dists_sanitize.py): compiled
// with csrc/sr_dists_host.cpp alone under -fsanitize=address,undefined, it takes seeded sums through sr_dists_layer_sizes ->
// sr_dists_score with exact-size heap buffers, dead, constant and equal channels and every refusal included.  It also walks the
// per-tile plan of the three feature stacks (csrc/sr_vgg_ranges.h, host only: lp_geometry, lp_ranges, lp_plan) over small and odd
// sizes and every tile, checking what the forwards index with: owned inside needed at every tap, the needed input of every
// layer covering its needed output, pitches and the buffer size.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <random>
#include <vector>

#include "sr_internal.h"
#include "sr_vgg_ranges.h"

static char g_err[512] = "";

// sr_host.cpp owns this in the library; the driver links sr_dists_host.cpp alone
int sr_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            fprintf(stderr, "dists_driver: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

static bool inside(Range in, Range out) { return in.empty() || (out.a <= in.a && in.b <= out.b); }

// every tile's plan of one stack on an h x w image; false where the forward would index outside a buffer
static bool plans_hold(const std::vector<LpLayer> &L, int h, int w, int tile)
{
    LpGeom G;
    if (!lp_geometry(L, h, w, G)) return true;                               // refused: nothing is planned
    int tx, ty;
    lp_tile_grid(h, w, tile, tx, ty);
    for (int ti = 0; ti < tx * ty; ++ti) {
        LpPlan P;
        lp_plan(L, G, tile, ti, P);
        const Range *need[2] = {P.ny.data(), P.nx.data()}, *own[2] = {P.oy.data(), P.ox.data()};
        const int *ext[2] = {G.H.data(), G.W.data()};
        for (size_t li = 0; li < L.size(); ++li) {
            const int ai = G.act_of_layer[li];
            for (int ax = 0; ax < 2; ++ax) {
                const Range n = need[ax][ai];
                if (!n.empty() && (n.a < 0 || n.b > ext[ax][ai])) return false;
                if (L[li].kind == LP_TAP) {
                    if (!inside(own[ax][ai], n)) return false;
                    continue;
                }
                const Range o = need[ax][ai + 1];
                if (o.empty()) continue;
                const Range reads = {std::max(o.a * L[li].s - L[li].p, 0), std::min((o.b - 1) * L[li].s - L[li].p + L[li].k, ext[ax][ai])};
                if (!inside(reads, n)) return false;
            }
        }
        for (size_t j = 1; j < G.H.size(); ++j)
            if (P.pitch[j] < P.nx[j].n() || P.pitch[j] % 4 || (size_t)P.plane[j] * G.C[j] > P.need_floats) return false;
    }
    return true;
}

int main()
{
    {
        std::vector<LpLayer> nets[3];
        lp_arch(true, nets[0]);
        lp_arch(false, nets[1]);
        ds_arch(nets[2]);
        const int sides[] = {1, 2, 16, 17, 31, 33, 35, 47, 53, 64, 67, 99, 131};
        const int tiles[] = {0, 16, 32, 48, 64, 128};
        for (auto &L : nets)
            for (int h : sides)
                for (int w : sides)
                    for (int t : tiles) REQUIRE(plans_hold(L, h, w, t));
    }
    constexpr int TOTAL = 1475;
    const int CH[6] = {3, 64, 128, 256, 512, 512};
    std::mt19937_64 rng(20260519);
    std::uniform_real_distribution<double> ud(0.0, 1.0);

    // sizes: exact-size output, ceil halving, the smallest image
    const int shapes[5][2] = {{1, 1}, {17, 1}, {33, 47}, {131, 77}, {4096, 4096}};
    for (auto &sh : shapes) {
        std::vector<int> hw(12, -1);
        REQUIRE(sr_dists_layer_sizes(sh[0], sh[1], hw.data()) == SR_OK);
        REQUIRE(hw[0] == sh[0] && hw[1] == sh[1] && hw[2] == sh[0] && hw[3] == sh[1]);
        for (int k = 2; k < 6; ++k) REQUIRE(hw[2 * k] == (hw[2 * k - 2] + 1) / 2 && hw[2 * k + 1] == (hw[2 * k - 1] + 1) / 2);
    }
    std::vector<int> hw(12);
    REQUIRE(sr_dists_layer_sizes(0, 4, hw.data()) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_dists_layer_sizes(4, 4, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_dists_layer_sizes(33, 47, hw.data()) == SR_OK);

    // sums of n samples per channel, drawn so that the variances are consistent
    std::vector<double> sums((size_t)TOTAL * 5), s1(TOTAL), s2(TOTAL);
    std::vector<float> alpha(TOTAL), beta(TOTAL);
    int ch = 0;
    for (int k = 0; k < 6; ++k) {
        const int n = hw[2 * k] * hw[2 * k + 1];
        for (int c = 0; c < CH[k]; ++c, ++ch) {
            double *s = &sums[(size_t)ch * 5];
            for (int i = 0; i < 5; ++i) s[i] = 0.0;
            for (int i = 0; i < n; ++i) {
                double a = ud(rng), b = 0.8 * a + 0.2 * ud(rng);
                if (k == 0) {
                    a = std::floor(a * 255.999);
                    b = std::floor(b * 255.999);
                }
                s[0] += a; s[1] += b; s[2] += a * a; s[3] += b * b; s[4] += a * b;
            }
            alpha[ch] = (float)ud(rng);
            beta[ch] = (float)ud(rng);
        }
    }
    for (int i = 0; i < 5; ++i) sums[(size_t)10 * 5 + i] = 0.0;                 // a dead channel
    {
        const double n = (double)hw[2] * hw[3];
        const double cst[5] = {0.5 * n, 0.25 * n, 0.25 * n, 0.0625 * n, 0.125 * n};
        for (int i = 0; i < 5; ++i) sums[(size_t)11 * 5 + i] = cst[i];         // constants 0.5 and 0.25
    }
    double score = -1.0;
    REQUIRE(sr_dists_score(sums.data(), hw.data(), alpha.data(), beta.data(), &score, s1.data(), s2.data()) == SR_OK);
    REQUIRE(std::isfinite(score) && score > 0.0 && score < 1.0);
    REQUIRE(s1[10] == 1.0 && s2[10] == 1.0 && s2[11] == 1.0);
    double again = -1.0;
    REQUIRE(sr_dists_score(sums.data(), hw.data(), alpha.data(), beta.data(), &again, nullptr, nullptr) == SR_OK);
    REQUIRE(again == score);
    REQUIRE(sr_dists_score(sums.data(), hw.data(), alpha.data(), beta.data(), &again, s1.data(), nullptr) == SR_OK);

    // a == b: every term is exactly 1
    for (int c = 0; c < TOTAL; ++c) {
        double *s = &sums[(size_t)c * 5];
        s[1] = s[0]; s[3] = s[2]; s[4] = s[2];
    }
    REQUIRE(sr_dists_score(sums.data(), hw.data(), alpha.data(), beta.data(), &score, s1.data(), s2.data()) == SR_OK);
    for (int c = 0; c < TOTAL; ++c) REQUIRE(s1[c] == 1.0 && s2[c] == 1.0);
    REQUIRE(std::fabs(score) <= 1e-12);

    // refusals
    REQUIRE(sr_dists_score(nullptr, hw.data(), alpha.data(), beta.data(), &score, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_dists_score(sums.data(), nullptr, alpha.data(), beta.data(), &score, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_dists_score(sums.data(), hw.data(), nullptr, beta.data(), &score, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_dists_score(sums.data(), hw.data(), alpha.data(), nullptr, &score, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_dists_score(sums.data(), hw.data(), alpha.data(), beta.data(), nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    std::vector<float> zero(TOTAL, 0.0f), bad(alpha);
    REQUIRE(sr_dists_score(sums.data(), hw.data(), zero.data(), zero.data(), &score, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    bad[TOTAL - 1] = NAN;
    REQUIRE(sr_dists_score(sums.data(), hw.data(), bad.data(), beta.data(), &score, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    std::vector<int> hw0(hw);
    hw0[11] = 0;
    REQUIRE(sr_dists_score(sums.data(), hw0.data(), alpha.data(), beta.data(), &score, nullptr, nullptr) == SR_ERR_INVALID_ARG);

    printf("dists-driver-ok\n");
    return 0;
}
