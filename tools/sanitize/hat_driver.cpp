// hat_driver.cpp -- stand-alone driver for the sanitizer run of the host side of the HAT backend
// (tests/test_hat_sanitize.py): compiled with csrc/sr_hat_host.cpp and csrc/sr_swinir_host.cpp (whose tail steps and extent rule
// HAT reuses) under -fsanitize=address,undefined, it takes the HAT, HAT-S and HAT-L descriptions and every refusal through
// ht_check_desc -> ht_tables -> ht_tail_steps -> ht_geometry (sr_hat_plan) with exact-size heap buffers, and checks both
// relative-position indices, the wrapping of a caller's index and the extent rule's invariants.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "sr_hat.h"

static char g_err[768] = "";

// sr_host.cpp owns this in the library; the driver links the two host units alone
int sr_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define REQUIRE(cond)                                                                    \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            fprintf(stderr, "hat_driver: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

static sr_hat_desc desc(int C, int heads, int hid, int mid, int sq, int L, int D, int s)
{
    sr_hat_desc d = {C, heads, hid, mid, sq, L, D, s, 0.01f, {0.4488f, 0.4371f, 0.4040f}, 1.0f};
    return d;
}

int main()
{
    // the window index into an exact-size buffer: symmetric under a swap with the mirrored offset, inside the table
    {
        std::vector<int> rel(HT_TOK * HT_TOK);
        REQUIRE(sr_hat_rel_index(rel.data(), (int)rel.size()) == SR_OK);
        for (int i = 0; i < HT_TOK; ++i)
            for (int j = 0; j < HT_TOK; ++j) {
                REQUIRE(rel[i * HT_TOK + j] >= 0 && rel[i * HT_TOK + j] < HT_REL);
                REQUIRE(rel[i * HT_TOK + j] + rel[j * HT_TOK + i] == HT_REL - 1);
            }
        REQUIRE(rel[0] == HT_REL / 2 && rel[HT_TOK - 1] == 0 && rel[(HT_TOK - 1) * HT_TOK] == HT_REL - 1);
        REQUIRE(sr_hat_rel_index(rel.data(), 17) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_hat_rel_index(nullptr, HT_TOK * HT_TOK) == SR_ERR_INVALID_ARG);
    }
    // the OCA index: inside the table after the wrap; a caller's raw index wraps to the same; out-of-range values are refused
    {
        std::vector<int> idx(HT_TOK * HT_KEYS), raw(HT_TOK * HT_KEYS), out(HT_TOK * HT_KEYS);
        REQUIRE(sr_hat_oca_index(idx.data(), (int)idx.size()) == SR_OK);
        int negatives = 0;
        for (int i = 0; i < HT_TOK; ++i)
            for (int j = 0; j < HT_KEYS; ++j) {
                const int v = (j / HT_EXT - i / HT_WIN - 7) * 39 + (j % HT_EXT - i % HT_WIN - 7);
                raw[i * HT_KEYS + j] = v;
                negatives += v < 0;
                REQUIRE(idx[i * HT_KEYS + j] >= 0 && idx[i * HT_KEYS + j] < HT_REL_OCA);
                REQUIRE(idx[i * HT_KEYS + j] == (v < 0 ? v + HT_REL_OCA : v));
            }
        REQUIRE(negatives > 0);
        REQUIRE(ht_wrap_oca_index("driver", raw.data(), out.data()) == SR_OK);
        REQUIRE(out == idx);
        raw[5] = HT_REL_OCA;
        REQUIRE(ht_wrap_oca_index("driver", raw.data(), out.data()) == SR_ERR_INVALID_ARG);
        raw[5] = -HT_REL_OCA - 1;
        REQUIRE(ht_wrap_oca_index("driver", raw.data(), out.data()) == SR_ERR_INVALID_ARG);
        raw[5] = -HT_REL_OCA;
        REQUIRE(ht_wrap_oca_index("driver", raw.data(), out.data()) == SR_OK && out[5] == 0);
        REQUIRE(sr_hat_oca_index(idx.data(), 17) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_hat_oca_index(nullptr, HT_TOK * HT_KEYS) == SR_ERR_INVALID_ARG);
    }
    const sr_hat_desc good[] = {desc(180, 6, 360, 60, 6, 6, 6, 4),   desc(180, 6, 360, 60, 6, 6, 6, 3), desc(144, 6, 288, 6, 6, 6, 6, 2),
                                desc(180, 6, 360, 60, 6, 12, 6, 4),  desc(4, 1, 16, 1, 1, 1, 1, 2),     desc(256, 8, 1024, 256, 256, 12, 12, 2)};
    const int sizes[][2] = {{1, 1}, {1, 50}, {50, 1}, {16, 16}, {19, 37}, {257, 300}, {512, 512}, {1000, 3}};
    const int tails[] = {0, 1, 7, 64, 1000};
    for (const sr_hat_desc &d : good) {
        REQUIRE(ht_check_desc("driver", &d) == SR_OK);
        const std::vector<SwTable> t = ht_tables(d);
        const std::vector<SwStep> steps = ht_tail_steps(d);
        const int recon = d.scale == 4 ? 4 : 3;
        REQUIRE((int)t.size() == 2 + d.n_groups * (11 * d.depth + 8) + 2 + recon);
        REQUIRE((int)steps.size() == recon);
        REQUIRE(t.front().kind == SW_T_HEAD && t.back().kind == SW_T_LAST);
        int mult = 1;
        for (const SwStep &s : steps) {                  // a step runs at the resolution its predecessors produced
            REQUIRE(s.mult == mult);
            mult *= s.r;
        }
        REQUIRE(mult == d.scale);
        for (const auto &hw : sizes)
            for (int tail : tails) {
                if (tail == 1 && (long long)hw[0] * hw[1] > 4000) continue;
                int hp = 0, wp = 0, halo = 0, nt = 0;
                size_t ws = 0;
                REQUIRE(sr_hat_plan(&d, hw[0], hw[1], tail, &hp, &wp, &halo, &nt, &ws) == SR_OK);
                REQUIRE(hp % HT_WIN == 0 && wp % HT_WIN == 0 && hp >= hw[0] && hp < hw[0] + HT_WIN && wp >= hw[1] && wp < hw[1] + HT_WIN);
                const int tl = tail ? tail : SW_DEFAULT_TAIL;
                REQUIRE(nt == ((hw[0] + tl - 1) / tl) * ((hw[1] + tl - 1) / tl));
                REQUIRE(halo >= 1 && ws >= (size_t)hp * wp * 3);
                REQUIRE(sr_hat_plan(&d, hw[0], hw[1], tail, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);
                std::vector<int> a, b;
                for (int lo = 0; lo < hw[0]; lo += tl) {
                    const int hi = lo + tl < hw[0] ? lo + tl : hw[0];
                    sw_backward_extents(steps.data(), (int)steps.size(), d.scale, lo, hi, hp, a, b);
                    REQUIRE(a.size() == steps.size() && b.size() == steps.size());
                    for (size_t i = 0; i < steps.size(); ++i) REQUIRE(0 <= a[i] && a[i] < b[i] && b[i] <= hp * steps[i].mult);
                    REQUIRE(a.back() * steps.back().r == lo * d.scale && b.back() * steps.back().r == hi * d.scale);
                }
            }
    }
    // refusals, each by its own code
    sr_hat_desc nan_scale = desc(60, 6, 120, 20, 2, 1, 2, 2), zero_range = nan_scale, nan_mean = nan_scale;
    nan_scale.conv_scale = std::numeric_limits<float>::infinity();
    nan_mean.mean[1] = std::numeric_limits<float>::quiet_NaN();
    zero_range.range = 0.0f;
    const sr_hat_desc bad[] = {desc(260, 10, 520, 20, 2, 1, 2, 2), desc(62, 2, 124, 20, 2, 1, 2, 2),  desc(0, 1, 1, 1, 1, 1, 1, 2),
                               desc(132, 4, 264, 20, 2, 1, 2, 2),  desc(60, 0, 120, 20, 2, 1, 2, 2),  desc(60, 7, 120, 20, 2, 1, 2, 2),
                               desc(60, 6, 241, 20, 2, 1, 2, 2),   desc(60, 6, 0, 20, 2, 1, 2, 2),    desc(60, 6, 120, 0, 2, 1, 2, 2),
                               desc(60, 6, 120, 61, 2, 1, 2, 2),   desc(60, 6, 120, 20, 0, 1, 2, 2),  desc(60, 6, 120, 20, 61, 1, 2, 2),
                               desc(60, 6, 120, 20, 2, 13, 2, 2),  desc(60, 6, 120, 20, 2, 1, 0, 2),  desc(60, 6, 120, 20, 2, 1, 13, 2),
                               desc(60, 6, 120, 20, 2, 1, 2, 1),   desc(60, 6, 120, 20, 2, 1, 2, 8),  nan_scale, nan_mean, zero_range};
    for (const sr_hat_desc &b : bad) REQUIRE(sr_hat_plan(&b, 16, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
    REQUIRE(sr_hat_plan(nullptr, 16, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    const sr_hat_desc d = good[0];
    const sr_hat_desc tiny = good[4];                                                     // C = 4: the cap is far, the 32-bit offsets are not
    REQUIRE(sr_hat_plan(&d, 0, 8, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    REQUIRE(sr_hat_plan(&d, 8, -3, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    REQUIRE(sr_hat_plan(&d, 8, 8, -1, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_hat_plan(&d, 2048, 2048, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);          // one pipeline block fits
    REQUIRE(sr_hat_plan(&d, 2400, 2400, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);    // the trunk cap
    REQUIRE(sr_hat_plan(&d, 300000, 8, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);     // rows of one launch
    REQUIRE(sr_hat_plan(&tiny, 262128, 8, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);         // 262128 rows: the most that fit
    REQUIRE(sr_hat_plan(&tiny, 262129, 8, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);  // padded to 262144: the padded rows count
    REQUIRE(sr_hat_plan(&d, 8, 2000000000, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    REQUIRE(sr_hat_plan(&d, 200000, 2000000000, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    REQUIRE(sr_hat_plan(&tiny, 9000, 9000, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    REQUIRE(sr_hat_plan(&tiny, 4000, 4000, 1, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);        // 16 M sub-pieces still fit int
    printf("hat-driver-ok\n");
    return 0;
}
