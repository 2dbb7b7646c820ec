// swinir_driver.cpp -- stand-alone driver for the sanitizer run of the host side of the SwinIR backend
// (tests/test_swinir_sanitize.py): compiled with csrc/sr_swinir_host.cpp alone under -fsanitize=address,undefined, it takes
// every supported kind of description and every refusal through sw_check_desc -> sw_tables -> sw_tail_steps -> sw_geometry
// (sr_swinir_plan) with exact-size heap buffers, and checks the relative-position index and the extent rule's invariants.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "sr_swinir.h"

static char g_err[768] = "";

// sr_host.cpp owns this in the library; the driver links sr_swinir_host.cpp alone
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
            fprintf(stderr, "swinir_driver: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

static sr_swinir_desc desc(int C, int heads, int hid, int L, int D, int s, int up)
{
    sr_swinir_desc d = {C, heads, hid, L, D, s, up, {0.4488f, 0.4371f, 0.4040f}, 1.0f};
    return d;
}

int main()
{
    // the relative-position index into an exact-size buffer: symmetric under a swap with the mirrored offset, inside the table
    {
        std::vector<int> rel(SW_TOK * SW_TOK);
        REQUIRE(sr_swinir_rel_index(rel.data(), (int)rel.size()) == SR_OK);
        for (int i = 0; i < SW_TOK; ++i)
            for (int j = 0; j < SW_TOK; ++j) {
                REQUIRE(rel[i * SW_TOK + j] >= 0 && rel[i * SW_TOK + j] < SW_REL);
                REQUIRE(rel[i * SW_TOK + j] + rel[j * SW_TOK + i] == SW_REL - 1);
            }
        REQUIRE(rel[0] == SW_REL / 2 && rel[SW_TOK - 1] == 0 && rel[(SW_TOK - 1) * SW_TOK] == SW_REL - 1);
        REQUIRE(sr_swinir_rel_index(rel.data(), 17) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_swinir_rel_index(nullptr, SW_TOK * SW_TOK) == SR_ERR_INVALID_ARG);
    }
    const sr_swinir_desc good[] = {desc(180, 6, 360, 6, 6, 4, SR_SWINIR_PIXELSHUFFLE),       desc(180, 6, 360, 6, 6, 3, SR_SWINIR_PIXELSHUFFLE),
                                   desc(60, 6, 120, 4, 6, 2, SR_SWINIR_PIXELSHUFFLEDIRECT),   desc(60, 6, 120, 1, 1, 1, SR_SWINIR_PIXELSHUFFLEDIRECT),
                                   desc(240, 8, 480, 9, 6, 4, SR_SWINIR_NEAREST_CONV),        desc(4, 1, 16, 1, 1, 4, SR_SWINIR_PIXELSHUFFLEDIRECT),
                                   desc(256, 8, 1024, 12, 12, 2, SR_SWINIR_PIXELSHUFFLE)};
    const int sizes[][2] = {{1, 1}, {1, 50}, {50, 1}, {8, 8}, {13, 21}, {257, 300}, {512, 512}, {1000, 3}};
    const int tails[] = {0, 1, 7, 64, 1000};
    for (const sr_swinir_desc &d : good) {
        REQUIRE(sw_check_desc("driver", &d) == SR_OK);
        const std::vector<SwTable> t = sw_tables(d);
        const std::vector<SwStep> steps = sw_tail_steps(d);
        const int recon = d.upsampler == SR_SWINIR_PIXELSHUFFLEDIRECT ? 1 : (d.upsampler == SR_SWINIR_NEAREST_CONV ? 5 : (d.scale == 4 ? 4 : 3));
        REQUIRE((int)t.size() == 2 + d.n_groups * (7 * d.depth + 1) + 2 + recon);
        REQUIRE((int)steps.size() == recon);
        REQUIRE(t.front().kind == SW_T_HEAD && (t.back().kind == SW_T_LAST || t.back().kind == SW_T_UPD));
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
                REQUIRE(sr_swinir_plan(&d, hw[0], hw[1], tail, &hp, &wp, &halo, &nt, &ws) == SR_OK);
                REQUIRE(hp % SW_WIN == 0 && wp % SW_WIN == 0 && hp >= hw[0] && hp < hw[0] + SW_WIN && wp >= hw[1] && wp < hw[1] + SW_WIN);
                const int tl = tail ? tail : SW_DEFAULT_TAIL;
                REQUIRE(nt == ((hw[0] + tl - 1) / tl) * ((hw[1] + tl - 1) / tl));
                REQUIRE(halo >= 1 && ws >= (size_t)hp * wp * 3);
                REQUIRE(sr_swinir_plan(&d, hw[0], hw[1], tail, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);
                // the extents of every sub-piece along one axis, into vectors the rule sizes itself: inside the padded layer
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
    struct Bad {
        sr_swinir_desc d;
        int code;
    };
    sr_swinir_desc nan_mean = desc(60, 6, 120, 1, 2, 2, SR_SWINIR_PIXELSHUFFLE), zero_range = nan_mean;
    nan_mean.mean[1] = std::numeric_limits<float>::quiet_NaN();
    zero_range.range = 0.0f;
    const Bad bad[] = {{desc(260, 10, 520, 1, 2, 2, 0), SR_ERR_UNSUPPORTED}, {desc(62, 2, 124, 1, 2, 2, 0), SR_ERR_UNSUPPORTED},
                       {desc(0, 1, 1, 1, 1, 2, 0), SR_ERR_UNSUPPORTED},      {desc(132, 4, 264, 1, 2, 2, 0), SR_ERR_UNSUPPORTED},
                       {desc(60, 0, 120, 1, 2, 2, 0), SR_ERR_UNSUPPORTED},   {desc(60, 7, 120, 1, 2, 2, 0), SR_ERR_UNSUPPORTED},
                       {desc(60, 6, 241, 1, 2, 2, 0), SR_ERR_UNSUPPORTED},   {desc(60, 6, 0, 1, 2, 2, 0), SR_ERR_UNSUPPORTED},
                       {desc(60, 6, 120, 13, 2, 2, 0), SR_ERR_UNSUPPORTED},  {desc(60, 6, 120, 1, 0, 2, 0), SR_ERR_UNSUPPORTED},
                       {desc(60, 6, 120, 1, 2, 1, 0), SR_ERR_UNSUPPORTED},   {desc(60, 6, 120, 1, 2, 5, 1), SR_ERR_UNSUPPORTED},
                       {desc(60, 6, 120, 1, 2, 2, 2), SR_ERR_UNSUPPORTED},   {desc(60, 6, 120, 1, 2, 2, 3), SR_ERR_UNSUPPORTED},
                       {desc(60, 6, 120, 1, 2, 2, -1), SR_ERR_UNSUPPORTED},  {nan_mean, SR_ERR_UNSUPPORTED},
                       {zero_range, SR_ERR_UNSUPPORTED}};
    for (const Bad &b : bad) REQUIRE(sr_swinir_plan(&b.d, 8, 8, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == b.code);
    REQUIRE(sr_swinir_plan(nullptr, 8, 8, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    const sr_swinir_desc d = good[0];
    REQUIRE(sr_swinir_plan(&d, 0, 8, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    REQUIRE(sr_swinir_plan(&d, 8, -3, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    REQUIRE(sr_swinir_plan(&d, 8, 8, -1, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_swinir_plan(&d, 2048, 2048, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);         // one pipeline block fits
    REQUIRE(sr_swinir_plan(&d, 2600, 2600, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);   // the trunk cap
    REQUIRE(sr_swinir_plan(&d, 300000, 8, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);    // rows of one launch
    REQUIRE(sr_swinir_plan(&d, 8, 2000000000, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    REQUIRE(sr_swinir_plan(&d, 200000, 2000000000, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    const sr_swinir_desc tiny = good[5];                                                   // C = 4: the cap is far, the 32-bit offsets are not
    REQUIRE(sr_swinir_plan(&tiny, 9000, 9000, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    REQUIRE(sr_swinir_plan(&tiny, 4000, 4000, 1, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);       // 16 M sub-pieces still fit int
    printf("swinir-driver-ok\n");
    return 0;
}
