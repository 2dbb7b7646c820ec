// swin2sr_driver.cpp -- stand-alone driver for the sanitizer run of the host side of the Swin2SR backend
// (tests/test_swin2sr_sanitize.py): compiled with csrc/sr_swin2sr_host.cpp and csrc/sr_swinir_host.cpp (whose ranges, tables of
// the reconstruction, extent rule and plan Swin2SR reuses) under -fsanitize=address,undefined, it takes the Swin2SR
// descriptions and every refusal through s2_check_desc -> s2_tables -> s2_tail_steps -> s2_geometry (sr_swin2sr_plan), the table
// check of a create (a k bias, a non-finite logit scale) and the two host tables (sr_swin2sr_cpb_bias) with exact-size heap
// buffers.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "sr_swin2sr.h"

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

#define REQUIRE(cond)                                                                        \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            fprintf(stderr, "swin2sr_driver: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

static sr_swin2sr_desc desc(int C, int heads, int hid, int L, int D, int s, int up)
{
    sr_swin2sr_desc d = {C, heads, hid, L, D, s, up, {0.4488f, 0.4371f, 0.4040f}, 1.0f, -200.0f};
    return d;
}

static int plan(const sr_swin2sr_desc *d, int h, int w, int tail)
{
    return sr_swin2sr_plan(d, h, w, tail, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int main()
{
    // the two host tables into exact-size buffers
    {
        const int heads = 6;
        std::vector<float> w1(S2_CPB_HIDDEN * 2), b1(S2_CPB_HIDDEN), w2((size_t)heads * S2_CPB_HIDDEN), ls(heads), table((size_t)SW_REL * heads),
            scale(heads);
        uint32_t r = 12345u;
        auto next = [&r]() {
            r = r * 1664525u + 1013904223u;
            return (float)((r >> 8) & 0xFFFF) / 32768.0f - 1.0f;
        };
        for (float &v : w1) v = next();
        for (float &v : b1) v = 0.5f * next();
        for (float &v : w2) v = 0.1f * next();
        const float logits[] = {std::log(200.0f), std::log(100.0f), std::log(5.0f), 10.0f, -3.0f, 0.0f};
        for (int i = 0; i < heads; ++i) ls[i] = logits[i];
        REQUIRE(sr_swin2sr_cpb_bias(w1.data(), b1.data(), w2.data(), ls.data(), heads, table.data(), scale.data()) == SR_OK);
        for (float v : table) REQUIRE(v > 0.0f && v < 16.0f);
        REQUIRE(scale[0] == 100.0f && scale[1] == 100.0f && scale[3] == 100.0f && scale[5] == 1.0f && scale[2] > 4.99f && scale[2] < 5.01f);
        // the centre of the grid has coordinates (0, 0): u = relu(b1), whatever W1 is
        for (int hd = 0; hd < heads; ++hd) {
            double z = 0.0;
            for (int i = 0; i < S2_CPB_HIDDEN; ++i) z += (double)w2[(size_t)hd * S2_CPB_HIDDEN + i] * (b1[i] > 0.0f ? (double)b1[i] : 0.0);
            REQUIRE(table[(size_t)(SW_REL / 2) * heads + hd] == (float)(16.0 / (1.0 + std::exp(-z))));
        }
        REQUIRE(sr_swin2sr_cpb_bias(w1.data(), b1.data(), w2.data(), nullptr, heads, table.data(), nullptr) == SR_OK);
        REQUIRE(sr_swin2sr_cpb_bias(nullptr, nullptr, nullptr, ls.data(), heads, nullptr, scale.data()) == SR_OK);
        REQUIRE(sr_swin2sr_cpb_bias(w1.data(), b1.data(), w2.data(), nullptr, heads, table.data(), scale.data()) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_swin2sr_cpb_bias(nullptr, b1.data(), w2.data(), ls.data(), heads, table.data(), scale.data()) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_swin2sr_cpb_bias(w1.data(), b1.data(), w2.data(), ls.data(), heads, nullptr, nullptr) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_swin2sr_cpb_bias(w1.data(), b1.data(), w2.data(), ls.data(), 0, table.data(), scale.data()) == SR_ERR_UNSUPPORTED);
    }
    const sr_swin2sr_desc good[] = {desc(180, 6, 360, 6, 6, 4, SR_SWINIR_PIXELSHUFFLE),       desc(180, 6, 360, 6, 6, 2, SR_SWINIR_PIXELSHUFFLE),
                                    desc(60, 6, 120, 4, 6, 2, SR_SWINIR_PIXELSHUFFLEDIRECT),  desc(180, 6, 360, 6, 6, 4, SR_SWINIR_NEAREST_CONV),
                                    desc(4, 1, 16, 1, 1, 3, SR_SWINIR_PIXELSHUFFLE),          desc(256, 8, 1024, 12, 12, 1, SR_SWINIR_PIXELSHUFFLEDIRECT)};
    const int sizes[][2] = {{1, 1}, {1, 50}, {50, 1}, {8, 8}, {13, 21}, {257, 300}, {512, 512}, {1000, 3}};
    const int tails[] = {0, 1, 7, 64, 1000};
    for (const sr_swin2sr_desc &d : good) {
        REQUIRE(s2_check_desc("driver", &d) == SR_OK);
        const std::vector<SwTable> t = s2_tables(d);
        const std::vector<SwStep> steps = s2_tail_steps(d);
        const int recon = d.upsampler == SR_SWINIR_PIXELSHUFFLEDIRECT ? 1 : d.upsampler == SR_SWINIR_NEAREST_CONV ? 5 : (d.scale == 4 ? 4 : 3);
        REQUIRE((int)t.size() == 3 + d.n_groups * (S2_LAYER_TABLES * d.depth + 2) + 2 + recon);
        REQUIRE((int)steps.size() == recon);
        REQUIRE(t[0].kind == SW_T_HEAD && t[1].kind == SW_T_PROJ && t[2].kind == SW_T_LN && t[3].kind == SW_T_QKV && t[4].kind == S2_T_LOGIT &&
                t[5].kind == S2_T_CPB1 && t[6].kind == S2_T_CPB2 && t[7].kind == SW_T_PROJ);
        // the table check of a create: exact-size arrays for the tables it reads
        std::vector<std::vector<float>> w(t.size()), b(t.size());
        std::vector<const float *> pw(t.size()), pb(t.size());
        for (size_t k = 0; k < t.size(); ++k) {
            w[k].assign(t[k].kind == S2_T_LOGIT ? d.n_heads : 1, 0.5f);
            b[k].assign(t[k].kind == SW_T_QKV ? 3 * d.n_feat : 1, 0.0f);
            if (t[k].kind == SW_T_QKV)
                for (int c = 0; c < 3 * d.n_feat; ++c) b[k][c] = c >= d.n_feat && c < 2 * d.n_feat ? 0.0f : 0.25f;
            pw[k] = w[k].data();
            pb[k] = b[k].data();
        }
        REQUIRE(s2_check_tables("driver", d, t, pw.data(), pb.data()) == SR_OK);
        b[3][2 * d.n_feat - 1] = -0.0f;                     // a negative zero is zero
        REQUIRE(s2_check_tables("driver", d, t, pw.data(), pb.data()) == SR_OK);
        b[3][2 * d.n_feat - 1] = 1e-30f;
        REQUIRE(s2_check_tables("driver", d, t, pw.data(), pb.data()) == SR_ERR_UNSUPPORTED);
        b[3][2 * d.n_feat - 1] = 0.0f;
        w[4][d.n_heads - 1] = std::numeric_limits<float>::quiet_NaN();
        REQUIRE(s2_check_tables("driver", d, t, pw.data(), pb.data()) == SR_ERR_UNSUPPORTED);
        for (const auto &hw : sizes)
            for (int tail : tails) {
                if (tail == 1 && (long long)hw[0] * hw[1] > 4000) continue;
                int hp = 0, wp = 0, halo = 0, nt = 0;
                size_t ws = 0;
                REQUIRE(sr_swin2sr_plan(&d, hw[0], hw[1], tail, &hp, &wp, &halo, &nt, &ws) == SR_OK);
                REQUIRE(hp % SW_WIN == 0 && wp % SW_WIN == 0 && hp >= hw[0] && hp < hw[0] + SW_WIN && wp >= hw[1] && wp < hw[1] + SW_WIN);
                const int tl = tail ? tail : SW_DEFAULT_TAIL;
                REQUIRE(nt == ((hw[0] + tl - 1) / tl) * ((hw[1] + tl - 1) / tl));
                REQUIRE(halo >= 1 && ws >= (size_t)hp * wp * 3);
                const sr_swinir_desc s = s2_as_swinir(d);   // the plan is SwinIR's
                int hp2 = 0, wp2 = 0, halo2 = 0, nt2 = 0;
                size_t ws2 = 0;
                REQUIRE(sr_swinir_plan(&s, hw[0], hw[1], tail, &hp2, &wp2, &halo2, &nt2, &ws2) == SR_OK);
                REQUIRE(hp == hp2 && wp == wp2 && halo == halo2 && nt == nt2 && ws == ws2);
                REQUIRE(plan(&d, hw[0], hw[1], tail) == SR_OK);
            }
    }
    // refusals, each by its own code
    sr_swin2sr_desc inf_mask = desc(60, 6, 120, 1, 2, 2, SR_SWINIR_PIXELSHUFFLE), nan_mask = inf_mask, zero_range = inf_mask, nan_mean = inf_mask;
    inf_mask.mask_value = -std::numeric_limits<float>::infinity();
    nan_mask.mask_value = std::numeric_limits<float>::quiet_NaN();
    nan_mean.mean[2] = std::numeric_limits<float>::quiet_NaN();
    zero_range.range = 0.0f;
    const sr_swin2sr_desc bad[] = {desc(260, 10, 520, 1, 2, 2, 0), desc(62, 2, 124, 1, 2, 2, 0), desc(0, 1, 1, 1, 1, 2, 0),  desc(132, 4, 264, 1, 2, 2, 0),
                                   desc(60, 0, 120, 1, 2, 2, 0),   desc(60, 7, 120, 1, 2, 2, 0), desc(60, 6, 241, 1, 2, 2, 0), desc(60, 6, 0, 1, 2, 2, 0),
                                   desc(60, 6, 120, 13, 2, 2, 0),  desc(60, 6, 120, 1, 0, 2, 0), desc(60, 6, 120, 1, 13, 2, 0), desc(60, 6, 120, 1, 2, 1, 0),
                                   desc(60, 6, 120, 1, 2, 8, 0),   desc(60, 6, 120, 1, 2, 5, 1), desc(60, 6, 120, 1, 2, 2, 2),  desc(60, 6, 120, 1, 2, 2, 3),
                                   inf_mask, nan_mask, nan_mean, zero_range};
    for (const sr_swin2sr_desc &b : bad) REQUIRE(plan(&b, 16, 16, 0) == SR_ERR_UNSUPPORTED);
    REQUIRE(plan(nullptr, 16, 16, 0) == SR_ERR_INVALID_ARG);
    const sr_swin2sr_desc d = good[0];
    const sr_swin2sr_desc tiny = good[4];
    REQUIRE(plan(&d, 0, 8, 0) == SR_ERR_SHAPE);
    REQUIRE(plan(&d, 8, -3, 0) == SR_ERR_SHAPE);
    REQUIRE(plan(&d, 8, 8, -1) == SR_ERR_INVALID_ARG);
    REQUIRE(plan(&d, 2048, 2048, 0) == SR_OK);              // one pipeline block fits
    REQUIRE(plan(&d, 3000, 3000, 0) == SR_ERR_SHAPE);       // the trunk cap
    REQUIRE(plan(&d, 300000, 8, 0) == SR_ERR_SHAPE);        // rows of one launch
    REQUIRE(plan(&d, 8, 2000000000, 0) == SR_ERR_SHAPE);
    REQUIRE(plan(&tiny, 9000, 9000, 0) == SR_ERR_SHAPE);
    printf("swin2sr-driver-ok\n");
    return 0;
}
