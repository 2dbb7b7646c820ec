// imresize_driver.cpp -- stand-alone driver for the sanitizer run of the host side of imresize (tests/test_imresize_sanitize.py):
// compiled with csrc/sr_imresize_host.cpp alone under -fsanitize=address,undefined, it takes sr_imresize_size,
// sr_imresize_weights (exact-size heap buffers) and sr_imresize_plan through the scale range, short axes and every refusal,
// and walks each table the way the kernel does: every index inside the axis, every tile inside the plan's span.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "sr_imresize.h"

static char g_err[512] = "";

// sr_host.cpp owns this in the library; the driver links sr_imresize_host.cpp alone
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
            fprintf(stderr, "imresize_driver: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

static int one_axis(int n, double scale, int aa)
{
    const int m = sr_imresize_size(n, scale);
    REQUIRE(m == (int)std::ceil((double)n * scale));
    int taps = 0;
    REQUIRE(sr_imresize_weights(n, m, scale, aa, 0, &taps, nullptr, nullptr) == SR_OK);
    REQUIRE(taps >= 1 && taps <= IMR_MAX_TAPS);
    std::vector<double> w((size_t)m * taps);            // exact size: a write past the end is the sanitizer's to find
    std::vector<int32_t> idx((size_t)m * taps);
    REQUIRE(sr_imresize_weights(n, m, scale, aa, taps, &taps, w.data(), idx.data()) == SR_OK);
    for (int i = 0; i < m; ++i) {
        double sum = 0.0;
        for (int k = 0; k < taps; ++k) {
            REQUIRE(idx[(size_t)i * taps + k] >= 0 && idx[(size_t)i * taps + k] < n);
            sum += w[(size_t)i * taps + k];
        }
        REQUIRE(std::fabs(sum - 1.0) <= 1e-14);
    }
    if (taps > 1) REQUIRE(sr_imresize_weights(n, m, scale, aa, taps - 1, &taps, w.data(), idx.data()) == SR_ERR_INVALID_ARG);
    return 0;
}

// the kernel's addressing, on the host: every LDS cell a tile touches lies inside the plan's budget
static int one_plan(int h, int w, int cn, double sy, double sx, int dh, int dw, int aa)
{
    ImrAxis ay, ax;
    ImrPlan p;
    REQUIRE(imr_plan("driver", h, w, cn, sy, sx, dh, dw, aa, &ay, &ax, &p) == SR_OK);
    const ImrAxis &A = p.order == 0 ? ay : ax, &B = p.order == 0 ? ax : ay;
    REQUIRE(p.order == (sy <= sx ? 0 : 1));
    REQUIRE(p.lds_bytes == (size_t)p.tile_a * p.span_b * cn * sizeof(double) && p.lds_bytes <= IMR_LDS_DOUBLES * sizeof(double));
    REQUIRE(p.tiles_a == (A.n_out + p.tile_a - 1) / p.tile_a && p.tiles_b == (B.n_out + p.tile_b - 1) / p.tile_b);
    for (long long tb = 0; tb < p.tiles_b; ++tb) {
        const int b0 = (int)tb * p.tile_b, b1 = std::min(b0 + p.tile_b, B.n_out);
        const int base = B.start[b0], span = B.start[b1 - 1] + B.taps - base;
        REQUIRE(span >= 1 && span <= p.span_b);
        for (int ob = b0; ob < b1; ++ob) {
            REQUIRE(B.start[ob] - base >= 0 && B.start[ob] - base + B.taps <= span);
            for (int k = 0; k < B.taps; ++k) REQUIRE(imr_reflect((long long)B.start[ob] + k, B.n_in) == B.idx[(size_t)ob * B.taps + k]);
        }
    }
    int order, ty, tx, th, tw;
    size_t lds, scratch;
    REQUIRE(sr_imresize_plan(h, w, cn, sy, sx, dh, dw, aa, &order, &ty, &tx, &th, &tw, &lds, &scratch) == SR_OK);
    REQUIRE(order == p.order && ty == ay.taps && tx == ax.taps && lds == p.lds_bytes && scratch == p.total);
    REQUIRE(sr_imresize_plan(h, w, cn, sy, sx, dh, dw, aa, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    return 0;
}

int main()
{
    std::mt19937_64 rng(20261020);
    const double scales[] = {1.0 / 2, 1.0 / 3, 1.0 / 4, 1.0 / 8, 1.0 / 16, 3.0 / 4, 1.0, 1.5, 2.0, 3.0, 4.0, 16.0, 0.07};
    const int sides[] = {1, 2, 5, 7, 31, 64, 97, 331};
    for (double s : scales)
        for (int n : sides)
            for (int aa = 0; aa < 2; ++aa)
                if (one_axis(n, s, aa)) return 1;
    std::uniform_real_distribution<double> us(1.0 / 16, 16.0);
    std::uniform_int_distribution<int> un(1, 400);
    for (int t = 0; t < 200; ++t)
        if (one_axis(un(rng), us(rng), t & 1)) return 1;
    // plans: the scalar form, the output-size form in both pass orders, every channel count
    for (double s : scales)
        for (int cn : {1, 3, 4}) {
            const int h = 97, w = 131;
            if (one_plan(h, w, cn, s, s, sr_imresize_size(h, s), sr_imresize_size(w, s), 1)) return 1;
        }
    for (int t = 0; t < 60; ++t) {
        const int h = un(rng), w = un(rng);
        const int dh = std::max(1, std::min(h * 16, std::max((h + 15) / 16, un(rng))));
        const int dw = std::max(1, std::min(w * 16, std::max((w + 15) / 16, un(rng))));
        if (one_plan(h, w, t % 3 == 0 ? 1 : t % 3 == 1 ? 3 : 4, (double)dh / h, (double)dw / w, dh, dw, t & 1)) return 1;
    }
    if (one_plan(5, 7, 3, 0.25, 0.25, 2, 2, 1) || one_plan(1, 40, 1, 0.25, 0.25, 1, 10, 1) || one_plan(11550, 17320, 3, 0.125, 0.125, 1444, 2165, 1))
        return 1;
    // refusals
    int taps = 0;
    double w8[8];
    int32_t i8[8];
    REQUIRE(sr_imresize_size(0, 0.5) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_imresize_size(10, 1.0 / 17) == SR_ERR_UNSUPPORTED && sr_imresize_size(10, 16.5) == SR_ERR_UNSUPPORTED);
    REQUIRE(sr_imresize_size(10, std::nan("")) == SR_ERR_UNSUPPORTED);
    REQUIRE(sr_imresize_weights(10, 5, 0.5, 1, 0, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_imresize_weights(10, 5, 0.5, 1, 8, &taps, w8, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_imresize_weights(10, 5, 0.5, 1, 8, &taps, nullptr, i8) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_imresize_weights(10, 6, 0.5, 1, 0, &taps, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_imresize_weights(0, 1, 0.5, 1, 0, &taps, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_imresize_weights(1, 1, 0.5, 1, 8, &taps, w8, i8) == SR_OK && taps == 8);
    REQUIRE(sr_imresize_plan(64, 64, 2, 0.5, 0.5, 32, 32, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_imresize_plan(64, 64, 3, 0.5, 0.05, 32, 4, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
    REQUIRE(sr_imresize_plan(64, 0, 3, 0.5, 0.5, 32, 32, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_imresize_plan(64, 64, 3, 0.5, 0.5, 32, 31, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    printf("imresize-driver-ok\n");
    return 0;
}
