// deltae_driver.cpp -- stand-alone driver for the sanitizer run of the host side of the colour difference
// (tests/test_deltae_sanitize.py): compiled with csrc/sr_deltae_host.cpp alone under -fsanitize=address,undefined, it takes
// sr_delta_e_plan, sr_delta_e_table, sr_delta_e_lab_u8, sr_delta_e_pair and the mean / rms / percentile / fraction functions
// through sizes up to the largest an int holds, every byte triple of a coarse cube, exact-size heap buffers and every refusal,
// and checks each plan the way the kernels use it: the tiles cover the cropped rectangle, the sections of the scratch lie
// inside it and do not overlap.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

#include "sr_deltae.h"

static char g_err[512] = "";

// sr_host.cpp owns this in the library; the driver links sr_deltae_host.cpp alone
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
            fprintf(stderr, "deltae_driver: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

static int one_plan(int h, int w, int cn, int cb, int formula)
{
    int ch = 0, cw = 0, blocks = 0;
    uint64_t count = 0;
    size_t bytes = 0;
    const int rc = sr_delta_e_plan(h, w, cn, cb, formula, &ch, &cw, &count, &blocks, &bytes);
    const long long lh = (long long)h - 2LL * cb, lw = (long long)w - 2LL * cb;
    if (lh < 1 || lw < 1) {
        REQUIRE(rc == SR_ERR_SHAPE);
        return 0;
    }
    if ((uint64_t)lh * (uint64_t)lw > (1ull << 40)) {
        REQUIRE(rc == SR_ERR_UNSUPPORTED);
        return 0;
    }
    REQUIRE(rc == SR_OK);
    REQUIRE(sr_delta_e_plan(h, w, cn, cb, formula, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    DePlan p;
    REQUIRE(delta_e_plan("driver", h, w, cn, cb, formula, &p) == SR_OK);
    REQUIRE(p.ch == lh && p.cw == lw && ch == lh && cw == lw && count == (uint64_t)lh * (uint64_t)lw && p.total == bytes);
    REQUIRE((long long)p.tiles_x * DE_TW >= lw && (long long)(p.tiles_x - 1) * DE_TW < lw);
    const long long tiles_y = p.tiles / p.tiles_x;
    REQUIRE(tiles_y * p.tiles_x == p.tiles && tiles_y * DE_TH >= lh && (tiles_y - 1) * DE_TH < lh);
    REQUIRE(blocks == p.blocks && blocks >= 1 && blocks <= DE_MAX_BLOCKS && blocks <= p.tiles);
    REQUIRE(blocks == DE_MAX_BLOCKS || blocks == p.tiles);
    // a block's 32-bit histogram counters: its share of the tiles, whole
    REQUIRE(((p.tiles + blocks - 1) / blocks) * (long long)(DE_TW * DE_TH) < (1LL << 32));
    REQUIRE(p.off_table == 0 && p.off_hist >= DE_TABLE * sizeof(double));
    REQUIRE(p.off_result >= p.off_hist + SR_DELTA_E_BINS * sizeof(uint64_t) && p.off_part >= p.off_result + 3 * sizeof(double));
    REQUIRE(p.total >= p.off_part + (size_t)blocks * 3 * sizeof(double));
    REQUIRE(p.off_hist % 256 == 0 && p.off_result % 256 == 0 && p.off_part % 256 == 0);
    return 0;
}

int main()
{
    const int big = std::numeric_limits<int>::max();
    const int sides[] = {1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 8192, 8193, 17320, 1 << 20, (1 << 20) + 1, big};
    for (int h : sides)
        for (int w : sides)
            for (int cn : {1, 3, 4})
                for (int cb : {0, 1, 2, 3, 128, big / 2})
                    for (int f : {SR_DELTA_E_2000, SR_DELTA_E_76})
                        if (one_plan(h, w, cn, cb, f)) return 1;
    for (int cn : {0, 2, 5, -1}) REQUIRE(sr_delta_e_plan(8, 8, cn, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    for (int f : {2, 3, -1, big}) REQUIRE(sr_delta_e_plan(8, 8, 3, 0, f, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
    REQUIRE(sr_delta_e_plan(8, 8, 3, -1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_delta_e_plan(0, 8, 3, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_delta_e_plan(8, -3, 3, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);

    // the table, into an exact-size heap buffer
    std::unique_ptr<double[]> table(new double[DE_TABLE]);
    REQUIRE(sr_delta_e_table(table.get()) == SR_OK && sr_delta_e_table(nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(table[0] == 0.0 && table[255] == 1.0);
    for (int c = 1; c < DE_TABLE; ++c) REQUIRE(table[c] > table[c - 1]);

    // Lab and both formulas over a coarse cube of byte triples, each against each neighbour in the walk
    std::unique_ptr<double[]> lab(new double[3]), prev(new double[3]);
    REQUIRE(sr_delta_e_lab_u8(0, 0, 0, prev.get()) == SR_OK && prev[0] == 0.0 && prev[1] == 0.0 && prev[2] == 0.0);
    double worst = 0.0;
    for (int r = 0; r < 256; r += 17)
        for (int g = 0; g < 256; g += 15)
            for (int b = 0; b < 256; b += 51) {
                REQUIRE(sr_delta_e_lab_u8(r, g, b, lab.get()) == SR_OK);
                REQUIRE(lab[0] >= 0.0 && lab[0] <= 100.0 + 1e-9 && std::fabs(lab[1]) < 130.0 && std::fabs(lab[2]) < 130.0);
                for (int f : {SR_DELTA_E_2000, SR_DELTA_E_76}) {
                    double d = -1.0, back = -1.0, self = -1.0;
                    REQUIRE(sr_delta_e_pair(prev.get(), lab.get(), f, &d) == SR_OK && d >= 0.0 && std::isfinite(d));
                    REQUIRE(sr_delta_e_pair(lab.get(), prev.get(), f, &back) == SR_OK && std::fabs(back - d) <= 1e-9 * (1.0 + d));
                    REQUIRE(sr_delta_e_pair(lab.get(), lab.get(), f, &self) == SR_OK && self == 0.0);
                    if (f == SR_DELTA_E_2000 && d > worst) worst = d;
                    REQUIRE(de_bin(d) >= 0 && de_bin(d) < SR_DELTA_E_BINS);
                }
                for (int k = 0; k < 3; ++k) prev[k] = lab[k];
            }
    REQUIRE(worst > 50.0 && worst < 128.0);
    REQUIRE(de_bin(0.0) == 0 && de_bin(0.0624) == 0 && de_bin(0.0625) == 1 && de_bin(127.9) == 2046 && de_bin(127.94) == 2047 &&
            de_bin(1e300) == 2047 && de_bin(std::numeric_limits<double>::infinity()) == 2047);
    double d = 0.0;
    const double z[3] = {50.0, 0.0, 0.0}, q[3] = {50.0, -20.0, 0.0}, e[3] = {50.0, 10.0, 0.0};
    REQUIRE(sr_delta_e_pair(e, q, SR_DELTA_E_2000, &d) == SR_OK && d > 0.0);       // h_diff == pi exactly
    REQUIRE(sr_delta_e_pair(z, q, SR_DELTA_E_2000, &d) == SR_OK && d > 0.0);       // a zero chroma
    REQUIRE(sr_delta_e_pair(z, z, SR_DELTA_E_2000, &d) == SR_OK && d == 0.0);
    REQUIRE(sr_delta_e_pair(nullptr, q, 0, &d) == SR_ERR_INVALID_ARG && sr_delta_e_pair(z, q, 0, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_delta_e_pair(z, q, 2, &d) == SR_ERR_UNSUPPORTED);
    REQUIRE(sr_delta_e_lab_u8(256, 0, 0, lab.get()) == SR_ERR_INVALID_ARG && sr_delta_e_lab_u8(0, -1, 0, lab.get()) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_delta_e_lab_u8(1, 2, 3, nullptr) == SR_ERR_INVALID_ARG);

    // the record's values, on an exact-size heap record
    std::unique_ptr<sr_delta_e_sums> rec(new sr_delta_e_sums());
    rec->hist[0] = 50; rec->hist[16] = 45; rec->hist[48] = 4; rec->hist[SR_DELTA_E_BINS - 1] = 1;
    rec->count = 100; rec->sum = 300.0; rec->sum2 = 2500.0; rec->max = 140.0;
    REQUIRE(sr_delta_e_mean(rec.get()) == 3.0 && sr_delta_e_rms(rec.get()) == 5.0);
    REQUIRE(sr_delta_e_percentile(rec.get(), 50.0) == 0.0 && sr_delta_e_percentile(rec.get(), 51.0) == 1.0);
    REQUIRE(sr_delta_e_percentile(rec.get(), 95.0) == 1.0 && sr_delta_e_percentile(rec.get(), 99.0) == 3.0);
    REQUIRE(sr_delta_e_percentile(rec.get(), 100.0) == (SR_DELTA_E_BINS - 1) / 16.0 && sr_delta_e_percentile(rec.get(), 1e-300) == 0.0);
    for (double p : {0.0, -1.0, 100.5, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()})
        REQUIRE(std::isnan(sr_delta_e_percentile(rec.get(), p)));
    double fr = -1.0;
    REQUIRE(sr_delta_e_fraction_at_least(rec.get(), 0.0, &fr) == SR_OK && fr == 1.0);
    REQUIRE(sr_delta_e_fraction_at_least(rec.get(), 1.0, &fr) == SR_OK && fr == 0.5);
    REQUIRE(sr_delta_e_fraction_at_least(rec.get(), 127.9375, &fr) == SR_OK && fr == 0.01);
    for (double t : {0.1, -0.0625, 128.0, 1e300, -1e300, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()})
        REQUIRE(sr_delta_e_fraction_at_least(rec.get(), t, &fr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_delta_e_fraction_at_least(rec.get(), 1.0, nullptr) == SR_ERR_INVALID_ARG);
    rec->hist[3] = std::numeric_limits<uint64_t>::max();                            // a histogram that overflows its own sum
    REQUIRE(std::isnan(sr_delta_e_percentile(rec.get(), 50.0)) && sr_delta_e_fraction_at_least(rec.get(), 1.0, &fr) == SR_ERR_INVALID_ARG);
    rec->hist[3] = 0;
    rec->count = std::numeric_limits<uint64_t>::max();                              // the largest count: k stays inside it
    rec->hist[0] = rec->count - 50;
    REQUIRE(sr_delta_e_percentile(rec.get(), 100.0) == (SR_DELTA_E_BINS - 1) / 16.0 && sr_delta_e_percentile(rec.get(), 50.0) == 0.0);
    rec->count = 0;
    REQUIRE(std::isnan(sr_delta_e_mean(rec.get())) && std::isnan(sr_delta_e_rms(rec.get())) && std::isnan(sr_delta_e_percentile(rec.get(), 50.0)));
    REQUIRE(std::isnan(sr_delta_e_mean(nullptr)) && std::isnan(sr_delta_e_percentile(nullptr, 50.0)));
    REQUIRE(sr_delta_e_fraction_at_least(nullptr, 1.0, &fr) == SR_ERR_INVALID_ARG);
    printf("deltae-driver-ok\n");
    return 0;
}
