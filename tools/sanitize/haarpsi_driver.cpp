// haarpsi_driver.cpp -- stand-alone driver for the sanitizer run of the host side of HaarPSI (tests/test_haarpsi_sanitize.py):
// compiled with csrc/sr_haarpsi_host.cpp alone under -fsanitize=address,undefined, it takes sr_haarpsi_plan through sizes,
// crops, switches and every refusal and checks each plan the way the kernel uses it; runs sr_haarpsi_host_u8 on exact-size
// heap images (dense, and strided views whose last row ends with the allocation) of every channel count, crop, convention and
// subsampling, against an independent direct evaluation of the definition; and reads the values off records.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "sr_haarpsi.h"

static char g_err[512] = "";

// sr_host.cpp owns this in the library; the driver links sr_haarpsi_host.cpp alone
int sr_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define REQUIRE(cond)                                                                              \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            fprintf(stderr, "haarpsi_driver: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
            return 1;                                                                              \
        }                                                                                          \
    } while (0)

static int one_plan(int h, int w, int cn, int cb, int sub, int conv)
{
    int mh = 0, mw = 0, blocks = 0;
    uint64_t cnt = 0;
    size_t bytes = 0;
    const int rc = sr_haarpsi_plan(h, w, cn, cb, sub, conv, &mh, &mw, &cnt, &blocks, &bytes);
    const long long ch = (long long)h - 2LL * cb, cw = (long long)w - 2LL * cb;
    if (ch < HP_MIN_SIDE || cw < HP_MIN_SIDE) {
        REQUIRE(rc == SR_ERR_SHAPE);
        return 0;
    }
    REQUIRE(rc == SR_OK);
    REQUIRE(mh == (sub ? (ch + 1) / 2 : ch) && mw == (sub ? (cw + 1) / 2 : cw) && cnt == (uint64_t)mh * (uint64_t)mw);
    REQUIRE(sr_haarpsi_plan(h, w, cn, cb, sub, conv, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    HpPlan p;
    REQUIRE(haarpsi_plan("driver", h, w, cn, cb, sub, conv, &p) == SR_OK);
    REQUIRE(p.tiles_x * HP_TW >= mw && (p.tiles_x - 1) * HP_TW < mw && p.tiles_y * HP_TH >= mh && (p.tiles_y - 1) * HP_TH < mh);
    REQUIRE(blocks == p.tiles_x * p.tiles_y && p.channels == (cn == 1 ? 2 : 3));
    const size_t tiles = (size_t)blocks;
    REQUIRE(p.total == bytes && p.off_part % 256 == 0 && p.off_buf0 >= p.off_part + tiles * HP_COMP * sizeof(double));
    REQUIRE(p.off_buf1 >= p.off_buf0 + ((tiles + 1023) / 1024) * HP_COMP * sizeof(double));
    REQUIRE(p.total >= p.off_buf1 + (p.off_buf1 - p.off_buf0));
    return 0;
}

// the definition once more, from the pixels: no pooled planes, every window summed directly
struct Img {
    const uint8_t *p;
    int64_t stride;
    int ch, cw, cn;
    // plane k (0: Y, 1: I, 2: Q; x 1000) of cropped pixel (r, c), zero outside
    long long px(int k, long long r, long long c) const
    {
        if (r < 0 || r >= ch || c < 0 || c >= cw) return 0;
        const uint8_t *q = p + r * stride + c * cn;
        if (cn == 1) return k == 0 ? 1000LL * q[0] : 0;
        const int R = q[0], G = q[1], B = q[2];
        return k == 0 ? 299 * R + 587 * G + 114 * B : k == 1 ? 596 * R - 274 * G - 322 * B : 211 * R - 523 * G + 312 * B;
    }
};

static long long sample(const Img &im, int k, int sub, int o, long long i, long long j, int mh, int mw)
{
    if (i < 0 || i >= mh || j < 0 || j >= mw) return 0;
    if (!sub) return im.px(k, i, j);
    long long s = 0;
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) s += im.px(k, 2 * i - o + dy, 2 * j - o + dx);
    return s;
}

static int one_image(int h, int w, int cn, int cb, int sub, int conv, int pad, unsigned seed)
{
    const int64_t stride = (int64_t)w * cn + pad;
    // exact size: the last row has no pad behind it
    const size_t bytes = (size_t)(h - 1) * (size_t)stride + (size_t)w * cn;
    std::vector<uint8_t> a(bytes), b(bytes);
    unsigned s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < bytes; ++i) {
        s = s * 1664525u + 1013904223u;
        a[i] = (uint8_t)(s >> 24);
        const int v = (int)a[i] + (int)((s >> 12) % 41u) - 20;
        b[i] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
    sr_haarpsi_sums got;
    REQUIRE(sr_haarpsi_host_u8(a.data(), stride, b.data(), stride, h, w, cn, cb, sub, conv, &got) == SR_OK);
    const int ch = h - 2 * cb, cw = w - 2 * cb, mh = sub ? (ch + 1) / 2 : ch, mw = sub ? (cw + 1) / 2 : cw, o = conv;
    const Img ia{a.data() + (size_t)cb * stride + (size_t)cb * cn, stride, ch, cw, cn};
    const Img ib{b.data() + (size_t)cb * stride + (size_t)cb * cn, stride, ch, cw, cn};
    const double div = sub ? 4000.0 : 1000.0, C = 30.0, alpha = 4.2;
    double num[3] = {0, 0, 0}, den[3] = {0, 0, 0};
    for (int i = 0; i < mh; ++i)
        for (int j = 0; j < mw; ++j) {
            double w2[2];
            for (int d = 0; d < 2; ++d) {
                double co[2][3];
                for (int s3 = 0; s3 < 3; ++s3) {
                    const int hf = 1 << s3;
                    long long va = 0, vb = 0;
                    for (int u = -hf + 1; u <= hf; ++u)
                        for (int v = -hf + 1; v <= hf; ++v) {
                            const int sign = (d == 0 ? u : v) <= 0 ? 1 : -1;
                            va += sign * sample(ia, 0, sub, o, (long long)i - o + u, (long long)j - o + v, mh, mw);
                            vb += sign * sample(ib, 0, sub, o, (long long)i - o + u, (long long)j - o + v, mh, mw);
                        }
                    co[0][s3] = (double)std::llabs(va) / (div * (2 << s3));
                    co[1][s3] = (double)std::llabs(vb) / (div * (2 << s3));
                }
                w2[d] = co[0][2] > co[1][2] ? co[0][2] : co[1][2];
                double ls = 0.0;
                for (int s3 = 0; s3 < 2; ++s3)
                    ls += (2.0 * co[0][s3] * co[1][s3] + C) / (co[0][s3] * co[0][s3] + co[1][s3] * co[1][s3] + C);
                num[d] += w2[d] / (1.0 + std::exp(-alpha * 0.5 * ls));
                den[d] += w2[d];
            }
            if (cn >= 3) {
                double ls = 0.0;
                for (int k = 1; k <= 2; ++k) {
                    long long ca = 0, cb2 = 0;
                    for (int u = 0; u < 2; ++u)
                        for (int v = 0; v < 2; ++v) {
                            ca += sample(ia, k, sub, o, (long long)i - o + u, (long long)j - o + v, mh, mw);
                            cb2 += sample(ib, k, sub, o, (long long)i - o + u, (long long)j - o + v, mh, mw);
                        }
                    const double x = (double)std::llabs(ca) / (4.0 * div), y = (double)std::llabs(cb2) / (4.0 * div);
                    ls += (2.0 * x * y + C) / (x * x + y * y + C);
                }
                const double wc = 0.5 * (w2[0] + w2[1]);
                num[2] += wc / (1.0 + std::exp(-alpha * 0.5 * ls));
                den[2] += wc;
            }
        }
    REQUIRE(got.channels == (cn == 1 ? 2 : 3) && got.count == (uint64_t)mh * (uint64_t)mw);
    double sn = 0.0, sd = 0.0;
    for (int k = 0; k < 3; ++k) {
        REQUIRE(std::fabs(got.num[k] - num[k]) <= 1e-12 * num[k] && std::fabs(got.den[k] - den[k]) <= 1e-12 * den[k]);
        if (k < got.channels) {
            sn += got.num[k];
            sd += got.den[k];
        }
    }
    const double v = sr_haarpsi_value(&got);
    REQUIRE(v == sr_haarpsi_cell_value(sn, sd) && v > 0.0 && v < 1.0);
    // identity: 1 within 1e-12
    REQUIRE(sr_haarpsi_host_u8(a.data(), stride, a.data(), stride, h, w, cn, cb, sub, conv, &got) == SR_OK);
    REQUIRE(std::fabs(sr_haarpsi_value(&got) - 1.0) <= 1e-12);
    return 0;
}

int main()
{
    const int sides[] = {1, 2, 3, 4, 5, 7, 8, 29, 30, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 257, 1052, 4097, 20011};
    for (int h : sides)
        for (int w : sides)
            for (int cb = 0; cb <= 3; ++cb)
                for (int sw = 0; sw < 4; ++sw)
                    if (one_plan(h, w, (h + w) % 3 == 0 ? 1 : (h + w) % 3 == 1 ? 3 : 4, cb, sw & 1, sw >> 1)) return 1;
    // the largest sides an int holds: the sizes are formed in 64 bits
    REQUIRE(sr_haarpsi_plan(2147483647, 2, 1, 0, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    REQUIRE(sr_haarpsi_plan(2147483647, 2, 3, 0, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    REQUIRE(sr_haarpsi_plan(2, 2147483647, 4, 0, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    REQUIRE(sr_haarpsi_plan(2147483647, 2147483647, 3, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    REQUIRE(sr_haarpsi_plan(2147483647, 2147483647, 3, 1073741822, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_OK);
    REQUIRE(sr_haarpsi_plan(2147483647, 2147483647, 3, 1073741823, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_SHAPE);
    // refusals
    REQUIRE(sr_haarpsi_plan(64, 64, 2, 0, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_haarpsi_plan(64, 64, 3, -1, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_haarpsi_plan(64, 64, 3, 0, 2, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_haarpsi_plan(64, 64, 3, 0, 1, 2, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_haarpsi_plan(0, 64, 3, 0, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    {
        std::vector<uint8_t> img(4 * 4 * 3, 9);
        sr_haarpsi_sums out;
        REQUIRE(sr_haarpsi_host_u8(nullptr, 12, img.data(), 12, 4, 4, 3, 0, 1, 0, &out) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_haarpsi_host_u8(img.data(), 12, img.data(), 12, 4, 4, 3, 0, 1, 0, nullptr) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_haarpsi_host_u8(img.data(), 11, img.data(), 12, 4, 4, 3, 0, 1, 0, &out) == SR_ERR_SHAPE);
        REQUIRE(sr_haarpsi_host_u8(img.data(), 12, img.data(), 12, 4, 4, 3, 2, 1, 0, &out) == SR_ERR_SHAPE);
    }
    // images: every channel count, crop, convention and subsampling, dense and padded
    unsigned seed = 1;
    const int shapes[][2] = {{2, 2}, {2, 3}, {3, 5}, {7, 8}, {9, 6}, {17, 33}, {20, 19}};
    for (const auto &sh : shapes)
        for (int cn : {1, 3, 4})
            for (int cb = 0; cb <= 2; ++cb) {
                if (sh[0] - 2 * cb < HP_MIN_SIDE || sh[1] - 2 * cb < HP_MIN_SIDE) continue;
                for (int sw = 0; sw < 4; ++sw)
                    if (one_image(sh[0], sh[1], cn, cb, sw & 1, sw >> 1, (seed % 3) * 5, seed++)) return 1;
            }
    // values
    sr_haarpsi_sums r = {{1.0, 2.0, 3.0}, {2.0, 4.0, 6.0}, 3, 0, 10};       // x = 1 / 2: the logit is 0
    REQUIRE(sr_haarpsi_value(&r) == 0.0);
    r.channels = 2;
    r.num[2] = 1e9;                                                          // a gray record ignores the third channel
    REQUIRE(sr_haarpsi_value(&r) == 0.0);
    r = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 3, 0, 10};
    REQUIRE(std::isnan(sr_haarpsi_value(&r)) && std::isnan(sr_haarpsi_cell_value(0.0, 0.0)));
    r.channels = 4;
    REQUIRE(std::isnan(sr_haarpsi_value(&r)) && std::isnan(sr_haarpsi_value(nullptr)));
    const double x = 1.0 / (1.0 + std::exp(-4.2));
    REQUIRE(std::fabs(sr_haarpsi_cell_value(x, 1.0) - 1.0) <= 1e-12);
    printf("haarpsi-driver-ok\n");
    return 0;
}
