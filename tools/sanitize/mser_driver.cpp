// mser_driver.cpp -- stand-alone driver for the sanitizer run of the host side of MSER (tests/test_mser_sanitize.py): compiled
// with csrc/sr_mser_host.cpp alone under -fsanitize=address,undefined, it takes sr_mser_plan through sizes up to the cap and
// every refusal, checks the layout the way the kernels use it, runs sr_mser_tree_host_u8 and sr_mser_host_u8 on exact-size
// heap images (dense and strided, every channel count, both polarities) against a flood-fill evaluation of the definition,
// and the text-box filter at its edges.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "sr_mser.h"

static char g_err[512] = "";

// sr_host.cpp owns this in the library; the driver links sr_mser_host.cpp alone
int sr_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define REQUIRE(cond)                                                                           \
    do {                                                                                        \
        if (!(cond)) {                                                                          \
            fprintf(stderr, "mser_driver: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)

static int one_plan(int h, int w)
{
    sr_mser_params p;
    REQUIRE(sr_mser_default_params(&p) == SR_OK);
    size_t bytes = 0;
    int64_t cap = 0;
    const int rc = sr_mser_plan(h, w, &p, &bytes, &cap);
    const long long n = (long long)h * w;
    if (n > MSER_MAX_PIXELS) {
        REQUIRE(rc == SR_ERR_UNSUPPORTED);
        return 0;
    }
    REQUIRE(rc == SR_OK && cap == n && sr_mser_plan(h, w, &p, nullptr, nullptr) == SR_OK);
    MserPlan l;
    mser_layout(h, w, &l);
    REQUIRE(l.total == bytes && bytes < ((size_t)1 << 30) && bytes <= (size_t)n * 53 + 12288);
    REQUIRE(l.off_order >= (size_t)n && l.off_parent >= l.off_order + (size_t)n * 4 && l.off_nor >= l.off_parent + (size_t)n * 4);
    REQUIRE(l.off_list >= l.off_nor + (size_t)n * 4 && l.list_bytes >= (size_t)n * 8 && l.list_bytes >= sizeof(sr_mser_region));
    REQUIRE(l.off_nodes == l.off_list + l.list_bytes && l.off_ctr >= l.off_nodes + (size_t)n * sizeof(MserNode));
    REQUIRE(l.total == l.off_ctr + 4096);
    for (size_t o : {l.off_order, l.off_parent, l.off_nor, l.off_list, l.off_nodes, l.off_ctr}) REQUIRE(o % 256 == 0);
    return 0;
}

// The definition by flood fill: for every level the components of {g <= t}; a node per component holding a pixel of value t.
struct Ref {
    int level, area, x0, y0, x1, y1, seed;
    std::vector<char> in;
};

static std::vector<Ref> flood_tree(const std::vector<uint8_t> &g, int h, int w)
{
    std::vector<Ref> out;
    for (int t = 0; t < 256; ++t) {
        std::vector<char> seen((size_t)h * w, 0);
        for (int s = 0; s < h * w; ++s) {
            if (seen[s] || g[s] > t) continue;
            Ref r{t, 0, w, h, -1, -1, s, std::vector<char>((size_t)h * w, 0)};
            bool has = false;
            std::vector<int> stack{s};
            seen[s] = 1;
            while (!stack.empty()) {
                const int p = stack.back(), y = p / w, x = p % w;
                stack.pop_back();
                r.in[p] = 1;
                ++r.area;
                has = has || g[p] == t;
                r.x0 = std::min(r.x0, x);
                r.y0 = std::min(r.y0, y);
                r.x1 = std::max(r.x1, x);
                r.y1 = std::max(r.y1, y);
                const int nb[4] = {y > 0 ? p - w : -1, y + 1 < h ? p + w : -1, x > 0 ? p - 1 : -1, x + 1 < w ? p + 1 : -1};
                for (int q : nb)
                    if (q >= 0 && !seen[q] && g[q] <= t) {
                        seen[q] = 1;
                        stack.push_back(q);
                    }
            }
            if (has) out.push_back(std::move(r));
        }
    }
    return out;
}

static int one_image(int h, int w, int cn, int pad, int levels, unsigned seed)
{
    const int64_t stride = (int64_t)w * cn + pad;
    const size_t bytes = (size_t)(h - 1) * (size_t)stride + (size_t)w * cn;      // exact size: no pad behind the last row
    std::vector<uint8_t> img(bytes);
    unsigned s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < bytes; ++i) {
        s = s * 1664525u + 1013904223u;
        img[i] = (uint8_t)(((s >> 24) % (unsigned)levels) * (255u / (unsigned)levels));
    }
    for (int pol = 0; pol < 2; ++pol) {
        std::vector<uint8_t> g((size_t)h * w);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const uint8_t *px = img.data() + (size_t)y * stride + (size_t)x * cn;
                const int v = cn == 1 ? px[0] : (px[0] * 3735 + px[1] * 19235 + px[2] * 9798 + (1 << 14)) >> 15;
                g[(size_t)y * w + x] = (uint8_t)(pol ? 255 - v : v);
            }
        const std::vector<Ref> ref = flood_tree(g, h, w);            // already in (level, seed) order
        std::vector<sr_mser_node> got((size_t)h * w);
        int64_t n = 0;
        REQUIRE(sr_mser_tree_host_u8(img.data(), stride, h, w, cn, pol, got.data(), (int64_t)got.size(), &n) == SR_OK);
        REQUIRE(n == (int64_t)ref.size());
        for (size_t i = 0; i < ref.size(); ++i) {
            const Ref &r = ref[i];
            const sr_mser_node &q = got[i];
            REQUIRE(q.level == r.level && q.area == r.area && q.x0 == r.x0 && q.y0 == r.y0 && q.x1 == r.x1 && q.y1 == r.y1 &&
                    q.seed == r.seed);
            // the parent: the node of the smallest level above that contains the seed
            int pl = -1, ps = -1;
            for (size_t j = i + 1; j < ref.size(); ++j)
                if (ref[j].level > r.level && ref[j].in[r.seed]) {
                    pl = ref[j].level;
                    ps = ref[j].seed;
                    break;
                }
            REQUIRE(q.parent_level == pl && q.parent_seed == ps);
        }
        // a short buffer: the count alone
        int64_t n2 = 0;
        REQUIRE(sr_mser_tree_host_u8(img.data(), stride, h, w, cn, pol, got.data(), 0, &n2) == SR_OK && n2 == n);
    }
    // regions: sorted, inside the image, consistent with their own records; a short buffer still reports the total
    sr_mser_params p;
    sr_mser_default_params(&p);
    p.min_area = 1;
    std::vector<sr_mser_region> regs((size_t)2 * h * w);
    int64_t n = 0;
    REQUIRE(sr_mser_host_u8(img.data(), stride, h, w, cn, &p, 3, regs.data(), (int64_t)regs.size(), &n) == SR_OK);
    REQUIRE(n >= 1 && n <= (int64_t)regs.size());
    for (int64_t i = 0; i < n; ++i) {
        const sr_mser_region &r = regs[i];
        REQUIRE(r.polarity >= 0 && r.polarity <= 1 && r.area >= 1 && r.S >= r.area && r.x0 >= 0 && r.y0 >= 0 && r.x1 < w && r.y1 < h);
        REQUIRE(r.area <= (r.x1 - r.x0 + 1) * (r.y1 - r.y0 + 1) && r.seed >= r.y0 * w + r.x0 && r.seed <= r.y0 * w + r.x1);
        if (i > 0) {
            const sr_mser_region &q = regs[i - 1];
            REQUIRE(q.polarity < r.polarity || (q.polarity == r.polarity && (q.level < r.level || (q.level == r.level && q.seed < r.seed))));
        }
    }
    sr_mser_region one;
    int64_t n1 = 0;
    REQUIRE(sr_mser_host_u8(img.data(), stride, h, w, cn, &p, 3, &one, 1, &n1) == SR_OK && n1 == n);
    REQUIRE(one.level == regs[0].level && one.seed == regs[0].seed);
    int64_t nd = 0, nb = 0;
    REQUIRE(sr_mser_host_u8(img.data(), stride, h, w, cn, &p, 1, nullptr, 0, &nd) == SR_OK);
    REQUIRE(sr_mser_host_u8(img.data(), stride, h, w, cn, &p, 2, nullptr, 0, &nb) == SR_OK && nd + nb == n);
    return 0;
}

int main()
{
    const int sides[] = {1, 2, 3, 7, 63, 64, 65, 255, 256, 257, 1080, 4095, 4096, 4097, 65536, 2147483647};
    for (int h : sides)
        for (int w : sides)
            if (one_plan(h, w)) return 1;
    // refusals
    sr_mser_params d, p;
    sr_mser_default_params(&d);
    REQUIRE(d.delta == 5 && d.min_area == 60 && d.max_area == 14400 && d.max_variation == 0.25 && d.min_diversity == 0.2);
    REQUIRE(sr_mser_default_params(nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_mser_plan(0, 4, &d, nullptr, nullptr) == SR_ERR_INVALID_ARG && sr_mser_plan(4, 4, nullptr, nullptr, nullptr) == SR_ERR_INVALID_ARG);
    REQUIRE(sr_mser_plan(4096, 4097, &d, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
    for (int delta : {0, 256, -1}) {
        p = d;
        p.delta = delta;
        REQUIRE(sr_mser_plan(8, 8, &p, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
    }
    for (int delta : {1, 255}) {
        p = d;
        p.delta = delta;
        REQUIRE(sr_mser_plan(8, 8, &p, nullptr, nullptr) == SR_OK);
    }
    p = d;
    p.min_area = 0;
    REQUIRE(sr_mser_plan(8, 8, &p, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
    p = d;
    p.max_area = p.min_area - 1;
    REQUIRE(sr_mser_plan(8, 8, &p, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
    p.max_area = p.min_area;
    REQUIRE(sr_mser_plan(8, 8, &p, nullptr, nullptr) == SR_OK);
    for (double bad : {-1e-300, -1.0, std::numeric_limits<double>::quiet_NaN()}) {
        p = d;
        p.max_variation = bad;
        REQUIRE(sr_mser_plan(8, 8, &p, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
        p = d;
        p.min_diversity = bad;
        REQUIRE(sr_mser_plan(8, 8, &p, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
    }
    {
        std::vector<uint8_t> img(4 * 4 * 3, 9);
        sr_mser_region r;
        sr_mser_node nd;
        int64_t n = 0;
        REQUIRE(sr_mser_host_u8(nullptr, 12, 4, 4, 3, &d, 3, &r, 1, &n) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_mser_host_u8(img.data(), 11, 4, 4, 3, &d, 3, &r, 1, &n) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_mser_host_u8(img.data(), 12, 4, 4, 2, &d, 3, &r, 1, &n) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_mser_host_u8(img.data(), 12, 4, 4, 3, &d, 0, &r, 1, &n) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_mser_host_u8(img.data(), 12, 4, 4, 3, &d, 4, &r, 1, &n) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_mser_host_u8(img.data(), 12, 4, 4, 3, &d, 3, nullptr, 1, &n) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_mser_host_u8(img.data(), 12, 4, 4, 3, &d, 3, &r, 1, nullptr) == SR_ERR_INVALID_ARG);
        p = d;
        p.delta = 0;
        REQUIRE(sr_mser_host_u8(img.data(), 12, 4, 4, 3, &p, 3, &r, 1, &n) == SR_ERR_UNSUPPORTED);
        REQUIRE(sr_mser_tree_host_u8(img.data(), 12, 4, 4, 3, 2, &nd, 1, &n) == SR_ERR_INVALID_ARG);
        REQUIRE(sr_mser_tree_host_u8(img.data(), 12, 4, 4, 3, 0, &nd, 1, &n) == SR_OK && n == 1 && nd.area == 16 && nd.parent_level == -1);
    }
    // images: every channel count, dense and padded, few and many levels
    unsigned seed = 1;
    const int shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {3, 5}, {9, 6}, {13, 16}, {16, 16}};
    for (const auto &sh : shapes)
        for (int cn : {1, 3, 4})
            for (int levels : {2, 5, 255}) {
                if (one_image(sh[0], sh[1], cn, (int)(seed % 3) * 5, levels, seed)) return 1;
                ++seed;
            }
    // text boxes: w 20 / 21, h 10 / 11, w against W / 2 for odd and even W
    auto box = [](int w, int h) { return sr_mser_region{0, 1, w * h, 3, 4, 3 + w - 1, 4 + h - 1, 0, w * h}; };
    const sr_mser_region regs[] = {box(20, 30), box(21, 30), box(30, 10), box(30, 11), box(49, 12), box(50, 12), box(51, 12), box(21, 30)};
    sr_tile_rect rects[8];
    int64_t m = -1;
    REQUIRE(sr_mser_text_boxes(regs, 8, 100, rects, &m) == SR_OK && m == 4);          // 21x30, 30x11, 49x12, 21x30 again (50 < 50.0 fails)
    REQUIRE(rects[0].x == 3 && rects[0].y == 4 && rects[0].w == 21 && rects[0].h == 30 && rects[1].h == 11 && rects[2].w == 49 &&
            rects[3].w == 21);
    REQUIRE(sr_mser_text_boxes(regs, 8, 101, rects, &m) == SR_OK && m == 5 && rects[3].w == 50);      // 50 < 50.5, 51 is not
    REQUIRE(sr_mser_text_boxes(regs, 8, 103, rects, &m) == SR_OK && m == 6 && rects[4].w == 51);      // 51 < 51.5
    REQUIRE(sr_mser_text_boxes(nullptr, 0, 100, nullptr, &m) == SR_OK && m == 0);
    REQUIRE(sr_mser_text_boxes(regs, 8, 0, rects, &m) == SR_ERR_INVALID_ARG && sr_mser_text_boxes(regs, 8, 100, rects, nullptr) == SR_ERR_INVALID_ARG);
    printf("mser-driver-ok\n");
    return 0;
}
