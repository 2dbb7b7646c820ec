// cascade_driver.cpp -- stand-alone driver for the sanitizer run of the host side of cascade detection
// (tests/test_cascade_sanitize.py): compiled with csrc/sr_cascade_host.cpp alone under -fsanitize=address,undefined, it
// builds LBP and HAAR models whose features touch the window's far corner, takes sr_cascade_create through its refusals and
// sr_cascade_plan through sizes up to the cap, checks the layout the way the kernels use it, and runs the restatement, the
// planes and the stage maps on exact-size heap images (dense and strided, every channel count, the window itself, one row
// more) against a direct evaluation without tables; then the grouping on short and empty lists and short output buffers.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "sr_cascade.h"

static char g_err[512] = "";

// sr_host.cpp owns this in the library; the driver links sr_cascade_host.cpp alone
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
            fprintf(stderr, "cascade_driver: %s failed at line %d (%s)\n", #cond, __LINE__, g_err); \
            return 1;                                                                              \
        }                                                                                          \
    } while (0)

static unsigned g_seed = 12345u;
static unsigned rnd_u()
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}

struct Tables {
    sr_cascade_info info{};
    std::vector<float> stage_thr, stump_thr, leaves, weights;
    std::vector<int> stage_count, stump_feature, nrects, rects;
    std::vector<int32_t> subsets;
    int create(sr_cascade **out) const
    {
        return sr_cascade_create(&info, stage_thr.data(), stage_count.data(), stump_feature.data(), stump_thr.data(), leaves.data(),
                                 subsets.data(), nrects.data(), rects.data(), weights.data(), out);
    }
};

// W0 x H0 model; feature 0 reaches the far corner of the window
static Tables make_tables(int type, int W0, int H0, const std::vector<int> &stages)
{
    Tables t;
    const int nf = 6;
    int ns = 0;
    for (int c : stages) ns += c;
    t.info = {type, W0, H0, (int)stages.size(), ns, nf, 0, 0, 1, 0, type == SR_CASCADE_HAAR ? 3 : 0, 256};
    for (int c : stages) {
        t.stage_count.push_back(c);
        t.stage_thr.push_back(-0.4f * std::sqrt((float)c));
    }
    for (int k = 0; k < ns; ++k) {
        t.stump_feature.push_back(k % nf);
        t.stump_thr.push_back(((int)(rnd_u() % 2001) - 1000) * 1e-5f);
        t.leaves.push_back(((int)(rnd_u() % 2001) - 1000) * 1e-3f);
        t.leaves.push_back(((int)(rnd_u() % 2001) - 1000) * 1e-3f);
        for (int j = 0; j < 8; ++j) t.subsets.push_back((int32_t)(rnd_u() * 2654435761u));
    }
    for (int i = 0; i < nf; ++i) {
        if (type == SR_CASCADE_LBP) {
            const int bw = i == 0 ? W0 / 3 : 1 + (int)(rnd_u() % (W0 / 3)), bh = i == 0 ? H0 / 3 : 1 + (int)(rnd_u() % (H0 / 3));
            const int x = i == 0 ? W0 - 3 * bw : (int)(rnd_u() % (W0 - 3 * bw + 1)), y = i == 0 ? H0 - 3 * bh : (int)(rnd_u() % (H0 - 3 * bh + 1));
            for (int v : {x, y, bw, bh}) t.rects.push_back(v);
        } else {
            const int n = 2 + i % 2;
            t.nrects.push_back(n);
            const int ow = i == 0 ? W0 : 2 + (int)(rnd_u() % (W0 - 1)), oh = i == 0 ? H0 : 2 + (int)(rnd_u() % (H0 - 1));
            const int ox = W0 - ow - (i == 0 ? 0 : (int)(rnd_u() % (W0 - ow + 1))), oy = H0 - oh - (i == 0 ? 0 : (int)(rnd_u() % (H0 - oh + 1)));
            for (int j = 0; j < 3; ++j) {
                const int rw = j == 0 ? ow : 1 + (int)(rnd_u() % (ow - 1)), rh = j == 0 ? oh : 1 + (int)(rnd_u() % (oh - 1));
                const int rx = ox + ow - rw, ry = oy + oh - rh;               // every rectangle ends at the outer one's far corner
                for (int v : {j < n ? rx : 0, j < n ? ry : 0, j < n ? rw : 0, j < n ? rh : 0}) t.rects.push_back(v);
                t.weights.push_back(j == 0 ? -1.f : j < n ? (float)(ow * oh) / (float)((n - 1) * rw * rh) : 0.f);
            }
        }
    }
    return t;
}

// the definition without tables: sums over pixels
static long long px_sum(const std::vector<uint8_t> &p, int pw, int x, int y, int w, int h, bool sq)
{
    long long s = 0;
    for (int yy = y; yy < y + h; ++yy)
        for (int xx = x; xx < x + w; ++xx) s += sq ? (long long)p[(size_t)yy * pw + xx] * p[(size_t)yy * pw + xx] : p[(size_t)yy * pw + xx];
    return s;
}

static int direct_stages(const Tables &t, const std::vector<uint8_t> &p, int pw, int x, int y)
{
    const int W0 = t.info.win_w, H0 = t.info.win_h;
    double nf = 1.0;
    if (t.info.feature_type == SR_CASCADE_HAAR) {
        const long long A = (long long)(W0 - 2) * (H0 - 2), s = px_sum(p, pw, x + 1, y + 1, W0 - 2, H0 - 2, false),
                        q = px_sum(p, pw, x + 1, y + 1, W0 - 2, H0 - 2, true), v = A * q - s * s;
        nf = v > 0 ? std::sqrt((double)v) : 1.0;
    }
    int k = 0;
    for (int si = 0; si < t.info.n_stages; ++si) {
        float sum = 0.f;
        for (int c = 0; c < t.stage_count[si]; ++c, ++k) {
            const int fi = t.stump_feature[k];
            bool first;
            if (t.info.feature_type == SR_CASCADE_HAAR) {
                double val = 0.0;
                for (int i = 0; i < t.nrects[fi]; ++i) {
                    const int *r = &t.rects[12 * (size_t)fi + 4 * i];
                    const double prod = (double)t.weights[3 * (size_t)fi + i] * (double)px_sum(p, pw, x + r[0], y + r[1], r[2], r[3], false);
                    val = i ? val + prod : prod;
                }
                first = val < (double)t.stump_thr[k] * nf;
            } else {
                const int *r = &t.rects[4 * (size_t)fi];
                long long b[9];
                for (int j = 0; j < 9; ++j) b[j] = px_sum(p, pw, x + r[0] + (j % 3) * r[2], y + r[1] + (j / 3) * r[3], r[2], r[3], false);
                const int order[8] = {0, 1, 2, 5, 8, 7, 6, 3};
                unsigned code = 0;
                for (int j = 0; j < 8; ++j) code = code << 1 | (unsigned)(b[order[j]] >= b[4]);
                first = ((uint32_t)t.subsets[8 * (size_t)k + (code >> 5)] >> (code & 31u) & 1u) != 0u;
            }
            sum = sum + t.leaves[2 * (size_t)k + (first ? 0 : 1)];
        }
        if (sum < t.stage_thr[si]) return si;
    }
    return t.info.n_stages;
}

static int one_image(const Tables &t, const sr_cascade *m, int h, int w, int cn, int pad)
{
    const int64_t stride = (int64_t)w * cn + pad;
    std::vector<uint8_t> img((size_t)(stride * (h - 1) + (int64_t)w * cn));                // exact size: not a byte after the last pixel
    for (uint8_t &v : img) v = (uint8_t)(rnd_u() % 7 == 0 ? rnd_u() : 100 + rnd_u() % 40);
    std::vector<uint8_t> g((size_t)h * w);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint8_t *px = &img[(size_t)(y * stride) + (size_t)x * cn];
            g[(size_t)y * w + x] = (uint8_t)(cn == 1 ? px[0] : (px[0] * 3735 + px[1] * 19235 + px[2] * 9798 + (1 << 14)) >> 15);
        }
    sr_cascade_params p;
    REQUIRE(sr_cascade_default_params(&p) == SR_OK);
    p.scale_factor = 1.3;
    std::vector<sr_cascade_scale> sc(SR_CASCADE_MAX_SCALES);
    int ns = 0;
    size_t bytes = 0;
    int64_t positions = 0;
    REQUIRE(sr_cascade_plan(m, h, w, &p, sc.data(), (int)sc.size(), &ns, &bytes, &positions) == SR_OK);
    const int W0 = t.info.win_w, H0 = t.info.win_h;
    REQUIRE((ns > 0) == (w >= W0 && h >= H0));
    // stage maps of the gray plane itself against the direct evaluation
    for (int step = 1; step <= 2; ++step) {
        const int nx = w >= W0 && h >= H0 ? (w - W0) / step + 1 : 0, ny = nx ? (h - H0) / step + 1 : 0;
        std::vector<int32_t> map((size_t)nx * ny);                                         // exact size
        int64_t count = -1;
        REQUIRE(sr_cascade_stage_map_host_u8(m, img.data(), stride, h, w, cn, step, map.data(), (int64_t)map.size(), &count) == SR_OK);
        REQUIRE(count == (int64_t)map.size());
        for (int iy = 0; iy < ny; ++iy)
            for (int ix = 0; ix < nx; ++ix) REQUIRE(map[(size_t)iy * nx + ix] == direct_stages(t, g, w, ix * step, iy * step));
        if (!map.empty()) {
            int32_t none = -7;
            REQUIRE(sr_cascade_stage_map_host_u8(m, img.data(), stride, h, w, cn, step, &none, 0, &count) == SR_OK && none == -7);
        }
    }
    // planes: exact-size outputs; scale 0 is the gray plane
    long long want_positions = 0;
    for (int k = 0; k < ns; ++k) {
        std::vector<uint8_t> plane((size_t)sc[k].sw * sc[k].sh);
        REQUIRE(sr_cascade_plane_host_u8(m, img.data(), stride, h, w, cn, &p, k, plane.data()) == SR_OK);
        if (sc[k].f == 1.0) REQUIRE(plane == g);
        REQUIRE(sc[k].nx == (sc[k].sw - W0) / sc[k].step + 1 && sc[k].ny == (sc[k].sh - H0) / sc[k].step + 1);
        want_positions += (long long)sc[k].nx * sc[k].ny;
    }
    REQUIRE(positions == want_positions);
    REQUIRE(ns == 0 || sr_cascade_plane_host_u8(m, img.data(), stride, h, w, cn, &p, ns, g.data()) == SR_ERR_INVALID_ARG);
    // candidates: the count alone, a short buffer, the whole list; scale-0 candidates against the direct evaluation
    int64_t n = -1;
    REQUIRE(sr_cascade_host_u8(m, img.data(), stride, h, w, cn, &p, nullptr, 0, &n) == SR_OK && n >= 0 && n <= positions);
    std::vector<sr_tile_rect> all((size_t)n), part((size_t)(n / 2));
    int64_t n2 = -1;
    REQUIRE(sr_cascade_host_u8(m, img.data(), stride, h, w, cn, &p, all.data(), n, &n2) == SR_OK && n2 == n);
    REQUIRE(sr_cascade_host_u8(m, img.data(), stride, h, w, cn, &p, part.data(), (int64_t)part.size(), &n2) == SR_OK && n2 == n);
    for (size_t i = 0; i < part.size(); ++i) REQUIRE(part[i].x == all[i].x && part[i].y == all[i].y && part[i].w == all[i].w);
    size_t at = 0;
    if (ns)
        for (int y = 0; y + H0 <= h; y += 2)
            for (int x = 0; x + W0 <= w; x += 2)
                if (direct_stages(t, g, w, x, y) == t.info.n_stages) {
                    REQUIRE(at < all.size() && all[at].x == x && all[at].y == y && all[at].w == W0 && all[at].h == H0);
                    ++at;
                }
    REQUIRE(at == all.size() || all[at].w > W0 || all[at].h > H0);
    for (const sr_tile_rect &r : all) REQUIRE(r.x >= 0 && r.y >= 0 && r.w >= W0 && r.h >= H0);
    // the grouping on what was found, into an exact-size output
    std::vector<sr_tile_rect> boxes(all.size());
    int64_t nb = -1;
    REQUIRE(sr_cascade_group(all.data(), n, 1, boxes.data(), &nb) == SR_OK && nb >= 0 && nb <= n);
    REQUIRE(sr_cascade_group(all.data(), n, 0, boxes.data(), &nb) == SR_OK && nb == n);
    return 0;
}

static int one_plan(const sr_cascade *m, int h, int w, double factor)
{
    sr_cascade_params p;
    REQUIRE(sr_cascade_default_params(&p) == SR_OK);
    p.scale_factor = factor;
    CcPlan pl;
    const int rc = cascade_plan("driver", m, h, w, &p, &pl);
    if ((long long)h * w > CC_MAX_PIXELS) {
        REQUIRE(rc == SR_ERR_UNSUPPORTED);
        return 0;
    }
    REQUIRE(rc == SR_OK && pl.dev.size() == pl.scales.size() && pl.scales.size() <= SR_CASCADE_MAX_SCALES);
    long long pix = 0, tab = 0, pos = 0, rows = 0, cols = 0;
    for (size_t k = 0; k < pl.dev.size(); ++k) {
        const CcScale &d = pl.dev[k];
        REQUIRE(d.pix_off == pix && d.tab_off == tab && d.pos_off == pos && d.row_off == rows && d.col_off == cols);
        REQUIRE(d.sw >= m->info.win_w && d.sh >= m->info.win_h && d.sw <= w && d.sh <= h && d.nx >= 1 && d.ny >= 1);
        REQUIRE((d.nx - 1) * d.step + m->info.win_w <= d.sw && (d.ny - 1) * d.step + m->info.win_h <= d.sh);
        pix += (long long)d.sw * d.sh;
        tab += (long long)(d.sw + 1) * (d.sh + 1);
        pos += (long long)d.nx * d.ny;
        rows += d.sh;
        cols += d.sw + 1;
    }
    REQUIRE(pix == pl.plane_px && tab == pl.table_el && pos == pl.positions && tab < std::numeric_limits<int>::max());
    REQUIRE(pl.off_planes >= (size_t)pl.npx && pl.off_tab >= pl.off_planes + (size_t)pix && pl.off_sq >= pl.off_tab + (size_t)tab * 4);
    REQUIRE(pl.off_stumps >= pl.off_sq + (m->info.feature_type == SR_CASCADE_HAAR ? (size_t)tab * 4 : 0));
    REQUIRE(pl.off_stages >= pl.off_stumps + m->stumps.size() * 4 && pl.off_scales >= pl.off_stages + m->stages.size() * sizeof(CcStage));
    REQUIRE(pl.off_ctr >= pl.off_scales + pl.dev.size() * sizeof(CcScale) && pl.off_surv >= pl.off_ctr + 8);
    REQUIRE(pl.off_cand >= pl.off_surv + (size_t)pos * 4 && pl.total >= pl.off_cand + (size_t)pos * 4 &&
            pl.total <= (size_t)pl.npx + (size_t)pix + (size_t)tab * 8 + (size_t)pos * 8 + ((size_t)1 << 20));
    for (size_t o : {pl.off_planes, pl.off_tab, pl.off_sq, pl.off_stumps, pl.off_stages, pl.off_scales, pl.off_ctr, pl.off_surv, pl.off_cand})
        REQUIRE(o % 256 == 0);
    return 0;
}

int main()
{
    for (int type : {SR_CASCADE_LBP, SR_CASCADE_HAAR}) {
        const Tables t = make_tables(type, 9, 7, {2, 0, 5, 70, 3});
        sr_cascade *m = nullptr;
        REQUIRE(t.create(&m) == SR_OK && m && m->dense_stages == 3 && m->dense_stumps == 7);
        sr_cascade_info back;
        REQUIRE(sr_cascade_desc(m, &back) == SR_OK && back.n_stumps == 80 && back.win_w == 9);
        for (int cn : {1, 3, 4})
            for (int pad : {0, 5}) {
                if (one_image(t, m, 7, 9, cn, pad)) return 1;          // the window itself
                if (one_image(t, m, 8, 9, cn, pad)) return 1;
                if (one_image(t, m, 6, 30, cn, pad)) return 1;         // smaller than the window: no scale
                if (one_image(t, m, 23, 31, cn, pad)) return 1;
            }
        for (double f : {1.05, 1.1, 2.0, 9.0})
            for (int hw : {1, 7, 9, 10, 255, 256, 257, 1000, 4095}) {
                if (one_plan(m, hw, hw + 3, f) || one_plan(m, 4096, hw, f)) return 1;
            }
        if (one_plan(m, 4096, 4096, 1.1) || one_plan(m, 4097, 4096, 1.1) || one_plan(m, 7, 1 << 21, 1.1)) return 1;
        if (one_plan(m, std::numeric_limits<int>::max(), std::numeric_limits<int>::max(), 1.1)) return 1;
        // refusals: every one leaves *out null and nothing allocated
        auto refused = [](Tables b) {
            sr_cascade *o = (sr_cascade *)1;
            return b.create(&o) == SR_ERR_UNSUPPORTED && o == nullptr;
        };
        Tables b = t;
        b.info.old_layout = 1;
        REQUIRE(refused(b));
        b = t, b.info.stage_type = 1;
        REQUIRE(refused(b));
        b = t, b.info.max_tree_nodes = 2;
        REQUIRE(refused(b));
        b = t, b.info.win_w = 256;
        REQUIRE(refused(b));
        b = t, b.info.win_h = 2;
        REQUIRE(refused(b));
        b = t, b.info.n_stages = 0;
        REQUIRE(refused(b));
        b = t, b.stump_feature[79] = 6;
        REQUIRE(refused(b));
        b = t, b.stump_feature[0] = -1;
        REQUIRE(refused(b));
        b = t, b.rects[2] += 1;                                          // feature 0 ends at the corner: one more leaves the window
        REQUIRE(refused(b));
        b = t, b.leaves[159] = std::nanf("");
        REQUIRE(refused(b));
        b = t, b.stage_thr[4] = std::nanf("");
        REQUIRE(refused(b));
        if (type == SR_CASCADE_HAAR) {
            b = t, b.info.tilted = 1;
            REQUIRE(refused(b));
            b = t, b.info.max_rects = 4;
            REQUIRE(refused(b));
            b = t, b.nrects[1] = 4;
            REQUIRE(refused(b));
            b = t, b.weights[4] = std::nanf("");
            REQUIRE(refused(b));
            b = t, b.stump_thr[3] = std::nanf("");
            REQUIRE(refused(b));
        } else {
            b = t, b.info.max_cat_count = 0;
            REQUIRE(refused(b));
        }
        b = t, b.stage_count[0] = 3;
        sr_cascade *o = nullptr;
        REQUIRE(b.create(&o) == SR_ERR_INVALID_ARG && !o);
        sr_cascade_params p;
        REQUIRE(sr_cascade_default_params(&p) == SR_OK);
        p.scale_factor = 1.0;
        REQUIRE(sr_cascade_plan(m, 50, 50, &p, nullptr, 0, nullptr, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
        p.scale_factor = std::nan("");
        REQUIRE(sr_cascade_plan(m, 50, 50, &p, nullptr, 0, nullptr, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
        p.scale_factor = 1.001;
        REQUIRE(sr_cascade_plan(m, 500, 500, &p, nullptr, 0, nullptr, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
        p.scale_factor = 1.1, p.min_neighbors = -1;
        REQUIRE(sr_cascade_plan(m, 50, 50, &p, nullptr, 0, nullptr, nullptr, nullptr) == SR_ERR_UNSUPPORTED);
        REQUIRE(sr_cascade_destroy(m) == SR_OK && sr_cascade_destroy(m) == SR_ERR_INVALID_ARG && sr_cascade_destroy(nullptr) == SR_OK);
        REQUIRE(sr_cascade_desc(m, &back) == SR_ERR_INVALID_ARG);
    }
    // neither the pixel cap nor the step cap keeps the pyramid's indices inside an int32 at a factor close to 1: refused by name
    for (int type : {SR_CASCADE_LBP, SR_CASCADE_HAAR}) {
        sr_cascade *wide = nullptr, *tiny = nullptr;
        REQUIRE(make_tables(type, 24, 24, {0}).create(&wide) == SR_OK && make_tables(type, 3, 3, {0}).create(&tiny) == SR_OK);
        sr_cascade_params p;
        REQUIRE(sr_cascade_default_params(&p) == SR_OK);
        p.scale_factor = 1.000165, p.max_w = p.max_h = 24;               // 125 scales of 24 x 699050: 2 162 340 575 table elements
        int ns = -1;
        CcPlan pl;
        REQUIRE(sr_cascade_plan(wide, 24, 699050, &p, nullptr, 0, &ns, nullptr, nullptr) == SR_ERR_UNSUPPORTED && ns == -1);
        REQUIRE(cascade_plan("driver", wide, 24, 699050, &p, &pl) == SR_ERR_UNSUPPORTED && pl.dev.empty());
        p.scale_factor = 1.0002;                                          // 104 scales, 1 798 942 375: the largest offsets in use
        REQUIRE(cascade_plan("driver", wide, 24, 699050, &p, &pl) == SR_OK && pl.dev.size() == 104 && pl.table_el == 1798942375LL);
        REQUIRE(pl.dev.back().tab_off > 0 && pl.dev.back().tab_off + 25LL * (pl.dev.back().sw + 1) == pl.table_el);
        p.scale_factor = 1.0013, p.max_w = p.max_h = 0;                   // 119 scales of 3 x 5592405: 2 468 023 484
        REQUIRE(sr_cascade_plan(tiny, 3, 5592405, &p, nullptr, 0, &ns, nullptr, nullptr) == SR_ERR_UNSUPPORTED && ns == -1);
        REQUIRE(sr_cascade_destroy(wide) == SR_OK && sr_cascade_destroy(tiny) == SR_OK);
    }
    // grouping: empty, one, a chain, exact-size outputs
    int64_t nb = -1;
    REQUIRE(sr_cascade_group(nullptr, 0, 3, nullptr, &nb) == SR_OK && nb == 0);
    std::vector<sr_tile_rect> chain = {{0, 0, 20, 20}, {3, 0, 20, 20}, {6, 0, 20, 20}}, out(3);
    REQUIRE(sr_cascade_group(chain.data(), 3, 2, out.data(), &nb) == SR_OK && nb == 1 && out[0].x == 3 && out[0].w == 20);
    REQUIRE(sr_cascade_group(chain.data(), 3, 3, out.data(), &nb) == SR_OK && nb == 0);
    REQUIRE(sr_cascade_group(chain.data(), 3, -1, out.data(), &nb) == SR_ERR_UNSUPPORTED);
    std::vector<sr_tile_rect> big = {{std::numeric_limits<int>::max() / 4, 5, 1 << 20, 1 << 20}, {std::numeric_limits<int>::max() / 4, 5, 1 << 20, 1 << 20}};
    REQUIRE(sr_cascade_group(big.data(), 2, 1, out.data(), &nb) == SR_OK && nb == 1);
    // a long class far from the origin: the sums pass an int (1100 x 2 000 000), rectangles at the ends of the int range compare
    std::vector<sr_tile_rect> far(1100, sr_tile_rect{2000000, 5, 40, 40}), one(1100);
    REQUIRE(sr_cascade_group(far.data(), 1100, 3, one.data(), &nb) == SR_OK && nb == 1 && one[0].x == 2000000 && one[0].w == 40);
    std::vector<sr_tile_rect> ends = {{std::numeric_limits<int>::min(), 0, 5, 5}, {std::numeric_limits<int>::max() - 5, 0, 5, 5}};
    REQUIRE(sr_cascade_group(ends.data(), 2, 1, out.data(), &nb) == SR_OK && nb == 0);
    printf("cascade-driver-ok\n");
    return 0;
}
