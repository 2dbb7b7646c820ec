// Host-side sanitizer driver ("-fsanitize=address host build of the C ABI"): every host-only entry point of
// libsrhip (csrc/sr_host.cpp, csrc/sr_encode.cpp) is called over a spread of geometries with EXACT-size output buffers, built
// with -fsanitize=address,undefined -fno-sanitize-recover=all, so an overrun, a signed overflow or a misaligned access ends
// the run; the blend planner (csrc/sr_blend_plan.cpp) is called directly and its tables are held to what they promise.
// Built and run by tests/test_sanitizers.py (CPU); GPU sanitizers are not available on the pool.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sr_blend_tables.h"
#include "sr_hip.h"

static const int MAX_LEVELS = 16;     // SR_MAX_LEVELS of csrc/sr_internal.h

static uint32_t rng_state = 20260313u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static int rint_(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "CHECK failed line %d: %s (%s)\n", __LINE__, #cond, sr_last_error()); std::exit(1); } \
    } while (0)

// ---- blend planner -----------------------------------------------------------------------------------------------------
// the tiles that meet the canvas rectangle [x0, x0 + w) x [y0, y0 + h), cut at the strip's right / bottom end: ascending
static std::vector<int> tiles_meeting(const std::vector<sr_tile_rect> &r, long long x0, long long y0, long long w, long long h, int cw, int row_end)
{
    const long long x1 = std::min<long long>(x0 + w, cw), y1 = std::min<long long>(y0 + h, row_end);
    std::vector<int> out;
    for (size_t t = 0; t < r.size() && x0 < x1 && y0 < y1; ++t)
        if (r[t].x < x1 && (long long)r[t].x + r[t].w > x0 && r[t].y < y1 && (long long)r[t].y + r[t].h > y0) out.push_back((int)t);
    return out;
}

static void check_csr(const std::vector<sr_tile_rect> &r, const std::vector<int> &off, const std::vector<int> &idx, int bw, int bh, int cw, int rb, int re)
{
    const int nbx = std::max((cw + bw - 1) / bw, 1), nby = std::max((re - rb + bh - 1) / bh, 1);
    CHECK(off.size() == (size_t)nbx * nby + 1 && off[0] == 0 && (size_t)off.back() <= idx.size());
    for (int by = 0; by < nby; ++by)
        for (int bx = 0; bx < nbx; ++bx) {
            const size_t b = (size_t)by * nbx + bx;
            CHECK(off[b] <= off[b + 1]);
            CHECK(std::vector<int>(idx.begin() + off[b], idx.begin() + off[b + 1]) == tiles_meeting(r, (long long)bx * bw, rb + (long long)by * bh, bw, bh, cw, re));
        }
}

static void check_edges(const std::vector<sr_tile_rect> &r, const std::vector<EdgeBlock> &eb, const std::vector<int> &cand, int n_blocks, int w0, int h0,
                        int w1, int h1, int cw, int rb, int re)
{
    CHECK(eb.size() == (size_t)n_blocks + 1 && (size_t)eb.back().first == cand.size());
    for (int b = 0; b < n_blocks; ++b) {
        const EdgeBlock &e = eb[(size_t)b];
        CHECK((e.shape == 0 || e.shape == 1) && e.x >= 0 && e.x < cw && e.y >= rb && e.y < re && e.first <= eb[(size_t)b + 1].first);
        CHECK(std::vector<int>(cand.begin() + e.first, cand.begin() + eb[(size_t)b + 1].first) ==
              tiles_meeting(r, e.x, e.y, e.shape ? w1 : w0, e.shape ? h1 : h0, cw, re));
    }
}

static void check_blend_tables(const std::vector<sr_tile_rect> &r, int cn, int ch, int cw, int levels, int wt, int rb, int re, int num_cu,
                               const BlendSwitches &sw)
{
    BlendTables T;
    CHECK(sr_build_blend_tables(r.data(), (int)r.size(), cn, ch, cw, levels, wt, rb, re, num_cu, sw, &T) == SR_OK);
    const int n = (int)r.size(), rows = re - rb;
    CHECK((int)T.tiles.size() == n && (int)T.fdesc.size() == n && (int)T.tile_rows.size() == n && T.fused == (cn == 1 || cn == 3));
    // pitches: whole 128-byte lines, level 1 also as 16-bit planes; arena ranges of the active levels disjoint and inside the arena
    std::vector<std::pair<long long, long long>> ranges;
    for (const TileDev &C : T.classes)
        for (int i = 1; i < C.nl; ++i) ranges.push_back({C.g_off[i], C.g_off[i] + (long long)C.H[i] * C.P[i]});
    bool any_l1 = false;
    for (const TileDev &D : T.tiles) {
        CHECK(D.nl >= 1 && D.nl <= MAX_LEVELS && D.cls >= 0 && D.cls < (int)T.classes.size());
        for (int i = 0; i < D.nl; ++i) CHECK(D.P[i] % 32 == 0 && D.P[i] >= D.W[i] && (i != 1 || D.P[i] % 64 == 0) && T.classes[(size_t)D.cls].P[i] == D.P[i]);
        for (int i = 1; i < D.nl; ++i) {
            if (D.g0[i] >= D.g1[i]) continue;
            const long long sz = (long long)cn * D.H[i] * D.P[i];
            ranges.push_back({D.g_off[i], D.g_off[i] + sz});
            if (!(T.fused && i == 1)) ranges.push_back({D.r_off[i], D.r_off[i] + sz});
        }
        if (D.nl >= 2 && D.g0[1] < D.g1[1]) {
            any_l1 = true;
            if (T.g1_u16) CHECK(down2_takes(D));
        }
    }
    CHECK(!T.g1_u16 || (any_l1 && cn == 3 && sw.g1_u16 && sw.down2));
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 0; i < ranges.size(); ++i) {
        CHECK(ranges[i].first >= 0 && ranges[i].first < ranges[i].second && (size_t)ranges[i].second <= T.arena_floats);
        if (i) CHECK(ranges[i - 1].second <= ranges[i].first);
    }
    // candidate lists: every one the brute-force list of the tiles that meet the block, ascending
    check_csr(r, T.cand_off, T.cand_idx, FIN_BW, FIN_BH, cw, rb, re);
    check_edges(r, T.edge_blocks, T.edge_cand, T.n_edge_blocks, 256, 8, 16, 128, cw, rb, re);
    long long marched = 0;
    for (int nt = 1; nt <= MARCH_NT; ++nt) marched += (long long)T.march_items[nt].size();
    CHECK(marched == T.n_march_total && (T.fused || (marched == 0 && T.fcand_off.empty() && T.fedge_blocks.empty())));
    if (!T.fused) return;
    check_csr(r, T.fcand_off, T.fcand_idx, FU_BW, FU_BH, cw, rb, re);
    check_edges(r, T.fedge_blocks, T.fedge_cand, T.n_fedge_blocks, 256, FU_E0H, FU_E1W, FU_E1H, cw, rb, re);
    CHECK((marched > 0 || T.rects.empty()) && (long long)T.rects.size() == T.n_rects && (marched == 0 || (sw.march && rows >= 4)));
    if (marched == 0) return;
    // a march exists: every cell of the strip (4 x 2 pixels, the ragged ones included) lies in exactly one item or rectangle
    const int ncx = (cw + 3) / 4, ncy = (rows + 1) / 2;
    std::vector<unsigned char> cnt((size_t)ncx * ncy, 0);
    auto cover = [&](long long cx, long long cy, long long w, long long h) {
        CHECK(cx >= 0 && cy >= 0 && w >= 1 && h >= 1 && cx + w <= ncx && cy + h <= ncy);
        for (long long y = cy; y < cy + h; ++y)
            for (long long x = cx; x < cx + w; ++x) CHECK(++cnt[(size_t)(y * ncx + x)] == 1);
    };
    for (int nt = 1; nt <= MARCH_NT; ++nt) {
        CHECK(T.n_march_items[nt] == (int)T.march_items[nt].size());
        for (const MarchItem &it : T.march_items[nt]) {
            CHECK(it.ncell >= 1 && it.ncell <= MARCH_CELLS && it.nstep >= 2 && it.nstep <= MARCH_SEG && it.nstep % 2 == 0);
            CHECK(it.x0 >= 0 && it.x0 % 4 == 0 && (it.y0 - rb) % 2 == 0 && it.y0 + 2 * it.nstep <= re && it.x0 + 4 * (it.ncell + 2) <= cw);
            cover(it.x0 / 4 + 1, (it.y0 - rb) / 2, it.ncell, it.nstep);
            for (int k = 0; k < 4; ++k) CHECK(it.tile[k] >= 0 && it.tile[k] < n && (k == 0 || k >= nt || it.tile[k] > it.tile[k - 1]) && (k < nt || it.tile[k] == 0));
        }
    }
    for (const RectItem &it : T.rects) {
        CHECK(it.x % 4 == 0 && (it.y - rb) % 2 == 0 && it.w * it.h <= 256 && it.cand >= 0 && it.ncand >= 0 && (size_t)(it.cand + it.ncand) <= T.rect_cand.size());
        CHECK(it.lp >= rect_lp(it.w) && rect_rows(it.h) * it.lp <= FU_PLANE);
        cover(it.x / 4, (it.y - rb) / 2, it.w, it.h);
        CHECK(std::vector<int>(T.rect_cand.begin() + it.cand, T.rect_cand.begin() + it.cand + it.ncand) == tiles_meeting(r, it.x, it.y, 4ll * it.w, 2ll * it.h, cw, re));
    }
    for (unsigned char c : cnt) CHECK(c == 1);
}

static int blend_planner_section()
{
    int calls = 0;
    BlendSwitches forced, plain;
    forced.march_force = true;
    // the arrangements of the march-variant tests (tests/_march_geoms.py), restated as numbers: 2 x 2 grids of 424 x 400 tiles
    // with 96 px of overlap and T-junctions of two 160 x 136 tiles above one wide tile with 48 px, shifted by (dx, dy), the
    // second column / row by a further (ex, ey)
    const int grids[][4] = {{0, 0, 1, 3}, {2, 0, 1, 3}, {0, 1, 1, 1}, {2, 1, 1, 1}, {0, 0, 1, 2}, {2, 0, 1, 2}, {1, 2, 2, 0}, {3, 3, 0, 1}};
    const int tjs[][4] = {{0, 0, 1, 1}, {1, 0, 1, 3}, {2, 0, 1, 1}, {3, 0, 1, 3}, {0, 1, 1, 1}, {2, 1, 1, 1}};
    for (int fam = 0; fam < 2; ++fam)
        for (int g = 0; g < (fam ? 6 : 8); ++g) {
            const int *s = fam ? tjs[g] : grids[g];
            const int tw = fam ? 160 : 424, th = fam ? 136 : 400, ov = fam ? 48 : 96, dx = s[0], dy = s[1], sx = tw - ov + s[2], sy = th - ov + s[3];
            std::vector<sr_tile_rect> r = {{dx, dy, tw, th}, {dx + sx, dy, tw, th}};
            if (fam) r.push_back({dx, dy + sy, sx + tw, th});
            else { r.push_back({dx, dy + sy, tw, th}); r.push_back({dx + sx, dy + sy, tw, th}); }
            const int H = dy + sy + th, W = dx + sx + tw;
            for (int cn : {3, 1}) {
                BlendSwitches sw = forced;
                sw.g1_u16 = cn == 3 && (g & 1);
                if (g % 3 == 0) sw.march_rounds[0] = sw.march_rounds[1] = sw.march_rounds[2] = 0.0001;      // the long-item form
                sw.march_taper = g % 4 != 3;
                check_blend_tables(r, cn, H, W, 6, g % 3, 0, H, 256, sw);
                check_blend_tables(r, cn, H, W, 6, g % 3, th / 3 + g, H - th / 2 - 1, 304, sw);              // a strip with an odd end
                calls += 2;
            }
        }
    // seeded small cases
    for (int it = 0; it < 400; ++it) {
        const int n = rint_(1, 6), cn = rint_(1, 4), levels = rint_(1, 6), wt = rint_(0, SR_W_ONES);
        std::vector<sr_tile_rect> r;
        int H = 1, W = 1;
        for (int t = 0; t < n; ++t) {
            sr_tile_rect q;
            q.w = rint_(8, 300); q.h = rint_(8, 300);
            // most tiles hang on an earlier one (overlaps and shared edge lines), some lie anywhere
            if (t && it % 4) {
                const sr_tile_rect &p = r[(size_t)rint_(0, t - 1)];
                q.x = std::max(0, std::min(700 - q.w, p.x + (rint_(0, 1) ? p.w - rint_(0, 64) : rint_(-3, 3))));
                q.y = std::max(0, std::min(700 - q.h, p.y + (rint_(0, 1) ? p.h - rint_(0, 64) : rint_(-3, 3))));
            } else {
                q.x = rint_(0, 700 - q.w); q.y = rint_(0, 700 - q.h);
            }
            r.push_back(q);
            H = std::max(H, q.y + q.h); W = std::max(W, q.x + q.w);
        }
        if (it % 5 == 0) { H = std::min(700, H + rint_(0, 9)); W = std::min(700, W + rint_(0, 9)); }
        int rb = 0, re = H;                                                   // whole, odd-ended, an interior strip, empty
        switch (it % 4) {
        case 1: re = std::max(1, H - 1 - 2 * rint_(0, H / 4)); break;
        case 2: rb = rint_(0, H - 1); re = rint_(rb, H); break;
        case 3: if (it % 8 == 3) { rb = re = rint_(0, H); } break;
        }
        BlendSwitches sw = (it & 1) ? forced : plain;
        sw.march = it % 16 != 15;
        sw.g1_u16 = it % 3 != 0;
        sw.down2 = it % 7 != 0;
        sw.march_taper = it % 6 != 0;
        if (it % 9 == 0) sw.rect_cells = rint_(32, 256);
        if (it % 10 == 0) sw.march_rounds[rint_(0, 2)] = 0.5 * rint_(1, 12);
        check_blend_tables(r, cn, H, W, levels, wt, rb, re, (it & 2) ? 256 : 1, sw);
        ++calls;
    }
    // the refusals keep their codes
    {
        BlendTables T;
        const sr_tile_rect ok = {0, 0, 64, 64}, thin = {0, 0, 64, 4}, neg = {-1, 0, 64, 64};
        CHECK(sr_build_blend_tables(nullptr, 1, 3, 64, 64, 6, 1, 0, 64, 256, plain, &T) == SR_ERR_INVALID_ARG);
        CHECK(sr_build_blend_tables(&ok, 0, 3, 64, 64, 6, 1, 0, 64, 256, plain, &T) == SR_ERR_INVALID_ARG);
        CHECK(sr_build_blend_tables(&ok, 1, 5, 64, 64, 6, 1, 0, 64, 256, plain, &T) == SR_ERR_INVALID_ARG);
        CHECK(sr_build_blend_tables(&ok, 1, 3, 0, 64, 6, 1, 0, 0, 256, plain, &T) == SR_ERR_SHAPE);
        CHECK(sr_build_blend_tables(&ok, 1, 3, 64, 64, 0, 1, 0, 64, 256, plain, &T) == SR_ERR_INVALID_ARG);
        CHECK(sr_build_blend_tables(&ok, 1, 3, 64, 64, 6, SR_W_ONES + 1, 0, 64, 256, plain, &T) == SR_ERR_INVALID_ARG);
        CHECK(sr_build_blend_tables(&thin, 1, 3, 64, 64, 6, 1, 0, 64, 256, plain, &T) == SR_ERR_INVALID_ARG);
        CHECK(sr_build_blend_tables(&thin, 1, 3, 64, 64, 6, SR_W_ONES, 0, 64, 256, plain, &T) == SR_OK);
        CHECK(sr_build_blend_tables(&neg, 1, 3, 64, 64, 6, 1, 0, 64, 256, plain, &T) == SR_ERR_INVALID_ARG);
        calls += 9;
    }
    return calls;
}

int main(int argc, char **argv)
{
    const std::string tmp = argc > 1 ? argv[1] : "/tmp";
    int calls = 0;
    // ---- bookkeeping ---------------------------------------------------------------------------------------------
    for (int it = 0; it < 300; ++it) {
        const int W = rint_(1, 9000), H = rint_(1, 9000), block = rint_(2, 4096), ov = rint_(0, block - 1);
        int n = 0;
        int rc = sr_tile_plan(W, H, block, ov, &n, nullptr, 0);
        CHECK(rc == SR_OK || rc == SR_ERR_SHAPE);
        CHECK(n >= 1);
        std::vector<int> xywh((size_t)n * 4);
        CHECK(sr_tile_plan(W, H, block, ov, &n, xywh.data(), n) == SR_OK);
        if (n > 1) { int m = 0; CHECK(sr_tile_plan(W, H, block, ov, &m, xywh.data(), n - 1) == SR_ERR_SHAPE && m == n); }
        for (int t = 0; t < n; t += (n > 64 ? n / 32 : 1)) {
            int tblr[4];
            CHECK(sr_tile_overlaps(xywh[4 * t], xywh[4 * t + 1], xywh[4 * t + 2], xywh[4 * t + 3], W, H, block, ov, tblr) == SR_OK);
        }
        if (n <= 4096) {
            std::vector<int> nbr((size_t)n * 4);
            CHECK(sr_tile_neighbors(xywh.data(), n, block, ov, nbr.data()) == SR_OK);
            for (int v : nbr) CHECK(v >= -1 && v < n);
        }
        calls += 3;
    }
    for (int mp : {100, 150, 200})
        for (int it = 0; it < 50; ++it) { int ow, oh; CHECK(sr_target_size(rint_(1, 8000), rint_(1, 8000), mp, &ow, &oh) == SR_OK && ow > 0 && oh > 0); }
    { int ow, oh; CHECK(sr_target_size(100, 100, 123, &ow, &oh) != SR_OK); CHECK(sr_target_size(0, 5, 100, &ow, &oh) != SR_OK); }
    for (int wt = 0; wt <= 3; ++wt)
        for (int fw : {1, 2, 7, 371, 4096}) { std::vector<float> lut((size_t)fw + 1); CHECK(sr_weight_lut(fw, wt, lut.data()) == SR_OK); }
    CHECK(sr_psnr_from_sse(0, 10, 255.0) > 1e300);           // MSE 0 -> inf (skimage)
    CHECK(sr_psnr_from_sse(650250, 10, 255.0) == 0.0);
    // ---- strip planner -------------------------------------------------------------------------------------------
    for (int it = 0; it < 120; ++it) {
        const int rows = rint_(1, 6), cols = rint_(1, 6), tw = rint_(16, 900), th = rint_(16, 900);
        const int ovx = rint_(0, tw / 2), ovy = rint_(0, th / 2), levels = rint_(1, MAX_LEVELS), cn = (it & 1) ? 3 : 1;
        std::vector<sr_tile_rect> rects;
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) rects.push_back({c * (tw - ovx), r * (th - ovy), tw, th});
        const int n = (int)rects.size();
        const int CW = (cols - 1) * (tw - ovx) + tw, CH = (rows - 1) * (th - ovy) + th - (it % 5 == 0 ? rint_(0, th / 3) : 0);
        for (int world : {1, 2, 3, 8}) {
            std::vector<int> bounds((size_t)world + 1), rws((size_t)2 * world), need((size_t)2 * world * n), owner((size_t)n);
            CHECK(sr_strip_bounds(rects.data(), n, levels, CH, CW, world, bounds.data()) == SR_OK);
            CHECK(bounds[0] == 0 && bounds[(size_t)world] == CH);
            for (int pol = 0; pol <= 2; ++pol) {
                CHECK(sr_exchange_plan(rects.data(), n, cn, levels, CH, CW, world, 5, pol, bounds.data(), rws.data(), need.data(), owner.data()) == SR_OK);
                for (int o : owner) CHECK(o >= 0 && o < world);
            }
            std::vector<int> rr((size_t)2 * n);
            CHECK(sr_strip_tile_rows(rects.data(), n, levels, CH, rws[0], rws[1], rr.data()) == SR_OK);
            for (int rank = 0; rank < world; ++rank) {
                std::vector<const void *> owned((size_t)n, nullptr);
                std::vector<void *> recv((size_t)n, nullptr);
                std::vector<int64_t> stride((size_t)n);
                for (int t = 0; t < n; ++t) {
                    stride[(size_t)t] = (int64_t)rects[(size_t)t].w * cn;
                    if (owner[(size_t)t] == rank) owned[(size_t)t] = (const void *)(uintptr_t)(0x10000000u + 0x100000u * (unsigned)t);
                    else recv[(size_t)t] = (void *)(uintptr_t)(0x70000000u + 0x100000u * (unsigned)t);
                }
                std::vector<sr_xfer> sends((size_t)n * world), recvs((size_t)n);
                int ns = 0, nr = 0;
                CHECK(sr_exchange_xfers(rects.data(), n, cn, world, rank, need.data(), owner.data(), owned.data(), stride.data(), recv.data(),
                                        sends.data(), n * world, &ns, recvs.data(), n, &nr) == SR_OK);
                if (ns > 0) { int a = 0, b = 0; CHECK(sr_exchange_xfers(rects.data(), n, cn, world, rank, need.data(), owner.data(), owned.data(), stride.data(),
                                                                      recv.data(), sends.data(), ns - 1, &a, recvs.data(), n, &b) == SR_ERR_SHAPE && a == ns); }
            }
            calls += 6;
        }
    }
    for (int l = 1; l <= MAX_LEVELS; ++l) { int b, a; CHECK(sr_pyramid_halo(l, &b, &a) == SR_OK && b >= 0 && a >= 0); }
    // ---- self-ensemble planner -------------------------------------------------------------------------------------
    for (int it = 0; it < 400; ++it) {
        const int h = rint_(-1, 5000), w = rint_(-1, 5000), scale = rint_(0, 5), mask = rint_(-2, 258);
        int n = -1;
        size_t ws = 0;
        const int rc = sr_ens_plan(h, w, scale, mask, &n, &ws);
        const bool good = h >= 1 && w >= 1 && scale >= 1 && mask >= 1 && mask <= 255;
        CHECK((rc == SR_OK) == good);
        if (good) CHECK(n == __builtin_popcount((unsigned)mask) && ws >= (size_t)2 * h * scale * w * scale * 12);
        CHECK(sr_ens_plan(h, w, scale, mask, nullptr, nullptr) == rc);
        ++calls;
    }
    {   // the sizes where the arithmetic is widest: the largest outputs that fit int, and the first that do not
        size_t ws = 0;
        CHECK(sr_ens_plan(536870911, 1, 4, 0x0F, nullptr, &ws) == SR_OK && ws > ((size_t)1 << 34));
        CHECK(sr_ens_plan(536870911, 1, 4, 0x1F, nullptr, &ws) == SR_ERR_SHAPE);
        CHECK(sr_ens_plan(1, 178956970, 4, 0xFF, nullptr, &ws) == SR_OK);
        CHECK(sr_ens_plan(1, 178956971, 4, 0x01, nullptr, &ws) == SR_ERR_SHAPE);
        CHECK(sr_ens_plan(2147483647, 2147483647, 1, 0xFF, nullptr, &ws) == SR_ERR_SHAPE);
        CHECK(sr_ens_plan(715827882, 715827882, 1, 0xFF, nullptr, &ws) == SR_OK);
    }
    calls += blend_planner_section();
    // ---- encoders --------------------------------------------------------------------------------------------------
    const int sizes[][2] = {{1, 1}, {1, 17}, {17, 1}, {7, 9}, {16, 16}, {33, 65}, {257, 131}, {600, 811}};
    for (auto &sz : sizes)
        for (int cn : {1, 3, 4}) {
            const int h = sz[0], w = sz[1];
            const int64_t stride = (int64_t)w * cn + (h % 3);          // padded rows too
            std::vector<uint8_t> img((size_t)(stride * h));
            for (size_t i = 0; i < img.size(); ++i) img[i] = (uint8_t)((i % 7 == 0) ? rnd() : (i / 5));
            const std::string base = tmp + "/san_" + std::to_string(h) + "x" + std::to_string(w) + "_" + std::to_string(cn);
            for (int threads : {1, 3}) {
                CHECK(sr_encode_tiff_lzw(img.data(), h, w, cn, stride, (base + ".tif").c_str(), threads) == SR_OK);
                CHECK(sr_encode_png(img.data(), h, w, cn, stride, 3, (base + ".png").c_str(), threads) == SR_OK);
                if (cn != 4) CHECK(sr_encode_jpeg(img.data(), h, w, cn, stride, 95, (base + ".jpg").c_str(), threads) == SR_OK);
                calls += 3;
            }
            std::remove((base + ".tif").c_str()); std::remove((base + ".png").c_str()); std::remove((base + ".jpg").c_str());
        }
    // LZW worst cases: constant data (longest matches) and noise (table clears), big enough for several clears per strip
    for (int mode = 0; mode < 2; ++mode) {
        const int h = 64, w = 4096;
        std::vector<uint8_t> img((size_t)h * w * 3);
        for (auto &v : img) v = mode ? (uint8_t)rnd() : (uint8_t)77;
        const std::string p = tmp + "/san_lzw.tif";
        CHECK(sr_encode_tiff_lzw(img.data(), h, w, 3, (int64_t)w * 3, p.c_str(), 2) == SR_OK);
        std::remove(p.c_str());
    }
    CHECK(sr_encode_png(nullptr, 4, 4, 3, 12, 3, (tmp + "/x.png").c_str(), 1) != SR_OK);
    CHECK(sr_encode_jpeg(nullptr, 4, 4, 3, 12, 95, (tmp + "/x.jpg").c_str(), 1) != SR_OK);
    std::printf("sanitizer-driver-ok %d\n", calls);
    return 0;
}
