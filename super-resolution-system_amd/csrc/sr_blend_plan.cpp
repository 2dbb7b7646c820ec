// sr_blend_plan.cpp -- the blend planner: a tile list and a canvas row range in, the tables the blend kernels read out
// (sr_blend_tables.h).  Pure host code: no device call, no context, no environment -- sr_engine.hip reads the switches,
// calls sr_build_blend_tables and uploads what it returns; tools/sanitize/host_driver.cpp runs it under the sanitizers.
#include <algorithm>
#include <cstring>
#include <map>
#include <utility>

#include "sr_blend_tables.h"

static int round_up(int v, int m) { return (v + m - 1) / m * m; }

// the tile meets the canvas rectangle [x0, x1) x [y0, y1)
static bool tile_meets(const TileDev &T, long long x0, long long y0, long long x1, long long y1)
{
    return T.x < x1 && (long long)T.x + T.w > x0 && T.y < y1 && (long long)T.y + T.h > y0;
}

// ---- tiles, weight classes, arena layout, final descriptors ----
static int plan_tiles(const sr_tile_rect *h_tiles, int weight_type, const BlendSwitches &sw, BlendTables *P)
{
    const int n = P->n, cn = P->cn;
    P->tiles.resize(n);
    P->tile_rows.resize(n);
    std::map<std::pair<int, int>, int> cls_of;
    std::vector<SrTileLevels> lv(n);
    size_t off = 0;
    for (int t = 0; t < n; ++t) {
        const sr_tile_rect &r = h_tiles[t];
        if (r.w < 1 || r.h < 1 || r.x < 0 || r.y < 0)
            return sr_set_error(SR_ERR_INVALID_ARG, "sr_blend_plan_create: tile %d has bad rectangle (%d,%d,%d,%d)", t, r.x, r.y, r.w, r.h);
        if (std::min(r.w, r.h) < 8 && weight_type != SR_W_ONES)
            return sr_set_error(SR_ERR_INVALID_ARG, "sr_blend_plan_create: tile %d is %dx%d; min side < 8 gives the reference a zero "
                                "feather width (NaN weights)", t, r.w, r.h);
        sr_plan_windows(r.h, r.w, r.y, P->levels, P->row_begin, P->row_end, P->canvas_h, &lv[t]);
        TileDev &T = P->tiles[t];
        memset(&T, 0, sizeof(T));
        T.h = r.h; T.w = r.w; T.x = r.x; T.y = r.y;
        T.nl = lv[t].nl;
        T.fw = std::max(std::min(r.w, r.h) / 8, 1);
        P->max_nl = std::max(P->max_nl, T.nl);
        auto key = std::make_pair(r.h, r.w);
        auto it = cls_of.find(key);
        if (it == cls_of.end()) {
            const int id = (int)P->classes.size();
            cls_of[key] = id;
            TileDev C;
            memset(&C, 0, sizeof(C));
            C.h = r.h; C.w = r.w; C.nl = T.nl; C.fw = T.fw;
            C.lut_off = (int)P->luts.size();
            P->luts.resize(P->luts.size() + T.fw + 1);
            if (const int rc = sr_weight_lut(T.fw, weight_type, P->luts.data() + C.lut_off)) return rc;
            for (int i = 0; i < T.nl; ++i) {
                C.H[i] = lv[t].H[i];
                C.W[i] = lv[t].W[i];
                C.P[i] = round_up(C.W[i], i == 1 ? 64 : 32);
                C.g0[i] = C.g1[i] = 0;
                if (i >= 1) {
                    C.g_off[i] = (long long)off;
                    off += (size_t)C.H[i] * C.P[i];
                }
            }
            P->classes.push_back(C);
            T.cls = id;
        } else {
            T.cls = it->second;
        }
        TileDev &C = P->classes[T.cls];
        T.lut_off = C.lut_off;
        for (int i = 0; i < T.nl; ++i) {
            T.H[i] = lv[t].H[i];
            T.W[i] = lv[t].W[i];
            T.P[i] = round_up(T.W[i], i == 1 ? 64 : 32);       // level 1: rows of 16-bit planes start on 128-byte lines, too
            T.g0[i] = lv[t].gw[i].a; T.g1[i] = lv[t].gw[i].b;
            T.r0[i] = lv[t].rw[i].a; T.r1[i] = lv[t].rw[i].b;
            T.w_off[i] = C.g_off[i];
            if (i >= 1) {
                const bool active = T.g0[i] < T.g1[i];
                if (active) {                                  // weight level i must cover every member tile's G window (hull)
                    const bool first = C.g0[i] >= C.g1[i];
                    C.g0[i] = first ? T.g0[i] : std::min(C.g0[i], T.g0[i]);
                    C.g1[i] = first ? T.g1[i] : std::max(C.g1[i], T.g1[i]);
                }
                T.g_off[i] = (long long)off;
                if (active) off += (size_t)cn * T.H[i] * T.P[i];
                T.r_off[i] = (long long)off;
                if (active && !(P->fused && i == 1)) off += (size_t)cn * T.H[i] * T.P[i];     // fused gather: R_1 lives in LDS only
            }
        }
        P->tile_rows[t] = lv[t].gw[0];
    }
    for (const TileDev &T : P->tiles)
        for (int i = 0; i < T.nl; ++i) {
            P->max_w[i] = std::max(P->max_w[i], T.W[i]);
            P->max_grows[i] = std::max(P->max_grows[i], T.g1[i] - T.g0[i]);
            P->max_rrows[i] = std::max(P->max_rrows[i], T.r1[i] - T.r0[i]);
        }
    for (const TileDev &C : P->classes)
        for (int i = 0; i < C.nl; ++i) {
            P->cmax_w[i] = std::max(P->cmax_w[i], C.W[i]);
            P->cmax_rows[i] = std::max(P->cmax_rows[i], C.g1[i] - C.g0[i]);
        }
    P->arena_floats = off;
    // the plan's part of the G_1 format: the only writer of 16-bit planes is k_down2_march, the readers are the fused gather's
    bool ok = P->down2 && P->fused && cn == 3 && sw.g1_u16 && off * sizeof(float) < 0xFFFF0000ull, any = false;
    for (const TileDev &T : P->tiles) {
        if (T.nl < 2 || T.g0[1] >= T.g1[1]) continue;            // no level 1, or none of its rows in use
        any = true;
        ok = ok && down2_takes(T);
    }
    P->g1_u16 = ok && any;
    P->fdesc.resize(n);
    for (int t = 0; t < n; ++t) {
        const TileDev &T = P->tiles[t];
        FinalDesc &D = P->fdesc[t];
        memset(&D, 0, sizeof(D));
        D.x = T.x; D.y = T.y; D.w = T.w; D.h = T.h;
        D.fw = T.fw; D.lut_off = T.lut_off; D.nl = T.nl;
        D.H1 = T.nl > 1 ? T.H[1] : 1; D.W1 = T.nl > 1 ? T.W[1] : 1; D.P1 = T.nl > 1 ? T.P[1] : 16;
        D.g1 = T.nl > 1 ? T.g_off[1] : 0; D.r1 = T.nl > 1 ? T.r_off[1] : 0;
        D.H2 = T.nl > 2 ? T.H[2] : 1; D.W2 = T.nl > 2 ? T.W[2] : 1; D.P2 = T.nl > 2 ? T.P[2] : 16;
        D.g2 = T.nl > 2 ? T.g_off[2] : 0; D.r2 = T.nl > 2 ? T.r_off[2] : 0;
        D.w1 = T.nl > 1 ? T.w_off[1] : 0;
    }
    return SR_OK;
}

// ---- block tables of the two block gathers (k_final_fast, k_final_fused) ----
// Candidate tiles per regular block of bw x bh pixels of the strip, CSR, tiles in list order (the accumulation order of
// the reference).  The grid is nbx x nby blocks, at least 1 x 1.
static void block_candidates(const std::vector<TileDev> &tiles, int canvas_w, int row_begin, int row_end, int bw, int bh,
                             std::vector<int> &coff, std::vector<int> &cidx)
{
    const int rows = row_end - row_begin;
    const int nbx = std::max((canvas_w + bw - 1) / bw, 1), nby = std::max((rows + bh - 1) / bh, 1);
    const size_t nblk = (size_t)nbx * nby;
    // per tile: the blocks its part of the strip meets (none: bxa > bxb)
    struct Span { int bxa, bxb, bya, byb; };
    std::vector<Span> span(tiles.size(), Span{0, -1, 0, -1});
    for (size_t t = 0; t < tiles.size() && rows > 0; ++t) {
        const TileDev &T = tiles[t];
        const long long x0 = std::max<long long>(T.x, 0), x1 = std::min<long long>((long long)T.x + T.w, canvas_w);
        const long long y0 = std::max<long long>(T.y, row_begin), y1 = std::min<long long>((long long)T.y + T.h, row_end);
        if (x0 >= x1 || y0 >= y1) continue;
        span[t] = Span{(int)(x0 / bw), (int)((x1 - 1) / bw), (int)((y0 - row_begin) / bh), (int)((y1 - 1 - row_begin) / bh)};
    }
    coff.assign(nblk + 1, 0);
    for (const Span &sp : span)
        for (int by = sp.bya; by <= sp.byb; ++by)
            for (int bx = sp.bxa; bx <= sp.bxb; ++bx) ++coff[(size_t)by * nbx + bx + 1];
    for (size_t i = 0; i < nblk; ++i) coff[i + 1] += coff[i];
    cidx.assign((size_t)std::max(coff[nblk], 1), 0);
    std::vector<int> fill(coff.begin(), coff.end() - 1);
    for (size_t t = 0; t < span.size(); ++t)
        for (int by = span[t].bya; by <= span[t].byb; ++by)
            for (int bx = span[t].bxa; bx <= span[t].bxb; ++bx) cidx[(size_t)fill[(size_t)by * nbx + bx]++] = (int)t;
}

// The marks of an edge pass: shape 0 blocks of w[0] x h[0] pixels of the strip along horizontal tile edges, shape 1 blocks of
// w[1] x h[1] along vertical ones.
struct EdgeMarks {
    int w[2], h[2], nbx[2], nby[2];
    std::vector<unsigned char> m[2];
    EdgeMarks(int w0, int h0, int w1, int h1, int canvas_w, int rows) : w{w0, w1}, h{h0, h1}
    {
        for (int s = 0; s < 2; ++s) {
            nbx[s] = (canvas_w + w[s] - 1) / w[s];
            nby[s] = (rows + h[s] - 1) / h[s];
            m[s].assign((size_t)std::max(nbx[s], 1) * std::max(nby[s], 1), 0);
        }
    }
    void mark(int s, long long bx, long long by) { m[s][(size_t)by * nbx[s] + bx] = 1; }
};

// The marked blocks as a work list -- shape 0 first, rows of blocks from the top -- with the candidate tiles of each (every
// tile that meets the block, list order) and the closing sentinel.
static void edge_candidates(const EdgeMarks &E, const std::vector<TileDev> &tiles, int canvas_w, int row_begin, int row_end,
                            std::vector<EdgeBlock> &blocks, std::vector<int> &cand)
{
    for (int s = 0; s < 2; ++s)
        for (int by = 0; by < E.nby[s]; ++by)
            for (int bx = 0; bx < E.nbx[s]; ++bx)
                if (E.m[s][(size_t)by * E.nbx[s] + bx]) blocks.push_back(EdgeBlock{bx * E.w[s], row_begin + by * E.h[s], s, 0});
    for (EdgeBlock &b : blocks) {
        const long long bx1 = std::min<long long>((long long)b.x + E.w[b.shape], canvas_w);
        const long long by1 = std::min<long long>((long long)b.y + E.h[b.shape], row_end);
        b.first = (int)cand.size();
        for (int t = 0; t < (int)tiles.size(); ++t)
            if (tile_meets(tiles[t], b.x, b.y, bx1, by1)) cand.push_back(t);
    }
    blocks.push_back(EdgeBlock{0, 0, 0, (int)cand.size()});       // sentinel: end of the last list
}

// Edge blocks of k_final_fast: the cells (4 x 2 pixel rectangles of one thread) in which a visit can be a border visit lie
// within 8 px of a tile edge line (or on the ragged right / bottom canvas edge).  Horizontal lines are covered by 256 x 8
// blocks of the fast pass's grid (shape 0), vertical lines by 16 x 128 blocks (shape 1: 4 x 64 cells), so a wave of the edge
// pass is mostly border cells either way.  A cell reached through both shapes is computed twice with identical results.
static EdgeMarks mark_edge_bands(const std::vector<TileDev> &tiles, int canvas_w, int row_begin, int row_end)
{
    const int rows = row_end - row_begin;
    EdgeMarks E(256, 8, 16, 128, canvas_w, rows);
    auto mark_rect = [&](int s, long long x0, long long y0, long long x1, long long y1) {   // canvas px, half-open
        x0 = std::max<long long>(x0, 0); x1 = std::min<long long>(x1, canvas_w);
        y0 = std::max<long long>(y0, row_begin); y1 = std::min<long long>(y1, row_end);
        if (x0 >= x1 || y0 >= y1) return;
        for (long long by = (y0 - row_begin) / E.h[s]; by <= (y1 - 1 - row_begin) / E.h[s]; ++by)
            for (long long bx = x0 / E.w[s]; bx <= (x1 - 1) / E.w[s]; ++bx) E.mark(s, bx, by);
    };
    const int M = 8;
    for (size_t t = 0; t < tiles.size() && rows > 0; ++t) {
        const TileDev &T = tiles[t];
        const long long xa = T.x, xb = (long long)T.x + T.w, ya = T.y, yb = (long long)T.y + T.h;
        mark_rect(1, xa - M, ya - M, xa + M, yb + M);
        mark_rect(1, xb - M, ya - M, xb + M, yb + M);
        mark_rect(0, xa - M, ya - M, xb + M, ya + M);
        mark_rect(0, xa - M, yb - M, xb + M, yb + M);
    }
    if (rows > 0) {
        if (canvas_w % 4) mark_rect(1, canvas_w - 4, row_begin, canvas_w, row_end);
        if (rows % 2) mark_rect(0, 0, row_end - 2, canvas_w, row_end);
    }
    return E;
}

// Edge blocks of k_final_fused: every cell with a border visit lies within a few pixels of the edge line of the tile it
// visits (or on the ragged right / bottom end of the strip): walk the cells of a 24-pixel frame around each tile's outline,
// test them exactly, mark the block that holds them -- blocks along horizontal lines in shape 0 (256 x FU_E0H), along
// vertical lines in shape 1 (FU_E1W x FU_E1H; a corner cell may be marked in both: computed twice, identical bytes).
static EdgeMarks mark_edge_cells(const std::vector<TileDev> &tiles, int canvas_w, int row_begin, int row_end)
{
    const int rows = row_end - row_begin;
    EdgeMarks E(256, FU_E0H, FU_E1W, FU_E1H, canvas_w, rows);
    // host mirror of visit_is_interior<true> (device): a 4 x 2 cell at tile-local (lx0, ly0), nx x ny of it on the strip
    auto cell_interior = [](const TileDev &T, long long lx0, long long ly0, int nx, int ny) {
        if (nx != 4 || ny != 2 || lx0 < 0 || ly0 < 0 || lx0 + 3 >= T.w || ly0 + 1 >= T.h) return false;
        if (T.nl > 1) {
            const long long r0 = (ly0 - 1) >> 1, c0 = (lx0 - 1) >> 1;
            return c0 >= 0 && c0 + 3 <= T.W[1] - 1 && r0 >= 0 && r0 + 2 <= T.H[1] - 1;
        }
        return true;
    };
    auto scan = [&](const TileDev &T, long long xa, long long ya, long long xb, long long yb, int s) {   // canvas px, half-open
        xa = std::max<long long>(xa, 0); xb = std::min<long long>(xb, canvas_w);
        ya = std::max<long long>(ya, row_begin); yb = std::min<long long>(yb, row_end);
        if (xa >= xb || ya >= yb) return;
        for (long long cy = (ya - row_begin) / 2; cy <= (yb - 1 - row_begin) / 2; ++cy)
            for (long long cx = xa / 4; cx <= (xb - 1) / 4; ++cx) {
                const long long x0 = cx * 4, y0 = row_begin + cy * 2;
                const int nx = (int)std::min<long long>(4, canvas_w - x0), ny = (int)std::min<long long>(2, row_end - y0);
                const long long lx0 = x0 - T.x, ly0 = y0 - T.y;
                if (lx0 + nx <= 0 || ly0 + ny <= 0 || lx0 >= T.w || ly0 >= T.h) continue;
                if (cell_interior(T, lx0, ly0, nx, ny)) continue;
                if (s == 0) E.mark(0, x0 / 256, (y0 - row_begin) / FU_E0H);
                else E.mark(1, x0 / FU_E1W, (y0 - row_begin) / FU_E1H);
            }
    };
    const long long F = 24;
    for (size_t t = 0; t < tiles.size() && rows > 0; ++t) {
        const TileDev &T = tiles[t];
        const long long xa = T.x, xb = (long long)T.x + T.w, ya = T.y, yb = (long long)T.y + T.h;
        scan(T, xa - F, ya - F, xb + F, ya + F, 0);
        scan(T, xa - F, yb - F, xb + F, yb + F, 0);
        scan(T, xa - F, ya - F, xa + F, yb + F, 1);
        scan(T, xb - F, ya - F, xb + F, yb + F, 1);
        // the ragged ends of the strip (cells narrower / shorter than 4): border visits of every tile they touch
        if (canvas_w % 4) scan(T, canvas_w - (canvas_w % 4), row_begin, canvas_w, row_end, 1);
        if (rows % 2) scan(T, 0, row_end - 1, canvas_w, row_end, 0);
    }
    return E;
}

// ---------------------------------------------------------------------------------------------
// Work lists of the marched gather (k_final_march, sr_march.inc).  A cell column (4 canvas pixels) / cell row (2 canvas
// rows) is, for one tile, 0 = not touched, 1 = marchable (the cell is an interior visit and neither the level-1 columns /
// rows the lane produces nor their level-2 taps meet a border rule), 2 = touched otherwise.  Between two consecutive class
// changes of any tile the classes are constant, so the canvas falls into rectangles with a fixed list of visiting tiles;
// a rectangle is marched when every tile that touches it is marchable in both directions.  Rectangles lose one cell
// column per side to the halo lanes and are cut into strips of <= MARCH_CELLS cells and segments of <= MARCH_SEG steps
// (an even number: an odd last cell row is left to the rectangles).
// cover: [cell row][word of 32 cell columns] bits of the marched cells (row pitch nbx_r words).
// ---------------------------------------------------------------------------------------------
static void plan_march(BlendTables *P, const BlendSwitches &sw, int num_cu, int nbx_r, int nby_r, std::vector<unsigned> &cover)
{
    const int rows = P->row_end - P->row_begin, cw = P->canvas_w, n = P->n;
    const int ncx = cw / 4, ncy = rows / 2;                    // whole cells only: ragged ends are border visits
    const int CPB = FU_BH / 2;                                 // cell rows per regular block
    cover.assign((size_t)nbx_r * nby_r * CPB, 0u);                         // [cell row][block column]: cell column bits (1 = marched)
    // the marched kernels address the arena and a tile's pixels with 32-bit byte offsets (buffer instructions)
    bool fits32 = P->arena_floats * sizeof(float) < MARCH_OFF_LIMIT && (unsigned long long)cw * P->cn * 4ull * MARCH_SPAN_ROWS < MARCH_OFF_LIMIT;
    for (int t = 0; t < n && fits32; ++t) fits32 = (unsigned long long)P->tiles[t].h * P->tiles[t].w * P->cn * 4ull < 0x7FFF0000ull;
    // The march is four launches of long work items: it wins on a big canvas (200 MP: 1.12 against 1.22 ms for the block kernel
    // alone) and loses on a small one, where every launch is a few short items deep -- a rank's strip of a world of 4 / 8:
    // 0.39 / 0.27 ms against 0.33 / 0.18 (tools/virtual_scaling.py, profiles/r04_virtual_scaling.json); even at 100 MP.
    // BlendSwitches::march_force marches whatever the size.
    const bool big = sw.march_force || (double)rows * (double)cw >= 90e6;
    const bool on = P->march && big && fits32 && n <= 128 && ncx >= 3 && ncy >= 2;
    if (!on) return;
    auto xclass = [&](const TileDev &T, int x0) -> unsigned char {
        const long long lx0 = (long long)x0 - T.x;
        if (lx0 + 4 <= 0 || lx0 >= T.w) return 0;
        if (T.nl < 3 || lx0 < 0 || lx0 + 3 >= T.w) return 2;
        const long long c0 = (lx0 - 1) >> 1, n0 = c0 >> 1;
        if (c0 < 0 || c0 + 3 > T.W[1] - 1 || n0 + 2 > T.W[2] - 1) return 2;
        return 1;
    };
    auto yclass = [&](const TileDev &T, int y0) -> unsigned char {
        const long long ly0 = (long long)y0 - T.y;
        if (ly0 + 2 <= 0 || ly0 >= T.h) return 0;
        if (T.nl < 3 || ly0 < 0 || ly0 + 1 >= T.h) return 2;
        const long long r0 = (ly0 - 1) >> 1;
        if (r0 < 1 || r0 + 2 > T.H[1] - 1 || ((r0 + 1) >> 1) + 2 > T.H[2] - 1) return 2;
        return 1;
    };
    std::vector<std::vector<unsigned char>> xc(n, std::vector<unsigned char>(ncx)), yc(n, std::vector<unsigned char>(ncy));
    std::vector<int> xb{0, ncx}, yb{0, ncy};
    for (int t = 0; t < n; ++t) {
        const TileDev &T = P->tiles[t];
        for (int c = 0; c < ncx; ++c) {
            xc[t][c] = xclass(T, 4 * c);
            if (c && xc[t][c] != xc[t][c - 1]) xb.push_back(c);
        }
        for (int c = 0; c < ncy; ++c) {
            yc[t][c] = yclass(T, P->row_begin + 2 * c);
            if (c && yc[t][c] != yc[t][c - 1]) yb.push_back(c);
        }
    }
    std::sort(xb.begin(), xb.end());
    xb.erase(std::unique(xb.begin(), xb.end()), xb.end());
    std::sort(yb.begin(), yb.end());
    yb.erase(std::unique(yb.begin(), yb.end()), yb.end());
    struct Strip { int ca, cb, ya, ye, nt, tile[4]; };
    std::vector<Strip> strips;
    std::vector<int> vis, run_vis;
    for (size_t iy = 0; iy + 1 < yb.size(); ++iy) {
        const int ya = yb[iy], ye = ya + (yb[iy + 1] - ya) / 2 * 2;      // an even number of steps (the loop is unrolled by two)
        if (ye - ya < 2) continue;
        // runs of consecutive x intervals with the same (valid) tile list
        int run_a = -1, run_b = -1;
        auto flush = [&]() {
            if (run_a < 0) return;
            const int ua = run_a + 1, ub = run_b - 1;          // one cell column per side goes to the halo lanes
            const int nu = ub - ua, nt = (int)run_vis.size();
            if (nu >= 1) {
                const int ns = (nu + MARCH_CELLS - 1) / MARCH_CELLS;
                for (int si = 0; si < ns; ++si) {
                    const int ca = ua + (int)((long long)nu * si / ns), cb = ua + (int)((long long)nu * (si + 1) / ns);
                    Strip st;
                    st.ca = ca; st.cb = cb; st.ya = ya; st.ye = ye; st.nt = nt;
                    for (int k = 0; k < 4; ++k) st.tile[k] = k < nt ? run_vis[k] : 0;
                    strips.push_back(st);
                }
                for (int cy = ya; cy < ye; ++cy)
                    for (int c = ua; c < ub; ++c) cover[(size_t)cy * nbx_r + c / 32] |= 1u << (c & 31);
            }
            run_a = -1;
        };
        for (size_t ix = 0; ix + 1 < xb.size(); ++ix) {
            vis.clear();
            bool ok = true;
            for (int t = 0; t < n && ok; ++t) {
                const unsigned char cx = xc[t][xb[ix]], cy = yc[t][yb[iy]];
                if (cx == 0 || cy == 0) continue;
                if (cx == 1 && cy == 1) vis.push_back(t);
                else ok = false;
            }
            ok = ok && !vis.empty() && (int)vis.size() <= MARCH_NT;
            if (ok && run_a >= 0 && vis == run_vis) {
                run_b = xb[ix + 1];
                continue;
            }
            flush();
            if (ok) {
                run_a = xb[ix];
                run_b = xb[ix + 1];
                run_vis = vis;
            }
        }
        flush();
    }
    // Segment length per tile count: as long as MARCH_SEG steps where that still leaves every wave slot of the GPU a few
    // items (the warm-up of an item costs about two steps), shorter where a list is small -- a short list of long items
    // is a latency-bound launch of one or two rounds.
    long long steps_of[MARCH_NT + 1] = {0}, cells_of[MARCH_NT + 1] = {0};
    for (const Strip &st : strips) {
        steps_of[st.nt] += st.ye - st.ya;
        cells_of[st.nt] += (long long)(st.ye - st.ya) * (st.cb - st.ca);
    }
    for (int nt = 1; nt <= MARCH_NT; ++nt) {
        if (!steps_of[nt]) continue;
        // Rounds per list, measured (profiles/r04_e_gather_sweep.txt): four for the 1-tile list, three for the 2-tile list, two
        // for the short 3- / 4-tile lists (an item's warm-up is ~2.5 steps: at six rounds the 4-tile list was cut into 8-step
        // items); the tapered end of a list (below) is what makes long items affordable.
        // BlendSwitches::march_rounds: A/B runs.
        double rounds = nt >= 3 ? MARCH_ROUNDS_N : (nt == 2 ? MARCH_ROUNDS_2 : MARCH_ROUNDS);
        if (sw.march_rounds[std::min(nt, 3) - 1] > 0) rounds = sw.march_rounds[std::min(nt, 3) - 1];
        const long long want_items = std::max<long long>((long long)((double)(num_cu * 8 / nt) * rounds), 1);   // rounds at two waves per SIMD
        int seg = (int)std::min<long long>(MARCH_SEG, std::max<long long>(8, steps_of[nt] / want_items));
        seg = seg / 2 * 2;
        // The items of a list run in list order, a few rounds of them: the last round leaves the GPU emptier and emptier
        // while its long items finish (half an item's duration per launch, ~30 us of march1's 300).  So the list ends
        // with short items: the last `tail` strip-steps (about one round of full-length items) are cut into segments of
        // half the length, the last quarter of those into the shortest ones (8 steps: an item's warm-up is ~2).
        // BlendSwitches::march_taper off: uniform segments (A/B runs).  Which segment a canvas row falls into changes no value.
        const long long slots = std::max<long long>((long long)num_cu * 8 / nt, 1);
        const long long tail = sw.march_taper && seg > 8 ? std::min<long long>(slots * seg, steps_of[nt] / 3) : 0;
        long long done = 0;
        for (const Strip &st : strips) {
            if (st.nt != nt) continue;
            for (int sy = st.ya; sy < st.ye;) {
                const long long left = steps_of[nt] - done;
                int sg = seg;
                if (left <= tail / 4) sg = 8;
                else if (left <= tail) sg = std::max(8, seg / 4 * 2);
                MarchItem it;
                memset(&it, 0, sizeof(it));
                it.x0 = 4 * (st.ca - 1); it.y0 = P->row_begin + 2 * sy;
                it.ncell = st.cb - st.ca; it.nstep = std::min(sg, st.ye - sy);
                for (int k = 0; k < nt; ++k) it.tile[k] = st.tile[k];
                P->march_items[nt].push_back(it);
                sy += it.nstep;
                done += it.nstep;
            }
        }
        if (sw.stats)
            fprintf(stderr, "[march] %d-tile zones: %lld strip-steps, %lld cells (%.2f %% of %d x %d), segments of %d steps, %zu items\n", nt,
                    steps_of[nt], cells_of[nt], 100.0 * (double)cells_of[nt] / ((double)ncx * ncy), ncx, ncy, seg, P->march_items[nt].size());
    }
}

// What the marched zones leave, cut into rectangles of cells for k_final_rect: every cell row's runs of unmarched cells --
// a narrow run (<= 8 cells: a band along a vertical tile edge) whole, a wide one in pieces that end on multiples of 32 cells
// -- stacked downwards while the next row holds the same piece and the rectangle still fits 256 threads and the LDS window.
// cover: plan_march's bitmap (row pitch nbx_r words); ragged cells at the right / bottom end are unmarched cells like any other.
static void plan_rects(BlendTables *P, const BlendSwitches &sw, int nbx_r, const std::vector<unsigned> &cover)
{
    std::vector<int> &rcand = P->rect_cand;
    const int rows = P->row_end - P->row_begin, cw = P->canvas_w;
    const int ncxp = (cw + 3) / 4, ncyp = (rows + 1) / 2;
    const int max_cells = sw.rect_cells;                          // A/B runs: most cells per rectangle (<= 256 threads)
    // window pitch: two pixel pairs more than needed, so that consecutive rows start 36 (not 32) dwords apart for a band 5 cells
    // wide -- column-major lanes read the same columns of consecutive rows
    const int pad = 2;
    auto hmax = [max_cells, pad](int w) {
        int h = std::max(max_cells / w, 1);
        while (h > 1 && rect_rows(h) * (rect_lp(w) + pad) > FU_PLANE) --h;
        return h;
    };
    struct Open { int ya, h; };
    std::map<std::pair<int, int>, Open> open;                     // (first cell column, end) -> rectangle still growing
    auto emit = [&](int xa, int xb, int ya, int h) {
        RectItem it;
        it.x = 4 * xa; it.y = P->row_begin + 2 * ya;
        it.w = xb - xa; it.h = h;
        it.cand = (int)rcand.size();
        const long long bx1 = std::min<long long>(it.x + 4ll * it.w, cw), by1 = std::min<long long>(it.y + 2ll * it.h, P->row_end);
        for (int t = 0; t < P->n; ++t)
            if (tile_meets(P->tiles[t], it.x, it.y, bx1, by1)) rcand.push_back(t);
        it.ncand = (int)rcand.size() - it.cand;
        it.lp = rect_lp(it.w) + pad;
        it.colmajor = it.h > it.w ? 1 : 0;
        P->rects.push_back(it);
    };
    std::vector<std::pair<int, int>> segs;
    std::map<std::pair<int, int>, std::pair<int, int>> wide;      // wide run (first cell, end) -> (piece width, last row seen)
    auto unmarched = [&](int cy, int cx) { return !((cover[(size_t)cy * nbx_r + (cx >> 5)] >> (cx & 31)) & 1u); };
    auto run_is = [&](int cy, int xa, int xe) {                   // row cy holds exactly the run [xa, xe) of unmarched cells
        if (xa > 0 && unmarched(cy, xa - 1)) return false;
        if (xe < ncxp && unmarched(cy, xe)) return false;
        for (int c = xa; c < xe; ++c)
            if (!unmarched(cy, c)) return false;
        return true;
    };
    for (int cy = 0; cy < ncyp; ++cy) {
        segs.clear();
        const unsigned *row = cover.data() + (size_t)cy * nbx_r;
        for (int cx = 0; cx < ncxp;) {
            const unsigned wd = row[cx >> 5];
            if ((cx & 31) == 0 && wd == 0xFFFFFFFFu) { cx += 32; continue; }
            if ((wd >> (cx & 31)) & 1u) { ++cx; continue; }
            int xe = cx;
            while (xe < ncxp && !((row[xe >> 5] >> (xe & 31)) & 1u)) ++xe;
            if (xe - cx <= 8) segs.emplace_back(cx, xe);
            else {
                // a wide run: pieces as wide as the band's height allows (a band 3-4 cell rows high along a horizontal tile
                // edge: 60 cells x 4 rows instead of 32 x 4 -- fewer, fuller items); the width is chosen where the band starts
                // and kept for its rows, so that the pieces of consecutive rows stack
                int pw = 32;
                auto rec = wide.find({cx, xe});
                if (rec != wide.end() && rec->second.second == cy - 1) {
                    pw = rec->second.first;
                    rec->second.second = cy;
                } else {
                    int H = 1;
                    while (H < 9 && cy + H < ncyp && run_is(cy + H, cx, xe)) ++H;
                    if (H <= 8) {
                        pw = std::min(64, 256 / H) / 4 * 4;
                        while (pw > 32 && rect_rows(H) * (rect_lp(pw) + pad) > FU_PLANE) pw -= 4;
                        pw = std::max(pw, 32);
                    }
                    wide[{cx, xe}] = {pw, cy};
                }
                for (int a = cx; a < xe;) {
                    const int b = std::min(xe, (a / pw + 1) * pw);
                    segs.emplace_back(a, b);
                    a = b;
                }
            }
            cx = xe;
        }
        std::map<std::pair<int, int>, Open> next;
        for (const auto &sg : segs) {
            auto f = open.find(sg);
            if (f != open.end() && f->second.h < hmax(sg.second - sg.first)) {
                next[sg] = Open{f->second.ya, f->second.h + 1};
                open.erase(f);
            } else {
                next[sg] = Open{cy, 1};                               // (a full one stays in `open` and is closed below)
            }
        }
        for (const auto &o : open) emit(o.first.first, o.first.second, o.second.ya, o.second.h);
        open.swap(next);
    }
    for (const auto &o : open) emit(o.first.first, o.first.second, o.second.ya, o.second.h);
    if (sw.stats) {
        long long cells = 0;
        for (const RectItem &r : P->rects) cells += (long long)r.w * r.h;
        fprintf(stderr, "[march] rectangles of the remainder: %zu items, %lld cells (%.1f per item), %zu candidate visits\n", P->rects.size(), cells,
                P->rects.empty() ? 0.0 : (double)cells / (double)P->rects.size(), rcand.size());
    }
}

int sr_build_blend_tables(const sr_tile_rect *h_tiles, int n, int cn, int canvas_h, int canvas_w, int levels, int weight_type,
                          int row_begin, int row_end, int num_cu, const BlendSwitches &sw, BlendTables *P)
{
    if (!h_tiles || n < 1 || n > 65535) return sr_set_error(SR_ERR_INVALID_ARG, "sr_blend_plan_create: need 1..65535 tiles");
    if (cn < 1 || cn > 4) return sr_set_error(SR_ERR_INVALID_ARG, "sr_blend_plan_create: channels must be 1..4");
    if (canvas_h < 1 || canvas_w < 1) return sr_set_error(SR_ERR_SHAPE, "sr_blend_plan_create: empty canvas");
    if (levels < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_blend_plan_create: levels must be >= 1");
    if (weight_type < 0 || weight_type > SR_W_ONES) return sr_set_error(SR_ERR_INVALID_ARG, "sr_blend_plan_create: bad weight type");
    *P = BlendTables();
    P->n = n; P->cn = cn; P->canvas_h = canvas_h; P->canvas_w = canvas_w;
    P->levels = std::min(levels, SR_MAX_LEVELS); P->wtype = weight_type;
    P->row_begin = row_begin; P->row_end = row_end;
    P->fused = cn == 3 || cn == 1;
    P->march = P->fused && sw.march;                  // off: every zone through k_final_fused (A/B runs)
    P->down2 = sw.down2;
    if (const int rc = plan_tiles(h_tiles, weight_type, sw, P)) return rc;

    // k_final_fast (the weighted average)
    edge_candidates(mark_edge_bands(P->tiles, canvas_w, row_begin, row_end), P->tiles, canvas_w, row_begin, row_end, P->edge_blocks, P->edge_cand);
    P->n_edge_blocks = (int)P->edge_blocks.size() - 1;
    block_candidates(P->tiles, canvas_w, row_begin, row_end, FIN_BW, FIN_BH, P->cand_off, P->cand_idx);
    if (!P->fused) return SR_OK;
    // k_final_fused
    edge_candidates(mark_edge_cells(P->tiles, canvas_w, row_begin, row_end), P->tiles, canvas_w, row_begin, row_end, P->fedge_blocks, P->fedge_cand);
    P->n_fedge_blocks = (int)P->fedge_blocks.size() - 1;
    block_candidates(P->tiles, canvas_w, row_begin, row_end, FU_BW, FU_BH, P->fcand_off, P->fcand_idx);
    // marched zones and the rectangles of what they leave
    const int rows = row_end - row_begin;
    const int nbx_r = std::max((canvas_w + FU_BW - 1) / FU_BW, 1), nby_r = std::max((rows + FU_BH - 1) / FU_BH, 1);
    std::vector<unsigned> cover;
    plan_march(P, sw, num_cu, nbx_r, nby_r, cover);
    for (int k = 1; k <= MARCH_NT; ++k) {
        P->n_march_items[k] = (int)P->march_items[k].size();
        P->n_march_total += (long long)P->march_items[k].size();
    }
    if (P->n_march_total > 0) {
        plan_rects(P, sw, nbx_r, cover);
        P->n_rects = (long long)P->rects.size();
    }
    return SR_OK;
}
