// sr_vgg_ranges.h -- the host-only half of what the tile-streamed feature-stack metrics (sr_lpips.hip, sr_dists.hip) share: the
// layer tables of the three backbones, the per-activation geometry, the per-tile range algebra and the plan of one tile (ranges,
// pitches, buffer size).  No HIP: a host unit or a stand-alone program can include it.  Whether a tiled forward equals the untiled
// one rests on this file alone; tests/test_lpips_plan_host.py holds it against a brute-force restatement through
// sr_lpips_tile_plan.  Internal: nothing here is part of the C ABI.  Everything sits in an unnamed namespace.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace {

// LP_L2POOL is DISTS's padded pooling (k 3, s 2, p 1); LP_POOL the unpadded max pooling of the LPIPS backbones.
enum { LP_CONV = 0, LP_POOL = 1, LP_TAP = 2, LP_L2POOL = 3 };

struct LpLayer {
    int kind;
    int cout, cin, k, s, p;   // conv / pool geometry
    int tap;                  // LP_TAP: tap index
    int widx;                 // LP_CONV: index into the weight arrays
};

// The LPIPS backbones.  alex: torchvision AlexNet.features (lpips/pretrained_networks.py alexnet); otherwise torchvision
// VGG16.features, taps relu1_2 .. relu5_3.
inline void lp_arch(bool alex, std::vector<LpLayer> &L)
{
    auto conv = [&](int cout, int cin, int k, int s, int p) {
        int widx = 0;
        for (auto &l : L) widx += l.kind == LP_CONV;
        L.push_back({LP_CONV, cout, cin, k, s, p, -1, widx});
    };
    auto pool = [&](int k, int s) { L.push_back({LP_POOL, 0, 0, k, s, 0, -1, -1}); };
    auto tap = [&](int i) { L.push_back({LP_TAP, 0, 0, 1, 1, 0, i, -1}); };
    if (alex) {
        conv(64, 3, 11, 4, 2); tap(0);
        pool(3, 2); conv(192, 64, 5, 1, 2); tap(1);
        pool(3, 2); conv(384, 192, 3, 1, 1); tap(2);
        conv(256, 384, 3, 1, 1); tap(3);
        conv(256, 256, 3, 1, 1); tap(4);
    } else {
        conv(64, 3, 3, 1, 1); conv(64, 64, 3, 1, 1); tap(0);
        pool(2, 2); conv(128, 64, 3, 1, 1); conv(128, 128, 3, 1, 1); tap(1);
        pool(2, 2); conv(256, 128, 3, 1, 1); conv(256, 256, 3, 1, 1); conv(256, 256, 3, 1, 1); tap(2);
        pool(2, 2); conv(512, 256, 3, 1, 1); conv(512, 512, 3, 1, 1); conv(512, 512, 3, 1, 1); tap(3);
        pool(2, 2); conv(512, 512, 3, 1, 1); conv(512, 512, 3, 1, 1); conv(512, 512, 3, 1, 1); tap(4);
    }
}

// DISTS: VGG16's thirteen convolutions, an L2 pooling in place of every max pooling, the image itself as stage 0.
inline void ds_arch(std::vector<LpLayer> &L)
{
    auto conv = [&](int cout, int cin) {
        int widx = 0;
        for (auto &l : L) widx += l.kind == LP_CONV;
        L.push_back({LP_CONV, cout, cin, 3, 1, 1, -1, widx});
    };
    auto pool = [&]() { L.push_back({LP_L2POOL, 0, 0, 3, 2, 1, -1, -1}); };
    auto tap = [&](int i) { L.push_back({LP_TAP, 0, 0, 1, 1, 0, i, -1}); };
    tap(0);                                               // stage 0: the image itself
    conv(64, 3); conv(64, 64); tap(1);
    pool(); conv(128, 64); conv(128, 128); tap(2);
    pool(); conv(256, 128); conv(256, 256); conv(256, 256); tap(3);
    pool(); conv(512, 256); conv(512, 512); conv(512, 512); tap(4);
    pool(); conv(512, 512); conv(512, 512); conv(512, 512); tap(5);
}

struct Range {
    int a = 0, b = 0;                 // [a, b)
    bool empty() const { return a >= b; }
    int n() const { return b > a ? b - a : 0; }
};

inline Range hull(Range p, Range q)
{
    if (p.empty()) return q;
    if (q.empty()) return p;
    Range r;
    r.a = std::min(p.a, q.a);
    r.b = std::max(p.b, q.b);
    return r;
}

// Per-activation geometry of an h x w input: activation 0 is the image, activation j the output of the j-th conv / pool.
struct LpGeom {
    std::vector<int> H, W, C, S;      // extent, channels and cumulative stride per activation
    std::vector<int> act_of_layer;    // activation a layer reads (conv / pool) or taps
};

inline bool lp_geometry(const std::vector<LpLayer> &L, int h, int w, LpGeom &G)
{
    G.H = {h}; G.W = {w}; G.C = {3}; G.S = {1};
    G.act_of_layer.clear();
    for (auto &l : L) {
        G.act_of_layer.push_back((int)G.H.size() - 1);
        if (l.kind == LP_TAP) continue;
        const int hi = G.H.back(), wi = G.W.back();
        const int ho = (hi + 2 * l.p - l.k) / l.s + 1, wo = (wi + 2 * l.p - l.k) / l.s + 1;
        if (hi + 2 * l.p < l.k || wi + 2 * l.p < l.k || ho < 1 || wo < 1) return false;
        G.H.push_back(ho); G.W.push_back(wo);
        G.C.push_back(l.kind == LP_CONV ? l.cout : G.C.back());
        G.S.push_back(G.S.back() * l.s);
    }
    return true;
}

// Ranges (one axis) every activation of a tile must cover: its own part of every tapped activation plus what the
// deeper layers need of it.  t0 / t1: the tile's span in input pixels (t1 < 0: to the end).
inline void lp_ranges(const std::vector<LpLayer> &L, const LpGeom &G, const std::vector<int> &ext, int t0, int t1,
                      std::vector<Range> &need, std::vector<Range> &own)
{
    const int na = (int)ext.size();
    need.assign(na, Range());
    own.assign(na, Range());
    for (int j = 0; j < na; ++j) {
        own[j].a = std::min(t0 / G.S[j], ext[j]);
        own[j].b = t1 < 0 ? ext[j] : std::min(t1 / G.S[j], ext[j]);
    }
    for (int li = (int)L.size() - 1; li >= 0; --li) {
        const LpLayer &l = L[li];
        const int ai = G.act_of_layer[li];
        if (l.kind == LP_TAP) {
            need[ai] = hull(need[ai], own[ai]);
            continue;
        }
        const Range o = need[ai + 1];
        if (o.empty()) continue;
        Range r;
        r.a = std::max(o.a * l.s - l.p, 0);
        r.b = std::min((o.b - 1) * l.s - l.p + l.k, ext[ai]);
        need[ai] = hull(need[ai], r);
    }
}

// The tile grid of an h x w image: tile <= 0 (or a tile no smaller than the side) is one tile along that axis.
inline void lp_tile_grid(int h, int w, int tile, int &tiles_x, int &tiles_y)
{
    tiles_x = tile <= 0 || tile >= w ? 1 : (w + tile - 1) / tile;
    tiles_y = tile <= 0 || tile >= h ? 1 : (h + tile - 1) / tile;
}

// What the forward of tile ti (row-major in the tile grid) works on: per activation the needed and the owned range on both
// axes, the buffer pitch (columns rounded up to 4 floats) and plane, and the floats one activation buffer must hold.
// Activation 0 is read from the image itself and has no buffer.
struct LpPlan {
    std::vector<Range> ny, oy, nx, ox;
    std::vector<int> pitch;
    std::vector<long long> plane;
    size_t need_floats = 0;
};

inline void lp_plan(const std::vector<LpLayer> &L, const LpGeom &G, int tile, int ti, LpPlan &P)
{
    int tiles_x, tiles_y;
    lp_tile_grid(G.H[0], G.W[0], tile, tiles_x, tiles_y);
    const int ty = ti / tiles_x, tx = ti % tiles_x;
    lp_ranges(L, G, G.H, ty * tile, ty + 1 < tiles_y ? (ty + 1) * tile : -1, P.ny, P.oy);
    lp_ranges(L, G, G.W, tx * tile, tx + 1 < tiles_x ? (tx + 1) * tile : -1, P.nx, P.ox);
    const int na = (int)G.H.size();
    P.pitch.assign(na, 0);
    P.plane.assign(na, 0);
    P.need_floats = 0;
    for (int j = 1; j < na; ++j) {
        P.pitch[j] = (P.nx[j].n() + 3) / 4 * 4;
        P.plane[j] = (long long)P.ny[j].n() * P.pitch[j];
        P.need_floats = std::max(P.need_floats, (size_t)P.plane[j] * G.C[j]);
    }
}

// The plan of one tile as the host-only exports (sr_lpips_tile_plan, sr_dists_tile_plan) hand it out: per activation
// LP_PLAN_FIELDS ints -- needed rows, owned rows, needed columns, owned columns (each [a, b)), pitch, channels, full height, width.
constexpr int LP_PLAN_FIELDS = 12;

inline void lp_plan_records(const std::vector<LpLayer> &L, const LpGeom &G, int tile, int ti, int *n_act, int *rec, long long *floats)
{
    LpPlan P;
    lp_plan(L, G, tile, ti, P);
    const int na = (int)G.H.size();
    *n_act = na;
    *floats = (long long)P.need_floats;
    for (int j = 0; j < na; ++j) {
        const int r[LP_PLAN_FIELDS] = {P.ny[j].a, P.ny[j].b, P.oy[j].a, P.oy[j].b, P.nx[j].a, P.nx[j].b, P.ox[j].a, P.ox[j].b,
                                       P.pitch[j], G.C[j], G.H[j], G.W[j]};
        std::copy(r, r + LP_PLAN_FIELDS, rec + (size_t)j * LP_PLAN_FIELDS);
    }
}

}  // namespace
