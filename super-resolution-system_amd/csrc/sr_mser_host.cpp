// sr_mser_host.cpp -- the host-only half of MSER text-region detection (include/sr_hip.h, "MSER"): the plan and every
// refusal, the canonical orders of the outputs, the text-box filter of tiling_module.py:231-235, and the restatement of
// the whole definition on host pointers (a sorted-pixel sequential union-find; nodes of one level that meet are merged
// through an alias table) that sr_mser.hip is held to at sizes the Python restatement is too slow for.  No HIP here.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include "sr_mser.h"

int mser_check(const char *who, int h, int w, const sr_mser_params *p)
{
    if (h < 1 || w < 1 || !p) return sr_set_error(SR_ERR_INVALID_ARG, "%s: bad arguments", who);
    if ((long long)h * w > MSER_MAX_PIXELS)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d x %d is above the cap of %lld pixels", who, w, h, (long long)MSER_MAX_PIXELS);
    if (p->delta < 1 || p->delta > 255) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: delta %d outside 1..255", who, p->delta);
    if (p->min_area < 1) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: min_area %d below 1", who, p->min_area);
    if (p->max_area < p->min_area)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: max_area %d below min_area %d", who, p->max_area, p->min_area);
    if (!(p->max_variation >= 0.0)) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: max_variation is negative or NaN", who);
    if (!(p->min_diversity >= 0.0)) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: min_diversity is negative or NaN", who);
    return SR_OK;
}

void mser_layout(int h, int w, MserPlan *out)
{
    MserPlan p;
    const size_t n = (size_t)h * w;
    p.npx = (long long)n;
    p.node_cap = (long long)n;
    p.list_bytes = std::max(up256(n * 8), (size_t)MSER_MIN_LIST_BYTES);
    p.off_gray = 0;
    p.off_order = up256(n);
    p.off_parent = p.off_order + up256(n * 4);
    p.off_nor = p.off_parent + up256(n * 4);
    p.off_list = p.off_nor + up256(n * 4);
    p.off_nodes = p.off_list + p.list_bytes;
    p.off_ctr = p.off_nodes + up256(n * sizeof(MserNode));
    p.total = p.off_ctr + 4096;
    *out = p;
}

void mser_sort_regions(sr_mser_region *r, size_t n)
{
    std::sort(r, r + n, [](const sr_mser_region &a, const sr_mser_region &b) {
        if (a.polarity != b.polarity) return a.polarity < b.polarity;
        if (a.level != b.level) return a.level < b.level;
        return a.seed < b.seed;
    });
}

void mser_canonical_tree(const std::vector<MserNode> &nodes, sr_mser_node *out)
{
    std::vector<int> idx(nodes.size());
    std::iota(idx.begin(), idx.end(), 0);
    std::sort(idx.begin(), idx.end(), [&](int a, int b) {
        return nodes[a].level != nodes[b].level ? nodes[a].level < nodes[b].level : nodes[a].seed < nodes[b].seed;
    });
    for (size_t i = 0; i < idx.size(); ++i) {
        const MserNode &n = nodes[idx[i]];
        out[i] = {n.level, n.area, n.x0, n.y0, n.x1, n.y1, n.seed, n.parent >= 0 ? nodes[n.parent].level : -1,
                  n.parent >= 0 ? nodes[n.parent].seed : -1};
    }
}

namespace {

bool bad_host_image(const uint8_t *img, int64_t stride, int h, int w, int cn)
{
    return !img || h < 1 || w < 1 || (cn != 1 && cn != 3 && cn != 4) || stride < (int64_t)w * cn;
}

// The gray plane of the content section: cv2.COLOR_BGR2GRAY applied to RGB data (15-bit rule), cn 1 the value itself.
std::vector<uint8_t> gray_plane(const uint8_t *img, int64_t stride, int h, int w, int cn, bool bright)
{
    std::vector<uint8_t> g((size_t)h * w);
    for (int y = 0; y < h; ++y) {
        const uint8_t *row = img + (int64_t)y * stride;
        for (int x = 0; x < w; ++x) {
            const uint8_t *px = row + (size_t)x * cn;
            const int v = cn == 1 ? px[0] : (px[0] * 3735 + px[1] * 19235 + px[2] * 9798 + (1 << 14)) >> 15;
            g[(size_t)y * w + x] = (uint8_t)(bright ? 255 - v : v);
        }
    }
    return g;
}

std::vector<MserNode> host_tree(const std::vector<uint8_t> &g, int h, int w)
{
    const int n = h * w;
    std::vector<int> order(n), start(257, 0);
    for (int p = 0; p < n; ++p) ++start[g[p] + 1];
    for (int t = 0; t < 256; ++t) start[t + 1] += start[t];
    {
        std::vector<int> cur(start.begin(), start.end() - 1);
        for (int p = 0; p < n; ++p) order[cur[g[p]]++] = p;
    }
    std::vector<int> uf(n), nodeof(n, -1), alias;
    std::vector<char> active(n, 0);
    std::vector<MserNode> nodes;
    nodes.reserve(n);
    alias.reserve(n);
    auto find = [&](int p) {
        while (uf[p] != p) {
            uf[p] = uf[uf[p]];
            p = uf[p];
        }
        return p;
    };
    auto res = [&](int a) {
        int r = a;
        while (alias[r] != r) r = alias[r];
        while (alias[a] != r) {                            // compress: a flat zone merges a node per pixel into one
            const int next = alias[a];
            alias[a] = r;
            a = next;
        }
        return r;
    };
    const int dy[4] = {-1, 1, 0, 0}, dx[4] = {0, 0, -1, 1};
    for (int i = 0; i < n; ++i) {
        const int p = order[i], t = g[p], y = p / w, x = p - y * w;
        const int id = (int)nodes.size();
        nodes.push_back({t, 1, x, y, x, y, p, -1});
        alias.push_back(id);
        uf[p] = p;
        active[p] = 1;
        nodeof[p] = id;
        for (int k = 0; k < 4; ++k) {
            const int yy = y + dy[k], xx = x + dx[k];
            if (yy < 0 || yy >= h || xx < 0 || xx >= w || !active[yy * w + xx]) continue;
            const int rp = find(p), rq = find(yy * w + xx);
            if (rp == rq) continue;
            const int a = res(nodeof[rp]), b = res(nodeof[rq]);
            if (nodes[b].level == t) alias[b] = a;
            else nodes[b].parent = a;
            MserNode &A = nodes[a];
            const MserNode &B = nodes[b];
            A.area += B.area;
            A.x0 = std::min(A.x0, B.x0);
            A.y0 = std::min(A.y0, B.y0);
            A.x1 = std::max(A.x1, B.x1);
            A.y1 = std::max(A.y1, B.y1);
            A.seed = std::min(A.seed, B.seed);
            uf[rq] = rp;
            nodeof[rp] = a;
        }
    }
    std::vector<int> pos(nodes.size(), -1);
    std::vector<MserNode> out;
    for (size_t i = 0; i < nodes.size(); ++i)
        if (alias[i] == (int)i) {
            pos[i] = (int)out.size();
            out.push_back(nodes[i]);
        }
    for (MserNode &nd : out)
        if (nd.parent >= 0) nd.parent = pos[res(nd.parent)];
    return out;
}

// The rules in the order of the definition; appends the regions of one polarity (any order).
void host_select(const std::vector<MserNode> &nd, const sr_mser_params &p, int polarity, std::vector<sr_mser_region> &out)
{
    const size_t n = nd.size();
    std::vector<int> S(n);
    for (size_t i = 0; i < n; ++i) {
        int a = (int)i;
        while (nd[a].parent >= 0 && nd[nd[a].parent].level <= nd[i].level + p.delta) a = nd[a].parent;
        S[i] = nd[a].area;
    }
    std::vector<char> ok(n, 1);
    for (size_t c = 0; c < n; ++c) {
        const int q = nd[c].parent;
        if (q < 0) continue;
        const int64_t vc = (int64_t)(S[c] - nd[c].area) * nd[q].area, vq = (int64_t)(S[q] - nd[q].area) * nd[c].area;
        if (vc > vq) ok[c] = 0;
        if (vq > vc) ok[q] = 0;
    }
    for (size_t i = 0; i < n; ++i) {
        const double lim = p.max_variation * (double)nd[i].area;
        if (ok[i] && !(nd[i].area >= p.min_area && nd[i].area <= p.max_area && (double)(S[i] - nd[i].area) < lim)) ok[i] = 0;
    }
    for (size_t i = 0; i < n; ++i) {
        if (!ok[i]) continue;
        int a = nd[i].parent;
        while (a >= 0 && !ok[a]) a = nd[a].parent;
        if (a >= 0) {
            const double lim = p.min_diversity * (double)nd[a].area;
            if ((double)(nd[a].area - nd[i].area) < lim) continue;
        }
        out.push_back({polarity, nd[i].level, nd[i].area, nd[i].x0, nd[i].y0, nd[i].x1, nd[i].y1, nd[i].seed, S[i]});
    }
}

}  // namespace

extern "C" {

int sr_mser_default_params(sr_mser_params *out)
{
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_mser_default_params: null output");
    *out = {5, 60, 14400, 0.25, 0.2};
    return SR_OK;
}

int sr_mser_plan(int h, int w, const sr_mser_params *params, size_t *workspace_bytes, int64_t *node_cap)
{
    const int rc = mser_check("sr_mser_plan", h, w, params);
    if (rc) return rc;
    MserPlan p;
    mser_layout(h, w, &p);
    if (workspace_bytes) *workspace_bytes = p.total;
    if (node_cap) *node_cap = p.node_cap;
    return SR_OK;
}

int sr_mser_host_u8(const uint8_t *img, int64_t stride, int h, int w, int cn, const sr_mser_params *params, int polarity_mask,
                    sr_mser_region *regions, int64_t cap, int64_t *count)
{
    if (bad_host_image(img, stride, h, w, cn) || !count || cap < 0 || (cap > 0 && !regions) || polarity_mask < 1 || polarity_mask > 3)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_mser_host_u8: bad arguments");
    const int rc = mser_check("sr_mser_host_u8", h, w, params);
    if (rc) return rc;
    std::vector<sr_mser_region> out;
    for (int pol = 0; pol < 2; ++pol)
        if (polarity_mask >> pol & 1) host_select(host_tree(gray_plane(img, stride, h, w, cn, pol == 1), h, w), *params, pol, out);
    mser_sort_regions(out.data(), out.size());
    *count = (int64_t)out.size();
    const size_t m = std::min<size_t>(out.size(), (size_t)cap);
    if (m) std::memcpy(regions, out.data(), m * sizeof(sr_mser_region));
    return SR_OK;
}

int sr_mser_tree_host_u8(const uint8_t *img, int64_t stride, int h, int w, int cn, int polarity, sr_mser_node *nodes, int64_t cap,
                         int64_t *count)
{
    if (bad_host_image(img, stride, h, w, cn) || !count || cap < 0 || (cap > 0 && !nodes) || polarity < 0 || polarity > 1)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_mser_tree_host_u8: bad arguments");
    if ((long long)h * w > MSER_MAX_PIXELS)
        return sr_set_error(SR_ERR_UNSUPPORTED, "sr_mser_tree_host_u8: %d x %d is above the cap of %lld pixels", w, h,
                            (long long)MSER_MAX_PIXELS);
    const std::vector<MserNode> t = host_tree(gray_plane(img, stride, h, w, cn, polarity == 1), h, w);
    *count = (int64_t)t.size();
    if ((int64_t)t.size() > cap) return SR_OK;            // the count alone: call again with room for all of it
    mser_canonical_tree(t, nodes);
    return SR_OK;
}

int sr_mser_text_boxes(const sr_mser_region *regions, int64_t n, int w, sr_tile_rect *rects, int64_t *m)
{
    if (n < 0 || (n > 0 && (!regions || !rects)) || !m || w < 1)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_mser_text_boxes: bad arguments");
    int64_t k = 0;
    const double half = (double)w * 0.5;
    for (int64_t i = 0; i < n; ++i) {
        const int bw = regions[i].x1 - regions[i].x0 + 1, bh = regions[i].y1 - regions[i].y0 + 1;
        if (bw > 20 && bh > 10 && (double)bw < half) rects[k++] = {regions[i].x0, regions[i].y0, bw, bh};
    }
    *m = k;
    return SR_OK;
}

}  // extern "C"
