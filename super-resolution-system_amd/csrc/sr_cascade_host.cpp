// sr_cascade_host.cpp -- the host-only half of cascade detection (include/sr_hip.h, "Cascade"): the model's checks and
// packing, the scale list and the plan of a call, every refusal, the canonical order of the candidates, OpenCV's
// groupRectangles, and the restatement of the whole definition on host pointers that sr_cascade.hip is held to (the window
// evaluation itself is the text of sr_cascade.h, compiled here for the host).  No HIP here.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>

#include "sr_cascade.h"

namespace {

std::mutex g_models_mu;
std::set<const sr_cascade *> g_models;

double rnd(double v) { return std::nearbyint(v); }        // round half to even (the default rounding mode)

bool bad_host_image(const uint8_t *img, int64_t stride, int h, int w, int cn)
{
    return !img || h < 1 || w < 1 || (cn != 1 && cn != 3 && cn != 4) || stride < (int64_t)w * cn;
}

uint32_t f32_bits(float f)
{
    uint32_t v;
    std::memcpy(&v, &f, 4);
    return v;
}

// rectangle inside the window, not empty -> packed; false otherwise
bool pack_rect(int x, int y, int w, int h, int W0, int H0, uint32_t *out)
{
    if (x < 0 || y < 0 || w < 1 || h < 1 || (long long)x + w > W0 || (long long)y + h > H0) return false;
    *out = (uint32_t)x | (uint32_t)y << 8 | (uint32_t)w << 16 | (uint32_t)h << 24;
    return true;
}

// The offsets of every scale and the workspace sections.  SR_ERR_UNSUPPORTED for a pyramid whose samples, table elements or
// positions do not fit an int32 (the image cap and the step cap do not bound them at a factor close to 1).
int layout(const char *who, const sr_cascade *m, int h, int w, CcPlan *pl)
{
    const int W0 = m->info.win_w, H0 = m->info.win_h;
    pl->npx = (long long)h * w;
    pl->dev.clear();
    long long pix = 0, tab = 0, pos = 0, rows = 0, cols = 0;
    long long all_tab = 0;
    for (const sr_cascade_scale &s : pl->scales) all_tab += (long long)(s.sw + 1) * (s.sh + 1);        // the largest of the three
    if (all_tab > CC_MAX_INDEX)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: the pyramid of %d scales holds %lld table elements, above the cap of %lld",
                            who, (int)pl->scales.size(), all_tab, (long long)CC_MAX_INDEX);
    for (sr_cascade_scale &s : pl->scales) {
        s.nx = (s.sw - W0) / s.step + 1;
        s.ny = (s.sh - H0) / s.step + 1;
        pl->dev.push_back({s.sw, s.sh, s.step, s.nx, s.ny, (int)pix, (int)tab, (int)pos, (int)rows, (int)cols, 0, 0});
        pix += (long long)s.sw * s.sh;
        tab += (long long)(s.sw + 1) * (s.sh + 1);
        pos += (long long)s.nx * s.ny;
        rows += s.sh;
        cols += s.sw + 1;
    }
    pl->plane_px = pix;
    pl->table_el = tab;
    pl->positions = pos;
    pl->rows = rows;
    pl->cols = cols;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at += up256(bytes);
        return o;
    };
    pl->off_gray = take((size_t)pl->npx);
    pl->off_planes = take((size_t)pix);
    pl->off_tab = take((size_t)tab * 4);
    pl->off_sq = take(m->info.feature_type == SR_CASCADE_HAAR ? (size_t)tab * 4 : 0);
    pl->off_stumps = take(m->stumps.size() * 4);
    pl->off_stages = take(m->stages.size() * sizeof(CcStage));
    pl->off_scales = take(SR_CASCADE_MAX_SCALES * sizeof(CcScale));
    pl->off_ctr = take(256);
    pl->off_surv = take((size_t)pos * 4);
    pl->off_cand = take((size_t)pos * 4);
    pl->total = at;
    return SR_OK;
}

int check_image_size(const char *who, int h, int w)
{
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: bad arguments", who);
    if ((long long)h * w > CC_MAX_PIXELS)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d x %d is above the cap of %lld pixels", who, w, h, (long long)CC_MAX_PIXELS);
    return SR_OK;
}

std::vector<uint8_t> gray_plane(const uint8_t *img, int64_t stride, int h, int w, int cn)
{
    std::vector<uint8_t> g((size_t)h * w);
    for (int y = 0; y < h; ++y) {
        const uint8_t *row = img + (int64_t)y * stride;
        for (int x = 0; x < w; ++x) {
            const uint8_t *px = row + (size_t)x * cn;
            g[(size_t)y * w + x] = (uint8_t)(cn == 1 ? px[0] : (px[0] * 3735 + px[1] * 19235 + px[2] * 9798 + (1 << 14)) >> 15);
        }
    }
    return g;
}

std::vector<uint8_t> scaled_plane(const std::vector<uint8_t> &g, int h, int w, int sh, int sw)
{
    std::vector<uint8_t> p((size_t)sh * sw);
    for (int y = 0; y < sh; ++y)
        for (int x = 0; x < sw; ++x) p[(size_t)y * sw + x] = (uint8_t)cc_resample(g.data(), w, h, sw, sh, x, y);
    return p;
}

// (sw + 1) x (sh + 1) wrapping tables of the plane (and of its squares)
void tables(const std::vector<uint8_t> &p, int sh, int sw, bool squares, std::vector<uint32_t> &T, std::vector<uint32_t> &S)
{
    const int pitch = sw + 1;
    T.assign((size_t)pitch * (sh + 1), 0u);
    S.assign(squares ? T.size() : 0, 0u);
    for (int y = 0; y < sh; ++y) {
        uint32_t rs = 0, rq = 0;
        for (int x = 0; x < sw; ++x) {
            const uint32_t v = p[(size_t)y * sw + x];
            rs += v;
            rq += v * v;
            T[(size_t)(y + 1) * pitch + x + 1] = T[(size_t)y * pitch + x + 1] + rs;
            if (squares) S[(size_t)(y + 1) * pitch + x + 1] = S[(size_t)y * pitch + x + 1] + rq;
        }
    }
}

// stages passed per position of one scale, row-major
void eval_scale(const sr_cascade *m, const std::vector<uint8_t> &plane, const sr_cascade_scale &s, std::vector<int> &passed)
{
    std::vector<uint32_t> T, S;
    const bool haar = m->info.feature_type == SR_CASCADE_HAAR;
    tables(plane, s.sh, s.sw, haar, T, S);
    passed.resize((size_t)s.nx * s.ny);
    for (int iy = 0; iy < s.ny; ++iy)
        for (int ix = 0; ix < s.nx; ++ix)
            passed[(size_t)iy * s.nx + ix] = cc_run(m->stages.data(), m->stumps.data(), 0, 0, m->info.n_stages, m->info.feature_type,
                                                    T.data(), haar ? S.data() : nullptr, s.sw + 1, ix * s.step, iy * s.step,
                                                    m->info.win_w, m->info.win_h);
}

bool similar(const sr_tile_rect &a, const sr_tile_rect &b)
{
    const double delta = 0.2 * ((double)std::min(a.w, b.w) + (double)std::min(a.h, b.h)) * 0.5;
    const long long dx = (long long)a.x - b.x, dy = (long long)a.y - b.y;                      // 64 bits: any int rectangle
    return std::llabs(dx) <= delta && std::llabs(dy) <= delta && std::llabs(dx + a.w - b.w) <= delta && std::llabs(dy + a.h - b.h) <= delta;
}

}  // namespace

bool cascade_is_live(const sr_cascade *m)
{
    std::lock_guard<std::mutex> lk(g_models_mu);
    return m && g_models.count(m) && m->magic == CC_MAGIC;
}

int cascade_plan(const char *who, const sr_cascade *m, int h, int w, const sr_cascade_params *p, CcPlan *out)
{
    if (!cascade_is_live(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed cascade", who);
    if (!p || p->min_w < 0 || p->min_h < 0 || p->max_w < 0 || p->max_h < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: bad arguments", who);
    const int rc = check_image_size(who, h, w);
    if (rc) return rc;
    if (!(p->scale_factor > 1.0)) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: scale_factor must be above 1 (and not NaN)", who);
    if (p->min_neighbors < 0) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: min_neighbors %d is negative", who, p->min_neighbors);
    const int W0 = m->info.win_w, H0 = m->info.win_h;
    const double max_w = p->max_w ? p->max_w : w, max_h = p->max_h ? p->max_h : h;
    CcPlan pl;
    double f = 1.0;
    for (int it = 0;; ++it, f *= p->scale_factor) {
        const double ww = rnd(W0 * f), wh = rnd(H0 * f), sw = rnd(w / f), sh = rnd(h / f);
        if (ww > max_w || wh > max_h) break;
        if (sw < W0 || sh < H0) break;
        if (it >= SR_CASCADE_MAX_SCALES)
            return sr_set_error(SR_ERR_UNSUPPORTED, "%s: more than %d steps in the scale list (scale_factor %.17g)", who,
                                SR_CASCADE_MAX_SCALES, p->scale_factor);
        if (ww < p->min_w || wh < p->min_h) continue;
        pl.scales.push_back({f, (int)ww, (int)wh, (int)sw, (int)sh, f <= 2.0 ? 2 : 1, 0, 0});
    }
    const int lrc = layout(who, m, h, w, &pl);
    if (lrc) return lrc;
    *out = std::move(pl);
    return SR_OK;
}

int cascade_plan_map(const char *who, const sr_cascade *m, int h, int w, int step, CcPlan *out)
{
    if (!cascade_is_live(m)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null or destroyed cascade", who);
    if (step != 1 && step != 2) return sr_set_error(SR_ERR_INVALID_ARG, "%s: step must be 1 or 2", who);
    const int rc = check_image_size(who, h, w);
    if (rc) return rc;
    CcPlan pl;
    if (w >= m->info.win_w && h >= m->info.win_h) pl.scales.push_back({1.0, m->info.win_w, m->info.win_h, w, h, step, 0, 0});
    const int lrc = layout(who, m, h, w, &pl);
    if (lrc) return lrc;
    *out = std::move(pl);
    return SR_OK;
}

void cascade_candidates(const CcPlan &pl, const uint32_t *pos, size_t n, sr_tile_rect *out)
{
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) {
        while (k + 1 < pl.dev.size() && pos[i] >= (uint32_t)pl.dev[k + 1].pos_off) ++k;
        const sr_cascade_scale &s = pl.scales[k];
        const int q = (int)(pos[i] - (uint32_t)pl.dev[k].pos_off), iy = q / s.nx, ix = q - iy * s.nx;
        out[i] = {(int)rnd(ix * s.step * s.f), (int)rnd(iy * s.step * s.f), s.win_w, s.win_h};
    }
}

extern "C" {

int sr_cascade_create(const sr_cascade_info *info, const float *stage_thr, const int *stage_count, const int *stump_feature,
                      const float *stump_thr, const float *stump_leaves, const int32_t *stump_subsets, const int *feat_nrects,
                      const int *feat_rects, const float *feat_weights, sr_cascade **out)
{
    const char *who = "sr_cascade_create";
    if (!info || !out) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    *out = nullptr;
    const sr_cascade_info &d = *info;
    if (d.old_layout) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: the old opencv-haar-classifier XML layout is not read", who);
    if (d.feature_type != SR_CASCADE_LBP && d.feature_type != SR_CASCADE_HAAR)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: feature type %d is neither LBP nor HAAR (HOG cascades are not built)", who, d.feature_type);
    if (d.stage_type != 0) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: stageType other than BOOST", who);
    if (d.max_tree_nodes != 1) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: trees of %d nodes; only depth-1 stumps are built", who, d.max_tree_nodes);
    const bool haar = d.feature_type == SR_CASCADE_HAAR;
    if (haar && d.tilted) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: tilted Haar rectangles are not built", who);
    if (haar && d.max_rects > 3) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d rectangles in a Haar feature; at most 3", who, d.max_rects);
    if (!haar && d.max_cat_count != 256) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: LBP maxCatCount %d is not 256", who, d.max_cat_count);
    if (d.win_w < CC_MIN_SIDE || d.win_w > CC_MAX_SIDE || d.win_h < CC_MIN_SIDE || d.win_h > CC_MAX_SIDE)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: window %d x %d outside %d..%d", who, d.win_w, d.win_h, CC_MIN_SIDE, CC_MAX_SIDE);
    if (d.n_stages == 0) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: zero stages", who);
    if (d.n_stages < 0 || d.n_stumps < 0 || d.n_features < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: negative count", who);
    if (d.n_stages > CC_MAX_STAGES || d.n_stumps > CC_MAX_STUMPS)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d stages / %d stumps above the caps of %d / %d", who, d.n_stages, d.n_stumps,
                            CC_MAX_STAGES, CC_MAX_STUMPS);
    if (!stage_thr || !stage_count || (d.n_stumps && (!stump_feature || !stump_leaves)) || (d.n_features && !feat_rects) ||
        (d.n_stumps && (haar ? !stump_thr : !stump_subsets)) || (haar && d.n_features && (!feat_nrects || !feat_weights)))
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: a model table is missing", who);
    sr_cascade *m = new sr_cascade;
    m->info = d;
    int at = 0;
    for (int s = 0; s < d.n_stages; ++s) {
        if (stage_count[s] < 0 || stage_count[s] > d.n_stumps - at) {
            delete m;
            return sr_set_error(SR_ERR_INVALID_ARG, "%s: the stage sizes do not add up to %d stumps", who, d.n_stumps);
        }
        if (std::isnan(stage_thr[s])) {
            delete m;
            return sr_set_error(SR_ERR_UNSUPPORTED, "%s: NaN threshold of stage %d", who, s);
        }
        m->stages.push_back({at, stage_count[s], stage_thr[s], 0});
        at += stage_count[s];
    }
    if (at != d.n_stumps) {
        delete m;
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: the stage sizes do not add up to %d stumps", who, d.n_stumps);
    }
    m->stumps.assign((size_t)d.n_stumps * CC_STUMP_WORDS, 0u);
    for (int k = 0; k < d.n_stumps; ++k) {
        uint32_t *st = m->stumps.data() + (size_t)k * CC_STUMP_WORDS;
        const int fi = stump_feature[k];
        int rc = SR_OK;
        if (fi < 0 || fi >= d.n_features) rc = sr_set_error(SR_ERR_UNSUPPORTED, "%s: stump %d names feature %d of %d", who, k, fi, d.n_features);
        else if (std::isnan(stump_leaves[2 * k]) || std::isnan(stump_leaves[2 * k + 1]) || (haar && std::isnan(stump_thr[k])))
            rc = sr_set_error(SR_ERR_UNSUPPORTED, "%s: NaN leaf or threshold in stump %d", who, k);
        else if (!haar) {
            const int *r = feat_rects + 4 * (size_t)fi;
            // the grid is 3 x 3 blocks: its far corner has to lie inside the window
            if (r[2] < 1 || r[3] < 1 || r[2] > 85 || r[3] > 85 || !pack_rect(r[0], r[1], 3 * r[2], 3 * r[3], d.win_w, d.win_h, st))
                rc = sr_set_error(SR_ERR_UNSUPPORTED, "%s: the grid of LBP feature %d lies outside the window", who, fi);
            else {
                st[0] = (uint32_t)r[0] | (uint32_t)r[1] << 8 | (uint32_t)r[2] << 16 | (uint32_t)r[3] << 24;
                for (int j = 0; j < 8; ++j) st[1 + j] = (uint32_t)stump_subsets[8 * (size_t)k + j];
                st[9] = f32_bits(stump_leaves[2 * k]);
                st[10] = f32_bits(stump_leaves[2 * k + 1]);
            }
        } else {
            const int n = feat_nrects[fi];
            if (n < 2 || n > 3) rc = sr_set_error(SR_ERR_UNSUPPORTED, "%s: Haar feature %d has %d rectangles; 2 or 3 are built", who, fi, n);
            else {
                st[0] = (uint32_t)n;
                st[1] = f32_bits(stump_thr[k]);
                st[2] = f32_bits(stump_leaves[2 * k]);
                st[3] = f32_bits(stump_leaves[2 * k + 1]);
                for (int i = 0; i < n && rc == SR_OK; ++i) {
                    const int *r = feat_rects + 12 * (size_t)fi + 4 * i;
                    const float wgt = feat_weights[3 * (size_t)fi + i];
                    if (std::isnan(wgt)) rc = sr_set_error(SR_ERR_UNSUPPORTED, "%s: NaN weight in Haar feature %d", who, fi);
                    else if (!pack_rect(r[0], r[1], r[2], r[3], d.win_w, d.win_h, st + 4 + 2 * i))
                        rc = sr_set_error(SR_ERR_UNSUPPORTED, "%s: a rectangle of Haar feature %d lies outside the window", who, fi);
                    st[5 + 2 * i] = f32_bits(wgt);
                }
            }
        }
        if (rc) {
            delete m;
            return rc;
        }
    }
    for (const CcStage &g : m->stages) {
        if (m->dense_stumps + g.count > CC_DENSE_STUMPS || m->dense_stages >= CC_DENSE_STAGES) break;
        m->dense_stumps += g.count;
        ++m->dense_stages;
    }
    {
        std::lock_guard<std::mutex> lk(g_models_mu);
        g_models.insert(m);
    }
    *out = m;
    return SR_OK;
}

int sr_cascade_destroy(sr_cascade *model)
{
    if (!model) return SR_OK;
    {
        std::lock_guard<std::mutex> lk(g_models_mu);
        if (!g_models.erase(model)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_destroy: not a live cascade");
    }
    model->magic = 0;
    delete model;
    return SR_OK;
}

int sr_cascade_desc(const sr_cascade *model, sr_cascade_info *out)
{
    if (!cascade_is_live(model) || !out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_desc: null or destroyed cascade");
    *out = model->info;
    return SR_OK;
}

int sr_cascade_default_params(sr_cascade_params *out)
{
    if (!out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_default_params: null output");
    *out = {1.1, 4, 0, 0, 0, 0};
    return SR_OK;
}

int sr_cascade_plan(const sr_cascade *model, int h, int w, const sr_cascade_params *params, sr_cascade_scale *scales, int cap,
                    int *n_scales, size_t *workspace_bytes, int64_t *positions)
{
    if (cap < 0 || (cap > 0 && !scales)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_plan: bad arguments");
    CcPlan pl;
    const int rc = cascade_plan("sr_cascade_plan", model, h, w, params, &pl);
    if (rc) return rc;
    for (int i = 0; i < cap && i < (int)pl.scales.size(); ++i) scales[i] = pl.scales[i];
    if (n_scales) *n_scales = (int)pl.scales.size();
    if (workspace_bytes) *workspace_bytes = pl.total;
    if (positions) *positions = pl.positions;
    return SR_OK;
}

int sr_cascade_group(const sr_tile_rect *cands, int64_t n, int min_neighbors, sr_tile_rect *rects, int64_t *m)
{
    if (n < 0 || (n > 0 && (!cands || !rects)) || !m) return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_group: bad arguments");
    if (min_neighbors < 0) return sr_set_error(SR_ERR_UNSUPPORTED, "sr_cascade_group: min_neighbors %d is negative", min_neighbors);
    if (min_neighbors == 0 || n == 0) {
        for (int64_t i = 0; i < n; ++i) rects[i] = cands[i];
        *m = n;
        return SR_OK;
    }
    // classes: the transitive closure of similar(), numbered by their first member
    std::vector<int64_t> root((size_t)n);
    for (int64_t i = 0; i < n; ++i) root[i] = i;
    auto find = [&](int64_t a) {
        while (root[a] != a) a = root[a] = root[root[a]];
        return a;
    };
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = i + 1; j < n; ++j)
            if (similar(cands[i], cands[j])) {
                const int64_t a = find(i), b = find(j);
                if (a != b) root[std::max(a, b)] = std::min(a, b);        // the root of a class is its first member
            }
    std::vector<int> cls((size_t)n, -1);
    int nclasses = 0;
    for (int64_t i = 0; i < n; ++i)
        if (find(i) == i) cls[i] = nclasses++;
    struct Sum64 {
        int64_t x, y, w, h;                      // 64 bits: a long chained class on a wide image overflows an int
    };
    std::vector<Sum64> acc((size_t)nclasses, Sum64{0, 0, 0, 0});
    std::vector<int> cnt((size_t)nclasses, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int c = cls[find(i)];
        acc[c].x += cands[i].x;
        acc[c].y += cands[i].y;
        acc[c].w += cands[i].w;
        acc[c].h += cands[i].h;
        ++cnt[c];
    }
    auto mean = [](int64_t v, float s) {
        const float prod = (float)v * s;
        return (int)std::nearbyintf(prod);
    };
    std::vector<sr_tile_rect> sum((size_t)nclasses);
    for (int c = 0; c < nclasses; ++c) {
        const float s = 1.f / (float)cnt[c];
        sum[c] = {mean(acc[c].x, s), mean(acc[c].y, s), mean(acc[c].w, s), mean(acc[c].h, s)};
    }
    int64_t k = 0;
    for (int i = 0; i < nclasses; ++i) {
        const sr_tile_rect r1 = sum[i];
        const int n1 = cnt[i];
        if (n1 <= min_neighbors) continue;
        int j = 0;
        for (; j < nclasses; ++j) {
            const int n2 = cnt[j];
            if (j == i || n2 <= min_neighbors) continue;
            const sr_tile_rect r2 = sum[j];
            const int dx = (int)rnd(r2.w * 0.2), dy = (int)rnd(r2.h * 0.2);
            if (r1.x >= r2.x - dx && r1.y >= r2.y - dy && r1.x + r1.w <= r2.x + r2.w + dx && r1.y + r1.h <= r2.y + r2.h + dy &&
                (n2 > std::max(3, n1) || n1 < 3))
                break;
        }
        if (j == nclasses) rects[k++] = r1;
    }
    *m = k;
    return SR_OK;
}

int sr_cascade_host_u8(const sr_cascade *model, const uint8_t *img, int64_t stride, int h, int w, int cn,
                       const sr_cascade_params *params, sr_tile_rect *cands, int64_t cap, int64_t *count)
{
    if (bad_host_image(img, stride, h, w, cn) || !count || cap < 0 || (cap > 0 && !cands))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_host_u8: bad arguments");
    CcPlan pl;
    const int rc = cascade_plan("sr_cascade_host_u8", model, h, w, params, &pl);
    if (rc) return rc;
    const std::vector<uint8_t> g = gray_plane(img, stride, h, w, cn);
    std::vector<uint32_t> pos;
    std::vector<int> passed;
    for (size_t k = 0; k < pl.scales.size(); ++k) {
        const sr_cascade_scale &s = pl.scales[k];
        eval_scale(model, scaled_plane(g, h, w, s.sh, s.sw), s, passed);
        for (size_t q = 0; q < passed.size(); ++q)
            if (passed[q] == model->info.n_stages) pos.push_back((uint32_t)pl.dev[k].pos_off + (uint32_t)q);
    }
    *count = (int64_t)pos.size();
    std::vector<sr_tile_rect> all(pos.size());
    cascade_candidates(pl, pos.data(), pos.size(), all.data());
    const size_t m = std::min<size_t>(all.size(), (size_t)cap);
    if (m) std::memcpy(cands, all.data(), m * sizeof(sr_tile_rect));
    return SR_OK;
}

int sr_cascade_plane_host_u8(const sr_cascade *model, const uint8_t *img, int64_t stride, int h, int w, int cn,
                             const sr_cascade_params *params, int k, uint8_t *plane)
{
    if (bad_host_image(img, stride, h, w, cn) || !plane) return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_plane_host_u8: bad arguments");
    CcPlan pl;
    const int rc = cascade_plan("sr_cascade_plane_host_u8", model, h, w, params, &pl);
    if (rc) return rc;
    if (k < 0 || k >= (int)pl.scales.size())
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_plane_host_u8: scale %d of %d", k, (int)pl.scales.size());
    const std::vector<uint8_t> p = scaled_plane(gray_plane(img, stride, h, w, cn), h, w, pl.scales[k].sh, pl.scales[k].sw);
    std::memcpy(plane, p.data(), p.size());
    return SR_OK;
}

int sr_cascade_stage_map_host_u8(const sr_cascade *model, const uint8_t *img, int64_t stride, int h, int w, int cn, int step,
                                 int32_t *map, int64_t cap, int64_t *count)
{
    if (bad_host_image(img, stride, h, w, cn) || !count || cap < 0 || (cap > 0 && !map))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_cascade_stage_map_host_u8: bad arguments");
    CcPlan pl;
    const int rc = cascade_plan_map("sr_cascade_stage_map_host_u8", model, h, w, step, &pl);
    if (rc) return rc;
    *count = pl.positions;
    if (pl.positions > cap || pl.scales.empty()) return SR_OK;
    std::vector<int> passed;
    eval_scale(model, gray_plane(img, stride, h, w, cn), pl.scales[0], passed);
    for (size_t q = 0; q < passed.size(); ++q) map[q] = passed[q];
    return SR_OK;
}

}  // extern "C"
