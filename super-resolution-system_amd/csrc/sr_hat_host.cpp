// sr_hat_host.cpp -- the host side of the HAT backend: what a description may hold, the list of tables a model is made from, the
// relative-position index of a 16 x 16 window, the index of the overlapping cross-attention (256 queries x 576 keys) and the
// plan (padded size, buffer geometry, the tail's sub-piece grid, every refusal by size).  Pure host code: no device call, no
// context -- sr_hat.hip plans with ht_geometry; tools/sanitize/hat_driver.cpp runs this file under the sanitizers.  The
// definition is in include/sr_hip.h ("HAT").
#include <algorithm>
#include <climits>
#include <cmath>

#include "sr_hat.h"

namespace {

constexpr size_t HT_TRUNK_CAP = SR_HAT_TRUNK_CAP;
constexpr int HT_MAX_ROWS = 65535 * 4;                 // rows of one launch: the head's grid is rows / 4 blocks high
constexpr int HT_MAX_C = 256, HT_MAX_D = 32, HT_MAX_L = 12, HT_MAX_DEPTH = 12;
constexpr int HT_ROWS = 32;                            // rows of a chunk of the channel mean (sr_chan_attn.h's RC_ROWS)

long long pad4ll(long long v) { return (v + 3) / 4 * 4; }

sr_swinir_desc tail_desc(const sr_hat_desc &d)         // the reconstruction is SwinIR's pixelshuffle one
{
    sr_swinir_desc s{};
    s.n_feat = d.n_feat;
    s.scale = d.scale;
    s.upsampler = SR_SWINIR_PIXELSHUFFLE;
    return s;
}

}  // namespace

int ht_check_desc(const char *who, const sr_hat_desc *d)
{
    if (!d) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null description", who);
    const int C = d->n_feat, nh = d->n_heads, hid = d->n_hidden, s = d->scale;
    if (C < 4 || C > HT_MAX_C || C % 4)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: embed_dim %d is outside 4 <= C <= %d, a multiple of 4", who, C, HT_MAX_C);
    if (nh < 1 || C % nh || C / nh > HT_MAX_D)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: num_heads %d does not divide embed_dim %d into heads of at most %d channels", who, nh, C, HT_MAX_D);
    if (hid < 1 || hid > 4 * C)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: an MLP hidden width of %d is outside 1 <= hidden <= 4 C = %d", who, hid, 4 * C);
    if (d->n_mid < 1 || d->n_mid > C)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: a CAB middle width of %d is outside 1 <= n_mid <= C = %d", who, d->n_mid, C);
    if (d->n_squeeze < 1 || d->n_squeeze > C)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: a squeeze width of %d is outside 1 <= n_squeeze <= C = %d", who, d->n_squeeze, C);
    if (d->n_groups < 1 || d->n_groups > HT_MAX_L || d->depth < 1 || d->depth > HT_MAX_DEPTH)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d RHAGs of depth %d are outside 1 <= L <= %d, 1 <= D <= %d", who, d->n_groups, d->depth,
                            HT_MAX_L, HT_MAX_DEPTH);
    if (s < 2 || s > 4) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: upsampler pixelshuffle at scale %d (supported: 2, 3, 4)", who, s);
    const float v[] = {d->conv_scale, d->mean[0], d->mean[1], d->mean[2], d->range};
    for (float x : v)
        if (!std::isfinite(x)) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: conv_scale, mean and range must be finite", who);
    if (d->range == 0.0f) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: range must not be 0", who);
    return SR_OK;
}

std::vector<SwTable> ht_tables(const sr_hat_desc &d)
{
    const int C = d.n_feat, hid = d.n_hidden, s = d.scale, nh = d.n_heads;
    std::vector<SwTable> t;
    t.push_back({SW_T_HEAD, 1, C, 3, 3});
    t.push_back({SW_T_LN, 1, C, 0, 0});
    for (int i = 0; i < d.n_groups; ++i) {
        for (int j = 0; j < d.depth; ++j) {
            t.push_back({SW_T_LN, 1, C, 0, 0});
            t.push_back({SW_T_QKV, 1, 3 * C, C, 1});
            t.push_back({SW_T_RPB, 1, HT_REL, nh, 0});
            t.push_back({SW_T_PROJ, 1, C, C, 1});
            t.push_back({HT_T_CAB0, 1, d.n_mid, C, 3});
            t.push_back({HT_T_CAB2, 1, C, d.n_mid, 3});
            t.push_back({HT_T_ATT1, 1, d.n_squeeze, C, 1});
            t.push_back({HT_T_ATT3, 1, C, d.n_squeeze, 1});
            t.push_back({SW_T_LN, 1, C, 0, 0});
            t.push_back({SW_T_FC1, 1, hid, C, 1});
            t.push_back({SW_T_FC2, 1, C, hid, 1});
        }
        t.push_back({SW_T_LN, 1, C, 0, 0});
        t.push_back({SW_T_QKV, 1, 3 * C, C, 1});
        t.push_back({HT_T_RPB_OCA, 1, HT_REL_OCA, nh, 0});
        t.push_back({SW_T_PROJ, 1, C, C, 1});
        t.push_back({SW_T_LN, 1, C, 0, 0});
        t.push_back({SW_T_FC1, 1, hid, C, 1});
        t.push_back({SW_T_FC2, 1, C, hid, 1});
        t.push_back({SW_T_CONV, 1, C, C, 3});
    }
    t.push_back({SW_T_LN, 1, C, 0, 0});
    t.push_back({SW_T_CONV, 1, C, C, 3});
    t.push_back({SW_T_CBU, 1, SW_MID, C, 3});
    if (s == 4) {
        t.push_back({SW_T_UP, 2, SW_MID * 4, SW_MID, 3});
        t.push_back({SW_T_UP, 2, SW_MID * 4, SW_MID, 3});
    } else {
        t.push_back({SW_T_UP, s, SW_MID * s * s, SW_MID, 3});
    }
    t.push_back({SW_T_LAST, 1, 3, SW_MID, 3});
    return t;
}

std::vector<SwStep> ht_tail_steps(const sr_hat_desc &d) { return sw_tail_steps(tail_desc(d)); }

void ht_rel_index(int *rel)
{
    for (int i = 0; i < HT_TOK; ++i)
        for (int j = 0; j < HT_TOK; ++j) {
            const int dy = i / HT_WIN - j / HT_WIN + HT_WIN - 1, dx = i % HT_WIN - j % HT_WIN + HT_WIN - 1;
            rel[i * HT_TOK + j] = dy * (2 * HT_WIN - 1) + dx;
        }
}

void ht_oca_index(int *idx)
{
    constexpr int off = HT_WIN - HT_EXT + 1, side = HT_WIN + HT_EXT - 1;       // -7, 39
    for (int i = 0; i < HT_TOK; ++i)
        for (int j = 0; j < HT_KEYS; ++j) {
            const int row = j / HT_EXT - i / HT_WIN + off, col = j % HT_EXT - i % HT_WIN + off;
            const int v = row * side + col;
            idx[i * HT_KEYS + j] = v < 0 ? v + HT_REL_OCA : v;                   // torch wraps a negative index once
        }
}

int ht_wrap_oca_index(const char *who, const int *in, int *out)
{
    for (int k = 0; k < HT_TOK * HT_KEYS; ++k) {
        const int v = in[k];
        if (v < -HT_REL_OCA || v >= HT_REL_OCA)
            return sr_set_error(SR_ERR_INVALID_ARG, "%s: relative_position_index_OCA[%d][%d] = %d is outside [-%d, %d]", who, k / HT_KEYS,
                                k % HT_KEYS, v, HT_REL_OCA, HT_REL_OCA - 1);
        out[k] = v < 0 ? v + HT_REL_OCA : v;
    }
    return SR_OK;
}

int ht_geometry(const char *who, const sr_hat_desc &d, int h, int w, int tail, HtGeom &g)
{
    const int S = d.scale, C = d.n_feat;
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_SHAPE, "%s: %dx%d image", who, w, h);
    if (tail < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: %s must be >= 1, or 0 for the library's choice", who, "tail");
    const long long hp = ((long long)h + HT_WIN - 1) / HT_WIN * HT_WIN;        // the launches cover the PADDED rows
    if (hp > HT_MAX_ROWS)
        return sr_set_error(SR_ERR_SHAPE, "%s: %d rows, padded to %lld, are more than one launch covers (%d)", who, h, hp, HT_MAX_ROWS);
    if ((long long)h * S > INT_MAX || (long long)w * S * 3 > INT_MAX - 64)
        return sr_set_error(SR_ERR_SHAPE, "%s: a %dx%d output (x%d) overflows int", who, w, h, S);
    if (tail == 0) tail = SW_DEFAULT_TAIL;
    g.tail = tail;
    g.hp = (int)hp;
    g.wp = (int)(((long long)w + HT_WIN - 1) / HT_WIN * HT_WIN);
    g.cp = sw_pad64(C);
    g.qp = std::max(sw_pad64(3 * C), sw_pad64(d.n_hidden));
    g.tp = sw_pad64(d.n_mid);
    g.plane0 = (long long)g.hp * g.wp;
    g.chunks = (g.hp + HT_ROWS - 1) / HT_ROWS;
    const int planes = 5 * g.cp + g.tp + g.qp;
    const size_t per_pixel = (size_t)planes * sizeof(float);
    if ((size_t)g.plane0 * per_pixel > HT_TRUNK_CAP) {
        const long long fit = (long long)(HT_TRUNK_CAP / per_pixel);
        return sr_set_error(SR_ERR_SHAPE, "%s: the trunk of a %dx%d input (padded to %dx%d) is one piece of %d planes, %zu bytes per pixel, "
                            "above SR_HAT_TRUNK_CAP = %d GiB: at C = %d the largest input that fits has %lld pixels (about %.1f MP)",
                            who, w, h, g.wp, g.hp, planes, per_pixel, (int)(HT_TRUNK_CAP >> 30), C, fit, (double)fit / 1e6);
    }
    if (g.plane0 * SW_LIN_CC > INT_MAX)                 // the mainloop indexes one cin chunk of a buffer with 32-bit offsets
        return sr_set_error(SR_ERR_SHAPE, "%s: an image of %lld activations per channel is too large (the trunk is one piece)", who, g.plane0);
    g.trunk_bytes = (size_t)g.plane0 * per_pixel;
    const std::vector<SwStep> steps = ht_tail_steps(d);
    const int n = (int)steps.size();
    g.halo = 0;
    for (int i = n - 1; i >= 0; --i) g.halo = (g.halo + steps[i].r - 1) / steps[i].r + 1;
    std::vector<int> a, b;
    long long rows_t = 0, pitch_t = 0, cnt[2] = {0, 0};
    for (int axis = 0; axis < 2; ++axis) {
        const int len = axis == 0 ? h : w, plen = axis == 0 ? g.hp : g.wp;
        for (long long lo = 0; lo < len; lo += tail) {
            sw_backward_extents(steps.data(), n, S, (int)lo, (int)std::min<long long>(lo + tail, len), plen, a, b);
            long long m = 0;
            for (int i = 0; i + 1 < n; ++i) m = std::max(m, (long long)(b[i] - a[i]) * steps[i].r);    // the last one stores no plane
            if (axis == 0) rows_t = std::max(rows_t, m);
            else pitch_t = std::max(pitch_t, pad4ll(m));
            ++cnt[axis];
        }
    }
    g.tail_tiles = cnt[0] * cnt[1];
    if (g.tail_tiles > INT_MAX) return sr_set_error(SR_ERR_SHAPE, "%s: %lld tail sub-pieces overflow int; use a larger tail", who, g.tail_tiles);
    g.plane_t = rows_t * pitch_t;
    if (g.plane_t * 8 > INT_MAX || rows_t > 2LL * HT_MAX_ROWS)
        return sr_set_error(SR_ERR_SHAPE, "%s: a tail sub-piece of %lld activations per channel is too large; use a smaller tail", who, g.plane_t);
    g.workspace_bytes = g.trunk_bytes + (size_t)2 * SW_MID * (size_t)g.plane_t * sizeof(float) + (size_t)g.plane0 * 3 +
                        (size_t)C * g.chunks * sizeof(double) + (size_t)C * sizeof(float);
    return SR_OK;
}

extern "C" {

int sr_hat_plan(const sr_hat_desc *desc, int h, int w, int tail, int *hp, int *wp, int *halo, int *n_tail_tiles, size_t *workspace_bytes)
{
    int rc = ht_check_desc("sr_hat_plan", desc);
    if (rc) return rc;
    HtGeom g;
    rc = ht_geometry("sr_hat_plan", *desc, h, w, tail, g);
    if (rc) return rc;
    if (hp) *hp = g.hp;
    if (wp) *wp = g.wp;
    if (halo) *halo = g.halo;
    if (n_tail_tiles) *n_tail_tiles = (int)g.tail_tiles;
    if (workspace_bytes) *workspace_bytes = g.workspace_bytes;
    return SR_OK;
}

int sr_hat_rel_index(int *rel, int n)
{
    if (!rel || n != HT_TOK * HT_TOK) return sr_set_error(SR_ERR_INVALID_ARG, "sr_hat_rel_index: rel must hold %d ints", HT_TOK * HT_TOK);
    ht_rel_index(rel);
    return SR_OK;
}

int sr_hat_oca_index(int *idx, int n)
{
    if (!idx || n != HT_TOK * HT_KEYS) return sr_set_error(SR_ERR_INVALID_ARG, "sr_hat_oca_index: idx must hold %d ints", HT_TOK * HT_KEYS);
    ht_oca_index(idx);
    return SR_OK;
}

}  // extern "C"
