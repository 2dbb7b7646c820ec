// sr_swinir_host.cpp -- the host side of the SwinIR backend, and the host side that every window-attention family shares.
// Shared (sr_hat_host.cpp calls it): the front of a description check, the table emitters of an attention block, an MLP and
// the pixelshuffle reconstruction, the relative-position index of a win x win window, the extent rule and the plan
// (sw_plan_geometry: padded size, buffer geometry, the tail's sub-piece grid, every refusal by size; a SwFamily tells the
// families apart).  SwinIR's own: what its description may hold, its table list and its three reconstructions.  Pure host
// code: no device call, no context -- sr_swinir.hip plans with sw_geometry; tools/sanitize/swinir_driver.cpp runs this file
// under the sanitizers.  The definition is in include/sr_hip.h ("SwinIR").
#include <algorithm>
#include <climits>
#include <cmath>

#include "sr_swinir.h"

namespace {

constexpr int SW_MAX_ROWS = 65535 * 4;                 // rows of one launch: the head's grid is rows / 4 blocks high
constexpr int SW_MAX_C = 256, SW_MAX_D = 32, SW_MAX_L = 12, SW_MAX_DEPTH = 12;

long long pad4ll(long long v) { return (v + 3) / 4 * 4; }

}  // namespace

int sw_check_widths(const char *who, int C, int nh, int hid)
{
    if (C < 4 || C > SW_MAX_C || C % 4)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: embed_dim %d is outside 4 <= C <= %d, a multiple of 4", who, C, SW_MAX_C);
    if (nh < 1 || C % nh || C / nh > SW_MAX_D)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: num_heads %d does not divide embed_dim %d into heads of at most %d channels", who, nh, C, SW_MAX_D);
    if (hid < 1 || hid > 4 * C)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: an MLP hidden width of %d is outside 1 <= hidden <= 4 C = %d", who, hid, 4 * C);
    return SR_OK;
}

int sw_check_depths(const char *who, int n_groups, int depth, const char *group_name)
{
    if (n_groups < 1 || n_groups > SW_MAX_L || depth < 1 || depth > SW_MAX_DEPTH)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d %ss of depth %d are outside 1 <= L <= %d, 1 <= D <= %d", who, n_groups, group_name, depth,
                            SW_MAX_L, SW_MAX_DEPTH);
    return SR_OK;
}

int sw_check_affine(const char *who, const char *what, const float *mean, float range, float extra)
{
    const float v[] = {extra, mean[0], mean[1], mean[2], range};
    for (float x : v)
        if (!std::isfinite(x)) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %s must be finite", who, what);
    if (range == 0.0f) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: range must not be 0", who);
    return SR_OK;
}

int sw_check_desc(const char *who, const sr_swinir_desc *d)
{
    if (!d) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null description", who);
    const int s = d->scale;
    int rc;
    if ((rc = sw_check_widths(who, d->n_feat, d->n_heads, d->n_hidden))) return rc;
    if ((rc = sw_check_depths(who, d->n_groups, d->depth, "RSTB"))) return rc;
    switch (d->upsampler) {
    case SR_SWINIR_PIXELSHUFFLE:
        if (s < 2 || s > 4) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: upsampler pixelshuffle at scale %d (supported: 2, 3, 4)", who, s);
        break;
    case SR_SWINIR_PIXELSHUFFLEDIRECT:
        if (s < 1 || s > 4) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: upsampler pixelshuffledirect at scale %d (supported: 1 .. 4)", who, s);
        break;
    case SR_SWINIR_NEAREST_CONV:
        if (s != 4) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: upsampler nearest+conv at scale %d (supported: 4)", who, s);
        break;
    default:
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: upsampler kind %d (0 pixelshuffle, 1 pixelshuffledirect, 2 nearest+conv)", who, d->upsampler);
    }
    return sw_check_affine(who, "mean and range", d->mean, d->range);
}

void sw_emit_attention(std::vector<SwTable> &t, int C, int heads, int rpb_kind, int rpb_rows)
{
    t.push_back({SW_T_LN, 1, C, 0, 0});
    t.push_back({SW_T_QKV, 1, 3 * C, C, 1});
    t.push_back({rpb_kind, 1, rpb_rows, heads, 0});
    t.push_back({SW_T_PROJ, 1, C, C, 1});
}

void sw_emit_mlp(std::vector<SwTable> &t, int C, int hid)
{
    t.push_back({SW_T_LN, 1, C, 0, 0});
    t.push_back({SW_T_FC1, 1, hid, C, 1});
    t.push_back({SW_T_FC2, 1, C, hid, 1});
}

void sw_emit_shuffle_tail(std::vector<SwTable> &t, int C, int s)
{
    t.push_back({SW_T_CBU, 1, SW_MID, C, 3});
    if (s == 4) {
        t.push_back({SW_T_UP, 2, SW_MID * 4, SW_MID, 3});
        t.push_back({SW_T_UP, 2, SW_MID * 4, SW_MID, 3});
    } else {
        t.push_back({SW_T_UP, s, SW_MID * s * s, SW_MID, 3});
    }
    t.push_back({SW_T_LAST, 1, 3, SW_MID, 3});
}

std::vector<SwTable> sw_tables(const sr_swinir_desc &d)
{
    const int C = d.n_feat, s = d.scale;
    std::vector<SwTable> t;
    t.push_back({SW_T_HEAD, 1, C, 3, 3});
    t.push_back({SW_T_LN, 1, C, 0, 0});
    for (int i = 0; i < d.n_groups; ++i) {
        for (int j = 0; j < d.depth; ++j) {
            sw_emit_attention(t, C, d.n_heads, SW_T_RPB, SW_REL);
            sw_emit_mlp(t, C, d.n_hidden);
        }
        t.push_back({SW_T_CONV, 1, C, C, 3});
    }
    t.push_back({SW_T_LN, 1, C, 0, 0});
    t.push_back({SW_T_CONV, 1, C, C, 3});
    sw_emit_tail(t, C, s, d.upsampler);
    return t;
}

void sw_emit_tail(std::vector<SwTable> &t, int C, int s, int upsampler)
{
    if (upsampler == SR_SWINIR_PIXELSHUFFLE) {
        sw_emit_shuffle_tail(t, C, s);
    } else if (upsampler == SR_SWINIR_PIXELSHUFFLEDIRECT) {
        t.push_back({SW_T_UPD, s, 3 * s * s, C, 3});
    } else {
        t.push_back({SW_T_CBU, 1, SW_MID, C, 3});
        for (int k = 0; k < 3; ++k) t.push_back({SW_T_C64, 1, SW_MID, SW_MID, 3});
        t.push_back({SW_T_LAST, 1, 3, SW_MID, 3});
    }
}

// The tail phase's convolutions: {factor by which the stored output is replicated or shuffled, multiplier of the resolution
// the convolution itself runs at}.
std::vector<SwStep> sw_shuffle_steps(int s)
{
    if (s == 4) return {{1, 1}, {2, 1}, {2, 2}, {1, 4}};
    return {{1, 1}, {s, 1}, {1, s}};
}

std::vector<SwStep> sw_tail_steps(const sr_swinir_desc &d)
{
    if (d.upsampler == SR_SWINIR_PIXELSHUFFLEDIRECT) return {{d.scale, 1}};
    if (d.upsampler == SR_SWINIR_NEAREST_CONV) return {{2, 1}, {2, 2}, {1, 4}, {1, 4}, {1, 4}};
    return sw_shuffle_steps(d.scale);
}

void sw_rel_index(int win, int *rel)
{
    const int tok = win * win;
    for (int i = 0; i < tok; ++i)
        for (int j = 0; j < tok; ++j) {
            const int dy = i / win - j / win + win - 1, dx = i % win - j % win + win - 1;
            rel[i * tok + j] = dy * (2 * win - 1) + dx;
        }
}

void sw_backward_extents(const SwStep *steps, int n, int out_mult, int lo, int hi, int len, std::vector<int> &a, std::vector<int> &b)
{
    a.resize(n);
    b.resize(n);
    long long na = (long long)lo * out_mult, nb = (long long)hi * out_mult;
    for (int i = n - 1; i >= 0; --i) {
        const int r = steps[i].r;
        na = na / r;                                       // outward: floor, ceil
        nb = (nb + r - 1) / r;
        a[i] = (int)na;
        b[i] = (int)nb;
        na = std::max(na - 1, 0LL);
        nb = std::min(nb + 1, (long long)len * steps[i].mult);
    }
}

int sw_plan_geometry(const char *who, const SwFamily &f, int C, int hidden, int S, const std::vector<SwStep> &steps, int h, int w, int tail,
                     SwGeom &g)
{
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_SHAPE, "%s: %dx%d image", who, w, h);
    if (tail < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: %s must be >= 1, or 0 for the library's choice", who, "tail");
    const long long hp = ((long long)h + f.win - 1) / f.win * f.win;
    if (f.padded_rows) {                                    // the launches cover the PADDED rows
        if (hp > SW_MAX_ROWS)
            return sr_set_error(SR_ERR_SHAPE, "%s: %d rows, padded to %lld, are more than one launch covers (%d)", who, h, hp, SW_MAX_ROWS);
    } else if (h > SW_MAX_ROWS) {
        return sr_set_error(SR_ERR_SHAPE, "%s: %d rows are more than one launch covers (%d)", who, h, SW_MAX_ROWS);
    }
    if ((long long)h * S > INT_MAX || (long long)w * S * 3 > INT_MAX - 64)
        return sr_set_error(SR_ERR_SHAPE, "%s: a %dx%d output (x%d) overflows int", who, w, h, S);
    if (tail == 0) tail = SW_DEFAULT_TAIL;
    g.tail = tail;
    g.hp = (int)hp;
    g.wp = (int)(((long long)w + f.win - 1) / f.win * f.win);
    g.cp = sw_pad64(C);
    g.qp = std::max(sw_pad64(3 * C), sw_pad64(hidden));
    g.tp = f.tp;
    g.trunk_bufs = f.trunk_bufs;
    g.plane0 = (long long)g.hp * g.wp;
    g.chunks = f.chunk_rows ? (g.hp + f.chunk_rows - 1) / f.chunk_rows : 0;
    g.red_bytes = f.chunk_rows ? (size_t)C * g.chunks * sizeof(double) + (size_t)C * sizeof(float) : 0;
    const int planes = f.trunk_bufs * g.cp + g.tp + g.qp;
    const size_t per_pixel = (size_t)planes * sizeof(float);
    if ((size_t)g.plane0 * per_pixel > f.cap) {
        const long long fit = (long long)(f.cap / per_pixel);
        return sr_set_error(SR_ERR_SHAPE, "%s: the trunk of a %dx%d input (padded to %dx%d) is one piece of %d planes, %zu bytes per pixel, "
                            "above %s = %d GiB: at C = %d the largest input that fits has %lld pixels (about %.1f MP)",
                            who, w, h, g.wp, g.hp, planes, per_pixel, f.cap_name, (int)(f.cap >> 30), C, fit, (double)fit / 1e6);
    }
    if (g.plane0 * SW_LIN_CC > INT_MAX)                 // the mainloop indexes one cin chunk of a buffer with 32-bit offsets
        return sr_set_error(SR_ERR_SHAPE, "%s: an image of %lld activations per channel is too large (the trunk is one piece)", who, g.plane0);
    g.trunk_bytes = (size_t)g.plane0 * per_pixel;
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
    if (g.plane_t * 8 > INT_MAX || rows_t > 2LL * SW_MAX_ROWS)
        return sr_set_error(SR_ERR_SHAPE, "%s: a tail sub-piece of %lld activations per channel is too large; use a smaller tail", who, g.plane_t);
    g.workspace_bytes = g.trunk_bytes + (size_t)2 * SW_MID * (size_t)g.plane_t * sizeof(float) + (size_t)g.plane0 * 3 + g.red_bytes;
    return SR_OK;
}

int sw_geometry(const char *who, const sr_swinir_desc &d, int h, int w, int tail, SwGeom &g)
{
    const SwFamily f{SW_WIN, 4, 0, 0, SR_SWINIR_TRUNK_CAP, "SR_SWINIR_TRUNK_CAP", false};
    return sw_plan_geometry(who, f, d.n_feat, d.n_hidden, d.scale, sw_tail_steps(d), h, w, tail, g);
}

void sw_write_plan(const SwGeom &g, int *hp, int *wp, int *halo, int *n_tail_tiles, size_t *workspace_bytes)
{
    if (hp) *hp = g.hp;
    if (wp) *wp = g.wp;
    if (halo) *halo = g.halo;
    if (n_tail_tiles) *n_tail_tiles = (int)g.tail_tiles;
    if (workspace_bytes) *workspace_bytes = g.workspace_bytes;
}

extern "C" {

int sr_swinir_plan(const sr_swinir_desc *desc, int h, int w, int tail, int *hp, int *wp, int *halo, int *n_tail_tiles, size_t *workspace_bytes)
{
    int rc = sw_check_desc("sr_swinir_plan", desc);
    if (rc) return rc;
    SwGeom g;
    if ((rc = sw_geometry("sr_swinir_plan", *desc, h, w, tail, g))) return rc;
    sw_write_plan(g, hp, wp, halo, n_tail_tiles, workspace_bytes);
    return SR_OK;
}

int sr_swinir_rel_index(int *rel, int n)
{
    if (!rel || n != SW_TOK * SW_TOK) return sr_set_error(SR_ERR_INVALID_ARG, "sr_swinir_rel_index: rel must hold %d ints", SW_TOK * SW_TOK);
    sw_rel_index(SW_WIN, rel);
    return SR_OK;
}

}  // extern "C"
