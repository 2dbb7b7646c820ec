// sr_hat_host.cpp -- the host side of the HAT backend: what a description may hold beyond the shared front, the list of tables a
// model is made from, the index of the overlapping cross-attention (256 queries x 576 keys) and the SwFamily of its plan.  The
// description's front, the table emitters, the relative-position index, the extent rule and the plan itself are
// sr_swinir_host.cpp's (sr_swinir.h).  Pure host code: no device call, no context -- sr_hat.hip plans with ht_geometry;
// tools/sanitize/hat_driver.cpp runs this file under the sanitizers.  The definition is in include/sr_hip.h ("HAT").
#include "sr_hat.h"

namespace {

constexpr int HT_ROWS = 32;                            // rows of a chunk of the channel mean (sr_chan_attn.h's RC_ROWS)

}  // namespace

int ht_check_desc(const char *who, const sr_hat_desc *d)
{
    if (!d) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null description", who);
    const int C = d->n_feat, s = d->scale;
    int rc;
    if ((rc = sw_check_widths(who, C, d->n_heads, d->n_hidden))) return rc;
    if (d->n_mid < 1 || d->n_mid > C)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: a CAB middle width of %d is outside 1 <= n_mid <= C = %d", who, d->n_mid, C);
    if (d->n_squeeze < 1 || d->n_squeeze > C)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: a squeeze width of %d is outside 1 <= n_squeeze <= C = %d", who, d->n_squeeze, C);
    if ((rc = sw_check_depths(who, d->n_groups, d->depth, "RHAG"))) return rc;
    if (s < 2 || s > 4) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: upsampler pixelshuffle at scale %d (supported: 2, 3, 4)", who, s);
    return sw_check_affine(who, "conv_scale, mean and range", d->mean, d->range, d->conv_scale);
}

std::vector<SwTable> ht_tables(const sr_hat_desc &d)
{
    const int C = d.n_feat, hid = d.n_hidden, nh = d.n_heads;
    std::vector<SwTable> t;
    t.push_back({SW_T_HEAD, 1, C, 3, 3});
    t.push_back({SW_T_LN, 1, C, 0, 0});
    for (int i = 0; i < d.n_groups; ++i) {
        for (int j = 0; j < d.depth; ++j) {
            sw_emit_attention(t, C, nh, SW_T_RPB, HT_REL);
            t.push_back({HT_T_CAB0, 1, d.n_mid, C, 3});
            t.push_back({HT_T_CAB2, 1, C, d.n_mid, 3});
            t.push_back({HT_T_ATT1, 1, d.n_squeeze, C, 1});
            t.push_back({HT_T_ATT3, 1, C, d.n_squeeze, 1});
            sw_emit_mlp(t, C, hid);
        }
        sw_emit_attention(t, C, nh, HT_T_RPB_OCA, HT_REL_OCA);
        sw_emit_mlp(t, C, hid);
        t.push_back({SW_T_CONV, 1, C, C, 3});
    }
    t.push_back({SW_T_LN, 1, C, 0, 0});
    t.push_back({SW_T_CONV, 1, C, C, 3});
    sw_emit_shuffle_tail(t, C, d.scale);
    return t;
}

std::vector<SwStep> ht_tail_steps(const sr_hat_desc &d) { return sw_shuffle_steps(d.scale); }   // SwinIR's pixelshuffle reconstruction

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

int ht_geometry(const char *who, const sr_hat_desc &d, int h, int w, int tail, SwGeom &g)
{
    const SwFamily f{HT_WIN, 5, sw_pad64(d.n_mid), HT_ROWS, SR_HAT_TRUNK_CAP, "SR_HAT_TRUNK_CAP", true};
    return sw_plan_geometry(who, f, d.n_feat, d.n_hidden, d.scale, ht_tail_steps(d), h, w, tail, g);
}

extern "C" {

int sr_hat_plan(const sr_hat_desc *desc, int h, int w, int tail, int *hp, int *wp, int *halo, int *n_tail_tiles, size_t *workspace_bytes)
{
    int rc = ht_check_desc("sr_hat_plan", desc);
    if (rc) return rc;
    SwGeom g;
    if ((rc = ht_geometry("sr_hat_plan", *desc, h, w, tail, g))) return rc;
    sw_write_plan(g, hp, wp, halo, n_tail_tiles, workspace_bytes);
    return SR_OK;
}

int sr_hat_rel_index(int *rel, int n)
{
    if (!rel || n != HT_TOK * HT_TOK) return sr_set_error(SR_ERR_INVALID_ARG, "sr_hat_rel_index: rel must hold %d ints", HT_TOK * HT_TOK);
    sw_rel_index(HT_WIN, rel);
    return SR_OK;
}

int sr_hat_oca_index(int *idx, int n)
{
    if (!idx || n != HT_TOK * HT_KEYS) return sr_set_error(SR_ERR_INVALID_ARG, "sr_hat_oca_index: idx must hold %d ints", HT_TOK * HT_KEYS);
    ht_oca_index(idx);
    return SR_OK;
}

}  // extern "C"
