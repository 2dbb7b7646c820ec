// sr_swin2sr_host.cpp -- the host side of the Swin2SR backend: what a description may hold, the list of tables a model is made
// from, what a create refuses of the caller's arrays, and the two tables the cosine attention takes from the host -- the
// continuous position bias (the cpb MLP over the 15 x 15 log-spaced coordinate grid, 16 sigmoid) and the clamped logit scale.
// The description's ranges, the reconstruction's tables and steps, the relative-position index and the plan are
// sr_swinir_host.cpp's (sr_swinir.h).  Pure host code: no device call, no context -- sr_swin2sr.hip plans with s2_geometry;
// tools/sanitize/swin2sr_driver.cpp runs this file under the sanitizers.  The definition is in include/sr_hip.h ("Swin2SR").
#include <algorithm>
#include <cmath>

#include "sr_swin2sr.h"

sr_swinir_desc s2_as_swinir(const sr_swin2sr_desc &d)
{
    sr_swinir_desc s = {d.n_feat, d.n_heads, d.n_hidden, d.n_groups, d.depth, d.scale, d.upsampler, {d.mean[0], d.mean[1], d.mean[2]}, d.range};
    return s;
}

int s2_check_desc(const char *who, const sr_swin2sr_desc *d)
{
    if (!d) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null description", who);
    const sr_swinir_desc s = s2_as_swinir(*d);
    const int rc = sw_check_desc(who, &s);
    if (rc) return rc;
    if (!std::isfinite(d->mask_value)) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: mask_value must be finite", who);
    return SR_OK;
}

std::vector<SwTable> s2_tables(const sr_swin2sr_desc &d)
{
    const int C = d.n_feat, nh = d.n_heads;
    std::vector<SwTable> t;
    t.push_back({SW_T_HEAD, 1, C, 3, 3});
    t.push_back({SW_T_PROJ, 1, C, C, 1});                  // P_0
    t.push_back({SW_T_LN, 1, C, 0, 0});
    for (int i = 0; i < d.n_groups; ++i) {
        for (int j = 0; j < d.depth; ++j) {
            t.push_back({SW_T_QKV, 1, 3 * C, C, 1});
            t.push_back({S2_T_LOGIT, 1, nh, 0, 0});
            t.push_back({S2_T_CPB1, 1, S2_CPB_HIDDEN, 2, 1});
            t.push_back({S2_T_CPB2, 1, nh, S2_CPB_HIDDEN, 1});
            t.push_back({SW_T_PROJ, 1, C, C, 1});
            t.push_back({SW_T_LN, 1, C, 0, 0});
            t.push_back({SW_T_FC1, 1, d.n_hidden, C, 1});
            t.push_back({SW_T_FC2, 1, C, d.n_hidden, 1});
            t.push_back({SW_T_LN, 1, C, 0, 0});
        }
        t.push_back({SW_T_CONV, 1, C, C, 3});
        t.push_back({SW_T_PROJ, 1, C, C, 1});              // P_i
    }
    t.push_back({SW_T_LN, 1, C, 0, 0});
    t.push_back({SW_T_CONV, 1, C, C, 3});
    sw_emit_tail(t, C, d.scale, d.upsampler);
    return t;
}

std::vector<SwStep> s2_tail_steps(const sr_swin2sr_desc &d) { return sw_tail_steps(s2_as_swinir(d)); }

int s2_geometry(const char *who, const sr_swin2sr_desc &d, int h, int w, int tail, SwGeom &g)
{
    const SwFamily f{SW_WIN, 4, 0, 0, SR_SWIN2SR_TRUNK_CAP, "SR_SWIN2SR_TRUNK_CAP", false};
    return sw_plan_geometry(who, f, d.n_feat, d.n_hidden, d.scale, s2_tail_steps(d), h, w, tail, g);
}

int s2_check_tables(const char *who, const sr_swin2sr_desc &d, const std::vector<SwTable> &tables, const float *const *h_w,
                    const float *const *h_b)
{
    const int C = d.n_feat;
    for (size_t k = 0; k < tables.size(); ++k) {
        if (tables[k].kind == SW_T_QKV) {
            for (int c = C; c < 2 * C; ++c)
                if (h_b[k][c] != 0.0f)
                    return sr_set_error(SR_ERR_UNSUPPORTED, "%s: table %zu: the k bias of a Swin2SR attention must be zero (q_bias, 0, v_bias), entry %d is %g",
                                        who, k, c - C, (double)h_b[k][c]);
        } else if (tables[k].kind == S2_T_LOGIT) {
            for (int n = 0; n < d.n_heads; ++n)
                if (!std::isfinite(h_w[k][n])) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: table %zu: logit_scale must be finite", who, k);
        }
    }
    return SR_OK;
}

void s2_cpb_table(const float *w1, const float *b1, const float *w2, int heads, float *table)
{
    const int side = 2 * SW_WIN - 1;
    auto coord = [](int delta) {                            // 8 delta / 7, then sign(v) log2(|v| + 1) / log2(8)
        const double v = 8.0 * (double)delta / (double)(SW_WIN - 1);
        const double g = std::log2(std::fabs(v) + 1.0) / 3.0;
        return v < 0.0 ? -g : (v > 0.0 ? g : 0.0);
    };
    std::vector<double> u(S2_CPB_HIDDEN);
    for (int t = 0; t < SW_REL; ++t) {
        const double cy = coord(t / side - (SW_WIN - 1)), cx = coord(t % side - (SW_WIN - 1));
        for (int i = 0; i < S2_CPB_HIDDEN; ++i) {
            const double a = (double)w1[2 * i] * cy + (double)w1[2 * i + 1] * cx + (double)b1[i];
            u[i] = a > 0.0 ? a : 0.0;
        }
        for (int hd = 0; hd < heads; ++hd) {
            double z = 0.0;
            for (int i = 0; i < S2_CPB_HIDDEN; ++i) z += (double)w2[(size_t)hd * S2_CPB_HIDDEN + i] * u[i];
            table[(size_t)t * heads + hd] = (float)(16.0 / (1.0 + std::exp(-z)));
        }
    }
}

void s2_logit_scale(const float *logit, int heads, float *scale)
{
    const double cap = std::log(100.0);
    for (int hd = 0; hd < heads; ++hd) scale[hd] = (float)std::exp(std::min((double)logit[hd], cap));
}

extern "C" {

int sr_swin2sr_plan(const sr_swin2sr_desc *desc, int h, int w, int tail, int *hp, int *wp, int *halo, int *n_tail_tiles, size_t *workspace_bytes)
{
    int rc = s2_check_desc("sr_swin2sr_plan", desc);
    if (rc) return rc;
    SwGeom g;
    if ((rc = s2_geometry("sr_swin2sr_plan", *desc, h, w, tail, g))) return rc;
    sw_write_plan(g, hp, wp, halo, n_tail_tiles, workspace_bytes);
    return SR_OK;
}

int sr_swin2sr_cpb_bias(const float *h_w1, const float *h_b1, const float *h_w2, const float *h_logit_scale, int n_heads, float *h_table,
                        float *h_scale)
{
    const char *who = "sr_swin2sr_cpb_bias";
    if (n_heads < 1 || n_heads > 256) return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d heads is outside 1 .. 256", who, n_heads);
    if (!h_table && !h_scale) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    if (h_table && (!h_w1 || !h_b1 || !h_w2)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    if (h_scale && !h_logit_scale) return sr_set_error(SR_ERR_INVALID_ARG, "%s: null argument", who);
    if (h_table) s2_cpb_table(h_w1, h_b1, h_w2, n_heads, h_table);
    if (h_scale) s2_logit_scale(h_logit_scale, n_heads, h_scale);
    return SR_OK;
}

}  // extern "C"
