// sr_vif_host.cpp -- the host side of VIF and GMSD: sizes, launches and scratch layouts (vif_plan, gmsd_plan: every shape
// refusal of both metrics), the windows of VIF's four scales and the two value formulas.  Pure host code: nothing here touches
// the device, so the unit also links into a stand-alone program (tools/sanitize/vif_gmsd_driver.cpp).  The definitions are in
// include/sr_hip.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "sr_vif.h"

namespace {

// what both metrics refuse alike; the cropped size comes back in *ch, *cw
int plane_args(const char *scope, int h, int w, int cn, int crop_border, int mode, int min_side, int *ch, int *cw)
{
    if (cn != 1 && cn != 3) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need 1 or 3 channels (got %d)", scope, cn);
    if (mode != SR_BENCH_CHANNELS && mode != SR_BENCH_Y && mode != SR_BENCH_Y_ROUND)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: unknown mode %d", scope, mode);
    if (mode != SR_BENCH_CHANNELS && cn != 3)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: the Y modes need 3 channels (RGB), got %d", scope, cn);
    if (mode == SR_BENCH_CHANNELS && cn != 1)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: SR_BENCH_CHANNELS takes one gray plane (cn = 1), got %d channels: use a Y mode",
                            scope, cn);
    if (crop_border < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: crop_border must be >= 0 (got %d)", scope, crop_border);
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need h, w >= 1", scope);
    const long long lh = (long long)h - 2LL * crop_border, lw = (long long)w - 2LL * crop_border;
    if (lh < min_side || lw < min_side)
        return sr_set_error(SR_ERR_SHAPE, "%s: image %dx%d with crop_border %d leaves %lldx%lld: both sides must be at least %d "
                            "after the crop", scope, w, h, crop_border, std::max(lw, 0LL), std::max(lh, 0LL), min_side);
    *ch = (int)lh;
    *cw = (int)lw;
    return SR_OK;
}

// Chunks of at most VIF_ROWS rows; a small plane takes shorter ones (down to VIF_ROWS_MIN) until it has VIF_BLOCKS blocks.
// The cut depends on the size alone, never on the device: equal bits everywhere.
void cut_rows(int rows_total, int gy, VifLaunch *l)
{
    int rows = VIF_ROWS;
    const long long total = rows_total;
    while (rows > VIF_ROWS_MIN && ((total + rows - 1) / rows) * gy < VIF_BLOCKS) rows /= 2;
    const long long n = (total + rows - 1) / rows;
    l->step = (int)((total + n - 1) / n);
    l->gx = (int)((total + l->step - 1) / l->step);
    l->gy = gy;
}

int too_wide(const char *scope, int cw)
{
    return sr_set_error(SR_ERR_SHAPE, "%s: %d columns after the crop are more than one launch covers (%d)", scope, cw,
                        VIF_GRID_Y * vif_stats_out(VIF_TX_U8, vif_taps(0)) + vif_taps(0) - 1);
}

// the per-block partials of a two-component sum and the two ping-pong buffers of its reduction, from byte offset off on
void partials_layout(size_t off, size_t nblk, size_t *off_part, size_t *off_buf0, size_t *off_buf1, size_t *end)
{
    const size_t part = up256(nblk * 2 * sizeof(double)), buf = up256((nblk / 1024 + 2) * 2 * sizeof(double));
    *off_part = off;
    *off_buf0 = off + part;
    *off_buf1 = off + part + buf;
    *end = off + part + 2 * buf;
}

}  // namespace

int vif_plan(const char *scope, int h, int w, int cn, int crop_border, int mode, VifPlan *p)
{
    int ch = 0, cw = 0;
    const int rc = plane_args(scope, h, w, cn, crop_border, mode, VIF_MIN_SIDE, &ch, &cw);
    if (rc) return rc;
    memset(p, 0, sizeof(*p));
    p->ch = ch;
    p->cw = cw;
    size_t off = 0;
    for (int s = 0; s < VIF_SCALES; ++s) {
        VifScale &v = p->s[s];
        v.n = vif_taps(s);
        if (s == 0) {
            v.h = ch;
            v.w = cw;
        } else {   // the scale before, filtered with THIS scale's window over the valid region, every second sample from 0
            const VifScale &u = p->s[s - 1];
            v.h = (u.h - (v.n - 1) + 1) / 2;
            v.w = (u.w - (v.n - 1) + 1) / 2;
            v.down.tx = s == 1 ? VIF_TX_U8 : VIF_TX_F64;
            const int dout = vif_down_out(v.down.tx, v.n);
            const long long dgy = ((long long)v.w + dout - 1) / dout;
            if (dgy > VIF_GRID_Y) return too_wide(scope, cw);
            cut_rows(v.h, (int)dgy, &v.down);
            v.off_x = off;
            off += up256((size_t)v.h * (size_t)v.w * sizeof(double));
            v.off_y = off;
            off += up256((size_t)v.h * (size_t)v.w * sizeof(double));
        }
        v.mh = v.h - (v.n - 1);
        v.mw = v.w - (v.n - 1);
        v.count = (uint64_t)v.mh * (uint64_t)v.mw;
        v.stats.tx = s == 0 ? VIF_TX_U8 : VIF_TX_F64;
        const int out = vif_stats_out(v.stats.tx, v.n);
        const long long gy = ((long long)v.mw + out - 1) / out;
        if (gy > VIF_GRID_Y) return too_wide(scope, cw);
        cut_rows(v.mh, (int)gy, &v.stats);
        p->nblk = std::max(p->nblk, (size_t)v.stats.gx * (size_t)v.stats.gy);
    }
    partials_layout(off, p->nblk, &p->off_part, &p->off_buf0, &p->off_buf1, &p->total);
    return SR_OK;
}

void vif_window(int s, double *taps)
{
    const int n = vif_taps(s);
    const double sd = (double)n / 5.0, c = (double)(n - 1) / 2.0;
    double sum = 0.0;
    for (int k = 0; k < n; ++k) {
        const double r = (double)k - c;
        taps[k] = std::exp(-(r * r) / (2.0 * sd * sd));
        sum += taps[k];
    }
    for (int k = 0; k < n; ++k) taps[k] /= sum;
}

int gmsd_plan(const char *scope, int h, int w, int cn, int crop_border, int mode, GmsdPlan *p)
{
    int ch = 0, cw = 0;
    const int rc = plane_args(scope, h, w, cn, crop_border, mode, GMSD_MIN_SIDE, &ch, &cw);
    if (rc) return rc;
    memset(p, 0, sizeof(*p));
    p->ch = ch;
    p->cw = cw;
    p->h2 = ch / 2 + (ch & 1);
    p->w2 = cw / 2 + (cw & 1);
    p->count = (uint64_t)p->h2 * (uint64_t)p->w2;
    p->tiles_x = (p->w2 + GMSD_TW - 1) / GMSD_TW;
    p->tiles_y = (p->h2 + GMSD_TH - 1) / GMSD_TH;
    const long long tiles = (long long)p->tiles_x * (long long)p->tiles_y;
    if (tiles > 0x7FFFFFFFLL)
        return sr_set_error(SR_ERR_SHAPE, "%s: %dx%d after the crop is more than one launch covers", scope, cw, ch);
    partials_layout(0, (size_t)tiles, &p->off_part, &p->off_buf0, &p->off_buf1, &p->total);
    return SR_OK;
}

extern "C" {

int sr_vif_plan(int h, int w, int cn, int crop_border, int mode, int *scale_h, int *scale_w, uint64_t *counts, size_t *scratch_bytes)
{
    VifPlan p;
    const int rc = vif_plan("sr_vif_plan", h, w, cn, crop_border, mode, &p);
    if (rc) return rc;
    for (int s = 0; s < VIF_SCALES; ++s) {
        if (scale_h) scale_h[s] = p.s[s].h;
        if (scale_w) scale_w[s] = p.s[s].w;
        if (counts) counts[s] = p.s[s].count;
    }
    if (scratch_bytes) *scratch_bytes = p.total;
    return SR_OK;
}

int sr_vif_window(int scale, double *taps)
{
    if (scale < 1 || scale > VIF_SCALES) return sr_set_error(SR_ERR_INVALID_ARG, "sr_vif_window: scale must be 1 .. %d (got %d)", VIF_SCALES, scale);
    if (!taps) return sr_set_error(SR_ERR_INVALID_ARG, "sr_vif_window: null taps");
    vif_window(scale - 1, taps);
    return SR_OK;
}

double sr_vif_value(const sr_vif_scale *out, int scales)
{
    if (!out || scales != VIF_SCALES) {
        sr_set_error(SR_ERR_INVALID_ARG, "sr_vif_value: need the %d scale records of sr_vif_u8", VIF_SCALES);
        return std::numeric_limits<double>::quiet_NaN();
    }
    double num = 0.0, den = 0.0;
    for (int s = 0; s < scales; ++s) {
        num += out[s].num;
        den += out[s].den;
    }
    return num / den;       // 0 / 0 (a flat reference) is NaN, as in MATLAB
}

int sr_gmsd_plan(int h, int w, int cn, int crop_border, int mode, int *map_h, int *map_w, uint64_t *count, size_t *scratch_bytes)
{
    GmsdPlan p;
    const int rc = gmsd_plan("sr_gmsd_plan", h, w, cn, crop_border, mode, &p);
    if (rc) return rc;
    if (map_h) *map_h = p.h2;
    if (map_w) *map_w = p.w2;
    if (count) *count = p.count;
    if (scratch_bytes) *scratch_bytes = p.total;
    return SR_OK;
}

double sr_gmsd_value(const sr_gmsd_sums *sums)
{
    if (!sums || sums->count < 2) {
        sr_set_error(SR_ERR_INVALID_ARG, "sr_gmsd_value: need a record of at least 2 samples");
        return std::numeric_limits<double>::quiet_NaN();
    }
    const double n = (double)sums->count;
    const double var = (sums->sum_d2 - sums->sum_d * sums->sum_d / n) / (n - 1.0);
    return var > 0.0 ? std::sqrt(var) : 0.0;
}

}  // extern "C"
