// sr_deltae_host.cpp -- the host side of the colour difference: the plan (cropped size, launch, scratch layout and every
// refusal that depends on the arguments), the linearisation table, the float64 restatement of Lab and both formulas (the
// expressions of sr_deltae.h, which the kernels share) and the values read off the record: mean, rms, percentile, fraction.
// Pure host code: nothing here touches the device, so the unit also links into a stand-alone program
// (tools/sanitize/deltae_driver.cpp).  The definition is in include/sr_hip.h.
#include <algorithm>
#include <cmath>
#include <limits>

#include "sr_deltae.h"

namespace {

constexpr double DE_NAN = std::numeric_limits<double>::quiet_NaN();

// the record's count, or 0 with an error for a record nothing can be read from
uint64_t usable(const char *scope, const sr_delta_e_sums *s)
{
    if (!s) {
        sr_set_error(SR_ERR_INVALID_ARG, "%s: null record", scope);
        return 0;
    }
    if (s->count == 0) sr_set_error(SR_ERR_INVALID_ARG, "%s: the record holds no pixel", scope);
    return s->count;
}

bool hist_adds_up(const sr_delta_e_sums *s)
{
    uint64_t n = 0;
    for (int i = 0; i < SR_DELTA_E_BINS; ++i) {
        if (s->hist[i] > s->count - n) return false;
        n += s->hist[i];
    }
    return n == s->count;
}

}  // namespace

int delta_e_plan(const char *scope, int h, int w, int cn, int crop_border, int formula, DePlan *p)
{
    if (cn != 1 && cn != 3 && cn != 4)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: need 1 (gray), 3 (RGB) or 4 (RGBA) channels of u8 (got %d)", scope, cn);
    if (formula != SR_DELTA_E_2000 && formula != SR_DELTA_E_76)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: formula %d: only SR_DELTA_E_2000 (kL = kC = kH = 1) and SR_DELTA_E_76 under "
                            "D65 / 2 degrees are built (no CIE94, no CMC, no other weights or illuminants)", scope, formula);
    if (crop_border < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: crop_border must be >= 0 (got %d)", scope, crop_border);
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need h, w >= 1", scope);
    const long long lh = (long long)h - 2LL * crop_border, lw = (long long)w - 2LL * crop_border;
    if (lh < 1 || lw < 1)
        return sr_set_error(SR_ERR_SHAPE, "%s: image %dx%d with crop_border %d leaves %lldx%lld: both sides must be at least 1 "
                            "after the crop", scope, w, h, crop_border, std::max(lw, 0LL), std::max(lh, 0LL));
    p->ch = (int)lh;
    p->cw = (int)lw;
    p->count = (uint64_t)lh * (uint64_t)lw;
    if (p->count > (1ull << 40))        // a block's 32-bit histogram counters hold count / DE_MAX_BLOCKS pixels and a tile more
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %dx%d after the crop is more than 2^40 pixels", scope, p->cw, p->ch);
    p->tiles_x = (int)((lw + DE_TW - 1) / DE_TW);
    p->tiles = (long long)p->tiles_x * ((lh + DE_TH - 1) / DE_TH);
    p->blocks = (int)std::min<long long>(p->tiles, DE_MAX_BLOCKS);
    p->off_table = 0;
    p->off_hist = up256(DE_TABLE * sizeof(double));
    p->off_result = p->off_hist + up256(SR_DELTA_E_BINS * sizeof(uint64_t));
    p->off_part = p->off_result + up256(3 * sizeof(double));
    p->total = p->off_part + up256((size_t)p->blocks * 3 * sizeof(double));
    return SR_OK;
}

void delta_e_table(double *table)
{
    for (int c = 0; c < DE_TABLE; ++c) {
        const double v = (double)c / 255.0;
        table[c] = v > 0.04045 ? std::pow((v + 0.055) / 1.055, 2.4) : v / 12.92;
    }
}

extern "C" {

int sr_delta_e_plan(int h, int w, int cn, int crop_border, int formula, int *crop_h, int *crop_w, uint64_t *count, int *blocks,
                    size_t *scratch_bytes)
{
    DePlan p;
    const int rc = delta_e_plan("sr_delta_e_plan", h, w, cn, crop_border, formula, &p);
    if (rc) return rc;
    if (crop_h) *crop_h = p.ch;
    if (crop_w) *crop_w = p.cw;
    if (count) *count = p.count;
    if (blocks) *blocks = p.blocks;
    if (scratch_bytes) *scratch_bytes = p.total;
    return SR_OK;
}

int sr_delta_e_table(double *table256)
{
    if (!table256) return sr_set_error(SR_ERR_INVALID_ARG, "sr_delta_e_table: null table");
    delta_e_table(table256);
    return SR_OK;
}

int sr_delta_e_lab_u8(int r, int g, int b, double *lab3)
{
    if (!lab3) return sr_set_error(SR_ERR_INVALID_ARG, "sr_delta_e_lab_u8: null output");
    if ((r | g | b) < 0 || r > 255 || g > 255 || b > 255)
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_delta_e_lab_u8: bytes must be 0 .. 255 (got %d, %d, %d)", r, g, b);
    double table[DE_TABLE];
    delta_e_table(table);
    de_lab(table[r], table[g], table[b], lab3[0], lab3[1], lab3[2]);
    return SR_OK;
}

int sr_delta_e_pair(const double *lab1, const double *lab2, int formula, double *out)
{
    if (!lab1 || !lab2 || !out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_delta_e_pair: null argument");
    if (formula == SR_DELTA_E_2000) *out = de_2000(lab1[0], lab1[1], lab1[2], lab2[0], lab2[1], lab2[2]);
    else if (formula == SR_DELTA_E_76) *out = de_76(lab1[0], lab1[1], lab1[2], lab2[0], lab2[1], lab2[2]);
    else
        return sr_set_error(SR_ERR_UNSUPPORTED, "sr_delta_e_pair: formula %d: only SR_DELTA_E_2000 and SR_DELTA_E_76 are built",
                            formula);
    return SR_OK;
}

double sr_delta_e_mean(const sr_delta_e_sums *sums)
{
    const uint64_t n = usable("sr_delta_e_mean", sums);
    return n ? sums->sum / (double)n : DE_NAN;
}

double sr_delta_e_rms(const sr_delta_e_sums *sums)
{
    const uint64_t n = usable("sr_delta_e_rms", sums);
    return n ? std::sqrt(sums->sum2 / (double)n) : DE_NAN;
}

double sr_delta_e_percentile(const sr_delta_e_sums *sums, double p)
{
    const uint64_t n = usable("sr_delta_e_percentile", sums);
    if (!n) return DE_NAN;
    if (!(p > 0.0 && p <= 100.0)) {
        sr_set_error(SR_ERR_INVALID_ARG, "sr_delta_e_percentile: p must lie in (0, 100] (got %g)", p);
        return DE_NAN;
    }
    if (!hist_adds_up(sums)) {
        sr_set_error(SR_ERR_INVALID_ARG, "sr_delta_e_percentile: the histogram does not add up to count");
        return DE_NAN;
    }
    // k = max(1, ceil(p n / 100)) in exact integer arithmetic wherever p n / 100 is one: the long double product of two values
    // below 2^64 and 100 keeps 64 bits, and the correction steps settle the last unit
    long double q = std::ceil((long double)p * (long double)n / 100.0L);
    uint64_t k = q < 1.0L ? 1 : (q >= (long double)n ? n : (uint64_t)q);
    while (k > 1 && (long double)(k - 1) * 100.0L >= (long double)p * (long double)n) --k;
    while (k < n && (long double)k * 100.0L < (long double)p * (long double)n) ++k;
    uint64_t cum = 0;
    for (int j = 0; j < SR_DELTA_E_BINS; ++j) {
        cum += sums->hist[j];
        if (cum >= k) return (double)j / 16.0;
    }
    return (double)(SR_DELTA_E_BINS - 1) / 16.0;        // not reached: the histogram adds up to n >= k
}

int sr_delta_e_fraction_at_least(const sr_delta_e_sums *sums, double t, double *fraction)
{
    if (!fraction) return sr_set_error(SR_ERR_INVALID_ARG, "sr_delta_e_fraction_at_least: null output");
    const uint64_t n = usable("sr_delta_e_fraction_at_least", sums);
    if (!n) return SR_ERR_INVALID_ARG;
    const double s = 16.0 * t;
    if (!(t >= 0.0 && s < (double)SR_DELTA_E_BINS) || s != std::floor(s))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_delta_e_fraction_at_least: the threshold must be a multiple of 1/16 in [0, %d) "
                            "(got %g): the histogram's bin edges are the only exact thresholds", SR_DELTA_E_BINS / 16, t);
    if (!hist_adds_up(sums))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_delta_e_fraction_at_least: the histogram does not add up to count");
    uint64_t above = 0;
    for (int j = (int)s; j < SR_DELTA_E_BINS; ++j) above += sums->hist[j];
    *fraction = (double)above / (double)n;
    return SR_OK;
}

}  // extern "C"
