// sr_haarpsi_host.cpp -- the host side of HaarPSI: the plan (cropped size, sample map, launch, scratch layout and every refusal
// that depends on the arguments), the values read off a record, and the float64 restatement of the definition on host memory
// (direct window sums over the pooled integer planes, then the per-sample expressions of sr_haarpsi.h, which the kernel shares).
// Pure host code: nothing here touches the device, so the unit also links into a stand-alone program
// (tools/sanitize/haarpsi_driver.cpp).  The definition is in include/sr_hip.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <vector>

#include "sr_haarpsi.h"

namespace {

constexpr double HP_NAN = std::numeric_limits<double>::quiet_NaN();

// the three pooled integer planes of one image: plane[k][i * mw + j]
template <int CN, bool SUB>
void pool_planes(const unsigned char *img, long long stride, const HpPlan &p, int o, std::vector<int> *plane)
{
    for (int i = 0; i < p.mh; ++i)
        for (int j = 0; j < p.mw; ++j) {
            const size_t at = (size_t)i * (size_t)p.mw + (size_t)j;
            hp_pool<CN, SUB>(img, stride, p.ch, p.cw, o, i, j, plane[0][at], plane[1][at], plane[2][at]);
        }
}

struct Plane {
    const int *v;
    int mh, mw;
    // the sum over rows r0 .. r1 and columns c0 .. c1 (inclusive), zero outside the plane
    long long box(long long r0, long long r1, long long c0, long long c1) const
    {
        r0 = std::max(r0, 0LL);
        c0 = std::max(c0, 0LL);
        r1 = std::min(r1, (long long)mh - 1);
        c1 = std::min(c1, (long long)mw - 1);
        long long s = 0;
        for (long long r = r0; r <= r1; ++r)
            for (long long c = c0; c <= c1; ++c) s += v[(size_t)r * (size_t)mw + (size_t)c];
        return s;
    }
};

void haar_sums(const Plane &y, long long ci, long long cj, int (&v)[2][3])
{
    for (int s = 0; s < 3; ++s) {
        const long long hf = 1LL << s;
        v[0][s] = (int)(y.box(ci - hf + 1, ci, cj - hf + 1, cj + hf) - y.box(ci + 1, ci + hf, cj - hf + 1, cj + hf));
        v[1][s] = (int)(y.box(ci - hf + 1, ci + hf, cj - hf + 1, cj) - y.box(ci - hf + 1, ci + hf, cj + 1, cj + hf));
    }
}

template <int CN, bool SUB>
int host_run(const unsigned char *a, long long sa, const unsigned char *b, long long sb, const HpPlan &p, int o,
             sr_haarpsi_sums *out)
{
    constexpr bool COLOUR = CN >= 3;
    std::vector<int> pa[3], pb[3];
    try {
        for (int k = 0; k < 3; ++k) {
            pa[k].assign((size_t)p.count, 0);
            pb[k].assign((size_t)p.count, 0);
        }
    } catch (const std::bad_alloc &) {
        return sr_set_error(SR_ERR_OOM, "sr_haarpsi_host_u8: out of host memory for %dx%d planes", p.mw, p.mh);
    }
    pool_planes<CN, SUB>(a, sa, p, o, pa);
    pool_planes<CN, SUB>(b, sb, p, o, pb);
    const Plane ya{pa[0].data(), p.mh, p.mw}, yb{pb[0].data(), p.mh, p.mw};
    const Plane ia{pa[1].data(), p.mh, p.mw}, ib{pb[1].data(), p.mh, p.mw};
    const Plane qa{pa[2].data(), p.mh, p.mw}, qb{pb[2].data(), p.mh, p.mw};
    const double div = SUB ? 4000.0 : 1000.0;
    double num[3] = {0.0, 0.0, 0.0}, den[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < p.mh; ++i)
        for (int j = 0; j < p.mw; ++j) {
            const long long ci = (long long)i - o, cj = (long long)j - o;
            int va[2][3], vb[2][3];
            haar_sums(ya, ci, cj, va);
            haar_sums(yb, ci, cj, vb);
            int sia = 0, sqa = 0, sib = 0, sqb = 0;
            if (COLOUR) {
                sia = (int)ia.box(ci, ci + 1, cj, cj + 1);
                sqa = (int)qa.box(ci, ci + 1, cj, cj + 1);
                sib = (int)ib.box(ci, ci + 1, cj, cj + 1);
                sqb = (int)qb.box(ci, ci + 1, cj, cj + 1);
            }
            double n[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0};
            hp_sample<COLOUR>(va, vb, sia, sqa, sib, sqb, div, n, d);
            for (int k = 0; k < 3; ++k) {
                num[k] += n[k];
                den[k] += d[k];
            }
        }
    for (int k = 0; k < 3; ++k) {
        out->num[k] = num[k];
        out->den[k] = den[k];
    }
    out->channels = p.channels;
    out->reserved = 0;
    out->count = p.count;
    return SR_OK;
}

}  // namespace

int haarpsi_plan(const char *scope, int h, int w, int cn, int crop_border, int subsample, int convention, HpPlan *p)
{
    if (cn != 1 && cn != 3 && cn != 4)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: need 1 (gray), 3 (RGB) or 4 (RGBA) channels of u8 (got %d)", scope, cn);
    if (subsample != 0 && subsample != 1)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: subsample must be 0 or 1 (got %d)", scope, subsample);
    if (convention != SR_HAARPSI_MATLAB && convention != SR_HAARPSI_PYTHON)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: convention %d: only SR_HAARPSI_MATLAB (conv2 'same') and SR_HAARPSI_PYTHON "
                            "(scipy convolve2d 'same') are built", scope, convention);
    if (crop_border < 0) return sr_set_error(SR_ERR_INVALID_ARG, "%s: crop_border must be >= 0 (got %d)", scope, crop_border);
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need h, w >= 1", scope);
    const long long lh = (long long)h - 2LL * crop_border, lw = (long long)w - 2LL * crop_border;
    if (lh < HP_MIN_SIDE || lw < HP_MIN_SIDE)
        return sr_set_error(SR_ERR_SHAPE, "%s: image %dx%d with crop_border %d leaves %lldx%lld: both sides must be at least %d "
                            "after the crop", scope, w, h, crop_border, std::max(lw, 0LL), std::max(lh, 0LL), HP_MIN_SIDE);
    memset(p, 0, sizeof(*p));
    p->ch = (int)lh;
    p->cw = (int)lw;
    p->mh = subsample ? (int)((lh + 1) / 2) : (int)lh;
    p->mw = subsample ? (int)((lw + 1) / 2) : (int)lw;
    p->channels = cn == 1 ? 2 : 3;
    p->count = (uint64_t)p->mh * (uint64_t)p->mw;
    p->tiles_x = (int)(((long long)p->mw + HP_TW - 1) / HP_TW);
    p->tiles_y = (int)(((long long)p->mh + HP_TH - 1) / HP_TH);
    const long long tiles = (long long)p->tiles_x * (long long)p->tiles_y;
    if (tiles > 0x7FFFFFFFLL)
        return sr_set_error(SR_ERR_SHAPE, "%s: %dx%d after the crop is more than one launch covers", scope, p->cw, p->ch);
    // the per-block partials of the six sums and the two ping-pong buffers of reduce_partials
    const size_t part = up256((size_t)tiles * HP_COMP * sizeof(double));
    const size_t buf = up256(((size_t)tiles / 1024 + 2) * HP_COMP * sizeof(double));
    p->off_part = 0;
    p->off_buf0 = part;
    p->off_buf1 = part + buf;
    p->total = part + 2 * buf;
    return SR_OK;
}

extern "C" {

int sr_haarpsi_plan(int h, int w, int cn, int crop_border, int subsample, int convention, int *map_h, int *map_w, uint64_t *count,
                    int *blocks, size_t *scratch_bytes)
{
    HpPlan p;
    const int rc = haarpsi_plan("sr_haarpsi_plan", h, w, cn, crop_border, subsample, convention, &p);
    if (rc) return rc;
    if (map_h) *map_h = p.mh;
    if (map_w) *map_w = p.mw;
    if (count) *count = p.count;
    if (blocks) *blocks = p.tiles_x * p.tiles_y;
    if (scratch_bytes) *scratch_bytes = p.total;
    return SR_OK;
}

double sr_haarpsi_cell_value(double num, double den)
{
    if (den == 0.0) return HP_NAN;
    const double x = num / den;
    const double l = std::log(x / (1.0 - x)) / HP_ALPHA;
    return l * l;
}

double sr_haarpsi_value(const sr_haarpsi_sums *sums)
{
    if (!sums || (sums->channels != 2 && sums->channels != 3)) {
        sr_set_error(SR_ERR_INVALID_ARG, "sr_haarpsi_value: need a record of 2 or 3 channels");
        return HP_NAN;
    }
    double num = 0.0, den = 0.0;
    for (int k = 0; k < sums->channels; ++k) {
        num += sums->num[k];
        den += sums->den[k];
    }
    return sr_haarpsi_cell_value(num, den);
}

int sr_haarpsi_host_u8(const uint8_t *a, int64_t stride_a, const uint8_t *b, int64_t stride_b, int h, int w, int cn,
                       int crop_border, int subsample, int convention, sr_haarpsi_sums *out)
{
    if (!a || !b || !out) return sr_set_error(SR_ERR_INVALID_ARG, "sr_haarpsi_host_u8: null argument");
    HpPlan p;
    const int rc = haarpsi_plan("sr_haarpsi_host_u8", h, w, cn, crop_border, subsample, convention, &p);
    if (rc) return rc;
    const int64_t min_stride = (int64_t)w * cn;
    if (stride_a < min_stride || stride_b < min_stride)
        return sr_set_error(SR_ERR_SHAPE, "sr_haarpsi_host_u8: stride smaller than a row");
    const unsigned char *pa = a + (size_t)crop_border * (size_t)stride_a + (size_t)crop_border * (size_t)cn;
    const unsigned char *pb = b + (size_t)crop_border * (size_t)stride_b + (size_t)crop_border * (size_t)cn;
    const int o = convention == SR_HAARPSI_PYTHON ? 1 : 0;
    const long long sa = stride_a, sb = stride_b;
    if (subsample) {
        if (cn == 1) return host_run<1, true>(pa, sa, pb, sb, p, o, out);
        if (cn == 3) return host_run<3, true>(pa, sa, pb, sb, p, o, out);
        return host_run<4, true>(pa, sa, pb, sb, p, o, out);
    }
    if (cn == 1) return host_run<1, false>(pa, sa, pb, sb, p, o, out);
    if (cn == 3) return host_run<3, false>(pa, sa, pb, sb, p, o, out);
    return host_run<4, false>(pa, sa, pb, sb, p, o, out);
}

}  // extern "C"
