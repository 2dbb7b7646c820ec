// sr_imresize_host.cpp -- the host side of MATLAB's bicubic imresize: the output size, one axis' weights and indices, and the
// plan (pass order, tap counts, tile geometry, table layout) with every refusal.  Pure host code: no device call, no context --
// sr_imresize.hip plans with imr_plan; tools/sanitize/imresize_driver.cpp runs this file under the sanitizers.  The definition
// is in include/sr_hip.h.  Every expression below is float64 and written in the order of that text (build with
// -ffp-contract=off).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "sr_imresize.h"

namespace {

constexpr double SCALE_MIN = 1.0 / 16.0, SCALE_MAX = 16.0;

double cubic(double x)
{
    x = std::fabs(x);
    if (x <= 1.0) return 1.5 * (x * x * x) - 2.5 * (x * x) + 1.0;
    if (x <= 2.0) return -0.5 * (x * x * x) + 2.5 * (x * x) - 4.0 * x + 2.0;
    return 0.0;
}

double triangle(double x)
{
    x = std::fabs(x);
    return x < 1.0 ? 1.0 - x : 0.0;
}

int check_scale(const char *scope, const char *axis, double scale)
{
    if (!(scale >= SCALE_MIN && scale <= SCALE_MAX))
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: the %s scale %.17g is outside [1/16, 16]", scope, axis, scale);
    return SR_OK;
}

}  // namespace

int imr_axis(const char *scope, int n_in, int n_out, double scale, int antialias, ImrAxis *a)
{
    if (n_in < 1 || n_out < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: sides must be >= 1 (got %d -> %d)", scope, n_in, n_out);
    const int rc = check_scale(scope, "axis", scale);
    if (rc) return rc;
    return imr_axis_kernel(scope, n_in, n_out, scale, antialias, IMR_CUBIC, true, a);
}

int imr_axis_kernel(const char *scope, int n_in, int n_out, double scale, int antialias, ImrKernel kernel, bool trim, ImrAxis *a)
{
    if (n_in < 1 || n_out < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: sides must be >= 1 (got %d -> %d)", scope, n_in, n_out);
    if (!(scale > 0.0)) return sr_set_error(SR_ERR_INVALID_ARG, "%s: the scale must be positive (got %.17g)", scope, scale);
    const bool tri = kernel == IMR_TRIANGLE;
    const double support = tri ? 2.0 : 4.0;
    if (std::ceil((double)n_in * scale) != (double)n_out && scale != (double)n_out / (double)n_in)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: %d -> %d is neither ceil(n * scale) nor scale = m / n for scale %.17g", scope, n_in,
                            n_out, scale);
    const bool shrink = antialias && scale < 1.0;
    const double kw = shrink ? support / scale : support;
    const int P = (int)std::ceil(kw) + 2;
    std::vector<double> w((size_t)n_out * P);
    std::vector<long long> left(n_out);
    for (int i = 0; i < n_out; ++i) {
        const double u = (double)(i + 1) / scale + 0.5 * (1.0 - 1.0 / scale);
        const double lf = std::floor(u - kw / 2.0);
        left[i] = (long long)lf;
        double *row = &w[(size_t)i * P];
        double sum = 0.0;
        for (int k = 0; k < P; ++k) {
            const double d = u - lf - (double)k;
            if (tri) row[k] = shrink ? scale * triangle(scale * d) : triangle(d);
            else row[k] = shrink ? scale * cubic(scale * d) : cubic(d);
            sum += row[k];
        }
        for (int k = 0; k < P; ++k) row[k] /= sum;
    }
    // taps that are zero for every output: dropped at both ends (at least one tap stays)
    int c0 = 0, c1 = P - 1;
    auto all_zero = [&](int k) {
        for (int i = 0; i < n_out; ++i)
            if (w[(size_t)i * P + k] != 0.0) return false;
        return true;
    };
    while (trim && c0 < c1 && all_zero(c0)) ++c0;
    while (trim && c1 > c0 && all_zero(c1)) --c1;
    const int taps = c1 - c0 + 1;
    a->n_in = n_in;
    a->n_out = n_out;
    a->taps = taps;
    a->scale = scale;
    a->w.resize((size_t)n_out * taps);
    a->idx.resize((size_t)n_out * taps);
    a->start.resize(n_out);
    for (int i = 0; i < n_out; ++i) {
        a->start[i] = (int32_t)(left[i] + c0);
        for (int k = 0; k < taps; ++k) {
            a->w[(size_t)i * taps + k] = w[(size_t)i * P + c0 + k];
            a->idx[(size_t)i * taps + k] = imr_reflect(left[i] + c0 + k, n_in);
        }
    }
    return SR_OK;
}

int imr_plan(const char *scope, int h, int w, int cn, double scale_y, double scale_x, int dh, int dw, int antialias, ImrAxis *ay,
             ImrAxis *ax, ImrPlan *p)
{
    if (h < 1 || w < 1 || dh < 1 || dw < 1)
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: sides must be >= 1 (got %d x %d -> %d x %d)", scope, h, w, dh, dw);
    if (cn != 1 && cn != 3 && cn != 4) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need 1, 3 or 4 channels (got %d)", scope, cn);
    int rc = check_scale(scope, "vertical", scale_y);
    if (rc) return rc;
    rc = check_scale(scope, "horizontal", scale_x);
    if (rc) return rc;
    rc = imr_axis(scope, h, dh, scale_y, antialias, ay);
    if (rc) return rc;
    rc = imr_axis(scope, w, dw, scale_x, antialias, ax);
    if (rc) return rc;
    *p = ImrPlan();
    p->order = scale_y <= scale_x ? 0 : 1;              // the smaller scale first; a tie: the vertical pass
    const ImrAxis &A = p->order == 0 ? *ay : *ax, &B = p->order == 0 ? *ax : *ay;
    // tile_b: wide enough that the apron of the second pass (taps - 1 positions) stays a small part of what the first pass
    // computes; tile_a: what the LDS budget then leaves
    int tile_b = B.scale < 1.0 ? 32 : 64, span = 0;
    for (;; tile_b /= 2) {
        span = (int)std::ceil((double)(tile_b - 1) / B.scale) + 2 + B.taps;
        if ((long long)span * cn <= IMR_LDS_DOUBLES || tile_b == 1) break;
    }
    for (int b0 = 0; b0 < B.n_out; b0 += tile_b) {     // the bound holds for the tables as they are
        const int b1 = std::min(b0 + tile_b, B.n_out);
        if ((long long)B.start[b1 - 1] + B.taps - B.start[b0] > span)
            return sr_set_error(SR_ERR_INVALID_ARG, "%s: internal: a tile of %d outputs spans more than %d inputs", scope, tile_b, span);
    }
    p->tile_b = tile_b;
    p->span_b = span;
    p->tile_a = std::max(1, std::min(IMR_TILE_A_MAX, IMR_LDS_DOUBLES / (span * cn)));
    p->tiles_a = ((long long)A.n_out + p->tile_a - 1) / p->tile_a;
    p->tiles_b = ((long long)B.n_out + p->tile_b - 1) / p->tile_b;
    if (p->tiles_a * p->tiles_b > 0x7fffffffLL)
        return sr_set_error(SR_ERR_SHAPE, "%s: too many tiles (%lld x %lld)", scope, p->tiles_a, p->tiles_b);
    p->lds_bytes = (size_t)p->tile_a * (size_t)span * (size_t)cn * sizeof(double);
    size_t off = 0;
    const ImrAxis *axes[2] = {ay, ax};
    for (int s = 0; s < 2; ++s) {
        const size_t n = (size_t)axes[s]->n_out * (size_t)axes[s]->taps;
        p->off_w[s] = off;
        off += up256(n * sizeof(double));
        p->off_idx[s] = off;
        off += up256(n * sizeof(int32_t));
        p->off_start[s] = off;
        off += up256((size_t)axes[s]->n_out * sizeof(int32_t));
    }
    p->total = off;
    return SR_OK;
}

extern "C" {

int sr_imresize_size(int n, double scale)
{
    if (n < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_imresize_size: n must be >= 1 (got %d)", n);
    const int rc = check_scale("sr_imresize_size", "axis", scale);
    if (rc) return rc;
    const double m = std::ceil((double)n * scale);
    if (!(m >= 1.0 && m <= (double)INT_MAX)) return sr_set_error(SR_ERR_SHAPE, "sr_imresize_size: %d * %.17g does not fit", n, scale);
    return (int)m;
}

int sr_imresize_weights(int n_in, int n_out, double scale, int antialias, int cap, int *taps, double *w, int32_t *idx)
{
    if (!taps || (w == nullptr) != (idx == nullptr))
        return sr_set_error(SR_ERR_INVALID_ARG, "sr_imresize_weights: taps is null, or only one of w and idx");
    ImrAxis a;
    const int rc = imr_axis("sr_imresize_weights", n_in, n_out, scale, antialias, &a);
    if (rc) return rc;
    *taps = a.taps;
    if (!w) return SR_OK;
    if (cap < a.taps) return sr_set_error(SR_ERR_INVALID_ARG, "sr_imresize_weights: room for %d taps, %d needed", cap, a.taps);
    memcpy(w, a.w.data(), a.w.size() * sizeof(double));
    memcpy(idx, a.idx.data(), a.idx.size() * sizeof(int32_t));
    return SR_OK;
}

int sr_imresize_plan(int h, int w, int cn, double scale_y, double scale_x, int dh, int dw, int antialias, int *order, int *taps_y,
                     int *taps_x, int *tile_h, int *tile_w, size_t *lds_bytes, size_t *scratch_bytes)
{
    ImrAxis ay, ax;
    ImrPlan p;
    const int rc = imr_plan("sr_imresize_plan", h, w, cn, scale_y, scale_x, dh, dw, antialias, &ay, &ax, &p);
    if (rc) return rc;
    if (order) *order = p.order;
    if (taps_y) *taps_y = ay.taps;
    if (taps_x) *taps_x = ax.taps;
    if (tile_h) *tile_h = p.order == 0 ? p.tile_a : p.tile_b;
    if (tile_w) *tile_w = p.order == 0 ? p.tile_b : p.tile_a;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    if (scratch_bytes) *scratch_bytes = p.total;
    return SR_OK;
}

}  // extern "C"
