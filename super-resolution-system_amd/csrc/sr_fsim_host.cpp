// sr_fsim_host.cpp -- the host side of FSIM / FSIMc: F, the pooled size and the workspace layout (fsim_plan: every shape
// refusal), the eight filter planes of the phase congruency with EM_n, S2 and Sij, the twiddle tables of the dense transform
// and the value.  Pure host code: nothing here touches the device, so the unit also links into a stand-alone program
// (tools/sanitize/fsim_driver.cpp).  The definition is in include/sr_hip.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "sr_fsim.h"

namespace {

constexpr double PI = 3.14159265358979323846;

// the centred frequency of index i of an ifftshifted axis of length n (DC at i = 0)
double axis_freq(int i, int n)
{
    const int half = n / 2;                 // (n - 1) / 2 for an odd n
    const int k = (i + half) % n - half;
    return (n & 1) ? (double)k / (double)(n - 1) : (double)k / (double)n;
}

int side_bounds(const char *scope, int rows, int cols)
{
    if (rows < FSIM_MIN_SIDE || cols < FSIM_MIN_SIDE)
        return sr_set_error(SR_ERR_SHAPE, "%s: plane %dx%d: both sides must be at least %d", scope, cols, rows, FSIM_MIN_SIDE);
    if (rows > FSIM_MAX_SIDE || cols > FSIM_MAX_SIDE)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: pooled plane %dx%d: a side above %d is not supported (the transform is dense)",
                            scope, cols, rows, FSIM_MAX_SIDE);
    return SR_OK;
}

void layout(FsimPlan *p)
{
    const size_t n = p->n, dbl = up256(n * sizeof(double)), cpx = up256(n * 2 * sizeof(double));
    size_t off = 0;
    auto take = [&off](size_t bytes) {
        const size_t at = off;
        off += up256(bytes);
        return at;
    };
    p->off_pool = take(6 * n * sizeof(int64_t));
    p->off_filt = take(8 * n * sizeof(double));
    p->off_tw_r = take((size_t)p->rows * 2 * sizeof(double));
    p->off_tw_c = take((size_t)p->cols * 2 * sizeof(double));
    p->off_plane = take(dbl);
    p->off_spec = take(cpx);
    p->off_half = take(4 * n * 2 * sizeof(double));
    p->off_eo = take(4 * n * 2 * sizeof(double));
    p->off_pc = take(2 * n * sizeof(double));
    p->off_energy_all = take(dbl);
    p->off_an_all = take(dbl);
    p->off_energy = take(dbl);
    p->off_e2 = take(dbl);
    p->off_hist = take(2 * 256 * sizeof(uint32_t) + 64);
    p->off_med = take(2 * 8 * sizeof(double));
    p->score_blocks = (n + FSIM_THREADS - 1) / FSIM_THREADS;
    p->off_part = take(p->score_blocks * 3 * sizeof(double));
    const size_t buf = (p->score_blocks / 1024 + 2) * 3 * sizeof(double);
    p->off_buf0 = take(buf);
    p->off_buf1 = take(buf);
    p->total = off;
}

}  // namespace

int fsim_auto_f(int h, int w)
{
    // floor(m / 256 + 0.5) = (2 m + 256) / 512 in integers
    const long long m = std::min(h, w);
    return (int)std::max(1LL, (2 * m + 256) / 512);
}

int fsim_plan(const char *scope, int h, int w, int cn, int F, FsimPlan *p)
{
    if (cn != 1 && cn != 3 && cn != 4) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need 1, 3 or 4 channels (got %d)", scope, cn);
    if (h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "%s: need h, w >= 1", scope);
    const bool own = F == 0;
    if (own) {
        if (h < FSIM_MIN_SIDE || w < FSIM_MIN_SIDE)
            return sr_set_error(SR_ERR_SHAPE, "%s: image %dx%d: both sides must be at least %d", scope, w, h, FSIM_MIN_SIDE);
        F = fsim_auto_f(h, w);
        if (F > FSIM_MAX_F)
            return sr_set_error(SR_ERR_UNSUPPORTED, "%s: image %dx%d pools by F = %d: F above %d is not supported", scope, w, h, F,
                                FSIM_MAX_F);
    } else if (F < 1 || F > FSIM_MAX_F) {
        return sr_set_error(SR_ERR_INVALID_ARG, "%s: F must be 1 .. %d (got %d)", scope, FSIM_MAX_F, F);
    }
    memset(p, 0, sizeof(*p));
    p->h = h;
    p->w = w;
    p->cn = cn;
    p->F = F;
    p->rows = (int)(((long long)h + F - 1) / F);
    p->cols = (int)(((long long)w + F - 1) / F);
    if (own && (p->rows > FSIM_MAX_SIDE || p->cols > FSIM_MAX_SIDE))
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: image %dx%d pools (F = %d) to %dx%d: a pooled side above %d is not supported "
                            "(the transform is dense)", scope, w, h, F, p->cols, p->rows, FSIM_MAX_SIDE);
    p->n = (size_t)p->rows * (size_t)p->cols;
    const int out = fsim_pool_out(F);
    p->pool_gx = (p->cols + out - 1) / out;
    if (p->rows > 65535)
        return sr_set_error(SR_ERR_UNSUPPORTED, "%s: %d pooled rows are more than one launch covers (65535)", scope, p->rows);
    layout(p);
    return SR_OK;
}

int fsim_plan_plane(const char *scope, int rows, int cols, FsimPlan *p)
{
    const int rc = side_bounds(scope, rows, cols);
    if (rc) return rc;
    return fsim_plan(scope, rows, cols, 1, 1, p);
}

void fsim_filters(int rows, int cols, double *log_gabor, double *spread, double *em, double *s2, double *sij)
{
    const size_t n = (size_t)rows * (size_t)cols;
    std::vector<double> lg_own, sp_own;
    if (!log_gabor) {
        lg_own.resize(4 * n);
        log_gabor = lg_own.data();
    }
    if (!spread) {
        sp_own.resize(4 * n);
        spread = sp_own.data();
    }
    const double theta_sigma = PI / 4.0 / 1.2, lg_den = 2.0 * std::log(0.55) * std::log(0.55);
    for (int r = 0; r < rows; ++r) {
        const double y = axis_freq(r, rows);
        for (int c = 0; c < cols; ++c) {
            const double x = axis_freq(c, cols);
            const size_t i = (size_t)r * cols + c;
            const double r0 = std::sqrt(x * x + y * y);
            const double radius = i == 0 ? 1.0 : r0;
            const double lp = 1.0 / (1.0 + std::pow(r0 / 0.45, 30.0));
            for (int s = 0; s < FSIM_SCALES; ++s) {
                const double fo = 1.0 / (6.0 * (double)(1 << s));
                const double l = std::log(radius / fo);
                log_gabor[s * n + i] = i == 0 ? 0.0 : std::exp(-(l * l) / lg_den) * lp;
            }
            const double theta = std::atan2(-y, x), st = std::sin(theta), ct = std::cos(theta);
            for (int o = 0; o < FSIM_ORIENTS; ++o) {
                const double angl = (double)o * PI / 4.0;
                const double ds = st * std::cos(angl) - ct * std::sin(angl), dc = ct * std::cos(angl) + st * std::sin(angl);
                const double dt = std::fabs(std::atan2(ds, dc));
                spread[o * n + i] = std::exp(-(dt * dt) / (2.0 * theta_sigma * theta_sigma));
            }
        }
    }
    if (!em && !s2 && !sij) return;
    // g(u) = (f(u) + f(-u)) / 2 is the spectrum of real(ifft2(f)); Parseval turns the pixel sums of a_s a_t into sums over u
    for (int o = 0; o < FSIM_ORIENTS; ++o) {
        long double e = 0.0L, a2 = 0.0L, aij = 0.0L;
        const double *sp = spread + o * n;
        for (int r = 0; r < rows; ++r) {
            const int rm = (rows - r) % rows;
            for (int c = 0; c < cols; ++c) {
                const size_t i = (size_t)r * cols + c, m = (size_t)rm * cols + (size_t)((cols - c) % cols);
                double g[FSIM_SCALES];
                for (int s = 0; s < FSIM_SCALES; ++s) g[s] = (log_gabor[s * n + i] * sp[i] + log_gabor[s * n + m] * sp[m]) / 2.0;
                const double f0 = log_gabor[i] * sp[i];
                e += (long double)(f0 * f0);
                for (int s = 0; s < FSIM_SCALES; ++s) {
                    a2 += (long double)(g[s] * g[s]);
                    for (int t = s + 1; t < FSIM_SCALES; ++t) aij += (long double)(g[s] * g[t]);
                }
            }
        }
        if (em) em[o] = (double)e;
        if (s2) s2[o] = (double)a2;
        if (sij) sij[o] = (double)aij;
    }
}

void fsim_twiddles(int n, double *tw)
{
    // the angle's index is an integer below n: long double keeps the argument's error far below a float64 rounding
    const long double step = 2.0L * 3.14159265358979323846264338327950288L / (long double)n;
    for (int j = 0; j < n; ++j) {
        tw[2 * j] = (double)cosl(step * (long double)j);
        tw[2 * j + 1] = (double)-sinl(step * (long double)j);
    }
}

extern "C" {

int sr_fsim_plan(int h, int w, int cn, int *F, int *rows, int *cols, size_t *workspace_bytes)
{
    FsimPlan p;
    const int rc = fsim_plan("sr_fsim_plan", h, w, cn, 0, &p);
    if (rc) return rc;
    if (F) *F = p.F;
    if (rows) *rows = p.rows;
    if (cols) *cols = p.cols;
    if (workspace_bytes) *workspace_bytes = p.total;
    return SR_OK;
}

int sr_fsim_filters(int rows, int cols, double *log_gabor, double *spread, double *em, double *s2, double *sij)
{
    const int rc = side_bounds("sr_fsim_filters", rows, cols);
    if (rc) return rc;
    fsim_filters(rows, cols, log_gabor, spread, em, s2, sij);
    return SR_OK;
}

int sr_fsim_value(const sr_fsim_sums *sums, double *fsim, double *fsimc)
{
    if (!sums) return sr_set_error(SR_ERR_INVALID_ARG, "sr_fsim_value: null record");
    if (fsim) *fsim = sums->sum_s / sums->sum_pcm;          // 0 / 0 (a flat pair) is NaN, as in MATLAB
    if (fsimc) *fsimc = sums->sum_sc / sums->sum_pcm;
    return SR_OK;
}

double sr_fsim_chroma_weight(double s_i, double s_q) { return fsim_chroma_weight(s_i, s_q); }

}  // extern "C"
