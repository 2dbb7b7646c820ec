// sr_brisque_host.cpp -- the host side of BRISQUE: the plan, the GGD / AGGD features of the two scale records, the feature
// scaler and the RBF epsilon-SVR.  Pure host code: no device call, no context -- sr_brisque.hip plans with bq_plan;
// tools/sanitize/brisque_driver.cpp runs this file under the sanitizers.  The definition is in include/sr_hip.h; the
// crop refusals, the Gamma-ratio table with its argmin and the AGGD fit are sr_mscn.h's, shared with NIQE.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "sr_mscn.h"

namespace {

constexpr int F = NQ_FEAT;

// X_0: [alpha, s2]
void ggd_fit(const sr_niqe_moments &m, double n, double *o)
{
    const double nan = std::nan("");
    o[0] = o[1] = nan;
    if (!(m.sabs > 0.0)) return;
    const double s2 = (m.ssq_neg + m.ssq_pos) / n, E = m.sabs / n;
    const double rho = s2 / (E * E);
    if (!(rho == rho)) return;
    const std::vector<double> &tab = nq_gam_table().rinv;
    int best = 0;
    double bd = std::fabs(tab[0] - rho);
    for (int t = 1; t < NQ_GAM_N; ++t) {
        const double d = std::fabs(tab[t] - rho);
        if (d < bd) {
            bd = d;
            best = t;
        }
    }
    o[0] = nq_gam_at(best);
    o[1] = s2;
}

// a shift: [alpha, mean, ls^2, rs^2] from sr_mscn.h's fit (shared with NIQE)
void aggd_fit(const sr_niqe_moments &m, double n, double *o)
{
    const double nan = std::nan("");
    o[0] = o[1] = o[2] = o[3] = nan;
    const MscnAggd a = mscn_aggd(m, n);
    if (!(a.alpha == a.alpha)) return;
    const double alpha = a.alpha, ls = a.ls, rs = a.rs;
    const double G1 = std::tgamma(1.0 / alpha), G2 = std::tgamma(2.0 / alpha), G3 = std::tgamma(3.0 / alpha);
    o[0] = alpha;
    o[1] = (rs - ls) * (G2 / G1) * (std::sqrt(G1) / std::sqrt(G3));
    o[2] = ls * ls;
    o[3] = rs * rs;
}

}  // namespace

int bq_plan(const char *scope, int h, int w, int cn, int crop_border, BqPlan *p)
{
    long long ch, cw;
    const int rc = mscn_crop(scope, h, w, cn, crop_border, BQ_MIN, &ch, &cw);
    if (rc) return rc;
    memset(p, 0, sizeof(*p));
    p->H = (int)ch;
    p->W = (int)cw;
    p->H2 = (int)((ch + 1) / 2);
    p->W2 = (int)((cw + 1) / 2);
    const auto tiles = [](long long n) { return (n + BQ_TILE - 1) / BQ_TILE; };
    p->nt[0] = tiles(p->H) * tiles(p->W);
    p->nt[1] = tiles(p->H2) * tiles(p->W2);
    size_t off = up256((size_t)p->H2 * (size_t)p->W2 * sizeof(int32_t));
    for (int s = 0; s < 2; ++s) {
        p->off_part[s] = off;
        off += up256((size_t)p->nt[s] * BQ_Q * sizeof(double));
    }
    const size_t buf = up256(((size_t)p->nt[0] / 1024 + 2) * BQ_Q * sizeof(double));   // reduce_partials' ping-pong buffers
    p->off_buf0 = off;
    p->off_buf1 = off + buf;
    p->total = off + 2 * buf;
    return SR_OK;
}

extern "C" {

int sr_brisque_plan(int h, int w, int cn, int crop_border, int *H, int *W, int *H2, int *W2, size_t *scratch_bytes)
{
    BqPlan p;
    const int rc = bq_plan("sr_brisque_plan", h, w, cn, crop_border, &p);
    if (rc) return rc;
    if (H) *H = p.H;
    if (W) *W = p.W;
    if (H2) *H2 = p.H2;
    if (W2) *W2 = p.W2;
    if (scratch_bytes) *scratch_bytes = p.total;
    return SR_OK;
}

int sr_brisque_features(const sr_brisque_record *records, double *feat36)
{
    if (!records || !feat36) return sr_set_error(SR_ERR_INVALID_ARG, "sr_brisque_features: null argument");
    for (int s = 0; s < 2; ++s)
        if (records[s].n < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_brisque_features: scale %d has no elements", s + 1);
    for (int s = 0; s < 2; ++s) {
        const double n = (double)records[s].n;
        double *f = feat36 + s * (F / 2);
        ggd_fit(records[s].x[0], n, f);
        for (int i = 1; i < 5; ++i) aggd_fit(records[s].x[i], n, f + 2 + 4 * (i - 1));
    }
    return SR_OK;
}

double sr_brisque_score(const double *feat36, const double *sv, const double *coef, int64_t n_sv, double gamma, double rho,
                        const double *fmin, const double *fmax, double lower, double upper)
{
    const double nan = std::nan("");
    if (!feat36 || !sv || !coef || !fmin || !fmax) return sr_set_error(SR_ERR_INVALID_ARG, "sr_brisque_score: null argument"), nan;
    if (n_sv < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_brisque_score: need at least one support vector (got %lld)", (long long)n_sv), nan;
    if (!(std::isfinite(gamma) && gamma > 0.0)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_brisque_score: gamma must be finite and positive"), nan;
    double x[F];
    for (int k = 0; k < F; ++k) {
        if (!(feat36[k] == feat36[k])) return nan;
        x[k] = fmax[k] == fmin[k] ? 0.0 : lower + (upper - lower) * (feat36[k] - fmin[k]) / (fmax[k] - fmin[k]);
    }
    double score = 0.0;
    for (int64_t i = 0; i < n_sv; ++i) {
        const double *v = sv + i * F;
        double d2 = 0.0;
        for (int k = 0; k < F; ++k) d2 += (v[k] - x[k]) * (v[k] - x[k]);
        score += coef[i] * std::exp(-gamma * d2);
    }
    return score - rho;
}

}  // extern "C"
