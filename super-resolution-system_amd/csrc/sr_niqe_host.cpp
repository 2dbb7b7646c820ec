// sr_niqe_host.cpp -- the host side of NIQE: the plan, the AGGD features of the block records, the pristine-model fit and the
// score (a small cyclic Jacobi eigen-solver for the symmetric 36 x 36 matrix).  Pure host code: no device call, no context --
// sr_niqe.hip plans with nq_plan and takes its window from nq_window; tools/sanitize/niqe_driver.cpp runs this file under the
// sanitizers.  The definition is in include/sr_hip.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sr_mscn.h"

namespace {

constexpr int F = NQ_FEAT;
constexpr int MIN_FIT_ROWS = F + 1;         // a sample covariance of 36 features has full rank from 37 rows on

struct Aggd {
    double alpha, beta_l, beta_r;
};

// sr_mscn.h's fit (shared with BRISQUE) with NIQE's scales: beta = the side's root mean square * sqrt(G1 / G3)
Aggd aggd_fit(const sr_niqe_moments &m, double n)
{
    const MscnAggd a = mscn_aggd(m, n);
    if (!(a.alpha == a.alpha)) return {a.alpha, a.ls, a.rs};            // all NaN
    const double s = std::sqrt(std::tgamma(1.0 / a.alpha) / std::tgamma(3.0 / a.alpha));
    return {a.alpha, a.ls * s, a.rs * s};
}

void scale_features(const sr_niqe_block &rec, double n, double *f)
{
    const Aggd a0 = aggd_fit(rec.x[0], n);
    f[0] = a0.alpha;
    f[1] = (a0.beta_l + a0.beta_r) / 2.0;
    for (int s = 1; s < 5; ++s) {
        const Aggd a = aggd_fit(rec.x[s], n);
        double *o = f + 2 + 4 * (s - 1);
        o[0] = a.alpha;
        o[1] = (a.beta_r - a.beta_l) * (std::tgamma(2.0 / a.alpha) / std::tgamma(1.0 / a.alpha));
        o[2] = a.beta_l;
        o[3] = a.beta_r;
    }
}

bool row_has_nan(const double *row)
{
    for (int f = 0; f < F; ++f)
        if (!(row[f] == row[f])) return true;
    return false;
}

// mean[F] and the sample covariance (ddof 1) cov[F][F] of the listed rows (at least 2)
void mean_cov(const double *feat, const std::vector<int64_t> &rows, double *mean, double *cov)
{
    const double n = (double)rows.size();
    for (int f = 0; f < F; ++f) {
        double s = 0.0;
        for (int64_t r : rows) s += feat[r * F + f];
        mean[f] = s / n;
    }
    std::vector<double> acc((size_t)F * F, 0.0), d(F);
    for (int64_t r : rows) {
        for (int f = 0; f < F; ++f) d[f] = feat[r * F + f] - mean[f];
        for (int a = 0; a < F; ++a)
            for (int b = a; b < F; ++b) acc[(size_t)a * F + b] += d[a] * d[b];
    }
    for (int a = 0; a < F; ++a)
        for (int b = a; b < F; ++b) cov[a * F + b] = cov[b * F + a] = acc[(size_t)a * F + b] / (n - 1.0);
}

// Cyclic Jacobi on the symmetric A (n x n, destroyed): eigenvalues on its diagonal, eigenvectors in the columns of V.
void jacobi_eig(double *A, double *V, int n)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[i * n + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < n; ++i) {
            diag += A[i * n + i] * A[i * n + i];
            for (int j = i + 1; j < n; ++j) off += A[i * n + j] * A[i * n + j];
        }
        if (off == 0.0 || off <= 1e-60 * diag) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {                                   // columns p, q
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq;
                    A[k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {                                   // rows p, q
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - s * aqk;
                    A[q * n + k] = s * apk + c * aqk;
                }
                A[p * n + q] = A[q * n + p] = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
            }
    }
}

}  // namespace

int nq_plan(const char *scope, int h, int w, int cn, int crop_border, NqPlan *p)
{
    long long ch, cw;
    const int rc = mscn_crop(scope, h, w, cn, crop_border, NQ_BLOCK, &ch, &cw);
    if (rc) return rc;
    memset(p, 0, sizeof(*p));
    p->nby = (int)(ch / NQ_BLOCK);
    p->nbx = (int)(cw / NQ_BLOCK);
    p->H = p->nby * NQ_BLOCK;
    p->W = p->nbx * NQ_BLOCK;
    p->off_half = 0;
    p->off_rec = up256((size_t)(p->H / 2) * (size_t)(p->W / 2) * sizeof(int32_t));
    p->total = p->off_rec + up256(2 * (size_t)p->nby * (size_t)p->nbx * sizeof(sr_niqe_block));
    return SR_OK;
}

void nq_window(double k[2 * NQ_R + 1])
{
    const double sigma = 7.0 / 6.0;
    double sum = 0.0;
    for (int i = -NQ_R; i <= NQ_R; ++i) sum += k[i + NQ_R] = std::exp(-(double)(i * i) / (2.0 * sigma * sigma));
    for (int i = 0; i < 2 * NQ_R + 1; ++i) k[i] /= sum;
}

extern "C" {

int sr_niqe_plan(int h, int w, int cn, int crop_border, int *H, int *W, int *nby, int *nbx, size_t *scratch_bytes)
{
    NqPlan p;
    const int rc = nq_plan("sr_niqe_plan", h, w, cn, crop_border, &p);
    if (rc) return rc;
    if (H) *H = p.H;
    if (W) *W = p.W;
    if (nby) *nby = p.nby;
    if (nbx) *nbx = p.nbx;
    if (scratch_bytes) *scratch_bytes = p.total;
    return SR_OK;
}

int sr_niqe_features(const sr_niqe_block *records, int64_t nblocks, double *feat36)
{
    if (!records || !feat36) return sr_set_error(SR_ERR_INVALID_ARG, "sr_niqe_features: null argument");
    if (nblocks < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_niqe_features: need at least one block (got %lld)", (long long)nblocks);
    for (int64_t b = 0; b < nblocks; ++b)
        for (int s = 0; s < 2; ++s) {
            const double side = NQ_BLOCK >> s;
            scale_features(records[s * nblocks + b], side * side, feat36 + b * F + s * (F / 2));
        }
    return SR_OK;
}

int sr_niqe_fit(const double *feat, const double *sharp, const int64_t *image_off, int n_images, double T, double *mu, double *cov,
                int64_t *rows_used)
{
    if (!feat || !sharp || !image_off || !mu || !cov) return sr_set_error(SR_ERR_INVALID_ARG, "sr_niqe_fit: null argument");
    if (n_images < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_niqe_fit: need at least one image (got %d)", n_images);
    if (!(T >= 0.0 && T < 1.0)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_niqe_fit: the threshold must be in [0, 1)");
    if (image_off[0] != 0) return sr_set_error(SR_ERR_INVALID_ARG, "sr_niqe_fit: image offsets must start at 0");
    for (int i = 0; i < n_images; ++i)
        if (image_off[i + 1] < image_off[i])
            return sr_set_error(SR_ERR_INVALID_ARG, "sr_niqe_fit: image offsets must ascend (image %d)", i);
    std::vector<int64_t> rows;
    for (int i = 0; i < n_images; ++i) {
        double top = 0.0;
        for (int64_t r = image_off[i]; r < image_off[i + 1]; ++r) top = std::max(top, sharp[r]);
        for (int64_t r = image_off[i]; r < image_off[i + 1]; ++r)
            if (sharp[r] > T * top && !row_has_nan(feat + r * F)) rows.push_back(r);
    }
    if (rows_used) *rows_used = (int64_t)rows.size();
    if ((int64_t)rows.size() < MIN_FIT_ROWS)
        return sr_set_error(SR_ERR_SHAPE, "sr_niqe_fit: %lld blocks pass the sharpness threshold without a NaN; a 36 x 36 covariance "
                            "needs at least %d", (long long)rows.size(), MIN_FIT_ROWS);
    mean_cov(feat, rows, mu, cov);
    return SR_OK;
}

double sr_niqe_score(const double *feat, int64_t nblocks, const double *mu_pris, const double *cov_pris)
{
    const double nan = std::nan("");
    if (!feat || !mu_pris || !cov_pris) return sr_set_error(SR_ERR_INVALID_ARG, "sr_niqe_score: null argument"), nan;
    std::vector<int64_t> rows;
    for (int64_t r = 0; r < nblocks; ++r)
        if (!row_has_nan(feat + r * F)) rows.push_back(r);
    if (rows.size() < 2)
        return sr_set_error(SR_ERR_SHAPE, "sr_niqe_score: %lld of %lld blocks are free of NaN; the covariance needs at least 2",
                            (long long)rows.size(), (long long)std::max<int64_t>(nblocks, 0)), nan;
    double mu_d[F], unused[F], d[F];
    std::vector<double> S((size_t)F * F), V((size_t)F * F);
    mean_cov(feat, rows, unused, S.data());
    for (int f = 0; f < F; ++f) {                       // the mean is over every non-NaN entry, not only the NaN-free rows
        double s = 0.0;
        int64_t n = 0;
        for (int64_t r = 0; r < nblocks; ++r) {
            const double v = feat[r * F + f];
            if (v == v) {
                s += v;
                ++n;
            }
        }
        mu_d[f] = s / (double)n;
        d[f] = mu_pris[f] - mu_d[f];
    }
    for (int a = 0; a < F; ++a)
        for (int b = a; b < F; ++b) {                   // symmetrised: the solver reads both triangles
            const double v = ((cov_pris[a * F + b] + cov_pris[b * F + a]) / 2.0 + S[(size_t)a * F + b]) / 2.0;
            S[(size_t)a * F + b] = S[(size_t)b * F + a] = v;
        }
    jacobi_eig(S.data(), V.data(), F);
    double top = 0.0;
    for (int k = 0; k < F; ++k) top = std::max(top, std::fabs(S[(size_t)k * F + k]));
    double q = 0.0;
    for (int k = 0; k < F; ++k) {
        const double lam = S[(size_t)k * F + k];
        if (!(std::fabs(lam) > 1e-15 * top)) continue;
        double proj = 0.0;
        for (int f = 0; f < F; ++f) proj += V[(size_t)f * F + k] * d[f];
        q += proj * proj / lam;
    }
    return std::sqrt(q);
}

}  // extern "C"
