// sr_dists_host.cpp -- the host side of DISTS: the six feature-map sizes and the score from the per-channel sums.  Pure host
// code: no device call, no context -- sr_dists.hip produces the sums; tools/sanitize/dists_driver.cpp runs this file under
// the sanitizers.  The definition is in include/sr_hip.h.  All arithmetic is float64.
#include <cmath>

#include "sr_internal.h"

namespace {

constexpr int DS_STAGES = 6;
constexpr int DS_CH[DS_STAGES] = {3, 64, 128, 256, 512, 512};
constexpr int DS_TOTAL = 1475;

}  // namespace

extern "C" {

int sr_dists_layer_sizes(int h, int w, int *h_hw)
{
    if (!h_hw || h < 1 || w < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_layer_sizes: null output or a side below 1");
    h_hw[0] = h;
    h_hw[1] = w;
    for (int k = 1; k < DS_STAGES; ++k) {
        if (k >= 2) {                      // the L2 pooling in front of stages 2 .. 5: k 3, s 2, p 1 -> ceil(n / 2)
            h = (h - 1) / 2 + 1;
            w = (w - 1) / 2 + 1;
        }
        h_hw[2 * k] = h;
        h_hw[2 * k + 1] = w;
    }
    return SR_OK;
}

int sr_dists_score(const double *sums, const int *hw, const float *alpha, const float *beta, double *score, double *s1, double *s2)
{
    if (!sums || !hw || !alpha || !beta || !score) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_score: null argument");
    for (int k = 0; k < DS_STAGES; ++k)
        if (hw[2 * k] < 1 || hw[2 * k + 1] < 1) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_score: stage %d has no pixels", k);
    double wsum = 0.0;
    for (int i = 0; i < DS_TOTAL; ++i) wsum += (double)alpha[i];
    for (int i = 0; i < DS_TOTAL; ++i) wsum += (double)beta[i];
    if (!std::isfinite(wsum) || !(wsum > 0.0)) return sr_set_error(SR_ERR_INVALID_ARG, "sr_dists_score: alpha and beta must be finite with a positive total");
    const double c1 = 1e-6, c2 = 1e-6;
    double acc = 0.0;
    int ch = 0;
    for (int k = 0; k < DS_STAGES; ++k) {
        const double n = (double)hw[2 * k] * (double)hw[2 * k + 1];
        // stage 0 holds integer sums of the u8 values: x = u8 / 255
        const double d1 = k == 0 ? 255.0 : 1.0, d2 = k == 0 ? 255.0 * 255.0 : 1.0;
        for (int c = 0; c < DS_CH[k]; ++c, ++ch) {
            const double *s = sums + (size_t)ch * 5;
            const double ma = s[0] / d1 / n, mb = s[1] / d1 / n;
            const double va = s[2] / d2 / n - ma * ma, vb = s[3] / d2 / n - mb * mb, cab = s[4] / d2 / n - ma * mb;
            const double t1 = (2.0 * ma * mb + c1) / (ma * ma + mb * mb + c1);
            const double t2 = (2.0 * cab + c2) / (va + vb + c2);
            if (s1) s1[ch] = t1;
            if (s2) s2[ch] = t2;
            acc += (double)alpha[ch] / wsum * t1 + (double)beta[ch] / wsum * t2;
        }
    }
    *score = 1.0 - acc;
    return SR_OK;
}

}  // extern "C"
