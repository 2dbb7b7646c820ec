"""Writes tests/golden/brisque_svr_sklearn.npz: an RBF epsilon-SVR fitted by libsvm itself (scikit-learn's SVR is libsvm), with
probe feature rows and libsvm's own predictions for them, so that sr_brisque_score's scaler and decision function are pinned
against the library the published BRISQUE models come from.  Run by hand (scikit-learn 1.7.2 wrote the committed file); no
test runs this script, tests read only the .npz.

The regressor is NOT a quality model: it is fitted on seeded 36-vectors in [-1, 1] to a smooth seeded target around 50.  The
feature ranges are seeded around what BRISQUE's features take on natural-image-like planes (alpha in 0.2 .. 4, variances in
0 .. 1.5, AGGD means in -0.5 .. 0.5), so features of test images land inside the box the regressor was fitted on."""
import os

import numpy as np
from sklearn.svm import SVR

HERE = os.path.dirname(os.path.abspath(__file__))
GAMMA = 0.05


def main():
    rng = np.random.default_rng(20121)
    x = rng.uniform(-1.0, 1.0, size=(160, 36))
    w = rng.standard_normal(36)
    y = 50.0 + 20.0 * np.sin(x @ w / 3.0) + 5.0 * x[:, 0] * x[:, 18]
    svr = SVR(kernel="rbf", gamma=GAMMA, C=100.0, epsilon=0.1).fit(x, y)
    sv, coef, rho = svr.support_vectors_, svr.dual_coef_.reshape(-1), -float(svr.intercept_[0])
    # the formula as the definition states it, against predict: the file is only written if libsvm agrees with it
    k = np.exp(-GAMMA * ((x[:, None, :] - sv[None, :, :]) ** 2).sum(-1))
    assert np.abs(k @ coef - rho - svr.predict(x)).max() < 1e-12 * 50
    # per scale: [alpha, s2] then four of [alpha, mean, ls^2, rs^2]
    lo18 = np.array([0.2, 0.0] + [0.2, -0.5, 0.0, 0.0] * 4)
    hi18 = np.array([4.0, 1.5] + [4.0, 0.5, 1.5, 1.5] * 4)
    jitter = rng.uniform(0.0, 0.05, size=(2, 36))
    fmin = np.tile(lo18, 2) - jitter[0]
    fmax = np.tile(hi18, 2) + jitter[1]
    # probes: scaled positions inside and a little outside the box (the scaler does not clamp), as unscaled feature rows
    px = rng.uniform(-1.2, 1.2, size=(12, 36))
    probes = fmin + (px + 1.0) / 2.0 * (fmax - fmin)
    scaled = -1.0 + 2.0 * (probes - fmin) / (fmax - fmin)
    answers = svr.predict(scaled)
    np.savez(os.path.join(HERE, "brisque_svr_sklearn.npz"), sv=sv, sv_coef=coef, gamma=np.float64(GAMMA), rho=np.float64(rho),
             feature_min=fmin, feature_max=fmax, lower=np.float64(-1.0), upper=np.float64(1.0), probe_features=probes,
             probe_scores=answers)
    print(sv.shape, float(answers.min()), float(answers.max()))


if __name__ == "__main__":
    main()
