"""NumPy / SciPy restatement of the gradient magnitude similarity deviation (the authors' GMSD.m), written from the
definition in include/sr_hip.h: MATLAB's q = (2 m1 m2 + 170) / (m1^2 + m2^2 + 170) and std2(q) = np.std(q, ddof=1), computed in
two passes.  `mutant` switches one line of the definition to a plausible wrong one; tests/test_gmsd_host.py checks that each
moves the answer."""
import numpy as np
from scipy.signal import convolve2d

from _vif_ref import CHANNELS, Y, Y_ROUND, crop, plane  # noqa: F401  (the planes are VIF's)

MIN_SIDE = 4
C = 170.0
MUTANTS = ("n_divisor", "replicate")


def conv_same(x, k, replicate=False):
    """MATLAB's conv2(x, k, 'same'): the central part of the full convolution, from row ceil((kh + 1) / 2) (1-based) on --
    for the 2 x 2 kernel that is the mean of x(i .. i + 1, j .. j + 1) with zero beyond the last row and column."""
    kh, kw = k.shape
    r0, c0 = (kh + 2) // 2 - 1, (kw + 2) // 2 - 1
    if replicate:     # the mutant: the border is the edge value instead of zero
        xp = np.pad(x, ((kh - 1 - r0, r0), (kw - 1 - c0, c0)), mode="edge")
        return convolve2d(xp, k, mode="valid")
    full = convolve2d(x, k, mode="full")
    return full[r0:r0 + x.shape[0], c0:c0 + x.shape[1]]


def gmsd(a, b, crop_border=0, mode=Y, mutant=None):
    """-> {'score', 'sum_d', 'sum_d2', 'count', 'q'}"""
    assert mutant is None or mutant in MUTANTS
    if a.shape != b.shape:
        raise ValueError("shapes differ")
    if crop_border < 0:
        raise ValueError("crop_border")
    x, y = plane(crop(a, crop_border), mode), plane(crop(b, crop_border), mode)
    if min(x.shape) < MIN_SIDE:
        raise ValueError(f"both sides must be at least {MIN_SIDE}")
    rep = mutant == "replicate"
    dx = np.array([[1.0, 0.0, -1.0]] * 3) / 3.0
    dy = dx.T
    ave = np.ones((2, 2)) / 4.0
    x, y = conv_same(x, ave, rep)[::2, ::2], conv_same(y, ave, rep)[::2, ::2]
    m1 = np.sqrt(conv_same(x, dx, rep) ** 2 + conv_same(x, dy, rep) ** 2)
    m2 = np.sqrt(conv_same(y, dx, rep) ** 2 + conv_same(y, dy, rep) ** 2)
    q = (2.0 * m1 * m2 + C) / (m1 * m1 + m2 * m2 + C)
    d = 1.0 - q
    return {"score": float(np.std(q, ddof=0 if mutant == "n_divisor" else 1)), "sum_d": float(d.sum()),
            "sum_d2": float((d * d).sum()), "count": int(q.size), "q": q}
